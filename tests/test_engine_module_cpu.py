"""CPU: the host-side machinery the three front ends share (smtc_amd/engine_module.py) -- range merging, the layout -> nn.Parameter round trip
over flat buffers, the dropout seed sequence.  mmhip_create / mmhip_txt_create / mmhip_early_create only lay out memory: no GPU work here."""
import ctypes as C

import pytest
import torch
import torch.nn as nn

import smtc_amd  # noqa: F401
from smtc_amd import _lib, build
from smtc_amd.engine_module import EngineModule, merge_ranges, read_param_infos, register_flat_parameters

G = _lib


@pytest.fixture(scope="module")
def layouts():
    """one handle per family at the smallest legal shapes -> {family: (infos, {buffer: numel})}; the handles are destroyed again"""
    build.build(verbose=False)
    lib = _lib.lib()
    small = dict(hidden=128, heads=2, inter=128, vocab=50, max_pos=16, num_labels=3, p_hidden=0.1, p_attn=0.1, p_head=0.1, dtype=_lib.BF16, max_posts=2,
                 max_text_len=8)
    late = _lib.Config(layers_txt=1, layers_img=1, type_vocab=1, txt_kind=_lib.TXT_XLMR, pad_id=1, ln_eps_txt=1e-5, ln_eps_img=1e-12, image=32, patch=16,
                       proj_dim=8, fusion=_lib.FUSION_ATTENTION, loss_scale=0.0, **small)
    txt = _lib.TxtConfig(layers=1, type_vocab=1, txt_kind=_lib.TXT_XLMR, pad_id=1, ln_eps=1e-5, loss_scale=0.0, **small)
    early = _lib.EarlyConfig(l_layers=1, r_layers=1, x_layers=1, type_vocab=2, feat_dim=2048, pos_dim=4, max_boxes=4, ln_eps=1e-12, **small)
    out = {}
    for fam, cfg, pre, numel in (("late", late, "mmhip_", lambda h: {0: lib.mmhip_buffer_numel(h, 0), 1: lib.mmhip_buffer_numel(h, 1)}),
                                 ("txt", txt, "mmhip_txt_", lambda h: {1: lib.mmhip_txt_numel(h)}),
                                 ("early", early, "mmhip_early_", lambda h: {1: lib.mmhip_early_numel(h)})):
        h = C.c_void_p()
        assert getattr(lib, pre + "create")(C.byref(cfg), C.byref(h)) == 0, fam
        infos = read_param_infos(getattr(lib, pre + "param_count"), getattr(lib, pre + "param_info_at"), h)
        out[fam] = (infos, {b: int(n) for b, n in numel(h).items()})
        getattr(lib, pre + "destroy")(h)
    return out


def test_merge_ranges_on_hand_written_spans():
    assert merge_ranges([]) == []
    assert merge_ranges([(0, 8), (8, 4)]) == [(0, 12)]                        # adjacent
    assert merge_ranges([(0, 8), (12, 4)]) == [(0, 8), (12, 16)]              # a gap
    assert merge_ranges([(12, 4), (0, 8), (8, 4), (32, 8)]) == [(0, 16), (32, 40)]      # out of order
    assert merge_ranges([(0, 5), (8, 3), (12, 1)]) == [(0, 16)]               # numel padded to a multiple of 4: 5 -> 8, 3 -> 4, 1 -> 4
    assert merge_ranges([(0, 5), (12, 2)]) == [(0, 8), (12, 16)]
    assert merge_ranges(iter([(4, 4)])) == [(4, 8)]


def _ranges_as_before(infos, keep):
    """the loop mm_late.active_ranges, text_only.active_ranges and mm_early.grad_ranges each carried before they shared merge_ranges"""
    spans = sorted((i["offset"], i["offset"] + ((i["numel"] + 3) & ~3)) for i in infos if keep(i))
    out = []
    for b, e in spans:
        if out and out[-1][1] == b:
            out[-1][1] = e
        else:
            out.append([b, e])
    return [tuple(x) for x in out]


def test_merge_ranges_equals_the_front_ends_former_loops_on_real_layouts(layouts):
    subsets = [{G.G_ALWAYS}, {G.G_ALWAYS, G.G_ITC}, {G.G_ALWAYS, G.G_ITM}, {G.G_ALWAYS, G.G_FUSION_ATT}, {G.G_ALWAYS, G.G_ITC, G.G_ITM},
               {G.G_ALWAYS, G.G_FUSION_ATT, G.G_ITC, G.G_ITM}]
    cases = [("late", lambda i, g=g: i["buffer"] == 1 and i["group"] in g) for g in subsets]
    cases += [("early", lambda i, g=g: i["group"] in g) for g in subsets if G.G_FUSION_ATT not in g]
    cases += [("txt", lambda i: i["group"] != G.G_NEVER)]                    # the text-only "everything but never"
    for fam, keep in cases:
        infos = layouts[fam][0]
        want = _ranges_as_before(infos, keep)
        got = merge_ranges((i["offset"], i["numel"]) for i in infos if keep(i))
        assert got == want and want and all(isinstance(r, tuple) for r in got), fam
        assert all(b < e for b, e in got) and all(got[k][1] < got[k + 1][0] for k in range(len(got) - 1))
    # the subsets differ on these layouts (the comparison above is not vacuous)
    late = layouts["late"][0]
    assert len({tuple(merge_ranges((i["offset"], i["numel"]) for i in late if i["buffer"] == 1 and i["group"] in g)) for g in subsets}) == len(subsets)
    assert any(i["numel"] % 4 for i in late)


def _keys_as_before(infos):
    """named_parameters() order of the registration loop each front end carried before register_flat_parameters"""
    class Node(nn.Module):
        pass
    root = Node()
    for inf in infos:
        node, parts = root, inf["name"].split(".")
        for part in parts[:-1]:
            if part not in node._modules:
                node.add_module(part, Node())
            node = node._modules[part]
        node.register_parameter(parts[-1], nn.Parameter(torch.zeros(())))
    return [k for k, _ in root.named_parameters()]


@pytest.mark.parametrize("fam", ["late", "txt", "early"])
def test_layout_round_trip_through_flat_buffers(layouts, fam):
    infos, numel = layouts[fam]
    infos = [dict(i) for i in infos]
    flats = {b: torch.zeros(n) for b, n in numel.items()}
    mod = nn.Module()
    register_flat_parameters(mod, infos, flats)
    named = dict(mod.named_parameters())
    # the layout's names, each once.  (nn.Module lists a module's own parameters before its children's, so the ORDER of named_parameters() /
    # state_dict() is the tree walk's, not the layout's: it is pinned to what the front ends' former registration loop gives.)
    assert len(named) == len(infos) and sorted(named) == sorted(i["name"] for i in infos)
    assert list(named) == list(mod.state_dict()) == _keys_as_before(infos)
    assert {i["buffer"] for i in infos} == set(numel)
    for inf in infos:
        k, p, flat = inf["name"], named[inf["name"]], flats[inf["buffer"]]
        assert p is inf["param"] and tuple(p.shape) == inf["shape"] and p.numel() == inf["numel"], k
        assert p.data_ptr() == flat.data_ptr() + 4 * inf["offset"], k
        assert p.requires_grad == (inf["buffer"] != 0), k                       # frozen <=> buffer 0
        assert inf["offset"] + inf["numel"] <= flat.numel()
    for k in (0, len(infos) // 2, len(infos) - 1):                               # a write through the flat buffer is visible through the parameter
        inf = infos[k]
        flats[inf["buffer"]][inf["offset"]: inf["offset"] + inf["numel"]] = torch.arange(1, inf["numel"] + 1, dtype=torch.float32)
        assert torch.equal(inf["param"].detach().reshape(-1), torch.arange(1, inf["numel"] + 1, dtype=torch.float32)), inf["name"]
    if fam == "late":
        assert any(i["buffer"] == 0 for i in infos) and all(("vision" in i["name"]) == (i["buffer"] == 0) for i in infos)


@pytest.mark.parametrize("base", [0, 30])
def test_seed_sequence(base):
    m = EngineModule()
    m._init_engine(base)
    got = [m._next_seed() for _ in range(3)]
    assert got == [(base * 0x9E3779B97F4A7C15 + k) & (2 ** 64 - 1) for k in (1, 2, 3)]
    assert m._calls == 3 and m._seed_base == base
