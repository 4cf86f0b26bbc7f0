"""CPU: the aspect-att fusion's host side -- the C ABI's layout of a MMHIP_FUSION_ASPECT handle (mmhip_create only lays out memory: no GPU work),
the refusals that are decided before the GPU is touched, the command line."""
import ctypes as C
import types

import pytest

import smtc_amd  # noqa: F401
from smtc_amd import _lib, build
from smtc_amd.engine_module import merge_ranges, read_param_infos
from oracle import mm_oracle as O

G = _lib
H, LAYERS = 128, 2


def config(fusion, **kw):
    base = dict(hidden=H, heads=2, inter=128, layers_txt=LAYERS, layers_img=1, vocab=50, max_pos=16, type_vocab=1, txt_kind=_lib.TXT_XLMR, pad_id=1,
                ln_eps_txt=1e-5, ln_eps_img=1e-12, image=32, patch=16, proj_dim=8, num_labels=3, fusion=fusion, p_hidden=0.1, p_attn=0.1, p_head=0.1,
                dtype=_lib.BF16, max_posts=2, max_text_len=8, loss_scale=0.0)
    base.update(kw)
    return _lib.Config(**base)


def layout(lib, cfg):
    """-> (infos, stage ranges, {buffer: numel}) of a handle that is destroyed again"""
    h = C.c_void_p()
    assert lib.mmhip_create(C.byref(cfg), C.byref(h)) == 0
    infos = read_param_infos(lib.mmhip_param_count, lib.mmhip_param_info_at, h)
    stages = []
    for st in range(lib.mmhip_num_backward_stages(h)):
        b, e = C.c_uint64(), C.c_uint64()
        assert lib.mmhip_stage_grad_range(h, st, C.byref(b), C.byref(e)) == 0
        stages.append((b.value, e.value))
    numel = {0: int(lib.mmhip_buffer_numel(h, 0)), 1: int(lib.mmhip_buffer_numel(h, 1))}
    lib.mmhip_destroy(h)
    return infos, stages, numel


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def test_enum_value():
    assert (_lib.FUSION_CONCAT, _lib.FUSION_ATTENTION, _lib.FUSION_ASPECT) == (0, 1, 2)


def test_create_accepts_the_fusion_and_refuses_unequal_towers(lib):
    h = C.c_void_p()
    assert lib.mmhip_create(C.byref(config(_lib.FUSION_ASPECT)), C.byref(h)) == 0
    lib.mmhip_destroy(h)
    assert lib.mmhip_create(C.byref(config(_lib.FUSION_ASPECT, hidden_img=H)), C.byref(h)) == 0          # stated width equal to the text tower's
    lib.mmhip_destroy(h)
    clip = dict(img_kind=_lib.IMG_CLIP, hidden_img=256, heads_img=4, inter_img=256)
    assert lib.mmhip_create(C.byref(config(_lib.FUSION_ASPECT, **clip)), C.byref(h)) == -1
    assert lib.mmhip_create(C.byref(config(_lib.FUSION_ATTENTION, **clip)), C.byref(h)) == -1            # as for attention
    assert lib.mmhip_create(C.byref(config(_lib.FUSION_CONCAT, **clip)), C.byref(h)) == 0
    lib.mmhip_destroy(h)


def test_aspect_layout(lib):
    infos, stages, numel = layout(lib, config(_lib.FUSION_ASPECT))
    by = {i["name"]: i for i in infos}
    # names and shapes are the reference's state dict
    want = O.param_shapes(O.OracleConfig(hidden=H, heads=2, inter=128, layers_txt=LAYERS, layers_img=1, vocab=50, max_pos=16, num_labels=3, image=32,
                                         patch=16, proj_dim=8, fusion="aspect-att"))
    assert len(by) == len(infos) and set(by) == set(want)
    for k, shp in want.items():
        assert tuple(by[k]["shape"]) == tuple(shp), k
    # groups
    for k, i in by.items():
        if "vision_model" in k:
            assert i["group"] == G.G_FROZEN and i["buffer"] == 0, k
            continue
        assert i["buffer"] == 1, k
        top = k.split(".")[0]
        if top == "aspectattention" or k.startswith("dual_encoder.text_model.pooler.dense."):
            assert i["group"] == G.G_ALWAYS, k                   # trained with or without ITC
        elif top in ("linear_fusion", "fc_Q", "fc_K", "fc_V", "linear_gmu_t", "linear_gmu_v", "linear_iadds"):
            assert i["group"] == G.G_NEVER, k                    # mm_late.py:115-131 reads none of them
        elif top == "linear_tim":
            assert i["group"] == G.G_ITM, k                      # no ITM pass exists: never active in practice
        elif k in ("dual_encoder.logit_scale", "dual_encoder.visual_projection.weight", "dual_encoder.text_projection.weight"):
            assert i["group"] == G.G_ITC, k
        else:
            assert i["group"] == G.G_ALWAYS, k
    # spans do not overlap inside a buffer and stay inside it
    for buf in (0, 1):
        spans = sorted((i["offset"], i["offset"] + i["numel"]) for i in infos if i["buffer"] == buf)
        assert all(spans[k][1] <= spans[k + 1][0] for k in range(len(spans) - 1)) and spans[-1][1] <= numel[buf]
    # every parameter that can be active sits in exactly one backward stage's range (the data-parallel exchange walks these)
    assert len(stages) == LAYERS + 2 and all(b < e for b, e in stages)
    assert all(stages[k][1] <= stages[k + 1][0] for k in range(len(stages) - 1))
    for i in infos:
        if i["buffer"] == 1 and i["group"] in (G.G_ALWAYS, G.G_ITC):
            inside = [st for st, (b, e) in enumerate(stages) if b <= i["offset"] and i["offset"] + i["numel"] <= e]
            assert len(inside) == 1, i["name"]
            if i["name"].split(".")[0] in ("aspectattention", "linear_cls") or ".pooler." in i["name"]:
                assert inside == [0], i["name"]
    # the never group lies in front of the heads' range: AdamW's active ranges without ITC are the pooler .. and aspectattention .. on
    never_end = max(i["offset"] + i["numel"] for i in infos if i["buffer"] == 1 and i["group"] == G.G_NEVER)
    assert never_end <= stages[0][0]
    active = merge_ranges((i["offset"], i["numel"]) for i in infos if i["buffer"] == 1 and i["group"] == G.G_ALWAYS)
    assert all(b >= stages[0][0] for b, _ in active)


def test_other_fusions_keep_their_layout(lib):
    """the (name, offset, group) list of an attention / concat handle is the same before and after an aspect handle existed, the two agree with each
    other, and they keep the order the aspect handle changes"""
    key = lambda infos: [(i["name"], i["buffer"], i["offset"], i["group"], tuple(i["shape"])) for i in infos]
    before = {f: key(layout(lib, config(f))[0]) for f in (_lib.FUSION_ATTENTION, _lib.FUSION_CONCAT)}
    aspect = key(layout(lib, config(_lib.FUSION_ASPECT))[0])
    after = {f: key(layout(lib, config(f))[0]) for f in (_lib.FUSION_ATTENTION, _lib.FUSION_CONCAT)}
    assert before == after and before[_lib.FUSION_ATTENTION] == before[_lib.FUSION_CONCAT]
    att = {n: (off, g) for n, _, off, g, _ in before[_lib.FUSION_ATTENTION]}
    train = [n for n, buf, _, _, _ in before[_lib.FUSION_ATTENTION] if buf == 1]
    assert train[:2] == ["aspectattention.weight", "aspectattention.bias"] and att["aspectattention.weight"] == (0, G.G_NEVER)
    assert att["dual_encoder.text_model.pooler.dense.weight"][1] == G.G_ITC and att["linear_fusion.weight"][1] == G.G_ALWAYS
    assert att["fc_Q.weight"][1] == G.G_FUSION_ATT
    assert aspect != before[_lib.FUSION_ATTENTION] and sorted(x[0] for x in aspect) == sorted(x[0] for x in before[_lib.FUSION_ATTENTION])


def test_itm_with_aspect_att_is_refused_before_the_gpu_is_touched():
    """MMLate_Model checks the flag pair next to the multilabel check, before MM_Model (and so a GPU) is asked for"""
    from smtc_amd.mm_late import MMLate_Model, ASPECT_ITM_MESSAGE
    cfg = types.SimpleNamespace(use_tim_loss=True, use_clip_loss=False)
    with pytest.raises(NotImplementedError, match=r"mm_late\.py:181"):
        MMLate_Model(cfg, "bernice", "vit", "aspect-att")
    assert "mm_late.py:181" in ASPECT_ITM_MESSAGE


def test_command_line_takes_the_fusion_and_refuses_itm_with_it(monkeypatch, tmp_path):
    """the parser round-trips the name, the file names follow the pattern, and --use_tim_loss with it is refused through the entry point itself,
    before a model (and a GPU) is asked for"""
    from smtc_amd import run_mm_late
    from smtc_amd.run_mm_late import build_parser, file_names
    monkeypatch.delenv("RANK", raising=False)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(NotImplementedError, match=r"mm_late\.py:181"):
        run_mm_late.main(["--txt_model_name", "bernice", "--img_model_name", "vit", "--fusion_name", "aspect-att", "--task", "2", "--synthetic",
                          "--use_tim_loss", "--results_dir", str(tmp_path) + "/"])
    assert not any(tmp_path.iterdir())
    args = build_parser().parse_args(["--txt_model_name", "bernice", "--img_model_name", "vit", "--fusion_name", "aspect-att", "--task", "2",
                                      "--use_clip_loss"])
    assert args.fusion_name == "aspect-att" and args.use_clip_loss and not args.use_tim_loss
    names = file_names(args, "/r/", "itc")
    assert names["val"] == "/r/bernice-vit-aspect-att_task2_seed30_itc_metrics_val.csv"
