"""CPU: the BEiT image tower's host side -- the C ABI's layout of a MMHIP_IMG_BEIT handle (mmhip_create only lays out memory: no GPU work) against
the reference fixture's vision state dict, the key maps, the setter, the refusals that are decided before the GPU is touched, and the operator
bounds of tests/beit_ref.py (a missing, transposed or wrong-head bias leaves them by far)."""
import ast
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import smtc_amd  # noqa: F401
from smtc_amd import _lib, build
from smtc_amd.engine_module import read_param_infos
from oracle import mm_oracle as O
import beit_ref as R
import op_bounds as OB

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def config(fusion=_lib.FUSION_ATTENTION, **kw):
    base = dict(hidden=128, heads=2, inter=256, layers_txt=2, layers_img=2, vocab=1000, max_pos=130, type_vocab=1, txt_kind=_lib.TXT_XLMR, pad_id=1,
                ln_eps_txt=1e-5, ln_eps_img=1e-12, image=64, patch=16, proj_dim=512, num_labels=3, fusion=fusion, p_hidden=0.1, p_attn=0.1, p_head=0.05,
                dtype=_lib.BF16, max_posts=4, max_text_len=32, loss_scale=0.0, img_kind=_lib.IMG_BEIT)
    base.update(kw)
    return _lib.Config(**base)


@pytest.fixture(scope="module")
def lib():
    build.build(verbose=False)
    return _lib.lib()


def create(lib, cfg):
    h = C.c_void_p()
    rc = lib.mmhip_create(C.byref(cfg), C.byref(h))
    return rc, h


def layout(lib, cfg):
    rc, h = create(lib, cfg)
    assert rc == 0
    infos = read_param_infos(lib.mmhip_param_count, lib.mmhip_param_info_at, h)
    numel = {0: int(lib.mmhip_buffer_numel(h, 0)), 1: int(lib.mmhip_buffer_numel(h, 1))}
    ws = int(lib.mmhip_workspace_bytes(h))
    lib.mmhip_destroy(h)
    return infos, numel, ws


def test_enum_value_and_exports():
    assert (_lib.IMG_VIT, _lib.IMG_CLIP, _lib.IMG_BEIT) == (0, 1, 2)
    for name in ("mmhip_set_drop_path", "mmhip_op_attn_fwd_bias", "mmhip_op_beit_bias_image", "mmhip_op_patch_mean_ln"):
        assert name in _lib.EXPORTS


@pytest.mark.parametrize("fusion", ["attention", "concat", "aspect-att"])
def test_layout_is_the_reference_state_dict(lib, fusion):
    """names and shapes of a BEiT handle = the parameters the restatement loads into the reference's own model (tests/golden/make_beit_golden.py
    asserts that set against HF's state dict, key for key, in 4.25.1 naming through _beit_ref_to_key)"""
    z = np.load(os.path.join(GOLD, "beit_small_xlmr.npz"), allow_pickle=False)
    ocfg = O.OracleConfig(**ast.literal_eval(str(z[f"{fusion}.cfg"])))
    code = {"attention": _lib.FUSION_ATTENTION, "concat": _lib.FUSION_CONCAT, "aspect-att": _lib.FUSION_ASPECT}[fusion]
    infos, numel, _ = layout(lib, config(code))
    by = {i["name"]: i for i in infos}
    want = R.param_shapes(ocfg)
    assert len(by) == len(infos) and set(by) == set(want), set(by) ^ set(want)
    for k, shp in want.items():
        assert tuple(by[k]["shape"]) == tuple(shp), k
    vision = [i for i in infos if "vision_model" in i["name"]]
    assert len(vision) == 3 + 18 * 2 + 2
    assert all(i["group"] == _lib.G_FROZEN and i["buffer"] == 0 for i in vision)
    assert all(i["buffer"] == 1 for i in infos if "vision_model" not in i["name"])
    names = {i["name"] for i in vision}
    assert not any("key.bias" in n or "position_embeddings" in n or n.endswith("vision_model.layernorm.weight") or "pooler.dense" in n for n in names)
    assert "dual_encoder.vision_model.pooler.layernorm.weight" in names
    assert by["dual_encoder.vision_model.encoder.layer.1." + R.TABLE]["shape"] == (52, 2)
    # buffers do not overlap and stay inside their flat buffer
    for buf in (0, 1):
        spans = sorted((i["offset"], i["offset"] + i["numel"]) for i in infos if i["buffer"] == buf)
        assert all(spans[k][1] <= spans[k + 1][0] for k in range(len(spans) - 1)) and spans[-1][1] <= numel[buf]
    # the packed QKV bias block: query.bias, an unnamed slot of `hidden` elements where HF has no key bias, value.bias -- contiguous
    for l in range(2):
        p = f"dual_encoder.vision_model.encoder.layer.{l}.attention.attention."
        q, v = by[p + "query.bias"], by[p + "value.bias"]
        assert v["offset"] == q["offset"] + 2 * 128
        assert not any(q["offset"] + 128 <= i["offset"] < v["offset"] for i in vision)
        w = [by[p + n + ".weight"]["offset"] for n in ("query", "key", "value")]
        assert w[1] == w[0] + 128 * 128 and w[2] == w[1] + 128 * 128


def test_other_image_kinds_keep_their_layout_and_workspace(lib):
    key = lambda r: ([(i["name"], i["buffer"], i["offset"], i["group"], tuple(i["shape"])) for i in r[0]], r[1], r[2])
    before = key(layout(lib, config(img_kind=_lib.IMG_VIT)))
    beit = key(layout(lib, config()))
    after = key(layout(lib, config(img_kind=_lib.IMG_VIT)))
    assert before == after
    assert beit[2] > before[2]          # the bias images, the folded biases and the drop-path scratch exist on BEiT handles only
    train = lambda r: [x for x in r[0] if x[1] == 1]
    assert train(beit) == train(before)          # the trainable side is the same layout


def test_create_refusals(lib, monkeypatch):
    assert create(lib, config(image=72))[0] == -1                                    # image % patch != 0
    wide = dict(hidden_img=256, heads_img=4, inter_img=256)
    assert create(lib, config(_lib.FUSION_ATTENTION, **wide))[0] == -1               # unequal widths under attention ...
    assert create(lib, config(_lib.FUSION_ASPECT, **wide))[0] == -1                  # ... and aspect-att: the existing rules
    rc, h = create(lib, config(_lib.FUSION_CONCAT, **wide))
    assert rc == 0
    lib.mmhip_destroy(h)
    assert create(lib, config(image=240))[0] == -1                                   # 226 tokens: no bias instantiation past 224 keys
    assert create(lib, config(img_kind=3))[0] == -1
    # parity mode with the vector-ALU attention forced: no bias form exists there, refused at creation (the 16-bit modes and other towers are not)
    monkeypatch.setenv("MMHIP_X3_FAST", "0")
    assert create(lib, config(dtype=_lib.BF16X3))[0] == -1
    for ok in (config(), config(dtype=_lib.BF16X3, img_kind=_lib.IMG_VIT)):
        rc, h = create(lib, ok)
        assert rc == 0
        lib.mmhip_destroy(h)
    monkeypatch.delenv("MMHIP_X3_FAST")
    rc, h = create(lib, config(dtype=_lib.BF16X3))
    assert rc == 0
    lib.mmhip_destroy(h)


def test_set_drop_path(lib):
    rc, h = create(lib, config())
    assert rc == 0
    assert lib.mmhip_set_drop_path(h, 0.1) == 0 and lib.mmhip_set_drop_path(h, 0.0) == 0
    assert lib.mmhip_set_drop_path(h, -0.1) == -1 and lib.mmhip_set_drop_path(h, 1.0) == -1 and lib.mmhip_set_drop_path(h, float("nan")) == -1
    lib.mmhip_destroy(h)
    for kind in (_lib.IMG_VIT, _lib.IMG_CLIP):
        rc, h = create(lib, config(_lib.FUSION_CONCAT, img_kind=kind))
        assert rc == 0
        assert lib.mmhip_set_drop_path(h, 0.1) == -1          # a handle of another kind
        lib.mmhip_destroy(h)
    assert lib.mmhip_set_drop_path(None, 0.1) == -1
    tc = _lib.TxtConfig(hidden=128, heads=2, inter=128, layers=1, vocab=50, max_pos=16, type_vocab=1, txt_kind=_lib.TXT_XLMR, pad_id=1, ln_eps=1e-5,
                        num_labels=2, p_hidden=0.0, p_attn=0.0, p_head=0.0, dtype=_lib.BF16, max_posts=2, max_text_len=8, loss_scale=0.0)
    th = C.c_void_p()
    assert lib.mmhip_txt_create(C.byref(tc), C.byref(th)) == 0
    assert lib.mmhip_set_drop_path(th, 0.1) == -1
    lib.mmhip_txt_destroy(th)


def test_key_maps_round_trip():
    from smtc_amd.mm_late import _beit_key_to_ref, _beit_ref_to_key
    v5 = ["embeddings.cls_token", "embeddings.patch_embeddings.projection.weight", "embeddings.patch_embeddings.projection.bias", "layers.0.lambda_1",
          "layers.0.lambda_2", "layers.0.attention.q_proj.weight", "layers.0.attention.q_proj.bias", "layers.0.attention.k_proj.weight",
          "layers.0.attention.v_proj.weight", "layers.0.attention.v_proj.bias", "layers.0.attention.o_proj.weight", "layers.0.attention.o_proj.bias",
          "layers.0.layernorm_before.weight", "layers.0.layernorm_before.bias", "layers.0.layernorm_after.weight", "layers.0.layernorm_after.bias",
          "layers.0.mlp.fc1.weight", "layers.0.mlp.fc1.bias", "layers.0.mlp.fc2.weight", "layers.0.mlp.fc2.bias",
          "layers.11.relative_position_bias.relative_position_bias_table", "pooler.layernorm.weight", "pooler.layernorm.bias"]
    ref = [_beit_key_to_ref(k) for k in v5]
    assert [_beit_ref_to_key(k) for k in ref] == v5
    assert _beit_key_to_ref("layers.3.attention.q_proj.weight") == "encoder.layer.3.attention.attention.query.weight"
    assert _beit_key_to_ref("layers.3.attention.o_proj.bias") == "encoder.layer.3.attention.output.dense.bias"
    assert _beit_key_to_ref("layers.3.mlp.fc2.weight") == "encoder.layer.3.output.dense.weight"
    assert _beit_key_to_ref("layers.11.relative_position_bias.relative_position_bias_table") == \
        "encoder.layer.11.attention.attention.relative_position_bias.relative_position_bias_table"
    assert _beit_key_to_ref("layers.3.lambda_1") == "encoder.layer.3.lambda_1"
    # the mapped names are exactly the engine's vision names (minus the prefix)
    cfg = O.OracleConfig(hidden=128, heads=2, inter=256, layers_img=12, image=64, patch=16, img_kind="beit")
    own = {k[len(R.VM):] for k in R.vision_shapes(cfg)}
    assert set(ref) <= own


def test_default_arch_and_config_checks():
    from smtc_amd.mm_late import default_arch, check_beit_config, BEIT_SUPPORTED
    a = default_arch("bernice", "beit")
    assert (a["img_kind"], a["image"], a["patch"], a["ln_eps_img"], a["drop_path_rate"], a["layer_scale_init_value"]) == ("beit", 224, 16, 1e-12, 0.1, 0.1)
    assert default_arch("bernice", "vit")["drop_path_rate"] == 0.0
    with pytest.raises(ValueError, match="beit"):
        default_arch("bernice", "deit")
    good = dict(BEIT_SUPPORTED, drop_path_rate=0.1, layer_scale_init_value=0.1)
    check_beit_config(good)
    for flag, bad in (("use_shared_relative_position_bias", True), ("use_absolute_position_embeddings", True), ("use_mean_pooling", False),
                      ("use_relative_position_bias", False)):
        with pytest.raises(NotImplementedError, match=flag):
            check_beit_config(dict(good, **{flag: bad}))
    with pytest.raises(NotImplementedError, match="use_relative_position_bias"):
        check_beit_config({})                                   # HF's own defaults are not the supported configuration
    with pytest.raises(NotImplementedError, match="layer_scale"):
        check_beit_config(dict(good, layer_scale_init_value=0.0))
    with pytest.raises(NotImplementedError, match="dropout"):
        check_beit_config(dict(good, hidden_dropout_prob=0.1))


def test_vision_cache_is_refused_under_drop_path():
    """decided before the library or a GPU is touched"""
    from smtc_amd.mm_late import MM_Model, VISION_CACHE_DROP_PATH_MESSAGE
    with pytest.raises(NotImplementedError, match="stochastic depth"):
        MM_Model.enable_vision_cache(types.SimpleNamespace(drop_path_rate=0.1), 8)
    assert "drop_path_rate" in VISION_CACHE_DROP_PATH_MESSAGE
    stub = types.SimpleNamespace(arch=dict(img_kind="beit"), _vcache=dict(), drop_path_rate=0.0)
    with pytest.raises(NotImplementedError, match="stochastic depth"):
        MM_Model.set_drop_path(stub, 0.2)
    with pytest.raises(ValueError, match="BEiT"):
        MM_Model.set_drop_path(types.SimpleNamespace(arch=dict(img_kind="vit")), 0.2)


def test_command_line_takes_the_tower(monkeypatch):
    from smtc_amd.run_mm_late import build_parser, file_names
    p = build_parser()
    args = p.parse_args(["--txt_model_name", "bernice", "--img_model_name", "beit", "--fusion_name", "attention", "--task", "2", "--use_clip_loss",
                         "--use_tim_loss"])
    assert args.img_model_name == "beit"
    assert file_names(args, "/r/", "itc0.1itm0.1")["val"] == "/r/bernice-beit-attention_task2_seed30_itc0.1itm0.1_metrics_val.csv"
    text = p.format_help()
    assert "one set of stochastic-depth draws" in " ".join(text.split()) and "drop_path_rate" in text


def test_preprocessor_config(tmp_path):
    from smtc_amd.datasets import read_preprocessor_config
    assert read_preprocessor_config(str(tmp_path / "absent")) == dict(size=224, image_mean=[0.5] * 3, image_std=[0.5] * 3)
    d = tmp_path / "beit"
    d.mkdir()
    write = lambda **kw: (d / "preprocessor_config.json").write_text(json.dumps(kw))
    write(size=224, resample=2, image_mean=[0.5, 0.5, 0.5], image_std=[0.5, 0.5, 0.5], do_resize=True, do_normalize=True)
    assert read_preprocessor_config(str(d)) == dict(size=224, image_mean=[0.5] * 3, image_std=[0.5] * 3)
    write(size={"height": 384, "width": 384}, image_mean=[0.485, 0.456, 0.406], image_std=[0.229, 0.224, 0.225])
    assert read_preprocessor_config(str(d)) == dict(size=384, image_mean=[0.485, 0.456, 0.406], image_std=[0.229, 0.224, 0.225])
    for bad, what in ((dict(resample=3), "resample"), (dict(size={"height": 224, "width": 256}), "square"), (dict(size={"shortest_edge": 256}), "shortest"),
                      (dict(do_normalize=False), "do_normalize"), (dict(size=[224, 256]), "square")):
        write(**bad)
        with pytest.raises(NotImplementedError, match=what):
            read_preprocessor_config(str(d))
    # a key the reference's ViTFeatureExtractor does not know has no effect
    write(size=224, do_center_crop=True, crop_size=224)
    assert read_preprocessor_config(str(d)) == dict(size=224, image_mean=[0.5] * 3, image_std=[0.5] * 3)


def test_only_the_beit_tower_reads_the_preprocessor_file(tmp_path):
    """the decision loaders_from_data_key takes: a ViT or CLIP run keeps the fixed defaults whatever its directory holds -- a CLIP-style file (bicubic,
    centre crop, shortest-edge size, its own mean / std) neither raises nor changes anything -- and the BEiT run reads, checks and refuses"""
    from smtc_amd.datasets import image_preprocessing
    d = tmp_path / "m"
    d.mkdir()
    clip_style = dict(size={"shortest_edge": 224}, crop_size={"height": 224, "width": 224}, do_center_crop=True, resample=3,
                      image_mean=[0.48145466, 0.4578275, 0.40821073], image_std=[0.26862954, 0.26130258, 0.27577711])
    vit_style = dict(size=224, resample=2, image_mean=[0.4, 0.5, 0.6], image_std=[0.2, 0.3, 0.4])
    default = lambda size: dict(size=size, image_mean=[0.5] * 3, image_std=[0.5] * 3)
    for style in (clip_style, vit_style):
        (d / "preprocessor_config.json").write_text(json.dumps(style))
        assert image_preprocessing("clip", str(d), 224) == default(224)
        assert image_preprocessing("clip", str(d), 336) == default(336)
        assert image_preprocessing("vit", str(d), 224) == default(224)
    assert image_preprocessing("beit", str(d), 224) == dict(size=224, image_mean=[0.4, 0.5, 0.6], image_std=[0.2, 0.3, 0.4])
    with pytest.raises(ValueError, match="224"):
        image_preprocessing("beit", str(d), 64)
    (d / "preprocessor_config.json").write_text(json.dumps(clip_style))
    with pytest.raises(NotImplementedError):
        image_preprocessing("beit", str(d), 224)
    assert image_preprocessing("beit", str(tmp_path / "absent"), 224) == default(224)


# ---------------------------------------------------------------------------------------------------- the operator bounds themselves
@pytest.mark.parametrize("dt", ["bf16", "f16", "x3", "pair"])
@pytest.mark.parametrize("S,kind", [(5, "random"), (37, "asym"), (37, "perhead")])
def test_attention_bias_bounds_hold_for_the_emulation_and_reject_wrong_biases(dt, S, kind):
    posts, heads = 2, 2
    qkv, bias = R.attn_bias_inputs(dt, posts, S, heads, seed=10 * S, kind=kind)
    r = R.attn_bias_reference(qkv, bias, posts, S, heads)
    ctx_b, lse_b = R.attn_bias_bounds(r, bias, dt, S)
    assert torch.isfinite(ctx_b).all() and (ctx_b > 0).all() and ctx_b.max().item() < 0.05 * max(1.0, r.ctx.abs().max().item())
    # an fp32 evaluation with the format's casts stays inside
    fmt = OB.FMT[dt]
    s32 = (r.q.float() @ r.k.float().transpose(-1, -2) * 0.125 + bias.unsqueeze(0)).double()
    p32 = torch.softmax(s32.float(), dim=-1).double()
    p_op = OB.rnd(p32, dt) if fmt.u_p else p32
    ctx_emu = OB.rnd(p_op @ r.v, dt)
    assert ((ctx_emu - r.ctx).abs() <= ctx_b).all()
    # wrong biases leave the bounds in most elements: none, transposed (asymmetric cases), the other head's (per-head cases)
    wrong = [torch.zeros_like(bias)]
    if kind in ("random", "asym"):
        wrong.append(bias.transpose(1, 2).contiguous())
    if kind in ("random", "perhead"):
        wrong.append(bias.flip(0).contiguous())
    for wb in wrong:
        rw = R.attn_bias_reference(qkv, wb, posts, S, heads)
        assert ((rw.ctx - r.ctx).abs() > 10 * ctx_b).float().mean().item() > 0.5
        assert ((rw.lse - r.lse).abs() > 10 * lse_b).float().mean().item() > 0.4


def test_bias_image_reference_and_patch_mean_ln_bound():
    g = torch.Generator().manual_seed(3)
    for W in (2, 4, 14):
        n, P = (2 * W - 1) ** 2 + 3, W * W + 1
        table = torch.randn(n, 3, generator=g)
        img = R.bias_image(table, W, W, (P + 3) // 4 * 4)
        idx = R.relative_position_index(W, W)
        assert img.shape == (3, P, (P + 3) // 4 * 4) and (img[:, :, P:] == 0).all()
        for (h, i, j) in ((0, 0, 0), (1, 0, P - 1), (2, P - 1, 0), (1, 1, P - 1), (2, P - 1, 1), (0, P // 2, P // 3 + 1)):
            assert img[h, i, j] == table[idx[i, j], h]
    # the pooler: CLS row excluded, an fp32 evaluation stays inside the bound, including the CLS row moves it outside
    for rows, width in ((5, 128), (197, 768)):
        x = OB.rnd((torch.randn(3 * rows, width, generator=g) * 2 + 0.3).double(), "bf16")
        x.view(3, rows, width)[:, 0] += 50.0
        gamma, beta = 1 + 0.1 * torch.randn(width, generator=g), 0.02 * torch.randn(width, generator=g)
        y, b = R.patch_mean_ln_reference(x, rows, gamma, beta, 1e-12)
        y32 = torch.nn.functional.layer_norm(x.float().view(3, rows, width)[:, 1:].mean(1), (width,), gamma, beta, 1e-12).double()
        assert ((y32 - y).abs() <= b).all() and b.max().item() < 5e-3          # (the worst case of 196 sequential fp32 adds, amplified by rstd ~ 7)
        with_cls = torch.nn.functional.layer_norm(x.float().view(3, rows, width).mean(1), (width,), gamma, beta, 1e-12).double()
        assert ((with_cls - y).abs() > b).float().mean().item() > 0.9
