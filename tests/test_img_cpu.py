"""Image-only path, CPU side (no launches): the library's exports, the C ABI's parameter layout against the reference golden's key list, the stage
ranges, the refusals of create and across handle kinds, the command line."""
import ctypes as C
import os

import numpy as np
import pytest

import smtc_amd  # noqa: F401
from smtc_amd import _lib
import img_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "img_small_vit.npz")
NAMES = ["mmhip_img_create", "mmhip_img_destroy", "mmhip_img_param_count", "mmhip_img_param_info_at", "mmhip_img_numel", "mmhip_img_workspace_bytes",
         "mmhip_img_bind", "mmhip_img_refresh_weights", "mmhip_img_forward", "mmhip_img_loss", "mmhip_img_backward", "mmhip_img_train_step",
         "mmhip_op_vit_embed_bwd", "mmhip_op_vit_embed_bwd_ws_bytes"]


def _img_cfg(**kw):
    base = dict(hidden=768, heads=12, inter=3072, layers=2, image=192, patch=16, ln_eps=1e-12, num_labels=3, dtype=_lib.BF16, max_posts=2, loss_scale=0.0,
                p_hidden=0.0, p_attn=0.0)
    base.update(kw)
    return _lib.ImgConfig(**base)


def _create(cfg):
    h = C.c_void_p()
    assert _lib.lib().mmhip_img_create(C.byref(cfg), C.byref(h)) == 0
    return h


def _infos(h):
    lib, out, pi = _lib.lib(), [], _lib.ParamInfo()
    for i in range(lib.mmhip_img_param_count(h)):
        assert lib.mmhip_img_param_info_at(h, i, C.byref(pi)) == 0
        out.append((pi.name.decode(), tuple(pi.dims[: pi.ndim]), pi.buffer, pi.group, int(pi.offset), int(pi.numel)))
    return out


def test_library_exports_the_new_names():
    lib = _lib.lib()
    for n in NAMES:
        assert n in _lib.EXPORTS and hasattr(lib, n), n


def test_dtype_codes_are_the_header_enum():
    """_lib.BF16 / F16 / F32 / BF16X3 / PAIR, which the operator tests pass to the entry points, are the values include/mmhip.h gives them"""
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmhip.h")) as f:
        enum = dict((k, int(v)) for k, v in re.findall(r"\bMMHIP_(BF16X3|BF16|F16|F32|PAIR)\s*=\s*(\d+)", f.read()))
    assert enum == dict(BF16=_lib.BF16, F16=_lib.F16, F32=_lib.F32, BF16X3=_lib.BF16X3, PAIR=_lib.PAIR)


def test_layout_is_the_reference_state_dict():
    """names and shapes = the key list the reference's ViTForImageClassification gave (the golden), every tensor trainable in one group; q/k/v weights
    and biases of a layer contiguous; order [classifier, vit.layernorm | layers last -> first | patch weight, patch bias, positions, cls_token]"""
    lib = _lib.lib()
    h = _create(_img_cfg())
    infos = _infos(h)
    want = R.param_shapes(R.oracle_cfg())
    assert sorted(n for n, *_ in infos) == [str(k) for k in np.load(GOLD, allow_pickle=False)["keys"]]
    assert {n: s for n, s, *_ in infos} == want
    assert all(buf == 1 and grp == _lib.G_ALWAYS for _n, _s, buf, grp, _o, _c in infos)
    at = {n: (off, cnt) for n, _s, _b, _g, off, cnt in infos}
    end = 0
    for _n, _s, _b, _g, off, cnt in infos:                      # layout order is address order, nothing overlaps
        assert off >= end and off % 4 == 0
        end = off + cnt
    assert end <= lib.mmhip_img_numel(h)
    for l in range(2):
        p = f"vit.encoder.layer.{l}.attention.attention."
        for kind, n in (("weight", 768 * 768), ("bias", 768)):
            q, k, v = (at[p + x + "." + kind][0] for x in ("query", "key", "value"))
            assert k == q + n and v == k + n
    names = [n for n, *_ in infos]
    assert names[:4] == ["classifier.weight", "classifier.bias", "vit.layernorm.weight", "vit.layernorm.bias"]
    assert names[4].startswith("vit.encoder.layer.1.") and names[-5].startswith("vit.encoder.layer.0.")
    assert names[-4:] == ["vit.embeddings.patch_embeddings.projection.weight", "vit.embeddings.patch_embeddings.projection.bias",
                          "vit.embeddings.position_embeddings", "vit.embeddings.cls_token"]
    # stages tile [0, numel) in backward order: head + final LayerNorm, layers last -> first, embeddings
    assert lib.mmhip_num_backward_stages(h) == 4
    b, e, cur = C.c_uint64(), C.c_uint64(), 0
    for st, first in enumerate(["classifier.weight", "vit.encoder.layer.1.attention.attention.query.weight",
                                "vit.encoder.layer.0.attention.attention.query.weight", "vit.embeddings.patch_embeddings.projection.weight"]):
        assert lib.mmhip_stage_grad_range(h, st, C.byref(b), C.byref(e)) == 0
        assert b.value == cur == at[first][0] and e.value > b.value
        cur = e.value
    assert cur == lib.mmhip_img_numel(h)
    assert lib.mmhip_stage_grad_range(h, 4, C.byref(b), C.byref(e)) == -1
    assert lib.mmhip_img_workspace_bytes(h) > 0
    lib.mmhip_img_destroy(h)


@pytest.mark.parametrize("bad", [dict(image=160), dict(image=384), dict(image=224, patch=14), dict(p_hidden=0.1), dict(p_attn=0.1), dict(patch=12, image=144),
                                 dict(num_labels=17), dict(hidden=704, heads=11), dict(heads=8), dict(inter=3000), dict(dtype=7), dict(max_posts=0)])
def test_create_rejects(bad):
    """a token count outside 129..288 (160 px: 101, 384 px: 577, 224 / 14: 257 is inside but 3 * 14^2 = 588 is no multiple of 64), a non-zero tower
    dropout, 3 * patch^2 no multiple of 64 (12 x 12 at 144 px: 145 tokens, 432), num_labels > 16, the hidden / heads / inter rules of mmhip_txt_create"""
    h = C.c_void_p()
    cfg = _img_cfg(**bad)
    assert _lib.lib().mmhip_img_create(C.byref(cfg), C.byref(h)) == -1


@pytest.mark.parametrize("image", [192, 224, 256])
def test_create_accepts_the_token_range(image):
    h = _create(_img_cfg(image=image))
    assert _lib.lib().mmhip_img_numel(h) > 0
    _lib.lib().mmhip_img_destroy(h)


def test_cross_handle_calls_are_refused():
    """late-fusion and text-only calls answer an error on an image handle, and the reverse -- before anything is touched (nothing is bound here)"""
    lib = _lib.lib()
    hi = _create(_img_cfg())
    txt = _lib.TxtConfig(hidden=768, heads=12, inter=3072, layers=2, vocab=500, max_pos=130, type_vocab=1, txt_kind=_lib.TXT_XLMR, pad_id=1, ln_eps=1e-5,
                         num_labels=3, p_hidden=0.1, p_attn=0.1, p_head=0.05, dtype=_lib.BF16, max_posts=4, max_text_len=32, loss_scale=0.0)
    ht = C.c_void_p()
    assert lib.mmhip_txt_create(C.byref(txt), C.byref(ht)) == 0
    mm = _lib.Config(hidden=768, heads=12, inter=3072, layers_txt=2, layers_img=2, vocab=500, max_pos=130, type_vocab=1, txt_kind=1, pad_id=1,
                     ln_eps_txt=1e-5, ln_eps_img=1e-12, image=224, patch=16, proj_dim=512, num_labels=3, fusion=1, p_hidden=0.1, p_attn=0.1,
                     p_head=0.05, dtype=0, max_posts=4, max_text_len=32, loss_scale=0.0)
    hm = C.c_void_p()
    assert lib.mmhip_create(C.byref(mm), C.byref(hm)) == 0
    fake = C.c_void_p(256)          # a non-null, aligned address: every call below must answer before it looks at it
    # on the image handle
    assert lib.mmhip_txt_param_count(hi) == -1 and lib.mmhip_txt_numel(hi) == 0 and lib.mmhip_txt_workspace_bytes(hi) == 0
    assert lib.mmhip_txt_bind(hi, fake, fake, fake, 1 << 40) == -1
    assert lib.mmhip_txt_refresh_weights(hi, None) == -1
    assert lib.mmhip_txt_forward(hi, fake, fake, None, 1, 8, 0, 0, None, None) == -2
    assert lib.mmhip_txt_loss(hi, fake, None, None, None, None) == -2
    assert lib.mmhip_txt_backward(hi, None, None) == -2
    assert lib.mmhip_bind(hi, fake, fake, fake, fake, 1 << 40) == -1
    assert lib.mmhip_refresh_weights(hi, 3, None) == -2
    assert lib.mmhip_forward(hi, fake, fake, fake, None, None, 1, 8, 0, 0, None, None, None, None, None) == -2
    assert lib.mmhip_loss(hi, fake, None, None, 1.0, 0.0, 0.0, None, None, None) == -2
    assert lib.mmhip_reserve_itc_global(hi, 2) == -2 and lib.mmhip_set_itc_global(hi, 1, 0) == -2
    # image calls on the other kinds
    for h in (ht, hm):
        assert lib.mmhip_img_param_count(h) == -1 and lib.mmhip_img_numel(h) == 0 and lib.mmhip_img_workspace_bytes(h) == 0
        assert lib.mmhip_img_bind(h, fake, fake, fake, 1 << 40) == -1
        assert lib.mmhip_img_refresh_weights(h, None) == -1
        assert lib.mmhip_img_forward(h, fake, 1, 0, None, None) == -2
        assert lib.mmhip_img_loss(h, fake, None, None, None, None) == -2
        assert lib.mmhip_img_backward(h, None, None) == -2
        assert lib.mmhip_img_train_step(h, fake, fake, None, 1, fake, fake, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, None, None, None) == -2
    # the per-handle setters that make sense take an image handle
    assert lib.mmhip_set_loss_scale(hi, 512.0) == 0 and lib.mmhip_set_guard(hi, None) == 0 and lib.mmhip_set_backward_products(hi, 3) == 0
    assert lib.mmhip_set_backward_products(hi, 2) == -2          # a bf16 handle has one product
    assert lib.mmhip_step_spans(hi, 0, None) == 0
    lib.mmhip_img_destroy(ht)          # wrong kind: ignored
    lib.mmhip_txt_destroy(ht)
    lib.mmhip_destroy(hm)
    lib.mmhip_img_destroy(hi)


def test_op_entry_rejects_before_any_launch():
    """mmhip_op_vit_embed_bwd: shape rules and alignment are answered on the host"""
    lib = _lib.lib()
    a = lambda off=0: C.c_void_p(4096 + off)
    f = lambda dtype=_lib.BF16, dx=a(), B=2, P=145, H=768, dpos=a(), dcls=a(), dpe=a(), ws=None, wsb=0: \
        lib.mmhip_op_vit_embed_bwd(dtype, dx, B, P, H, 1.0, dpos, dcls, dpe, 0, ws, wsb, None)
    assert f(H=764) == -1 and f(H=1032) == -1 and f(P=1) == -1 and f(B=0) == -1 and f(dtype=9) == -1 and f(dx=None) == -1 and f(dpe=None) == -1
    for k in ("dx", "dpos", "dcls", "dpe"):
        assert f(**{k: a(8)}) == -1, k
    assert lib.mmhip_op_vit_embed_bwd_ws_bytes(8, 145, 768) == 0 and lib.mmhip_op_vit_embed_bwd_ws_bytes(9, 145, 768) == 2 * 145 * 768 * 4
    assert f(B=9) == -3 and f(B=9, ws=a(), wsb=16) == -3 and f(B=9, ws=a(8), wsb=1 << 30) == -1


def test_parser_accepts_the_reference_command_lines():
    from smtc_amd.run_img import build_parser, check_supported, file_names
    p = build_parser()
    a = p.parse_args("--model_name vit --task 3".split())
    assert (a.epochs, a.weight_decay, a.lr, a.dropout, a.seed) == (2, 0.00025, 1e-5, 0.05, 30)
    assert not (a.testing or a.save_model or a.save_preds or a.conv_att or a.feature_extract or a.synthetic) and a.dtype == "bf16"
    check_supported(a)
    a = p.parse_args("--model_name vit --task 2 --epochs 10 --weight_decay 0.01 --lr 2e-5 --dropout 0.1 --seed 7 --testing --save_model --save_preds".split())
    assert a.task == 2 and a.epochs == 10 and a.testing and a.save_model and a.save_preds
    names = file_names(a, "../results/img_only/")
    assert names["val"] == "../results/img_only/vit_task2_seed7_metrics_val.csv" and names["model"].endswith("vit_task2_seed7_net.pth")
    assert p.parse_args("--model_name vit --task 3 --synthetic --dtype bf16x3 --arch_layers 2".split()).arch_layers == 2
    for m in ("beit", "deit", "resnet50", "resnet152"):
        with pytest.raises(NotImplementedError):
            check_supported(p.parse_args(["--model_name", m, "--task", "0"]))
    for flag in ("--conv_att", "--feature_extract"):
        with pytest.raises(NotImplementedError):
            check_supported(p.parse_args(["--model_name", "vit", "--task", "0", flag]))


def test_refusals(monkeypatch):
    from smtc_amd.image_only import ImageModel
    from smtc_amd.run_img import main
    for m in ("beit", "deit", "resnet50"):
        with pytest.raises(NotImplementedError):
            ImageModel(8, 3, m)
        with pytest.raises(NotImplementedError):
            main(["--model_name", m, "--task", "3", "--synthetic"])
    with pytest.raises(NotImplementedError):
        ImageModel(8, 3, "vit", conv_att=True)
    with pytest.raises(NotImplementedError):
        main("--model_name vit --task 3 --synthetic --conv_att".split())
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="single-process"):
        main("--model_name vit --task 3 --synthetic".split())
