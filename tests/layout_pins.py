"""What a handle's host-side layout consists of, measured through the C ABI alone (mmhip_create and its siblings do no GPU work): the parameter
table, both buffer sizes, the workspace size, every backward stage's gradient range and, for a late-fusion handle, the workspace size after
mmhip_reserve_itc_global(h, 4).  tests/golden/make_layout_pins.py records these into tests/golden/layout_pins.json; test_layout_pins_cpu.py
asserts them, so a change of the layout or of the workspace carve-up is a failing test, not a silent shift of every offset."""
import ctypes as C
import hashlib
import os

from smtc_amd import _lib

# (suffix, dtype, MMHIP_X3_PAIRS): bf16, the parity mode with plane pairs (the variable unset) and without (=0)
MODES = [("bf16", _lib.BF16, None), ("bf16x3", _lib.BF16X3, None), ("bf16x3_nopairs", _lib.BF16X3, "0")]


def _late(**kw):
    base = dict(hidden=768, heads=12, inter=3072, layers_txt=2, layers_img=2, vocab=1000, max_pos=130, type_vocab=1, txt_kind=_lib.TXT_XLMR,
                pad_id=1, ln_eps_txt=1e-5, ln_eps_img=1e-12, image=224, patch=16, proj_dim=512, num_labels=3, fusion=_lib.FUSION_CONCAT,
                p_hidden=0.1, p_attn=0.1, p_head=0.05, dtype=_lib.BF16, max_posts=4, max_text_len=64, loss_scale=0.0)
    base.update(kw)
    return "late", _lib.Config(**base)


def _txt(**kw):
    base = dict(hidden=768, heads=12, inter=3072, layers=2, vocab=1000, max_pos=130, type_vocab=1, txt_kind=_lib.TXT_XLMR, pad_id=1, ln_eps=1e-5,
                num_labels=3, p_hidden=0.1, p_attn=0.1, p_head=0.05, dtype=_lib.BF16, max_posts=4, max_text_len=64, loss_scale=0.0)
    base.update(kw)
    return "txt", _lib.TxtConfig(**base)


def _img(**kw):
    base = dict(hidden=768, heads=12, inter=3072, layers=2, image=224, patch=16, ln_eps=1e-12, num_labels=3, dtype=_lib.BF16, max_posts=4,
                loss_scale=0.0, p_hidden=0.0, p_attn=0.0)
    base.update(kw)
    return "img", _lib.ImgConfig(**base)


_CLIP = dict(img_kind=_lib.IMG_CLIP, hidden_img=1024, heads_img=16, inter_img=4096, patch=14)


def cases():
    """{case id: (handle kind, config, MMHIP_X3_PAIRS or None)}: 2 layers, max_posts 4, max_text_len 64 throughout"""
    out = {}
    for tag, dtype, pairs in MODES:
        shapes = {"late_concat_vit224": _late(dtype=dtype), "late_attention_vit224": _late(dtype=dtype, fusion=_lib.FUSION_ATTENTION),
                  "late_aspect_vit224": _late(dtype=dtype, fusion=_lib.FUSION_ASPECT),
                  "late_concat_clip224": _late(dtype=dtype, image=224, **_CLIP), "late_concat_clip336": _late(dtype=dtype, image=336, **_CLIP),
                  "txt_xlmr": _txt(dtype=dtype), "txt_bert": _txt(dtype=dtype, type_vocab=2, txt_kind=_lib.TXT_BERT, pad_id=0),
                  "img_192": _img(dtype=dtype, image=192), "img_224": _img(dtype=dtype, image=224), "img_256": _img(dtype=dtype, image=256)}
        for name, (kind, cfg) in shapes.items():
            out[f"{name}-{tag}"] = (kind, cfg, pairs)
    return out


# per handle kind: create, destroy, param_count, param_info_at, workspace_bytes, and the two buffer sizes
_API = {"late": ("mmhip_create", "mmhip_destroy", "mmhip_param_count", "mmhip_param_info_at", "mmhip_workspace_bytes"),
        "txt": ("mmhip_txt_create", "mmhip_txt_destroy", "mmhip_txt_param_count", "mmhip_txt_param_info_at", "mmhip_txt_workspace_bytes"),
        "img": ("mmhip_img_create", "mmhip_img_destroy", "mmhip_img_param_count", "mmhip_img_param_info_at", "mmhip_img_workspace_bytes")}


def measure(kind, cfg, pairs):
    lib = _lib.lib()
    create, destroy, count, info_at, ws_bytes = (getattr(lib, n) for n in _API[kind])
    saved = os.environ.pop("MMHIP_X3_PAIRS", None)          # read by the library at create
    if pairs is not None:
        os.environ["MMHIP_X3_PAIRS"] = pairs
    try:
        h = C.c_void_p()
        assert create(C.byref(cfg), C.byref(h)) == 0
    finally:
        os.environ.pop("MMHIP_X3_PAIRS", None)
        if saved is not None:
            os.environ["MMHIP_X3_PAIRS"] = saved
    sha, pi, n = hashlib.sha256(), _lib.ParamInfo(), count(h)
    for i in range(n):
        assert info_at(h, i, C.byref(pi)) == 0
        sha.update(repr((pi.name.decode(), tuple(pi.dims[: pi.ndim]), pi.buffer, pi.group, int(pi.offset), int(pi.numel))).encode())
    if kind == "late":
        numel = [int(lib.mmhip_buffer_numel(h, 0)), int(lib.mmhip_buffer_numel(h, 1))]
    else:
        numel = [0, int((lib.mmhip_txt_numel if kind == "txt" else lib.mmhip_img_numel)(h))]
    got = dict(params=n, params_sha256=sha.hexdigest(), buffer_numel=numel, workspace_bytes=int(ws_bytes(h)), stage_grad_range=[])
    b, e = C.c_uint64(), C.c_uint64()
    for st in range(lib.mmhip_num_backward_stages(h)):
        assert lib.mmhip_stage_grad_range(h, st, C.byref(b), C.byref(e)) == 0
        got["stage_grad_range"].append([int(b.value), int(e.value)])
    if kind == "late":
        assert lib.mmhip_reserve_itc_global(h, 4) == 0
        got["workspace_bytes_itc_global_4"] = int(ws_bytes(h))
    destroy(h)
    return got
