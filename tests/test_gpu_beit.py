"""-m gpu: --img_model_name beit through the whole HIP path (MM_Model / MMLate_Model -> C ABI -> engine) against the fixtures made by the reference's
own MM_Model over a tiny HF BeitModel (tests/golden/beit_small_*.npz) and the fp32 restatement tests/beit_ref.py.  Tolerances are the ones
tests/test_gpu_model.py holds the ViT tower to per dtype (imported, not restated); gradients are compared with the engine's ReLU pattern passed to the
restatement as relu_mask, as that file does.  The stochastic depth of the training forward is replayed draw for draw by the restatement."""
import ast
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mm_oracle as O
import beit_ref as R
from test_gpu_model import TOL_OUT, TOL_LOSS, TOL_GRAD, TOL_GRAD_MEDIAN

if torch.cuda.is_available():
    import smtc_amd  # noqa: F401
    from smtc_amd import _lib, config as smtc_config
    from smtc_amd.mm_late import MM_Model
    from gpu_util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
TAGS = ["beit_small_xlmr", "beit_small_bert"]
DTYPES = ["bf16", "f16", "bf16x3"]


def load(tag, fusion):
    z = np.load(os.path.join(GOLD, tag + ".npz"), allow_pickle=False)
    cfg = O.OracleConfig(**ast.literal_eval(str(z[f"{fusion}.cfg"])))
    return z, cfg, R.make_params(cfg, int(z["seed_w"])), (lambda k: torch.from_numpy(z[k]))


def build(cfg, P, dtype, B, T, p_zero=False, drop_path_rate=0.1, layers_img=None):
    L = cfg.layers_img if layers_img is None else layers_img
    arch = dict(hidden=cfg.hidden, heads=cfg.heads, inter=cfg.inter, layers_txt=cfg.layers_txt, layers_img=L, vocab=cfg.vocab, max_pos=cfg.max_pos,
                type_vocab=cfg.type_vocab, image=cfg.image, patch=cfg.patch, p_hidden=0.0 if p_zero else cfg.p_hidden, p_attn=0.0 if p_zero else cfg.p_attn,
                drop_path_rate=drop_path_rate)
    model = MM_Model(cfg.num_labels, "bert" if cfg.txt_kind == "bert" else "bernice", "beit", 0.0 if p_zero else cfg.p_head, cfg.fusion, arch=arch,
                     dtype=dtype, max_posts=B, max_text_len=T)
    own = {k: v for k, v in P.items() if not any(f"vision_model.encoder.layer.{l}." in k for l in range(L, cfg.layers_img))}
    missing, unexpected = model.load_state_dict(own, strict=False)
    buffers = {"dual_encoder.text_model.embeddings.position_ids"} | {f"{R.VM}encoder.layer.{l}.{R.INDEX}" for l in range(L)}
    assert unexpected == [] and set(missing) == buffers
    return model


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fusion", ["attention", "concat", "aspect-att"])
@pytest.mark.parametrize("tag", TAGS)
def test_forward_matches_reference_golden(tag, fusion, dtype):
    z, cfg, P, t = load(tag, fusion)
    T = int(z["T"])
    model = build(cfg, P, dtype, 4, T)
    model.eval()
    for B in (1, 3, 4):
        k = f"{fusion}.fwd{B}."
        pixels = O.synthetic_batch(cfg, B, T, int(z[k + "seed_x"]), True)[2]
        tim = (t(k + "tim_ids"), t(k + "tim_mask")) if fusion == "attention" else None
        with torch.no_grad():
            out_cls, lpt, out_tim, none, feats = model(t(k + "ids"), t(k + "mask"), pixels, tim_inputs=tim)
            again = model(t(k + "ids"), t(k + "mask"), pixels, tim_inputs=tim)
        assert none is None and (out_tim is None) == (tim is None)
        for a, b in zip((out_cls, lpt, feats), (again[0], again[1], again[4])):
            assert torch.equal(a, b)          # eval mode: no draw anywhere, two calls give the same bits
        outs = [("out_cls", out_cls), ("logits_per_text", lpt), ("mm_features", feats)] + ([("out_tim", out_tim)] if tim is not None else [])
        errs = {n: rel_err(v, t(k + n)) for n, v in outs}
        print("BEIT_FWD", tag, fusion, dtype, B, {n: float("%.3g" % e) for n, e in errs.items()})
        for n, e in errs.items():
            assert e < TOL_OUT[dtype][n], (B, n, e)


def grad_err(got, ref, got_norm, ref_norm):
    return max((got - ref).norm().item() / max(ref.norm().item(), 1e-20), abs(got_norm - ref_norm) / ref_norm)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("fusion,mix", [("attention", "itcitm"), ("aspect-att", "itc")])
@pytest.mark.parametrize("tag", TAGS)
def test_loss_and_gradients_match_golden_and_restatement(tag, fusion, mix, dtype):
    """a training step's loss and gradients (drop path 0, dropout 0: deterministic) with ITC and ITM under attention, with ITC under aspect-att:
    (1) against the fixture's slices and norms, (2) whole tensors against the restatement under the engine's own ReLU pattern"""
    z, cfg, P, t = load(tag, fusion)
    cfg0 = O.OracleConfig(**{**O.asdict(cfg), "p_hidden": 0.0, "p_attn": 0.0, "p_head": 0.0})
    tr, m = f"{fusion}.train.", f"{fusion}.{mix}."
    itc, itm = mix in ("itc", "itcitm"), mix in ("itm", "itcitm")
    B, T = int(z[tr + "B"]), int(z["T"])
    model = build(cfg, P, dtype, B, T, p_zero=True, drop_path_rate=0.0)
    model.train()
    dev = model.device_
    pixels = O.synthetic_batch(cfg0, B, T, int(z[tr + "seed_x"]), True)[2]
    ids, mask, onehot, w = t(tr + "ids"), t(tr + "mask"), t(tr + "onehot"), t(tr + "class_weight")
    tim = (t(tr + "tim_ids"), t(tr + "tim_mask"), t(tr + "lbl_tim"))
    bi, bm = (float(z[tr + "beta_itc"]) if itc else 0.0), (float(z[tr + "beta_itm"]) if itm else 0.0)
    model._flat_grad.zero_()
    _, _, _, feats = model._engine_forward(ids, mask, pixels, tim[0] if itm else None, tim[1] if itm else None)
    lo = torch.empty(4, device=dev)
    oh, cw, lt = onehot.to(dev).contiguous(), w.to(dev), tim[2].to(dev).contiguous()
    _lib.check(_lib.lib().mmhip_loss(model._handle, _lib.ptr(oh), _lib.ptr(cw), _lib.ptr(lt) if itm else None, 1.0 - bi - bm, bi, bm, _lib.ptr(lo), None,
                                     _lib.stream_ptr()))
    _lib.check(_lib.lib().mmhip_backward(model._handle, None, None, None, None, _lib.stream_ptr()))
    grads = {i["name"]: model._flat_grad[i["offset"]: i["offset"] + i["numel"]].view(i["shape"]).detach().float().cpu() for i in model._train_params}
    loss_v, ref_loss = lo[0].item(), float(z[m + "loss"])
    assert abs(loss_v - ref_loss) < TOL_LOSS[dtype] * abs(ref_loss), (loss_v, ref_loss)
    none_ref = {str(k) for k in z[m + "grad_none"]}
    groups = model.active_groups(itc, itm)
    for i in model._train_params:
        assert (i["name"] in none_ref) == (i["group"] not in groups), i["name"]
        if i["name"] in none_ref:
            assert grads[i["name"]].abs().max().item() == 0.0, i["name"]
    watch = [k for k in (str(s) for s in z["watch"]) if k not in none_ref]
    mask_eng = (feats.detach().cpu() > 0).float()
    flips = int((mask_eng != (t(m + "mm_features") > 0).float()).sum())
    assert flips <= 0.01 * feats.numel(), flips
    _, r_loss, _, _, G = R.loss_and_grads(P, ids, mask, pixels, onehot, w, cfg0, itc, itm, tim, 0.1, 0.1, relu_mask=mask_eng)
    assert abs(loss_v - r_loss.item()) < TOL_LOSS[dtype] * abs(r_loss.item())
    whole = {k: grad_err(grads[k], G[k], 1.0, 1.0) for k in watch}
    print("BEIT_GRADERR restated", tag, fusion, mix, dtype, "flips", flips, {k: float("%.3g" % e) for k, e in whole.items()})
    for k, e in whole.items():
        assert e < TOL_GRAD[dtype], (k, e)
    assert float(np.median(list(whole.values()))) < TOL_GRAD_MEDIAN[dtype], sorted(whole.values())
    if flips == 0:          # the same function was differentiated: the fixture's own slices and norms
        worst = {}
        for k in watch:
            g = grads[k]
            sl = g[t(m + f"gslice_rows.{k}")][:, :48] if k.endswith("word_embeddings.weight") else (g[:8, :48] if g.dim() == 2 else g.flatten()[:64])
            worst[k] = grad_err(sl, t(m + f"gslice.{k}"), g.norm().item(), float(z[m + f"gnorm.{k}"]))
        print("BEIT_GRADERR golden", tag, fusion, mix, dtype, {k: float("%.3g" % e) for k, e in worst.items()})
        for k, e in worst.items():
            assert e < TOL_GRAD[dtype], (k, e)
        assert float(np.median(list(worst.values()))) < TOL_GRAD_MEDIAN[dtype]
    # the tower is frozen: nothing of it is a trainable parameter
    assert not any("vision_model" in i["name"] for i in model._train_params)


def tower_output(model, B):
    """last_hidden_state [B, P, H] and pooler_output [B, H] of the engine's last forward, through the image-tower cache records"""
    lib = _lib.lib()
    rec = int(lib.mmhip_vision_record_bytes(model._handle))
    buf = torch.zeros(B * rec, dtype=torch.uint8, device=model.device_)
    slots = torch.arange(B, dtype=torch.int64, device=model.device_)
    _lib.check(lib.mmhip_vision_export(model._handle, _lib.ptr(slots), _lib.ptr(buf), B, _lib.stream_ptr()), "vision_export")
    torch.cuda.synchronize()
    a = model.arch
    Pn, H = (a["image"] // a["patch"]) ** 2 + 1, a["hidden"]
    et = {"bf16": torch.bfloat16, "f16": torch.float16, "bf16x3": torch.float32}[model.dtype_name]
    nb = Pn * H * (4 if model.dtype_name == "bf16x3" else 2)
    rows = buf.view(B, rec)
    tok = rows[:, :nb].contiguous().view(et).view(B, Pn, H)
    pool = rows[:, nb: nb + H * 4].contiguous().view(torch.float32).view(B, H)
    return tok.cpu(), pool.cpu()


@pytest.mark.parametrize("dtype", DTYPES)
def test_drop_path_forward_replays_the_kernels_draws(dtype):
    """rate 0.5 on the 2-layer model (layer 0 never drops, layer 1 drops each branch of each post with probability 1/2), train mode, every other
    dropout off: the outputs equal the restatement replaying the draws of this forward's seed; a post with both branches of layer 1 dropped leaves
    the tower with its layer-0 output bit for bit; a second forward draws again"""
    z, cfg, P, t = load("beit_small_xlmr", "attention")
    cfg0 = O.OracleConfig(**{**O.asdict(cfg), "p_hidden": 0.0, "p_attn": 0.0, "p_head": 0.0})
    B, T = 8, int(z["T"])
    ids, mask, pixels, _ = O.synthetic_batch(cfg0, B, T, 77, True)
    model = build(cfg, P, dtype, B, T, p_zero=True, drop_path_rate=0.0)
    model.set_drop_path(0.5)
    model.train()
    with torch.no_grad():
        out_cls, lpt, _, _, feats = model(ids, mask, pixels)
    seed = model._last["seed"]
    tok, pool = tower_output(model, B)
    k0, s0 = R.droppath_keep(seed, 1, 0, B, R.drop_path_p(0.5, 1, 2))
    k1, s1 = R.droppath_keep(seed, 1, 1, B, R.drop_path_p(0.5, 1, 2))
    assert (s0, s1) == (2.0, 2.0) and (~k0 & ~k1).any() and (k0 | k1).any(), (k0, k1)
    with torch.no_grad():
        x_v, v_pool = R.beit_forward(P, pixels, cfg0, (0.5, seed))
        r_cls, r_lpt, _, _, r_feats = R.mm_forward(P, ids, mask, pixels, cfg0, drop_path=(0.5, seed))
        x_eval = R.beit_forward(P, pixels, cfg0)[0]
    errs = dict(out_cls=rel_err(out_cls, r_cls), logits_per_text=rel_err(lpt, r_lpt), mm_features=rel_err(feats, r_feats))
    tower = dict(tokens=rel_err(tok, x_v), pooler=rel_err(pool, v_pool))
    print("BEIT_DROPPATH", dtype, {n: float("%.3g" % e) for n, e in {**errs, **tower}.items()}, "kept", k0.astype(int).tolist(), k1.astype(int).tolist())
    for n, e in errs.items():
        assert e < TOL_OUT[dtype][n], (n, e)
    assert tower["tokens"] < TOL_OUT[dtype]["mm_features"] and tower["pooler"] < TOL_OUT[dtype]["mm_features"]
    # the draws matter: on the posts that kept a branch (scaled by 2) the eval-mode tower is 2.8e-2 away, the dropped posts' lack of layer 1 more;
    # in the parity mode the replay is three orders of magnitude closer than that
    kept = torch.from_numpy(k0 | k1)
    effect = rel_err(x_v[kept], x_eval[kept])
    assert effect > 1e-2 and rel_err(x_v[~kept], x_eval[~kept]) > 1e-2
    if dtype == "bf16x3":
        assert tower["tokens"] < effect / 1000
    # layer-0 output of the same engine kernels: a one-layer tower with the same weights, eval mode
    one = build(cfg, P, dtype, B, T, p_zero=True, drop_path_rate=0.0, layers_img=1)
    one.eval()
    with torch.no_grad():
        one(ids, mask, pixels)
    tok1, _ = tower_output(one, B)
    for b in range(B):
        if not k0[b] and not k1[b]:
            assert torch.equal(tok[b], tok1[b]), b
        else:
            assert not torch.equal(tok[b], tok1[b]), b
    # another forward, another seed, other draws; eval mode ignores the rate
    with torch.no_grad():
        again = model(ids, mask, pixels)[0]
    assert model._last["seed"] != seed and not torch.equal(again, out_cls)
    model.eval()
    with torch.no_grad():
        e1, e2 = model(ids, mask, pixels)[0], model(ids, mask, pixels)[0]
        r_eval = R.mm_forward(P, ids, mask, pixels, cfg0)[0]
    assert torch.equal(e1, e2) and rel_err(e1, r_eval) < TOL_OUT[dtype]["out_cls"]


def test_state_dict_round_trips_with_the_reference_checkpoint_keys():
    z, cfg, P, t = load("beit_small_xlmr", "attention")
    T = int(z["T"])
    model = build(cfg, P, "bf16x3", 4, T)
    sd = model.state_dict()
    buffers = R.buffer_shapes(cfg)
    assert set(sd) == set(P) | set(buffers) | {"dual_encoder.text_model.embeddings.position_ids"}
    for k, v in P.items():
        assert torch.equal(sd[k].cpu(), v), k
    idx = torch.from_numpy(R.relative_position_index(4, 4))
    for k in buffers:
        assert sd[k].dtype == torch.int64 and torch.equal(sd[k].cpu(), idx), k
    assert not any("key.bias" in k for k in sd if "vision_model" in k)
    # a checkpoint as the reference writes it (every key, the index buffers included) loads strictly into a fresh model and computes the same
    other = build(cfg, R.make_params(cfg, 5), "bf16x3", 4, T)
    other.load_state_dict({k: v.cpu() for k, v in sd.items()}, strict=True)
    model.eval()
    other.eval()
    k = "attention.fwd3."
    pixels = O.synthetic_batch(cfg, 3, T, int(z[k + "seed_x"]), True)[2]
    with torch.no_grad():
        a, b = model(t(k + "ids"), t(k + "mask"), pixels), other(t(k + "ids"), t(k + "mask"), pixels)
    assert torch.equal(a[0], b[0]) and torch.equal(a[4], b[4])
    assert rel_err(a[0], t(k + "out_cls")) < TOL_OUT["bf16x3"]["out_cls"]


def test_refusals(tmp_path, monkeypatch):
    z, cfg, P, t = load("beit_small_xlmr", "concat")
    T = int(z["T"])
    model = build(cfg, P, "bf16", 4, T)                       # drop_path_rate 0.1, as the checkpoint's config has it
    with pytest.raises(NotImplementedError, match="stochastic depth"):
        model.enable_vision_cache(8)
    model.set_drop_path(0.0)
    model.enable_vision_cache(8)                              # a deterministic tower may be cached
    with pytest.raises(NotImplementedError, match="stochastic depth"):
        model.set_drop_path(0.1)
    with pytest.raises(NotImplementedError, match="equally wide|as wide as"):
        MM_Model(2, "bernice", "beit", 0.05, "attention", arch=dict(layers_txt=1, layers_img=1, hidden_img=256, heads_img=4, inter_img=256))
    vit = MM_Model(2, "bernice", "vit", 0.05, "concat", arch=dict(layers_txt=1, layers_img=1, hidden=128, heads=2, inter=256, image=64, vocab=100), max_posts=2,
                   max_text_len=8)
    assert _lib.lib().mmhip_set_drop_path(vit._handle, 0.1) == -1
    with pytest.raises(ValueError, match="BEiT"):
        vit.set_drop_path(0.1)
    # a model directory whose config.json asks for another BEiT than the one built
    d = tmp_path / "BEiT"
    d.mkdir()
    base = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=1, intermediate_size=256, image_size=64, patch_size=16, layer_norm_eps=1e-12,
                use_absolute_position_embeddings=False, use_relative_position_bias=True, use_shared_relative_position_bias=False, use_mean_pooling=True,
                layer_scale_init_value=0.1, drop_path_rate=0.2)
    monkeypatch.setitem(smtc_config.MODEL_DIR_DICT, "beit", str(d))
    arch = dict(layers_txt=1, hidden=128, heads=2, inter=256, vocab=100)
    (d / "config.json").write_text(json.dumps(base))
    ok = MM_Model(2, "bernice", "beit", 0.05, "concat", arch=arch, max_posts=2, max_text_len=8)
    assert ok.drop_path_rate == pytest.approx(0.2) and ok.arch["layers_img"] == 1 and ok.arch["image"] == 64
    for flag, bad in (("use_shared_relative_position_bias", True), ("use_absolute_position_embeddings", True), ("use_mean_pooling", False)):
        (d / "config.json").write_text(json.dumps(dict(base, **{flag: bad})))
        with pytest.raises(NotImplementedError, match=flag):
            MM_Model(2, "bernice", "beit", 0.05, "concat", arch=arch, max_posts=2, max_text_len=8)


def test_checkpoint_directory_loads_every_tower_parameter_or_raises(tmp_path, monkeypatch):
    """a model directory in the installed transformers' naming (config.json + model.safetensors): every frozen parameter is assigned and the model
    computes the fixture; a checkpoint that misses a tensor, or holds one of another shape, raises instead of leaving the initial value in place"""
    from safetensors.torch import save_file
    from smtc_amd.mm_late import _beit_ref_to_key
    z, cfg, P, t = load("beit_small_xlmr", "concat")
    T = int(z["T"])
    d = tmp_path / "BEiT"
    d.mkdir()
    (d / "config.json").write_text(json.dumps(dict(
        hidden_size=cfg.hidden, num_attention_heads=cfg.heads, num_hidden_layers=cfg.layers_img, intermediate_size=cfg.inter, image_size=cfg.image,
        patch_size=cfg.patch, layer_norm_eps=1e-12, use_absolute_position_embeddings=False, use_relative_position_bias=True,
        use_shared_relative_position_bias=False, use_mean_pooling=True, layer_scale_init_value=0.1, drop_path_rate=0.1)))
    vision = {_beit_ref_to_key(k[len(R.VM):]): v.contiguous() for k, v in P.items() if k.startswith(R.VM)}
    monkeypatch.setitem(smtc_config.MODEL_DIR_DICT, "beit", str(d))
    arch = dict(hidden=cfg.hidden, heads=cfg.heads, inter=cfg.inter, layers_txt=cfg.layers_txt, vocab=cfg.vocab, max_pos=cfg.max_pos)
    make = lambda: MM_Model(cfg.num_labels, "bernice", "beit", cfg.p_head, "concat", arch=arch, dtype="bf16x3", max_posts=4, max_text_len=T)
    save_file(vision, str(d / "model.safetensors"))
    model = make()
    sd = model.state_dict()
    for k, v in P.items():
        if k.startswith(R.VM):
            assert torch.equal(sd[k].cpu(), v), k
    model.load_state_dict({k: v for k, v in P.items() if not k.startswith(R.VM)}, strict=False)
    model.eval()
    k = "concat.fwd3."
    with torch.no_grad():
        out = model(t(k + "ids"), t(k + "mask"), O.synthetic_batch(cfg, 3, T, int(z[k + "seed_x"]), True)[2])[0]
    assert rel_err(out, t(k + "out_cls")) < TOL_OUT["bf16x3"]["out_cls"]
    table = "layers.1.relative_position_bias.relative_position_bias_table"
    for broken in ({n: v for n, v in vision.items() if n != "layers.0.lambda_2"}, dict(vision, **{table: torch.zeros(732, cfg.heads)})):
        save_file(broken, str(d / "model.safetensors"))
        with pytest.raises(_lib.MMHipError, match="not found in it"):
            make()


def test_command_line_trains_to_its_csvs(tmp_path):
    cmd = ["timeout", "-k", "10", "200", sys.executable, "-m", "smtc_amd.run_mm_late", "--txt_model_name", "bernice", "--img_model_name", "beit",
           "--fusion_name", "attention", "--use_clip_loss", "--use_tim_loss", "--task", "2", "--synthetic", "--arch_layers", "1", "--n_synthetic", "32",
           "--batch_size", "8", "--epochs", "1", "--results_dir", str(tmp_path) + "/"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    stem = "bernice-beit-attention_task2_seed30_itc0.1itm0.1_"
    for kind in ("val", "test"):
        path = os.path.join(str(tmp_path), stem + f"metrics_{kind}.csv")
        assert os.path.exists(path), os.listdir(str(tmp_path))
        assert len(open(path).read().splitlines()) > 1
