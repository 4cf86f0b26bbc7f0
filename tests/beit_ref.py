"""fp32 restatement of the late-fusion model with the BEiT image tower (--img_model_name beit: HF BeitModel inside VisionTextDualEncoderModel, reference
models/mm_late.py:59, models/config.py:145), composed from the pinned oracle (oracle.mm_oracle is imported, not modified), and the fp64 references of
the three BEiT operators with their per-element error bounds.

The tower, in the configuration of microsoft/beit-base-patch16-224-pt22k-ft22k (no absolute positions, a relative position bias per layer, mean
pooling, layer scale, stochastic depth):

    x = [cls_token | patch_conv(pixels)]
    per layer:  y = LN_before(x);  q = y Wq^T + bq;  k = y Wk^T (no bias);  v = y Wv^T + bv
                s = q k^T / sqrt(64) + bias[h];  a = softmax(s) v;  x = x + droppath(lambda_1 * (a Wo^T + bo))
                x = x + droppath(lambda_2 * fc2(gelu(fc1(LN_after(x)))))
    last_hidden_state = x;  pooler_output = LN_pooler(mean over the patch tokens of x)

bias[h, i, j] = table[index[i, j], h] (relative_position_index below; tests/test_beit_golden_cpu.py holds it to HF's).  droppath draws one Bernoulli
variable per post and branch, active in train mode at p_l = linspace(0, rate, L)[l] > 0; the draws are the engine's hash (droppath_keep), so a
kernel run is replayed exactly.  The ITM pass reuses the first pass's image tokens, as the engine does (the one deviation)."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import mm_oracle as O
import aspect_ref as A
import op_bounds as OB

VM = "dual_encoder.vision_model."
REL = "attention.attention.relative_position_bias."
TABLE = REL + "relative_position_bias_table"
INDEX = REL + "relative_position_index"


def window(cfg):
    return cfg.image // cfg.patch


def relative_position_index(wh, ww):
    """int64 [P, P], P = wh * ww + 1: patches i, j at (y, x) of the window -> (y_i - y_j + wh - 1)(2 ww - 1) + (x_i - x_j + ww - 1); row 0 (CLS to
    token) n - 3, column 0 (token to CLS) n - 2, [0, 0] n - 1, n = (2 wh - 1)(2 ww - 1) + 3 table rows"""
    n = (2 * wh - 1) * (2 * ww - 1) + 3
    idx = np.empty((wh * ww + 1, wh * ww + 1), dtype=np.int64)
    for i in range(wh * ww):
        for j in range(wh * ww):
            idx[1 + i, 1 + j] = (i // ww - j // ww + wh - 1) * (2 * ww - 1) + (i % ww - j % ww + ww - 1)
    idx[0, :] = n - 3
    idx[:, 0] = n - 2
    idx[0, 0] = n - 1
    return idx


def bias_image(table, wh, ww, ld=None):
    """table [n, heads] -> [heads, P, ld]: the gather the engine's refresh kernel does, columns P .. ld-1 zero"""
    table = torch.as_tensor(table)
    P = wh * ww + 1
    ld = P if ld is None else ld
    idx = torch.from_numpy(relative_position_index(wh, ww))
    out = torch.zeros(table.shape[1], P, ld, dtype=table.dtype)
    out[:, :, :P] = table[idx.view(-1)].view(P, P, -1).permute(2, 0, 1)
    return out


# ---------------------------------------------------------------------------------------------------- parameters (4.25.1 checkpoint naming)
def vision_shapes(cfg):
    H, I, W = cfg.Hv, cfg.Iv, window(cfg)
    s = {VM + "embeddings.cls_token": (1, 1, H),
         VM + "embeddings.patch_embeddings.projection.weight": (H, 3, cfg.patch, cfg.patch),
         VM + "embeddings.patch_embeddings.projection.bias": (H,)}
    for l in range(cfg.layers_img):
        p = f"{VM}encoder.layer.{l}."
        s[p + "lambda_1"] = (H,)
        s[p + "lambda_2"] = (H,)
        s[p + "attention.attention.query.weight"] = (H, H)
        s[p + "attention.attention.query.bias"] = (H,)
        s[p + "attention.attention.key.weight"] = (H, H)
        s[p + "attention.attention.value.weight"] = (H, H)
        s[p + "attention.attention.value.bias"] = (H,)
        s[p + TABLE] = ((2 * W - 1) * (2 * W - 1) + 3, cfg.heads_v)
        s[p + "attention.output.dense.weight"] = (H, H)
        s[p + "attention.output.dense.bias"] = (H,)
        s[p + "intermediate.dense.weight"] = (I, H)
        s[p + "intermediate.dense.bias"] = (I,)
        s[p + "output.dense.weight"] = (H, I)
        s[p + "output.dense.bias"] = (H,)
        for n in ("layernorm_before", "layernorm_after"):
            s[p + n + ".weight"] = (H,)
            s[p + n + ".bias"] = (H,)
    s[VM + "pooler.layernorm.weight"] = (H,)
    s[VM + "pooler.layernorm.bias"] = (H,)
    return s


def param_shapes(cfg):
    s = {"dual_encoder.logit_scale": ()}
    s.update(vision_shapes(cfg))
    return O._param_shapes_text_heads(cfg, s)


def buffer_shapes(cfg):
    """the int64 buffers a 4.25.1 checkpoint carries beside the parameters"""
    P = window(cfg) ** 2 + 1
    return {f"{VM}encoder.layer.{l}.{INDEX}": (P, P) for l in range(cfg.layers_img)}


def make_params(cfg, seed=0):
    """the oracle's recipe (a value depends on name, shape and seed only), with the three kinds of BEiT parameter that HF initialises to a constant
    made non-trivial: lambda = 0.1 + 0.05 N(0, 1) (HF: 0.1), the bias tables 0.5 N(0, 1) (HF: zeros -- the bias would be invisible) and, as the
    oracle does for every LayerNorm, the pooler's 1 + 0.1 N(0, 1) / 0.02 N(0, 1)"""
    P = {}
    for k, shp in param_shapes(cfg).items():
        v = O.make_param(k, shp, seed)
        if k.endswith(".lambda_1") or k.endswith(".lambda_2"):
            v = 0.1 + 2.5 * v
        elif k.endswith("relative_position_bias_table"):
            v = 25.0 * v
        P[k] = v
    return P


# ---------------------------------------------------------------------------------------------------- stochastic depth: the engine's draws
def stream_droppath(layer, branch):
    return 0x1000 + 2 * layer + branch


def drop_path_p(rate, layer, layers):
    """linspace(0, rate, layers)[layer] as the engine computes it, in fp32"""
    if layers < 2 or rate <= 0:
        return np.float32(0.0)
    return np.float32(rate) * np.float32(layer) / np.float32(layers - 1)


def drop_threshold16(p):
    return min(int(np.rint(np.float32(p) * np.float32(65536.0))), 65535)


def droppath_keep(seed, layer, branch, posts, p):
    """-> (keep [posts] bool, scale): post b is kept when its 16 random bits reach round(p * 65536): the low half of rng_u32(b >> 1) for even b, the
    high half for odd b (csrc/mmhip_common.h mm_keep on element index b); a kept branch is multiplied by 1 / (1 - threshold / 65536) (fp32)"""
    t = drop_threshold16(p)
    e = np.arange(posts, dtype=np.uint32)
    h = O.rng_u32(e >> np.uint32(1), stream_droppath(layer, branch), seed)
    r = np.where((e & np.uint32(1)) == 1, h >> np.uint32(16), h & np.uint32(0xFFFF))
    scale = np.float32(1.0) / (np.float32(1.0) - np.float32(t) / np.float32(65536.0))
    return r >= np.uint32(t), float(scale)


# ---------------------------------------------------------------------------------------------------- the tower
def _lin_scaled(x, P, name, lam):
    """lam * Linear(x), the way the engine computes it: the layer scale folded into weight rows and bias in fp32, before the operand is rounded"""
    return F.linear(O._qo(x), O._qw(lam.unsqueeze(1) * P[name + ".weight"]), lam * P[name + ".bias"])


def beit_forward(P, pixels, cfg, drop_path=None, collect=None):
    """-> (last_hidden_state [B, P, H], pooler_output [B, H]).  drop_path = (rate, seed): train-mode stochastic depth with the engine's draws of the
    forward whose dropout seed is `seed`; None: eval mode / rate 0"""
    B, H, nh, L = pixels.shape[0], cfg.Hv, cfg.heads_v, cfg.layers_img
    W = window(cfg)
    x = F.conv2d(O._qo(pixels), O._qw(P[VM + "embeddings.patch_embeddings.projection.weight"]), P[VM + "embeddings.patch_embeddings.projection.bias"],
                 stride=cfg.patch).flatten(2).transpose(1, 2)
    x = O._q(torch.cat([P[VM + "embeddings.cls_token"].expand(B, -1, -1), O._q(x)], dim=1), "resid")          # no position embedding is added
    idx = torch.from_numpy(relative_position_index(W, W)).view(-1)
    scale = (H // nh) ** -0.5
    ident = lambda a: a

    def droppath(l, branch, o):
        if drop_path is None:
            return o
        p = drop_path_p(drop_path[0], l, L)
        if not p > 0:
            return o
        keep, ks = droppath_keep(drop_path[1], l, branch, B, p)
        return O._q(o) * (torch.from_numpy(keep).to(o.dtype) * ks).view(B, 1, 1)          # the branch is stored, then scaled per post

    for l in range(L):
        p = f"{VM}encoder.layer.{l}."
        h = O._q(O._ln(x, P, p + "layernorm_before", cfg.ln_eps_img), "ln")
        q = O._heads(O._q(O._lin(h, P, p + "attention.attention.query")), nh)
        k = O._heads(O._q(O._lin(h, P, p + "attention.attention.key")), nh)                 # no key bias
        v = O._heads(O._q(O._lin(h, P, p + "attention.attention.value")), nh)
        bias = P[p + TABLE][idx].view(W * W + 1, W * W + 1, nh).permute(2, 0, 1).unsqueeze(0)      # added AFTER the scaling
        c = O._q(O._attend(q, k, v, scale, bias, ident)).permute(0, 2, 1, 3).reshape(B, -1, H)
        x = O._q(x + droppath(l, 0, _lin_scaled(c, P, p + "attention.output.dense", P[p + "lambda_1"])), "resid")
        h = O._q(O._ln(x, P, p + "layernorm_after", cfg.ln_eps_img), "ln")
        h = O._q(O._gelu(O._lin(h, P, p + "intermediate.dense")))
        x = O._q(x + droppath(l, 1, _lin_scaled(h, P, p + "output.dense", P[p + "lambda_2"])), "resid")
        if collect is not None:
            collect.append(x)
    pooled = O._ln(x[:, 1:].mean(dim=1), P, VM + "pooler.layernorm", cfg.ln_eps_img)          # BeitPooler: no dense, no tanh
    return x, pooled


def mm_forward(P, ids, mask, pixels, cfg, tim_inputs=None, drop=None, relu_mask=None, drop_path=None, collect=None):
    """reference models/mm_late.py:148-193 with the BEiT tower -> (out_cls, logits_per_text, out_tim, None, mm_features)"""
    drop = drop or O.Dropout("none")
    B = ids.shape[0]
    x_v, v_pool = beit_forward(P, pixels, cfg, drop_path, collect)
    x_t, t_pool = O.text_forward(P, ids, mask, cfg, drop, 0, None)
    lpt = O.itc_logits(P, t_pool, v_pool)
    if cfg.fusion == "aspect-att":
        feats = A.fusion(t_pool, v_pool, P[A.ASPECT_W], P[A.ASPECT_B], relu_mask)[0]
    else:
        feats = O.mm_fusion(P, x_t, x_v, cfg, relu_mask)
    out_cls = O._lin32(drop(feats, cfg.p_head, O.STREAM_HEAD, 0), P, "linear_cls")
    out_tim = None
    if tim_inputs is not None:
        # the second text pass against the SAME image tokens: one set of stochastic-depth draws per step (the reference's second encoder call
        # draws again; identical when the rate is 0)
        x_t2, _ = O.text_forward(P, tim_inputs[0], tim_inputs[1], cfg, drop, B, None)
        out_tim = O._lin32(O.mm_fusion(P, x_t2, x_v, cfg), P, "linear_tim")
    return out_cls, lpt, out_tim, None, feats


def trainable(name, cfg, use_itc):
    if cfg.fusion == "aspect-att":
        return A.trainable(name, use_itc)
    return O.trainable(name)


def loss_and_grads(P, ids, mask, pixels, onehot, weight, cfg, use_itc, use_itm=False, tim=None, beta_itc=0.1, beta_itm=0.1, relu_mask=None, drop_path=None):
    """-> (out_cls, loss, mm_features, out_tim, {name: grad or None}); tim = (tim_ids, tim_mask, lbl_tim) with use_itm"""
    Pg = {k: v.clone().requires_grad_(trainable(k, cfg, use_itc)) for k, v in P.items()}
    out_cls, lpt, out_tim, _, feats = mm_forward(Pg, ids, mask, pixels, cfg, tim[:2] if use_itm else None, None, relu_mask, drop_path)
    loss = O.mix_loss(out_cls, onehot, weight, lpt, out_tim, tim[2] if use_itm else None, use_itc, use_itm, beta_itc, beta_itm)
    loss.backward()
    return out_cls.detach(), loss.detach(), feats.detach(), None if out_tim is None else out_tim.detach(), {k: v.grad for k, v in Pg.items()}


# ---------------------------------------------------------------------------------------------------- operators in fp64, with error bounds
U_32, SLACK = OB.U_32, OB.SLACK


def attn_bias_reference(qkv, bias, posts, S, heads):
    """fp64 softmax(q k^T / 8 + bias[h]) v on qkv [posts*S, 3*heads*64] (already rounded to what the kernel reads), bias [heads, S, S] -> OB.AttnRef"""
    x = qkv.double().view(posts, S, 3, heads, 64)
    q, k, v = (x[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(-1, -2) * 0.125 + bias.double().unsqueeze(0)
    lse = torch.logsumexp(s, dim=-1)
    p = torch.softmax(s, dim=-1)
    return OB.AttnRef(q, k, v, s, torch.ones_like(s, dtype=torch.bool), lse, p, p, torch.ones_like(p), p @ v, None, None, None, None)


def attn_bias_bounds(r, bias, dt, S):
    """op_bounds.attn_fwd_bounds with one more term in the score error: the bias joins the score by one fused multiply-add (bias * log2(e) + score,
    the constant rounded to fp32) -- 2 U_32 (|bias| + |s|).  Everything else is that function's: the q k^T product, the soft-max, P rounded to the
    operand type, the P V product, the stored result; the same overall factor."""
    fmt = OB.FMT[dt]
    e, m = OB._score_err(r, fmt)
    e = e + 2 * U_32 * (bias.double().abs().unsqueeze(0) + r.s.abs())
    E = e.amax(-1)
    av = r.a @ r.v.abs()
    ctx_b = SLACK * ((2 * E.unsqueeze(-1) + fmt.u_p + OB._acc(S) * U_32) * av + OB.split_err_w(fmt, r.a, r.v) + fmt.u_out * r.ctx.abs())
    lse_b = SLACK * (E + OB._acc(S) * U_32 + 4 * U_32 * (r.lse.abs() + m.abs()))
    return ctx_b, lse_b


def attn_bias_inputs(dt, posts, S, heads, seed, kind="random"):
    """qkv as fp64 values the kernel reads exactly, and a bias [heads, S, S] of the order of the scores (|q k^T| / 8 ~ 1 for unit-variance q, k):
    'random' N(0, 1.5) per element; 'asym' depends on (q - k) with opposite signs on the two sides of the diagonal, equal for all heads (its transpose
    is its negative); 'perhead' a constant per head times a fixed pattern (heads differ, so a bias read from another head is wrong everywhere)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    name = "x3" if dt in ("x3", "alu") else dt
    qkv = OB.rnd(torch.randn(posts * S, 3 * heads * 64, generator=g).double(), name)
    if kind == "random":
        bias = 1.5 * torch.randn(heads, S, S, generator=g)
    elif kind == "asym":
        d = (torch.arange(S)[:, None] - torch.arange(S)[None, :]).float()
        bias = (2.0 * torch.tanh(d / max(S / 4.0, 1.0)) + 0.5 * torch.sign(d)).unsqueeze(0).expand(heads, S, S).contiguous()
    else:
        pat = torch.randn(S, S, generator=g)
        bias = torch.stack([(1.0 + h) * (-1.0) ** h * pat for h in range(heads)])
    return qkv, bias.float()


def pad_bias(bias, ld):
    """[heads, S, S] -> [heads, S, ld] fp32, zero columns past S (what the kernel's clamped loads may read)"""
    heads, S, _ = bias.shape
    out = torch.zeros(heads, S, ld, dtype=torch.float32)
    out[:, :, :S] = bias
    return out


PM_SUM_DEPTH = 12          # roundings behind one of the LayerNorm's two sums: 3 adds in the thread, 6 shuffle steps, 2 adds across the four waves, 1 spare


def patch_mean_ln_reference(x, rows_per_post, gamma, beta, eps):
    """fp64 LayerNorm(mean over rows 1 .. rows_per_post-1 of each post's block) on x [posts*rows_per_post, W] (values the kernel reads) with the
    per-element bound of csrc/rowops.hip patch_mean_ln_kernel:
        m = mean of the R = rows_per_post - 1 patch rows, added in token order in fp32 and multiplied by 1 / R:  d m = (R + 2) U_32 mean|x|
        the LayerNorm of m (fp32 row of width W), n = PM_SUM_DEPTH roundings per sum, its input carrying d m:
            mean:  n U_32 mean|m| + mean(d m);   x - mean: d m + d mean;   var: 2 mean(|m - mean| d(x - mean)), rstd relative (n + 2) U_32 + d var rstd^2 / 2
            y:  |gamma| rstd d(x - mean) + |y - beta| (rel rstd + 3 U_32) + 2 U_32 |y|  [the add, the fp32 store],  times SLACK"""
    x, gamma, beta = x.double(), gamma.double(), beta.double()
    W = x.shape[-1]
    blk = x.view(-1, rows_per_post, W)[:, 1:]
    R = rows_per_post - 1
    m = blk.mean(1)
    d_m = (R + 2) * U_32 * blk.abs().mean(1)
    mean = m.mean(-1, keepdim=True)
    var = ((m - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (m - mean) * rstd * gamma + beta
    n = PM_SUM_DEPTH
    d_mean = n * U_32 * m.abs().mean(-1, keepdim=True) + d_m.mean(-1, keepdim=True)
    d_c = d_m + d_mean
    rel_rstd = (n + 2) * U_32 + ((m - mean).abs() * d_c).mean(-1, keepdim=True) * rstd ** 2
    bound = SLACK * (gamma.abs() * rstd * d_c + (y - beta).abs() * (rel_rstd + 3 * U_32) + 2 * U_32 * y.abs())
    return y, bound
