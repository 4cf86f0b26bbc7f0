"""fp32 restatement of the reference's late-fusion model under --fusion_name aspect-att (models/mm_late.py:115-131,148-166), composed from the
pinned oracle (oracle.mm_oracle is imported, not modified), and the fp64 reference of the fusion operator with its per-element error bounds.

    V   = cat(t_pool, v_pool, dim=0).reshape(B, 2, H)      # stack(dim=0) then reshape: a RESHAPE, not a transpose
    e   = tanh(V @ a^T + b);  w = softmax(e, dim=1);  mm_features = relu(sum_j w[:, j] * V[:, j])

Slot j of post n is row 2 n + j of the [2 B, H] matrix [t_pool; v_pool]: only B = 1 pairs a post's own text and image (at odd B post (B - 1) / 2
holds (t_pool[B - 1], v_pool[0])).  That is the reference's behaviour and the parity target; it is reproduced, not repaired."""
import numpy as np
import torch

from oracle import mm_oracle as O

ASPECT_W, ASPECT_B = "aspectattention.weight", "aspectattention.bias"
# parameters that no aspect-att forward reads: grad None in the reference (with ITC; without it the two projections and logit_scale join them)
UNUSED = ("linear_fusion.", "fc_Q.", "fc_K.", "fc_V.", "linear_gmu_t.", "linear_gmu_v.", "linear_iadds.", "linear_tim.")
ITC_ONLY = ("dual_encoder.logit_scale", "dual_encoder.visual_projection.weight", "dual_encoder.text_projection.weight")


def fusion(t_pool, v_pool, a, b, relu_mask=None, keep=None):
    """-> (mm_features [B, H], w [B, 2], e [B, 2]); relu_mask as O._relu's; keep (a dict): the pre-tanh tensor is left in keep["pre"] with its
    gradient retained (d b is the sum of that gradient's elements)"""
    B, H = t_pool.shape
    V = torch.cat((t_pool, v_pool), dim=0).reshape(B, 2, H)
    pre = V @ a.reshape(-1) + b.reshape(())
    if keep is not None:
        keep["pre"] = pre
        if pre.requires_grad:
            pre.retain_grad()
    e = torch.tanh(pre)
    w = torch.softmax(e, dim=1)
    return O._relu((w.unsqueeze(-1) * V).sum(dim=1), relu_mask), w, e


def trainable(name, use_itc):
    """gets a gradient in the reference (the frozen image tower aside)"""
    if "vision_model" in name or name.startswith(UNUSED):
        return False
    return use_itc or name not in ITC_ONLY


def forward(P, ids, mask, pixels, cfg, drop=None, relu_mask=None, keep=None):
    """reference models/mm_late.py:148-166 under aspect-att -> (out_cls, logits_per_text, mm_features, w)"""
    drop = drop or O.Dropout("none")
    _, v_pool = O.vit_forward(P, pixels, cfg, None)
    _, t_pool = O.text_forward(P, ids, mask, cfg, drop, 0, None)
    lpt = O.itc_logits(P, t_pool, v_pool)
    feats, w, _ = fusion(t_pool, v_pool, P[ASPECT_W], P[ASPECT_B], relu_mask, keep)
    out_cls = O._lin32(drop(feats, cfg.p_head, O.STREAM_HEAD, 0), P, "linear_cls")
    return out_cls, lpt, feats, w


def loss_and_grads(P, ids, mask, pixels, onehot, weight, cfg, use_itc, beta_itc=0.1, drop=None, relu_mask=None, keep=None):
    Pg = {k: v.clone().requires_grad_(trainable(k, use_itc)) for k, v in P.items()}
    out_cls, lpt, feats, _ = forward(Pg, ids, mask, pixels, cfg, drop, relu_mask, keep)
    loss = O.mix_loss(out_cls, onehot, weight, lpt, None, None, use_itc, False, beta_itc)
    loss.backward()
    return out_cls.detach(), loss.detach(), feats.detach(), {k: v.grad for k, v in Pg.items()}


# ---------------------------------------------------------------------------------------------------- the operator in fp64, with error bounds
U = 2.0 ** -24          # fp32 unit roundoff
# documented maximum errors of the device library's single-precision functions the kernel calls (HIP math API): tanhf 2 ulp, expf 1 ulp; an
# ulp is 2 u relative
TANH_ULP, EXP_ULP = 2, 1


def op_reference(t_pool, v_pool, a, b, d_feats=None, d_tpool0=None, relu_mask=None):
    """fp64 numpy of csrc/heads.hip aspect_fusion_fwd / _bwd from fp32 inputs.  -> dict with feats, w, e, pre (pre-tanh), mix (pre-relu) and, with
    d_feats, d_tpool (added onto d_tpool0 when given), da, db and the intermediates the bounds need.  relu_mask [B, H] (0/1): the units that pass in the
    backward instead of mix > 0 (the kernel's own pattern, which may differ where |mix| is within the forward's error: op_bounds' relu_unsafe)"""
    t, v, a, b = (np.asarray(x, dtype=np.float64) for x in (t_pool, v_pool, a, b))
    B, H = t.shape
    V = np.concatenate([t, v], axis=0).reshape(B, 2, H)
    a = a.reshape(H)
    pre = V @ a + b.reshape(())
    e = np.tanh(pre)
    p = np.exp(e - e.max(axis=1, keepdims=True))
    w = p / p.sum(axis=1, keepdims=True)
    mix = (w[:, :, None] * V).sum(axis=1)
    r = dict(V=V, b=float(b.reshape(())), pre=pre, e=e, w=w, mix=mix, feats=np.maximum(mix, 0.0))
    if d_feats is None:
        return r
    g = np.asarray(d_feats, dtype=np.float64) * ((mix > 0) if relu_mask is None else np.asarray(relu_mask, dtype=np.float64))
    dw = np.einsum("nh,njh->nj", g, V)
    ds = w * (dw - (w * dw).sum(axis=1, keepdims=True))
    dpre = ds * (1.0 - e * e)
    dV = w[:, :, None] * g[:, None, :] + dpre[:, :, None] * a[None, None, :]
    d_t = dV.reshape(2 * B, H)[:B].copy()
    if d_tpool0 is not None:
        d_t += np.asarray(d_tpool0, dtype=np.float64)
    r.update(g=g, dw=dw, ds=ds, dpre=dpre, d_tpool=d_t, da=np.einsum("nj,njh->h", dpre, V), db=dpre.sum())
    return r


def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error constant of n fp32 roundings"""
    return n * U / (1.0 - n * U)


def dot_depth(H):
    """roundings a term of a length-H dot passes through in the kernel: one wave per row, a lane chains its H / 64 fmas, six shuffle steps add the lanes"""
    return H // 64 + 6


def op_bounds(r, a, d_feats=None, d_tpool0=None):
    """per-element absolute bounds on |kernel - op_reference| for a kernel that works in fp32 with correctly rounded + - * / fma, sums a dot of
    length H as dot_depth says (gamma_depth times the magnitude sum), and calls tanhf / expf within their documented ulp.  First-order propagation; every constant is a rounding
    count of the formula it stands beside, doubled once (the factor 2 below) to cover the second-order terms.  -> dict of arrays shaped like
    the outputs.  Elements whose ReLU decision the forward error can flip are reported in `relu_unsafe` (the caller excludes them)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1)
    V, pre, e, w = r["V"], r["pre"], r["e"], r["w"]
    B, _, H = V.shape
    # pre_j = sum_h V_jh a_h + b: a dot of H terms and one addition
    d_pre = gamma(dot_depth(H) + 1) * ((np.abs(V) * np.abs(a)).sum(axis=2) + abs(r["b"]))
    # e = tanh(pre): |tanh'| <= 1 - e^2, plus tanhf's own error
    d_e = (1.0 - e * e) * d_pre + TANH_ULP * 2 * U * np.abs(e) + U * np.abs(e)
    # w_j = p_j / (p_0 + p_1), p = exp(e - max): d w_0 = w_0 w_1 (d e_0 - d e_1) to first order; exp, the subtraction, the sum and the division
    # add (EXP_ULP * 2 + 1 + 1 + 1) u relative to each p and w
    d_w = (w[:, 0] * w[:, 1])[:, None] * (d_e.sum(axis=1, keepdims=True) + 2 * U * np.abs(e).sum(axis=1, keepdims=True)) + (2 * EXP_ULP + 3) * 2 * U * w
    # mix = w_0 V_0 + w_1 V_1: one product, one fma
    d_mix = (d_w[:, :, None] * np.abs(V)).sum(axis=1) + gamma(2) * (w[:, :, None] * np.abs(V)).sum(axis=1)
    out = dict(e=2 * d_e, w=2 * d_w, feats=2 * d_mix, relu_unsafe=np.abs(r["mix"]) <= 2 * d_mix)
    if d_feats is None:
        return out
    g, dw, dpre = np.abs(r["g"]), r["dw"], r["dpre"]
    # dw_0 - dw_1 = g . V_0 - g . V_1: two dots of H terms and a subtraction
    d_dd = gamma(dot_depth(H) + 1) * (g[:, None, :] * np.abs(V)).sum(axis=(1, 2))
    dd = np.abs(dw[:, 0] - dw[:, 1])
    # ds_0 = w_0 w_1 (dw_0 - dw_1) = -ds_1: two products; the weights' own errors
    ww = w[:, 0] * w[:, 1]
    d_ds = ww * d_dd + (d_w[:, 0] * w[:, 1] + w[:, 0] * d_w[:, 1]) * dd + gamma(2) * ww * dd
    # dpre_j = ds_j (1 - e_j^2): a product, a subtraction, a product; d(1 - e^2) = 2 |e| d e
    om = 1.0 - e * e
    d_dpre = d_ds[:, None] * om + np.abs(r["ds"]) * (2 * np.abs(e) * d_e + gamma(2) * (1.0 + e * e)) + gamma(1) * np.abs(dpre)
    # dV_j = w_j g + dpre_j a: a product and an fma
    d_dV = d_w[:, :, None] * g[:, None, :] + d_dpre[:, :, None] * np.abs(a)[None, None, :] + \
        gamma(2) * (w[:, :, None] * g[:, None, :] + np.abs(dpre)[:, :, None] * np.abs(a)[None, None, :])
    d_t = d_dV.reshape(2 * B, H)[:B]
    if d_tpool0 is not None:          # one more addition
        d_t = d_t + U * (np.abs(r["d_tpool"]) + np.abs(np.asarray(d_tpool0, dtype=np.float64)))
    # d a = sum over 2 B rows of dpre V (a product and an fma per post, then B - 1 additions in some order), d b = sum of 2 B terms
    d_da = (d_dpre[:, :, None] * np.abs(V)).sum(axis=(0, 1)) + gamma(B + 2) * (np.abs(dpre)[:, :, None] * np.abs(V)).sum(axis=(0, 1))
    d_db = d_dpre.sum() + gamma(2 * B) * np.abs(dpre).sum()
    out.update(d_tpool=2 * d_t, da=2 * d_da, db=2 * d_db)
    return out
