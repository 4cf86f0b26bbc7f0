"""fp64 references of the text-embedding operators (include/mmhip.h mmhip_op_embed_fwd / mmhip_op_embed_bwd; csrc/rowops.hip pos_ids_kernel,
embed_fwd_kernel, embed_bwd_kernel, embed_scatter_det_kernel), the per-element bounds the op tests hold the kernels to, an fp32 emulation of the
kernels' arithmetic order and a set of deliberately wrong variants (pure torch on the CPU: tests/test_embed_bounds_cpu.py checks the bounds
themselves, tests/test_gpu_ops_embed.py the kernels against them).

Bounds are written in the manner of tests/op_bounds.py: sums of named terms read off the kernels' rounding points, from U_BF16, U_F16, U_32, U_PAIR
and the one factor SLACK = 2 (rsqrtf, the fused multiply-adds the compiler may or may not form).  Nothing is fitted to what a kernel returns.
One wave sum over a row of width H is n(H) = 4 ceil(H / 256) + 6 fp32 additions deep (a lane's own elements, then six shuffle steps), as in
op_bounds.ln_bounds.

Forward (one wave per row; v = (word[id] + type[tt]) + pos[pid] in fp32, then LayerNorm, then dropout):
    d v      = 2 U_32 (|word| + |type| + |pos|)                         [two additions]
    d mean   = n U_32 mean|v| + mean(d v) + U_32 |mean|                 [wave sum, division]
    d (v-m)  = d v + d mean + U_32 |v - mean|
    rel rstd = (d var) / (2 (var + eps)) + 3 U_32,  d var = (n + 2) U_32 var + 2 mean(|v - mean| d (v-m))      [squares, wave sum, division; eps add,
                                                                                                                rsqrt, store]
    xhat     : rstd d (v-m) + |xhat| (rel rstd + U_32)   + u_out |xhat|  [stored in the activation type]
    x        : ((|gamma| d xhat + U_32 |xhat gamma| + 2 U_32 |y|) keep scale) + u_out |x|;  a dropped element has bound 0: exactly 0 is required
    x_pair   : the x bound + U_PAIR |x|, and op_bounds.pair_hi_is_nearest must hold
    pos_ids, maskbias: exact (bound 0).

Backward (block (t, 16 posts), one wave per row at a time).  dy = dx keep scale, g = dy gamma, c1 = mean(g), c2 = mean(g xhat),
d = rstd (g - c1 - xhat c2), and a slot's contribution to its table rows is c = alpha d:
    e_d = rstd (4 U_32 |g| + (n + 3) U_32 mean|g| + |xhat| (n + 4) U_32 mean|g xhat| + 3 U_32 (|c1| + |xhat c2|)) + U_32 |d|
    e_c = |alpha| e_d + U_32 |c|
Every table element is a sum, in an order nobody fixes (fp32 atomics; wave, block and partial sums in between), of its prefill and its k
contributions: each of the k additions rounds a running sum no larger than |prefill| + sum |c|, so
    dword[r]  : sum e_c + k U_32 (|prefill| + sum |c|)
    dpos[r]   : the same with k + 1 (posts of one wave that share the position id are summed BEFORE alpha multiplies: one more rounding)
    dtype[r]  : the same with k + 2 (sums of d over the block, alpha once per block or once after the partial reduction)
    dgamma    : terms alpha dy xhat (2 U_32 each: the dropout scale, the product), rows + 2 additions;   dbeta: terms alpha dy (U_32 each) alike
all times SLACK.  A row with k = 0 -- a row no slot names, the padding_idx row of the word table (and of the position table under XLM-R), row 0 of
dtype in the one-row mode, row 1 without type ids -- has bound 0: it must keep its prefill to the bit.  det_rows[slot] = c within SLACK e_c.
row_state, status: exact.

What accumulates and what overwrites (the kernels' comments; embed_backward in csrc/engine.hip and its twin in csrc/early.hip add the step's gradient
into a buffer that an earlier stage may already have written): dword, dpos, dtype, dgamma, dbeta are ADDED to; row_state is OR-ed; status is
added to / OR-ed; det_rows and partial are overwritten; every forward output is overwritten.  The tests prefill accordingly."""
from types import SimpleNamespace

import torch

from op_bounds import FMT, SLACK, U_32, U_PAIR, rnd, split_pair

STREAM_EMBED = 1                      # csrc/mmhip_host.h STREAM_EMBED, oracle/mm_oracle.py STREAM_EMBED
LAYOUTS = ("right", "left", "middle", "allpad", "none")
TT_MODES = ("none", "one", "two")     # no type ids | type ids, one-row gradient (type_rows != 2) | type ids, type_rows == 2
EPS = 1e-5


def nsum(H):
    return 4 * ((H + 255) // 256) + 6


# (posts, T, H): one lane active | second wave with one post, first chunk group partly filled | a full block | second block row with one post, pos_ids
# loops twice | pos_ids loops three times, pads across slot 64 | all four chunk groups, LDS rows full
SHAPES = [(1, 1, 4), (5, 3, 132), (16, 7, 768), (17, 65, 768), (33, 130, 256), (4, 5, 1024)]
# (layout, xlmr, small vocabulary, type mode, p, alpha, partial): every layout under XLM-R and under BERT; the other axes cycle so that each value of
# each meets both values of the others somewhere (type_rows == 2 with and without partial, dropout with and without alpha, ...)
VARIANTS = [("right", 1, True, "none", 0.1, 0.37, True), ("left", 1, False, "one", 0.0, 0.0, False), ("middle", 1, True, "two", 0.1, 0.37, False),
            ("allpad", 1, False, "none", 0.0, 0.37, True), ("none", 1, True, "one", 0.1, 0.0, True), ("right", 0, False, "two", 0.0, 0.0, True),
            ("left", 0, True, "none", 0.1, 0.0, False), ("middle", 0, False, "one", 0.1, 0.37, True), ("allpad", 0, True, "two", 0.0, 0.37, False),
            ("none", 0, False, "none", 0.1, 0.0, False)]
SMALL_VOCAB = 37          # far fewer rows than slots: every row collides
DROP_SEED = 0x1234567


def case_of(shape, k):
    """the case of shape x variant k, with its dropout / alpha / partial settings attached; vocabulary 37, or the slot count + 101 (most rows unnamed)"""
    layout, xlmr, small, tt, p, alpha, partial = VARIANTS[k]
    posts, T, H = shape
    c = make_case(posts, T, H, SMALL_VOCAB if small else posts * T + 101, layout, xlmr, tt, seed=k)
    c.p, c.alpha, c.partial, c.seed = p, alpha, partial, DROP_SEED + k
    return c


def make_case(posts, T, H, vocab, layout, xlmr, tt, seed=0):
    """ids / mask / type ids, the three tables, gamma, beta, a raw incoming gradient and the prefill of every accumulated output.  The pad id is 1 under
    XLM-R and 0 under BERT; live tokens never carry it.  Layouts: right- / left-padded (lengths drawn, post 0 full), pads in the middle (30 % of
    the slots, one forced into the middle of post 0 and a run across slot 64 of post 1), right-padded with post posts // 2 all pads, no pads."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * posts + 3 * T + H + vocab)
    pad = 1 if xlmr else 0
    ids = torch.randint(0, vocab - 1, (posts, T), generator=g)
    ids = ids + (ids >= pad).long()
    t = torch.arange(T)[None, :]
    lens = torch.randint(1, T + 1, (posts,), generator=g)
    lens[0] = T
    if layout in ("right", "allpad"):
        dead = t >= lens[:, None]
        if layout == "allpad":
            dead[posts // 2] = True
    elif layout == "left":
        dead = t < (T - lens)[:, None]
    elif layout == "middle":
        dead = torch.rand(posts, T, generator=g) < 0.3
        if T >= 3:
            dead[0, 0], dead[0, T // 2], dead[0, T - 1] = False, True, False
        if posts > 1 and T > 66:
            dead[1, 62:66] = True
    else:
        dead = torch.zeros(posts, T, dtype=torch.bool)
    ids = torch.where(dead, torch.full_like(ids, pad), ids)
    c = SimpleNamespace(posts=posts, T=T, H=H, vocab=vocab, layout=layout, xlmr=int(xlmr), tt=tt, pad=pad, pos_pad=pad if xlmr else -1,
                        rows=posts * T, max_pos=T + pad + 2, ids=ids, mask=(ids != pad).long())
    c.type_ids = None if tt == "none" else torch.randint(0, 2, (posts, T), generator=g)
    r = lambda *s: torch.randn(*s, generator=g)
    c.word, c.pos, c.type = 0.5 * r(vocab, H), 0.5 * r(c.max_pos, H), 0.5 * r(2, H)
    c.gamma, c.beta = 1 + 0.1 * r(H), 0.1 * r(H)
    c.dx_raw = r(c.rows, H)
    c.pre = dict(dword=0.1 * r(vocab, H), dpos=0.1 * r(c.max_pos, H), dtype=0.1 * r(2, H), dgamma=0.1 * r(H), dbeta=0.1 * r(H))
    return c


def keep_of(c, p, seed):
    """(keep, scale) of the embedding dropout: the kernels' hash over the row-major [rows, H] tensor, stream 1"""
    if p == 0:
        return torch.ones(c.rows, c.H, dtype=torch.bool), 1.0
    from gpu_util import keep_mask
    return keep_mask((c.rows, c.H), STREAM_EMBED, seed, p)


# ---------------------------------------------------------------------------------------------------------------- forward
def pos_ids_reference(c, mutant=None):
    live = c.ids != c.pad
    if not c.xlmr:
        return torch.arange(c.T)[None, :].expand(c.posts, c.T).contiguous()
    counted = torch.ones_like(live) if mutant == "pos_no_skip" else live          # the mutant counts the pads it passes
    return torch.cumsum(counted.long(), 1) * live.long() + c.pad


def fwd_reference(c, p=0.0, seed=0, mutant=None):
    """fp64 forward on the fp32 tables.  mutant: "pos_no_skip" (XLM-R position ids do not skip a pad inside a post), "type_row0" (row 0 of the type
    table where the id says 1)"""
    pid = pos_ids_reference(c, mutant)
    tt = torch.zeros_like(c.ids) if (c.type_ids is None or mutant == "type_row0") else c.type_ids
    w, ty, po = c.word.double()[c.ids.reshape(-1)], c.type.double()[tt.reshape(-1)], c.pos.double()[pid.reshape(-1)]
    v = w + ty + po
    mean = v.mean(-1, keepdim=True)
    var = ((v - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (v - mean) * rstd
    y = xhat * c.gamma.double() + c.beta.double()
    keep, scale = keep_of(c, p, seed)
    ks = keep.double() * scale
    maskbias = torch.where(c.mask.reshape(-1) != 0, 0.0, float("-inf")).double()
    return SimpleNamespace(pos_ids=pid.reshape(-1), maskbias=maskbias, v=v, mean=mean, var=var, rstd=rstd.squeeze(-1), xhat=xhat, y=y, x=y * ks, ks=ks,
                           mag=w.abs() + ty.abs() + po.abs())


def fwd_bounds(c, r, dt):
    """bounds of xhat, rstd, x (and x_pair for the fp32 form) as derived in the module docstring"""
    u_out, n, H = FMT[dt].u_out, nsum(c.H), c.H
    dv = 2 * U_32 * r.mag
    d_mean = n * U_32 * r.v.abs().mean(-1, keepdim=True) + dv.mean(-1, keepdim=True) + U_32 * r.mean.abs()
    dev = (r.v - r.mean).abs()
    d_dev = dv + d_mean + U_32 * dev
    d_var = (n + 2) * U_32 * r.var + 2 * (dev * d_dev).mean(-1, keepdim=True)
    rel = d_var / (2 * (r.var + EPS)) + 3 * U_32
    rstd = r.rstd.unsqueeze(-1)
    e_xhat = rstd * d_dev + r.xhat.abs() * (rel + U_32)
    e_x = (c.gamma.double().abs() * e_xhat + U_32 * (r.xhat * c.gamma.double()).abs() + 2 * U_32 * r.y.abs()) * r.ks
    b = dict(xhat=SLACK * (e_xhat + u_out * r.xhat.abs()), rstd=SLACK * (rel + U_32).squeeze(-1) * r.rstd, x=SLACK * (e_x + u_out * r.x.abs()))
    b["x_pair"] = b["x"] + SLACK * U_PAIR * r.x.abs()
    return b


def emulate_fwd(c, p, seed, dt):
    """the kernels' order in fp32: a running count of the live tokens for the position ids; (word + type) + pos, mean, the squared differences from
    it, rsqrt, xhat, xhat gamma + beta, keep * scale; xhat and x rounded as stored.  Returns pos_ids, maskbias, xhat, rstd, x, (hi, lo)."""
    pid = torch.empty(c.posts, c.T, dtype=torch.long)
    for post in range(c.posts):
        running = 0
        for t in range(c.T):
            nz = int(c.ids[post, t]) != c.pad
            running += nz
            pid[post, t] = (running + c.pad if nz else c.pad) if c.xlmr else t
    tt = torch.zeros_like(c.ids) if c.type_ids is None else c.type_ids
    v = (c.word[c.ids.reshape(-1)] + c.type[tt.reshape(-1)]) + c.pos[pid.reshape(-1)]
    mean = v.sum(-1, keepdim=True) / c.H
    d = v - mean
    rstd = torch.rsqrt((d * d).sum(-1, keepdim=True) / c.H + torch.tensor(EPS, dtype=torch.float32))
    xh = d * rstd
    o = xh * c.gamma + c.beta
    keep, scale = keep_of(c, p, seed)
    if p:
        o = torch.where(keep, o * torch.tensor(scale, dtype=torch.float32), torch.zeros_like(o))
    maskbias = torch.where(c.mask.reshape(-1) != 0, 0.0, float("-inf"))
    return pid.reshape(-1), maskbias, rnd(xh.double(), dt), rstd.squeeze(-1), rnd(o.double(), dt), split_pair(o)


# ---------------------------------------------------------------------------------------------------------------- backward
def bwd_inputs(c, fr, dt):
    """what the backward kernel reads: dx and the forward's xhat in the activation type, rstd as fp32 (all as fp64 values)"""
    name = "x3" if dt == "x3" else dt
    return SimpleNamespace(dx=rnd(c.dx_raw.double(), name), xhat=rnd(fr.xhat, name), rstd=fr.rstd.float().double(), pos_ids=fr.pos_ids)


def _alpha(alpha):
    return 1.0 if alpha == 0 else float(torch.tensor(alpha, dtype=torch.float32))


def _type_index(c, mutant=None):
    """(table row, contributes) per slot for the three type modes"""
    rows = c.rows
    if c.tt == "none":
        return torch.zeros(rows, dtype=torch.long), torch.ones(rows, dtype=torch.bool)
    t = c.type_ids.reshape(-1)
    if mutant == "type0_into_row1":
        return torch.ones(rows, dtype=torch.long), torch.ones(rows, dtype=torch.bool)
    return t, (t == 1) if c.tt == "one" else torch.ones(rows, dtype=torch.bool)


def bwd_reference(c, bi, keep, scale, alpha, mutant=None, with_bounds=True):
    """fp64 closed form on exactly what the kernel reads, by explicit index-add onto the prefill; (reference dict, bound dict).  mutants:
    "drop_word_slot" (the last live slot does not reach its word row), "pad_row" (pad slots add to the padding_idx row), "keep_shift" (the keep mask
    one element late), "type0_into_row1", "alpha_twice_pos", "dbeta_raw" (dbeta from dx before the dropout mask and scale)"""
    H, U = c.H, U_32
    al = _alpha(alpha)
    ks = keep.double() * scale
    if mutant == "keep_shift":
        ks = torch.roll(ks.reshape(-1), 1).reshape(ks.shape)
    gam = c.gamma.double()
    dy = bi.dx * ks
    g = dy * gam
    xh, rstd = bi.xhat, bi.rstd.unsqueeze(-1)
    c1, c2 = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    d = rstd * (g - c1 - xh * c2)
    con = al * d
    n = nsum(H)
    e_d = rstd * (4 * U * g.abs() + (n + 3) * U * g.abs().mean(-1, keepdim=True) + xh.abs() * (n + 4) * U * (g * xh).abs().mean(-1, keepdim=True)
                  + 3 * U * (c1.abs() + (xh * c2).abs())) + U * d.abs()
    e_c = abs(al) * e_d + U * con.abs()
    ids, pid = c.ids.reshape(-1), bi.pos_ids

    def scatter(pre, idx, sel, vals, extra):
        """pre + index-add of vals[sel] at idx[sel]; bound SLACK (sum e_c + (k + extra) U_32 (|pre| + sum |vals|)), 0 where k = 0"""
        pre = pre.double()
        R = pre.shape[0]
        ref = pre.clone().index_add_(0, idx[sel], vals[sel])
        if not with_bounds:
            return ref, None
        mag = pre.abs().index_add_(0, idx[sel], vals[sel].abs())
        err = torch.zeros_like(pre).index_add_(0, idx[sel], e_c[sel])
        k = torch.bincount(idx[sel], minlength=R).double().unsqueeze(-1)
        return ref, torch.where(k > 0, SLACK * (err + (k + extra) * U * mag), torch.zeros_like(mag))

    ref, b = {}, {}
    wsel = ids != c.pad
    if mutant == "pad_row":
        wsel = torch.ones_like(wsel)
    if mutant == "drop_word_slot":
        wsel = wsel.clone()
        wsel[int(wsel.nonzero().max())] = False
    ref["dword"], b["dword"] = scatter(c.pre["dword"], ids, wsel, con, 0)
    psel = pid != c.pos_pad
    ref["dpos"], b["dpos"] = scatter(c.pre["dpos"], pid, psel, con * (al if mutant == "alpha_twice_pos" else 1.0), 1)
    trow, tsel = _type_index(c, mutant)
    ref["dtype"], b["dtype"] = scatter(c.pre["dtype"], trow, tsel, con, 2)
    for name, term, e in (("dgamma", al * dy * xh, 2 * U), ("dbeta", al * (bi.dx if mutant == "dbeta_raw" else dy), U)):
        pre = c.pre[name].double()
        ref[name] = pre + term.sum(0)
        b[name] = SLACK * (e * term.abs().sum(0) + (c.rows + 2) * U * (pre.abs() + term.abs().sum(0)))
    ref["det_rows"], b["det_rows"] = con, SLACK * e_c
    return ref, (b if with_bounds else None)


def row_state_reference(c, pre):
    """bit 0 of byte id set for exactly the ids that occur, the pad id excepted; every other bit and byte as prefilled (pre: uint8 [>= vocab])"""
    out = pre.clone()
    seen = torch.unique(c.ids[c.ids != c.pad])
    out[seen] |= 1
    return out


def emulate_bwd(c, bi, keep, scale, alpha, perm_seed=0, deterministic=False):
    """embed_bwd_kernel's arithmetic in fp32, block by block: wave-sequential sums of four posts, the four waves added, alpha after the sum; the
    position rows merged over the posts and waves that share an id, direct adds otherwise; word rows (and the direct position adds) land in a random
    permutation of the slot order, as atomics may.  deterministic: the two-kernel form (rows stored, summed in slot order from 0, then added)."""
    f = torch.float32
    H, T, posts = c.H, c.T, c.posts
    al = torch.tensor(_alpha(alpha), dtype=f)
    dv = bi.dx.to(f)
    if scale != 1.0:
        dv = torch.where(keep, dv * torch.tensor(scale, dtype=f), torch.zeros_like(dv))
    xh, rstd, gam = bi.xhat.to(f), bi.rstd.to(f).unsqueeze(-1), c.gamma.to(f)
    g = dv * gam
    c1, c2 = g.sum(-1, keepdim=True) / H, (g * xh).sum(-1, keepdim=True) / H
    o = rstd * (g - c1 - xh * c2)
    ov = o * al
    out = {k: v.clone().to(f) for k, v in c.pre.items()}
    ids, pid = c.ids.reshape(-1), bi.pos_ids
    tts = None if c.type_ids is None else c.type_ids.reshape(-1)
    toks = torch.arange(T)
    late = {"dword": [], "dpos": []}                # slots whose row takes a direct atomic: the order nobody fixes
    zero = torch.zeros((), dtype=f)
    for blk in range((posts + 15) // 16):           # every token slot of the block row at once: tensors [T, H]
        ws = {k: [torch.zeros(T, H, dtype=f) for _ in range(4)] for k in ("dg", "db", "dt", "dt0", "pacc")}
        wpid = [torch.full((T,), -1, dtype=torch.long) for _ in range(4)]
        for w in range(4):
            for post in range(blk * 16 + 4 * w, min(blk * 16 + 4 * w + 4, posts)):
                sl = slice(post * T, (post + 1) * T)
                ws["dg"][w] = ws["dg"][w] + dv[sl] * xh[sl]
                ws["db"][w] = ws["db"][w] + dv[sl]
                t1 = (torch.ones(T, dtype=torch.bool) if tts is None else tts[sl] == 1)[:, None]
                ws["dt"][w] = ws["dt"][w] + torch.where(t1, o[sl], zero)          # (adding 0 is exact)
                ws["dt0"][w] = ws["dt0"][w] + torch.where(~t1, o[sl], zero)
                on = pid[sl] != c.pos_pad
                wpid[w] = torch.where(on & (wpid[w] < 0), pid[sl], wpid[w])
                reg = on & (pid[sl] == wpid[w])
                ws["pacc"][w] = ws["pacc"][w] + torch.where(reg[:, None], o[sl], zero)
                late["dpos"].append((post * T + toks)[on & ~reg])
                late["dword"].append((post * T + toks)[ids[sl] != c.pad])
        tot = {k: (((ws[k][0] + ws[k][1]) + ws[k][2]) + ws[k][3]) * al for k in ("dg", "db", "dt", "dt0")}
        for t in range(T):                          # one atomic per block and column
            out["dgamma"] += tot["dg"][t]
            out["dbeta"] += tot["db"][t]
            out["dtype"][0 if tts is None else 1] += tot["dt"][t]
            if c.tt == "two":
                out["dtype"][0] += tot["dt0"][t]
        if not deterministic:
            for i in range(4):                      # waves that share a position id leave as one add; the first such wave owns it
                owner = wpid[i] >= 0
                for j in range(i):
                    owner = owner & (wpid[j] != wpid[i])
                sp = ws["pacc"][i] * al
                for j in range(i + 1, 4):
                    sp = sp + torch.where((wpid[j] == wpid[i])[:, None], ws["pacc"][j] * al, zero)
                out["dpos"].index_add_(0, wpid[i][owner], sp[owner])
    if deterministic:
        for name, idx, padv in (("dword", ids, c.pad), ("dpos", pid, c.pos_pad)):
            for r_ in torch.unique(idx).tolist():
                if r_ == padv:
                    continue
                acc = torch.zeros(H, dtype=f)
                for s in (idx == r_).nonzero().flatten().tolist():
                    acc = acc + ov[s]
                out[name][r_] += acc
    else:
        gen = torch.Generator().manual_seed(perm_seed)
        for name, idx in (("dword", ids), ("dpos", pid)):
            slots = torch.cat(late[name]) if late[name] else torch.zeros(0, dtype=torch.long)
            slots = slots[torch.randperm(len(slots), generator=gen)]
            out[name].index_add_(0, idx[slots], ov[slots])          # (one row after the other, in this order)
    out["det_rows"] = ov
    return out
