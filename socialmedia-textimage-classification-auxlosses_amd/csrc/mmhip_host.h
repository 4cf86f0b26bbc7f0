// Host-side launch vocabulary shared by the two engines (engine.hip, early.hip) and the operator entry points (capi_ops.hip): how the launcher
// argument structs of mmhip_kernels.h are filled.  Every convention -- the dropout threshold, the GEMM epilogue flags, the plane-pair strides of the
// parity mode, the attention scale -- is written here once.  Host code only: no kernels, nothing that knows an engine struct; everything inline.
#pragma once
#include <cmath>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>
#include <cstring>
#include "mmhip_kernels.h"
#include "../../include/mmhip.h"

#define CHECK_HIP(expr)                       \
    do {                                      \
        hipError_t _e = (expr);               \
        if (_e != hipSuccess) return (int)_e; \
    } while (0)
#define CHECK_RC(expr)          \
    do {                        \
        int _r = (expr);        \
        if (_r) return _r;      \
    } while (0)

namespace mmhip {

// integer environment switch: atoi of the variable, `dflt` when it is unset.  Reads the environment on every call: whether a value is kept (a
// function-level static, an engine field) or read again per call is the caller's choice
inline int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }

// ------------------------------------------------------------------------------------------------ dropout
// Drop when an element's 16 random bits < thresh16 = round(p * 65536), at most 65535; `on` = false (eval mode) or p = 0 turn it off (thresh16 = 0,
// keep_scale = 1).  The oracle replays the masks, so this is the one place the threshold is computed: for every p >= 0 -- every value a caller can
// validly pass -- it equals the three copies it replaces (the late engine's, which tested `on` only; the early engine's; the op entry points', which
// tested p > 0 only).
inline DropCfg make_drop(float p, uint64_t seed, uint32_t stream, bool on = true) {
    DropCfg d;
    d.seed = seed;
    d.stream = stream;
    uint32_t t = (on && p > 0.f) ? (uint32_t)lrintf(p * 65536.0f) : 0u;
    if (t > 65535u) t = 65535u;
    d.thresh16 = t;
    d.keep_scale = 1.0f / (1.0f - (float)t / 65536.0f);
    return d;
}

// dropout streams every engine shares (oracle/mm_oracle.py STREAM_*); the per-layer ones are each engine's own
enum { STREAM_EMBED = 1, STREAM_HEAD = 2 };

// ------------------------------------------------------------------------------------------------ NT GEMM
// C[M,N] = epilogue(A[M,K] B[N,K]^T): every setter that takes an operand also raises its flag, so no caller writes a.flags
struct G {
    GemmNTArgs a{};
    G(const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K) {
        a.A = A; a.lda = lda; a.B = B; a.ldb = ldb; a.C = C; a.ldc = ldc; a.M = M; a.N = N; a.K = K;
    }
    G& bias(const float* b) { a.bias = b; a.flags |= GEMM_BIAS; return *this; }
    G& gelu() { a.flags |= GEMM_GELU; return *this; }
    G& qgelu() { a.flags |= GEMM_QGELU; return *this; }
    G& tanh() { a.flags |= GEMM_TANH; return *this; }
    G& out_f32() { a.flags |= GEMM_OUT_F32; return *this; }
    G& aux(void* p, int ld) { a.aux = p; a.ldaux = ld; a.flags |= GEMM_AUX_PRE; return *this; }
    G& residual(const void* p, int ld) { a.residual = p; a.ldres = ld; a.flags |= GEMM_RESIDUAL; return *this; }
    G& mul_gelu_grad(const void* p, int ld) { a.mul_in = p; a.ldmul = ld; a.flags |= GEMM_MUL_GELU_GRAD; return *this; }
    // the flag goes up only when the configuration drops anything (make_drop: p > 0 and train mode)
    G& dropout(const DropCfg& d, int row_mul = 1) { a.drop = d; a.drop_row_mul = row_mul; if (d.thresh16) a.flags |= GEMM_DROPOUT; return *this; }
    G& force_slow(int on) { a.force_slow = on; return *this; }
    G& tile(int code) { a.tile = code; return *this; }
    G& grid(int workgroups) { a.grid = workgroups; return *this; }
    // parity mode with plane pairs: both operands are pairs whose rows hold [hi(W) | lo(W)] -- the leading dimensions given in logical
    // elements double, the lo planes sit K elements behind; px_out: C as a pair, rows [hi(N) | lo(N)]
    G& px_in(bool px, int nprod = 0) { if (px) { a.a_pair = a.b_pair = 1; a.lda *= 2; a.ldb *= 2; a.a_lo = a.b_lo = a.K; a.nprod = nprod; } return *this; }
    G& px_out(bool px, bool hi_only = false) { if (px) { a.flags |= GEMM_OUT_PAIR | (hi_only ? GEMM_OUT_PAIR_HI : 0); a.ldc *= 2; a.c_lo = a.N; } return *this; }
};
// the same rule for a weight-gradient problem C = A^T B whose operands are pairs: rows [hi(Nn) | lo(Nn)] of A, [hi(Nc) | lo(Nc)] of B
inline void tn_pair(GemmTNProblem& p, int nprod) { p.pair = 1; p.lda *= 2; p.ldb *= 2; p.a_lo = p.Nn; p.b_lo = p.Nc; p.nprod = nprod; }

inline SmallGemmArgs small(const void* A, int lda, const float* W, int ldw, const float* bias, float* out, int ldo, int M, int N, int K, int act = ACT_NONE, int acc = 0) {
    SmallGemmArgs a{};
    a.A = A; a.W = W; a.bias = bias; a.out = out; a.M = M; a.N = N; a.K = K; a.lda = lda; a.ldw = ldw; a.ldo = ldo; a.act = act; a.accumulate = acc;
    return a;
}

// ------------------------------------------------------------------------------------------------ fused CLS classifier head
// the part both launches share: the CLS rows (x_stride: H compact, T * H inside the full tensor), the classifier and the head dropout
inline ClsHeadArgs cls_head(const void* x, size_t x_stride, int x_dtype, const float* W, int B, int C, int H, const DropCfg& drop) {
    ClsHeadArgs a{};
    a.x = x; a.x_stride = x_stride; a.x_dtype = x_dtype; a.W = W; a.B = B; a.C = C; a.H = H; a.drop = drop;
    return a;
}

// ------------------------------------------------------------------------------------------------ aspect-att fusion head
// the part both launches share: the two pooler outputs, aspectattention.*, and what the forward leaves for the backward
inline AspectFusionArgs aspect_fusion(const float* t_pool, const float* v_pool, const float* a, const float* b, int B, int H, float* feats, float* w, float* e) {
    AspectFusionArgs f{};
    f.t_pool = t_pool; f.v_pool = v_pool; f.a = a; f.b = b; f.B = B; f.H = H; f.feats = feats; f.w = w; f.e = e;
    return f;
}

// ------------------------------------------------------------------------------------------------ attention
// qkv is [rows, 3 hidden] packed q | k | v, ctx [rows, hidden]; scores are scaled by 1 / sqrt(head width).  Every model here has 64-wide heads
// (mmhip_create / mmhip_early_create insist on heads * 64 == hidden; the op entry points pass hidden = heads * 64), and 1 / sqrtf(64.f) is exactly
// 0.125f, the literal the op entry points used to write.
template <typename A>
inline void attn_common(A& a, const float* maskbias, int posts, int S, int heads, int hidden, const DropCfg& drop) {
    a.maskbias = maskbias; a.posts = posts; a.S = S; a.heads = heads; a.hidden = hidden; a.drop = drop;
    a.ld_qkv = 3 * hidden; a.ld_ctx = hidden;
    a.scale = 1.0f / sqrtf((float)(hidden / heads));
}
inline AttnArgs attn_args(const void* qkv, const float* maskbias, void* ctx, float* lse, int posts, int S, int heads, int hidden, const DropCfg& drop = DropCfg{}) {
    AttnArgs a{};
    a.qkv = qkv; a.ctx = ctx; a.lse = lse;
    attn_common(a, maskbias, posts, S, heads, hidden, drop);
    return a;
}
inline AttnBwdArgs attn_bwd_args(const void* qkv, const float* maskbias, const void* ctx, const void* dctx, const float* lse, void* dqkv, int posts, int S, int heads,
                                 int hidden, const DropCfg& drop = DropCfg{}) {
    AttnBwdArgs a{};
    a.qkv = qkv; a.ctx = ctx; a.dctx = dctx; a.lse = lse; a.dqkv = dqkv;
    attn_common(a, maskbias, posts, S, heads, hidden, drop);
    return a;
}
// parity mode with plane pairs: qkv (and dqkv) rows hold [hi(3 hidden) | lo(3 hidden)], ctx (and d ctx) rows [hi(hidden) | lo(hidden)] -- leading
// dimensions in 16-bit elements, the lo plane one logical row width behind the hi plane
template <typename A>
inline void attn_pair(A& a, bool px) {
    if (px) { a.pair = 1; a.ld_qkv = 6 * a.hidden; a.lo_qkv = 3 * a.hidden; a.ld_ctx = 2 * a.hidden; a.lo_ctx = a.hidden; }
}
inline void attn_pair(AttnBwdArgs& a, bool px, int nprod) { attn_pair(a, px); if (px) a.nprod = nprod; }      // nprod: AttnBwdArgs::nprod, the backward's product policy
// the forward with a per-head 2-D score bias: `a` as filled above (pair strides included) plus the bias image [heads][S][ld_bias]
inline AttnBiasArgs attn_bias(const AttnArgs& a, const float* bias2d, int ld_bias) {
    AttnBiasArgs b{};
    static_cast<AttnArgs&>(b) = a;
    b.bias2d = bias2d; b.ld_bias = ld_bias;
    return b;
}
// cross attention on compact tensors: Sq queries per post against Sk keys; the Q columns of qkv and ctx hold Sq rows per post, the K | V columns Sk
template <typename A>
inline void attn_cross(A& a, int Sq, int Sk) { a.Sq_live = Sq; a.Sk_live = Sk; a.q_rps = Sq; a.kv_rps = Sk; a.ctx_rps = Sq; }

// ------------------------------------------------------------------------------------------------ row-op outputs as plane pairs (parity mode)
// A producer whose output feeds a matrix product also writes it as rows [hi(width) | lo(width)] at `pair`.
// pair_only: nothing but GEMMs read the output -- the plain form is not written
inline void ln_pair(LNArgs& a, bool px, void* pair, bool pair_only = false) {
    if (px) { a.y_pair = pair; a.ld_pair = 2 * a.width; a.lo_pair = a.width; if (pair_only) a.y = nullptr; }
}
// LayerNorm backward: the tensor the following GEMMs read (dx_drop where dropout is on, else dx); hi_only: every reader takes one product
inline void ln_bwd_pair(LNBwdArgs& a, bool px, void* pair, bool hi_only) {
    if (px) { a.pair_out = pair; a.ld_pair = 2 * a.width; a.lo_pair = a.width; a.pair_hi_only = hi_only; }
}
inline void embed_pair(EmbedArgs& a, bool px, void* pair) {
    if (px) { a.x_pair = pair; a.ld_pair = 2 * a.H; a.lo_pair = a.H; }
}

// ------------------------------------------------------------------------------------------------ grouped launches
// launch(items + i, n) for consecutive groups of at most max_group items
template <typename T, typename F>
inline int launch_grouped(const T* items, size_t count, size_t max_group, F launch) {
    for (size_t i = 0; i < count; i += max_group) {
        const size_t n = count - i < max_group ? count - i : max_group;
        CHECK_HIP(launch(items + i, (int)n));
    }
    return 0;
}
inline int launch_cast_groups(const std::vector<CastMat>& mats, int dtype, hipStream_t s) {
    return launch_grouped(mats.data(), mats.size(), CAST_MAX_GROUP, [&](const CastMat* m, int n) { return launch_cast_group(m, n, dtype, s); });
}
inline int launch_tn_groups(const std::vector<GemmTNProblem>& probs, int accumulate, int dtype, hipStream_t s) {
    return launch_grouped(probs.data(), probs.size(), GEMM_TN_MAX_GROUP,
                          [&](const GemmTNProblem* p, int n) { return launch_gemm_tn(p, n, accumulate, dtype, 0, s, 1.0f); });
}

// ------------------------------------------------------------------------------------------------ optimizer
// everything of an AdamW launch but the range (p, g, m, v, n), which the caller fills per launch: the hyper-parameters, the bias corrections of
// `step` (computed in double), and the overflow guard's words (either may be null)
inline AdamWArgs adamw_args(float lr, float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale, int zero_grad,
                            unsigned* nonfinite = nullptr, const unsigned* skip = nullptr) {
    AdamWArgs a{};
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
    a.bc1 = (float)(1.0 - pow((double)beta1, step));
    a.bc2_sqrt = (float)sqrt(1.0 - pow((double)beta2, step));
    a.zero_grad = zero_grad; a.grad_scale = grad_scale; a.nonfinite = nonfinite; a.skip = skip;
    return a;
}

// ------------------------------------------------------------------------------------------------ layout
// workspace carve-up: byte offsets, every piece 256-byte aligned
struct Carver {
    size_t off = 0;
    size_t take(size_t bytes) { size_t r = off; off += (bytes + 255) & ~(size_t)255; return r; }
};
// parameter table of a flat fp32 layout: appends to `params`, one running element offset per buffer (0 frozen, 1 trainable)
struct ParamTable {
    std::vector<mmhip_param_info>& params;
    size_t off[2] = {0, 0};
    size_t add(const std::string& name, int buffer, int group, std::initializer_list<int64_t> dims) {
        mmhip_param_info p{};
        strncpy(p.name, name.c_str(), sizeof(p.name) - 1);
        p.ndim = (int)dims.size();
        size_t n = 1;
        int i = 0;
        for (auto d : dims) { p.dims[i++] = d; n *= (size_t)d; }
        p.buffer = buffer;
        p.group = group;
        p.offset = off[buffer];
        p.numel = n;
        params.push_back(p);
        off[buffer] += (n + 3) & ~(size_t)3;      // keep every tensor 16-byte aligned
        return (size_t)p.offset;
    }
};

}  // namespace mmhip
