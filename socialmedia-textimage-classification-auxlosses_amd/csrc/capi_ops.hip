// Operator-level C entry points (parity tests call the very launchers the engine uses) and the hardware-layout probe.
#include <map>
#include <mutex>
#include <vector>
#include "mmhip_common.h"
#include "mmhip_host.h"

using namespace mmhip;

// ------------------------------------------------------------------------------------------------ probe
// Index-coded operands make every lane's view of the MFMA / transposing-read layouts observable:
//   out[0    .. 1023]  D of mfma_f32_16x16x32_bf16 with A[i][k] = (k==0) * (i+1),  B[k][j] = (k==0) * (j+1)*32
//                      -> D[i][j] = (i+1)*(j+1)*32, stored as out[lane*4 + reg]
//   out[1024 .. 2047]  D of mfma_f32_32x32x16_bf16, same construction, out[1024 + lane*16 + reg]
//   out[2048 .. 2303]  ds_read_b64_tr_b16 of a [16 rows][64 cols] bf16 image holding row*64+col; lane's address =
//                      row (lane>>4)*4 + ((lane>>2)&3), col 4*(lane&3); out[2048 + lane*4 + e]
//   out[2304 .. 2815]  k-order probe of mfma_f32_16x16x32: A[i][k] = 1 for all, B[k][j] = (j==0) ? 2^k' ... (see test)
__global__ __launch_bounds__(64) void probe_kernel(int32_t* out) {
    __shared__ __attribute__((aligned(16))) bf16_t img[16 * 64];
    const int lane = threadIdx.x;
    {   // 16x16x32: lane l holds A[l&15][8(l>>4)+j], B[8(l>>4)+j][l&15]
        bf16x8 a, b;
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * (lane >> 4) + j;
            a[j] = (bf16_t)(k == 0 ? (float)((lane & 15) + 1) : 0.f);
            b[j] = (bf16_t)(k == 0 ? (float)(((lane & 15) + 1) * 32) : 0.f);
        }
        f32x4 d = mfma16(a, b, f32x4{0.f, 0.f, 0.f, 0.f});
        for (int r = 0; r < 4; ++r) out[lane * 4 + r] = (int)d[r];
    }
    {   // 32x32x16: lane l holds A[l&31][8(l>>5)+j], B[8(l>>5)+j][l&31]
        bf16x8 a, b;
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * (lane >> 5) + j;
            a[j] = (bf16_t)(k == 0 ? (float)((lane & 31) + 1) : 0.f);
            b[j] = (bf16_t)(k == 0 ? (float)(((lane & 31) + 1) * 32) : 0.f);
        }
        f32x16 d = mfma32(a, b, f32x16{});
        for (int r = 0; r < 16; ++r) out[1024 + lane * 16 + r] = (int)d[r];
    }
    for (int i = lane; i < 16 * 64; i += 64) img[i] = (bf16_t)(float)(i % 256);   // value = (row*64+col) mod 256 (exact in bf16)
    __syncthreads();
    {
        const int row = (lane >> 4) * 4 + ((lane >> 2) & 3), col = 4 * (lane & 3);
        s16x4 t = lds_read_tr4(reinterpret_cast<const char*>(img), (row * 64 + col) * 2);
        bf16x4 tb = __builtin_bit_cast(bf16x4, t);
        for (int e = 0; e < 4; ++e) out[2048 + lane * 4 + e] = (int)(float)tb[e];
    }
    {   // k-order: A[i][k] = k+1 (all rows), B[k][j] = (k == j) for j < 16 (k < 16) -> D[i][j] = j+1;  second half k>=16: B[k][j] = (k-16==j)*64
        bf16x8 a, b;
        for (int j = 0; j < 8; ++j) {
            const int k = 8 * (lane >> 4) + j;
            a[j] = (bf16_t)(float)(k + 1);
            b[j] = (bf16_t)((k & 15) == (lane & 15) ? (k < 16 ? 1.f : 64.f) : 0.f);
        }
        f32x4 d = mfma16(a, b, f32x4{0.f, 0.f, 0.f, 0.f});
        for (int r = 0; r < 4; ++r) out[2304 + lane * 4 + r] = (int)d[r];
    }
}

extern "C" {

int mmhip_op_probe_layouts(int32_t* out, void* stream) {
    if (!out) return MMHIP_E_INVALID;
    hipLaunchKernelGGL(probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, out);
    CHECK_HIP(hipGetLastError());
    return 0;
}

// parity mode through the op entry points: a split-plane scratch PER STREAM, grown on demand (hipFree waits for the device, so a buffer still
// in use by an earlier launch is never pulled away).  One shared buffer was a race as soon as two streams ran operators side by side
// (the early-fusion path's vision stream: run-to-run different outputs in bf16x3).  The engine carves its own per-stream scratch.
static void* ops_x3_scratch(size_t bytes, void* stream) {
    struct Buf { void* p = nullptr; size_t cap = 0; };
    static std::mutex mu;
    static std::map<void*, Buf> bufs;
    std::lock_guard<std::mutex> lock(mu);
    Buf& b = bufs[stream];
    if (bytes > b.cap) {
        if (b.p) (void)hipFree(b.p);
        b.p = nullptr; b.cap = 0;
        if (hipMalloc(&b.p, bytes) != hipSuccess) { b.p = nullptr; return nullptr; }
        b.cap = bytes;
    }
    return b.p;
}

int mmhip_op_gemm_nt(int dtype, const void* A, int lda, const void* B, int ldb, void* C, int ldc, int M, int N, int K,
                     const float* bias, int act, void* aux_pre, int ldaux, const void* mul_gelu_grad_of, int ldmul,
                     float p_drop, uint64_t seed, uint32_t stream_id, const void* residual, int ldres, int out_f32,
                     int force_slow, void* stream) {
    if (!A || !B || !C || M < 0 || N < 1 || K < 1 || (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_F32)) return MMHIP_E_INVALID;
    if ((force_slow >> 4) && !nt_tile_known(force_slow >> 4)) return MMHIP_E_INVALID;      // a tile code no launcher has
    G g(A, lda, B, ldb, C, ldc, M, N, K);
    if (bias) g.bias(bias);
    if (act == 1) g.gelu();
    if (act == 2) g.tanh();
    if (act == 3) g.qgelu();
    if (aux_pre) g.aux(aux_pre, ldaux);
    if (mul_gelu_grad_of) g.mul_gelu_grad(mul_gelu_grad_of, ldmul);
    g.dropout(make_drop(p_drop, seed, stream_id));
    if (residual) g.residual(residual, ldres);
    if (out_f32) g.out_f32();
    g.force_slow(force_slow & 1).tile(force_slow >> 4);      // bits 4.. select the tile variant (test / tuning hook)
    GemmNTArgs& a = g.a;
    if (dtype == MMHIP_F32 && M > 128 && !a.force_slow) {
        a.x3_ws_bytes = x3_nt_scratch_bytes(M, N, K);
        a.x3_ws = ops_x3_scratch(a.x3_ws_bytes, stream);
    }
    // 16-bit, few rows, long K: the split-K path the engine's CLS-row GEMMs take (gemm.hip splitk_slices); its fp32 partial products live in the same
    // per-stream scratch (one operator at a time per stream; the parity mode never takes this path)
    if (const size_t sk = nt_splitk_scratch_bytes(a, dtype)) a.splitk_ws = (float*)ops_x3_scratch(sk, stream);
    CHECK_HIP(launch_gemm_nt(a, dtype, (hipStream_t)stream));
    return 0;
}

int mmhip_op_last_gemm_path(int which, int32_t* out) {
    if (!out || (which != 0 && which != 1)) return MMHIP_E_INVALID;
    const GemmPathRecord& r = gemm_path_record();
    for (int i = 0; i < 8; ++i) out[i] = which ? r.tn[i] : r.nt[i];
    return 0;
}
int mmhip_tn_max_group(void) { return GEMM_TN_MAX_GROUP; }

int mmhip_op_gemm_tn(int dtype, const void* A, int lda, const void* B, int ldb, float* C, int ldc, int M, int Nn, int Nc,
                     int accumulate, int force_slow, float* colsum, void* stream) {
    if (!A || !B || !C || M < 1 || Nn < 1 || Nc < 1 || (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_F32)) return MMHIP_E_INVALID;
    if ((force_slow >> 4) && !tn_variant_known(force_slow >> 4)) return MMHIP_E_INVALID;      // a variant no launcher has
    GemmTNProblem p{A, B, C, M, Nn, Nc, lda, ldb, ldc, 0, colsum};
    size_t xb = dtype == MMHIP_F32 && !force_slow ? x3_tn_scratch_bytes(M, Nn, Nc) : 0;
    void* xw = xb ? ops_x3_scratch(xb, stream) : nullptr;
    CHECK_HIP(launch_gemm_tn(&p, 1, accumulate, dtype, force_slow, (hipStream_t)stream, 1.0f, xw, xw ? xb : 0));
    return 0;
}

int mmhip_op_gemm_tn_group(int dtype, const mmhip_tn_problem* problems, int count, int accumulate, void* stream) {
    if (!problems || count < 0 || (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_F32)) return MMHIP_E_INVALID;
    std::vector<GemmTNProblem> ps((size_t)count);
    for (int i = 0; i < count; ++i) {
        const mmhip_tn_problem& q = problems[i];
        if (!q.A || !q.B || !q.C || q.M < 1 || q.Nn < 1 || q.Nc < 1) return MMHIP_E_INVALID;
        ps[i] = GemmTNProblem{q.A, q.B, q.C, q.M, q.Nn, q.Nc, q.lda, q.ldb, q.ldc, 0, q.colsum};
    }
    size_t xb = 0;
    if (dtype == MMHIP_F32) for (int i = 0; i < count; ++i) xb += x3_tn_scratch_bytes(ps[i].M, ps[i].Nn, ps[i].Nc);
    void* xw = xb ? ops_x3_scratch(xb, stream) : nullptr;
    if (count) CHECK_HIP(launch_gemm_tn(ps.data(), count, accumulate, dtype, 0, (hipStream_t)stream, 1.0f, xw, xw ? xb : 0));
    return 0;
}

int mmhip_op_cast_group(int dtype, const mmhip_cast_mat* mats, int count, void* stream) {
    if (!mats || count < 0 || (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_F32)) return MMHIP_E_INVALID;
    std::vector<CastMat> g((size_t)count);
    for (int i = 0; i < count; ++i) {
        if (!mats[i].src || !mats[i].dst || mats[i].rows < 4 || mats[i].cols < 4) return MMHIP_E_INVALID;
        g[i] = CastMat{mats[i].src, mats[i].dst, mats[i].dst_t, mats[i].rows, mats[i].cols, 0};
    }
    return launch_cast_groups(g, dtype, (hipStream_t)stream);
}

// ---- composite operators: one post-LN sub-block of a BERT-shaped stream per call (the early-fusion path's host time is launch
// and interpreter work: a block is 3-4 launches of the same kernels, enqueued from C++)
// (dropout stream ids inside a block: 7 attention probabilities, 8 attention output, 9 feed-forward output)
namespace {
// backward of the block's closing LayerNorm: d pre, and its dropout-backward copy dd when the block's output dropout was on
LNBwdArgs block_ln_bwd(const void* dy, const void* pre, const float* gamma, const float* mean, const float* rstd, void* dpre, float* dgamma, float* dbeta, int rows, int width,
                       void* dd, float p_hid, uint64_t seed, uint32_t stream_id) {
    LNBwdArgs b{};
    b.dy = dy; b.x = pre; b.gamma = gamma; b.mean = mean; b.rstd = rstd; b.dx = dpre; b.dgamma = dgamma; b.dbeta = dbeta; b.rows = rows; b.width = width; b.alpha = 1.0f;
    if (p_hid > 0.f) { b.dx_drop = dd; b.drop = make_drop(p_hid, seed, stream_id); b.drop_row_mul = 1; }
    return b;
}
}  // namespace

int mmhip_op_self_att_block_fwd(int dtype, const void* x, const float* maskbias, const void* wqkv, const float* bqkv, const void* wo, const float* bo,
                                const float* gamma, const float* beta, float eps, int posts, int S, int heads, float p_att, float p_hid, uint64_t seed,
                                void* qkv, void* att, float* lse, void* pre, float* mean, float* rstd, void* y, void* stream) {
    if (!x || !wqkv || !bqkv || !wo || !bo || !gamma || !beta || !qkv || !att || !lse || !pre || !mean || !rstd || !y || posts < 1 || S < 1 || heads < 1)
        return MMHIP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int H = heads * 64, M = posts * S;
    CHECK_HIP(launch_gemm_nt(G(x, H, wqkv, H, qkv, 3 * H, M, 3 * H, H).bias(bqkv).a, dtype, s));
    CHECK_HIP(launch_attn_fwd(attn_args(qkv, maskbias, att, lse, posts, S, heads, H, make_drop(p_att, seed, 7)), dtype, s));
    CHECK_HIP(launch_gemm_nt(G(att, H, wo, H, pre, H, M, H, H).bias(bo).dropout(make_drop(p_hid, seed, 8)).residual(x, H).a, dtype, s));
    LNArgs ln{pre, y, gamma, beta, mean, rstd, M, H, H, H, eps};
    CHECK_HIP(launch_layernorm_fwd(ln, dtype, s));
    return 0;
}

int mmhip_op_self_att_block_bwd(int dtype, const void* dy, const float* maskbias, const void* wqkvT, const void* woT, const float* gamma, int posts, int S,
                                int heads, float p_att, float p_hid, uint64_t seed, const void* qkv, const void* att, const float* lse, const void* pre,
                                const float* mean, const float* rstd, float* dgamma, float* dbeta, void* dpre, void* dd, void* datt, void* dqkv, void* dx,
                                void* stream) {
    if (!dy || !wqkvT || !woT || !gamma || !qkv || !att || !lse || !pre || !mean || !rstd || !dgamma || !dbeta || !dpre || !dd || !datt || !dqkv || !dx)
        return MMHIP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int H = heads * 64, M = posts * S;
    CHECK_HIP(launch_layernorm_bwd(block_ln_bwd(dy, pre, gamma, mean, rstd, dpre, dgamma, dbeta, M, H, dd, p_hid, seed, 8), dtype, s));
    const void* dsrc = p_hid > 0.f ? dd : dpre;          // gradient of the output projection's result
    CHECK_HIP(launch_gemm_nt(G(dsrc, H, woT, H, datt, H, M, H, H).a, dtype, s));
    CHECK_HIP(launch_attn_bwd(attn_bwd_args(qkv, maskbias, att, datt, lse, dqkv, posts, S, heads, H, make_drop(p_att, seed, 7)), dtype, s));
    CHECK_HIP(launch_gemm_nt(G(dqkv, 3 * H, wqkvT, 3 * H, dx, H, M, H, 3 * H).residual(dpre, H).a, dtype, s));
    return 0;
}

// ---- cross-attention block (LXMERT's cross-modality layers: queries from one stream, keys / values from the other).  Rounds 3-4 packed both
// streams into S-row blocks of one tensor (S = max(Sq, Sk)) with clears and row copies, then with a row remap in the projections' epilogue; since
// round 5 the attention kernels take the two streams' rows where the projections put them (compact tensors, two row pitches): see the forward below.
namespace {
inline size_t esz_of(int dtype) { return dtype == MMHIP_F32 ? 4 : 2; }
}  // namespace

int mmhip_op_cross_att_block_fwd(int dtype, const void* xq, const void* xc, const float* keybias, const void* wqkv, const float* bqkv, const void* wo,
                                 const float* bo, const float* gamma, const float* beta, float eps, int posts, int Sq, int Sk, int heads, float p_att,
                                 float p_hid, uint64_t seed, void* qkv, void* att, float* lse, void* tq, void* tkv, void* attq, void* pre, float* mean,
                                 float* rstd, void* y, void* stream) {
    (void)tq; (void)tkv; (void)attq;          // scratch of the padded forms of rounds 3-4: unused since round 5
    if (!xq || !xc || !keybias || !wqkv || !bqkv || !wo || !bo || !gamma || !beta || !qkv || !att || !lse || !pre || !mean || !rstd || !y || posts < 1 ||
        Sq < 1 || Sk < 1 || heads < 1)
        return MMHIP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int H = heads * 64, S = Sq > Sk ? Sq : Sk, Mq = posts * Sq, Mc = posts * Sk;
    const size_t Z = esz_of(dtype);
    // Round 5, every dtype: COMPACT tensors.  The query projection writes Mq rows into columns [0, H) of qkv, the key / value projection Mc rows into
    // columns [H, 3H) -- row p * Sq + q is query q of post p, row p * Sk + k its key k -- and the attention kernels are told the two row pitches
    // (AttnArgs::q_rps / kv_rps / ctx_rps) and the two lengths.  Nothing is padded, cleared, remapped or copied; key tiles past Sk are not computed;
    // att is [Mq, H], the operand of the output projection as it is.  The dropout masks, the lse rows and keybias keep the indices of the S x S layout.
    const char* w = (const char*)wqkv;
    // Q = xq Wq^T + bq
    CHECK_HIP(launch_gemm_nt(G(xq, H, w, H, qkv, 3 * H, Mq, H, H).bias(bqkv).a, dtype, s));
    // [K | V] = xc [Wk; Wv]^T + [bk; bv]
    CHECK_HIP(launch_gemm_nt(G(xc, H, w + (size_t)H * H * Z, H, (char*)qkv + (size_t)H * Z, 3 * H, Mc, 2 * H, H).bias(bqkv + H).a, dtype, s));
    AttnArgs at = attn_args(qkv, keybias, att, lse, posts, S, heads, H, make_drop(p_att, seed, 7));
    attn_cross(at, Sq, Sk);
    CHECK_HIP(launch_attn_fwd(at, dtype, s));
    CHECK_HIP(launch_gemm_nt(G(att, H, wo, H, pre, H, Mq, H, H).bias(bo).dropout(make_drop(p_hid, seed, 8)).residual(xq, H).a, dtype, s));
    LNArgs ln{pre, y, gamma, beta, mean, rstd, Mq, H, H, H, eps};
    CHECK_HIP(launch_layernorm_fwd(ln, dtype, s));
    return 0;
}

int mmhip_op_cross_att_block_bwd(int dtype, const void* dy, const float* keybias, const void* wqkvT, const void* woT, const float* gamma, int posts, int Sq,
                                 int Sk, int heads, float p_att, float p_hid, uint64_t seed, const void* qkv, const void* att, const float* lse,
                                 const void* pre, const float* mean, const float* rstd, float* dgamma, float* dbeta, void* dpre, void* dd, void* dattq,
                                 void* datt, void* dqkv, void* dq, void* dkv, void* dxq, void* dxc, void* stream) {
    (void)dattq; (void)dq; (void)dkv;          // scratch of the padded forms of rounds 3-4: unused since round 5
    if (!dy || !keybias || !wqkvT || !woT || !gamma || !qkv || !att || !lse || !pre || !mean || !rstd || !dgamma || !dbeta || !dpre || !dd || !datt || !dqkv ||
        !dxq || !dxc || posts < 1 || Sq < 1 || Sk < 1 || heads < 1)
        return MMHIP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    const int H = heads * 64, S = Sq > Sk ? Sq : Sk, Mq = posts * Sq, Mc = posts * Sk;
    const size_t Z = esz_of(dtype);
    CHECK_HIP(launch_layernorm_bwd(block_ln_bwd(dy, pre, gamma, mean, rstd, dpre, dgamma, dbeta, Mq, H, dd, p_hid, seed, 8), dtype, s));
    const void* dsrc = p_hid > 0.f ? dd : dpre;
    CHECK_HIP(launch_gemm_nt(G(dsrc, H, woT, H, datt, H, Mq, H, H).a, dtype, s));          // d att, compact [Mq, H] like att
    AttnBwdArgs ab = attn_bwd_args(qkv, keybias, att, datt, lse, dqkv, posts, S, heads, H, make_drop(p_att, seed, 7));
    attn_cross(ab, Sq, Sk);
    CHECK_HIP(launch_attn_bwd(ab, dtype, s));
    // dqkv as qkv: dQ in rows [0, Mq) of columns [0, H), [dK | dV] in rows [0, Mc) of columns [H, 3H) -- the operands of the two input-gradient products
    // below and of the caller's weight-gradient products (leading dimension 3H), as they are
    const char* wt = (const char*)wqkvT;              // [H, 3H]: columns [0,H) = Wq^T, [H,3H) = [Wk; Wv]^T
    // d xq = dQ Wq + d pre (residual branch)
    CHECK_HIP(launch_gemm_nt(G(dqkv, 3 * H, wt, 3 * H, dxq, H, Mq, H, H).residual(dpre, H).a, dtype, s));
    // d xc = [dK | dV] [Wk; Wv]
    CHECK_HIP(launch_gemm_nt(G((const char*)dqkv + (size_t)H * Z, 3 * H, wt + (size_t)H * Z, 3 * H, dxc, H, Mc, H, 2 * H).a, dtype, s));
    return 0;
}

int mmhip_op_ffn_block_fwd(int dtype, const void* x, const void* w1, const float* b1, const void* w2, const float* b2, const float* gamma, const float* beta,
                           float eps, int M, int H, int I, float p_hid, uint64_t seed, void* h, void* u, void* pre, float* mean, float* rstd, void* y,
                           void* stream) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !gamma || !beta || !h || !u || !pre || !mean || !rstd || !y || M < 1) return MMHIP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    CHECK_HIP(launch_gemm_nt(G(x, H, w1, H, h, I, M, I, H).bias(b1).aux(u, I).gelu().a, dtype, s));
    CHECK_HIP(launch_gemm_nt(G(h, I, w2, I, pre, H, M, H, I).bias(b2).dropout(make_drop(p_hid, seed, 9)).residual(x, H).a, dtype, s));
    LNArgs ln{pre, y, gamma, beta, mean, rstd, M, H, H, H, eps};
    CHECK_HIP(launch_layernorm_fwd(ln, dtype, s));
    return 0;
}

int mmhip_op_ffn_block_bwd(int dtype, const void* dy, const void* w1T, const void* w2T, const float* gamma, int M, int H, int I, float p_hid, uint64_t seed,
                           const void* u, const void* pre, const float* mean, const float* rstd, float* dgamma, float* dbeta, void* dpre, void* dd, void* du,
                           void* dx, void* stream) {
    if (!dy || !w1T || !w2T || !gamma || !u || !pre || !mean || !rstd || !dgamma || !dbeta || !dpre || !dd || !du || !dx) return MMHIP_E_INVALID;
    hipStream_t s = (hipStream_t)stream;
    CHECK_HIP(launch_layernorm_bwd(block_ln_bwd(dy, pre, gamma, mean, rstd, dpre, dgamma, dbeta, M, H, dd, p_hid, seed, 9), dtype, s));
    const void* dsrc = p_hid > 0.f ? dd : dpre;
    CHECK_HIP(launch_gemm_nt(G(dsrc, H, w2T, H, du, I, M, I, H).mul_gelu_grad(u, I).a, dtype, s));
    CHECK_HIP(launch_gemm_nt(G(du, I, w1T, I, dx, H, M, H, I).residual(dpre, H).a, dtype, s));
    return 0;
}

int mmhip_op_layernorm_fwd(int dtype, const void* x, void* y, const float* gamma, const float* beta, float* mean, float* rstd,
                           int rows, int width, float eps, void* stream) {
    if (!x || !y || !gamma || !beta) return MMHIP_E_INVALID;
    LNArgs a{x, y, gamma, beta, mean, rstd, rows, width, width, width, eps};
    if (dtype == MMHIP_PAIR) {          // parity mode as the engine runs it: fp32 rows in, the output as a plane pair only ([hi(width) | lo(width)] per row)
        ln_pair(a, true, y, true);
        dtype = MMHIP_F32;
    }
    CHECK_HIP(launch_layernorm_fwd(a, dtype, (hipStream_t)stream));
    return 0;
}
int mmhip_op_layernorm_bwd(int dtype, const void* dy, const void* x, const float* gamma, const float* mean, const float* rstd,
                           void* dx, const void* dres, float* dgamma, float* dbeta, int rows, int width, void* stream) {
    if (!dy || !x || !gamma || !mean || !rstd || !dx || !dgamma || !dbeta) return MMHIP_E_INVALID;
    LNBwdArgs a{};
    a.dy = dy; a.x = x; a.gamma = gamma; a.mean = mean; a.rstd = rstd; a.dx = dx; a.dres = dres; a.dgamma = dgamma; a.dbeta = dbeta;
    a.rows = rows; a.width = width; a.alpha = 1.0f;
    CHECK_HIP(launch_layernorm_bwd(a, dtype, (hipStream_t)stream));
    return 0;
}
int mmhip_op_attn_fwd(int dtype, const void* qkv, const float* maskbias, void* ctx, float* lse, int posts, int S, int heads,
                      float p_drop, uint64_t seed, uint32_t stream_id, void* stream) {
    if (!qkv || !ctx || posts < 1 || S < 1 || heads < 1) return MMHIP_E_INVALID;
    AttnArgs a = attn_args(qkv, maskbias, ctx, lse, posts, S, heads, heads * 64, make_drop(p_drop, seed, stream_id));
    if (dtype == MMHIP_PAIR) { attn_pair(a, true); dtype = MMHIP_F32; }
    CHECK_HIP(launch_attn_fwd(a, dtype, (hipStream_t)stream));
    return 0;
}
int mmhip_op_attn_fwd_bias(int dtype, const void* qkv, const float* bias2d, int ld_bias, void* ctx, float* lse, int posts, int S, int heads, void* stream) {
    if (!qkv || !bias2d || !ctx || posts < 1 || S < 1 || heads < 1) return MMHIP_E_INVALID;
    if (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_F32 && dtype != MMHIP_PAIR) return MMHIP_E_INVALID;
    AttnArgs a = attn_args(qkv, nullptr, ctx, lse, posts, S, heads, heads * 64);
    if (dtype == MMHIP_PAIR) { attn_pair(a, true); dtype = MMHIP_F32; }
    CHECK_HIP(launch_attn_fwd_bias(attn_bias(a, bias2d, ld_bias), dtype, (hipStream_t)stream));
    return 0;
}
int mmhip_op_beit_bias_image(const float* table, int heads, int window_h, int window_w, float* out, int ld_bias, void* stream) {
    if (!table || !out || heads < 1 || window_h < 1 || window_w < 1 || ld_bias < window_h * window_w + 1) return MMHIP_E_INVALID;
    CHECK_HIP(launch_beit_bias_image(table, heads, window_h, window_w, out, ld_bias, (hipStream_t)stream));
    return 0;
}
int mmhip_op_patch_mean_ln(int dtype, const void* x, int rows_per_post, int posts, int width, const float* gamma, const float* beta, float eps, float* out,
                           void* stream) {
    if (!x || !gamma || !beta || !out || posts < 1 || rows_per_post < 2 || width < 4 || width % 4 || width > 1024) return MMHIP_E_INVALID;
    if (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_F32) return MMHIP_E_INVALID;
    CHECK_HIP(launch_patch_mean_ln(x, rows_per_post, posts, width, gamma, beta, eps, out, dtype, (hipStream_t)stream));
    return 0;
}
int mmhip_op_attn_bwd(int dtype, const void* qkv, const float* maskbias, const void* ctx, const void* dctx, const float* lse,
                      void* dqkv, int posts, int S, int heads, float p_drop, uint64_t seed, uint32_t stream_id, void* stream) {
    if (!qkv || !ctx || !dctx || !lse || !dqkv || posts < 1 || S < 1 || heads < 1) return MMHIP_E_INVALID;
    AttnBwdArgs a = attn_bwd_args(qkv, maskbias, ctx, dctx, lse, dqkv, posts, S, heads, heads * 64, make_drop(p_drop, seed, stream_id));
    if (dtype == MMHIP_PAIR) { attn_pair(a, true); dtype = MMHIP_F32; }
    CHECK_HIP(launch_attn_bwd(a, dtype, (hipStream_t)stream));
    return 0;
}
int mmhip_op_attn_bwd_long(int dtype, const void* qkv, const float* maskbias, const void* ctx, const void* dctx, const float* lse,
                           void* dqkv, int posts, int S, int heads, float p_drop, uint64_t seed, uint32_t stream_id, void* stream) {
    if (!qkv || !ctx || !dctx || !lse || !dqkv || posts < 1 || posts > 65535 || heads < 1 || S < 129 || S > 288) return MMHIP_E_INVALID;
    if (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_F32 && dtype != MMHIP_PAIR) return MMHIP_E_INVALID;
    if (((uintptr_t)qkv | (uintptr_t)ctx | (uintptr_t)dctx | (uintptr_t)dqkv) & 15) return MMHIP_E_INVALID;      // 16-byte vector accesses, no ALU kernel behind this entry
    AttnBwdArgs a = attn_bwd_args(qkv, maskbias, ctx, dctx, lse, dqkv, posts, S, heads, heads * 64, make_drop(p_drop, seed, stream_id));
    if (dtype == MMHIP_PAIR) { attn_pair(a, true); dtype = MMHIP_F32; }
    CHECK_HIP(launch_attn_bwd_long(a, dtype, (hipStream_t)stream));
    return 0;
}
int mmhip_op_colsum(int dtype, const void* x, int rows, int cols, int ld, float* out, void* stream) {
    if (!x || !out || (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_F32)) return MMHIP_E_INVALID;      // (any other code would be read as fp32)
    CHECK_HIP(launch_colsum(x, rows, cols, ld, out, dtype, (hipStream_t)stream));
    return 0;
}
int mmhip_op_cast(int dtype, const float* src, void* dst, uint64_t n, int transpose_rows, int transpose_cols, void* stream) {
    if (!src || !dst) return MMHIP_E_INVALID;
    if (transpose_rows > 0) CHECK_HIP(launch_cast_transpose(src, dst, transpose_rows, transpose_cols, dtype, (hipStream_t)stream));
    else CHECK_HIP(launch_cast(src, dst, n, dtype, (hipStream_t)stream));
    return 0;
}


// ------------------------------------------------------------------------------------------------ ITC (rank-local pair: timing reference of the global one)
int mmhip_op_itc_fwd(const float* txt_e, const float* img_e, const float* logit_scale, int B, int E, float* txt_n, float* img_n, float* txt_inv, float* img_inv,
                     float* logits, void* stream) {
    if (B < 1 || B > 1024 || E < 1 || E > 1024 || !txt_e || !img_e || !logit_scale || !txt_n || !img_n || !txt_inv || !img_inv || !logits) return MMHIP_E_INVALID;
    ItcArgs a{txt_e, img_e, logit_scale, txt_n, img_n, txt_inv, img_inv, logits, B, E};
    CHECK_HIP(launch_itc_fwd(a, (hipStream_t)stream));
    return 0;
}
int mmhip_op_itc_bwd(const float* d_logits, const float* logits, const float* txt_n, const float* img_n, const float* txt_inv, const float* img_inv,
                     const float* logit_scale, int B, int E, float* d_txt_e, float* d_img_e, float* d_logit_scale, void* stream) {
    if (B < 1 || B > 1024 || E < 1 || E > 1024 || !d_logits || !logits || !txt_n || !img_n || !txt_inv || !img_inv || !logit_scale || !d_txt_e || !d_img_e) return MMHIP_E_INVALID;
    ItcBwdArgs a{d_logits, logits, txt_n, img_n, txt_inv, img_inv, logit_scale, d_txt_e, d_img_e, d_logit_scale, B, E};
    CHECK_HIP(launch_itc_bwd(a, (hipStream_t)stream));
    return 0;
}
// ------------------------------------------------------------------------------------------------ the late-fusion head's other kernels, alone
static bool fusion_attn_args_ok(int dtype, const void* rows32, const void* xv, const void* o1, const void* o2, int Bt, int B, int P, int H) {
    if (!rows32 || !xv || !o1 || !o2 || B < 1 || Bt < 1 || P < 1 || P > 512 || H < 4 || H > 1024 || H % 4) return false;
    if (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_F32) return false;
    return !(((uintptr_t)rows32 | (uintptr_t)xv) & 15);
}
int mmhip_op_fusion_attn_fwd(int dtype, const float* qk, const void* xv, int Bt, int B, int P, int H, float scale, float* prob, float* xbar, void* stream) {
    if (!fusion_attn_args_ok(dtype, qk, xv, prob, xbar, Bt, B, P, H)) return MMHIP_E_INVALID;
    FusionAttnArgs a{qk, xv, prob, xbar, Bt, B, P, H, scale};
    CHECK_HIP(launch_fusion_attn_fwd(a, dtype, (hipStream_t)stream));
    return 0;
}
int mmhip_op_fusion_attn_bwd(int dtype, const float* dxbar, const float* prob, const void* xv, int Bt, int B, int P, int H, float scale, float* dqk,
                             void* stream) {
    if (!fusion_attn_args_ok(dtype, dxbar, xv, prob, dqk, Bt, B, P, H)) return MMHIP_E_INVALID;
    FusionAttnBwdArgs a{dxbar, prob, xv, dqk, Bt, B, P, H, scale};
    CHECK_HIP(launch_fusion_attn_bwd(a, dtype, (hipStream_t)stream));
    return 0;
}
int mmhip_op_loss(const float* out_cls, const int64_t* onehot, const float* class_w, const float* logits_per_text, const float* itc_global_loss,
                  const float* out_tim, const int64_t* lbl_tim, float w_cls, float w_itc, float w_itm, int B, int C, float* loss, float* d_out_cls,
                  float* d_logits, float* d_out_tim, int32_t* n_correct, void* stream) {
    if (!out_cls || !onehot || !loss || B < 1 || B > 1024 || C < 1) return MMHIP_E_INVALID;
    if ((out_tim && !lbl_tim) || (logits_per_text && itc_global_loss)) return MMHIP_E_INVALID;
    LossArgs a{};
    a.out_cls = out_cls; a.onehot = onehot; a.class_w = class_w; a.logits_per_text = logits_per_text; a.itc_global_loss = itc_global_loss;
    a.out_tim = out_tim; a.lbl_tim = lbl_tim; a.w_cls = w_cls; a.w_itc = w_itc; a.w_itm = w_itm; a.loss = loss;
    a.d_out_cls = d_out_cls; a.d_logits = d_logits; a.d_out_tim = d_out_tim; a.n_correct = n_correct; a.B = B; a.C = C;
    CHECK_HIP(launch_loss(a, (hipStream_t)stream));
    return 0;
}
int mmhip_op_small_gemm(int mode, int a_dtype, const void* A, int lda, const float* W, int ldw, const float* bias, float* out, int ldo, int M, int N,
                        int K, int act, int accumulate, void* stream) {
    if (!A || !W || !out || M < 1 || N < 1 || K < 1 || mode < 0 || mode > 2 || ldo < N) return MMHIP_E_INVALID;
    if (act != ACT_NONE && act != ACT_TANH && act != ACT_RELU) return MMHIP_E_INVALID;
    if (a_dtype != MMHIP_F32 && (mode != 0 || (a_dtype != MMHIP_BF16 && a_dtype != MMHIP_F16))) return MMHIP_E_INVALID;
    if (lda < (mode == 2 ? M : K) || ldw < (mode == 0 ? K : N)) return MMHIP_E_INVALID;
    SmallGemmArgs g{};
    g.A = A; g.lda = lda; g.W = W; g.ldw = ldw; g.bias = bias; g.out = out; g.ldo = ldo; g.M = M; g.N = N; g.K = K; g.act = act; g.accumulate = accumulate ? 1 : 0;
    if (mode == 0) CHECK_HIP(launch_small_nt(g, a_dtype, (hipStream_t)stream));
    else if (mode == 1) CHECK_HIP(launch_small_nn(g, (hipStream_t)stream));
    else {
        g.M = K;          // launch_small_tn: the reduction length goes in as M, the output's rows as n_rows
        CHECK_HIP(launch_small_tn(g, DT_F32, M, (hipStream_t)stream));
    }
    return 0;
}
int mmhip_op_bias_grad_f32(const float* d, int rows, int cols, int ld, float* out, int accumulate, void* stream) {
    if (!d || !out || rows < 1 || cols < 1 || ld < cols) return MMHIP_E_INVALID;
    CHECK_HIP(launch_bias_grad_f32(d, rows, cols, ld, out, accumulate, (hipStream_t)stream));
    return 0;
}
// ------------------------------------------------------------------------------------------------ global-batch ITC
uint64_t mmhip_op_itc_global_ws_bytes(int G, int B_local) {
    if (G < 1 || G > ITC_GLOBAL_MAX_G || B_local < 1 || B_local > G) return 0;
    return (uint64_t)itc_global_ws_floats(G, B_local) * 4;
}
int mmhip_op_itc_global_fwd(const float* txt_n, const float* img_n, const float* logit_scale, int G, int E, float* logits, float* rowlse, float* collse,
                            float* loss, void* ws, uint64_t ws_bytes, void* stream) {
    if (G < 1 || G > ITC_GLOBAL_MAX_G || E < 1 || E > 1024) return MMHIP_E_INVALID;
    if (!txt_n || !img_n || !logit_scale || !rowlse || !collse || !loss || !ws) return MMHIP_E_INVALID;
    if (ws_bytes < (uint64_t)itc_global_ws_floats(G, 1) * 4) return MMHIP_E_CAPACITY;
    ItcGlobalArgs a{txt_n, img_n, logit_scale, logits, rowlse, collse, loss, (float*)ws, G, E};
    CHECK_HIP(launch_itc_global_fwd(a, (hipStream_t)stream));
    return 0;
}
int mmhip_op_itc_global_bwd(const float* txt_n, const float* img_n, const float* logit_scale, const float* rowlse, const float* collse, int G, int B_local,
                            int rank_offset, int E, float seed, float* d_txt_n, float* d_img_n, float* d_logit_scale, const float* txt_inv,
                            const float* img_inv, float* d_txt_e, float* d_img_e, void* ws, uint64_t ws_bytes, void* stream) {
    if (G < 1 || G > ITC_GLOBAL_MAX_G || E < 1 || E > 1024 || B_local < 1 || rank_offset < 0 || (int64_t)rank_offset + B_local > G) return MMHIP_E_INVALID;
    if (!txt_n || !img_n || !logit_scale || !rowlse || !collse || !d_txt_n || !d_img_n || !ws) return MMHIP_E_INVALID;
    if ((d_txt_e && !txt_inv) || (d_img_e && !img_inv)) return MMHIP_E_INVALID;
    if (ws_bytes < (uint64_t)itc_global_ws_floats(G, B_local) * 4) return MMHIP_E_CAPACITY;
    ItcGlobalBwdArgs a{};
    a.txt_n = txt_n; a.img_n = img_n; a.logit_scale = logit_scale; a.rowlse = rowlse; a.collse = collse; a.txt_inv = txt_inv; a.img_inv = img_inv;
    a.d_txt_n = d_txt_n; a.d_img_n = d_img_n; a.dtxt_e = d_txt_e; a.dimg_e = d_img_e; a.dlogit_scale = d_logit_scale; a.ws = (float*)ws;
    a.G = G; a.E = E; a.Bl = B_local; a.r0 = rank_offset; a.scale = seed / (2.f * (float)G);
    CHECK_HIP(launch_itc_global_bwd(a, (hipStream_t)stream));
    return 0;
}

// ------------------------------------------------------------------------------------------------ fused CLS classifier head (text-only model)
int mmhip_op_cls_head_fwd(int x_dtype, const void* x, uint64_t x_stride, const float* W, const float* bias, int B, int C, int H, float p, uint64_t seed,
                          float* logits, const int64_t* onehot, const float* class_w, float* loss, int32_t* n_correct, float* d_logits, void* stream) {
    if (!x || !W || !bias || !logits || !(p >= 0.f) || p >= 1.f) return MMHIP_E_INVALID;
    ClsHeadArgs a = cls_head(x, (size_t)x_stride, x_dtype, W, B, C, H, make_drop(p, seed, STREAM_HEAD));
    a.bias = bias; a.logits = logits; a.onehot = onehot; a.class_w = class_w; a.loss = loss; a.n_correct = n_correct; a.d_logits_out = d_logits;
    const hipError_t r = launch_cls_head_fwd(a, (hipStream_t)stream);
    return r == hipErrorInvalidValue ? MMHIP_E_INVALID : (int)r;
}
int mmhip_op_cls_head_bwd(int x_dtype, const void* x, uint64_t x_stride, const float* W, const float* d_logits, int B, int C, int H, float p, uint64_t seed,
                          float* dW, float* db, int dx_dtype, void* dx, uint64_t dx_stride, float dx_scale, int accumulate, void* stream) {
    if (!x || !W || !d_logits || !(p >= 0.f) || p >= 1.f) return MMHIP_E_INVALID;
    ClsHeadArgs a = cls_head(x, (size_t)x_stride, x_dtype, W, B, C, H, make_drop(p, seed, STREAM_HEAD));
    a.d_logits = d_logits; a.dW = dW; a.db = db; a.dx = dx; a.dx_stride = (size_t)dx_stride; a.dx_dtype = dx_dtype; a.dx_scale = dx_scale; a.accumulate = accumulate;
    const hipError_t r = launch_cls_head_bwd(a, (hipStream_t)stream);
    return r == hipErrorInvalidValue ? MMHIP_E_INVALID : (int)r;
}

// ------------------------------------------------------------------------------------------------ aspect-att fusion head
uint64_t mmhip_op_aspect_fusion_ws_bytes(int B, int H) { return B < 1 || H < 1 ? 0 : (uint64_t)aspect_fusion_partial_floats(B, H) * 4; }
int mmhip_op_aspect_fusion_fwd(const float* t_pool, const float* v_pool, const float* a, const float* b, int B, int H, float* feats, float* w, float* e,
                               void* stream) {
    const hipError_t r = launch_aspect_fusion_fwd(aspect_fusion(t_pool, v_pool, a, b, B, H, feats, w, e), (hipStream_t)stream);
    return r == hipErrorInvalidValue ? MMHIP_E_INVALID : (int)r;
}
int mmhip_op_aspect_fusion_bwd(const float* t_pool, const float* v_pool, const float* a, const float* b, int B, int H, const float* feats, const float* w,
                               const float* e, const float* d_feats, float* d_tpool, float* d_a, float* d_b, int accumulate, int accumulate_dw, void* ws,
                               uint64_t ws_bytes, void* stream) {
    if (B < 1 || H < 64 || H > 1024 || H % 64 || !ws) return MMHIP_E_INVALID;
    if (ws_bytes < mmhip_op_aspect_fusion_ws_bytes(B, H)) return MMHIP_E_CAPACITY;
    AspectFusionArgs f = aspect_fusion(t_pool, v_pool, a, b, B, H, const_cast<float*>(feats), const_cast<float*>(w), const_cast<float*>(e));
    f.d_feats = d_feats; f.d_tpool = d_tpool; f.da = d_a; f.db = d_b; f.partial = (float*)ws; f.accumulate = accumulate; f.accumulate_dw = accumulate_dw;
    const hipError_t r = launch_aspect_fusion_bwd(f, (hipStream_t)stream);
    return r == hipErrorInvalidValue ? MMHIP_E_INVALID : (int)r;
}

// ------------------------------------------------------------------------------------------------ ViT embedding backward (image-only model)
uint64_t mmhip_op_vit_embed_bwd_ws_bytes(int B, int P, int H) { return B < 1 || P < 1 || H < 1 ? 0 : (uint64_t)partial_floats_vit_embed(B, P, H) * 4; }
int mmhip_op_vit_embed_bwd(int dtype, const void* dx, int B, int P, int H, float alpha, float* dpos, float* dcls, void* dpe, int pair_hi_only, void* ws,
                           uint64_t ws_bytes, void* stream) {
    if (B < 1 || P < 2 || H < 8 || H % 8 || H > 1024 || !dx || !dpos || !dcls || !dpe) return MMHIP_E_INVALID;
    if (dtype != MMHIP_BF16 && dtype != MMHIP_F16 && dtype != MMHIP_F32 && dtype != MMHIP_PAIR) return MMHIP_E_INVALID;
    const uint64_t need = mmhip_op_vit_embed_bwd_ws_bytes(B, P, H);
    if (need && (!ws || ws_bytes < need)) return MMHIP_E_CAPACITY;
    VitEmbedBwdArgs a{};
    a.dx = dx; a.dpos = dpos; a.dcls = dcls; a.dpe = dpe; a.B = B; a.P = P; a.H = H; a.alpha = alpha; a.partial = need ? (float*)ws : nullptr;
    if (dtype == MMHIP_PAIR) { a.pair = 1; a.pair_hi_only = pair_hi_only != 0; a.ld_pair = 2 * H; a.lo_pair = H; }
    const hipError_t r = launch_vit_embed_bwd(a, dtype == MMHIP_PAIR ? DT_F32 : dtype, (hipStream_t)stream);
    return r == hipErrorInvalidValue ? MMHIP_E_INVALID : (int)r;
}

// ------------------------------------------------------------------------------------------------ text embeddings (forward, backward scatter)
namespace {
inline bool embed_shape_ok(int dtype, int posts, int T, int H) {
    return (dtype == MMHIP_BF16 || dtype == MMHIP_F16 || dtype == MMHIP_F32) && posts >= 1 && T >= 1 && H >= 4 && H % 4 == 0 && H <= 1024;
}
inline bool off16(std::initializer_list<const void*> ps) {
    uintptr_t v = 0;
    for (const void* p : ps) v |= (uintptr_t)p;
    return (v & 15) != 0;
}
}  // namespace

int mmhip_op_embed_fwd(int dtype, const int64_t* ids, const int64_t* mask, const int64_t* type_ids, const float* word, const float* pos, const float* type,
                       const float* gamma, const float* beta, float eps, int posts, int T, int H, int xlmr, int pad_id, float p, uint64_t seed, void* x,
                       void* xhat, float* rstd, int* pos_ids, float* maskbias, void* x_pair, int ld_pair, int lo_pair, void* stream) {
    if (!ids || !mask || !word || !pos || !type || !gamma || !beta || !x || !pos_ids || !maskbias) return MMHIP_E_INVALID;
    if (!embed_shape_ok(dtype, posts, T, H) || !(p >= 0.f) || p >= 1.f) return MMHIP_E_INVALID;
    if (off16({word, pos, type, gamma, beta, x, xhat, x_pair})) return MMHIP_E_INVALID;      // 16-byte row accesses (8-byte for the 16-bit rows)
    if (x_pair && (dtype != MMHIP_F32 || lo_pair < H || ld_pair < lo_pair + H || ld_pair % 4 || lo_pair % 4)) return MMHIP_E_INVALID;
    EmbedArgs a{};
    a.ids = ids; a.mask = mask; a.type_ids = type_ids; a.word = word; a.pos = pos; a.type = type; a.gamma = gamma; a.beta = beta; a.eps = eps;
    a.x = x; a.xhat = xhat; a.rstd = rstd; a.pos_ids = pos_ids; a.maskbias = maskbias;
    a.posts = posts; a.T = T; a.H = H; a.xlmr = xlmr; a.pad_id = pad_id;
    a.drop = make_drop(p, seed, STREAM_EMBED, 1);
    if (x_pair) { a.x_pair = x_pair; a.ld_pair = ld_pair; a.lo_pair = lo_pair; }
    const hipError_t r = launch_embed_fwd(a, dtype, (hipStream_t)stream);
    return r == hipErrorInvalidValue ? MMHIP_E_INVALID : (int)r;
}

uint64_t mmhip_op_embed_bwd_ws_bytes(int posts, int T, int H, int type_rows) {
    if (posts < 1 || T < 1 || H < 1) return 0;
    return (uint64_t)(partial_floats_embed(posts, T, H) / 3 * (type_rows == 2 ? 4 : 3)) * 4;
}
int mmhip_op_embed_bwd(int dtype, const void* dx, const void* xhat, const float* rstd, const float* gamma, const int64_t* ids, const int* pos_ids,
                       const int64_t* type_ids, int type_rows, int posts, int T, int H, int pad_id, int pos_pad_id, float p, uint64_t seed, float alpha,
                       float* dword, float* dpos, float* dtype_rows, float* dgamma, float* dbeta, void* partial, uint64_t partial_bytes, uint8_t* row_state,
                       float* det_rows, int max_pos, unsigned* status, void* stream) {
    if (!dx || !xhat || !rstd || !gamma || !ids || !pos_ids || !dword || !dpos || !dtype_rows || !dgamma || !dbeta) return MMHIP_E_INVALID;
    if (!embed_shape_ok(dtype, posts, T, H) || !(p >= 0.f) || p >= 1.f) return MMHIP_E_INVALID;
    if ((type_rows == 2 && !type_ids) || (det_rows && max_pos < 1)) return MMHIP_E_INVALID;
    if (off16({dx, xhat, gamma, det_rows}) || (((uintptr_t)row_state | (uintptr_t)status | (uintptr_t)partial) & 3)) return MMHIP_E_INVALID;
    if (partial && partial_bytes < mmhip_op_embed_bwd_ws_bytes(posts, T, H, type_rows)) return MMHIP_E_CAPACITY;
    EmbedBwdArgs b{};
    b.dx = dx; b.xhat = xhat; b.rstd = rstd; b.gamma = gamma; b.ids = ids; b.pos_ids = pos_ids; b.type_ids = type_ids; b.type_rows = type_rows;
    b.dword = dword; b.dpos = dpos; b.dtype = dtype_rows; b.dgamma = dgamma; b.dbeta = dbeta;
    b.posts = posts; b.T = T; b.H = H; b.pad_id = pad_id; b.pos_pad_id = pos_pad_id;
    b.drop = make_drop(p, seed, STREAM_EMBED, 1);
    b.partial = (float*)partial; b.alpha = alpha; b.row_state = row_state; b.det_rows = det_rows; b.max_pos = max_pos; b.status = status;
    const hipError_t r = launch_embed_bwd(b, dtype, (hipStream_t)stream);
    return r == hipErrorInvalidValue ? MMHIP_E_INVALID : (int)r;
}

// ------------------------------------------------------------------------------------------------ global-norm gradient clipping
uint64_t mmhip_grad_clip_state_bytes(void) { return (uint64_t)grad_clip_state_bytes(); }
// everything from the gradients to the four public words; every argument is checked on the host before the first launch
int mmhip_op_grad_clip(const float* const* seg_g, const uint64_t* seg_n, int segments, const float* row_g, int rows, int width, const uint8_t* row_state,
                       float max_norm, float grad_scale, const uint32_t* guard_words2, void* clip_state, void* stream) {
    if (segments < 0 || segments > GRADNORM_MAX_SEGMENTS || (segments > 0 && (!seg_g || !seg_n))) return MMHIP_E_INVALID;
    if (!clip_state || ((uintptr_t)clip_state & 15) || ((uintptr_t)guard_words2 & 3)) return MMHIP_E_INVALID;
    if (!(max_norm > 0.f) || std::isinf(max_norm) || std::isnan(grad_scale) || std::isinf(grad_scale)) return MMHIP_E_INVALID;
    if (rows < 0 || (rows > 0 && (!row_g || !row_state || ((uintptr_t)row_g & 15) || width <= 0 || width % 4))) return MMHIP_E_INVALID;
    GradNormSegments sg{};
    for (int i = 0; i < segments; ++i) {
        if (!seg_g[i] || ((uintptr_t)seg_g[i] & 15)) return MMHIP_E_INVALID;
        sg.g[i] = seg_g[i]; sg.n[i] = (size_t)seg_n[i];
    }
    sg.count = segments;
    const hipError_t r = launch_grad_clip(sg, rows > 0 ? row_g : nullptr, rows, width, row_state, max_norm, grad_scale, guard_words2 ? guard_words2 + 1 : nullptr,
                                          clip_state, (hipStream_t)stream);
    return r == hipErrorInvalidValue ? MMHIP_E_INVALID : (int)r;
}

}  // extern "C"
