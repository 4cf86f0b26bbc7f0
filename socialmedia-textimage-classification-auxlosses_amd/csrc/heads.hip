// Head kernels (fp32 arithmetic; B posts is 64..128, so these are latency-sized, not roofline-sized):
//   * cross-modal attention fusion for the CLS query only (reference models/mm_late.py:98-113, :195-210):
//     only row 0 of softmax(Q K^T) V is consumed, and K = x_v W_K^T + b_K, V = x_v W_V^T + b_V are affine in the
//     frozen image tokens, so   scores_j = (W_K^T q) . x_v[j] (+ const),  ctx = W_V (sum_j p_j x_v[j]) + b_V
//     -- exact algebra, 0.47 GF/post of fc_K/fc_V GEMMs become two [B,768]x[768,768] products.
//   * aspect-att fusion (reference models/mm_late.py:115-131) on the two pooler outputs: a two-slot tanh / softmax mix per post, one wave per
//     post, and its backward with ordered partial sums for the two parameter gradients (at the end of this file)
//   * ITC similarity (HF vision_text_dual_encoder :261-274) and its backward
//   * fused loss forward+backward: weighted soft-target CE (run_mm_late.py:85), clip_loss (utils.py:225-231),
//     ITM CE (run_mm_late.py:97), mixed as models/mm_late.py:473-487
#include "mmhip_common.h"
#include "mmhip_kernels.h"

namespace mmhip {

__device__ __forceinline__ float block_reduce(float v, float* red, bool is_max) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    v = is_max ? wave_max(v) : wave_sum(v);
    __syncthreads();
    if (lane == 0) red[w] = v;
    __syncthreads();
    float r = red[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); ++i) r = is_max ? fmaxf(r, red[i]) : r + red[i];
    return r;
}

// ------------------------------------------------------------------------------------------------ fusion attention
// One workgroup per text post.  Each wave takes image tokens j = w, w+4, ...: a lane owns 12 of the 768 columns
// (three 8-byte loads per token, independent across tokens, so the loads pipeline), dots reduce across the wave,
// weighted sums accumulate in registers and are combined across the 4 waves through LDS.
// 8 waves per post: the kernel is a latency chain over 197 x 768 image tokens read twice (300 KB per workgroup, 64-128 workgroups)
// on the critical path between the towers and the backward; eight waves keep twice the token loads in flight of four (40 KB of LDS partials)
static constexpr int FA_WAVES = 8, FA_THREADS = FA_WAVES * 64;
template <typename T>
__global__ __launch_bounds__(FA_THREADS) void fusion_attn_fwd_kernel(FusionAttnArgs a) {
    __shared__ __attribute__((aligned(16))) float q[1024];
    __shared__ float sc[FA_THREADS];
    __shared__ float red[FA_WAVES];
    __shared__ float part[FA_WAVES][1024];
    const int bt = blockIdx.x, b = bt % a.B, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < a.H; c += FA_THREADS) q[c] = a.qk[(size_t)bt * a.H + c];
    __syncthreads();
    const T* xv = (const T*)a.xv + (size_t)b * a.P * a.H;
    const int nch = a.H >> 2;                   // 4-element chunks; lane owns chunks lane, lane+64, ...
    // dots of 4 tokens at a time per wave: the four wave reductions interleave, hiding the cross-lane latency
    for (int j0 = w * 4; j0 < a.P; j0 += 4 * FA_WAVES) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int ch = lane; ch < nch; ch += 64) {
            const f32x4 qq = *reinterpret_cast<const f32x4*>(q + ch * 4);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = min(j0 + u, a.P - 1);
                typename Vec<T>::v4 x = *reinterpret_cast<const typename Vec<T>::v4*>(xv + (size_t)j * a.H + ch * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[u] += to_f<T>(x[e]) * qq[e];
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] += __shfl_xor(s[u], o);
        if (lane < 4 && j0 + lane < a.P) sc[j0 + lane] = s[lane] * a.scale;
    }
    __syncthreads();
    const float v = threadIdx.x < a.P ? sc[threadIdx.x] : -INFINITY;
    const float mx = block_reduce(v, red, true);
    const float e = threadIdx.x < a.P ? __expf(v - mx) : 0.f;
    const float sum = block_reduce(e, red, false);
    if (threadIdx.x < a.P) {
        sc[threadIdx.x] = e / sum;
        a.prob[(size_t)bt * a.P + threadIdx.x] = e / sum;
    }
    __syncthreads();
    float acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int ee = 0; ee < 4; ++ee) acc[t][ee] = 0.f;
    for (int j = w; j < a.P; j += FA_WAVES) {
        const float p = sc[j];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int ch = lane + 64 * t;
            if (ch < nch) {
                typename Vec<T>::v4 x = *reinterpret_cast<const typename Vec<T>::v4*>(xv + (size_t)j * a.H + ch * 4);
#pragma unroll
                for (int ee = 0; ee < 4; ++ee) acc[t][ee] += p * to_f<T>(x[ee]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (lane + 64 * t < nch)
#pragma unroll
            for (int ee = 0; ee < 4; ++ee) part[w][(lane + 64 * t) * 4 + ee] = acc[t][ee];
    __syncthreads();
    for (int c = threadIdx.x; c < a.H; c += FA_THREADS) {
        float sres = 0.f;
#pragma unroll
        for (int ww = 0; ww < FA_WAVES; ++ww) sres += part[ww][c];
        a.xbar[(size_t)bt * a.H + c] = sres;
    }
}
template <typename T>
__global__ __launch_bounds__(FA_THREADS) void fusion_attn_bwd_kernel(FusionAttnBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float dxb[1024];
    __shared__ float ds[FA_THREADS];
    __shared__ float red[FA_WAVES];
    __shared__ float part[FA_WAVES][1024];
    const int bt = blockIdx.x, b = bt % a.B, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int c = threadIdx.x; c < a.H; c += FA_THREADS) dxb[c] = a.dxbar[(size_t)bt * a.H + c];
    __syncthreads();
    const T* xv = (const T*)a.xv + (size_t)b * a.P * a.H;
    const int nch = a.H >> 2;
    for (int j0 = w * 4; j0 < a.P; j0 += 4 * FA_WAVES) {
        float s[4] = {0.f, 0.f, 0.f, 0.f};
        for (int ch = lane; ch < nch; ch += 64) {
            const f32x4 qq = *reinterpret_cast<const f32x4*>(dxb + ch * 4);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = min(j0 + u, a.P - 1);
                typename Vec<T>::v4 x = *reinterpret_cast<const typename Vec<T>::v4*>(xv + (size_t)j * a.H + ch * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) s[u] += to_f<T>(x[e]) * qq[e];
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1)
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] += __shfl_xor(s[u], o);
        if (lane < 4 && j0 + lane < a.P) ds[j0 + lane] = s[lane];          // dp_j
    }
    __syncthreads();
    const float p = threadIdx.x < a.P ? a.prob[(size_t)bt * a.P + threadIdx.x] : 0.f;
    const float dp = threadIdx.x < a.P ? ds[threadIdx.x] : 0.f;
    const float tsum = block_reduce(p * dp, red, false);
    __syncthreads();
    if (threadIdx.x < a.P) ds[threadIdx.x] = p * (dp - tsum) * a.scale;
    __syncthreads();
    float acc[4][4];
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int ee = 0; ee < 4; ++ee) acc[t][ee] = 0.f;
    for (int j = w; j < a.P; j += FA_WAVES) {
        const float d = ds[j];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int ch = lane + 64 * t;
            if (ch < nch) {
                typename Vec<T>::v4 x = *reinterpret_cast<const typename Vec<T>::v4*>(xv + (size_t)j * a.H + ch * 4);
#pragma unroll
                for (int ee = 0; ee < 4; ++ee) acc[t][ee] += d * to_f<T>(x[ee]);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
        if (lane + 64 * t < nch)
#pragma unroll
            for (int ee = 0; ee < 4; ++ee) part[w][(lane + 64 * t) * 4 + ee] = acc[t][ee];
    __syncthreads();
    for (int c = threadIdx.x; c < a.H; c += FA_THREADS) {
        float sres = 0.f;
#pragma unroll
        for (int ww = 0; ww < FA_WAVES; ++ww) sres += part[ww][c];
        a.dqk[(size_t)bt * a.H + c] = sres;
    }
}

// ------------------------------------------------------------------------------------------------ ITC
// block b < B: normalise txt_e[b]; block B + b: normalise img_e[b]
__global__ __launch_bounds__(256) void itc_norm_kernel(ItcArgs a) {
    __shared__ float red[4];
    const int i = blockIdx.x % a.B;
    const bool img = blockIdx.x >= a.B;
    const float* e = (img ? a.img_e : a.txt_e) + (size_t)i * a.E;
    float s = 0.f;
    for (int c = threadIdx.x; c < a.E; c += 256) s += e[c] * e[c];
    const float inv = 1.0f / sqrtf(block_reduce(s, red, false));
    float* n = (img ? a.img_n : a.txt_n) + (size_t)i * a.E;
    for (int c = threadIdx.x; c < a.E; c += 256) n[c] = e[c] * inv;
    if (threadIdx.x == 0) (img ? a.img_inv : a.txt_inv)[i] = inv;
}
// logits_per_text[i][j] = txt_n[i] . img_n[j] * exp(logit_scale); one wave per (i, j)
__global__ __launch_bounds__(256) void itc_logits_kernel(ItcArgs a) {
    const int lane = threadIdx.x & 63;
    const int idx = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= a.B * a.B) return;
    const int i = idx / a.B, j = idx % a.B;
    float s = 0.f;
    for (int c = lane; c < a.E; c += 64) s += a.txt_n[(size_t)i * a.E + c] * a.img_n[(size_t)j * a.E + c];
    s = wave_sum(s);
    if (lane == 0) a.logits[idx] = s * __expf(a.logit_scale[0]);
}
// block b < B: d txt_e[b]; block B + b: d img_e[b]; block 0 also adds d logit_scale = sum dlogits * logits
__global__ __launch_bounds__(256) void itc_bwd_kernel(ItcBwdArgs a) {
    __shared__ float dn[1024];
    __shared__ float red[4];
    const int i = blockIdx.x % a.B;
    const bool img = blockIdx.x >= a.B;
    const float es = __expf(a.logit_scale[0]);
    const float* other = img ? a.txt_n : a.img_n;
    const float* mine = (img ? a.img_n : a.txt_n) + (size_t)i * a.E;
    float dot = 0.f;
    for (int c = threadIdx.x; c < a.E; c += 256) {
        float s = 0.f;
        for (int j = 0; j < a.B; ++j) {
            const float dl = img ? a.dlogits[(size_t)j * a.B + i] : a.dlogits[(size_t)i * a.B + j];
            s += dl * other[(size_t)j * a.E + c];
        }
        s *= es;
        dn[c] = s;
        dot += s * mine[c];
    }
    dot = block_reduce(dot, red, false);
    const float inv = (img ? a.img_inv : a.txt_inv)[i];
    float* out = (img ? a.dimg_e : a.dtxt_e) + (size_t)i * a.E;
    for (int c = threadIdx.x; c < a.E; c += 256) out[c] = (dn[c] - mine[c] * dot) * inv;
    if (blockIdx.x == 0 && a.dlogit_scale) {
        float s = 0.f;
        for (int k = threadIdx.x; k < a.B * a.B; k += 256) s += a.dlogits[k] * a.logits[k];
        s = block_reduce(s, red, false);
        if (threadIdx.x == 0) a.dlogit_scale[0] += s;
    }
}

// ------------------------------------------------------------------------------------------------ global-batch ITC
// Data parallelism with gathered embeddings: G = world * B posts, T_n / I_n [G, E] hold every rank's normalised rows in rank order, the logits
// S = exp(logit_scale) T_n I_n^T are G x G and the loss is clip_loss on S (utils.py:225-231).  G x G does not fit anywhere convenient (8192^2 fp32 =
// 256 MB), so S is never needed in memory: a workgroup owns one 32 x 32 tile, built like small_gemm_kernel's (exact fp32 on
// v_mfma_f32_32x32x2_f32, the K range split over the 8 waves, partial tiles summed through LDS in wave order), and leaves
//   forward   per tile-column tj an online-softmax pair (max, sum exp) of every row over the tile's 32 columns, per tile-row ti the same of every
//             column over its 32 rows, and the diagonal; itc_global_lse_kernel folds the G / 32 pairs of a row / column IN TILE ORDER into
//             rowlse / collse -- both log-sum-exps from one pass over S, every word has one writer, no atomics: the same bits on every call;
//   backward  the rank's strips of dS = scale (softmax_row + softmax_col - 2 I): rows [r0, r0 + Bl) x all columns (-> d T_n of the local texts, and
//             d logit_scale = sum dS S over that strip: the strips of the ranks tile S exactly once) and all rows x columns [r0, r0 + Bl)
//             (stored transposed, -> d I_n of the local images), recomputed from the gathered rows; the two [Bl, G] x [G, E] products that follow
//             are small_gemm launches.
static constexpr int IG_WAVES = 8, IG_THREADS = IG_WAVES * 64;
// tile[r][c] = es * T[i0 + r] . I[j0 + c] (rows / columns past G repeat row G - 1: finite, never stored).  Ends with a barrier.
__device__ __forceinline__ void itc_tile(const float* __restrict__ T, const float* __restrict__ I, int G, int E, int i0, int j0, float es,
                                         float (*red)[32][32], float (*tile)[33]) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const float* Tp = T + (size_t)min(i0 + r, G - 1) * E;
    const float* Ip = I + (size_t)min(j0 + r, G - 1) * E;
    f32x16 acc = f32x16{};
    for (int k0 = w * 8 + h * 4; k0 < E; k0 += 8 * IG_WAVES) {
        float av[4], bv[4];
        if (k0 + 3 < E && ((((uintptr_t)(Tp + k0)) | ((uintptr_t)(Ip + k0))) & 15) == 0) {
            const f32x4 ta = *reinterpret_cast<const f32x4*>(Tp + k0), tb = *reinterpret_cast<const f32x4*>(Ip + k0);
#pragma unroll
            for (int e = 0; e < 4; ++e) { av[e] = ta[e]; bv[e] = tb[e]; }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) { av[e] = k0 + e < E ? Tp[k0 + e] : 0.f; bv[e] = k0 + e < E ? Ip[k0 + e] : 0.f; }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], bv[e], acc, 0, 0, 0);
    }
    // D: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) red[w][(reg & 3) + 8 * (reg >> 2) + 4 * h][r] = acc[reg];
    __syncthreads();
    for (int i = threadIdx.x; i < 32 * 32; i += IG_THREADS) {
        const int row = i >> 5, col = i & 31;
        float v = 0.f;
#pragma unroll
        for (int ww = 0; ww < IG_WAVES; ++ww) v += red[ww][row][col];
        tile[row][col] = v * es;
    }
    __syncthreads();
}
__global__ __launch_bounds__(IG_THREADS) void itc_global_fwd_kernel(ItcGlobalArgs a, float* row_m, float* row_s, float* col_m, float* col_s, float* diag) {
    __shared__ float red[IG_WAVES][32][32];
    __shared__ float tile[32][33];
    const int tj = blockIdx.x, ti = blockIdx.y, i0 = ti * 32, j0 = tj * 32, G = a.G, t = threadIdx.x;
    itc_tile(a.txt_n, a.img_n, G, a.E, i0, j0, expf(a.logit_scale[0]), red, tile);
    const int nr = min(32, G - i0), nc = min(32, G - j0);
    if (a.logits)
        for (int i = t; i < 32 * 32; i += IG_THREADS) {
            const int row = i >> 5, col = i & 31;
            if (row < nr && col < nc) a.logits[(size_t)(i0 + row) * G + j0 + col] = tile[row][col];
        }
    if (t < 32) {                     // row t of the tile over its columns
        if (t < nr) {
            float m = -INFINITY, s = 0.f;
            for (int c = 0; c < nc; ++c) m = fmaxf(m, tile[t][c]);
            for (int c = 0; c < nc; ++c) s += expf(tile[t][c] - m);
            row_m[(size_t)tj * G + i0 + t] = m; row_s[(size_t)tj * G + i0 + t] = s;
        }
    } else if (t < 64) {              // column t - 32 over its rows
        const int c = t - 32;
        if (c < nc) {
            float m = -INFINITY, s = 0.f;
            for (int r = 0; r < nr; ++r) m = fmaxf(m, tile[r][c]);
            for (int r = 0; r < nr; ++r) s += expf(tile[r][c] - m);
            col_m[(size_t)ti * G + j0 + c] = m; col_s[(size_t)ti * G + j0 + c] = s;
        }
    } else if (t < 96 && ti == tj) {
        if (t - 64 < nr) diag[i0 + t - 64] = tile[t - 64][t - 64];
    }
}
// one thread per index i: rowlse[i], collse[i], term[i] = (rowlse[i] - S_ii) + (collse[i] - S_ii)
__global__ __launch_bounds__(256) void itc_global_lse_kernel(ItcGlobalArgs a, const float* row_m, const float* row_s, const float* col_m, const float* col_s,
                                                             const float* diag, float* term) {
    const int i = blockIdx.x * 256 + threadIdx.x, G = a.G, nt = (G + 31) / 32;
    if (i >= G) return;
    float lse[2];
#pragma unroll
    for (int d = 0; d < 2; ++d) {
        const float* pm = d ? col_m : row_m;
        const float* ps = d ? col_s : row_s;
        float m = -INFINITY, s = 0.f;
        for (int t = 0; t < nt; ++t) m = fmaxf(m, pm[(size_t)t * G + i]);
        for (int t = 0; t < nt; ++t) s += ps[(size_t)t * G + i] * expf(pm[(size_t)t * G + i] - m);
        lse[d] = m + logf(s);
    }
    a.rowlse[i] = lse[0]; a.collse[i] = lse[1];
    term[i] = (lse[0] - diag[i]) + (lse[1] - diag[i]);
}
// loss = sum_i term[i] / (2 G): one block, fixed order
__global__ __launch_bounds__(256) void itc_global_loss_kernel(const float* term, int G, float* loss) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < G; i += 256) s += term[i];
    s = block_reduce(s, red, false);
    if (threadIdx.x == 0) loss[0] = s / (2.f * G);
}
// blockIdx.z = 0: text rows [r0, r0 + Bl) x image columns tile blockIdx.x -> grow [Bl, G], dls_part;  1: text rows tile blockIdx.x x image columns
// [r0, r0 + Bl) -> gcol [Bl, G] (transposed).  Entries are dS * es: the factor of d(S)/d(T_n I_n^T)
__global__ __launch_bounds__(IG_THREADS) void itc_global_grad_kernel(ItcGlobalBwdArgs a, float* grow, float* gcol, float* dls_part) {
    __shared__ float red[IG_WAVES][32][32];
    __shared__ float tile[32][33];
    __shared__ float rsum[IG_WAVES];
    const bool colside = blockIdx.z != 0;
    const int G = a.G, t = threadIdx.x, hi = a.r0 + a.Bl;
    const int i0 = colside ? blockIdx.x * 32 : a.r0 + blockIdx.y * 32, j0 = colside ? a.r0 + blockIdx.y * 32 : blockIdx.x * 32;
    const float es = expf(a.logit_scale[0]);
    itc_tile(a.txt_n, a.img_n, G, a.E, i0, j0, es, red, tile);
    float part = 0.f;
    for (int i = t; i < 32 * 32; i += IG_THREADS) {
        // consecutive threads walk the long (all-G) direction of the strip: coalesced stores on both sides
        const int row = colside ? (i & 31) : (i >> 5), col = colside ? (i >> 5) : (i & 31);
        const int gi = i0 + row, gj = j0 + col;
        if (gi >= (colside ? G : hi) || gj >= (colside ? hi : G)) continue;
        const float s = tile[row][col];
        const float g = (expf(s - a.rowlse[gi]) + expf(s - a.collse[gj]) - (gi == gj ? 2.f : 0.f)) * a.scale;
        if (colside) gcol[(size_t)(gj - a.r0) * G + gi] = g * es;
        else { grow[(size_t)(gi - a.r0) * G + gj] = g * es; part += g * s; }
    }
    if (!colside) {
        part = block_reduce(part, rsum, false);
        if (t == 0) dls_part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = part;
    }
}
// block b < Bl: text row r0 + b, block Bl + b: image row r0 + b -- d e = (d n - n (d n . n)) / |e|; block 0 adds the ordered sum of dls_part
__global__ __launch_bounds__(256) void itc_global_normbwd_kernel(ItcGlobalBwdArgs a, const float* dls_part, int n_part) {
    __shared__ float red[4];
    const int i = blockIdx.x % a.Bl;
    const bool img = blockIdx.x >= a.Bl;
    float* out = img ? a.dimg_e : a.dtxt_e;
    if (out) {
        const float* mine = (img ? a.img_n : a.txt_n) + (size_t)(a.r0 + i) * a.E;
        const float* dn = (img ? a.d_img_n : a.d_txt_n) + (size_t)i * a.E;
        float dot = 0.f;
        for (int c = threadIdx.x; c < a.E; c += 256) dot += dn[c] * mine[c];
        dot = block_reduce(dot, red, false);
        const float inv = (img ? a.img_inv : a.txt_inv)[i];
        for (int c = threadIdx.x; c < a.E; c += 256) out[(size_t)i * a.E + c] = (dn[c] - mine[c] * dot) * inv;
    }
    if (blockIdx.x == 0 && a.dlogit_scale) {
        float s = 0.f;
        for (int k = threadIdx.x; k < n_part; k += 256) s += dls_part[k];
        s = block_reduce(s, red, false);
        if (threadIdx.x == 0) a.dlogit_scale[0] += s;
    }
}

// ------------------------------------------------------------------------------------------------ losses (one block)
__global__ __launch_bounds__(256) void loss_kernel(LossArgs a) {
    __shared__ float red[4];
    __shared__ float rowlse[1024], collse[1024];
    const int B = a.B, C = a.C, t = threadIdx.x;
    // ---- classification: -(1/B) sum_b sum_c w_c y_bc log_softmax(out)_bc   (soft-target CE, normalised by B)
    float lc = 0.f;
    int correct = 0;
    for (int b = t; b < B; b += 256) {
        const float* z = a.out_cls + (size_t)b * C;
        float mx = -INFINITY;
        int am = 0, ay = 0;
        long ymax = -1;
        for (int c = 0; c < C; ++c) {
            if (z[c] > mx) { mx = z[c]; am = c; }
            const long y = a.onehot[(size_t)b * C + c];
            if (y > ymax) { ymax = y; ay = c; }
        }
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += __expf(z[c] - mx);
        const float lse = mx + __logf(se);
        float wy = 0.f;
        for (int c = 0; c < C; ++c) {
            const float w = a.class_w ? a.class_w[c] : 1.f;
            const float y = (float)a.onehot[(size_t)b * C + c];
            lc -= w * y * (z[c] - lse);
            wy += w * y;
        }
        if (a.d_out_cls)
            for (int c = 0; c < C; ++c) {
                const float w = a.class_w ? a.class_w[c] : 1.f;
                const float y = (float)a.onehot[(size_t)b * C + c];
                a.d_out_cls[(size_t)b * C + c] = a.w_cls * (__expf(z[c] - lse) * wy - w * y) / B;
            }
        correct += (am == ay);
    }
    lc = block_reduce(lc, red, false) / B;
    const float fc = block_reduce((float)correct, red, false);
    // ---- ITC: (CE(S, arange) + CE(S^T, arange)) / 2
    float li = 0.f;
    if (a.logits_per_text) {
        const float* S = a.logits_per_text;
        for (int i = t; i < B; i += 256) {
            float mr = -INFINITY, mc = -INFINITY;
            for (int j = 0; j < B; ++j) { mr = fmaxf(mr, S[(size_t)i * B + j]); mc = fmaxf(mc, S[(size_t)j * B + i]); }
            float sr = 0.f, scn = 0.f;
            for (int j = 0; j < B; ++j) { sr += __expf(S[(size_t)i * B + j] - mr); scn += __expf(S[(size_t)j * B + i] - mc); }
            rowlse[i] = mr + __logf(sr);
            collse[i] = mc + __logf(scn);
            li += (rowlse[i] - S[(size_t)i * B + i]) + (collse[i] - S[(size_t)i * B + i]);
        }
        li = block_reduce(li, red, false) / (2.f * B);
        __syncthreads();
        if (a.d_logits)
            for (int k = t; k < B * B; k += 256) {
                const int i = k / B, j = k % B;
                const float s = S[k];
                a.d_logits[k] = a.w_itc * (__expf(s - rowlse[i]) + __expf(s - collse[j]) - (i == j ? 2.f : 0.f)) / (2.f * B);
            }
    } else if (a.itc_global_loss) {
        li = a.itc_global_loss[0];      // global-batch ITC: the loss over the gathered G x G logits (launch_itc_global_fwd); its gradient is launch_itc_global_bwd's
    }
    // ---- ITM: index-target CE, mean
    float lm = 0.f;
    if (a.out_tim) {
        for (int b = t; b < B; b += 256) {
            const float z0 = a.out_tim[b * 2], z1 = a.out_tim[b * 2 + 1];
            const float mx = fmaxf(z0, z1), lse = mx + __logf(__expf(z0 - mx) + __expf(z1 - mx));
            const int y = (int)a.lbl_tim[b];
            lm += lse - (y ? z1 : z0);
            if (a.d_out_tim) {
                a.d_out_tim[b * 2] = a.w_itm * (__expf(z0 - lse) - (y == 0 ? 1.f : 0.f)) / B;
                a.d_out_tim[b * 2 + 1] = a.w_itm * (__expf(z1 - lse) - (y == 1 ? 1.f : 0.f)) / B;
            }
        }
        lm = block_reduce(lm, red, false) / B;
    }
    if (t == 0) {
        a.loss[0] = a.w_cls * lc + ((a.logits_per_text || a.itc_global_loss) ? a.w_itc * li : 0.f) + (a.out_tim ? a.w_itm * lm : 0.f);
        a.loss[1] = lc; a.loss[2] = li; a.loss[3] = lm;
        if (a.n_correct) a.n_correct[0] = (int)(fc + 0.5f);
    }
}

// ------------------------------------------------------------------------------------------------ small elementwise
__global__ __launch_bounds__(256) void elementwise_kernel(int op, const float* a, const float* b, float* out, size_t n, float alpha, DropCfg drop) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        float v;
        switch (op) {
            case EW_TANH_BWD: v = a[i] * (1.f - b[i] * b[i]); break;             // a = dy, b = y
            case EW_RELU_BWD: v = b[i] > 0.f ? a[i] : 0.f; break;                // a = dy, b = y
            case EW_DROPOUT: v = (drop.thresh16 && !mm_keep((uint32_t)i, drop)) ? 0.f : a[i] * (drop.thresh16 ? drop.keep_scale : 1.f); break;
            case EW_ADD: v = a[i] + alpha * b[i]; break;
            default: v = a[i]; break;
        }
        out[i] = v;
    }
}
// out[c] (+)= sum_r d[r][c], fp32, small row counts
__global__ __launch_bounds__(256) void bias_grad_f32_kernel(const float* d, int rows, int cols, int ld, float* out, int accumulate) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    float s = 0.f;
    for (int r = 0; r < rows; ++r) s += d[(size_t)r * ld + c];
    out[c] = accumulate ? out[c] + s : s;
}

// ------------------------------------------------------------------------------------------------ fused AdamW
// torch.optim.AdamW semantics (decoupled decay first, then moments; models/mm_late.py:420-422) over one flat fp32 buffer.
// a gradient element that is inf / NaN (f16 mode: an overflow in the 16-bit gradient chain) must not reach m / v / p: it is read as
// 0 and counted; the trainer lowers the loss scale / raises when the counter moves (MMLate_Model.train)
__device__ __forceinline__ float guard_finite(float g, bool& bad) {
    const bool ok = fabsf(g) <= 3.4028234e38f;       // false for NaN
    bad = bad || !ok;
    return ok ? g : 0.f;
}
__global__ __launch_bounds__(256) void adamw_kernel(AdamWArgs a) {
    const size_t n4 = a.n / 4;
    if (a.skip && *a.skip) {          // the step is void: leave p / m / v alone, clear the gradient for the next step
        if (a.zero_grad) {
            for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) reinterpret_cast<f32x4*>(a.g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) a.g[n4 * 4 + threadIdx.x] = 0.f;
        }
        return;
    }
    bool bad = false;
    const float one_m_b1 = 1.f - a.beta1, one_m_b2 = 1.f - a.beta2;
    const float decay = 1.f - a.lr * a.wd, step = a.lr / a.bc1;
    const float gscale = a.clip ? a.grad_scale * *a.clip : a.grad_scale;          // global-norm clipping: the coefficient of launch_grad_clip
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        f32x4 p = reinterpret_cast<f32x4*>(a.p)[i], g = reinterpret_cast<f32x4*>(a.g)[i];
        f32x4 m = reinterpret_cast<f32x4*>(a.m)[i], v = reinterpret_cast<f32x4*>(a.v)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float ge = guard_finite(g[e] * gscale, bad);
            p[e] *= decay;
            m[e] = m[e] + one_m_b1 * (ge - m[e]);
            v[e] = v[e] * a.beta2 + one_m_b2 * ge * ge;
            const float denom = sqrtf(v[e]) / a.bc2_sqrt + a.eps;
            p[e] -= step * (m[e] / denom);
        }
        reinterpret_cast<f32x4*>(a.p)[i] = p;
        reinterpret_cast<f32x4*>(a.m)[i] = m;
        reinterpret_cast<f32x4*>(a.v)[i] = v;
        if (a.zero_grad) reinterpret_cast<f32x4*>(a.g)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    if (blockIdx.x == 0 && threadIdx.x < (a.n & 3)) {          // the n & 3 tail: its non-finite elements count with the thread's others
        const size_t i = n4 * 4 + threadIdx.x;
        const float ge = guard_finite(a.g[i] * gscale, bad);
        float p = a.p[i] * decay;
        const float m = a.m[i] + one_m_b1 * (ge - a.m[i]);
        const float v = a.v[i] * a.beta2 + one_m_b2 * ge * ge;
        p -= step * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
        a.p[i] = p; a.m[i] = m; a.v[i] = v;
        if (a.zero_grad) a.g[i] = 0.f;
    }
    if (bad && a.nonfinite) atomicAdd(a.nonfinite, 1u);
}

// ------------------------------------------------------------------------------------------------ launchers
hipError_t launch_fusion_attn_fwd(const FusionAttnArgs& a, int dtype, hipStream_t s) {
    if (a.Bt <= 0) return hipSuccess;
    if (a.P > FA_THREADS || a.H > 1024 || a.H % 4) return hipErrorInvalidValue;
    if (dtype == DT_BF16) hipLaunchKernelGGL(fusion_attn_fwd_kernel<bf16_t>, dim3(a.Bt), dim3(FA_THREADS), 0, s, a);
    else if (dtype == DT_F16) hipLaunchKernelGGL(fusion_attn_fwd_kernel<f16_t>, dim3(a.Bt), dim3(FA_THREADS), 0, s, a);
    else hipLaunchKernelGGL(fusion_attn_fwd_kernel<float>, dim3(a.Bt), dim3(FA_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_fusion_attn_bwd(const FusionAttnBwdArgs& a, int dtype, hipStream_t s) {
    if (a.Bt <= 0) return hipSuccess;
    if (a.P > FA_THREADS || a.H > 1024 || a.H % 4) return hipErrorInvalidValue;
    if (dtype == DT_BF16) hipLaunchKernelGGL(fusion_attn_bwd_kernel<bf16_t>, dim3(a.Bt), dim3(FA_THREADS), 0, s, a);
    else if (dtype == DT_F16) hipLaunchKernelGGL(fusion_attn_bwd_kernel<f16_t>, dim3(a.Bt), dim3(FA_THREADS), 0, s, a);
    else hipLaunchKernelGGL(fusion_attn_bwd_kernel<float>, dim3(a.Bt), dim3(FA_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_itc_fwd(const ItcArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    hipLaunchKernelGGL(itc_norm_kernel, dim3(2 * a.B), dim3(256), 0, s, a);
    hipLaunchKernelGGL(itc_logits_kernel, dim3((a.B * a.B + 3) / 4), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_itc_bwd(const ItcBwdArgs& a, hipStream_t s) {
    if (a.B <= 0) return hipSuccess;
    if (a.E > 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(itc_bwd_kernel, dim3(2 * a.B), dim3(256), 0, s, a);
    return hipGetLastError();
}
// fp32 words of ItcGlobalArgs::ws / ItcGlobalBwdArgs::ws: forward -- the (max, sum) pairs of both directions per 32-wide tile [4][G / 32][G], the
// diagonal [G], the loss terms [G]; backward -- the two dS strips [2][Bl][G] and the d logit_scale partial of every tile of the row strip
static size_t itc_global_fwd_words(int G) { return (size_t)(4 * ((G + 31) / 32) + 2) * G; }
size_t itc_global_ws_floats(int G, int Bl) { return itc_global_fwd_words(G) + 2 * (size_t)Bl * G + (size_t)((Bl + 31) / 32) * ((G + 31) / 32); }
static bool itc_global_shape_ok(int G, int E) { return G >= 1 && G <= ITC_GLOBAL_MAX_G && E >= 1 && E <= 1024; }
hipError_t launch_itc_global_fwd(const ItcGlobalArgs& a, hipStream_t s) {
    if (!itc_global_shape_ok(a.G, a.E) || !a.txt_n || !a.img_n || !a.logit_scale || !a.rowlse || !a.collse || !a.loss || !a.ws) return hipErrorInvalidValue;
    const int G = a.G, nt = (G + 31) / 32;
    const size_t pg = (size_t)nt * G;
    float *row_m = a.ws, *row_s = row_m + pg, *col_m = row_s + pg, *col_s = col_m + pg, *diag = col_s + pg, *term = diag + G;
    hipLaunchKernelGGL(itc_global_fwd_kernel, dim3(nt, nt), dim3(IG_THREADS), 0, s, a, row_m, row_s, col_m, col_s, diag);
    hipLaunchKernelGGL(itc_global_lse_kernel, dim3((G + 255) / 256), dim3(256), 0, s, a, row_m, row_s, col_m, col_s, diag, term);
    hipLaunchKernelGGL(itc_global_loss_kernel, dim3(1), dim3(256), 0, s, term, G, a.loss);
    return hipGetLastError();
}
hipError_t launch_itc_global_bwd(const ItcGlobalBwdArgs& a, hipStream_t s) {
    if (!itc_global_shape_ok(a.G, a.E) || a.Bl < 1 || a.r0 < 0 || (long)a.r0 + a.Bl > a.G) return hipErrorInvalidValue;
    if (!a.txt_n || !a.img_n || !a.logit_scale || !a.rowlse || !a.collse || !a.d_txt_n || !a.d_img_n || !a.ws) return hipErrorInvalidValue;
    if ((a.dtxt_e && !a.txt_inv) || (a.dimg_e && !a.img_inv)) return hipErrorInvalidValue;
    const int G = a.G, E = a.E, Bl = a.Bl, nt = (G + 31) / 32, nbl = (Bl + 31) / 32;
    float *grow = a.ws + itc_global_fwd_words(G), *gcol = grow + (size_t)Bl * G, *dls_part = gcol + (size_t)Bl * G;
    hipLaunchKernelGGL(itc_global_grad_kernel, dim3(nt, nbl, 2), dim3(IG_THREADS), 0, s, a, grow, gcol, dls_part);
    // d T_n[local] = grow . I_n, d I_n[local] = gcol . T_n: [Bl, G] x [G, E], exact fp32
    SmallGemmArgs g{};
    g.A = grow; g.lda = G; g.W = a.img_n; g.ldw = E; g.out = a.d_txt_n; g.ldo = E; g.M = Bl; g.N = E; g.K = G;
    hipError_t r = launch_small_nn(g, s);
    if (r != hipSuccess) return r;
    g.A = gcol; g.W = a.txt_n; g.out = a.d_img_n;
    r = launch_small_nn(g, s);
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(itc_global_normbwd_kernel, dim3(2 * Bl), dim3(256), 0, s, a, dls_part, nbl * nt);
    return hipGetLastError();
}
hipError_t launch_loss(const LossArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.B > 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_elementwise(int op, const float* a, const float* b, float* out, size_t n, float alpha, const DropCfg& drop, hipStream_t s) {
    if (!n) return hipSuccess;
    size_t g = (n + 255) / 256;
    hipLaunchKernelGGL(elementwise_kernel, dim3((int)(g > 4096 ? 4096 : g)), dim3(256), 0, s, op, a, b, out, n, alpha, drop);
    return hipGetLastError();
}
hipError_t launch_bias_grad_f32(const float* d, int rows, int cols, int ld, float* out, int accumulate, hipStream_t s) {
    if (cols <= 0) return hipSuccess;
    hipLaunchKernelGGL(bias_grad_f32_kernel, dim3((cols + 255) / 256), dim3(256), 0, s, d, rows, cols, ld, out, accumulate);
    return hipGetLastError();
}
// Row-lazy variant for embedding tables (the word table is 69 % of Bernice's parameters and <= B*T of its 250 002 rows see
// a gradient per step).  One wave per row per iteration; the state byte is wave-uniform.
//   state 0                : g = m = v = 0  ->  p *= (1 - lr*wd)   (exactly what the dense kernel computes; 8 B/param)
//   ROW_HAS_GRAD           : full update, gradient cleared, state -> ROW_HAS_MOMENTS
//   ROW_HAS_MOMENTS only   : full update with g = 0 (gradient neither read nor cleared)
__global__ __launch_bounds__(256) void adamw_rows_kernel(AdamWArgs a, int rows, int width, uint8_t* __restrict__ state) {
    const int lane = threadIdx.x & 63;
    const int nch = width >> 2;
    const float one_m_b1 = 1.f - a.beta1, one_m_b2 = 1.f - a.beta2;
    const float decay = 1.f - a.lr * a.wd, step = a.lr / a.bc1;
    bool bad = false;
    const float gscale = a.clip ? a.grad_scale * *a.clip : a.grad_scale;
    if (a.skip && *a.skip) {          // void step: rows that received a gradient lose it (and the flag), nothing else moves
        for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
            const int st = state[row];
            if (!(st & ROW_HAS_GRAD) || !a.zero_grad) continue;
            f32x4* __restrict__ g4 = reinterpret_cast<f32x4*>(a.g + (size_t)row * width);
            for (int c = lane; c < nch; c += 64) g4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (lane == 0) state[row] = (uint8_t)(st & ~ROW_HAS_GRAD);
        }
        return;
    }
    for (int row = blockIdx.x * 4 + (threadIdx.x >> 6); row < rows; row += gridDim.x * 4) {
        const int st = state[row];
        f32x4* __restrict__ p4 = reinterpret_cast<f32x4*>(a.p + (size_t)row * width);
        // 1 - lr*wd rounds to exactly 1.0f whenever lr*wd < 2^-24 -- true for the reference's defaults (1e-5 x 2.5e-4 = 2.5e-9;
        // torch's own param.mul_(1 - lr*wd) multiplies fp32 parameters by exactly 1.0f there): the decay-only rows are then
        // bit-identical without being read or written at all (1.5 GB of traffic per step for Bernice's word table)
        if (st == 0 && decay == 1.0f) continue;
        if (st == 0) {
            for (int c = lane; c < nch; c += 64) {
                f32x4 p = p4[c];
#pragma unroll
                for (int e = 0; e < 4; ++e) p[e] *= decay;
                p4[c] = p;
            }
            continue;
        }
        f32x4* __restrict__ g4 = reinterpret_cast<f32x4*>(a.g + (size_t)row * width);
        f32x4* __restrict__ m4 = reinterpret_cast<f32x4*>(a.m + (size_t)row * width);
        f32x4* __restrict__ v4 = reinterpret_cast<f32x4*>(a.v + (size_t)row * width);
        const bool has_g = st & ROW_HAS_GRAD;
        for (int c = lane; c < nch; c += 64) {
            f32x4 p = p4[c], m = m4[c], v = v4[c];
            f32x4 g = has_g ? g4[c] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ge = guard_finite(g[e] * gscale, bad);
                p[e] *= decay;
                m[e] = m[e] + one_m_b1 * (ge - m[e]);
                v[e] = v[e] * a.beta2 + one_m_b2 * ge * ge;
                const float denom = sqrtf(v[e]) / a.bc2_sqrt + a.eps;
                p[e] -= step * (m[e] / denom);
            }
            p4[c] = p; m4[c] = m; v4[c] = v;
            if (has_g && a.zero_grad) g4[c] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const int nst = ROW_HAS_MOMENTS | ((has_g && !a.zero_grad) ? ROW_HAS_GRAD : 0);
        if (lane == 0 && nst != st) state[row] = (uint8_t)nst;
    }
    if (bad && a.nonfinite) atomicAdd(a.nonfinite, 1u);
}
hipError_t launch_adamw_rows(const AdamWArgs& a, int rows, int width, uint8_t* row_state, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (width % 4 || !row_state) return hipErrorInvalidValue;
    const int g = (rows + 3) / 4;
    hipLaunchKernelGGL(adamw_rows_kernel, dim3(g > 16384 ? 16384 : g), dim3(256), 0, s, a, rows, width, row_state);
    return hipGetLastError();
}
hipError_t launch_adamw(const AdamWArgs& a, hipStream_t s) {
    if (!a.n) return hipSuccess;
    size_t g = (a.n / 4 + 255) / 256;
    hipLaunchKernelGGL(adamw_kernel, dim3((int)(g < 1 ? 1 : (g > 16384 ? 16384 : g))), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ fused CLS classifier head (text-only model)
// Latency-bound: B x C x H is a few hundred thousand multiply-adds.  The late-fusion head spends ~20 launches here; this is one per direction.
// element c of CLS row b, any of the storage forms the text tower leaves its last hidden state in (wave-uniform branch)
__device__ __forceinline__ float cls_head_load(const ClsHeadArgs& a, int b, int c) {
    const size_t off = (size_t)b * a.x_stride;
    if (a.x_dtype == DT_BF16) return (float)reinterpret_cast<const bf16_t*>(a.x)[off + c];
    if (a.x_dtype == DT_F16) return (float)reinterpret_cast<const f16_t*>(a.x)[off + c];
    if (a.x_dtype == DT_F32) return reinterpret_cast<const float*>(a.x)[off + c];
    const bf16_t* p = reinterpret_cast<const bf16_t*>(a.x) + 2 * off;          // plane pair: [hi(H) | lo(H)]
    return (float)p[c] + (float)p[a.H + c];
}
// Forward: one wave per post, 16 waves per block.  A lane keeps its H / 64 elements of the dropped row in registers and walks the C rows of W.
// With labels the launch is ONE block: its waves sum their posts' loss terms in post order, thread 0 adds the 16 wave sums in wave order.
static constexpr int CLS_HEAD_WAVES = 16;
__global__ __launch_bounds__(1024) void cls_head_fwd_kernel(ClsHeadArgs a) {
    __shared__ float s_loss[CLS_HEAD_WAVES];
    __shared__ int s_corr[CLS_HEAD_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int H = a.H, C = a.C;
    float lsum = 0.f;
    int corr = 0;
    for (int b = blockIdx.x * CLS_HEAD_WAVES + w; b < a.B; b += gridDim.x * CLS_HEAD_WAVES) {
        float xv[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = lane + 64 * j;
            float v = 0.f;
            if (c < H) {
                v = cls_head_load(a, b, c);
                if (a.drop.thresh16) v = mm_keep((uint32_t)b * (uint32_t)H + (uint32_t)c, a.drop) ? v * a.drop.keep_scale : 0.f;
            }
            xv[j] = v;
        }
        float z[CLS_HEAD_MAX_C];
#pragma unroll
        for (int k = 0; k < CLS_HEAD_MAX_C; ++k) {
            z[k] = 0.f;
            if (k < C) {
                const float* wr = a.W + (size_t)k * H;
                float acc = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int c = lane + 64 * j;
                    if (c < H) acc = fmaf(xv[j], wr[c], acc);
                }
                z[k] = wave_sum(acc) + a.bias[k];
                if (lane == 0) a.logits[(size_t)b * C + k] = z[k];
            }
        }
        if (a.onehot) {          // every lane holds all logits: the post's loss term, wave-uniform
            float mx = -INFINITY;
            int am = 0, ay = 0;
            long ymax = -1;
#pragma unroll
            for (int k = 0; k < CLS_HEAD_MAX_C; ++k)
                if (k < C) {
                    if (z[k] > mx) { mx = z[k]; am = k; }
                    const long y = a.onehot[(size_t)b * C + k];
                    if (y > ymax) { ymax = y; ay = k; }
                }
            float se = 0.f;
#pragma unroll
            for (int k = 0; k < CLS_HEAD_MAX_C; ++k) if (k < C) se += __expf(z[k] - mx);
            const float lse = mx + __logf(se);
            float wy = 0.f, lc = 0.f;
#pragma unroll
            for (int k = 0; k < CLS_HEAD_MAX_C; ++k)
                if (k < C) {
                    const float cw = a.class_w ? a.class_w[k] : 1.f;
                    const float y = (float)a.onehot[(size_t)b * C + k];
                    lc -= cw * y * (z[k] - lse);
                    wy += cw * y;
                }
            if (a.d_logits_out && lane == 0) {
#pragma unroll
                for (int k = 0; k < CLS_HEAD_MAX_C; ++k)
                    if (k < C) {
                        const float cw = a.class_w ? a.class_w[k] : 1.f;
                        const float y = (float)a.onehot[(size_t)b * C + k];
                        a.d_logits_out[(size_t)b * C + k] = (__expf(z[k] - lse) * wy - cw * y) / (float)a.B;
                    }
            }
            lsum += lc;
            corr += (am == ay);
        }
    }
    if (!a.onehot) return;
    if (lane == 0) { s_loss[w] = lsum; s_corr[w] = corr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        int n = 0;
        for (int i = 0; i < CLS_HEAD_WAVES; ++i) { t += s_loss[i]; n += s_corr[i]; }
        if (a.loss) a.loss[0] = t / (float)a.B;
        if (a.n_correct) a.n_correct[0] = n;
    }
}
// Backward: a block owns 64 columns of H; its four waves take the posts b = w, w + 4, ... and a thread one column: dW[:, h] in registers
// (x dropped again from the hash), dx[b, h] written as it goes; the four partial dW columns are added through LDS in wave order.
__global__ __launch_bounds__(256) void cls_head_bwd_kernel(ClsHeadArgs a) {
    __shared__ float red[4][CLS_HEAD_MAX_C][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int H = a.H, C = a.C, h = blockIdx.x * 64 + lane;
    float acc[CLS_HEAD_MAX_C], wr[CLS_HEAD_MAX_C];
#pragma unroll
    for (int k = 0; k < CLS_HEAD_MAX_C; ++k) { acc[k] = 0.f; wr[k] = k < C ? a.W[(size_t)k * H + h] : 0.f; }
    for (int b = w; b < a.B; b += 4) {
        float xd = cls_head_load(a, b, h);
        bool keep = true;
        if (a.drop.thresh16) {
            keep = mm_keep((uint32_t)b * (uint32_t)H + (uint32_t)h, a.drop);
            xd = keep ? xd * a.drop.keep_scale : 0.f;
        }
        float dxv = 0.f;
#pragma unroll
        for (int k = 0; k < CLS_HEAD_MAX_C; ++k)
            if (k < C) {
                const float dl = a.d_logits[(size_t)b * C + k];
                acc[k] = fmaf(dl, xd, acc[k]);
                dxv = fmaf(dl, wr[k], dxv);
            }
        if (a.drop.thresh16) dxv = keep ? dxv * a.drop.keep_scale : 0.f;
        dxv *= a.dx_scale;
        if (a.dx) {
            const size_t o = (size_t)b * a.dx_stride + h;
            if (a.dx_dtype == DT_BF16) reinterpret_cast<bf16_t*>(a.dx)[o] = (bf16_t)dxv;
            else if (a.dx_dtype == DT_F16) reinterpret_cast<f16_t*>(a.dx)[o] = (f16_t)dxv;
            else reinterpret_cast<float*>(a.dx)[o] = dxv;
        }
    }
#pragma unroll
    for (int k = 0; k < CLS_HEAD_MAX_C; ++k) red[w][k][lane] = acc[k];
    __syncthreads();
    if (w == 0 && a.dW) {
#pragma unroll
        for (int k = 0; k < CLS_HEAD_MAX_C; ++k)
            if (k < C) {
                const float v = ((red[0][k][lane] + red[1][k][lane]) + red[2][k][lane]) + red[3][k][lane];
                float* dst = a.dW + (size_t)k * H + h;
                *dst = a.accumulate ? *dst + v : v;
            }
    }
    if (blockIdx.x == 0 && w == 1 && lane < C && a.db) {
        float sb = 0.f;
        for (int b = 0; b < a.B; ++b) sb += a.d_logits[(size_t)b * C + lane];
        a.db[lane] = a.accumulate ? a.db[lane] + sb : sb;
    }
}
static bool cls_head_shape_ok(const ClsHeadArgs& a) {
    return a.B >= 1 && a.C >= 1 && a.C <= CLS_HEAD_MAX_C && a.H >= 64 && a.H <= 1024 && a.H % 64 == 0 && a.x && a.W && a.x_stride >= (size_t)a.H &&
           (a.x_dtype == DT_BF16 || a.x_dtype == DT_F16 || a.x_dtype == DT_F32 || a.x_dtype == DT_PAIR);
}
hipError_t launch_cls_head_fwd(const ClsHeadArgs& a, hipStream_t s) {
    if (!cls_head_shape_ok(a) || !a.bias || !a.logits) return hipErrorInvalidValue;
    if (!a.onehot && (a.loss || a.n_correct || a.d_logits_out)) return hipErrorInvalidValue;
    const int blocks = (a.B + CLS_HEAD_WAVES - 1) / CLS_HEAD_WAVES;
    hipLaunchKernelGGL(cls_head_fwd_kernel, dim3(a.onehot ? 1 : (blocks > 256 ? 256 : blocks)), dim3(64 * CLS_HEAD_WAVES), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cls_head_bwd(const ClsHeadArgs& a, hipStream_t s) {
    if (!cls_head_shape_ok(a) || !a.d_logits) return hipErrorInvalidValue;
    if (a.dx && (a.dx_stride < (size_t)a.H || (a.dx_dtype != DT_BF16 && a.dx_dtype != DT_F16 && a.dx_dtype != DT_F32))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cls_head_bwd_kernel, dim3(a.H / 64), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ aspect-att fusion (reference models/mm_late.py:115-131)
// V = reshape(cat(t_pool, v_pool), [B, 2, H]): slot j of post n is row 2 n + j of the [2 B, H] matrix [t_pool; v_pool] -- a RESHAPE, so for B > 1 a
// post pairs two text rows, a text and an image row of different posts, or two image rows.  That is the reference's behaviour and the parity target.
//   e_j = tanh(V_j . a + b),  w = softmax(e_0, e_1),  feats = relu(w_0 V_0 + w_1 V_1)
// Latency-bound like the CLS head: one wave per post, a lane keeps its H / 64 elements of both rows in registers.  fp32, tanhf / expf of the device
// library, no atomics: every output word has one writer and every sum a fixed order.
static constexpr int ASPECT_WAVES = 8;
__device__ __forceinline__ const float* aspect_row(const AspectFusionArgs& a, int r) {
    return r < a.B ? a.t_pool + (size_t)r * a.H : a.v_pool + (size_t)(r - a.B) * a.H;
}
__global__ __launch_bounds__(64 * ASPECT_WAVES) void aspect_fusion_fwd_kernel(AspectFusionArgs a) {
    const int lane = threadIdx.x & 63, n = blockIdx.x * ASPECT_WAVES + (threadIdx.x >> 6), H = a.H;
    if (n >= a.B) return;
    const float* v0 = aspect_row(a, 2 * n);
    const float* v1 = aspect_row(a, 2 * n + 1);
    float x0[16], x1[16], d0 = 0.f, d1 = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = lane + 64 * j;
        x0[j] = x1[j] = 0.f;
        if (c < H) {
            const float aw = a.a[c];
            x0[j] = v0[c]; x1[j] = v1[c];
            d0 = fmaf(x0[j], aw, d0);
            d1 = fmaf(x1[j], aw, d1);
        }
    }
    const float bias = a.b[0];
    const float e0 = tanhf(wave_sum(d0) + bias), e1 = tanhf(wave_sum(d1) + bias);
    const float mx = fmaxf(e0, e1), p0 = expf(e0 - mx), p1 = expf(e1 - mx);
    const float w0 = p0 / (p0 + p1), w1 = p1 / (p0 + p1);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = lane + 64 * j;
        if (c < H) a.feats[(size_t)n * H + c] = fmaxf(fmaf(w1, x1[j], w0 * x0[j]), 0.f);
    }
    if (lane == 0) {
        a.w[2 * n] = w0; a.w[2 * n + 1] = w1;
        a.e[2 * n] = e0; a.e[2 * n + 1] = e1;
    }
}
// Backward.  With g = d feats . (feats > 0) and dw_j = g . V_j the two-slot softmax gives ds_0 = w_0 (dw_0 - sum_k w_k dw_k) = w_0 w_1 (dw_0 - dw_1)
// = -ds_1 (the difference form: no cancellation against the weighted mean); dpre_j = ds_j (1 - e_j^2); dV_j = w_j g + dpre_j a.  Text rows of
// d t_pool are written by the one wave that owns them, image rows (the tower is frozen) not at all.  d a = sum dpre_j V_j and d b = sum dpre_j: the
// eight waves of a block add their posts' terms through LDS in wave order into the block's row of `partial`; aspect_fusion_reduce_kernel adds
// the rows in block order.
__global__ __launch_bounds__(64 * ASPECT_WAVES) void aspect_fusion_bwd_kernel(AspectFusionArgs a) {
    __shared__ float red[ASPECT_WAVES][1024];
    __shared__ float redb[ASPECT_WAVES];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, n = blockIdx.x * ASPECT_WAVES + w, H = a.H;
    float x0[16], x1[16], g[16], dp0 = 0.f, dp1 = 0.f, w0 = 0.f, w1 = 0.f;
    if (n < a.B) {          // wave-uniform
        const float* v0 = aspect_row(a, 2 * n);
        const float* v1 = aspect_row(a, 2 * n + 1);
        float s0 = 0.f, s1 = 0.f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int c = lane + 64 * j;
            x0[j] = x1[j] = g[j] = 0.f;
            if (c < H) {
                x0[j] = v0[c]; x1[j] = v1[c];
                g[j] = a.feats[(size_t)n * H + c] > 0.f ? a.d_feats[(size_t)n * H + c] : 0.f;
                s0 = fmaf(g[j], x0[j], s0);
                s1 = fmaf(g[j], x1[j], s1);
            }
        }
        w0 = a.w[2 * n]; w1 = a.w[2 * n + 1];
        const float e0 = a.e[2 * n], e1 = a.e[2 * n + 1];
        const float ds0 = w0 * w1 * (wave_sum(s0) - wave_sum(s1));
        dp0 = ds0 * (1.f - e0 * e0);
        dp1 = -ds0 * (1.f - e1 * e1);
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int c = lane + 64 * j;
        if (c < H) {
            float da = 0.f;
            if (n < a.B) {
                const float aw = a.a[c];
                if (2 * n < a.B) {
                    float* dst = a.d_tpool + (size_t)(2 * n) * H + c;
                    const float v = fmaf(dp0, aw, w0 * g[j]);
                    *dst = a.accumulate ? *dst + v : v;
                }
                if (2 * n + 1 < a.B) {
                    float* dst = a.d_tpool + (size_t)(2 * n + 1) * H + c;
                    const float v = fmaf(dp1, aw, w1 * g[j]);
                    *dst = a.accumulate ? *dst + v : v;
                }
                da = fmaf(dp1, x1[j], dp0 * x0[j]);
            }
            red[w][c] = da;
        }
    }
    if (lane == 0) redb[w] = n < a.B ? dp0 + dp1 : 0.f;
    __syncthreads();
    float* prow = a.partial + (size_t)blockIdx.x * (H + 4);
    for (int c = threadIdx.x; c < H; c += 64 * ASPECT_WAVES) {
        float v = red[0][c];
#pragma unroll
        for (int i = 1; i < ASPECT_WAVES; ++i) v += red[i][c];
        prow[c] = v;
    }
    if (threadIdx.x == 0) {
        float v = redb[0];
#pragma unroll
        for (int i = 1; i < ASPECT_WAVES; ++i) v += redb[i];
        prow[H] = v;
    }
}
__global__ __launch_bounds__(256) void aspect_fusion_reduce_kernel(AspectFusionArgs a, int blocks) {
    const int c = blockIdx.x * 256 + threadIdx.x, H = a.H;
    if (c > H) return;
    float v = a.partial[c];
    for (int i = 1; i < blocks; ++i) v += a.partial[(size_t)i * (H + 4) + c];
    float* dst = c < H ? a.da + c : a.db;
    *dst = a.accumulate_dw ? *dst + v : v;
}
static bool aspect_shape_ok(const AspectFusionArgs& a) {
    return a.B >= 1 && a.H >= 64 && a.H <= 1024 && a.H % 64 == 0 && a.t_pool && a.v_pool && a.a && a.b && a.feats && a.w && a.e;
}
size_t aspect_fusion_partial_floats(int B, int H) { return (size_t)((B + ASPECT_WAVES - 1) / ASPECT_WAVES) * (size_t)(H + 4); }
hipError_t launch_aspect_fusion_fwd(const AspectFusionArgs& a, hipStream_t s) {
    if (!aspect_shape_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(aspect_fusion_fwd_kernel, dim3((a.B + ASPECT_WAVES - 1) / ASPECT_WAVES), dim3(64 * ASPECT_WAVES), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_aspect_fusion_bwd(const AspectFusionArgs& a, hipStream_t s) {
    if (!aspect_shape_ok(a) || !a.d_feats || !a.d_tpool || !a.da || !a.db || !a.partial) return hipErrorInvalidValue;
    const int blocks = (a.B + ASPECT_WAVES - 1) / ASPECT_WAVES;
    hipLaunchKernelGGL(aspect_fusion_bwd_kernel, dim3(blocks), dim3(64 * ASPECT_WAVES), 0, s, a);
    hipError_t r = hipGetLastError();
    if (r != hipSuccess) return r;
    hipLaunchKernelGGL(aspect_fusion_reduce_kernel, dim3((a.H + 1 + 255) / 256), dim3(256), 0, s, a, blocks);
    return hipGetLastError();
}

}  // namespace mmhip
