// Global-norm gradient clipping (include/mmhip.h: mmhip_set_grad_clip, mmhip_op_grad_clip): the sum of squares of the step's gradient as
// per-workgroup partial sums, and the launch that turns them into the coefficient the fused AdamW reads.
//   total = grad_scale * sqrt(sum g^2),  coef = min(1, max_norm / (total + 1e-6))          (torch.nn.utils.clip_grad_norm_)
// Bit-reproducible by construction: both partial kernels run a FIXED grid (GRADNORM_BLOCKS / GRADNORM_ROW_BLOCKS workgroups of 256, on every
// device and under every CU cap), a lane adds its elements in address order into GRADNORM_UNROLL accumulators, lanes, waves and partials are
// added in one fixed tree, every partial has one writer (a plain store) and there is no float atomic.  The summation order is therefore a
// function of the segment list alone; tests/gradclip_ref.py emulates it.
// A gradient element AdamW would read as 0 (g * grad_scale not finite) adds 0 here as well.
#include "mmhip_common.h"
#include "mmhip_kernels.h"

namespace mmhip {

namespace {
constexpr int GN_THREADS = 256;

__device__ __forceinline__ float gn_read(float g, float gs) { return fabsf(g * gs) <= 3.4028234e38f ? g : 0.f; }      // false for NaN: guard_finite's test
__device__ __forceinline__ void gn_add4(float& acc, const f32x4& x, float gs) {
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float t = gn_read(x[e], gs); acc = fmaf(t, t, acc); }
}
// the lane's accumulators pairwise, the wave's 64 lanes by xor shuffles 32 .. 1, the four waves pairwise: thread 0 returns the workgroup's sum
__device__ __forceinline__ float gn_block_sum(const float (&acc)[GRADNORM_UNROLL], float* red) {
    float s = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}

// Dense segments.  Thread t of the whole grid (NT threads) takes the four-vectors t, t + NT, t + 2 NT, ... of each segment in turn; vector
// t + (4 i + u) NT goes to accumulator u.  The main loop issues its four 16-byte loads unconditionally (four independent loads and dependency
// chains per lane: at a few MB per segment the kernel is latency-bound otherwise), the remainder of a segment takes at most three more.
// A segment's n & 3 tail elements are added once, by the grid's first threads, to accumulator 0.
__global__ __launch_bounds__(GN_THREADS) void gradnorm_dense_kernel(GradNormSegments sg, float gs, float* __restrict__ partial) {
    __shared__ float red[4];
    constexpr size_t NT = (size_t)GRADNORM_BLOCKS * GN_THREADS;
    const size_t t = (size_t)blockIdx.x * GN_THREADS + threadIdx.x;
    float acc[GRADNORM_UNROLL] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < sg.count; ++s) {
        const float* __restrict__ g = sg.g[s];
        const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g);
        const size_t n = sg.n[s], n4 = n >> 2;
        size_t i = t;
        for (; i + 3 * NT < n4; i += 4 * NT) {
            const f32x4 x0 = g4[i], x1 = g4[i + NT], x2 = g4[i + 2 * NT], x3 = g4[i + 3 * NT];
            gn_add4(acc[0], x0, gs); gn_add4(acc[1], x1, gs); gn_add4(acc[2], x2, gs); gn_add4(acc[3], x3, gs);
        }
        if (i < n4) gn_add4(acc[0], g4[i], gs);
        if (i + NT < n4) gn_add4(acc[1], g4[i + NT], gs);
        if (i + 2 * NT < n4) gn_add4(acc[2], g4[i + 2 * NT], gs);
        if (t < (n & 3)) { const float x = gn_read(g[n4 * 4 + t], gs); acc[0] = fmaf(x, x, acc[0]); }
    }
    const float sum = gn_block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// Rows of a [rows, width] table whose state byte has bit0 (ROW_HAS_GRAD).  A wave takes 64 consecutive rows at a time (chunk w, w + NW, ...;
// NW waves in the grid): one byte per lane, a ballot, then the flagged rows in ascending order -- at most B * T of Bernice's 250 002 rows are
// flagged, so a wave that looked at one byte per trip would spend its time waiting for bytes.  Within a row lane l takes the four-vectors
// l, l + 64, ...; vector l + 64 (4 i + u) goes to accumulator u.  Unflagged rows are not read.
__global__ __launch_bounds__(GN_THREADS) void gradnorm_rows_kernel(const float* __restrict__ g, int rows, int width, const uint8_t* __restrict__ state, float gs,
                                                                   float* __restrict__ partial) {
    __shared__ float red[4];
    constexpr int NW = GRADNORM_ROW_BLOCKS * (GN_THREADS / 64);
    const int lane = threadIdx.x & 63, nch = width >> 2;
    const int chunks = (rows + 63) >> 6;
    float acc[GRADNORM_UNROLL] = {0.f, 0.f, 0.f, 0.f};
    for (int ch = blockIdx.x * (GN_THREADS / 64) + (threadIdx.x >> 6); ch < chunks; ch += NW) {
        const int r = ch * 64 + lane;
        const bool flagged = r < rows && (state[r] & ROW_HAS_GRAD);
        unsigned long long todo = __ballot(flagged);
        while (todo) {
            const int k = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const f32x4* __restrict__ g4 = reinterpret_cast<const f32x4*>(g + (size_t)(ch * 64 + k) * width);
            int c = lane;
            for (; c + 192 < nch; c += 256) {
                const f32x4 x0 = g4[c], x1 = g4[c + 64], x2 = g4[c + 128], x3 = g4[c + 192];
                gn_add4(acc[0], x0, gs); gn_add4(acc[1], x1, gs); gn_add4(acc[2], x2, gs); gn_add4(acc[3], x3, gs);
            }
            if (c < nch) gn_add4(acc[0], g4[c], gs);
            if (c + 64 < nch) gn_add4(acc[1], g4[c + 64], gs);
            if (c + 128 < nch) gn_add4(acc[2], g4[c + 128], gs);
        }
    }
    const float sum = gn_block_sum(acc, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// One workgroup: thread t adds partials t, t + 256, ... in fp64, a shared-memory tree (strides 128 .. 1) adds the threads; thread 0 writes the
// public words.  `flag` (the step guard's void-step word, may be null) set: the counters stay as they are.
__global__ __launch_bounds__(GN_THREADS) void gradnorm_finalize_kernel(const float* __restrict__ partial, int count, float max_norm, float gs, const unsigned* flag,
                                                                       float* __restrict__ words, unsigned* __restrict__ counters) {
    __shared__ double red[GN_THREADS];
    double s = 0.0;
    for (int i = threadIdx.x; i < count; i += GN_THREADS) s += (double)partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = GN_THREADS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float total = (float)((double)gs * sqrt(red[0]));
        const float q = max_norm / (total + 1e-6f);
        const float coef = q < 1.0f ? q : 1.0f;          // (a NaN quotient cannot arise: total >= 0 or +inf, max_norm finite and > 0)
        words[0] = coef;
        words[1] = total;
        if (!(flag && *flag)) {          // counters: {clipped steps, steps}, the two words behind coef and total
            if (coef < 1.0f) counters[0] += 1u;
            counters[1] += 1u;
        }
    }
}
}  // namespace

size_t grad_clip_state_bytes() { return 16 + sizeof(float) * (size_t)(GRADNORM_BLOCKS + GRADNORM_ROW_BLOCKS); }

hipError_t launch_grad_clip(const GradNormSegments& sg, const float* row_g, int rows, int width, const uint8_t* row_state, float max_norm, float grad_scale,
                            const unsigned* void_flag, void* clip_state, hipStream_t s) {
    if (sg.count < 0 || sg.count > GRADNORM_MAX_SEGMENTS || !clip_state || ((uintptr_t)clip_state & 15) || !(max_norm > 0.f) || !(max_norm <= 3.4028234e38f))
        return hipErrorInvalidValue;
    if (rows < 0 || (rows > 0 && (!row_g || !row_state || width <= 0 || width % 4 || ((uintptr_t)row_g & 15)))) return hipErrorInvalidValue;
    GradNormSegments live{};
    for (int i = 0; i < sg.count; ++i) {
        if (!sg.n[i]) continue;
        if (!sg.g[i] || ((uintptr_t)sg.g[i] & 15)) return hipErrorInvalidValue;
        live.g[live.count] = sg.g[i]; live.n[live.count] = sg.n[i]; ++live.count;
    }
    float* words = reinterpret_cast<float*>(clip_state);
    float* partial = words + 4;
    int count = 0;
    // the dense partials come first; without dense segments the row partials take their place (finalize reads `count` of them from the start)
    if (live.count) {
        hipLaunchKernelGGL(gradnorm_dense_kernel, dim3(GRADNORM_BLOCKS), dim3(GN_THREADS), 0, s, live, grad_scale, partial);
        count += GRADNORM_BLOCKS;
    }
    if (rows > 0) {
        hipLaunchKernelGGL(gradnorm_rows_kernel, dim3(GRADNORM_ROW_BLOCKS), dim3(GN_THREADS), 0, s, row_g, rows, width, row_state, grad_scale, partial + count);
        count += GRADNORM_ROW_BLOCKS;
    }
    hipLaunchKernelGGL(gradnorm_finalize_kernel, dim3(1), dim3(GN_THREADS), 0, s, partial, count, max_norm, grad_scale, void_flag, words, reinterpret_cast<unsigned*>(clip_state) + 2);
    return hipGetLastError();
}

}  // namespace mmhip
