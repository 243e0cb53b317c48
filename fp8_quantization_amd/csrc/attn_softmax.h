// attn_softmax.h -- the softmax block of approximate attention in one pass each way: from the raw
// scores of QK^T to the quantized A operand of PV, and from that operand's gradient back to the gradient of the raw
// scores.  Nothing is saved between the two but the scores: the backward recomputes the probabilities.
//
// s is [rows][n] float32, contiguous (rows = B H S, n = S); scale a float; the quantizer (optional, per tensor) is
// maxval on the device with E / M / S exponent, mantissa and sign bits.
//
// Arithmetic of one row (attn_probs: ONE device function, called by both directions, so the backward's p is the
// forward's bit for bit):
//   t_j = scale * s_j                  one fp32 multiply
//   m   = max_j t_j                    fmaxf, any order (the maximum does not depend on it)
//   e_j = expf(t_j - m)                expf: the device library's accurate single-precision exponential (not __expf)
//   l   = sum_j e_j                    fp32, in the fixed order below
//   p_j = e_j / l                      IEEE division
// Forward:   y_j = fq_apply(p_j), as fqt_quant (fq_train.h) and fp8a_fp8_quantize compute it -- the fq_fast form where
//            fq_fast_ok holds and option "fq_fast" is on (the same value bit for bit); without a quantizer y_j = p_j.
//            Thread 0 of workgroup 0 writes the quantizer's float and int32 bias, as fqt_write_bias does.
// Backward:  w_j  = the clamp weight of fq_train.h -- fqt_weights(fqt_code(p_j, lo, maxval, S)): 1 inside (lo, maxval),
//                   1/2 on a bound, 0 outside (and for a NaN); 1 everywhere without a quantizer
//            gq_j = g_j * w_j          a multiplication, as there (without a quantizer gq_j = g_j)
//            D    = sum_j (double)(gq_j * p_j)     the fp32 product widened, summed in double in the fixed order
//            ds_j = scale * (p_j * (gq_j - (float)D))      three fp32 operations: subtract, multiply, multiply
//            ds may alias g: a thread reads its elements of g before it writes the same elements of ds.
// n = 1: e = 1, l = 1, p = 1, D = gq, ds = 0 exactly.
//
// The fixed order of both sums: a thread adds its own values in index order (element t, t + T, t + 2 T, ... of the
// row, T threads per row); the 64 lanes of a wave are summed by the xor butterfly (offsets 32, 16, ..., 1: every lane
// ends with the same bits); the waves of a workgroup-wide row are added in wave order.  No floating-point atomics and
// no workspace; the form depends on n alone: two calls return identical bytes.
//
// Two forms, chosen from n alone (attn_form):
//   1 <= n <= 1024     WAVE PER ROW.  A workgroup of 256 threads owns four consecutive rows, one per wave; lane l
//                      holds elements l, l + 64, ... of its row in registers (coalesced 4-byte loads), V = 1, 2, 4, 8
//                      or 16 per lane (the smallest that covers n: ViT-B/16's n = 197 is V = 4), so every register loop
//                      unrolls.  The row is read once; max, sum and dot are butterflies inside the wave: no LDS, no
//                      barrier.  The last workgroup may own fewer than four live rows (its dead waves leave at once).
//   1024 < n <= 4096   WORKGROUP PER ROW.  256 threads x 16 values, the row resident in registers as
//                      bn_bwd_resident_kernel keeps a channel; the waves' results go through LDS (one array per
//                      reduction, so no array is rewritten) and are combined in wave order.
// All element offsets are 64-bit.  Rows of every n move as coalesced single values: the workload's n = 197 is odd, and
// a 16-byte form for n % 4 == 0 was not built (not measured).
#pragma once
#include "fp8approx_common.h"
#include "fq_train.h"

namespace fp8a {

constexpr int ATTN_NT = 256;               // threads per workgroup
constexpr int ATTN_WAVES = ATTN_NT / 64;   // rows per workgroup of the wave form
constexpr int ATTN_WAVE_MAX = 1024;        // longest row of the wave form (V = 16)
constexpr int ATTN_MAX = 4096;             // longest row at all (256 threads x 16 values)

struct AttnArgs {
    int64_t rows;
    int n;
    float scale;
    const float *s;
    const float *g;        // backward: the gradient of y
    float *out;            // forward: y; backward: ds (may be g)
    const float *maxval;   // device [1]; nullptr: no quantizer
    int E, M, S, fq_fast;
    float *bias_out;       // forward, or nullptr
    int32_t *ibias_out;
};

// per-lane values of the wave form: the smallest of 1, 2, 4, 8, 16 with 64 V >= n; 0: the workgroup form
static inline int attn_form(int64_t n) {
    if (n > ATTN_WAVE_MAX) return 0;
    int v = 1;
    while (64 * v < n) v *= 2;
    return v;
}

#if FP8A_OWN_ATTN
// The quantizer's constants (uniform); q.on = false: none.
struct AttnQ {
    bool on;
    float mx, lo, bias;
    FqFast k;
};
__device__ __forceinline__ AttnQ attn_q(const AttnArgs &a) {
    AttnQ q{};
    q.on = a.maxval != nullptr;
    if (q.on) {
        q.mx = *a.maxval;
        q.lo = a.S ? -q.mx : 0.0f;
        q.bias = fq_bias(q.mx, a.E, a.M);
        q.k = a.fq_fast && fq_fast_ok(q.mx, q.bias, a.M) ? fq_fast_k(q.mx, q.bias, a.M) : FqFast{0u, 0u, q.mx};
    }
    return q;
}

// The wave's butterfly, then (W > 1) the workgroup's waves in wave order through lds[W].  Every thread returns the
// same bits.  Each call of a kernel uses an array of its own, so one barrier per reduction is enough.
template <int W>
__device__ __forceinline__ float attn_reduce_max(float v, float *lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    if (W > 1) {
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < W; ++w) v = fmaxf(v, lds[w]);
    }
    return v;
}
template <int W, typename T>
__device__ __forceinline__ T attn_reduce_sum(T v, T *lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (W > 1) {
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < W; ++w) v += lds[w];
    }
    return v;
}

// p[j] = the probability of element t + j * 64 W of the row (0 past its end); t = the thread's index among the
// 64 W threads of the row.
template <int V, int W>
__device__ __forceinline__ void attn_probs(const float *row, int n, float scale, int t, float (&p)[V], float *lmax,
                                           float *lsum) {
    float m = -__builtin_huge_valf();
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int e = t + j * 64 * W;
        p[j] = e < n ? scale * row[e] : -__builtin_huge_valf();
        m = fmaxf(m, p[j]);
    }
    m = attn_reduce_max<W>(m, lmax);
    float l = 0.0f;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int e = t + j * 64 * W;
        p[j] = e < n ? expf(p[j] - m) : 0.0f;
        l += p[j];
    }
    l = attn_reduce_sum<W, float>(l, lsum);
#pragma unroll
    for (int j = 0; j < V; ++j) p[j] = p[j] / l;
}

template <int V, int W>
__device__ __forceinline__ void attn_forward_row(const AttnArgs &a, const AttnQ &q, int64_t r, int t, float *lmax,
                                                 float *lsum) {
    float p[V];
    attn_probs<V, W>(a.s + r * a.n, a.n, a.scale, t, p, lmax, lsum);
    float *const yr = a.out + r * a.n;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int e = t + j * 64 * W;
        if (e < a.n) yr[e] = q.on ? fq_apply_f<true>(p[j], q.mx, q.bias, a.M, a.S, q.k) : p[j];
    }
}

template <int V, int W>
__device__ __forceinline__ void attn_backward_row(const AttnArgs &a, const AttnQ &q, int64_t r, int t, float *lmax,
                                                  float *lsum, double *ldot) {
    float p[V], gq[V];
    const float *const gr = a.g + r * a.n;
#pragma unroll
    for (int j = 0; j < V; ++j) {  // (issued before the row's reductions: the loads overlap them)
        const int e = t + j * 64 * W;
        gq[j] = e < a.n ? gr[e] : 0.0f;
    }
    attn_probs<V, W>(a.s + r * a.n, a.n, a.scale, t, p, lmax, lsum);
    double d = 0.0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int e = t + j * 64 * W;
        if (q.on) {
            float wx, wm;
            fqt_weights(fqt_code(p[j], q.lo, q.mx, a.S), a.S, wx, wm);
            gq[j] = gq[j] * wx;
        }
        if (e < a.n) d += (double)(gq[j] * p[j]);
    }
    const float df = (float)attn_reduce_sum<W, double>(d, ldot);
    float *const dr = a.out + r * a.n;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int e = t + j * 64 * W;
        if (e < a.n) dr[e] = a.scale * (p[j] * (gq[j] - df));
    }
}

// Wave per row: n <= 64 V.
template <int V, bool BWD>
__global__ __launch_bounds__(ATTN_NT) void attn_wave_kernel(const AttnArgs a) {
    const AttnQ q = attn_q(a);
    if (!BWD && q.on && blockIdx.x == 0 && threadIdx.x == 0) {
        if (a.bias_out) a.bias_out[0] = q.bias;
        if (a.ibias_out) a.ibias_out[0] = (int32_t)q.bias;
    }
    const int64_t r = (int64_t)blockIdx.x * ATTN_WAVES + (threadIdx.x >> 6);
    if (r >= a.rows) return;  // (wave-uniform; this form has no barrier)
    const int lane = threadIdx.x & 63;
    if (BWD) attn_backward_row<V, 1>(a, q, r, lane, nullptr, nullptr, nullptr);
    else attn_forward_row<V, 1>(a, q, r, lane, nullptr, nullptr);
}

// Workgroup per row: n <= 4096.
template <bool BWD>
__global__ __launch_bounds__(ATTN_NT) void attn_row_kernel(const AttnArgs a) {
    __shared__ float lmax[ATTN_WAVES], lsum[ATTN_WAVES];
    __shared__ double ldot[ATTN_WAVES];
    const AttnQ q = attn_q(a);
    if (!BWD && q.on && blockIdx.x == 0 && threadIdx.x == 0) {
        if (a.bias_out) a.bias_out[0] = q.bias;
        if (a.ibias_out) a.ibias_out[0] = (int32_t)q.bias;
    }
    constexpr int V = ATTN_MAX / ATTN_NT;
    if (BWD) attn_backward_row<V, ATTN_WAVES>(a, q, blockIdx.x, threadIdx.x, lmax, lsum, ldot);
    else attn_forward_row<V, ATTN_WAVES>(a, q, blockIdx.x, threadIdx.x, lmax, lsum);
}
#endif  // FP8A_OWN_ATTN

}  // namespace fp8a
