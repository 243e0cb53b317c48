// fq_train.h -- the FP8 fake quantizer's training pair: one pass forward, one pass backward, for a
// quantizer whose maxval may be learned (FPQuantizer.learn_maxval).
//
// quantize_to_fp8_ste_MM (fp8_quantizer.py:97-173) rounds its bias, detaches its scales and rounds
// straight through power-of-two scales, so its gradient is that of the clamp
//   xc = min(max(x, lo), maxval),  lo = -maxval (sign_bits 1) or the constant 0,
// with ATen's half-and-half split of a max / min tie:
//   grad_x[i]   = g[i] wx[i]        wx = 1 inside (lo, maxval), 1/2 on a bound, 0 outside
//   grad_maxval = sum_i g[i] wm[i]  wm = +1 (x > maxval), +1/2 (x == maxval),
//                                        -1 (x < -maxval), -1/2 (x == -maxval) (signed only), else 0
// over the row of maxval (x viewed as [rows][inner]; rows = 1 per tensor).  A NaN in x: wx = wm = 0.
//
// Forward (fqt_forward_kernel / fqt_forward_rows_kernel): y = fq_apply(x) -- fp8a_fp8_quantize's
// arithmetic, in the fq_fast form where the row's constants pass fq_fast_ok and option "fq_fast" is on
// -- the row's float / int32 bias, and one code byte per element:
//   bits 0-1  2 wx = (x > lo & x < maxval) + (x >= lo & x <= maxval): 0, 1, 2
//   bits 2-3  the bound the element sits on or beyond: 0 none, 1 upper (x >= maxval),
//             2 lower of a signed quantizer (x <= -maxval)
// |wm| = 1 - wx on a side, so the backward needs neither x nor maxval.
//
// Backward (fqt_backward_kernel / fqt_backward_rows_kernel): grad_x = g wx (a multiplication: -3 * 0 =
// -0.0, inf * 0 = NaN, as ATen), and the term g wm as one fp32 multiply (exact up to underflow: wm is 0,
// +-1/2 or +-1), widened to double before it is summed.
//
// Two forms, chosen by the shape alone (fqt_short):
//   inner >  FQT_SHORT  a workgroup of FQT_NT threads works on ONE row and walks its share of the row's
//                       tiles of FQT_TILE values (fqt_parts workgroups per row, as fq_mse.h splits a
//                       row: every tile of a short row gets its own workgroup, long rows share
//                       "fqt_target_wgs" workgroups between all rows).  Full tiles move as 16-byte
//                       words when every row starts 16-byte aligned (a.vec: rows = 1 or inner % 4 = 0,
//                       and aligned pointers), else -- and in a row's ragged last tile -- as coalesced
//                       single values.  All offsets are 64-bit: rows = 1 with inner >= 2^31 is one launch.
//   inner <= FQT_SHORT  one THREAD per row (a depthwise weight [960, 1, 3, 3] is 960 rows of 9 values:
//                       4 workgroups, not 960 nearly empty ones).
//
// Reduction (deterministic, no floating-point atomics, as fq_mse.h):
//   1. a thread adds its terms to a double accumulator in index order, tile after tile;
//   2. the wave's accumulators are summed by a fixed xor butterfly, the workgroup's waves in wave order,
//      and written to the workspace as one double per (row, workgroup);
//   3. fqt_reduce_kernel: one thread per row sums the row's workgroups in workgroup order and rounds
//      the double to fp32 once; from 17 workgroups per row on, fqt_reduce_wave_kernel: one wave per row,
//      lane l sums workgroups l, l + 64, ... in order, then the xor butterfly (a single thread walking
//      2048 parts measured 0.15 ms, four times the backward pass itself).
// (One thread per row: step 1 is the whole sum.)  The split depends on the shape and the option alone, so
// two calls return identical bytes.  Error against the exact sum of the n terms of a row:
//   |result - exact| <= (2^-24 + n 2^-53) sum |g wm| < 2^-23 sum |g wm|  for n < 2^28
// (n - 1 double additions, each within 2^-53 of its partial sum, and the one rounding to fp32).
#pragma once
#include "fp8approx_common.h"

namespace fp8a {

constexpr int FQT_NT = 256;                 // threads per workgroup
constexpr int FQT_V = 16;                   // values a thread handles per tile
constexpr int FQT_TILE = FQT_NT * FQT_V;    // values per workgroup tile
constexpr int FQT_WAVES = FQT_NT / 64;
constexpr int64_t FQT_SHORT = 64;           // rows of at most this many values: one thread per row
constexpr int FQT_TARGET_WGS = 2048;        // option "fqt_target_wgs": workgroups a launch aims for

struct FqtArgs {
    int64_t rows, inner, parts;  // parts: workgroups per row (fqt_parts)
    int S;                       // sign bits
    int vec;                     // full tiles as 16-byte words (every row start is 16-byte aligned)
    // forward
    const float *x, *maxval;     // maxval [rows]
    float *y, *bias_out;         // bias_out / ibias_out [rows], or nullptr
    int32_t *ibias_out;
    int E, M, fq_fast;
    // both: forward writes, backward reads
    uint8_t *code;
    // backward
    const float *g;
    float *gx, *gmax;            // gmax [rows]
    double *part;                // [rows][parts]
};

static inline bool fqt_short(int64_t inner) { return inner <= FQT_SHORT; }

// Workgroups per row (the split rule; target = option "fqt_target_wgs").
static inline int64_t fqt_parts(int64_t rows, int64_t inner, int64_t target) {
    if (fqt_short(inner)) return 1;
    const int64_t tiles = (inner + FQT_TILE - 1) / FQT_TILE;
    const int64_t want = (target + rows - 1) / rows;
    return std::max<int64_t>(1, std::min(tiles, want));
}

// The ordered reduction's form, by the split alone: a wave per row from this many parts on.
static inline bool fqt_reduce_by_wave(int64_t parts) { return parts > 16; }

#if FP8A_OWN_FQT
__device__ __forceinline__ uint32_t fqt_code(float x, float lo, float mx, int S) {
    const uint32_t twice = (uint32_t)((x > lo) & (x < mx)) + (uint32_t)((x >= lo) & (x <= mx));
    const uint32_t side = (x >= mx) ? 1u : (S && x <= lo) ? 2u : 0u;
    return twice | (side << 2);
}

// (wx, wm) of a code byte
__device__ __forceinline__ void fqt_weights(uint32_t c, int S, float &wx, float &wm) {
    wx = (float)(c & 3u) * 0.5f;
    const uint32_t side = c >> 2;
    const float h = 1.0f - wx;
    wm = side == 1u ? h : (side == 2u && S) ? -h : 0.0f;
}

// The constants of one row's quantizer.
struct FqtRow {
    float mx, lo, bias;
    FqFast k;  // k.emn = 0: the literal form
};
__device__ __forceinline__ FqtRow fqt_row(const FqtArgs &a, int64_t r) {
    FqtRow q;
    q.mx = a.maxval[r];
    q.lo = a.S ? -q.mx : 0.0f;
    q.bias = fq_bias(q.mx, a.E, a.M);
    q.k = a.fq_fast && fq_fast_ok(q.mx, q.bias, a.M) ? fq_fast_k(q.mx, q.bias, a.M) : FqFast{0u, 0u, q.mx};
    return q;
}
__device__ __forceinline__ void fqt_write_bias(const FqtArgs &a, int64_t r, float bias) {
    if (a.bias_out) a.bias_out[r] = bias;
    if (a.ibias_out) a.ibias_out[r] = (int32_t)bias;
}
__device__ __forceinline__ float fqt_quant(const FqtArgs &a, const FqtRow &q, float v) {
    return fq_apply_f<true>(v, q.mx, q.bias, a.M, a.S, q.k);
}

// this workgroup's tiles [t0, t1) of its row
__device__ __forceinline__ void fqt_share(const FqtArgs &a, int64_t p, int64_t &t0, int64_t &t1) {
    const int64_t tiles = (a.inner + FQT_TILE - 1) / FQT_TILE;
    t0 = p * tiles / a.parts;
    t1 = (p + 1) * tiles / a.parts;
}

__global__ __launch_bounds__(FQT_NT) void fqt_forward_kernel(const FqtArgs a) {
    const int64_t r = blockIdx.x / a.parts, p = blockIdx.x - r * a.parts;
    const FqtRow q = fqt_row(a, r);
    if (p == 0 && threadIdx.x == 0) fqt_write_bias(a, r, q.bias);
    int64_t t0, t1;
    fqt_share(a, p, t0, t1);
    const float *const xr = a.x + r * a.inner;
    float *const yr = a.y + r * a.inner;
    uint8_t *const cr = a.code + r * a.inner;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t base = t * FQT_TILE;
        if (a.vec && base + FQT_TILE <= a.inner) {  // (workgroup-uniform)
            float4 v[FQT_V / 4];
#pragma unroll
            for (int j = 0; j < FQT_V / 4; ++j)
                v[j] = *reinterpret_cast<const float4 *>(xr + base + (int64_t)(j * FQT_NT + threadIdx.x) * 4);
#pragma unroll
            for (int j = 0; j < FQT_V / 4; ++j) {
                const int64_t e = base + (int64_t)(j * FQT_NT + threadIdx.x) * 4;
                const float in[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                float o[4];
                uint32_t c = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    o[i] = fqt_quant(a, q, in[i]);
                    c |= fqt_code(in[i], q.lo, q.mx, a.S) << (8 * i);
                }
                *reinterpret_cast<float4 *>(yr + e) = make_float4(o[0], o[1], o[2], o[3]);
                *reinterpret_cast<uint32_t *>(cr + e) = c;
            }
        } else {
#pragma unroll 4
            for (int j = 0; j < FQT_V; ++j) {
                const int64_t e = base + j * FQT_NT + threadIdx.x;
                if (e < a.inner) {
                    const float v = xr[e];
                    yr[e] = fqt_quant(a, q, v);
                    cr[e] = (uint8_t)fqt_code(v, q.lo, q.mx, a.S);
                }
            }
        }
    }
}

__global__ __launch_bounds__(FQT_NT) void fqt_forward_rows_kernel(const FqtArgs a) {
    const int64_t r = (int64_t)blockIdx.x * FQT_NT + threadIdx.x;
    if (r >= a.rows) return;
    const FqtRow q = fqt_row(a, r);
    fqt_write_bias(a, r, q.bias);
    const int64_t o = r * a.inner;
    for (int64_t i = 0; i < a.inner; ++i) {
        const float v = a.x[o + i];
        a.y[o + i] = fqt_quant(a, q, v);
        a.code[o + i] = (uint8_t)fqt_code(v, q.lo, q.mx, a.S);
    }
}

__global__ __launch_bounds__(FQT_NT) void fqt_backward_kernel(const FqtArgs a) {
    __shared__ double wsum[FQT_WAVES];
    const int64_t r = blockIdx.x / a.parts, p = blockIdx.x - r * a.parts;
    int64_t t0, t1;
    fqt_share(a, p, t0, t1);
    const float *const gr = a.g + r * a.inner;
    float *const xr = a.gx + r * a.inner;
    const uint8_t *const cr = a.code + r * a.inner;
    double acc = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t base = t * FQT_TILE;
        if (a.vec && base + FQT_TILE <= a.inner) {  // (workgroup-uniform)
            float4 v[FQT_V / 4];
            uint32_t c[FQT_V / 4];
#pragma unroll
            for (int j = 0; j < FQT_V / 4; ++j) {
                const int64_t e = base + (int64_t)(j * FQT_NT + threadIdx.x) * 4;
                v[j] = *reinterpret_cast<const float4 *>(gr + e);
                c[j] = *reinterpret_cast<const uint32_t *>(cr + e);
            }
#pragma unroll
            for (int j = 0; j < FQT_V / 4; ++j) {
                const int64_t e = base + (int64_t)(j * FQT_NT + threadIdx.x) * 4;
                const float in[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
                float o[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float wx, wm;
                    fqt_weights((c[j] >> (8 * i)) & 0xFFu, a.S, wx, wm);
                    o[i] = in[i] * wx;
                    acc += (double)(in[i] * wm);
                }
                *reinterpret_cast<float4 *>(xr + e) = make_float4(o[0], o[1], o[2], o[3]);
            }
        } else {
#pragma unroll 4
            for (int j = 0; j < FQT_V; ++j) {
                const int64_t e = base + j * FQT_NT + threadIdx.x;
                if (e < a.inner) {
                    const float gv = gr[e];
                    float wx, wm;
                    fqt_weights(cr[e], a.S, wx, wm);
                    xr[e] = gv * wx;
                    acc += (double)(gv * wm);
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
#pragma unroll
        for (int w = 1; w < FQT_WAVES; ++w) s += wsum[w];
        a.part[r * a.parts + p] = s;
    }
}

__global__ __launch_bounds__(FQT_NT) void fqt_backward_rows_kernel(const FqtArgs a) {
    const int64_t r = (int64_t)blockIdx.x * FQT_NT + threadIdx.x;
    if (r >= a.rows) return;
    const int64_t o = r * a.inner;
    double acc = 0.0;
    for (int64_t i = 0; i < a.inner; ++i) {
        const float gv = a.g[o + i];
        float wx, wm;
        fqt_weights(a.code[o + i], a.S, wx, wm);
        a.gx[o + i] = gv * wx;
        acc += (double)(gv * wm);
    }
    a.part[r] = acc;  // (parts = 1)
}

// Few parts per row (fqt_reduce_by_wave false): one thread per row sums them in order.  parts = 0 (an empty
// row): the sum of nothing.
__global__ __launch_bounds__(FQT_NT) void fqt_reduce_kernel(const FqtArgs a) {
    const int64_t r = (int64_t)blockIdx.x * FQT_NT + threadIdx.x;
    if (r >= a.rows) return;
    double s = 0.0;
    for (int64_t p = 0; p < a.parts; ++p) s += a.part[r * a.parts + p];
    a.gmax[r] = (float)s;
}

// Many parts per row: one WAVE per row -- lane l sums parts l, l + 64, ... in order (64 independent chains
// of loads instead of one), then the fixed xor butterfly.
__global__ __launch_bounds__(FQT_NT) void fqt_reduce_wave_kernel(const FqtArgs a) {
    const int64_t r = (int64_t)blockIdx.x * FQT_WAVES + (threadIdx.x >> 6);
    if (r >= a.rows) return;  // (wave-uniform)
    const int lane = threadIdx.x & 63;
    double s = 0.0;
    for (int64_t p = lane; p < a.parts; p += 64) s += a.part[r * a.parts + p];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) a.gmax[r] = (float)s;
}
#endif  // FP8A_OWN_FQT

}  // namespace fp8a
