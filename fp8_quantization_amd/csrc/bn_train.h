// bn_train.h -- training-mode batch norm on deterministic kernels of our own: the batch statistics of
// x viewed as [N][C][inner] (fp32, contiguous; inner = H * W for a convolution, 1 for a linear layer's
// [B, F]), the running-statistics update, and y = clamp(x * scale + shift) with an optional per-tensor
// output quantizer.  It replaces F.batch_norm (MIOpen) in BNFusedHijacker's training-mode forward
// (the BN re-estimation protocol, bn_reestimate.py): MIOpen's statistics are not reproducible run to
// run here, and they feed every later layer's quantizer through discontinuous rounding.
//
// Three kernels (structure and reduction discipline as fq_mse.h):
//   bn_stats_kernel     a workgroup of BN_NT threads works on ONE (channel, part): it walks its tiles
//                       of the channel's n = N * inner values, flattened index j -> (image j / inner,
//                       offset j % inner), lanes along inner (float4 loads when inner % 4 == 0 and x
//                       is 16-byte aligned).
//   bn_stats_lin_kernel inner < BN_LIN_INNER (the linear layout, and convolutions down to a few
//                       pixels): lanes along CHANNELS, so a wave's load of one (image, offset) is
//                       contiguous for inner = 1; a workgroup works on (64 channels, part), its waves
//                       take the part's values j round robin.
//   bn_finalize_kernel  one thread per channel: sums the parts in part order, writes save_mean /
//                       save_var (biased), scale / shift, and updates the running statistics.
//   bn_apply_kernel     elementwise, may run in place: y = fmaf(x, scale[c], shift[c]) (the eval
//                       store's form, epi() in fp8approx_common.h), the clamp, fq_apply.
//
// Shifted sums: K_c = x[image 0][c][offset 0].  Every value is widened to double BEFORE any
// arithmetic: d = (double)x - (double)K_c is exact while the two fp32 values lie within 29 binades of
// each other (else it carries one double rounding, 2^-53 of the larger: under the bound below),
// d * d is formed in double, and a thread accumulates S = sum d and Q = sum d^2 in double, in index
// order.  The shift removes the E[x^2] - mean^2 cancellation: with |mean| / std = 2^20 the unshifted
// fp32 form has no correct bit left in the variance, the shifted one loses none.
//
// Reduction (deterministic, no floating-point atomics):
//   1. thread partials (S, Q) in double, in index order over the thread's values of every tile;
//   2. summed over the wave by a fixed xor butterfly (lin form: lanes are channels, no butterfly);
//   3. the workgroup's waves summed in wave order through LDS: one (S, Q) double pair per
//      (channel, part) in the workspace;
//   4. bn_finalize_kernel sums the parts in part order.
// The split into parts depends on the shape alone, so two calls return identical bytes.
// Error: every step is a double addition of the n terms in some fixed tree, so with D = max |x - K_c|
//   |S^ - S| <= (n - 1) 2^-53 n D,   |Q^ - Q| <= (n + 1) 2^-53 n D^2
// hence |mean^ - mean| <= n 2^-52 D and |var^ - var| <= 4 n 2^-52 D^2 before the one fp32 rounding.
#pragma once
#include "fp8approx_common.h"

namespace fp8a {

constexpr int BN_NT = 256;                  // threads per workgroup
constexpr int BN_V = 16;                    // values a thread takes from one tile
constexpr int BN_TILE = BN_NT * BN_V;       // values per workgroup tile
constexpr int BN_WAVES = BN_NT / 64;
constexpr int BN_LIN_INNER = 16;            // inner below this: the lanes-along-channels mapping
constexpr int BN_LIN_TILE = 256;            // values (per channel) of one lin tile: 64 per wave
constexpr int64_t BN_TARGET_WGS = 2048;     // workgroups a launch aims for when channels are split

struct BnArgs {
    const float *x;
    float *y;                 // nullptr: statistics only
    int64_t N, C, inner, n;   // n = N * inner values per channel
    int64_t parts;            // workgroups per channel (lin form: per 64 channels)
    double2 *part;            // [C][parts] (S, Q)
    const float *gamma, *beta;
    float eps, momentum;
    float *running_mean, *running_var;  // nullable
    float *save_mean, *save_var;
    float2 *ss;               // [C] (scale, shift)
    int act;
    float lo, hi;
    FqIn q;                   // q.mx == nullptr: no output quantizer
    float *q_bias;
    int32_t *q_ibias;
    int vec;                  // inner % 4 == 0 and x (and y) 16-byte aligned: float4 accesses
};

static inline bool bn_lin(int64_t inner) { return inner < BN_LIN_INNER; }

// Workgroups per channel (lin form: per group of 64 channels): every tile of a short channel gets its
// own; long channels share BN_TARGET_WGS workgroups between all channels.  A function of the shape alone.
static inline int64_t bn_parts(int64_t N, int64_t C, int64_t inner) {
    const int64_t n = N * inner;
    const bool lin = bn_lin(inner);
    const int64_t tile = lin ? BN_LIN_TILE : BN_TILE;
    const int64_t groups = lin ? (C + 63) / 64 : C;
    const int64_t tiles = (n + tile - 1) / tile;
    const int64_t want = (BN_TARGET_WGS + groups - 1) / groups;
    return std::max<int64_t>(1, std::min(tiles, want));
}

#if FP8A_OWN_BN
__device__ __forceinline__ void bn_acc(double &S, double &Q, float v, double K) {
    const double d = (double)v - K;
    S += d;
    Q += d * d;
}

__global__ __launch_bounds__(BN_NT) void bn_stats_kernel(const BnArgs a) {
    __shared__ double2 wsum[BN_WAVES];
    const int64_t c = blockIdx.x / a.parts, p = blockIdx.x - c * a.parts;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t cstride = a.C * a.inner;          // image stride
    const float *const xc = a.x + c * a.inner;      // (image 0, channel c, offset 0)
    const double K = (double)xc[0];
    const uint32_t inner = (uint32_t)a.inner;       // (host: inner < 2^31 - BN_TILE)
    // this workgroup's tiles of the channel: [p tiles / parts, (p + 1) tiles / parts)
    const int64_t tiles = (a.n + BN_TILE - 1) / BN_TILE;
    const int64_t t0 = p * tiles / a.parts, t1 = (p + 1) * tiles / a.parts;
    double S = 0.0, Q = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * BN_TILE;             // (workgroup-uniform)
        const int64_t img0 = j0 / a.inner;
        const uint32_t off0 = (uint32_t)(j0 - img0 * a.inner);
        const uint32_t cnt = (uint32_t)min((int64_t)BN_TILE, a.n - j0);
        if (a.vec) {
            // inner % 4 == 0: n, j0 and every index below are multiples of 4, a float4 stays in one image
#pragma unroll
            for (int k = 0; k < BN_V / 4; ++k) {
                const uint32_t l = (uint32_t)(k * BN_NT + threadIdx.x) * 4u;
                if (l < cnt) {
                    const uint32_t o = off0 + l, di = o / inner, off = o - di * inner;
                    const float4 v = *reinterpret_cast<const float4 *>(xc + (img0 + di) * cstride + off);
                    bn_acc(S, Q, v.x, K);
                    bn_acc(S, Q, v.y, K);
                    bn_acc(S, Q, v.z, K);
                    bn_acc(S, Q, v.w, K);
                }
            }
        } else {
#pragma unroll 4
            for (int k = 0; k < BN_V; ++k) {
                const uint32_t l = (uint32_t)(k * BN_NT + threadIdx.x);
                if (l < cnt) {
                    const uint32_t o = off0 + l, di = o / inner, off = o - di * inner;
                    bn_acc(S, Q, xc[(img0 + di) * cstride + off], K);
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        S += __shfl_xor(S, off);
        Q += __shfl_xor(Q, off);
    }
    if (lane == 0) wsum[wave] = make_double2(S, Q);
    __syncthreads();
    if (threadIdx.x == 0) {
        double2 s = wsum[0];
#pragma unroll
        for (int w = 1; w < BN_WAVES; ++w) {
            s.x += wsum[w].x;
            s.y += wsum[w].y;
        }
        a.part[c * a.parts + p] = s;
    }
}

__global__ __launch_bounds__(BN_NT) void bn_stats_lin_kernel(const BnArgs a) {
    __shared__ double2 wsum[BN_WAVES][64];
    const int64_t g = blockIdx.x / a.parts, p = blockIdx.x - g * a.parts;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = g * 64 + lane;
    const bool live = c < a.C;
    const int64_t cstride = a.C * a.inner;
    const float *const xc = a.x + (live ? c : 0) * a.inner;
    const double K = (double)xc[0];
    const int64_t tiles = (a.n + BN_LIN_TILE - 1) / BN_LIN_TILE;
    const int64_t t0 = p * tiles / a.parts, t1 = (p + 1) * tiles / a.parts;
    const int64_t j1 = min(t1 * BN_LIN_TILE, a.n);
    double S = 0.0, Q = 0.0;
    if (live) {
        // the part's values j, round robin over the waves (wave-uniform j: lanes differ in channel only)
        for (int64_t j = t0 * BN_LIN_TILE + wave; j < j1; j += BN_WAVES) {
            const int64_t img = j / a.inner, off = j - img * a.inner;
            bn_acc(S, Q, xc[img * cstride + off], K);
        }
    }
    wsum[wave][lane] = make_double2(S, Q);
    __syncthreads();
    if (wave == 0 && live) {
        double2 s = wsum[0][lane];
#pragma unroll
        for (int w = 1; w < BN_WAVES; ++w) {
            s.x += wsum[w][lane].x;
            s.y += wsum[w][lane].y;
        }
        a.part[c * a.parts + p] = s;
    }
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const BnArgs a) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C) return;
    const double2 *const q = a.part + c * a.parts;
    double S = q[0].x, Q = q[0].y;
    for (int64_t p = 1; p < a.parts; ++p) {
        S += q[p].x;
        Q += q[p].y;
    }
    const double n = (double)a.n;
    const double K = (double)a.x[c * a.inner];
    const double mean = K + S / n;
    const double var = fmax(0.0, (Q - S * S / n) / n);   // biased: the one that normalizes
    const double unb = var * (n / (n - 1.0));
    a.save_mean[c] = (float)mean;
    a.save_var[c] = (float)var;
    const double g = a.gamma ? (double)a.gamma[c] : 1.0;
    const double b = a.beta ? (double)a.beta[c] : 0.0;
    const double scale = g / sqrt(var + (double)a.eps);
    a.ss[c] = make_float2((float)scale, (float)(b - mean * scale));
    const double m = (double)a.momentum;
    if (a.running_mean) a.running_mean[c] = (float)((1.0 - m) * (double)a.running_mean[c] + m * mean);
    if (a.running_var) a.running_var[c] = (float)((1.0 - m) * (double)a.running_var[c] + m * unb);
}

__device__ __forceinline__ float bn_apply1(const BnArgs &a, float x, float2 e, float mx, float bias) {
    float v = __fmaf_rn(x, e.x, e.y);
    if (a.act) v = fminf(fmaxf(v, a.lo), a.hi);
    if (a.q.mx) v = fq_apply(v, mx, bias, a.q.M, a.q.S);
    return v;
}

// IT: uint32_t when N * C * inner < 2^31 (32-bit divisions; the grid stride cannot wrap), else uint64_t.
template <typename IT>
__global__ __launch_bounds__(256) void bn_apply_kernel(const BnArgs a) {
    const IT inner = (IT)a.inner, C = (IT)a.C;
    const IT total = (IT)a.N * C * inner;
    float mx = 0.0f, bias = 0.0f;
    if (a.q.mx) {
        mx = *a.q.mx;
        bias = fq_bias(mx, a.q.E, a.q.M);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            if (a.q_bias) a.q_bias[0] = bias;
            if (a.q_ibias) a.q_ibias[0] = (int32_t)bias;
        }
    }
    const IT tid = (IT)blockIdx.x * blockDim.x + threadIdx.x, nth = (IT)gridDim.x * blockDim.x;
    if (a.vec) {
        for (IT i = tid; i < total / 4; i += nth) {
            const IT idx = i * 4;
            const float2 e = a.ss[(idx / inner) % C];
            const float4 v = *reinterpret_cast<const float4 *>(a.x + idx);
            *reinterpret_cast<float4 *>(a.y + idx) =
                make_float4(bn_apply1(a, v.x, e, mx, bias), bn_apply1(a, v.y, e, mx, bias),
                            bn_apply1(a, v.z, e, mx, bias), bn_apply1(a, v.w, e, mx, bias));
        }
    } else {
        for (IT idx = tid; idx < total; idx += nth)
            a.y[idx] = bn_apply1(a, a.x[idx], a.ss[(idx / inner) % C], mx, bias);
    }
}
#endif  // FP8A_OWN_BN

}  // namespace fp8a
