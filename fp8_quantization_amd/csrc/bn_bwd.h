// bn_bwd.h -- the backward of training-mode batch norm (+ a clamp activation) on deterministic kernels,
// the counterpart of bn_train.h: same layout (x, the pre-BN product, and dy fp32 contiguous, viewed as
// [N][C][inner], n = N * inner values per channel), same tiles, same split into parts (bn_parts()).
//
// Per channel, from the forward's own fp32 save_mean / save_var and (scale, shift):
//   z = fmaf(x, scale, shift)              bit-identical to the forward's pre-clamp value
//   m = lo < z < hi (act) else 1           the threshold_backward / hardtanh_backward rule; NaN: 0
//   g = m ? dy : 0                         a select: an inf in dy at a clamped position contributes nothing
//   invstd = 1 / sqrt(save_var + eps)      in double, from the fp32 save_var, as torch does
//   G = sum g,  H = sum g (x - save_mean)  every value widened to double BEFORE any arithmetic
//   dbeta = fp32(G),  dgamma = fp32(H invstd)
//   dx = k1 g + k2 (x - save_mean) + k3,   k1 = gamma invstd,  k2 = -k1 invstd^2 H / n,  k3 = -k1 G / n
// the three coefficients computed in double and rounded to fp32 once each.
//
// Three forms; the host picks one from the shape alone (bn_bwd_resident()):
//   bn_bwd_resident_kernel   inner >= BN_LIN_INNER and n <= BN_TILE: ONE workgroup of BN_NT threads owns a
//                            channel.  A thread loads its up-to-BN_V x and dy values once (index
//                            l = k BN_NT + thread, or 4 (k BN_NT + thread) .. + 3 as one float4 when a.vec),
//                            forms g and keeps x and g in registers; the workgroup reduces (G, H), thread 0
//                            computes the coefficients and writes dgamma / dbeta, the coefficients go to all
//                            threads through LDS, and every thread writes dx from its registers: one launch,
//                            three passes over memory (x, dy read; dx written).
//   general                  bn_bwd_reduce_kernel (grid (channel, part), tiles of BN_TILE values, the index
//                            mapping j -> (image, offset) and the float4 loads of bn_stats_kernel) or
//                            bn_bwd_reduce_lin_kernel (inner < BN_LIN_INNER: lanes along channels, as
//                            bn_stats_lin_kernel) write one (G, H) double pair per (channel, part);
//                            bn_bwd_finalize_kernel (one thread per channel) sums the parts in part order,
//                            writes dgamma / dbeta and the coefficient record (k1, k2, k3, save_mean);
//                            bn_bwd_apply_kernel<IT> (elementwise, grid stride, float4 where the forward's
//                            apply uses them) recomputes z and the mask and writes dx: five passes.
// dx may alias dy: every dx element is written by the thread that read the dy element of the same index,
// after that read, and the reduce launches end before the apply launch starts.
//
// Reduction (deterministic, no floating-point atomics), as bn_train.h:
//   1. thread partials (G, H) in double, in index order over the thread's values;
//   2. a fixed xor butterfly over the wave (lin form: lanes are channels, no butterfly);
//   3. the workgroup's waves in wave order through LDS;
//   4. (general form) bn_bwd_finalize_kernel sums the parts in part order.
// The parts depend on the shape alone, so two calls return identical bytes.
//
// Error bounds (u = 2^-24, e = 2^-53; A = sum |g|, B = sum |g (x - save_mean)| over the channel).
//   Sums.  (double)g and (double)x - (double)save_mean are exact or carry one double rounding; the
//   product carries one more, and each of the n terms then passes through at most n - 1 double additions
//   of a fixed tree:
//       |G^ - G| <= dG = (n - 1) e A,        |H^ - H| <= dH = (n + 1) e B      (to first order in e).
//   Where every g is a multiple of 2^q and n max|g| < 2^(q + 53), G^ = G exactly.
//   Stored quantities.  invstd and the products below are a few double operations on (G^, H^) (relative
//   error under 8 e, written c = 1 + 2^-20 below to cover it and the second-order terms), then ONE fp32
//   rounding each:
//       |dbeta  - G|        <= u |G| + dG                      (bit-equal to fp32(G) when G^ = G)
//       |dgamma - H invstd| <= c (u |H invstd| + dH invstd)
//       k_i = k_i* (1 + d_i), |d_i| <= u c, with k_i* the exact coefficients of the TRUE G, H shifted by
//       |k2^ - k2*| <= |k1| invstd^2 dH / n,  |k3^ - k3*| <= |k1| dG / n  before that rounding.
//   dx is a chain of exactly THREE fp32 operations (-ffp-contract=off; the fused ones are explicit):
//       d = x - save_mean            (one rounding; exact when x and save_mean lie within a binade)
//       t = fmaf(k2, d, k3)          (one rounding)
//       dx = fmaf(k1, g, t)          (one rounding)
//   so the term k1 g carries 2 roundings (k1, dx), k2 (x - mean) carries 4 (k2, d, t, dx), k3 carries 3:
//       |dx - dx*| <= c [ u (2 |k1 g| + 4 |k2 (x - mean)| + 3 |k3|)
//                         + |k1| (invstd^2 dH |x - mean| + dG) / n ] + 2^-149 (1 + |g| + |x - mean|)
//   (the last term: a subnormal result, or a subnormal k1 / k2 whose rounding is absolute, times its factor),
//   dx* the formula above evaluated exactly from the fp32 inputs.
#pragma once
#include "bn_train.h"

namespace fp8a {

struct BnBwdArgs {
    const float *x, *dy;
    float *dx;                // may be dy
    int64_t N, C, inner, n;   // n = N * inner values per channel
    int64_t parts;            // bn_parts(): workgroups per channel (lin form: per 64 channels)
    double2 *part;            // [C][parts] (G, H)                                 (general form)
    float4 *coef;             // [C] (k1, k2, k3, save_mean)                       (general form)
    const float *gamma;       // nullable: 1
    const float *save_mean, *save_var;
    float eps;
    const float2 *ss;         // [C] the forward's (scale, shift)
    int act;
    float lo, hi;
    float *dgamma, *dbeta;    // nullable
    int vec;                  // inner % 4 == 0 and x, dy, dx 16-byte aligned: float4 accesses
};

// The register-resident form: one workgroup per channel holds the channel's values.
static inline bool bn_bwd_resident(int64_t N, int64_t inner) { return !bn_lin(inner) && N * inner <= BN_TILE; }

#if FP8A_OWN_BN
// g = m ? dy : 0 with the forward's own z.
__device__ __forceinline__ float bn_bwd_g(const BnBwdArgs &a, float x, float dy, float2 e) {
    if (!a.act) return dy;
    const float z = __fmaf_rn(x, e.x, e.y);
    return (a.lo < z && z < a.hi) ? dy : 0.0f;
}

__device__ __forceinline__ void bn_bwd_acc(double &G, double &H, float g, float x, double mean) {
    const double gd = (double)g;
    G += gd;
    H += gd * ((double)x - mean);
}

// dx of one element: the three fp32 operations of the header's bound.
__device__ __forceinline__ float bn_bwd_dx(float4 k, float x, float g) {
    const float d = x - k.w;
    return __fmaf_rn(k.x, g, __fmaf_rn(k.y, d, k.z));
}

// From a channel's (G, H): dgamma / dbeta and the coefficient record, each rounded to fp32 once.
__device__ __forceinline__ float4 bn_bwd_coef(const BnBwdArgs &a, int64_t c, double G, double H) {
    const float mean = a.save_mean[c];
    const double invstd = 1.0 / sqrt((double)a.save_var[c] + (double)a.eps);
    const double n = (double)a.n;
    const double k1 = (a.gamma ? (double)a.gamma[c] : 1.0) * invstd;
    if (a.dgamma) a.dgamma[c] = (float)(H * invstd);
    if (a.dbeta) a.dbeta[c] = (float)G;
    return make_float4((float)k1, (float)(-k1 * invstd * invstd * H / n), (float)(-k1 * G / n), mean);
}

// Wave butterfly, then the waves in wave order: thread 0 returns with the workgroup's sums.
__device__ __forceinline__ void bn_bwd_wg_sum(double &G, double &H, double2 *wsum) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        G += __shfl_xor(G, off);
        H += __shfl_xor(H, off);
    }
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = make_double2(G, H);
    __syncthreads();
    if (threadIdx.x == 0) {
        G = wsum[0].x;
        H = wsum[0].y;
#pragma unroll
        for (int w = 1; w < BN_WAVES; ++w) {
            G += wsum[w].x;
            H += wsum[w].y;
        }
    }
}

__global__ __launch_bounds__(BN_NT) void bn_bwd_resident_kernel(const BnBwdArgs a) {
    __shared__ double2 wsum[BN_WAVES];
    __shared__ float4 kco;
    const int64_t c = blockIdx.x;
    const uint32_t inner = (uint32_t)a.inner, n = (uint32_t)a.n;   // (host: n <= BN_TILE)
    const int64_t cstride = a.C * a.inner;
    const int64_t base = c * a.inner;               // (image 0, channel c, offset 0)
    const float2 e = a.ss[c];
    const double mean = (double)a.save_mean[c];
    float xv[BN_V], gv[BN_V];
    double G = 0.0, H = 0.0;
    if (a.vec) {
        // inner % 4 == 0: n and every index are multiples of 4, a float4 stays in one image
#pragma unroll
        for (int k = 0; k < BN_V / 4; ++k) {
            const uint32_t l = (uint32_t)(k * BN_NT + threadIdx.x) * 4u;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f), d = v;
            if (l < n) {
                const uint32_t di = l / inner, off = l - di * inner;
                const int64_t at = base + di * cstride + off;
                v = *reinterpret_cast<const float4 *>(a.x + at);
                d = *reinterpret_cast<const float4 *>(a.dy + at);
            }
            xv[4 * k] = v.x; xv[4 * k + 1] = v.y; xv[4 * k + 2] = v.z; xv[4 * k + 3] = v.w;
            gv[4 * k] = bn_bwd_g(a, v.x, d.x, e); gv[4 * k + 1] = bn_bwd_g(a, v.y, d.y, e);
            gv[4 * k + 2] = bn_bwd_g(a, v.z, d.z, e); gv[4 * k + 3] = bn_bwd_g(a, v.w, d.w, e);
            if (l < n) {
#pragma unroll
                for (int i = 0; i < 4; ++i) bn_bwd_acc(G, H, gv[4 * k + i], xv[4 * k + i], mean);
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < BN_V; ++k) {
            const uint32_t l = (uint32_t)(k * BN_NT + threadIdx.x);
            xv[k] = 0.f;
            gv[k] = 0.f;
            if (l < n) {
                const uint32_t di = l / inner, off = l - di * inner;
                const int64_t at = base + di * cstride + off;
                xv[k] = a.x[at];
                gv[k] = bn_bwd_g(a, xv[k], a.dy[at], e);
                bn_bwd_acc(G, H, gv[k], xv[k], mean);
            }
        }
    }
    bn_bwd_wg_sum(G, H, wsum);
    if (threadIdx.x == 0) kco = bn_bwd_coef(a, c, G, H);
    __syncthreads();
    const float4 kc = kco;
    if (a.vec) {
#pragma unroll
        for (int k = 0; k < BN_V / 4; ++k) {
            const uint32_t l = (uint32_t)(k * BN_NT + threadIdx.x) * 4u;
            if (l < n) {
                const uint32_t di = l / inner, off = l - di * inner;
                *reinterpret_cast<float4 *>(a.dx + base + di * cstride + off) =
                    make_float4(bn_bwd_dx(kc, xv[4 * k], gv[4 * k]), bn_bwd_dx(kc, xv[4 * k + 1], gv[4 * k + 1]),
                                bn_bwd_dx(kc, xv[4 * k + 2], gv[4 * k + 2]), bn_bwd_dx(kc, xv[4 * k + 3], gv[4 * k + 3]));
            }
        }
    } else {
#pragma unroll
        for (int k = 0; k < BN_V; ++k) {
            const uint32_t l = (uint32_t)(k * BN_NT + threadIdx.x);
            if (l < n) {
                const uint32_t di = l / inner, off = l - di * inner;
                a.dx[base + di * cstride + off] = bn_bwd_dx(kc, xv[k], gv[k]);
            }
        }
    }
}

__global__ __launch_bounds__(BN_NT) void bn_bwd_reduce_kernel(const BnBwdArgs a) {
    __shared__ double2 wsum[BN_WAVES];
    const int64_t c = blockIdx.x / a.parts, p = blockIdx.x - c * a.parts;
    const int64_t cstride = a.C * a.inner;          // image stride
    const int64_t base = c * a.inner;               // (image 0, channel c, offset 0)
    const float2 e = a.ss[c];
    const double mean = (double)a.save_mean[c];
    const uint32_t inner = (uint32_t)a.inner;       // (host: inner < 2^31 - BN_TILE)
    // this workgroup's tiles of the channel: [p tiles / parts, (p + 1) tiles / parts)
    const int64_t tiles = (a.n + BN_TILE - 1) / BN_TILE;
    const int64_t t0 = p * tiles / a.parts, t1 = (p + 1) * tiles / a.parts;
    double G = 0.0, H = 0.0;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t j0 = t * BN_TILE;             // (workgroup-uniform)
        const int64_t img0 = j0 / a.inner;
        const uint32_t off0 = (uint32_t)(j0 - img0 * a.inner);
        const uint32_t cnt = (uint32_t)min((int64_t)BN_TILE, a.n - j0);
        if (a.vec) {
#pragma unroll
            for (int k = 0; k < BN_V / 4; ++k) {
                const uint32_t l = (uint32_t)(k * BN_NT + threadIdx.x) * 4u;
                if (l < cnt) {
                    const uint32_t o = off0 + l, di = o / inner, off = o - di * inner;
                    const int64_t at = base + (img0 + di) * cstride + off;
                    const float4 v = *reinterpret_cast<const float4 *>(a.x + at);
                    const float4 d = *reinterpret_cast<const float4 *>(a.dy + at);
                    bn_bwd_acc(G, H, bn_bwd_g(a, v.x, d.x, e), v.x, mean);
                    bn_bwd_acc(G, H, bn_bwd_g(a, v.y, d.y, e), v.y, mean);
                    bn_bwd_acc(G, H, bn_bwd_g(a, v.z, d.z, e), v.z, mean);
                    bn_bwd_acc(G, H, bn_bwd_g(a, v.w, d.w, e), v.w, mean);
                }
            }
        } else {
#pragma unroll 4
            for (int k = 0; k < BN_V; ++k) {
                const uint32_t l = (uint32_t)(k * BN_NT + threadIdx.x);
                if (l < cnt) {
                    const uint32_t o = off0 + l, di = o / inner, off = o - di * inner;
                    const int64_t at = base + (img0 + di) * cstride + off;
                    const float v = a.x[at];
                    bn_bwd_acc(G, H, bn_bwd_g(a, v, a.dy[at], e), v, mean);
                }
            }
        }
    }
    bn_bwd_wg_sum(G, H, wsum);
    if (threadIdx.x == 0) a.part[c * a.parts + p] = make_double2(G, H);
}

__global__ __launch_bounds__(BN_NT) void bn_bwd_reduce_lin_kernel(const BnBwdArgs a) {
    __shared__ double2 wsum[BN_WAVES][64];
    const int64_t grp = blockIdx.x / a.parts, p = blockIdx.x - grp * a.parts;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t c = grp * 64 + lane;
    const bool live = c < a.C;
    const int64_t cstride = a.C * a.inner;
    const int64_t base = (live ? c : 0) * a.inner;
    const float2 e = a.ss[live ? c : 0];
    const double mean = (double)a.save_mean[live ? c : 0];
    const int64_t tiles = (a.n + BN_LIN_TILE - 1) / BN_LIN_TILE;
    const int64_t t0 = p * tiles / a.parts, t1 = (p + 1) * tiles / a.parts;
    const int64_t j1 = min(t1 * BN_LIN_TILE, a.n);
    double G = 0.0, H = 0.0;
    if (live) {
        // the part's values j, round robin over the waves (wave-uniform j: lanes differ in channel only)
        for (int64_t j = t0 * BN_LIN_TILE + wave; j < j1; j += BN_WAVES) {
            const int64_t img = j / a.inner, off = j - img * a.inner;
            const int64_t at = base + img * cstride + off;
            const float v = a.x[at];
            bn_bwd_acc(G, H, bn_bwd_g(a, v, a.dy[at], e), v, mean);
        }
    }
    wsum[wave][lane] = make_double2(G, H);
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

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const BnBwdArgs a) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= a.C) return;
    const double2 *const q = a.part + c * a.parts;
    double G = q[0].x, H = q[0].y;
    for (int64_t p = 1; p < a.parts; ++p) {
        G += q[p].x;
        H += q[p].y;
    }
    a.coef[c] = bn_bwd_coef(a, c, G, H);
}

// IT: uint32_t when N * C * inner < 2^31 (32-bit divisions; the grid stride cannot wrap), else uint64_t.
template <typename IT>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const BnBwdArgs a) {
    const IT inner = (IT)a.inner, C = (IT)a.C;
    const IT total = (IT)a.N * C * inner;
    const IT tid = (IT)blockIdx.x * blockDim.x + threadIdx.x, nth = (IT)gridDim.x * blockDim.x;
    if (a.vec) {
        for (IT i = tid; i < total / 4; i += nth) {
            const IT idx = i * 4, c = (idx / inner) % C;
            const float2 e = a.ss[c];
            const float4 k = a.coef[c];
            const float4 v = *reinterpret_cast<const float4 *>(a.x + idx);
            const float4 d = *reinterpret_cast<const float4 *>(a.dy + idx);
            *reinterpret_cast<float4 *>(a.dx + idx) =
                make_float4(bn_bwd_dx(k, v.x, bn_bwd_g(a, v.x, d.x, e)), bn_bwd_dx(k, v.y, bn_bwd_g(a, v.y, d.y, e)),
                            bn_bwd_dx(k, v.z, bn_bwd_g(a, v.z, d.z, e)), bn_bwd_dx(k, v.w, bn_bwd_g(a, v.w, d.w, e)));
        }
    } else {
        for (IT idx = tid; idx < total; idx += nth) {
            const IT c = (idx / inner) % C;
            const float v = a.x[idx];
            a.dx[idx] = bn_bwd_dx(a.coef[c], v, bn_bwd_g(a, v, a.dy[idx], a.ss[c]));
        }
    }
}
#endif  // FP8A_OWN_BN

}  // namespace fp8a
