// fq_mse.h -- the fused candidate search of the FP8 MSE range estimator (FP_MSE_Estimator,
// range_estimators.py:285-369).  For x viewed as [rows][inner], a grid of candidate maxvals
// grid[n_cand][rows] and a list of mantissa widths, one pass over x computes
//   sse[m][i][r] = sum over inner of (x - fq(x; maxval = grid[i][r], M = mbits[m], sign_bits))^2
// where fq is fq_apply / fq_bias (fp8approx_common.h), bit for bit, and d = x - fq, d * d are
// single fp32 operations: the terms are the ones the literal loop (one fp8a_fp8_quantize per
// candidate, subtract, square) forms.
//
// Three kernels:
//   mse_prep_kernel   one thread per (row, width, candidate): MseCand {maxval, bias = fq_bias,
//                     qmx = fq(maxval), info} into the workspace.
//   mse_search_kernel a workgroup of MSE_NT threads works on ONE row: it copies the row's candidates
//                     to LDS (they are wave-uniform: read back through readfirstlane into SGPRs), then
//                     walks its share of the row in tiles of MSE_TILE values.  Each thread holds
//                     MSE_V values of the tile in registers and loops over every candidate, so x is
//                     read from memory once per call.  A long row is split over several workgroups.
//   mse_reduce_kernel sums the workgroups' parts per output in a fixed order.
//
// Reduction (deterministic, no floating-point atomics, as gemm_check.h):
//   1. a thread sums the terms of its MSE_V values of one tile in fp32, in index order: an fp32
//      partial never covers more than MSE_L = MSE_V terms;
//   2. the partial is widened to double and summed over the wave by a fixed xor butterfly;
//   3. lane 0 adds the wave's sum to the wave's own LDS slot of the candidate (double), tile after tile;
//   4. after the last tile the workgroup's waves are summed in wave order and written to the
//      workspace as one double per (workgroup, candidate);
//   5. mse_reduce_kernel: one thread per output sums the row's workgroups in workgroup order.
// The split of a row over workgroups depends on the shape alone, so two calls return identical bytes.
// Error against the exact sum of the same fp32 terms (non-negative terms, the standard bound):
// (MSE_L - 1) fp32 roundings in step 1, then double roundings only.
//
// A candidate whose bias is not finite (maxval = 0: the row's largest |x| is 0; the reference's
// log2(0) + inf = NaN poisons its scales) has sse = NaN, set explicitly: no float that is not finite
// is ever converted to int.
//
// Grouped form (GROUP = true; the runtime option "mse_group").  The grid spans 0.1 .. 1.2 max|x|,
// under four binades, so only a handful of distinct biases occur per width, in runs of consecutive
// candidates (the bias is monotone in maxval).  Within a run the unclamped quantizer q(x) =
// fq_apply_lit(x, bias, M) is the same function, and a candidate differs only in its clamp:
//   |x| <= mx:  xc = x exactly, so the term is (x - q(x))^2           -- once per run: e0
//   |x| >  mx:  xc = +-mx, q = +-q(mx) (frexp, rint and the scalings are odd functions), and
//               x - (+-qmx) = +-(|x| - qmx) exactly, so the term is (|x| - qmx)^2
// (sign_bits = 0: a negative x clamps to 0 for every candidate, which e0 carries; the upper test is
// x > mx).  The same fp32 terms summed in the same order: the two forms return identical bytes.
// (A NaN in x makes every sse of its row NaN in both forms; the NaN's payload is not pinned.)
#pragma once
#include "fp8approx_common.h"

namespace fp8a {

constexpr int MSE_NT = 256;                 // threads per workgroup
constexpr int MSE_V = 16;                   // values of x a thread holds
constexpr int MSE_L = MSE_V;                // terms per fp32 partial (the error bound's constant)
constexpr int MSE_TILE = MSE_NT * MSE_V;    // values per workgroup tile
constexpr int MSE_WAVES = MSE_NT / 64;
constexpr int MSE_MAX_MBITS = 7;
constexpr int MSE_MAX_CANDS = 1024;         // n_mbits * n_cand (LDS: 48 bytes per candidate)
constexpr int64_t MSE_TARGET_WGS = 2048;    // workgroups a launch aims for when rows are split

constexpr uint32_t MSE_BAD = 0x100u;        // info: the bias is not finite -> sse = NaN
constexpr uint32_t MSE_NEWRUN = 0x200u;     // info: first candidate of a run of equal (width, bias)

struct MseCand {
    float mx, bias, qmx;  // maxval, fq_bias(maxval), fq_apply_lit(maxval)
    uint32_t info;        // mantissa width | MSE_BAD | MSE_NEWRUN
};

struct MseArgs {
    const float *x;
    int64_t rows, inner;
    const float *grid;  // [n_cand][rows]
    int n_cand, n_mbits, n_bits, sign_bits;
    int mbits[MSE_MAX_MBITS];
    MseCand *cand;      // [rows][n_mbits * n_cand]
    double *part;       // [rows][parts][n_mbits * n_cand]
    int64_t parts;      // workgroups per row
    double *sse;        // [n_mbits][n_cand][rows]
};

// Workgroups per row: every tile of a short row gets its own; long rows share MSE_TARGET_WGS
// workgroups between all rows (each then walks several tiles).
static inline int64_t mse_parts(int64_t rows, int64_t inner) {
    const int64_t tiles = (inner + MSE_TILE - 1) / MSE_TILE;
    const int64_t want = (MSE_TARGET_WGS + rows - 1) / rows;
    return std::max<int64_t>(1, std::min(tiles, want));
}

#if FP8A_OWN_MSE
__global__ __launch_bounds__(256) void mse_prep_kernel(const MseArgs a) {
    const int nc = a.n_mbits * a.n_cand;
    const int64_t total = a.rows * nc;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = idx / nc;
        const int c = (int)(idx - r * nc), m = c / a.n_cand, i = c - m * a.n_cand;
        const int M = a.mbits[m], E = a.n_bits - a.sign_bits - M;
        const float mx = a.grid[(int64_t)i * a.rows + r];
        const float bias = fq_bias(mx, E, M);
        const bool bad = !(fabsf(bias) <= 3.0e38f);  // inf or NaN
        MseCand o;
        o.mx = mx;
        o.bias = bias;
        o.qmx = bad ? 0.0f : fq_apply_lit(mx, bias, M);
        bool newrun = true;
        if (i > 0) newrun = fq_bias(a.grid[(int64_t)(i - 1) * a.rows + r], E, M) != bias;
        o.info = (uint32_t)M | (bad ? MSE_BAD : 0u) | (newrun ? MSE_NEWRUN : 0u);
        a.cand[idx] = o;
    }
}

__device__ __forceinline__ float mse_uniform(float v) {
    return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(v)));
}

// One tile: the thread's values x[j] (valid bit j of vmask; FULL: all valid) against every candidate.
template <bool GROUP, bool FULL>
__device__ __forceinline__ void mse_tile(const float (&x)[MSE_V], uint32_t vmask, int sign_bits, int nc,
                                         const MseCand *cand, double *wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float ax[MSE_V], e0[MSE_V];
    if (GROUP) {
#pragma unroll
        for (int j = 0; j < MSE_V; ++j) {
            ax[j] = sign_bits ? fabsf(x[j]) : x[j];
            e0[j] = 0.0f;
        }
    }
    for (int c = 0; c < nc; ++c) {
        const MseCand cd = cand[c];
        const float mx = mse_uniform(cd.mx), bias = mse_uniform(cd.bias), qmx = mse_uniform(cd.qmx);
        const uint32_t info = __builtin_amdgcn_readfirstlane(cd.info);
        const int M = (int)(info & 0xFFu);
        float s = 0.0f;
        if (info & MSE_BAD) {
            s = __builtin_nanf("");
        } else if (GROUP) {
            if (info & MSE_NEWRUN) {
#pragma unroll
                for (int j = 0; j < MSE_V; ++j) {
                    const float d = x[j] - fq_apply_lit(sign_bits ? x[j] : fmaxf(x[j], 0.0f), bias, M);
                    e0[j] = d * d;
                }
            }
#pragma unroll
            for (int j = 0; j < MSE_V; ++j) {
                const float t = ax[j] - qmx;
                float e = (ax[j] > mx) ? t * t : e0[j];
                if (!FULL) e = ((vmask >> j) & 1u) ? e : 0.0f;
                s = (j == 0) ? e : s + e;
            }
        } else {
#pragma unroll
            for (int j = 0; j < MSE_V; ++j) {
                const float d = x[j] - fq_apply(x[j], mx, bias, M, sign_bits);
                float e = d * d;
                if (!FULL) e = ((vmask >> j) & 1u) ? e : 0.0f;
                s = (j == 0) ? e : s + e;
            }
        }
        double ds = (double)s;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) ds += __shfl_xor(ds, off);
        if (lane == 0) wsum[c * MSE_WAVES + wave] += ds;
    }
}

template <bool GROUP>
__global__ __launch_bounds__(MSE_NT) void mse_search_kernel(const MseArgs a) {
    extern __shared__ double mse_lds[];  // wsum [nc][MSE_WAVES] doubles, then the row's MseCand [nc]
    const int nc = a.n_mbits * a.n_cand;
    double *const wsum = mse_lds;
    MseCand *const cand = reinterpret_cast<MseCand *>(mse_lds + (size_t)nc * MSE_WAVES);
    const int64_t r = blockIdx.x / a.parts, p = blockIdx.x - r * a.parts;
    for (int i = threadIdx.x; i < nc; i += MSE_NT) cand[i] = a.cand[r * nc + i];
    for (int i = threadIdx.x; i < nc * MSE_WAVES; i += MSE_NT) wsum[i] = 0.0;
    __syncthreads();

    // this workgroup's tiles of the row: [p tiles / parts, (p + 1) tiles / parts)
    const int64_t tiles = (a.inner + MSE_TILE - 1) / MSE_TILE;
    const int64_t t0 = p * tiles / a.parts, t1 = (p + 1) * tiles / a.parts;
    const float *const xr = a.x + r * a.inner;
    for (int64_t t = t0; t < t1; ++t) {
        const int64_t base = t * MSE_TILE + threadIdx.x;
        float x[MSE_V];
        if ((t + 1) * MSE_TILE <= a.inner) {  // (workgroup-uniform)
#pragma unroll
            for (int j = 0; j < MSE_V; ++j) x[j] = xr[base + (int64_t)j * MSE_NT];
            mse_tile<GROUP, true>(x, 0xFFFFFFFFu, a.sign_bits, nc, cand, wsum);
        } else {
            // the row's ragged last tile
            uint32_t vmask = 0;
#pragma unroll
            for (int j = 0; j < MSE_V; ++j) {
                const int64_t e = base + (int64_t)j * MSE_NT;
                const bool in = e < a.inner;
                x[j] = in ? xr[e] : 0.0f;
                vmask |= in ? (1u << j) : 0u;
            }
            mse_tile<GROUP, false>(x, vmask, a.sign_bits, nc, cand, wsum);
        }
    }
    __syncthreads();
    double *const out = a.part + (r * a.parts + p) * nc;
    for (int i = threadIdx.x; i < nc; i += MSE_NT) {
        double s = wsum[i * MSE_WAVES];
#pragma unroll
        for (int w = 1; w < MSE_WAVES; ++w) s += wsum[i * MSE_WAVES + w];
        out[i] = s;
    }
}

__global__ __launch_bounds__(256) void mse_reduce_kernel(const MseArgs a) {
    const int nc = a.n_mbits * a.n_cand;
    const int64_t total = a.rows * nc;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = idx / nc;
        const int c = (int)(idx - r * nc);
        const double *const q = a.part + r * a.parts * nc + c;
        double s = q[0];
        for (int64_t p = 1; p < a.parts; ++p) s += q[p * nc];
        a.sse[(int64_t)c * a.rows + r] = s;
    }
}
#endif  // FP8A_OWN_MSE

}  // namespace fp8a
