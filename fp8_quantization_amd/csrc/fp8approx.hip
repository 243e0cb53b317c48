// fp8approx.hip -- the C-ABI (include/fp8approx.h) of the MI355X (gfx950) approx-FP8 matmul/conv
// engine: argument checks, table packing, workspace layout, the host dispatch of the GEMM paths
// (run_gemm), the convolution / linear entry points, and the small kernels (split-K reduce, gated
// exact kernel, tensor-bias depthwise forms, fake quantizer, pooling, the exact product of
// gemm_dense.h).  The approx GEMM kernel families are compiled in their own units (k_*.hip,
// fp8approx_launch.h).  Hot path: approx_v9 (revollllt/FP8_quantization,
// approx/approx_matmul_whole_v9.py:10-169); DESIGN.md has the derivations and the exactness argument.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/fp8approx.h"
#include "fp8approx_common.h"
#include "fp8approx_launch.h"
#include "gemm_f8mx.h"
#include "gemm_v5mx.h"
#include "gemm_tt.h"
#include "gemm_tt16.h"
#include "gemm_dense.h"
#include "conv_tbx.h"
#include "gemm_check.h"
#include "fq_mse.h"
#include "fq_train.h"
#include "bn_train.h"
#include "gemm_bmm.h"
#include "gemm_grad.h"

// (defined with C linkage below; run_gemm launches it too)
extern "C" __global__ void fq_bias_kernel(fp8a::FqIn fq, float *bias_out, int32_t *ibias_out);

namespace fp8a {

// ------------------------------------------------------------------------- error handling
static thread_local std::string g_err;

static int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

static int hip_check(const char *what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(FP8A_EHIP, std::string(what) + ": " + hipGetErrorString(e));
    return FP8A_OK;
}

static int pack_table(const int32_t *table, int M, bool approx, TablePack &tp, int &mode) {
    memset(&tp, 0, sizeof(tp));
    mode = TM_NONE;
    if (!approx || table == nullptr) return FP8A_OK;
    const int n = 1 << M;
    if (n * n > 1024) return fail(FP8A_EFORMAT, "error table larger than 32x32 (mant_width > 5)");
    int lo = 0, hi = 0;
    for (int i = 0; i < n * n; ++i) {
        if (table[i] < -128 || table[i] > 127) return fail(FP8A_EINVAL, "error table entry out of int8 range");
        tp.raw[i] = (int8_t)table[i];
        lo = std::min(lo, table[i]);
        hi = std::max(hi, table[i]);
    }
    if (lo == 0 && hi == 0) return FP8A_OK;
    const int words2 = (n * 2 + 31) / 32;
    if (lo >= 0 && hi <= 1 && n <= 32) {
        mode = TM_W1U;
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j)
                if (table[i * n + j]) tp.rows[i][0] |= 1u << j;
    } else if (lo >= -2 && hi <= 1 && words2 <= 2) {
        mode = words2 == 1 ? TM_W2S1 : TM_W2S2;
    } else if (lo >= 0 && hi <= 3 && words2 <= 2) {
        mode = words2 == 1 ? TM_W2U1 : TM_W2U2;
    } else {
        mode = TM_LUT;
    }
    if (mode >= TM_W2S1 && mode <= TM_W2U2) {
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) {
                const uint32_t code = (uint32_t)table[i * n + j] & 3u;
                const int bit = j * 2;
                tp.rows[i][bit >> 5] |= code << (bit & 31);
            }
    }
    return FP8A_OK;
}

// The error tables the E4M3 / E5M2 matrix-core form (gemm_f8mx.h) and its satellites -- the VALU TM_F8
// form, the depthwise table form (conv_tbx.h), the word-image hand-off -- can run: every
// entry >= 0, so the approximate magnitude never exceeds the golden one and the F7 sign rule cannot fire
// (what Q_R flushes in the golden product it flushes in the approximate one), and every
// N = (2^M + m_a)(2^M + m_b) - 2^M t >= 1, so V' = N 2^-2M is positive, normal and -- N <= 225 -- exact in
// bf16.  *vmin: the lowest binade of any V' (0 for the zero and the built-in tables, >= -2M).  A zeroed
// pack (no table, approx off) passes with vmin 0.
static bool xm_table_form(const TablePack &tp, int Mw, int *vmin) {
    if (Mw < 1 || Mw > 5) return false;
    const int n = 1 << Mw;
    int lo = 1;
    for (int ma = 0; ma < n; ++ma)
        for (int mb = 0; mb < n; ++mb) {
            const int t = tp.raw[ma * n + mb];
            const int N = (n + ma) * (n + mb) - n * t;
            if (t < 0 || N < 1) return false;
            int b = 0;
            while ((N >> (b + 1)) != 0) ++b;  // floor(log2 N)
            lo = std::min(lo, b - 2 * Mw);
        }
    if (vmin) *vmin = lo;
    return true;
}

// Fallback statistics since load (or the last reset): [0] launches whose gated exact kernel
// ran, [1] 64 x 64 output units it recomputed, [2] launches rerun in gemm_tt_kernel's f32 form
// (gemm_tt16_kernel's f16 window left), [3] tensor-bias launches recomputed by
// conv_tb_direct_kernel.  Read with fp8a_fallback_stats (include/fp8approx.h).
__device__ unsigned long long g_fallback[4];

// Sums the split-K partials in split order (deterministic) and writes the output mapping.
// Partial layout: row-major [M][N] (rowmajor output) or [img][N][hw] (NCHW output).
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const GemmArgs p) {
    // (the fast forms where the launch's one test allows: sc.fqf, StoreCtx; the per-value work is
    // splitk_finish4 / splitk_finish1, fp8approx_common.h, shared with the in-launch sum)
    const StoreCtx sc = store_ctx<true>(p);
    const int64_t MN = p.M * p.N;
    uint32_t sehi = 0, neg = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    if (splitk_vec(p)) {
        for (int64_t q4 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q4 < MN / 4; q4 += stride)
            splitk_finish4<true, true, true>(p, sc, q4 * 4, sehi, neg);
    } else {
        for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < MN; q += stride)
            splitk_finish1<true, true, true>(p, sc, q, sehi, neg);
    }
    if (p.em.w) {
        wave_max_atomic(p.em.invalid + 5, sehi);
        wave_sign_record(p.em.invalid + 6, neg);
    }
}

// A(m, k) for the exact kernels: matrix or implicit im2col (through the fused input quantizer
// when there is one).
__device__ __forceinline__ float load_A(const GemmArgs &p, int64_t m, int64_t k) {
    if (!p.conv) {
        const float v = p.A[m * p.lda + k];
        if (p.fqin.mx == nullptr) return v;
        const float mx = *p.fqin.mx;
        return fq_apply(v, mx, fq_bias(mx, p.fqin.E, p.fqin.M), p.fqin.M, p.fqin.S);
    }
    const int64_t hw = p.Ho * p.Wo, img = m / hw, pix = m - img * hw;
    const int64_t ho = pix / p.Wo, wo = pix - ho * p.Wo;
    const int64_t taps = (int64_t)p.kh * p.kw, c = k / taps, t = k - c * taps, ky = t / p.kw, kx = t - ky * p.kw;
    const int64_t hi = ho * p.sh - p.ph + ky * p.dh, wi = wo * p.sw - p.pw + kx * p.dw;
    if (hi < 0 || hi >= p.H || wi < 0 || wi >= p.W) return 0.0f;
    const float v = p.X[((img * p.Cin + p.cbase + c) * p.H + hi) * p.W + wi];
    if (p.fqin.mx == nullptr) return v;
    const float mx = *p.fqin.mx;
    return fq_apply(v, mx, fq_bias(mx, p.fqin.E, p.fqin.M), p.fqin.M, p.fqin.S);
}

__device__ __forceinline__ void gemm_exact_units(const GemmArgs &p, uint32_t f, const DFmt &fA, const DFmt &fR, bool tb);

__global__ __launch_bounds__(256) void gemm_exact_kernel(const GemmArgs p) {
    const bool tb = p.flags & F_TB;
    if (p.post_bout != nullptr && blockIdx.x == 0 && threadIdx.x == 0) {  // the output quantizer's bias
        const float b = fq_bias(*p.post_fq.mx, p.post_fq.E, p.post_fq.M);
        *p.post_bout = b;
        *p.post_ibout = (int32_t)b;
    }
    const DFmt fA = dfmt(p.E, p.Mw, *p.bA, tb), fR = dfmt(p.E, p.Mw, *p.bR, tb);
    if (p.flag == nullptr) {  // the tensor-bias path: the exact kernel is the product itself
        for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < p.M * p.N;
             idx += (int64_t)gridDim.x * blockDim.x) {
            const int64_t m = idx % p.M, n = idx / p.M;
            const DFmt fB = dfmt(p.E, p.Mw, p.bB[n * p.bBs], tb);
            float s = 0.0f, part = 0.0f;
            for (int64_t k = 0; k < p.K; ++k) {
                part += exact_term(load_A(p, m, k), p.B[k * p.sbk + n * p.sbn], fA, fB, fR, p.tab.raw, p.flags);
                if ((k & 15) == 15) {
                    s += part;
                    part = 0.0f;
                }
            }
            s += part;
            const int64_t o = out_index(p, m, n);
            const float r = post1(p, o, epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, p.coff + n, s), post_bias(p));
            p.C[o] = r;
            if (p.em.w) {
                uint32_t sh = 0, ng = 0;
                emit1(p, emit_ctx(p), o, r, sh, ng);
                if (sh) atomicMax(p.em.invalid + 5, sh);
                sign_record(p.em.invalid + 6, ng);
            }
        }
        return;
    }
    // Gated after a fast launch: nothing to do unless it flagged (uniform per grid; the grid is
    // capped, so the no-op case costs one small launch); then only the marked 64 x 64 units
    // (every unit with FB_ALL), one unit per block step: thread = (row, 16 columns).  The kernel
    // ends the launch: it reports the flag word to the caller (flag_out) and zeroes the flag
    // arena's other slot (arena_clear: the previous launch's words)
    arena_clear(p.arena_clr, p.arena_clr16);
    const uint32_t f = __hip_atomic_load(p.flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p.flag_out && blockIdx.x == 0 && threadIdx.x == 0) *p.flag_out = f;
    if (f & FB_ANY) gemm_exact_units(p, f, fA, fR, tb);
}

// The marked units of a flagged launch (gemm_exact_kernel); every thread returns here.
__device__ __forceinline__ void gemm_exact_units(const GemmArgs &p, uint32_t f, const DFmt &fA, const DFmt &fR, bool tb) {
    const bool all = (f & FB_ALL) != 0u || p.urow == nullptr;
    const int64_t nur = (p.M + 63) >> 6, nuc = (p.N + 63) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_fallback[0], 1ull);
    const float pb = post_bias(p);
    const EmitCtx ec = emit_ctx(p);
    for (int64_t u = blockIdx.x; u < nur * nuc; u += gridDim.x) {
        const int64_t ur = u / nuc, uc = u - ur * nuc;
        if (!all && !p.urow[ur] && !p.ucol[uc] && !(p.utile[u] & UT_EXACT)) continue;  // (block-uniform)
        if (threadIdx.x == 0) atomicAdd(&g_fallback[1], 1ull);
        const int64_t m = 64 * ur + (threadIdx.x & 63), nb = 64 * uc + 16 * (threadIdx.x >> 6);
        if (m >= p.M) continue;
        float s[16], part[16];
        DFmt fB[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            s[j] = part[j] = 0.0f;
            fB[j] = dfmt(p.E, p.Mw, p.bB[min(nb + j, p.N - 1) * p.bBs], tb);
        }
        for (int64_t k = 0; k < p.K; ++k) {
            const float a = load_A(p, m, k);
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int64_t n = min(nb + j, p.N - 1);
                part[j] += exact_term(a, p.B[k * p.sbk + n * p.sbn], fA, fB[j], fR, p.tab.raw, p.flags);
                if ((k & 15) == 15) {
                    s[j] += part[j];
                    part[j] = 0.0f;
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int64_t n = nb + j;
            if (n >= p.N) break;
            const int64_t o = out_index(p, m, n);
            const float r = post1(p, o, epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, p.coff + n, s[j] + part[j]), pb);
            p.C[o] = r;
            if (p.em.w) {
                uint32_t sh = 0, ng = 0;
                emit1(p, ec, o, r, sh, ng);
                if (sh) atomicMax(p.em.invalid + 5, sh);
                sign_record(p.em.invalid + 6, ng);
            }
        }
    }
}

__global__ __launch_bounds__(256) void terms_kernel(const GemmArgs p, float *T) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= p.M * p.K * p.N) return;
    const int64_t n = idx % p.N, k = (idx / p.N) % p.K, m = idx / (p.N * p.K);
    const bool tb = p.flags & F_TB;
    const DFmt fA = dfmt(p.E, p.Mw, *p.bA, tb), fR = dfmt(p.E, p.Mw, *p.bR, tb);
    const DFmt fB = dfmt(p.E, p.Mw, p.bB[n * p.bBs], tb);
    T[idx] = exact_term(p.A[m * p.lda + k], p.B[k * p.sbk + n * p.sbn], fA, fB, fR, p.tab.raw, p.flags);
}

__global__ __launch_bounds__(256) void decompose_kernel(const float *x, int64_t rows, int64_t cols, int64_t ld,
                                                        int E, int M, const int32_t *bias, int64_t bs,
                                                        uint32_t flags, int32_t *expo, int32_t *mant) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * cols) return;
    const int64_t r = idx / cols, c = idx - r * cols;
    const DFmt f = dfmt(E, M, bias[r * bs], flags & F_TB);
    int e, m;
    exact_dec(x[r * ld + c], f, flags & F_GCLIP, e, m);
    expo[idx] = e;
    mant[idx] = m;
}

__global__ __launch_bounds__(256) void quant_kernel(const float *x, int64_t n, int E, int M, const int32_t *bias,
                                                    uint32_t flags, float *out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n) return;
    const DFmt f = dfmt(E, M, *bias, flags & F_TB);
    out[idx] = exact_q(x[idx], f, flags & F_GCLIP);
}

// im2col, K ordered (c, ky, kx) like approx_calculation.py:738-745.
__global__ __launch_bounds__(256) void im2col_kernel(const float *x, float *out, int64_t Bn, int64_t C, int64_t H,
                                                     int64_t W, int kh, int kw, int sh, int sw, int ph, int pw,
                                                     int dh, int dw, int64_t Ho, int64_t Wo) {
    const int64_t K = C * kh * kw;
    const int64_t total = Bn * Ho * Wo * K;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = idx % K, m = idx / K;
        const int64_t kx = k % kw, ky = (k / kw) % kh, c = k / (kw * kh);
        const int64_t wo = m % Wo, ho = (m / Wo) % Ho, b = m / (Wo * Ho);
        const int64_t hi = ho * sh - ph + ky * dh, wi = wo * sw - pw + kx * dw;
        float v = 0.0f;
        if (hi >= 0 && hi < H && wi >= 0 && wi < W) v = x[((b * C + c) * H + hi) * W + wi];
        out[idx] = v;
    }
}

// Single-output-channel groups (depthwise): tensor-bias semantics, direct from NCHW x.
// TB = false: the same literal restatement with int-bias semantics -- the v5 model's depthwise
// convolutions (v5 has no tensor-bias path: its products are the GEMM path's, with a zero
// operand's NONZERO term at every padded position, as the reference's im2col supplies them).
template <bool TB>
__global__ __launch_bounds__(256) void conv_tb_direct_kernel(const float *x, const float *w, float *y, int64_t Bn,
                                                             int64_t Cin, int64_t H, int64_t W, int64_t Cout,
                                                             int kh, int kw, int sh, int sw, int ph, int pw, int dh,
                                                             int dw, int groups, int64_t Ho, int64_t Wo, int E,
                                                             int Mw, const int32_t *bA, const int32_t *bW,
                                                             const int32_t *bR, TablePack tab, uint32_t flags,
                                                             const uint32_t *gate, uint32_t *gate_out, uint4 *clr,
                                                             uint32_t clr16, const float2 *ep, int ep_act,
                                                             float ep_lo, float ep_hi, FqIn fq) {
    // after conv_tb_fast_kernel: run only if it flagged inputs outside its exactness window.  The
    // gate word is a slot of the stream's flag arena (flag_arena): this kernel reports it to the
    // caller's workspace word (gate_out) and zeroes the arena's other slot (arena_clear)
    arena_clear(clr, clr16);
    const uint32_t gv = gate != nullptr ? __hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 1u;
    if (gate_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *gate_out = gv;
    if (gv == 0u) return;
    if (gate != nullptr && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_fallback[3], 1ull);
    const int64_t total = Bn * Cout * Ho * Wo;
    const int64_t cpg = Cin / groups;   // input channels per group
    const DFmt fA = dfmt(E, Mw, *bA, TB), fR = dfmt(E, Mw, *bR, TB);
    const float fmx = fq.mx ? *fq.mx : 0.0f, fbias = fq.mx ? fq_bias(fmx, fq.E, fq.M) : 0.0f;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t wo = idx % Wo, ho = (idx / Wo) % Ho, co = (idx / (Wo * Ho)) % Cout, b = idx / (Wo * Ho * Cout);
        const int64_t g = co / (Cout / groups);
        const DFmt fB = dfmt(E, Mw, bW[co], TB);
        float s = 0.0f, part = 0.0f;
        int cnt = 0;
        for (int64_t c = 0; c < cpg; ++c)
            for (int ky = 0; ky < kh; ++ky)
                for (int kx = 0; kx < kw; ++kx) {
                    const int64_t hi = ho * sh - ph + ky * dh, wi = wo * sw - pw + kx * dw;
                    float a = (hi >= 0 && hi < H && wi >= 0 && wi < W)
                                  ? x[((b * Cin + g * cpg + c) * H + hi) * W + wi] : 0.0f;
                    if (fq.mx) a = fq_apply(a, fmx, fbias, fq.M, fq.S);
                    const float bv = w[((co * cpg + c) * kh + ky) * kw + kx];
                    part += exact_term(a, bv, fA, fB, fR, tab.raw, TB ? (flags | F_TB) : flags);
                    if (++cnt == 16) {
                        s += part;
                        part = 0.0f;
                        cnt = 0;
                    }
                }
        y[idx] = epi(ep, ep_act, ep_lo, ep_hi, co, s + part);
    }
}

// Single-output-channel groups (depthwise) with the tensor-bias semantics, fast form.
// With int32-tensor biases >= 2 the reference's param_prepare yields min_norm = 0 (quirk F5):
// no operand or result is subnormal, every nonzero value decodes at its own binade.  For
// exactly representable operands (M-bit mantissa at their binade, |x| in [2^-62, 2^50]) and
// with_s2nn2s_opt on, golden_clip_OF off, the term is then
//   v0 = a*b - T[mA][mB] * cA * cB * 2^-M                         (exact, as in the GEMM)
//   sign quirk F7: Q_R(g) is 0 only in the binade 2^-bR (expo 0, mantissa rounding to 0), where
//                  a negative g gives the term |v0| (with quant_btw_mult_accu only: without it g
//                  is not quantized and the term keeps g's sign)
//   Q_R, tb form: round at the value's own binade with the F6 clamp, except in the binade
//                  [2^-bR, 2^(1-bR)) (expo field 0), whose decode is 2^(1-bR) * m / 2^M, i.e.
//                  2 * (Q(x) - sign * 2^-bR)
// Anything else sets the gate word and conv_tb_direct_kernel recomputes the launch exactly.
// One thread per output pixel; grid (pixel chunks, Cout, Bn); the channel's decoded weights and
// the error table live in LDS.
constexpr int TBF_MAXK = 512;

__global__ __launch_bounds__(256) void conv_tb_fast_kernel(const float *x, const float *w, float *y, int64_t Cin,
                                                           int64_t H, int64_t W, int64_t Cout, int kh, int kw,
                                                           int sh, int sw, int ph, int pw, int dh, int dw, int groups,
                                                           int64_t Ho, int64_t Wo, int Mw, const int32_t *bA,
                                                           const int32_t *bW, const int32_t *bR, TablePack tab,
                                                           uint32_t flags, uint32_t *gate, const float2 *ep,
                                                           int ep_act, float ep_lo, float ep_hi) {
    __shared__ float sw_v[TBF_MAXK], sw_c[TBF_MAXK];
    __shared__ int32_t sw_m[TBF_MAXK];
    __shared__ float sT[1024];
    const int64_t co = blockIdx.y, img = blockIdx.z;
    const int64_t cpg = Cin / groups, g = co / (Cout / groups);
    const int K = (int)(cpg * kh * kw), M = Mw, n = 1 << M;
    const int a_b = *bA, r_b = *bR, w_b = bW[co];
    const bool approx = flags & F_APPROX, qbma = flags & F_QBMA;
    bool bad = !(a_b >= 2 && w_b >= 2 && r_b >= 2 && a_b <= 120 && w_b <= 120 && r_b <= 120 && K <= TBF_MAXK);
    const uint32_t offgrid = (1u << (23 - M)) - 1u;
    for (int i = threadIdx.x; i < n * n; i += blockDim.x) sT[i] = approx ? (float)tab.raw[i] : 0.0f;
    for (int k = threadIdx.x; k < K && k < TBF_MAXK; k += blockDim.x) {
        const float v = w[co * K + k];
        const uint32_t ua = __float_as_uint(v) & 0x7FFFFFFFu;
        bad |= (ua != 0u) && ((ua & offgrid) != 0u || ua < 0x20800000u || ua > 0x58800000u);
        sw_v[k] = v;
        sw_c[k] = __uint_as_float(__float_as_uint(v) & 0xFF800000u) * p2(-M);  // cB * 2^-M (0 for zeros)
        sw_m[k] = (int32_t)((ua >> (23 - M)) & (uint32_t)(n - 1));
    }
    __syncthreads();
    // Q_R constants (tb form: no subnormal floor)
    const float kb = 2.0f - p2(-M) - p2(-22), kc = 1.5f * p2(23 - M);
    const uint32_t q0exp = (uint32_t)(127 - r_b) << 23;             // exponent field of 2^-bR
    const float zlo = p2(-r_b), zhi = p2(-r_b) * (1.0f + p2(-M - 1));  // |g| where Q_R(g) == 0
    const int64_t pix = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = pix < Ho * Wo;
    const int64_t ho = live ? pix / Wo : 0, wo = live ? pix - ho * Wo : 0;
    float acc = 0.0f;
    int k = 0;
    for (int64_t c = 0; c < cpg; ++c) {
        const float *xc = x + ((img * Cin + g * cpg + c) * H) * W;
        for (int ky = 0; ky < kh; ++ky) {
            const int64_t hi = ho * sh - ph + (int64_t)ky * dh;
            for (int kx = 0; kx < kw; ++kx, ++k) {
                const int64_t wi = wo * sw - pw + (int64_t)kx * dw;
                const float a = (live && hi >= 0 && hi < H && wi >= 0 && wi < W) ? xc[hi * W + wi] : 0.0f;
                const uint32_t ua = __float_as_uint(a) & 0x7FFFFFFFu;
                bad |= (ua != 0u) && ((ua & offgrid) != 0u || ua < 0x20800000u || ua > 0x58800000u);
                const float cA = __uint_as_float(__float_as_uint(a) & 0xFF800000u);
                const int mA = (int)((ua >> (23 - M)) & (uint32_t)(n - 1));
                const float b = sw_v[k];
                const float gq = a * b;  // exact
                float v = __fmaf_rn(-sT[mA * n + sw_m[k]], cA * sw_c[k], gq);
                // F7: Q_R(g) == 0 (so the sign is +) only for |g| in [2^-bR, 2^-bR (1 + 2^-(M+1))]; without
                // quant_btw_mult_accu the sign is that of the unquantized g (v9:35-36, 68)
                const float ag = fabsf(gq);
                if (qbma && gq < 0.0f && ag >= zlo && ag <= zhi) v = fabsf(v);
                if (qbma) {
                    const uint32_t pb = __float_as_uint(v) & 0x7F800000u;
                    const float pe = __uint_as_float(pb);
                    const float bd = pe * kb;
                    const float xs = __builtin_amdgcn_fmed3f(v, -bd, bd);
                    const float cc = pe * kc;
                    float r = (xs + cc) - cc;
                    if (pb == q0exp) r = 2.0f * (r - copysignf(pe, v));  // expo field 0: 2^(1-bR) m / 2^M
                    v = r;
                }
                acc += v;
            }
        }
    }
    const bool anybad = __syncthreads_or(bad ? 1 : 0);
    if (anybad) {
        if (threadIdx.x == 0) atomicOr(gate, 1u);
        return;
    }
    if (live) y[((img * Cout + co) * Ho + ho) * Wo + wo] = epi(ep, ep_act, ep_lo, ep_hi, co, acc);
}


// FP8 fake quantizer (fp8_quantizer.py:97-173), one sign bit.
__global__ __launch_bounds__(256) void fp8_quantize_kernel(const float *x, int64_t rows, int64_t inner,
                                                           const float *maxval, int per_row, int E, int M,
                                                           int sign_bits, float *out, float *bias_out,
                                                           int32_t *ibias_out) {
    const int64_t total = rows * inner;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = per_row ? idx / inner : 0;
        const float mx = maxval[r];
        const float bias = fq_bias(mx, E, M);
        out[idx] = fq_apply(x[idx], mx, bias, M, sign_bits);
        if ((idx % inner) == 0) {
            if (bias_out) bias_out[r] = bias;
            if (ibias_out) ibias_out[r] = (int32_t)bias;
        }
    }
}

// nn.MaxPool2d (dilation 1, floor mode) on NCHW fp32: the stem pooling between the first conv
// and layer1 of the ResNets (torchvision layout), one thread per output, NaN-propagating like
// ATen's max_pool2d.  Not an approx op: it sits on the benchmarked step (torch's kernel took
// 0.59 ms of a 38 ms ResNet-18 batch-256 step).
__global__ __launch_bounds__(256) void max_pool2d_kernel(const float *x, float *y, int64_t planes, int H, int W,
                                                         int Ho, int Wo, int kh, int kw, int sh, int sw, int ph,
                                                         int pw) {
    const int64_t total = planes * Ho * Wo;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int wo = (int)(idx % Wo);
        const int64_t t = idx / Wo;
        const int ho = (int)(t % Ho);
        const int64_t pl = t / Ho;
        const float *xp = x + pl * H * W;
        float m = -INFINITY;
        const int h0 = ho * sh - ph, w0 = wo * sw - pw;
        for (int ky = 0; ky < kh; ++ky) {
            const int hi = h0 + ky;
            if ((unsigned)hi >= (unsigned)H) continue;
            for (int kx = 0; kx < kw; ++kx) {
                const int wi = w0 + kx;
                if ((unsigned)wi >= (unsigned)W) continue;
                const float v = xp[(int64_t)hi * W + wi];
                m = (v > m || v != v) ? v : m;
            }
        }
        y[idx] = m;
    }
}

// The ResNet stem configuration (3x3 window, stride 2, padding 1) on rows of W % 8 == 0: each
// thread makes 4 consecutive outputs of one row from two aligned float4 loads + one scalar per
// input row (27 scalar loads before), one float4 store.  Same scan order (window row, then
// column) and NaN rule as max_pool2d_kernel, so the same bits.
// nn.AvgPool2d with one output per plane (fp8a_avg_pool2d_plane; MobileNetV2's head).  ATen's
// avg_pool2d sums the window in row-major order in fp32 and divides by kh kw once; so does this
// (the same bits).  ATen reads with one thread per plane (lanes a plane apart: 0.41 ms for the
// head at batch 512); here a workgroup stages PB consecutive planes through LDS with contiguous
// loads (plane stride padded odd: conflict-free per-thread sums), then thread = plane.
__global__ __launch_bounds__(128) void avg_pool_plane_kernel(const float *x, float *y, int64_t planes, int PB, int W,
                                                             int hw, int ps, int kh, int kw, float inv_hw) {
    extern __shared__ float ap_sm[];
    const int tid = threadIdx.x;
    const int64_t P0 = (int64_t)blockIdx.x * PB;
    const int npl = (int)min((int64_t)PB, planes - P0), n = npl * hw;
    const float *xb = x + P0 * hw;
    for (int d0 = tid; d0 < n; d0 += 4 * 128) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = d0 + 128 * u < n ? xb[d0 + 128 * u] : 0.0f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int d = d0 + 128 * u;
            if (d < n) {
                const int pl = dw_div(d, hw, inv_hw);
                ap_sm[pl * ps + d - pl * hw] = v[u];
            }
        }
    }
    __syncthreads();
    for (int t = tid; t < npl; t += 128) {
        const float *s = ap_sm + t * ps;
        float acc = 0.0f;
        for (int r = 0; r < kh; ++r)
            for (int c = 0; c < kw; ++c) acc += s[r * W + c];
        y[P0 + t] = acc / (float)(kh * kw);
    }
}

__global__ __launch_bounds__(256) void max_pool2d_s2k3_kernel(const float *x, float *y, int64_t planes, int H, int W,
                                                             int Ho) {
    const int Wq = W / 8;  // 4-output groups per output row (Wo = W / 2)
    const int64_t total = planes * Ho * Wq;
    for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (int64_t)gridDim.x * blockDim.x) {
        const int q = (int)(idx % Wq);
        const int64_t t = idx / Wq;
        const int ho = (int)(t % Ho);
        const int64_t pl = t / Ho;
        const float *xp = x + pl * H * W;
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        const int c0 = 8 * q;  // input columns c0 - 1 .. c0 + 7
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int hi = 2 * ho - 1 + ky;
            if ((unsigned)hi >= (unsigned)H) continue;
            const float *r = xp + (int64_t)hi * W + c0;
            const float4 a = *reinterpret_cast<const float4 *>(r), b = *reinterpret_cast<const float4 *>(r + 4);
            const float v[9] = {c0 > 0 ? r[-1] : -INFINITY, a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
            for (int o = 0; o < 4; ++o)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) {
                    if (o == 0 && kx == 0 && c0 == 0) continue;  // left padding
                    const float u = v[2 * o + kx];
                    m[o] = (u > m[o] || u != u) ? u : m[o];
                }
        }
        *reinterpret_cast<float4 *>(y + (pl * Ho + ho) * (int64_t)(W / 2) + 4 * q) = make_float4(m[0], m[1], m[2], m[3]);
    }
}

// ------------------------------------------------------------------------- host dispatch
// The GEMM kernel families are instantiated and launched in their own translation units
// (fp8approx_launch.h): gemm_fast_kernel in k_fast.hip, gemm_f8mx_kernel in k_f8mx.hip, the
// tile-table kernels in k_tt.hip, the v5 form in k_v5.hip.
// E4M3 (XF 0) or E5M2 (mant_width 2) result grid; E5M2 launches both its kernels, the plain one
// (XF 1) over every tile and the halved-block one (XF 2), which recomputes only the tiles the plain
// one marked UT_HALF (the top binade, gemm_f8mx.h) and exits at once without FB_HALF
static void launch_f8mx(const GemmArgs &a, hipStream_t s) {
    if (a.Mw == 2) {
        launch_f8mx_xf1(a, s);
        launch_f8mx_xf2(a, s);
    } else {
        launch_f8mx_xf0(a, s);
    }
}

// ------------------------------------------------------------------------- options
// One table for fp8a_set_option and the FP8A_<NAME> environment variables read at load (documented in
// include/fp8approx.h).  kind: how fp8a_set_option normalises a value -- as given, != 0, max(lo, v) or
// min(hi, max(lo, v)); the environment's value takes the same normalisation unless env_raw.
enum OptKind { OPT_RAW, OPT_BOOL, OPT_AT_LEAST, OPT_CLAMP };
enum OptId { OPT_XM_NCG, OPT_XM_SIGN_ROWS, OPT_XM_PIPE, OPT_XM_WAVE_ROWS, OPT_SPLITK_FIXUP, OPT_SPLITK, OPT_FQ_FAST,
             OPT_AF32_MAXCT, OPT_TT_BAND, OPT_TT16_MINK, OPT_TBX_RW, OPT_TBS, OPT_DW_LDS, OPT_DW_TARGET, OPT_DN_DIRECT,
             OPT_V5DS, OPT_DW3, OPT_MSE_GROUP, OPT_FQT_TARGET_WGS, OPT_N };
struct Option {
    const char *name, *env;
    int def, kind, lo, hi;
    bool env_raw;
    int value;
};
static Option g_opts[OPT_N] = {
    {"xm_ncg", "FP8A_XM_NCG", 0, OPT_RAW},  // gemm_f8mx_kernel's tile width (1 | 2 | 4; 0: xm_ncg's choice)
    {"xm_sign_rows", "FP8A_XM_SIGN_ROWS", 1, OPT_BOOL, 0, 0, true},  // tile table: only the sign rows A addresses
    {"xm_pipe", "FP8A_XM_PIPE", 1, OPT_BOOL},            // K loop's LDS reads one stage ahead
    {"xm_wave_rows", "FP8A_XM_WAVE_ROWS", 1, OPT_BOOL},  // 128 x 64 instances: waves by rows
    {"splitk_fixup", "FP8A_SPLITK_FIXUP", 0, OPT_BOOL},  // split-K partials summed inside the launch (3v: slower)
    {"splitk", "FP8A_SPLITK", 0, OPT_AT_LEAST, 0},       // the forced split count (0: choose_splits)
    {"fq_fast", "FP8A_FQ_FAST", 1, OPT_BOOL},  // the matrix-core path's fake quantizers run fq_apply_fast / fq_word
    {"af32_maxct", "FP8A_AF32_MAXCT", 1, OPT_AT_LEAST, 0},  // column tiles up to which A is staged from fp32 (xm_af32)
    {"tt_band", "FP8A_TT_BAND", 1, OPT_RAW},                // gemm_tt_kernel's band / zero wave-tile forms
    {"tt16_mink", "FP8A_TT16_MINK", 64, OPT_AT_LEAST, 0},   // smallest K of an unsigned-table launch on gemm_tt16
    {"tbx_rw", "FP8A_TBX_RW", 2, OPT_RAW},  // output rows per thread of conv_tbx_kernel (2 needs undilated rows)
    {"tbs", "FP8A_TBS", 2, OPT_RAW},        // table-form depthwise 3x3: conv_tbsg (2), conv_tbs (1), conv_tbx (0)
    {"dw_lds", "FP8A_DW_LDS", 40960, OPT_CLAMP, 4096, 65536, true},   // LDS bytes the staged depthwise plans allow
    {"dw_target", "FP8A_DW_TARGET", 4096, OPT_AT_LEAST, 256, 0, true},  // outputs per workgroup those plans aim at
    {"dn_direct", "FP8A_DN_DIRECT", 1, OPT_RAW},  // exact convs with K <= 32, N <= 64 on dn_direct_kernel
    {"v5ds", "FP8A_V5DS", 1, OPT_RAW},            // v5 depthwise 3x3 on conv_v5ds_kernel (0: conv_v5dw_kernel)
    {"dw3", "FP8A_DW3", 2, OPT_RAW},              // exact depthwise 3x3: dn_dw3g (2), dn_dw3 (1), dn_group_conv (0)
    {"mse_group", "FP8A_MSE_GROUP", 1, OPT_BOOL},  // fp8a_fp8_mse_search's grouped kernel (fq_mse.h)
    {"fqt_target_wgs", "FP8A_FQT_TARGET_WGS", FQT_TARGET_WGS, OPT_CLAMP, 1, 1 << 20},  // fqt_parts' workgroups per launch (fq_train.h)
};
static int opt_norm(const Option &o, int v) {
    return o.kind == OPT_BOOL ? v != 0 : o.kind == OPT_AT_LEAST ? std::max(o.lo, v)
         : o.kind == OPT_CLAMP ? std::min(o.hi, std::max(o.lo, v)) : v;
}
static const bool g_opts_loaded = [] {
    for (Option &o : g_opts) {
        const char *e = getenv(o.env);
        o.value = !e ? o.def : o.env_raw ? atoi(e) : opt_norm(o, atoi(e));
    }
    return true;
}();
static inline int opt(OptId id) { return g_opts[id].value; }

// The FP8A_NO_* switches of A/B runs (set means on; FP8A_CHAIN_TBX: a nonzero number), read once at load.
struct EnvSwitches {
    bool no_f8 = getenv("FP8A_NO_F8") != nullptr, no_f8_e5m2 = getenv("FP8A_NO_F8_E5M2") != nullptr;
    bool no_v5mx = getenv("FP8A_NO_V5MX") != nullptr, no_tt = getenv("FP8A_NO_TT") != nullptr;
    bool no_tt16 = getenv("FP8A_NO_TT16") != nullptr, no_mx = getenv("FP8A_NO_MX") != nullptr;
    bool no_tbx = getenv("FP8A_NO_TBX") != nullptr, no_v5dw = getenv("FP8A_NO_V5DW") != nullptr;
    bool chain_tbx = getenv("FP8A_CHAIN_TBX") != nullptr && atoi(getenv("FP8A_CHAIN_TBX")) != 0;
};
static const EnvSwitches g_env{};

// gemm_f8mx_kernel's tile width: the fewest padded columns, ties to the wider tile (N = 16 -> 16,
// 24 / 32 / 96 / 160 -> 32, multiples of 64 -> 64); option "xm_ncg" forces it.
static int xm_ncg(int64_t N) {
    const int forced = opt(OPT_XM_NCG);
    if (forced == 1 || forced == 2 || forced == 4) return forced;
    int best = 4;
    int64_t bp = (N + 63) / 64 * 64;
    for (int c : {2, 1}) {
        const int64_t pad = (N + 16 * c - 1) / (16 * c) * (16 * c);
        if (pad < bp) {
            bp = pad;
            best = c;
        }
    }
    return best;
}

static void launch_fast(int mode, const GemmArgs &a, hipStream_t s) {
    const int64_t tiles = ((a.M + BM - 1) / BM) * ((a.N + BN - 1) / BN);
    const dim3 grid((unsigned)(tiles * a.splits));
    if (mode == TM_V5) {  // the v5 model has no s2n / qbma / golden-clip variants
        if (a.aw && a.wfmt == 4) launch_v5mx(a, s);  // the matrix-core form (gemm_v5mx.h)
        else launch_fast_p0(TM_V5, false, a, grid, s);
        return;
    }
    if (mode == TM_QAMAA) {
        launch_fast_p0(TM_QAMAA, false, a, grid, s);
        return;
    }
    if (a.aw && (a.wfmt == 1 || a.wfmt == 2)) {  // E3M4 / E2M5: the tile-table kernels (run_gemm)
        launch_tt(a, grid, s);
        return;
    }
    if (mode == TM_F8) {  // s2n + qbma, no golden clip (selected in run_gemm)
        // matrix-core accumulation on pre-decoded operands (gemm_f8mx.h) when run_gemm staged
        // them, else the VALU-accumulating form
        if (a.aw || a.af32) launch_f8mx(a, s);
        else launch_fast_p3(TM_F8, false, a, grid, s);
        return;
    }
    const bool s2n = a.flags & F_S2N, q = a.flags & F_QBMA, gc = a.flags & F_GCLIP;
    if (s2n) q ? launch_fast_p3(mode, gc, a, grid, s) : launch_fast_p2(mode, gc, a, grid, s);
    else q ? launch_fast_p1(mode, gc, a, grid, s) : launch_fast_p0(mode, gc, a, grid, s);
}

static int check_format(int E, int Mw) {
    if (E < 1 || Mw < 1 || Mw > 5 || E > 6 || E + Mw > 8)
        return fail(FP8A_EFORMAT, "Invalid combination of expo_width and mant_width");
    return FP8A_OK;
}

constexpr size_t FLAG_BYTES = 256;  // workspace prefix holding the off-grid flag word

// Launch paths taken by run_gemm since load (fp8a_path_stats): host-side counters.
enum { PATH_F8MX = 0, PATH_TT = 1, PATH_TT16 = 2, PATH_FAST = 3, PATH_EXACT = 4, PATH_DENSE = 5, PATH_V5MX = 6,
       PATH_N = 7 };
static std::atomic<uint64_t> g_paths[PATH_N];
// the path of a launch run_gemm has set up: by its pre-decoded operands (a.aw) and their word format
static int gemm_path(const GemmArgs &a) {
    return !a.aw ? PATH_FAST : a.wfmt == 0 ? PATH_F8MX : a.wfmt == 1 ? PATH_TT : a.wfmt == 4 ? PATH_V5MX : PATH_TT16;
}

// Kernel timing (fp8a_kernel_timing / fp8a_kernel_time): while on, run_gemm brackets the product
// kernel launch(es) of every GEMM (launch_fast: gemm_f8mx_kernel, gemm_tt*_kernel, gemm_v5mx_kernel
// or gemm_fast_kernel -- not the operand pre-passes, split-K reduce or gated exact kernel) with HIP
// events on the launching stream, so a benchmark can report the dominant kernel's own time next to
// the op's.  Host-side, single-threaded use (benchmarks); events come from a pool.
struct KernelEv {
    hipEvent_t a, b;
    int path, dispatches;
    double macs;
};
static bool g_ktime = false;
static std::vector<KernelEv> g_kev;
static std::vector<hipEvent_t> g_evpool;
static hipEvent_t pool_event() {
    if (!g_evpool.empty()) {
        hipEvent_t e = g_evpool.back();
        g_evpool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return e;
}

// Compute units of the current device (cached); 256 (MI355X) when no device is visible.
static int device_cus() {
    static int cache[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        return 256;
    }
    if (cache[dev] == 0) {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
            (void)hipGetLastError();
            cus = 256;
        }
        cache[dev] = cus;
    }
    return cache[dev];
}

// Split-K factor for a fast launch, from a time model fitted on MI355X (ResNet-18 layers,
// FP8A_SPLITK = 1..6 sweeps).  The fast kernel holds 4 workgroups per CU (128 VGPRs), so a launch
// runs in rounds of 4*CUs tiles, each round lasting one tile's time (BM*BN*K products at about
// 4.4 G products/s per workgroup slot); a last, partly filled round costs min(1, 0.4 + 1.1*fill)
// of a full one (a half-filled round costs a full one, a 6 %-filled one 0.45).  Splitting K
// multiplies the tile count and divides the round length, and adds a pass that writes and
// re-reads S*M*N partial floats (charged at 2 TB/s).  Each split keeps at least 16 K-tiles.
// FP8A_SPLITK=<S> forces S (experiments).  g_splitk_launches: launches that ran split (their
// splitk_reduce_kernel stores the output), host-side, fp8a_splitk_stats.
static uint64_t g_splitk_launches = 0;
static int choose_splits(int64_t M, int64_t N, int64_t K) {
    const int forced = opt(OPT_SPLITK);
    const int64_t kt = (K + BK - 1) / BK;
    if (forced > 0) return (int)std::max<int64_t>(1, std::min<int64_t>(forced, kt));
    const int64_t tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
    const double slots = 4.0 * device_cus();
    static double rate = 0.0;  // approx-MAC/s of one 64x64 workgroup at 4 per CU (FP8A_SPLITK_RATE overrides)
    if (rate == 0.0) {
        const char *e = getenv("FP8A_SPLITK_RATE");
        rate = e ? std::max(1e8, atof(e)) : 4.4e9;
    }
    const double t_round = (double)BM * BN * K / rate;                      // s
    const double t_split = 2.0 * (double)M * N * sizeof(float) / 2.0e12;   // s per split
    double best = 1e300;
    int bs = 1;
    for (int S = 1; S <= 8; ++S) {
        if (S > 1 && kt < 16 * S) break;
        const double q = (double)tiles * S / slots, fl = std::floor(q), fr = q - fl;
        const double rounds = fl + (fr > 1e-9 ? std::min(1.0, 0.4 + 1.1 * fr) : 0.0);
        const double t = rounds / S * t_round + (S > 1 ? S * t_split : 0.0);
        if (t < best * (1.0 - 1e-3)) {
            best = t;
            bs = S;
        }
    }
    return bs;
}

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Bytes of the pre-decoded operands of the matrix-core E4M3 kernel (gemm_f8mx.h): A words
// (a_words of them) + B column pairs [Kpad][Npad / 2] of 8 bytes.
// The B image: the E4M3 / E5M2 column pairs ([kpad][npad / 2] uint2) or the v5 form's four table
// words per column ([kpad][npad] uint2, gemm_v5mx.h) -- sized for the larger.
static size_t xm_b_bytes(int64_t kpad, int64_t npad) { return align256((size_t)(kpad * npad) * 8); }
constexpr size_t XM_TABLE_IMAGE_BYTES = 16384;  // the static table image (largest: the tile-table kernels')
// The region's layout, as byte offsets from its start: A words, B image, table image, E5M2 B exponent ranges
struct XmOperandLayout {
    size_t bqw, lutw, ebr, total;
};
static XmOperandLayout xm_operand_layout(int64_t N, int64_t K, int64_t a_words) {
    const int64_t kpad = (K + BK - 1) / BK * BK, npad = (N + BN - 1) / BN * BN;
    XmOperandLayout l;
    l.bqw = align256((size_t)a_words * 4);
    l.lutw = l.bqw + xm_b_bytes(kpad, npad);
    l.ebr = l.lutw + XM_TABLE_IMAGE_BYTES;
    l.total = l.ebr + align256((size_t)(kpad * npad / 16) * 2);
    return l;
}
static size_t xm_operand_bytes(int64_t N, int64_t K, int64_t a_words) { return xm_operand_layout(N, K, a_words).total; }

// The per-unit fallback marks after the flag word: urow [nur], ucol [nuc], utile [nur * nuc] bytes.
static size_t unit_bytes(int64_t M, int64_t N) {
    const int64_t nur = (M + 63) / 64, nuc = (N + 63) / 64;
    return align256((size_t)(nur + nuc + nur * nuc));
}
static size_t head_bytes(int64_t M, int64_t N) { return FLAG_BYTES + unit_bytes(M, N); }

// (the partial tiles, then the in-launch sum's arrival counters: one word per output tile, sized for the
// smallest tile -- 128 rows or 16 columns -- of gemm_f8mx_kernel)
static int64_t splitk_counter_words(int64_t M, int64_t N) { return ((M + 63) / 64) * ((N + 15) / 16); }
static size_t splitk_part_bytes(int S, int64_t M, int64_t N) {
    return align256((size_t)S * (size_t)M * (size_t)N * sizeof(float));
}
static size_t splitk_bytes(int64_t M, int64_t N, int64_t K) {
    const int S = choose_splits(M, N, K);
    return S > 1 ? splitk_part_bytes(S, M, N) + align256((size_t)splitk_counter_words(M, N) * 4) : 0;
}


// flag word + unit marks + split-K partials + the matrix-core kernels' pre-decoded operands
// (gemm_f8mx.h).  conv_words: the conv word image's element count, 0 for a matrix A.
static size_t gemm_workspace_bytes(int64_t M, int64_t N, int64_t K, int64_t conv_words) {
    const int64_t a_words = conv_words > 0 ? conv_words : M * ((K + BK - 1) / BK * BK);
    return head_bytes(M, N) + splitk_bytes(M, N, K) + xm_operand_bytes(N, K, a_words);
}

// The table + hardware-fp8 form applies (TM_F8; run_gemm then takes the matrix-core kernel when
// the workspace holds its pre-decoded operands): E4M3 (e4m3 conversion) or E5M2 (bf8 conversion,
// round 4), a table of xm_table_form (no negative entry, every V' positive: the zero table, the built-in
// {0,1} table, a custom multiplier's), s2n + qbma, no golden clip, int-bias semantics, not v5.
// (E5M2 has no VALU TM_F8 form: without the pre-decoded operands it keeps its table mode.  E4M3's VALU
// TM_F8 form builds its V' from the raw table as xm_lut_word does, in fp32, so it takes the same tables.)
// FP8A_NO_F8=1 keeps the arithmetic forms; FP8A_NO_F8_E5M2=1 only for E5M2 (A/B runs).
static bool f8_form(int E, int Mw, uint32_t flags, const TablePack &tab) {
    const bool fmt = (E == 4 && Mw == 3) || (E == 5 && Mw == 2 && !g_env.no_f8_e5m2);
    return !g_env.no_f8 && !(flags & F_V5) && fmt && xm_table_form(tab, Mw, nullptr) &&
           (flags & F_S2N) && (flags & F_QBMA) && !(flags & F_GCLIP) && !(flags & F_TB);
}

// v5 (E5M2, adder wrap on): the matrix-core form of gemm_v5mx.h; FP8A_NO_V5MX=1 keeps
// gemm_fast_kernel<TM_V5> (A/B runs)
static bool v5mx_form(int Mw, uint32_t flags, int table_mode) {
    return table_mode == TM_V5 && Mw == 2 && (flags & F_OFUF) && !g_env.no_v5mx;
}

// The tile-table kernel (gemm_tt_kernel) applies: E3M4 / E2M5 (mantissa 4 or 5), any table mode
// of the int-bias path, s2n + qbma, no golden clip, not v5 (FP8A_NO_TT=1 keeps gemm_fast_kernel);
// not E2M5 with a signed table: its F7 form (two 32-row tables, one K-step per staged tile) was
// measured slower than gemm_fast_kernel.
static bool tt_form(int Mw, uint32_t flags, const TablePack &tab) {
    if (g_env.no_tt || (flags & F_V5) || !(Mw == 4 || Mw == 5) || !(flags & F_S2N) || !(flags & F_QBMA) ||
        (flags & F_GCLIP) || (flags & F_TB))
        return false;
    bool neg = false;
    for (int i = 0; i < (1 << (2 * Mw)); ++i) neg |= tab.raw[i] < 0;
    return Mw == 4 || !neg;
}

// E3M4 on the tile-table path runs the packed-f16 form (gemm_tt16_kernel) for signed tables (F7:
// +23 % on the ResNet-18 layer set) and for K >= 256 (+2-9 %); on short K its per-tile prologue
// (the frame shift's bias range, two barriers) outweighs the gain (MobileNetV2 E3M4 -3 %), and
// gemm_tt_kernel<4, F7> runs.  FP8A_NO_TT16=1 keeps gemm_tt_kernel everywhere.
// (option "tt16_mink": the smallest K of an unsigned-table launch on the f16 form; default 64 since
// round 5: ResNet-50 E3M4 2,045 -> 2,082 images/s with its K = 64 / 128 / 147 launches on the f16
// form, profiles/r05_tt16_mink/ -- round 3's tt16 lost 3 % there)
static bool tt16_form(int Mw, bool f7, int64_t K) {
    return !g_env.no_tt16 && Mw == 4 && (f7 || K >= opt(OPT_TT16_MINK));
}

// Which matrix-core form (if any) a GEMM of this format, table and shape can take, and whether its
// pre-decoded operands lie within the kernels' 32-bit byte offsets: the part of the decision that
// run_gemm and the callers that fuse an input quantizer ahead of it share.  on: not FP8A_NO_MX.
struct MxPlan {
    bool f8, tt, v5mx, on, fits32;
    int64_t kpad, npad;
    bool any() const { return (f8 || tt || v5mx) && on; }
};
// gemm_f8mx_kernel decomposes blockIdx.x, its tile index and its rows with 32-bit fastdiv (dividends below
// 2^31).  Rows: M <= a_words < 2^30 (a conv's word image has at least one word per output pixel, a matrix
// kpad per row; the fp32-staged sources are bounded the same way, xm_af32).  Blocks: tiles x splits, bounded
// here with the smallest tile of either dimension (128 rows, 16 columns) and the splits run_gemm can choose.
static MxPlan mx_plan(int E, int Mw, uint32_t flags, const TablePack &tab, int mode, int64_t M, int64_t N, int64_t K,
                      int64_t a_words) {
    MxPlan p;
    p.f8 = f8_form(E, Mw, flags, tab);
    p.tt = !p.f8 && tt_form(Mw, flags, tab);
    p.v5mx = !p.f8 && v5mx_form(Mw, flags, mode);
    p.on = !g_env.no_mx;
    p.kpad = (K + BK - 1) / BK * BK;
    p.npad = (N + BN - 1) / BN * BN;
    p.fits32 = a_words < (1ll << 30) && p.kpad * p.npad * 4 < (1ll << 32);
    if (p.f8 && p.fits32 && M > 0 && N > 0 && K > 0)
        p.fits32 = M <= a_words && ((M + 127) / 128) * ((N + 15) / 16) * choose_splits(M, N, K) < (1ll << 31);
    return p;
}

// The conv word image: every plane is the input plane inside a zero border at least as wide as
// the convolution's padding -- ph rows above and below; pw columns on the left, widened to 4 when
// W % 4 == 0 so that the interior rows start 16-B aligned, and the row length rounded up to a
// multiple of 4 (the pre-decode then moves the interior with 16-B loads and stores).
struct WordImage {
    int64_t H, W;    // image height / width (words)
    int ph, pw;      // top / left border
};
static WordImage word_image(int64_t H, int64_t W, int ph, int pw) {
    WordImage w;
    w.ph = ph;
    w.H = H + 2 * ph;
    if (pw > 0 && pw <= 4 && W % 4 == 0) {
        w.pw = 4;
        w.W = (W + 4 + pw + 3) / 4 * 4;
    } else {
        w.pw = pw;
        w.W = W + 2 * pw;
    }
    return w;
}

// Words of the pre-decoded A operand: conv, the group's word image [Bn][aw_c][awH][awW]; matrix,
// [M][Kpad].
static int64_t xm_a_words(const GemmArgs &a) {
    const int64_t kpad = (a.K + BK - 1) / BK * BK;
    if (!a.conv) return a.M * kpad;
    const WordImage w = word_image(a.H, a.W, a.ph, a.pw);
    return (a.M / (a.Ho * a.Wo)) * a.aw_c * w.H * w.W;
}

// gemm_f8mx_kernel reads A as fp32 and decodes it while staging (no xm_decode_a pass) for a 1x1
// unpadded conv or a matrix A whose source lies within 32-bit byte offsets, when the launch has at
// most FP8A_AF32_MAXCT column tiles (default 1; 0 = never): each column tile decodes its A
// elements again (~25 VALU operations each), against the pre-pass's 8 B of HBM traffic per element.
// Round 2 measured at most 0 / 2 / 4 tiles 4610 / 4613 / 4543 images/s on ResNet-50 E4M3 and chose
// 3; with round 5's pre-pass (4 loads in flight per thread) at most 1 tile wins everywhere:
// MobileNetV2 E4M3 23,877 -> 24,482, E5M2 v9 21,225 -> 21,561, ResNet-50 E4M3 4,790 -> 4,840
// (profiles/r05_af32/).
// (a strided 1x1 conv's pre-pass decodes sh x sw input pixels per one the product reads, so the
// fp32 staging is allowed up to sh x sw times as many column tiles: ResNet-18's downsampling convs)
static int64_t af32_maxct(int sh, int sw) { return (int64_t)opt(OPT_AF32_MAXCT) * sh * sw; }
static bool xm_af32(const GemmArgs &a) {
    const int64_t bnt = 16 * a.xncg, ct = (a.N + bnt - 1) / bnt;
    if (ct > (a.conv ? af32_maxct(a.sh, a.sw) : opt(OPT_AF32_MAXCT))) return false;  // option "af32_maxct"
    if (a.conv) {
        if (a.kh != 1 || a.kw != 1 || a.ph != 0 || a.pw != 0) return false;
        const int64_t bn = a.M / (a.Ho * a.Wo);
        return bn * a.Cin * a.H * a.W * 4 < (1ll << 32);
    }
    return a.A != nullptr && a.M * a.lda * 4 < (1ll << 32) && a.lda >= a.K;
}

// The fallback-flag arena of a (device, stream): two slots, used by the launches on the stream in
// turn, each holding one launch's flag word, the pre-passes' extremes and its per-unit marks.  A
// launch finds its slot zero; its last kernel (the gated exact / literal kernel) zeroes the other
// slot's words, which the previous launch used (arena_clear) -- so launches need no fill, and the
// clearing races nothing.  Zeroed once when (re)allocated; grows by reallocation after the stream
// drains.  A launch that stops before its last kernel (a launch error) leaves its successor a slot
// with stale words: that launch then reruns the marked units exactly -- the same bits, more time.
//
// Stream capture (a HIP graph being recorded on s): the arena's host-side rotation would be frozen
// into the graph -- a forward with an odd number of launches would start every replay after the
// first on a slot its own last launch left dirty, and the clear sizes would be those of capture
// time.  So a captured launch never touches the arena: its words live in the head of the caller's
// workspace (which the caller allocates per call; torch's allocator gives a graph its own pool),
// zeroed by a fill kernel at the start of the launch (dev_fill: not a memset node), and it clears nothing.  Every replay then
// starts from zero words whatever ran before it, eager launches keep their own rotation, and an
// eager launch that grows the arena afterwards cannot touch memory a graph references.  Growth never
// frees an arena (retired ones stay allocated: at most the size of the current one in total), so
// it needs no stream synchronisation either.
struct FlagArena {
    uint32_t *p = nullptr;
    size_t slot = 0;       // bytes per slot
    int cur = 0;           // the slot the next launch uses
    size_t dirty[2] = {0, 0};
};
struct ArenaLease {
    uint32_t *mine = nullptr;  // this launch's slot (zero)
    uint4 *clr = nullptr;      // the other slot, and its 16-byte words the last kernel zeroes
    uint32_t clr16 = 0;
};
// Is a graph being captured on s?  (-1: the query itself failed; the error is recorded)
// In-stream fills as kernels of our own, not hipMemsetAsync / hipMemset2DAsync: under stream capture
// a memset becomes a graph memset node, and on this ROCm such nodes did not refill their destination
// on replays after the first (measured: tools/dbg_capture2.py, DESIGN.md §3r -- a captured launch's
// flag words then held stale data).  A kernel node re-executes every replay like any other.
__global__ __launch_bounds__(256) void fill_u8_kernel(uint8_t *p, size_t n, uint32_t v8) {
    const uint32_t w = v8 * 0x01010101u;
    const size_t lead = std::min(n, (size_t)((16 - ((uintptr_t)p & 15)) & 15)), n16 = (n - lead) / 16;
    const size_t t0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nt = (size_t)gridDim.x * blockDim.x;
    uint4 *q = reinterpret_cast<uint4 *>(p + lead);
    for (size_t i = t0; i < n16; i += nt) q[i] = make_uint4(w, w, w, w);
    for (size_t i = t0; i < lead; i += nt) p[i] = (uint8_t)v8;  // (bytes before the first 16-B boundary)
    for (size_t i = lead + 16 * n16 + t0; i < n; i += nt) p[i] = (uint8_t)v8;  // (and after the last)
}
__global__ __launch_bounds__(256) void fill_rows_kernel(float *p, int64_t ld, int64_t w, int64_t h) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < w * h; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = i / w;
        p[r * ld + (i - r * w)] = 0.0f;
    }
}
static hipError_t dev_fill(void *p, int v, size_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    fill_u8_kernel<<<(unsigned)std::max<size_t>(1, std::min<size_t>((n / 16 + 255) / 256, 1024)), 256, 0, s>>>(
        (uint8_t *)p, n, (uint32_t)(v & 0xFF));
    return hipGetLastError();
}
static hipError_t dev_zero_rows(float *p, int64_t ld, int64_t w, int64_t h, hipStream_t s) {
    if (w <= 0 || h <= 0) return hipSuccess;
    fill_rows_kernel<<<(unsigned)std::min<int64_t>((w * h + 255) / 256, 8192), 256, 0, s>>>(p, ld, w, h);
    return hipGetLastError();
}
static int stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &st) != hipSuccess) return -1;
    static const bool dbg = getenv("FP8A_DEBUG_CAPTURE") != nullptr;  // diagnostics: the query per lease
    if (dbg) fprintf(stderr, "fp8a lease stream=%p capturing=%d\n", (void *)s, (int)st);
    return st == hipStreamCaptureStatusActive ? 1 : 0;
}
// stream_capturing returned -1: HIP's recorded error, or an error of our own when it recorded none --
// never FP8A_OK, the caller has launched nothing.  who: "fp8a", "fp8a self-check:".
static int capture_query_error(const std::string &who) {
    const int rc = hip_check((who + " stream capture query").c_str());
    return rc ? rc : fail(FP8A_EHIP, who + " the stream capture query failed");
}
// The lease of a captured launch: `need` bytes at the head of its workspace, zeroed in-stream.
static bool capture_lease(hipStream_t s, void *ws, size_t ws_bytes, size_t need, ArenaLease &l) {
    if (ws == nullptr || ws_bytes < need) return false;
    static const bool dbg = getenv("FP8A_DEBUG_CAPTURE") != nullptr;
    if (dbg) fprintf(stderr, "fp8a capture lease ws=%p need=%zu ws_bytes=%zu\n", ws, need, ws_bytes);
    if (dev_fill(ws, 0, need, s) != hipSuccess) return false;
    l.mine = (uint32_t *)ws;
    l.clr = nullptr;
    l.clr16 = 0;
    return true;
}
static std::mutex g_arena_mu;
static std::map<std::pair<int, uintptr_t>, FlagArena> g_arenas;
static bool flag_arena(hipStream_t s, size_t need, ArenaLease &l) {
    static std::vector<void *> retired;  // grown-out-of arenas: never freed (in-flight launches may use them)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return false;
    need = (need + 255) & ~(size_t)255;
    std::lock_guard<std::mutex> lock(g_arena_mu);
    FlagArena &ar = g_arenas[{dev, (uintptr_t)s}];
    if (ar.slot < need) {
        const size_t slot = std::max(need, std::max(2 * ar.slot, (size_t)65536));
        void *p = nullptr;
        if (hipMalloc(&p, 2 * slot) != hipSuccess) return false;
        if (dev_fill(p, 0, 2 * slot, s) != hipSuccess) {
            (void)hipFree(p);
            return false;
        }
        if (ar.p) retired.push_back(ar.p);
        ar = FlagArena{};
        ar.p = (uint32_t *)p;
        ar.slot = slot;
    }
    const int other = 1 - ar.cur;
    l.mine = ar.p + (size_t)ar.cur * (ar.slot / 4);
    l.clr = reinterpret_cast<uint4 *>(ar.p + (size_t)other * (ar.slot / 4));
    l.clr16 = (uint32_t)(ar.dirty[other] / 16);
    ar.dirty[other] = 0;
    ar.dirty[ar.cur] = need;
    ar.cur = other;
    return true;
}
// A depthwise launch's gate word: the workspace head under capture, else an arena slot.
static bool dw_lease(hipStream_t s, void *ws, size_t ws_bytes, ArenaLease &l) {
    const int cap = stream_capturing(s);
    if (cap < 0) return false;
    return cap ? capture_lease(s, ws, ws_bytes, FLAG_BYTES, l) : flag_arena(s, FLAG_BYTES, l);
}
static int lease_error() {
    const int rc = hip_check("fp8a flag arena");
    return rc ? rc : fail(FP8A_EHIP, "fp8a flag arena: no room for the flag words (under stream capture they need "
                                     "the workspace head)");
}
// grid blocks of 256 threads that clear a lease's other slot in about four 16-byte stores each
static unsigned clear_blocks(const ArenaLease &l) { return (l.clr16 + 1023) / 1024; }

// Fast tiled kernel + gated exact kernel (int-bias path), or the exact kernel alone (tb path).
static int run_qamaa(GemmArgs &a, hipStream_t s);

static int run_gemm(GemmArgs &a, const int32_t *table, void *ws, size_t ws_bytes, hipStream_t s) {
    if (a.qmax) return run_qamaa(a, s);
    int rc = check_format(a.E, a.Mw);
    if (rc) return rc;
    if (a.M < 0 || a.N < 0 || a.K < 0) return fail(FP8A_EINVAL, "negative extent");
    if (a.post_bout && (a.M == 0 || a.N == 0 || a.K == 0)) {  // (no exact kernel below to write it)
        fq_bias_kernel<<<1, 1, 0, s>>>(a.post_fq, a.post_bout, a.post_ibout);
        const int rc0 = hip_check("fp8a output-quantizer bias");
        if (rc0) return rc0;
    }
    if (a.M == 0 || a.N == 0) return FP8A_OK;
    if (a.K == 0) {  // empty inner dimension: the reference's sum over an empty axis is 0
        if (a.nchw) return fail(FP8A_EINVAL, "empty convolution window");
        if (dev_zero_rows(a.C, a.ldc, a.N, a.M, s) != hipSuccess)
            return hip_check("fp8a zero fill");
        return FP8A_OK;
    }
    if ((!a.A && !a.conv) || (a.conv && !a.X) || !a.B || !a.C || !a.bA || !a.bB || !a.bR)
        return fail(FP8A_EINVAL, "null pointer");
    int mode;
    const bool v5 = a.flags & F_V5;
    if (v5 && (a.flags & F_TB)) return fail(FP8A_EINVAL, "the v5 model has no tensor-bias semantics");
    rc = pack_table(table, a.Mw, v5 || (a.flags & F_APPROX), a.tab, mode);
    if (rc) return rc;
    if (v5) mode = TM_V5;
    const int mode0 = mode;
    // E4M3 / E5M2 with a non-negative (or no) table (xm_table_form), s2n and per-product quantization:
    // the LUT + hardware fp8 / bf8 form (FP8A_NO_F8=1 keeps the arithmetic form, for comparison)
    const int64_t a_words = xm_a_words(a);
    const MxPlan mx = mx_plan(a.E, a.Mw, a.flags, a.tab, mode, a.M, a.N, a.K, a_words);
    if (mx.f8) mode = TM_F8;
    const int64_t total = a.M * a.N;
    const unsigned eblocks = (unsigned)std::min<int64_t>((total + 255) / 256, 4096);
    if (a.flags & F_TB) {
        a.flag = nullptr;
        ++g_paths[PATH_EXACT];
        gemm_exact_kernel<<<eblocks, 256, 0, s>>>(a);
        return hip_check("fp8a exact gemm launch");
    }
    if (ws == nullptr || ws_bytes < FLAG_BYTES) return fail(FP8A_EINVAL, "matmul workspace too small");
    // the flag word and the per-unit fallback marks live in the library's flag arena (zero on
    // entry, left zero by gemm_exact_kernel: no fill per launch); the workspace's first word
    // receives the final flag word, and its head stays reserved (the layout of the size queries)
    static const bool no_units = getenv("FP8A_NO_UNITS") != nullptr;  // diagnostics: whole-launch fallbacks
    const size_t head = ws_bytes >= head_bytes(a.M, a.N) ? head_bytes(a.M, a.N) : FLAG_BYTES;
    ArenaLease lease;
    const int cap = stream_capturing(s);  // (captured: the words live in the workspace head, flag_arena)
    if (cap < 0) return capture_query_error("fp8a");
    if (cap ? !capture_lease(s, ws, ws_bytes, head, lease) : !flag_arena(s, head_bytes(a.M, a.N), lease))
        return lease_error();
    a.flag = lease.mine;
    a.flag_out = (uint32_t *)ws;
    a.arena_clr = lease.clr;
    a.arena_clr16 = lease.clr16;
    a.nur = (a.M + 63) / 64;
    a.nuc = (a.N + 63) / 64;
    a.urow = no_units || (cap && head < head_bytes(a.M, a.N)) ? nullptr : (uint8_t *)a.flag + FLAG_BYTES;
    a.ucol = no_units ? nullptr : a.urow + a.nur;
    a.utile = no_units ? nullptr : a.ucol + a.nuc;
    // split-K when the caller's workspace holds the partials (else one split)
    a.splits = choose_splits(a.M, a.N, a.K);
    if (a.splits > 1 && ws_bytes < head + splitk_bytes(a.M, a.N, a.K)) a.splits = 1;
    const int64_t kt = (a.K + BK - 1) / BK;
    a.kchunk = ((kt + a.splits - 1) / a.splits) * BK;
    a.part = a.splits > 1 ? (float *)((char *)ws + head) : nullptr;
    // the matrix-core E4M3 kernel and the tile-table kernel (E3M4 / E2M5) need their pre-decoded
    // operands in the workspace (else gemm_fast_kernel runs); FP8A_NO_MX=1 forces the latter
    a.aw = nullptr;
    const bool tt = mx.tt, v5mx = mx.v5mx;
    if (mx.any()) {
        const int64_t kpad = mx.kpad, npad = mx.npad;
        const size_t off = head + (a.splits > 1 ? splitk_bytes(a.M, a.N, a.K) : 0);
        const WordImage wi = word_image(a.H, a.W, a.ph, a.pw);
        a.awH = wi.H; a.awW = wi.W; a.awph = wi.ph; a.awpw = wi.pw;
        // (the exact test: the operands behind this launch's own split-K partials; the callers that fuse
        // an input quantizer test gemm_workspace_bytes, which is never smaller)
        const XmOperandLayout lay = xm_operand_layout(a.N, a.K, a_words);
        if (mx.fits32 && ws_bytes >= off + lay.total) {
            char *base = (char *)ws + off;
            a.aw = (const uint32_t *)base;
            a.awld = kpad;
            a.bqw = (const uint2 *)(base + lay.bqw);
            a.lutw = (const uint32_t *)(base + lay.lutw);
            a.ebr = (const uint16_t *)(base + lay.ebr);
            a.xm_vmin = 0;  // the table's lowest V' binade (the E5M2 halved-block form's `tok` threshold)
            if (mode == TM_F8) (void)xm_table_form(a.tab, a.Mw, &a.xm_vmin);
            a.npad = npad;
            a.ttf7 = 0;
            for (int i = 0; tt && i < (1 << (2 * a.Mw)); ++i) a.ttf7 |= a.tab.raw[i] < 0;
            a.wfmt = v5mx ? 4 : tt ? (tt16_form(a.Mw, a.ttf7, a.K) ? 2 : 1) : 0;
            if (a.wfmt == 1 && !opt(OPT_TT_BAND)) a.ebr = nullptr;  // (gemm_tt_kernel: no band test)
            a.xncg = tt ? 4 : xm_ncg(a.N);
            a.xm_signs = opt(OPT_XM_SIGN_ROWS);
            a.xm_pipe = opt(OPT_XM_PIPE);
            a.xm_wave_rows = opt(OPT_XM_WAVE_ROWS);
            // the in-launch split-K sum: the E4M3 matrix-core kernel (the E5M2 form's halved-block rerun
            // writes a tile's partials a second time, after its counter has run out: it keeps the reduce pass)
            a.skcnt = nullptr;
            if (a.splits > 1 && opt(OPT_SPLITK_FIXUP) && a.wfmt == 0 && a.Mw == 3) {
                a.skcnt = (uint32_t *)((char *)ws + head + splitk_part_bytes(a.splits, a.M, a.N));
                a.sk_words = splitk_counter_words(a.M, a.N);
            }
            // the input's word image from the previous launch (fp8a_conv2d_chain): its words replace
            // the A pre-pass, which then runs gated (only to write the fused quantizer's bias, or to
            // re-decode x if the image arrived invalid)
            const bool use_img = a.in_img != nullptr && !tt && a.conv && a.fqin.mx != nullptr;
            if (use_img) a.aw = a.in_img + 64;
            a.af32 = !tt && !v5mx && !use_img && xm_af32(a) ? 1 : 0;
            const int64_t rows = a.conv ? a.M / (a.Ho * a.Wo) : a.M, cols = a_words / std::max<int64_t>(rows, 1);
            dim3 ga((unsigned)std::min<int64_t>((cols + 255) / 256, 64), (unsigned)std::min<int64_t>(rows, 1024));
            {  // the pre-pass's flattened 16-byte form (xm_decode_a: unbordered, rows and columns in
               // whole 16-byte chunks): a 1-D grid of about 4 chunks per thread
                const int64_t hw = a.H * a.W, lim0 = a.conv ? cols : a.K, istride = a.conv ? a.Cin * hw : a.lda;
                const float *in0 = a.conv ? a.X + a.cbase * hw : a.A;
                const bool flat = !(a.conv && (a.awph | a.awpw)) && lim0 % 4 == 0 && cols % 4 == 0 && istride % 4 == 0 &&
                                  ((uintptr_t)in0 & 15) == 0 && ((uintptr_t)a.aw & 15) == 0;
                if (flat) ga = dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>((a_words / 4 + 1023) / 1024, 8192)), 1);
            }
            if (use_img) {
                a.gate = a.in_img;
                xm_decode_a<<<ga.y == 1 ? dim3(std::min(ga.x, 512u)) : dim3(std::min(ga.x, 8u), std::min(ga.y, 64u)), 256, 0,
                              s>>>(a);
                a.gate = nullptr;
            } else if (!a.af32) {
                xm_decode_a<<<ga, 256, 0, s>>>(a);
            }
            if (v5mx) {  // the four table words per (k, n), [Kpad][Npad]
                const unsigned gb = (unsigned)std::min<int64_t>((kpad * npad + 255) / 256, 4096);
                v5mx_decode_b<<<gb, 256, 0, s>>>(a, kpad);
            } else if (tt) {  // B words [Kpad][Npad] (the same bytes as the E4M3 pair grid) + the static image
                const unsigned gb = (unsigned)std::min<int64_t>((kpad * npad + 255) / 256, 4096);
                tt_decode_b<<<gb, 256, 0, s>>>(a, kpad);  // (+ gemm_tt16_kernel's f16 image when wfmt == 2)
            } else {
                const unsigned gb = (unsigned)std::min<int64_t>((kpad * npad / 2 + 255) / 256, 4096);
                xm_decode_b<<<gb, 256, 0, s>>>(a, kpad);
            }
            rc = hip_check("fp8a operand pre-decode launch");
            if (rc) return rc;
        }
    }
    if (a.fqin.mx && !a.aw)  // the caller (conv2d_impl) only fuses where the pre-decode runs
        return fail(FP8A_EINVAL, "internal: fused input quantization without the matrix-core path");
    if (mode == TM_F8 && a.Mw != 3 && !a.aw) mode = mode0;  // (gemm_fast_kernel's TM_F8 form is E4M3 only)
    ++g_paths[gemm_path(a)];
    // word-image emission (fp8a_conv2d_chain): the E4M3 / E5M2 matrix-core kernel and the VALU
    // kernel emit the next convolution's words from their store; the tile-table and v5 matrix-core
    // kernels do not (store_tile<false>: the emission code cost gemm_tt16_kernel 32 SGPR spills and a
    // 38 % slower E3M4 layer set, round 4 -> 5), so their unsplit launch marks the image invalid
    // instead (emit_prep_kernel set the header valid before this launch) and the consumer's gated
    // pre-pass re-decodes its input from y (likewise under a GELU tail, which the emitting store
    // compiles out)
    if (a.em.w != nullptr && (a.em.form == 2 || (a.aw && a.wfmt != 0 && a.splits == 1) || a.post_act == 2)) {
        if (dev_fill(a.em.invalid, 1, sizeof(uint32_t), s) != hipSuccess) return hip_check("fp8a word image header");
        a.em.w = nullptr;
    }
    KernelEv kev{};
    if (g_ktime && !cap) {  // (no host-side events inside a captured graph)
        kev.a = pool_event();
        kev.b = pool_event();
        kev.path = gemm_path(a);
        // (E5M2: the plain and the halved-block form; E3M4 f16 form: + its gated f32 rerun)
        kev.dispatches = (a.aw && ((a.wfmt == 0 && a.Mw == 2) || a.wfmt == 2)) ? 2 : 1;
        kev.macs = (double)a.M * (double)a.N * (double)a.K;
        if (kev.a && kev.b) (void)hipEventRecord(kev.a, s);
    }
    launch_fast(mode, a, s);
    if (g_ktime && !cap && kev.a && kev.b) {
        (void)hipEventRecord(kev.b, s);
        g_kev.push_back(kev);
    }
    rc = hip_check("fp8a fast gemm launch");
    if (rc) return rc;
    if (a.splits > 1 && a.aw != nullptr && a.skcnt != nullptr) {
        ++g_splitk_launches;  // (summed inside the launch)
    } else if (a.splits > 1) {
        const int64_t q = a.M * a.N;
        const unsigned rb = (unsigned)std::min<int64_t>((q / 4 + 255) / 256 + 1, 8192);
        splitk_reduce_kernel<<<rb, 256, 0, s>>>(a);
        ++g_splitk_launches;
        rc = hip_check("fp8a split-K reduce launch");
        if (rc) return rc;
    }
    // (at most 512 blocks: the kernel is a no-op but for the arena clearing unless the launch
    // flagged, and its 268 VGPRs hold it at one wave per SIMD -- 4096 blocks cost ~7.5 us of wave
    // launches per GEMM; a flagged launch loops its units over the blocks)
    const unsigned ublocks = std::max((unsigned)std::min<int64_t>(a.nur * a.nuc, 512), clear_blocks(lease));
    gemm_exact_kernel<<<ublocks, 256, 0, s>>>(a);
    rc = hip_check("fp8a gated exact gemm launch");
    static const bool dbg = getenv("FP8A_DEBUG_FLAGS") != nullptr;  // diagnostics: the flag word per launch
    if (!rc && dbg) {
        uint32_t f = 0;
        if (hipStreamSynchronize(s) == hipSuccess && hipMemcpy(&f, a.flag_out, sizeof(f), hipMemcpyDeviceToHost) == hipSuccess)
            fprintf(stderr, "fp8a flag M=%lld N=%lld K=%lld E=%d M=%d wfmt=%d flag=%u\n", (long long)a.M, (long long)a.N,
                    (long long)a.K, a.E, a.Mw, a.aw ? a.wfmt : -1, f);
    }
    return rc;
}

// qamaa: term = fq(a*b) (no operand decode: exact for any fp32 inputs), then fq(sum) in place.
static int run_qamaa(GemmArgs &a, hipStream_t s) {
    if (a.M < 0 || a.N < 0 || a.K < 0) return fail(FP8A_EINVAL, "negative extent");
    if (a.M == 0 || a.N == 0) return FP8A_OK;
    if (a.qM < 1 || a.qE < 1) return fail(FP8A_EFORMAT, "bad qamaa quantizer format");
    if (!a.nchw && a.ldc != a.N) return fail(FP8A_EINVAL, "qamaa output must be dense");
    if (a.K == 0) {
        if (dev_fill(a.C, 0, (size_t)a.M * a.N * sizeof(float), s) != hipSuccess) return hip_check("fill");
    } else {
        a.splits = 1;
        a.kchunk = a.K;
        launch_fast(TM_QAMAA, a, s);
        int rc = hip_check("fp8a qamaa gemm launch");
        if (rc) return rc;
    }
    return FP8A_OK;
}

// ------------------------------------------------------------------ the exact product (gemm_dense.h)
static inline int64_t round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
static inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

static size_t dense_ws_bytes(int64_t M, int64_t N, int64_t K) {
    const int64_t mpad = round_up(std::max<int64_t>(M, 1), DN_T), npad = round_up(std::max<int64_t>(N, 1), DN_T);
    const int64_t kpad = round_up(std::max<int64_t>(K, 1), 32);
    // byte images at 2 B per element (the bf16 form; the fp8 forms use the first half)
    return al256(4 * (size_t)(mpad / DN_U + npad / DN_U) + 4) + al256((size_t)(2 * mpad * kpad)) +
           al256((size_t)(mpad * kpad / 32)) + al256((size_t)(2 * npad * kpad)) + al256((size_t)(npad * kpad / 32));
}

// A fresh, well-mixed nonzero mark tag per dense call (the dense path's marks are never cleared)
static uint32_t next_dense_gen() {
    static std::atomic<uint32_t> ctr{0};
    uint32_t g;
    do {
        g = (ctr.fetch_add(1) + 1) * 0x9E3779B1u;
        g ^= g >> 15;
    } while (g == 0u);
    return g;
}

static int run_dense(DenseArgs a, void *ws, size_t wsb, hipStream_t s) {
    if (a.M < 0 || a.N < 0 || a.K < 0) return fail(FP8A_EINVAL, "negative extent");
    if (a.fmt != FP8A_DENSE_E4M3 && a.fmt != FP8A_DENSE_E5M2 && a.fmt != FP8A_DENSE_BF16)
        return fail(FP8A_EINVAL, "unknown dense operand format");
    const bool qout = a.fz.qin.mx || a.fz.rq.mx || a.fz.oq.mx || a.fz.wq.mx;
    if (qout && (a.M == 0 || a.K == 0)) {  // no pack pass to leave the quantizers' biases
        dn_bias_kernel<<<(unsigned)std::max<int64_t>(1, (a.N + 255) / 256), 256, 0, s>>>(a.fz, a.N);
        const int rc = hip_check("fp8a dense quantizer biases");
        if (rc) return rc;
    }
    if (a.M == 0 || a.N == 0) return FP8A_OK;
    ++g_paths[PATH_DENSE];
    if (a.K == 0) {
        const hipError_t e = a.conv ? dev_fill(a.y, 0, (size_t)(a.M * a.N) * sizeof(float), s)
                                    : dev_zero_rows(a.y, a.ldc, a.N, a.M, s);
        return e == hipSuccess ? FP8A_OK : hip_check("fp8a dense fill");
    }
    // a small convolution (the stem: K = 27, N = 32) as direct fp32 FMAs (dn_direct_kernel; option
    // "dn_direct", default 1): a 128 x 128 MFMA tile would carry 32 live columns and 27 of 64 k
    if (opt(OPT_DN_DIRECT) && a.conv && a.K <= DD_K && a.N <= DD_N) {
        KernelEv kev{};
        if (g_ktime) {
            kev.a = pool_event();
            kev.b = pool_event();
            kev.path = PATH_DENSE;
            kev.dispatches = 1;
            kev.macs = 4.0 * ((double)a.M * a.K + (double)a.M * a.N) + 4.0 * (double)a.N * a.K;
            if (kev.a && kev.b) (void)hipEventRecord(kev.a, s);
        }
        const unsigned g = (unsigned)std::min<int64_t>((a.M + 255) / 256, 1 << 20);
        dn_direct_kernel<<<g, 256, 0, s>>>(a);
        if (g_ktime && kev.a && kev.b) {
            (void)hipEventRecord(kev.b, s);
            g_kev.push_back(kev);
        }
        return hip_check("fp8a dense direct launch");
    }
    a.mpad = round_up(a.M, DN_T);
    a.npad = round_up(a.N, DN_T);
    a.kpad = round_up(a.K, 32);
    if (a.kpad / 32 > 65535) return fail(FP8A_EINVAL, "K too large for the dense path (> 2097120)");
    if (ws == nullptr || wsb < dense_ws_bytes(a.M, a.N, a.K)) return fail(FP8A_EINVAL, "workspace too small");
    uint8_t *w = static_cast<uint8_t *>(ws);
    // the unit marks hold this call's tag, so no call clears them: a stale word matches the tag
    // only by chance (2^-32 per word), and then its unit is merely recomputed in fp32 by dn_fix
    const size_t nmark = 4 * (size_t)(a.mpad / DN_U + a.npad / DN_U) + 4;
    a.anymark = reinterpret_cast<uint32_t *>(w);
    a.urow = a.anymark + 1;
    a.ucol = a.urow + a.mpad / DN_U;
    a.gen = next_dense_gen();
    w += al256(nmark);
    a.qa = w;  w += al256((size_t)(2 * a.mpad * a.kpad));
    a.qas = w; w += al256((size_t)(a.mpad * a.kpad / 32));
    a.qb = w;  w += al256((size_t)(2 * a.npad * a.kpad));
    a.qbs = w;
    const dim3 ga((unsigned)((a.mpad + 255) / 256), (unsigned)(a.kpad / 32));
    const dim3 gb((unsigned)((a.npad + 255) / 256), (unsigned)(a.kpad / 32));
    const unsigned tiles = (unsigned)((a.mpad / DN_T) * (a.npad / DN_T));
    const unsigned units = (unsigned)((a.mpad / DN_U) * (a.npad / DN_U));
    // (kernel timing: the GEMM launch alone, its algorithmic bytes -- fp32 A read once, fp32 C
    // written once, the packed B image read once -- in the MAC slot)
    KernelEv kev{};
    auto kev_begin = [&]() {
        if (!g_ktime) return;
        kev.a = pool_event();
        kev.b = pool_event();
        kev.path = PATH_DENSE;
        kev.dispatches = 1;
        kev.macs = 4.0 * ((double)a.M * a.K + (double)a.M * a.N) +
                   (a.fmt == FP8A_DENSE_BF16 ? 2.0 : 1.0) * (double)a.npad * a.kpad;
        if (kev.a && kev.b) (void)hipEventRecord(kev.a, s);
    };
    auto kev_end = [&]() {
        if (g_ktime && kev.a && kev.b) {
            (void)hipEventRecord(kev.b, s);
            g_kev.push_back(kev);
        }
    };
    if (a.fmt == FP8A_DENSE_BF16) {  // (A straight from its fp32 source)
        dn_pack<true, 2><<<gb, 256, 0, s>>>(a);
        kev_begin();
        static const bool no_af = getenv("FP8A_NO_PW1") != nullptr;  // (A/B runs: the 64-bit indexing)
        const bool x32 = !no_af && a.conv && 4 * a.C * a.H * a.W * (a.M / (a.Ho * a.Wo)) < (1ll << 31);
        const bool pw1 = x32 && a.kh == 1 && a.kw == 1 && a.sh == 1 && a.sw == 1 && a.ph == 0 && a.pw == 0;
        if (pw1) dn_gemm_bf16<true, 1><<<tiles, 256, 0, s>>>(a);
        else if (x32) dn_gemm_bf16<true, 2><<<tiles, 256, 0, s>>>(a);
        else if (a.conv) dn_gemm_bf16<true><<<tiles, 256, 0, s>>>(a);
        else dn_gemm_bf16<false><<<tiles, 256, 0, s>>>(a);
    } else if (a.fmt == FP8A_DENSE_E4M3) {
        dn_pack<false, 0><<<ga, 256, 0, s>>>(a);
        dn_pack<true, 0><<<gb, 256, 0, s>>>(a);
        kev_begin();
        if (a.conv) dn_gemm<0, true><<<tiles, 256, 0, s>>>(a);
        else dn_gemm<0, false><<<tiles, 256, 0, s>>>(a);
    } else {
        dn_pack<false, 1><<<ga, 256, 0, s>>>(a);
        dn_pack<true, 1><<<gb, 256, 0, s>>>(a);
        kev_begin();
        if (a.conv) dn_gemm<1, true><<<tiles, 256, 0, s>>>(a);
        else dn_gemm<1, false><<<tiles, 256, 0, s>>>(a);
    }
    kev_end();
    dn_fix<<<std::min(units, 2048u), 256, 0, s>>>(a);
    return hip_check("fp8a dense launch");
}

static DenseArgs dense_args() {
    DenseArgs a;
    memset(&a, 0, sizeof(a));
    a.Ho = a.Wo = 1;
    a.kh = a.kw = a.sh = a.sw = a.dh = a.dw = 1;
    return a;
}

}  // namespace fp8a

using namespace fp8a;

template <typename I>
static void launch_group_conv(const GcArgs &a, hipStream_t s) {
    const unsigned g = (unsigned)std::min<int64_t>((a.total + 255) / 256, 65536);
    const bool d1 = a.dw == 1;
    if (d1 && a.kw == 3 && a.sw == 1) dn_group_conv<I, 3, 1><<<g, 256, 0, s>>>(a);
    else if (d1 && a.kw == 3 && a.sw == 2) dn_group_conv<I, 3, 2><<<g, 256, 0, s>>>(a);
    else if (d1 && a.kw == 5 && a.sw == 1) dn_group_conv<I, 5, 1><<<g, 256, 0, s>>>(a);
    else if (d1 && a.kw == 5 && a.sw == 2) dn_group_conv<I, 5, 2><<<g, 256, 0, s>>>(a);
    else dn_group_conv<I, 0, 1><<<g, 256, 0, s>>>(a);
}

// dn_dw3_kernel's block shape: about `target` outputs per workgroup (whole planes when a plane has
// fewer, else bands of rows of one plane), the staged window within dw_lds bytes of LDS (default
// 40 KB, four workgroups per CU: measured against 2 / 8 / 16 KB-windowed plans, §3l); false when even 256 outputs' window does not fit (very wide rows).
static bool plan_dw3(DwArgs &a, int S, size_t &lds, bool raw = false, int tap_bytes = 4) {
    const int64_t op = (int64_t)a.Ho * a.Wo;
    for (int target = std::max(256, opt(OPT_DW_TARGET)); target >= 256; target /= 2) {
        int PB, RB;
        if (op <= target) {
            RB = a.Ho;
            PB = (int)std::min<int64_t>(target / op, a.planes);
            if ((int64_t)a.H * a.W % 4 != 0 && PB >= 4) PB &= ~3;  // 16-byte aligned source ranges (dw_stage)
        } else {
            PB = 1;
            RB = std::max(1, target / a.Wo);
        }
        const int RS = (RB - 1) * S + 3,
                  WS = (std::max(a.W + DW_OX, DW_OX - a.pw + (a.Wo - 1) * S + 3) + 3) / 4 * 4;
        // raw (dn_dw3g_kernel): the unpadded source range from its 16-byte-aligned start
        const int64_t nsrc = RB == a.Ho ? (int64_t)PB * a.H * a.W : (int64_t)std::min(RS, a.H) * a.W;
        a.nimg = (int)(4 * ((nsrc + 6) / 4));
        const int64_t bytes = (raw ? (int64_t)a.nimg : (int64_t)PB * RS * WS) * 4 + (int64_t)PB * 9 * tap_bytes;
        if (bytes > std::min(65536, std::max(4096, opt(OPT_DW_LDS)))) continue;
        a.PB = PB; a.RB = RB; a.nb = (a.Ho + RB - 1) / RB; a.RS = RS; a.WS = WS;
        a.inv_c = 1.0f / a.C; a.inv_ws = 1.0f / WS; a.inv_pst = 1.0f / (RS * WS);
        a.inv_wo = 1.0f / a.Wo; a.inv_pout = 1.0f / (RB * a.Wo);
        a.inv_w = 1.0f / a.W; a.inv_hw = 1.0f / (a.H * a.W);
        a.inv_nqd = 1.0f / ((a.Wo + 3) / 4); a.inv_pq = 1.0f / (RB * ((a.Wo + 3) / 4));
        lds = (size_t)bytes;
        return ((a.planes + PB - 1) / PB) * a.nb < (1ll << 24);
    }
    return false;
}

// conv_tbs_kernel's block shape: dn_dw3_kernel's plan with quads of outputs and rows of staged
// words padded to a multiple of 4 (16-byte LDS reads).
static bool plan_tbs(TbsArgs &a, int S, int64_t planes, int64_t C, int64_t H, int64_t W, int64_t Ho, int64_t Wo,
                     int ph, int pw, size_t &lds) {
    if (H >= (1 << 20) || W >= (1 << 20) || C >= (1 << 20) || H * W >= (1ll << 22)) return false;  // (as plan_dw3's caller)
    a.planes = planes; a.C = (int)C; a.H = (int)H; a.W = (int)W; a.Ho = (int)Ho; a.Wo = (int)Wo; a.ph = ph; a.pw = pw;
    const int nq = (int)((Wo + TBX_TW - 1) / TBX_TW);
    const int WS = ((4 * nq - 1) * S + 3 + 3) / 4 * 4;
    const int64_t op = Ho * Wo;
    for (int target = std::max(256, opt(OPT_DW_TARGET)); target >= 256; target /= 2) {
        int PB, RB;
        if (op <= target) {
            RB = (int)Ho;
            PB = (int)std::min<int64_t>(target / op, planes);
            if (H * W % 4 != 0 && PB >= 4) PB &= ~3;  // 16-byte aligned source ranges (dw_stage)
        } else {
            PB = 1;
            RB = std::max(1, (int)(target / Wo));
        }
        const int RS = (RB - 1) * S + 3;
        const int64_t bytes = (int64_t)PB * RS * WS * 4 + 512 + (int64_t)PB * 9 * 8;
        if (bytes > std::min(65536, std::max(4096, opt(OPT_DW_LDS)))) continue;
        a.PB = PB; a.RB = RB; a.nb = (int)((Ho + RB - 1) / RB); a.RS = RS; a.WS = WS; a.nq = nq;
        a.inv_c = 1.0f / a.C; a.inv_ws = 1.0f / WS; a.inv_pst = 1.0f / (RS * WS);
        a.inv_nq = 1.0f / nq; a.inv_pq = 1.0f / (RB * nq);
        a.inv_w = 1.0f / a.W; a.inv_hw = 1.0f / (a.H * a.W);
        lds = (size_t)bytes;
        return ((planes + PB - 1) / PB) * a.nb < (1ll << 24);
    }
    return false;
}

// ------------------------------------------------------------------------- convolution calls
// A convolution's geometry: the caller's fields, and what conv_shape derives from them.
struct ConvShape {
    int64_t Bn, Cin, H, W, Cout;
    int kh, kw, sh, sw, ph, pw, dh, dw, groups;
    int64_t Ho, Wo, cog, cig, Mrows, Kg;  // output size, channels per group, the implicit GEMM's M and K
};
static bool groups_ok(int groups, int64_t Cin, int64_t Cout) {
    return groups > 0 && Cout % groups == 0 && Cin % groups == 0;
}
static bool bad_geometry(const ConvShape &c) {
    return c.kh < 1 || c.kw < 1 || c.sh < 1 || c.sw < 1 || c.dh < 1 || c.dw < 1 || c.ph < 0 || c.pw < 0;
}
// Checks the caller's fields (groups, then kernel / stride / dilation / padding, then the output size)
// and fills the derived ones.  Entry points without groups pass 1.
static int conv_shape(ConvShape &c) {
    if (!groups_ok(c.groups, c.Cin, c.Cout)) return fail(FP8A_EINVAL, "bad groups");
    if (bad_geometry(c)) return fail(FP8A_EINVAL, "bad convolution geometry");
    c.Ho = (c.H + 2 * c.ph - c.dh * (c.kh - 1) - 1) / c.sh + 1;
    c.Wo = (c.W + 2 * c.pw - c.dw * (c.kw - 1) - 1) / c.sw + 1;
    if (c.Ho <= 0 || c.Wo <= 0) return fail(FP8A_EINVAL, "empty convolution output");
    c.cog = c.Cout / c.groups;
    c.cig = c.Cin / c.groups;
    c.Mrows = c.Bn * c.Ho * c.Wo;
    c.Kg = c.cig * c.kh * c.kw;
    return FP8A_OK;
}

// One convolution launch family (conv2d_impl): every public entry point fills the fields it has.
struct ConvCall {
    ConvShape g;
    const float *x, *w;
    float *y;
    int E, Mw;
    const int32_t *bA, *bW, *bR, *table;
    uint32_t flags;
    const float *bn;  // the BN / activation epilogue
    int act;
    float act_lo, act_hi;
    void *workspace;
    size_t workspace_bytes;
    hipStream_t s;
    FqIn fq;  // the input quantizer (fq.mx set: x is not yet quantized), its bias outputs, the fake-quant buffer
    float *fqb;
    int32_t *fqi;
    float *xq;
    const float *res;  // the block tail
    int post_act;
    float post_lo, post_hi;
    FqIn post_fq;
    float *post_bout;
    int32_t *post_ibout;
    const uint32_t *in_img;  // the chain's word images
    EmitW em;
};

// A fused quantizer's arguments (none when mx is null): format, then its bias outputs.
static int fused_quantizer(const float *mx, int nbits, int mbits, int sign_bits, float *bias_out, int32_t *ibias_out,
                           FqIn &f) {
    f = FqIn{};
    if (!mx) return FP8A_OK;
    const int qE = nbits - sign_bits - mbits;
    if (mbits < 1 || qE < 1) return fail(FP8A_EFORMAT, "bad FP8 quantizer format");
    if (!bias_out || !ibias_out) return fail(FP8A_EINVAL, "null pointer");
    f = FqIn{mx, qE, mbits, sign_bits};
    return FP8A_OK;
}

// The fake-quant buffer of the non-fused paths (elems floats; elems < 0: none) sits at the workspace's
// end: rest = the bytes before it.
static int carve_xq(void *workspace, size_t workspace_bytes, int64_t elems, const char *name, size_t &rest,
                    float *&xq) {
    const size_t xq_bytes = elems < 0 ? 0 : align256((size_t)elems * sizeof(float));
    if (workspace == nullptr || workspace_bytes < FLAG_BYTES + xq_bytes)
        return fail(FP8A_EINVAL, std::string(name) + " workspace too small");
    rest = (workspace_bytes - xq_bytes) & ~(size_t)255;
    xq = elems < 0 ? nullptr : (float *)((char *)workspace + rest);
    return FP8A_OK;
}

static int invalidate_image(const EmitW &em, hipStream_t s) {
    return dev_fill(em.invalid, 1, sizeof(uint32_t), s) != hipSuccess ? hip_check("fp8a word image header") : FP8A_OK;
}

extern "C" {

const char *fp8a_version(void) { return "fp8approx gfx950 r1"; }

const char *fp8a_last_error(void) { return g_err.c_str(); }

int fp8a_path_stats(uint64_t *out, int reset) {
    if (out == nullptr) return fail(FP8A_EINVAL, "null pointer");
    for (int i = 0; i < PATH_N; ++i) out[i] = reset ? g_paths[i].exchange(0) : g_paths[i].load();
    return FP8A_OK;
}

size_t fp8a_flag_arena_slot_bytes(fp8a_stream_t stream) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lock(g_arena_mu);
    const auto it = g_arenas.find({dev, (uintptr_t)stream});
    return it == g_arenas.end() ? 0 : it->second.slot;
}

int fp8a_kernel_timing(int enable) {
    const int old = g_ktime ? 1 : 0;
    g_ktime = enable != 0;
    return old;
}

int fp8a_kernel_time(double *out, int reset) {
    if (out == nullptr) return fail(FP8A_EINVAL, "null pointer");
    for (int i = 0; i < 4 * PATH_N; ++i) out[i] = 0.0;
    for (const KernelEv &e : g_kev) {
        if (hipEventSynchronize(e.b) != hipSuccess) return hip_check("fp8a_kernel_time");
        float ms = 0.0f;
        if (hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) return hip_check("fp8a_kernel_time");
        out[4 * e.path] += ms;
        out[4 * e.path + 1] += 1.0;
        out[4 * e.path + 2] += e.dispatches;
        out[4 * e.path + 3] += e.macs;
    }
    if (reset) {
        for (const KernelEv &e : g_kev) {
            g_evpool.push_back(e.a);
            g_evpool.push_back(e.b);
        }
        g_kev.clear();
    }
    return FP8A_OK;
}

int fp8a_set_option(const char *name, int value) {
    if (name == nullptr) return fail(FP8A_EINVAL, "null pointer");
    for (Option &o : g_opts)
        if (strcmp(name, o.name) == 0) {
            const int old = o.value;
            o.value = opt_norm(o, value);
            return old;
        }
    return fail(FP8A_EINVAL, std::string("unknown option ") + name);
}

// fp8a_fq_selfcheck: the fast quantizer / word forms against the literal ones, pattern by pattern
__global__ __launch_bounds__(256) void fq_selfcheck_kernel(float mx, int E, int M, int S, int mode, int bR, uint64_t first,
                                                           uint64_t count, unsigned long long *out) {
    const float bias = fq_bias(mx, E, M);
    const bool fast = fq_fast_ok(mx, bias, M);
    const FqFast k = fast ? fq_fast_k(mx, bias, M) : FqFast{};
    const uint32_t emn = fast ? k.emn : 0x3F800000u;
    const int xb = xm_xbias(M), kse = 254 + xb - bR;
    const bool chk = fast && (mode == 2 || fq_word_chk(mx, bias, M, kse));
    unsigned long long bad = 0, lowest = ~0ull;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += stride) {
        const uint32_t bits = (uint32_t)(first + i);
        const float v = __uint_as_float(bits);
        const float ql = fq_apply(v, mx, bias, M, S);
        const float qf = fast ? fq_apply_f<true>(v, mx, bias, M, S, k) : ql;
        bool diff;
        if (mode == 0) {
            diff = __float_as_uint(ql) != __float_as_uint(qf);
        } else {
            bool okl = true, okf = true;
            const uint32_t wl = xm_word_a(ql, M, xb, emn, bR, okl);
            const uint32_t wf = fast ? fq_word(qf, M, kse, chk, okf) : xm_word_a(qf, M, xb, emn, bR, okf);
            diff = wl != wf || okl != okf;
        }
        if (diff) {
            ++bad;
            lowest = min(lowest, (unsigned long long)bits);
        }
    }
    if (bad) {
        atomicAdd(out, bad);
        atomicMin(out + 1, lowest);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) out[2] = (fast ? 1ull : 0ull) | (chk ? 2ull : 0ull);
}

int fp8a_fq_selfcheck(float maxval, int E, int M, int sign_bits, int mode, int bR, uint64_t first, uint64_t count,
                      uint64_t *out, fp8a_stream_t stream) {
    if (out == nullptr) return fail(FP8A_EINVAL, "null pointer");
    if (E < 1 || M < 1 || M > 6 || mode < 0 || mode > 2 || (mode != 0 && M != 3 && M != 2))
        return fail(FP8A_EFORMAT, "fp8a_fq_selfcheck: bad format or mode");
    if (first > 0xFFFFFFFFull || count > (1ull << 32) - first) return fail(FP8A_EINVAL, "pattern range beyond 2^32");
    hipStream_t s = (hipStream_t)stream;
    unsigned long long *d = nullptr;
    const unsigned long long init[3] = {0ull, ~0ull, 0ull};
    if (hipMalloc(&d, sizeof(init)) != hipSuccess) return hip_check("fp8a_fq_selfcheck");
    unsigned long long h[3] = {0, 0, 0};
    bool ok = hipMemcpyAsync(d, init, sizeof(init), hipMemcpyHostToDevice, s) == hipSuccess;
    if (ok && count > 0) {
        const unsigned blocks = (unsigned)std::min<uint64_t>((count + 255) / 256, 8192);
        fq_selfcheck_kernel<<<blocks, 256, 0, s>>>(maxval, E, M, sign_bits, mode, bR, first, count, d);
    }
    ok = ok && hipMemcpyAsync(h, d, sizeof(h), hipMemcpyDeviceToHost, s) == hipSuccess &&
         hipStreamSynchronize(s) == hipSuccess;
    (void)hipFree(d);
    if (!ok) return hip_check("fp8a_fq_selfcheck");
    for (int i = 0; i < 3; ++i) out[i] = h[i];
    return FP8A_OK;
}

int fp8a_fallback_stats(uint64_t *out, int reset) {
    if (out == nullptr) return fail(FP8A_EINVAL, "null pointer");
    unsigned long long v[4] = {0, 0, 0, 0}, tt = 0;
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(v, HIP_SYMBOL(g_fallback), sizeof(v)) != hipSuccess ||
        tt_rerun_stats(&tt, reset != 0) != 0)
        return hip_check("fp8a_fallback_stats");
    for (int i = 0; i < 4; ++i) out[i] = v[i];
    out[2] = tt;  // (gemm_tt_kernel's f32 reruns: k_tt.hip's counter)
    if (reset) {
        const unsigned long long z[4] = {0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_fallback), z, sizeof(z)) != hipSuccess) return hip_check("fp8a_fallback_stats");
    }
    return FP8A_OK;
}

size_t fp8a_dense_matmul_workspace_size(int64_t M, int64_t N, int64_t K) { return dense_ws_bytes(M, N, K); }

int fp8a_dense_matmul(const float *A, int64_t sam, int64_t sak, const float *B, int64_t sbk, int64_t sbn, float *C,
                      int64_t ldc, int64_t M, int64_t N, int64_t K, int fmt, void *workspace, size_t workspace_bytes,
                      fp8a_stream_t stream) {
    if (ldc < N) return fail(FP8A_EINVAL, "leading dimension smaller than extent");
    DenseArgs a = dense_args();
    a.x = A; a.sam = sam; a.sak = sak; a.w = B; a.sbk = sbk; a.sbn = sbn; a.y = C; a.ldc = ldc;
    a.M = M; a.N = N; a.K = K; a.fmt = fmt;
    return run_dense(a, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t fp8a_dense_conv2d_workspace_size(int64_t Bn, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int kh, int kw,
                                        int sh, int sw, int ph, int pw, int dh, int dw) {
    ConvShape c{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, 1};
    return conv_shape(c) ? 0 : dense_ws_bytes(c.Mrows, Cout, c.Kg);
}

// The exact convolution as run_dense's implicit GEMM (geometry rejected as conv_shape does, + negative counts).
static int dense_conv(ConvShape c, const float *x, const float *w, float *y, int fmt, const DnFuse &fz, void *ws,
                      size_t ws_bytes, hipStream_t s) {
    if (bad_geometry(c) || c.Bn < 0 || c.Cin < 0 || c.Cout < 0) return fail(FP8A_EINVAL, "bad convolution geometry");
    const int rc = conv_shape(c);
    if (rc) return rc;
    DenseArgs a = dense_args();
    a.x = x; a.w = w; a.y = y; a.conv = 1;
    a.C = c.Cin; a.H = c.H; a.W = c.W; a.Ho = c.Ho; a.Wo = c.Wo;
    a.kh = c.kh; a.kw = c.kw; a.sh = c.sh; a.sw = c.sw; a.ph = c.ph; a.pw = c.pw; a.dh = c.dh; a.dw = c.dw;
    a.M = c.Mrows; a.N = c.Cout; a.K = c.Kg;
    a.sbk = 1; a.sbn = a.K;  // w [Cout][Cin][kh][kw]: B(k, n) = w[n * K + k]
    a.ldc = c.Cout; a.fmt = fmt;
    a.fz = fz;
    return run_dense(a, ws, ws_bytes, s);
}

int fp8a_dense_conv2d(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                      int64_t Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int fmt,
                      void *workspace, size_t workspace_bytes, fp8a_stream_t stream) {
    return dense_conv(ConvShape{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, 1}, x, w, y, fmt, DnFuse{}, workspace,
                      workspace_bytes, (hipStream_t)stream);
}

static int grouped_conv_impl(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                             int64_t Cout, int groups, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                             const DnFuse &fz, hipStream_t stream);

int fp8a_grouped_conv2d(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                        int64_t Cout, int groups, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                        fp8a_stream_t stream) {
    return grouped_conv_impl(x, w, y, Bn, Cin, H, W, Cout, groups, kh, kw, sh, sw, ph, pw, dh, dw, DnFuse{},
                             (hipStream_t)stream);
}

static int grouped_conv_impl(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                             int64_t Cout, int groups, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw,
                             const DnFuse &fz, hipStream_t stream) {
    ConvShape c{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups};
    if (bad_geometry(c) || Bn < 0 || Cin < 0 || Cout < 0) return fail(FP8A_EINVAL, "bad convolution geometry");
    if (!groups_ok(groups, Cin, Cout)) return fail(FP8A_EINVAL, "channels not divisible by groups");
    const int rc = conv_shape(c);
    if (rc) return rc;
    const int64_t Ho = c.Ho, Wo = c.Wo;
    GcArgs a{};
    a.x = x; a.w = w; a.y = y;
    a.Cin = Cin; a.H = H; a.W = W; a.Cout = Cout; a.Ho = Ho; a.Wo = Wo;
    a.total = Bn * Cout * Ho * ((Wo + GC_OW - 1) / GC_OW);
    a.cig = (int)c.cig; a.cog = (int)c.cog;
    a.kh = kh; a.kw = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw; a.dh = dh; a.dw = dw;
    a.fz = fz;
    if (a.total == 0) {  // (no kernel to leave the fused quantizers' biases)
        if (fz.qin.mx || fz.rq.mx || fz.oq.mx || fz.wq.mx) {
            dn_bias_kernel<<<(unsigned)std::max<int64_t>(1, (Cout + 255) / 256), 256, 0, stream>>>(fz, Cout);
            return hip_check("fp8a grouped conv quantizer biases");
        }
        return FP8A_OK;
    }
    if (!x || !w || !y) return fail(FP8A_EINVAL, "null pointer");
    if (opt(OPT_DW3) && a.cig == 1 && a.cog == 1 && kh == 3 && kw == 3 && dh == 1 && dw == 1 && sh == sw && pw <= DW_OX &&
        (sh == 1 || sh == 2)) {
        DwArgs d{};
        d.x = x; d.w = w; d.y = y; d.fz = fz;
        d.planes = Bn * Cout; d.C = (int)Cout; d.H = (int)H; d.W = (int)W; d.Ho = (int)Ho; d.Wo = (int)Wo;
        d.ph = ph; d.pw = pw;
        size_t lds = 0;
        // (the staged kernels index a plane in 32-bit ints and divide by float reciprocals, dw_div:
        // planes of at most 2^22 values; larger ones take dn_group_conv)
        d.nx = Bn * Cin * H * W;
        const bool raw = opt(OPT_DW3) == 2;
        if (H < (1 << 20) && W < (1 << 20) && Cout < (1 << 20) && H * W < (1ll << 22) && plan_dw3(d, sh, lds, raw)) {
            const unsigned g = (unsigned)(((d.planes + d.PB - 1) / d.PB) * d.nb);
            if (raw && sh == 1) dn_dw3g_kernel<1><<<g, 256, lds, stream>>>(d);
            else if (raw) dn_dw3g_kernel<2><<<g, 256, lds, stream>>>(d);
            else if (sh == 1) dn_dw3_kernel<1><<<g, 256, lds, stream>>>(d);
            else dn_dw3_kernel<2><<<g, 256, lds, stream>>>(d);
            ++g_paths[PATH_DENSE];
            return hip_check("fp8a depthwise conv launch");
        }
    }
    if (a.total + 65536ll * 256 < (1ll << 31)) launch_group_conv<uint32_t>(a, stream);
    else launch_group_conv<int64_t>(a, stream);
    ++g_paths[PATH_DENSE];
    return hip_check("fp8a grouped conv launch");
}

int fp8a_clock_stats(uint64_t *out, int reset) {
    if (out == nullptr) return fail(FP8A_EINVAL, "null pointer");
    if (hipDeviceSynchronize() != hipSuccess) return hip_check("fp8a_clock_stats");
    // reset bit 0: zero the sums after reading; bit 1: out = the cycle sum's three phases (before the first
    // barrier, the K loop, after it: gemm_f8mx.h g_clk[3..5]) instead of {cycles, 100 MHz ticks, workgroups}
    unsigned long long v[6] = {0, 0, 0, 0, 0, 0};
    int (*parts[3])(unsigned long long *, bool) = {f8mx_clock_xf0, f8mx_clock_xf1, f8mx_clock_xf2};
    for (auto f : parts) {
        unsigned long long w[6] = {0, 0, 0, 0, 0, 0};
        if (f(w, (reset & 1) != 0) != 0) return hip_check("fp8a_clock_stats");
        for (int i = 0; i < 6; ++i) v[i] += w[i];
    }
    for (int i = 0; i < 3; ++i) out[i] = v[i + ((reset & 2) ? 3 : 0)];
    return FP8A_OK;
}

int fp8a_splitk_stats(uint64_t *out, int reset) {
    if (out == nullptr) return fail(FP8A_EINVAL, "null pointer");
    out[0] = g_splitk_launches;
    if (reset) g_splitk_launches = 0;
    return FP8A_OK;
}

int fp8a_xm_sign_stats(uint64_t *out, int reset) {
    if (out == nullptr) return fail(FP8A_EINVAL, "null pointer");
    if (hipDeviceSynchronize() != hipSuccess) return hip_check("fp8a_xm_sign_stats");
    unsigned long long v[2] = {0, 0};
    int (*parts[3])(unsigned long long *, bool) = {f8mx_signs_xf0, f8mx_signs_xf1, f8mx_signs_xf2};
    for (auto f : parts) {
        unsigned long long w[2] = {0, 0};
        if (f(w, reset != 0) != 0) return hip_check("fp8a_xm_sign_stats");
        for (int i = 0; i < 2; ++i) v[i] += w[i];
    }
    for (int i = 0; i < 2; ++i) out[i] = v[i];
    return FP8A_OK;
}

int fp8a_dense_stats(uint64_t *out, int reset) {
    if (out == nullptr) return fail(FP8A_EINVAL, "null pointer");
    unsigned long long v[2] = {0, 0};
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpyFromSymbol(v, HIP_SYMBOL(g_dense), sizeof(v)) != hipSuccess)
        return hip_check("fp8a_dense_stats");
    out[0] = v[0];
    out[1] = v[1];
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_dense), z, sizeof(z)) != hipSuccess) return hip_check("fp8a_dense_stats");
    }
    return FP8A_OK;
}

int fp8a_decompose(const float *x, int64_t rows, int64_t cols, int64_t ld, int E, int M, const int32_t *bias,
                   int64_t bias_stride, uint32_t flags, int32_t *expo, int32_t *mant, fp8a_stream_t stream) {
    int rc = check_format(E, M);
    if (rc) return rc;
    if (rows < 0 || cols < 0 || ld < cols) return fail(FP8A_EINVAL, "bad decompose extents");
    const int64_t total = rows * cols;
    if (total == 0) return FP8A_OK;
    decompose_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(
        x, rows, cols, ld, E, M, bias, bias_stride, flags, expo, mant);
    return hip_check("fp8a_decompose");
}

int fp8a_quant(const float *x, int64_t n, int E, int M, const int32_t *bias, uint32_t flags, float *out,
               fp8a_stream_t stream) {
    int rc = check_format(E, M);
    if (rc) return rc;
    if (n <= 0) return FP8A_OK;
    quant_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(x, n, E, M, bias, flags, out);
    return hip_check("fp8a_quant");
}

static GemmArgs make_args(const float *A, int64_t lda, const float *B, int64_t sbk, int64_t sbn, float *C,
                          int64_t ldc, int64_t M, int64_t N, int64_t K, int E, int Mw, const int32_t *bA,
                          const int32_t *bB, int64_t bBs, const int32_t *bR, uint32_t flags) {
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.lda = lda; a.B = B; a.sbk = sbk; a.sbn = sbn; a.C = C; a.ldc = ldc;
    a.M = M; a.N = N; a.K = K; a.E = E; a.Mw = Mw; a.kexp = 0x7F800000u; a.kdc = (uint32_t)(23 - Mw) << 23;
    a.bA = bA; a.bB = bB; a.bBs = bBs; a.bR = bR;
    a.flags = flags; a.nchw = 0; a.hw = 1; a.ctot = N; a.coff = 0;
    a.splits = 1; a.kchunk = K; a.part = nullptr;
    a.fq_fast = opt(OPT_FQ_FAST);
    return a;
}

size_t fp8a_matmul_workspace_size(void) { return FLAG_BYTES; }

size_t fp8a_matmul_workspace_size_mnk(int64_t M, int64_t N, int64_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return FLAG_BYTES;
    return gemm_workspace_bytes(M, N, K, 0);
}

int fp8a_matmul(const float *A, int64_t lda, const float *B, int64_t sbk, int64_t sbn, float *C, int64_t ldc,
                int64_t M, int64_t N, int64_t K, int E, int Mw, const int32_t *bA, const int32_t *bB,
                int64_t bB_stride, const int32_t *bR, const int32_t *table, uint32_t flags, void *workspace,
                size_t workspace_bytes, fp8a_stream_t stream) {
    if (lda < K || ldc < N) return fail(FP8A_EINVAL, "leading dimension smaller than extent");
    GemmArgs a = make_args(A, lda, B, sbk, sbn, C, ldc, M, N, K, E, Mw, bA, bB, bB_stride, bR, flags);
    return run_gemm(a, table, workspace, workspace_bytes, (hipStream_t)stream);
}

// ------------------------------------------------------------------------- batched product
// fp8a_bmm (gemm_bmm.h): one launch of gemm_bmm_kernel over (64 x 64 tiles, batch items); nothing else on
// the stream -- no workspace, no pre-pass, no gated kernel -- so it is capture-safe by construction.
static std::atomic<uint64_t> g_bmm_launches, g_bmm_tiles;  // host-side (a replayed graph adds nothing)

// elements spanned by a (batch, batch, rows, cols) view of non-negative strides
static int64_t bmm_span(int64_t n0, int64_t s0, int64_t n1, int64_t s1, int64_t r, int64_t sr, int64_t c, int64_t sc) {
    return (n0 - 1) * s0 + (n1 - 1) * s1 + (r - 1) * sr + (c - 1) * sc + 1;
}

// C over an operand, where that is cheap to see: the same base, or two dense spans that meet.  ea, eb, ec:
// the views' bmm_span; fp8a_bmm and fp8a_grad_bmm.
static bool c_overlaps_operand(const float *A, int64_t ea, const float *B, int64_t eb, const float *C, int64_t ec,
                               int64_t nb, int64_t M, int64_t N, int64_t K) {
    const bool dc = ec == nb * M * N;
    const bool oa = C == A || (dc && ea == nb * M * K && C < A + ea && A < C + ec);
    const bool ob = C == B || (dc && eb == nb * K * N && C < B + eb && B < C + ec);
    return oa || ob;
}

// What fp8a_bmm and fp8a_bmm_check refuse alike in a batched view, each in its own order: fp8a_bmm_check
// looks at the strides first.  who: the entry, for the texts that carry one.
static int bmm_view_check(const char *who, uint32_t flags, int64_t bB_stride, bool neg_stride, bool strides_first) {
    const std::string w = std::string(who) + ": ";
    if (strides_first && neg_stride) return fail(FP8A_EINVAL, w + "negative stride");
    if (flags & F_TB)
        return fail(FP8A_EINVAL, "fp8a_bmm: no tensor-bias semantics (FP8A_TB) for a batched product");
    if (flags & (F_V5 | F_OFUF | F_OF | F_UF))
        return fail(FP8A_EINVAL, "fp8a_bmm: the v5 model is not implemented for a batched product");
    if (flags & ~(F_APPROX | F_S2N | F_QBMA | F_GCLIP)) return fail(FP8A_EINVAL, w + "unknown flag bits");
    if (bB_stride != 0 && bB_stride != 1) return fail(FP8A_EINVAL, w + "bB_stride must be 0 or 1");
    if (neg_stride) return fail(FP8A_EINVAL, w + "negative stride");
    return FP8A_OK;
}

int fp8a_bmm(const float *A, const float *B, float *C, int64_t nb0, int64_t nb1, int64_t M, int64_t N, int64_t K,
             int64_t lda, int64_t sa0, int64_t sa1, int64_t sbk, int64_t sbn, int64_t sb0, int64_t sb1, int64_t ldc,
             int64_t sc0, int64_t sc1, int E, int Mw, const int32_t *bA, const int32_t *bB, int64_t bB_stride,
             const int32_t *bR, const int32_t *table, uint32_t flags, fp8a_stream_t stream) {
    int rc = check_format(E, Mw);
    if (rc) return rc;
    if (nb0 < 0 || nb1 < 0 || M < 0 || N < 0 || K < 0) return fail(FP8A_EINVAL, "fp8a_bmm: negative extent");
    const bool neg_stride = lda < 0 || sa0 < 0 || sa1 < 0 || sbk < 0 || sbn < 0 || sb0 < 0 || sb1 < 0 || ldc < 0 ||
                            sc0 < 0 || sc1 < 0;
    rc = bmm_view_check("fp8a_bmm", flags, bB_stride, neg_stride, false);
    if (rc) return rc;
    if ((M > 1 && lda < K) || (M > 1 && ldc < N)) return fail(FP8A_EINVAL, "leading dimension smaller than extent");
    TablePack tp;
    int mode;
    rc = pack_table(table, Mw, (flags & F_APPROX) != 0, tp, mode);
    if (rc) return rc;
    const int64_t nb = nb0 * nb1;
    if (nb == 0 || M == 0 || N == 0) return FP8A_OK;
    if (!C || (K > 0 && (!A || !B || !bA || !bB || !bR))) return fail(FP8A_EINVAL, "fp8a_bmm: null pointer");
    if (K > 0 && c_overlaps_operand(A, bmm_span(nb0, sa0, nb1, sa1, M, lda, K, 1), B,
                                    bmm_span(nb0, sb0, nb1, sb1, K, sbk, N, sbn), C,
                                    bmm_span(nb0, sc0, nb1, sc1, M, ldc, N, 1), nb, M, N, K))
        return fail(FP8A_EINVAL, "fp8a_bmm: C overlaps an operand");
    BmmArgs a;
    memset(&a, 0, sizeof(a));
    a.A = A; a.B = B; a.C = C; a.nb1 = nb1; a.M = M; a.N = N; a.K = K;
    a.lda = lda; a.sa0 = sa0; a.sa1 = sa1; a.sbk = sbk; a.sbn = sbn; a.sb0 = sb0; a.sb1 = sb1;
    a.ldc = ldc; a.sc0 = sc0; a.sc1 = sc1;
    a.num_mt = (M + BM - 1) / BM;
    a.tiles = a.num_mt * ((N + BN - 1) / BN);
    a.E = E; a.Mw = Mw; a.kexp = 0x7F800000u; a.kdc = (uint32_t)(23 - Mw) << 23;
    a.bA = bA; a.bB = bB; a.bBs = bB_stride; a.bR = bR; a.flags = flags;
    a.tab = tp;
    a.recount = bmm_recount_ptr();
    if (a.recount == nullptr) return fail(FP8A_EHIP, "fp8a_bmm: the recomputed-tile counter's address");
    if (a.tiles > 0x7FFFFFFFll / nb) return fail(FP8A_EINVAL, "fp8a_bmm: more than 2^31 - 1 tiles");
    if (f8_form(E, Mw, flags, tp)) mode = TM_F8;
    const dim3 grid((unsigned)(a.tiles * nb));
    const bool s2n = flags & F_S2N, q = flags & F_QBMA, gc = flags & F_GCLIP;
    hipStream_t s = (hipStream_t)stream;
    if (s2n) q ? launch_bmm_p3(mode, gc, a, grid, s) : launch_bmm_p2(mode, gc, a, grid, s);
    else q ? launch_bmm_p1(mode, gc, a, grid, s) : launch_bmm_p0(mode, gc, a, grid, s);
    ++g_bmm_launches;
    g_bmm_tiles += (uint64_t)(a.tiles * nb);
    return hip_check("fp8a_bmm launch");
}

int fp8a_bmm_stats(uint64_t out[3], int reset) {
    if (out == nullptr) return fail(FP8A_EINVAL, "null pointer");
    unsigned long long r = 0;
    if (hipDeviceSynchronize() != hipSuccess || bmm_recount_read(&r, reset != 0) != 0) return hip_check("fp8a_bmm_stats");
    out[0] = g_bmm_launches.load();
    out[1] = g_bmm_tiles.load();
    out[2] = r;
    if (reset) {
        g_bmm_launches = 0;
        g_bmm_tiles = 0;
    }
    return FP8A_OK;
}

// ------------------------------------------------------------------------- gradient GEMM
// fp8a_grad_bmm (gemm_grad.h): one launch of gemm_grad_kernel over (64 x 64 tiles, batch items), nothing else
// on the stream, as fp8a_bmm.  fp8a_grad_bmm_split: the same product with K split into S parts -- the product
// pass over (tiles, batch items, parts) into the caller's workspace, then the reduce pass, both on the stream.
static std::atomic<uint64_t> g_grad_launches, g_grad_tiles;  // host-side (a replayed graph adds nothing)

// What both entries check, with the same texts under the entry's own name, and the kernel's arguments.
// FP8A_OK with run = false: an empty product, nothing to launch.
static int grad_args(const char *who, const float *A, const float *B, float *C, int64_t nb, int64_t M, int64_t N,
                     int64_t K0, int64_t K1, int64_t sa_i, int64_t sa_m, int64_t sa_k0, int64_t sa_k1, int64_t sb_i,
                     int64_t sb_k0, int64_t sb_k1, int64_t sb_n, int64_t sc_i, int64_t sc_m, int64_t sc_n, GradArgs &a,
                     bool &run) {
    const std::string w = std::string(who) + ": ";
    run = false;
    if (nb < 0 || M < 0 || N < 0 || K0 < 0 || K1 < 0) return fail(FP8A_EINVAL, w + "negative extent");
    if (sa_i < 0 || sa_m < 0 || sa_k0 < 0 || sa_k1 < 0 || sb_i < 0 || sb_k0 < 0 || sb_k1 < 0 || sb_n < 0 || sc_i < 0 ||
        sc_m < 0 || sc_n < 0)
        return fail(FP8A_EINVAL, w + "negative stride");
    if (K0 > 0 && K1 > 0x7FFFFFFFll / K0) return fail(FP8A_EINVAL, w + "K0 * K1 exceeds 2^31 - 1");
    const int64_t K = K0 * K1;
    if (nb == 0 || M == 0 || N == 0) return FP8A_OK;
    if (!C || (K > 0 && (!A || !B))) return fail(FP8A_EINVAL, w + "null pointer");
    if ((sc_m == 0 && M > 1) || (sc_n == 0 && N > 1) || (sc_i == 0 && nb > 1))
        return fail(FP8A_EINVAL, w + "a zero stride of C over an extent above 1");
    if (K > 0 && c_overlaps_operand(A, bmm_span(nb, sa_i, M, sa_m, K0, sa_k0, K1, sa_k1), B,
                                    bmm_span(nb, sb_i, K0, sb_k0, K1, sb_k1, N, sb_n), C,
                                    bmm_span(1, 0, nb, sc_i, M, sc_m, N, sc_n), nb, M, N, K))
        return fail(FP8A_EINVAL, w + "C overlaps an operand");
    memset(&a, 0, sizeof(a));
    a.A = A; a.B = B; a.C = C; a.M = M; a.N = N;
    a.K0 = (uint32_t)K0; a.K1 = (uint32_t)K1; a.K = (uint32_t)K;
    a.sa_i = sa_i; a.sa_m = sa_m; a.sa_k0 = sa_k0; a.sa_k1 = sa_k1;
    a.sb_i = sb_i; a.sb_k0 = sb_k0; a.sb_k1 = sb_k1; a.sb_n = sb_n;
    a.sc_i = sc_i; a.sc_m = sc_m; a.sc_n = sc_n;
    a.num_mt = (M + GR_T - 1) / GR_T;
    a.tiles = a.num_mt * ((N + GR_T - 1) / GR_T);
    if (a.tiles > 0x7FFFFFFFll / nb) return fail(FP8A_EINVAL, w + "more than 2^31 - 1 tiles");
    run = true;
    return FP8A_OK;
}

int fp8a_grad_bmm(const float *A, const float *B, float *C, int64_t nb, int64_t M, int64_t N, int64_t K0, int64_t K1,
                  int64_t sa_i, int64_t sa_m, int64_t sa_k0, int64_t sa_k1, int64_t sb_i, int64_t sb_k0, int64_t sb_k1,
                  int64_t sb_n, int64_t sc_i, int64_t sc_m, int64_t sc_n, fp8a_stream_t stream) {
    GradArgs a;
    bool run;
    const int rc = grad_args("fp8a_grad_bmm", A, B, C, nb, M, N, K0, K1, sa_i, sa_m, sa_k0, sa_k1, sb_i, sb_k0, sb_k1,
                             sb_n, sc_i, sc_m, sc_n, a, run);
    if (rc || !run) return rc;
    a.recount = grad_recount_ptr();
    if (a.recount == nullptr) return fail(FP8A_EHIP, "fp8a_grad_bmm: the recomputed-tile counter's address");
    launch_grad(a, dim3((unsigned)(a.tiles * nb)), (hipStream_t)stream);
    ++g_grad_launches;
    g_grad_tiles += (uint64_t)(a.tiles * nb);
    return hip_check("fp8a_grad_bmm launch");
}

// The split plan: nst = ceil(K / 32) stages, per = ceil(nst / splits) stages per part, S = ceil(nst / per)
// parts, none empty; part s owns the stages [s per, min((s + 1) per, nst)).  S = 1 when nst <= 1 or splits = 1.
static void grad_split_plan(int64_t K, int64_t splits, int64_t &per, int64_t &S) {
    const int64_t nst = (K + GR_BK - 1) / GR_BK;
    per = nst > 0 ? (nst + splits - 1) / splits : 1;
    S = nst > 0 ? (nst + per - 1) / per : 1;
}

int fp8a_grad_bmm_split_workspace_size(int64_t nb, int64_t M, int64_t N, int64_t K0, int64_t K1, int64_t splits,
                                       int64_t *eff_splits, int64_t *bytes) {
    const char *const w = "fp8a_grad_bmm_split_workspace_size: ";
    if (!eff_splits || !bytes) return fail(FP8A_EINVAL, std::string(w) + "null pointer");
    if (nb < 0 || M < 0 || N < 0 || K0 < 0 || K1 < 0) return fail(FP8A_EINVAL, std::string(w) + "negative extent");
    if (K0 > 0 && K1 > 0x7FFFFFFFll / K0) return fail(FP8A_EINVAL, std::string(w) + "K0 * K1 exceeds 2^31 - 1");
    if (splits < 1) return fail(FP8A_EINVAL, std::string(w) + "splits below 1");
    int64_t per, S;
    grad_split_plan(K0 * K1, splits, per, S);
    const int64_t tiles = ((M + GR_T - 1) / GR_T) * ((N + GR_T - 1) / GR_T);
    if (nb > 0 && tiles > 0 && tiles > 0x7FFFFFFFll / nb / S)
        return fail(FP8A_EINVAL, std::string(w) + "more than 2^31 - 1 blocks");
    *eff_splits = S;
    *bytes = S > 1 ? S * nb * tiles * (GR_T * GR_T) * (int64_t)sizeof(float) : 0;
    return FP8A_OK;
}

int fp8a_grad_bmm_split(const float *A, const float *B, float *C, int64_t nb, int64_t M, int64_t N, int64_t K0,
                        int64_t K1, int64_t sa_i, int64_t sa_m, int64_t sa_k0, int64_t sa_k1, int64_t sb_i,
                        int64_t sb_k0, int64_t sb_k1, int64_t sb_n, int64_t sc_i, int64_t sc_m, int64_t sc_n,
                        int64_t splits, void *workspace, int64_t workspace_bytes, fp8a_stream_t stream) {
    GradArgs a;
    bool run;
    const int rc = grad_args("fp8a_grad_bmm_split", A, B, C, nb, M, N, K0, K1, sa_i, sa_m, sa_k0, sa_k1, sb_i, sb_k0,
                             sb_k1, sb_n, sc_i, sc_m, sc_n, a, run);
    if (rc) return rc;
    if (splits < 1) return fail(FP8A_EINVAL, "fp8a_grad_bmm_split: splits below 1");
    if (!run) return FP8A_OK;
    int64_t per, S;
    grad_split_plan(K0 * K1, splits, per, S);
    if (a.tiles * nb > 0x7FFFFFFFll / S) return fail(FP8A_EINVAL, "fp8a_grad_bmm_split: more than 2^31 - 1 blocks");
    const int64_t need = S * nb * a.tiles * (GR_T * GR_T) * (int64_t)sizeof(float);
    if (S > 1) {
        if (!workspace) return fail(FP8A_EINVAL, "fp8a_grad_bmm_split: null workspace");
        if (workspace_bytes < need)
            return fail(FP8A_EINVAL, "fp8a_grad_bmm_split: workspace of " + std::to_string(workspace_bytes) +
                                         " bytes, " + std::to_string(need) + " needed");
        if (((uintptr_t)workspace & 15u) != 0)
            return fail(FP8A_EINVAL, "fp8a_grad_bmm_split: workspace not 16-byte aligned");
        // the workspace over A, B or C, where that is cheap to see: c_overlaps_operand's rule with the workspace
        // (dense by construction) in C's place, and C as an operand when it is dense
        const float *const W = (const float *)workspace;
        const int64_t ew = need / (int64_t)sizeof(float), K = K0 * K1;
        const int64_t ea = bmm_span(nb, sa_i, M, sa_m, K0, sa_k0, K1, sa_k1);
        const int64_t eb = bmm_span(nb, sb_i, K0, sb_k0, K1, sb_k1, N, sb_n);
        const int64_t ec = bmm_span(1, 0, nb, sc_i, M, sc_m, N, sc_n);
        const bool oa = W == A || (ea == nb * M * K && W < A + ea && A < W + ew);
        const bool ob = W == B || (eb == nb * K * N && W < B + eb && B < W + ew);
        const bool oc = W == C || (ec == nb * M * N && W < C + ec && C < W + ew);
        if (oa || ob || oc) return fail(FP8A_EINVAL, "fp8a_grad_bmm_split: the workspace overlaps A, B or C");
    }
    a.recount = grad_recount_ptr();
    if (a.recount == nullptr) return fail(FP8A_EHIP, "fp8a_grad_bmm_split: the recomputed-tile counter's address");
    if (S == 1) launch_grad(a, dim3((unsigned)(a.tiles * nb)), (hipStream_t)stream);
    else launch_grad_split(a, nb, S, per, (float *)workspace, (hipStream_t)stream);
    ++g_grad_launches;
    g_grad_tiles += (uint64_t)(a.tiles * nb * S);
    return hip_check("fp8a_grad_bmm_split launch");
}

int fp8a_grad_stats(uint64_t out[3], int reset) {
    if (out == nullptr) return fail(FP8A_EINVAL, "null pointer");
    unsigned long long r = 0;
    if (hipDeviceSynchronize() != hipSuccess || grad_recount_read(&r, reset != 0) != 0)
        return hip_check("fp8a_grad_stats");
    out[0] = g_grad_launches.load();
    out[1] = g_grad_tiles.load();
    out[2] = r;
    if (reset) {
        g_grad_launches = 0;
        g_grad_tiles = 0;
    }
    return FP8A_OK;
}

int fp8a_terms(const float *A, int64_t lda, const float *B, int64_t sbk, int64_t sbn, float *T, int64_t M,
               int64_t N, int64_t K, int E, int Mw, const int32_t *bA, const int32_t *bB, int64_t bB_stride,
               const int32_t *bR, const int32_t *table, uint32_t flags, fp8a_stream_t stream) {
    int rc = check_format(E, Mw);
    if (rc) return rc;
    GemmArgs a = make_args(A, lda, B, sbk, sbn, nullptr, 0, M, N, K, E, Mw, bA, bB, bB_stride, bR, flags);
    int mode;
    rc = pack_table(table, Mw, (flags & (F_APPROX | F_V5)) != 0, a.tab, mode);
    if (rc) return rc;
    const int64_t total = M * N * K;
    if (total == 0) return FP8A_OK;
    terms_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(a, T);
    return hip_check("fp8a_terms");
}

// ------------------------------------------------------------------------- fused self-check
// fp8a_matmul_check / fp8a_bmm_check / fp8a_conv2d_check (gemm_check.h): one kernel over `units` products of
// M x N x K -- the one matrix product, the nb0 x nb1 batch items, the convolution groups.  Workspace = the
// dense S image (one float per output, units M N of them), then one CheckPart per workgroup (unit x 64 x 64 tile).
static int64_t check_tiles(int64_t M, int64_t N) { return ((M + CK_BM - 1) / CK_BM) * ((N + CK_BN - 1) / CK_BN); }
// Sizes saturate instead of wrapping, so an absurd extent fails the workspace test, not the arithmetic.
static size_t check_ws_bytes(int64_t units, int64_t M, int64_t N) {
    int64_t outs, parts;  // (positive extents; 2^56: far above any device, far below a wrap of the sums)
    if (__builtin_mul_overflow(units, M, &outs) || __builtin_mul_overflow(outs, N, &outs) || outs > (1ll << 56) ||
        M > (1ll << 40) || N > (1ll << 40) || __builtin_mul_overflow(units, check_tiles(M, N), &parts) ||
        parts > (1ll << 50))
        return SIZE_MAX;
    return align256((size_t)outs * 4) + align256(check_part_bytes(parts));
}
// (the size queries' answer: 0 for what no workspace can hold)
static size_t check_ws_query(int64_t units, int64_t M, int64_t N) {
    const size_t b = check_ws_bytes(units, M, N);
    return b == SIZE_MAX ? 0 : b;
}
// nb0 nb1 of non-negative extents, saturating
static int64_t bmm_units(int64_t nb0, int64_t nb1) {
    int64_t nb;
    return __builtin_mul_overflow(nb0, nb1, &nb) ? INT64_MAX : nb;
}

// The tail of all three entries, from the checks they share to the launch.  c: the operands, extents, units and
// flags; this fills tiles, S, part and the table.
static int run_check(CheckArgs &c, const int32_t *table, void *ws, size_t ws_bytes, hipStream_t s) {
    int rc = check_format(c.E, c.Mw);
    if (rc) return rc;
    if (c.flags & F_V5) return fail(FP8A_EINVAL, "the self-check covers the v9 model only (no FP8A_V5)");
    if (c.units <= 0 || c.M <= 0 || c.N <= 0 || c.K <= 0)
        return fail(FP8A_EINVAL, "self-check extents must be positive");
    if (!c.A || !c.B || !c.C || !c.bA || !c.bB || !c.bR || !c.stats) return fail(FP8A_EINVAL, "null pointer");
    if (ws == nullptr || (((uintptr_t)ws) & 255) != 0 || ws_bytes < check_ws_bytes(c.units, c.M, c.N))
        return fail(FP8A_EINVAL, "self-check workspace missing, misaligned or too small");
    if ((((uintptr_t)c.stats) & 7) != 0) return fail(FP8A_EINVAL, "stats must be 8-byte aligned");
    // (the workspace test bounds units M N: no product below wraps)
    c.tiles_n = (c.N + CK_BN - 1) / CK_BN;
    c.tiles = check_tiles(c.M, c.N);
    if (c.tiles > 0x7FFFFFFFll / c.units || (c.conv && c.units > 65535))
        return fail(FP8A_EINVAL, "self-check grid too large");
    int mode;
    rc = pack_table(table, c.Mw, (c.flags & F_APPROX) != 0, c.tab, mode);
    if (rc) return rc;
    // a diagnostic, not for graphs
    const int cap = stream_capturing(s);
    if (cap < 0) return capture_query_error("fp8a self-check:");
    if (cap) return fail(FP8A_EINVAL, "the self-check does not run on a capturing stream");
    c.S = (float *)ws;
    c.part = (CheckPart *)((char *)ws + align256((size_t)(c.units * c.M * c.N) * 4));
    launch_check(c, s);
    return hip_check("fp8a self-check launch");
}

// what all three entries set alike (one unit until the caller says otherwise); the rest stays zero
static CheckArgs check_args(const float *A, const float *B, float *C, int64_t M, int64_t N, int64_t K, int E, int Mw,
                            const int32_t *bA, const int32_t *bB, int64_t bBs, const int32_t *bR, uint32_t flags,
                            float *G, const float *Cprod, fp8a_check_stats *stats) {
    CheckArgs c{};
    c.A = A; c.B = B; c.C = C; c.G = G; c.Cprod = Cprod; c.stats = stats;
    c.M = M; c.N = N; c.K = K; c.E = E; c.Mw = Mw;
    c.bA = bA; c.bB = bB; c.bBs = bBs; c.bR = bR; c.flags = flags;
    c.units = 1; c.nb1 = 1;
    return c;
}

size_t fp8a_check_workspace_size(int64_t M, int64_t N, int64_t K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return check_ws_query(1, M, N);
}

int fp8a_matmul_check(const float *A, int64_t lda, const float *B, int64_t sbk, int64_t sbn, float *C, int64_t ldc,
                      int64_t M, int64_t N, int64_t K, int E, int Mw, const int32_t *bA, const int32_t *bB,
                      int64_t bB_stride, const int32_t *bR, const int32_t *table, uint32_t flags, float *G,
                      const float *Cprod, fp8a_check_stats *stats, void *workspace, size_t workspace_bytes,
                      fp8a_stream_t stream) {
    if (lda < K || ldc < N) return fail(FP8A_EINVAL, "leading dimension smaller than extent");
    CheckArgs c = check_args(A, B, C, M, N, K, E, Mw, bA, bB, bB_stride, bR, flags, G, Cprod, stats);
    c.lda = lda; c.sbk = sbk; c.sbn = sbn; c.ldc = ldc;
    return run_check(c, table, workspace, workspace_bytes, (hipStream_t)stream);
}

// fp8a_bmm_check: the units are the nb0 x nb1 items, C, G, Cprod and S dense [nb0][nb1][M][N].
size_t fp8a_bmm_check_workspace_size(int64_t nb0, int64_t nb1, int64_t M, int64_t N, int64_t K) {
    if (nb0 <= 0 || nb1 <= 0 || M <= 0 || N <= 0 || K <= 0) return 0;
    return check_ws_query(bmm_units(nb0, nb1), M, N);
}

int fp8a_bmm_check(const float *A, const float *B, float *C, int64_t nb0, int64_t nb1, int64_t M, int64_t N, int64_t K,
                   int64_t lda, int64_t sa0, int64_t sa1, int64_t sbk, int64_t sbn, int64_t sb0, int64_t sb1, int E,
                   int Mw, const int32_t *bA, const int32_t *bB, int64_t bB_stride, const int32_t *bR,
                   const int32_t *table, uint32_t flags, float *G, const float *Cprod, fp8a_check_stats *stats,
                   void *workspace, size_t workspace_bytes, fp8a_stream_t stream) {
    int rc = check_format(E, Mw);
    if (rc) return rc;
    if (nb0 < 0 || nb1 < 0 || M < 0 || N < 0 || K < 0) return fail(FP8A_EINVAL, "fp8a_bmm_check: negative extent");
    const bool neg_stride = lda < 0 || sa0 < 0 || sa1 < 0 || sbk < 0 || sbn < 0 || sb0 < 0 || sb1 < 0;
    rc = bmm_view_check("fp8a_bmm_check", flags, bB_stride, neg_stride, true);
    if (rc) return rc;
    if (M > 1 && lda < K) return fail(FP8A_EINVAL, "leading dimension smaller than extent");
    CheckArgs c = check_args(A, B, C, M, N, K, E, Mw, bA, bB, bB_stride, bR, flags, G, Cprod, stats);
    c.units = bmm_units(nb0, nb1); c.nb1 = nb1;
    c.lda = lda; c.sa0 = sa0; c.sa1 = sa1; c.sbk = sbk; c.sbn = sbn; c.sb0 = sb0; c.sb1 = sb1; c.ldc = N;
    return run_check(c, table, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t fp8a_conv2d_check_workspace_size(int64_t Bn, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int kh, int kw,
                                        int sh, int sw, int ph, int pw, int dh, int dw, int groups) {
    ConvShape c{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups};
    if (conv_shape(c) || Bn <= 0 || Cout <= 0 || Cin <= 0) return 0;
    return check_ws_query(groups, c.Mrows, c.cog);
}

int fp8a_conv2d_check(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                      int64_t Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups, int E,
                      int Mw, const int32_t *bA, const int32_t *bW, const int32_t *bR, const int32_t *table,
                      uint32_t flags, float *G, const float *Cprod, fp8a_check_stats *stats, void *workspace,
                      size_t workspace_bytes, fp8a_stream_t stream) {
    int rc = check_format(E, Mw);
    if (rc) return rc;
    // (the self-check wants positive extents on top of conv_shape's checks)
    ConvShape g{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups};
    if (!groups_ok(groups, Cin, Cout) || Cout <= 0 || Cin <= 0) return fail(FP8A_EINVAL, "bad groups");
    if (bad_geometry(g) || Bn <= 0 || H <= 0 || W <= 0) return fail(FP8A_EINVAL, "bad convolution geometry");
    rc = conv_shape(g);
    if (rc) return rc;
    const int64_t Ho = g.Ho, Wo = g.Wo, cog = g.cog, cig = g.cig, Kg = g.Kg, Mrows = g.Mrows;
    // single-output-channel groups: the tensor-bias semantics, as fp8a_conv2d (approx_calculation.py:800-809)
    const uint32_t fl = (flags & ~F_TB) | ((cog == 1 && !(flags & F_V5)) ? (uint32_t)F_TB : 0u);
    // the units are the groups: A = x's implicit-im2col rows, B = the group's [cog][Kg] weights
    CheckArgs c = check_args(x, w, y, Mrows, cog, Kg, E, Mw, bA, bW, 1, bR, fl, G, Cprod, stats);
    c.units = groups; c.conv = 1; c.sbk = 1; c.sbn = Kg;
    c.b_gs = cog * Kg; c.bb_gs = cog; c.cig = cig; c.cog = cog; c.ctot = Cout;
    c.Cin = Cin; c.H = H; c.W = W; c.Ho = Ho; c.Wo = Wo;
    c.kh = kh; c.kw = kw; c.sh = sh; c.sw = sw; c.ph = ph; c.pw = pw; c.dh = dh; c.dw = dw;
    return run_check(c, table, workspace, workspace_bytes, (hipStream_t)stream);
}

int fp8a_im2col(const float *x, float *out, int64_t Bn, int64_t Cin, int64_t H, int64_t W, int kh, int kw, int sh,
                int sw, int ph, int pw, int dh, int dw, fp8a_stream_t stream) {
    ConvShape c{Bn, Cin, H, W, Cin, kh, kw, sh, sw, ph, pw, dh, dw, 1};
    const int rc = conv_shape(c);
    if (rc) return rc;
    const int64_t Ho = c.Ho, Wo = c.Wo, total = c.Mrows * c.Kg;
    if (total == 0) return FP8A_OK;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 65536);
    im2col_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, out, Bn, Cin, H, W, kh, kw, sh, sw, ph, pw,
                                                                     dh, dw, Ho, Wo);
    return hip_check("fp8a_im2col");
}

size_t fp8a_conv2d_workspace_size(int64_t Bn, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int kh, int kw,
                                  int sh, int sw, int ph, int pw, int dh, int dw, int groups) {
    ConvShape c{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups};
    if (conv_shape(c)) return 0;
    // implicit GEMM (no im2col image): the off-grid flag word + split-K partials of one group
    const int64_t Mrows = c.Mrows, cog = c.cog, Kg = c.Kg;
    if (Mrows <= 0 || Kg <= 0) return FLAG_BYTES;
    // tensor-bias kernels: A words (+ the v5 depthwise form's B words)
    if (cog == 1) return FLAG_BYTES + align256((size_t)(Bn * Cin * H * W) * 4) + (size_t)(Cout * kh * kw) * 8;
    // A words: the zero-bordered word image of gemm_f8mx_kernel (xm_a_words)
    const WordImage wi = word_image(H, W, ph, pw);
    return gemm_workspace_bytes(Mrows, cog, Kg, Bn * (Cin / groups) * wi.H * wi.W);
}

int fp8a_conv2d(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                int64_t Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups, int E,
                int Mw, const int32_t *bA, const int32_t *bW, const int32_t *bR, const int32_t *table,
                uint32_t flags, void *workspace, size_t workspace_bytes, fp8a_stream_t stream) {
    return fp8a_conv2d_bn_act(x, w, y, Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, E, Mw, bA, bW, bR,
                              table, flags, nullptr, 0, 0.0f, 0.0f, workspace, workspace_bytes, stream);
}

// The convolution entry points.  fq.mx set: x is NOT yet quantized; the activation quantizer
// (fp8_quantizer.py:97-173, per tensor) is applied inside the matrix-core / tensor-bias-table
// pre-decodes (its bias written to fqb / fqi, which serve as bA), or -- for every other path --
// into xq (numel(x) floats) by one fake-quant pass first.

// A quantizer's bias (quantize_to_fp8_ste_MM's custom_bias) from its maxval, where no kernel of
// the launch family writes it.
__global__ void fq_bias_kernel(FqIn fq, float *bias_out, int32_t *ibias_out) {
    const float b = fq_bias(*fq.mx, fq.E, fq.M);
    *bias_out = b;
    *ibias_out = (int32_t)b;
}

// Non-fused input quantization: one fake-quant pass into xq, then the plain path on it.
static int materialize_input(ConvCall &c) {
    const int64_t nx = c.g.Bn * c.g.Cin * c.g.H * c.g.W;
    fp8_quantize_kernel<<<(unsigned)std::max<int64_t>(1, std::min<int64_t>((nx + 255) / 256, 65536)), 256, 0, c.s>>>(
        c.x, 1, nx, c.fq.mx, 0, c.fq.E, c.fq.M, c.fq.S, c.xq, c.fqb, c.fqi);
    c.x = c.xq;
    c.bA = c.fqi;
    c.fq.mx = nullptr;
    return hip_check("fp8a input fake-quant");
}

// The plan of the LDS-DMA-staged depthwise 3 x 3 kernels over the convolution's planes: plan_dw3's raw form,
// then the kernel's own LDS size (conv_tbsg_kernel: tbsg_lds_bytes; conv_v5ds_kernel: 8-byte tap words).
static bool plan_staged_dw(DwArgs &d, const ConvShape &g, int stride, bool tbsg, size_t &lds) {
    if (g.H >= (1 << 20) || g.W >= (1 << 20) || g.Cout >= (1 << 20) || g.H * g.W >= (1ll << 22)) return false;
    d.planes = g.Bn * g.Cout; d.C = (int)g.Cout; d.H = (int)g.H; d.W = (int)g.W;
    d.Ho = (int)g.Ho; d.Wo = (int)g.Wo; d.ph = g.ph; d.pw = g.pw; d.nx = g.Bn * g.Cin * g.H * g.W;
    if (!plan_dw3(d, stride, lds, true, tbsg ? tbsg_tap_bytes() : 4)) return false;
    lds = tbsg ? tbsg_lds_bytes(d.PB, d.nimg) : (size_t)d.nimg * 4 + (size_t)d.PB * 9 * 8;
    return lds <= 65536;
}

static TbxArgs tbx_args(const ConvShape &g, int64_t nwg, int64_t items) {
    TbxArgs ta;
    ta.Cin = g.Cin; ta.H = g.H; ta.W = g.W; ta.Cout = g.Cout; ta.Ho = g.Ho; ta.Wo = g.Wo;
    ta.kh = g.kh; ta.ph = g.ph; ta.pw = g.pw; ta.dh = g.dh; ta.cpg = (int)g.cig;
    ta.nwg = (uint32_t)nwg;
    ta.items = (uint32_t)items;
    return ta;
}

// The (stride, Mw[, rows per thread]) instances of the table-form depthwise kernels (conv_tbx.h), one launch
// macro per kernel family; they name conv_tensor_bias's locals.
#define FP8A_TBSG(S_, M_) conv_tbsg_kernel<S_, M_><<<gb, 256, glds, s>>>(x, w, y, dg, fq, fqb, fqi, bA, bW, bR, tp, gate, ep, act, act_lo, act_hi, emt)
#define FP8A_TBS(S_, M_) conv_tbs_kernel<S_, M_><<<gb, 256, tlds, s>>>(x, w, y, tb, fq, fqb, fqi, bA, bW, bR, tp, gate, ep, act, act_lo, act_hi)
#define FP8A_TBX(S_, M_) do { \
        if (rw2) conv_tbx_kernel<S_, M_, 2><<<gb, 256, 0, s>>>(aw, w, y, ta, bA, bW, bR, tp, gate, ep, act, act_lo, act_hi); \
        else conv_tbx_kernel<S_, M_, 1><<<gb, 256, 0, s>>>(aw, w, y, ta, bA, bW, bR, tp, gate, ep, act, act_lo, act_hi); \
    } while (0)
#define FP8A_BY_STRIDE_MW(LAUNCH_) do { \
        if (Mw == 2) { if (sw == 1) LAUNCH_(1, 2); else LAUNCH_(2, 2); } \
        else { if (sw == 1) LAUNCH_(1, 3); else LAUNCH_(2, 3); } \
    } while (0)

// Single-output-channel groups of the v9 model: the tensor-bias semantics (approx_calculation.py:800-809) on
// the table-form depthwise kernels, the general fast kernel, and the gated literal kernel behind them.
static int conv_tensor_bias(ConvCall &c) {
    const ConvShape &g = c.g;
    const int64_t Bn = g.Bn, Cin = g.Cin, H = g.H, W = g.W, Cout = g.Cout, Ho = g.Ho, Wo = g.Wo, cig = g.cig;
    const int kh = g.kh, kw = g.kw, sh = g.sh, sw = g.sw, ph = g.ph, pw = g.pw, dh = g.dh, dw = g.dw, groups = g.groups;
    const int E = c.E, Mw = c.Mw, act = c.act;
    const uint32_t flags = c.flags;
    const float act_lo = c.act_lo, act_hi = c.act_hi, *w = c.w;
    float *y = c.y, *fqb = c.fqb;
    int32_t *fqi = c.fqi;
    const int32_t *bW = c.bW, *bR = c.bR;
    const float2 *ep = reinterpret_cast<const float2 *>(c.bn);
    void *workspace = c.workspace;
    const size_t workspace_bytes = c.workspace_bytes;
    hipStream_t s = c.s;
    const EmitW &em = c.em;
    if (c.res || c.post_act || c.post_fq.mx)
        return fail(FP8A_EINVAL, "no block-output epilogue for single-output-channel groups");
    TablePack tp;
    int mode;
    int rc = pack_table(c.table, Mw, flags & F_APPROX, tp, mode);
    if (rc) return rc;
    const int64_t total = Bn * Cout * Ho * Wo;
    uint32_t *gate = nullptr;
    ArenaLease lease;  // (gate: a slot of the stream's flag arena, flag_arena)
    bool emitted = false;  // (a requested word image: only the staged table-form kernel writes it)
    // fast form: needs s2n on and golden_clip_OF off (else every launch would fall back)
    const bool fast_ok = (flags & F_S2N) && !(flags & F_GCLIP) && workspace != nullptr &&
                         workspace_bytes >= FLAG_BYTES && Cout <= 65535 && Bn <= 65535;
    // E4M3 / E5M2 table form (conv_tbx.h): a table of xm_table_form, qbma, 3-wide kernel rows, stride 1 or 2
    const int64_t nwg = (Wo + TBX_TW - 1) / TBX_TW, items = Bn * Cout * Ho * nwg;
    const bool tbx_ok = fast_ok && !g_env.no_tbx && ((E == 4 && Mw == 3) || (E == 5 && Mw == 2)) &&
                        xm_table_form(tp, Mw, nullptr) &&
                        (flags & F_QBMA) && kw == 3 && dw == 1 && sh == sw && (sw == 1 || sw == 2) &&
                        items < (1ll << 31) && Ho * Wo < (1ll << 31) &&
                        workspace_bytes >= FLAG_BYTES + (size_t)(Bn * Cin * H * W) * 4;
    if (c.fq.mx && !tbx_ok) {
        rc = materialize_input(c);
        if (rc) return rc;
    }
    const float *x = c.x;
    const int32_t *bA = c.bA;
    const FqIn fq = c.fq;
    if (tbx_ok) {
        if (!dw_lease(s, workspace, workspace_bytes, lease)) return lease_error();
        gate = lease.mine;
        // the input's table-form words from the producing launch (fp8a_conv2d_chain, next_form 1:
        // header + [Bn][Cin][H][W] words of fq_in(x)); the pre-pass then runs gated on its header
        const bool use_img = c.in_img != nullptr && fq.mx != nullptr;
        uint32_t *aw = use_img ? const_cast<uint32_t *>(c.in_img) + 64 : (uint32_t *)((char *)workspace + FLAG_BYTES);
        TbsArgs tb{};
        size_t tlds = 0;
        // tbs = 2 (default): the LDS-DMA-staged conv_tbsg_kernel
        DwArgs dg{};
        size_t glds = 0;
        const bool staged = !use_img && cig == 1 && kh == 3 && dh == 1;
        if (opt(OPT_TBS) == 2 && staged && plan_staged_dw(dg, g, sw, true, glds)) {
            const unsigned gb = (unsigned)(((dg.planes + dg.PB - 1) / dg.PB) * dg.nb);
            // (it emits the next matrix-core convolution's words when fp8a_conv2d_chain asked, em.form 0)
            const EmitW emt = em.w && em.form == 0 ? em : EmitW{};
            emitted = emt.w != nullptr;
            FP8A_BY_STRIDE_MW(FP8A_TBSG);
            if (fq.mx) bA = fqi;
            rc = hip_check("fp8a_conv2d (tensor-bias groups, LDS-DMA staged table form)");
            if (rc) return rc;
        } else if (opt(OPT_TBS) && staged && plan_tbs(tb, sw, Bn * Cout, Cout, H, W, Ho, Wo, ph, pw, tlds)) {
            const unsigned gb = (unsigned)(((tb.planes + tb.PB - 1) / tb.PB) * tb.nb);
            FP8A_BY_STRIDE_MW(FP8A_TBS);
            if (fq.mx) bA = fqi;
            rc = hip_check("fp8a_conv2d (tensor-bias groups, staged table form)");
            if (rc) return rc;
        } else {
            const int64_t nx = Bn * Cin * H * W;
            tbx_decode_a<<<(unsigned)std::min<int64_t>((nx + 255) / 256, use_img ? 1024 : 8192), 256, 0, s>>>(
                x, nx, aw, gate, fq, fqb, fqi, Mw, use_img ? c.in_img : nullptr);
            if (fq.mx) bA = fqi;
            const bool rw2 = opt(OPT_TBX_RW) == 2 && dh == 1;
            const TbxArgs ta = tbx_args(g, nwg, rw2 ? Bn * Cout * ((Ho + 1) / 2) * nwg : items);
            const unsigned gb = (unsigned)std::min<int64_t>((ta.items + 255) / 256, 8 * 1024);
            FP8A_BY_STRIDE_MW(FP8A_TBX);
            rc = hip_check("fp8a_conv2d (tensor-bias groups, E4M3 / E5M2 table form)");
            if (rc) return rc;
        }
    } else if (fast_ok) {
        if (!dw_lease(s, workspace, workspace_bytes, lease)) return lease_error();
        gate = lease.mine;
        dim3 grid((unsigned)((Ho * Wo + 255) / 256), (unsigned)Cout, (unsigned)Bn);
        conv_tb_fast_kernel<<<grid, 256, 0, s>>>(x, w, y, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups,
                                                 Ho, Wo, Mw, bA, bW, bR, tp, flags | F_TB, gate, ep, act, act_lo,
                                                 act_hi);
        rc = hip_check("fp8a_conv2d (tensor-bias groups, fast)");
        if (rc) return rc;
    }
    // (gated: at most 1024 blocks -- a no-op launch unless the fast kernel flagged)
    const unsigned eb = (unsigned)(fast_ok ? std::min<int64_t>((total + 255) / 256, 1024) : (total + 255) / 256);
    if (fast_ok) {  // gated, grid-capped: a no-op launch unless the fast kernel flagged
        conv_tb_direct_kernel<true><<<std::max(eb, clear_blocks(lease)), 256, 0, s>>>(
            x, w, y, Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, Ho, Wo, E, Mw, bA, bW, bR, tp,
            flags | F_TB, gate, (uint32_t *)workspace, lease.clr, lease.clr16, ep, act, act_lo, act_hi, fq);
    } else {
        conv_tb_direct_kernel<true><<<eb, 256, 0, s>>>(x, w, y, Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw,
                                                 groups, Ho, Wo, E, Mw, bA, bW, bR, tp, flags | F_TB, nullptr,
                                                 nullptr, nullptr, 0u, ep, act, act_lo, act_hi, FqIn{});
    }
    if (em.w && !emitted && (rc = invalidate_image(em, s))) return rc;  // (no emission here)
    return hip_check("fp8a_conv2d (tensor-bias groups)");
}

// v5 depthwise: one direct launch (a GEMM per single-column group would be `groups` launches of N = 1
// tiles: MobileNetV2 E5M2 v5 ran at ~500 images/s that way) -- the staged kernel, the word form, or
// the literal kernel alone.
static int conv_v5_depthwise(ConvCall &c) {
    const ConvShape &g = c.g;
    const int64_t Bn = g.Bn, Cin = g.Cin, H = g.H, W = g.W, Cout = g.Cout, Ho = g.Ho, Wo = g.Wo, cig = g.cig;
    const int kh = g.kh, kw = g.kw, sh = g.sh, sw = g.sw, ph = g.ph, pw = g.pw, dh = g.dh, dw = g.dw, groups = g.groups;
    const int E = c.E, Mw = c.Mw, act = c.act;
    const uint32_t flags = c.flags;
    const float act_lo = c.act_lo, act_hi = c.act_hi, *x = c.x, *w = c.w;
    float *y = c.y, *fqb = c.fqb;
    int32_t *fqi = c.fqi;
    const int32_t *bA = c.bA, *bW = c.bW, *bR = c.bR;
    const float2 *ep = reinterpret_cast<const float2 *>(c.bn);
    void *workspace = c.workspace;
    const size_t workspace_bytes = c.workspace_bytes;
    hipStream_t s = c.s;
    const FqIn fq = c.fq;
    const EmitW &em = c.em;
    TablePack tp;
    int mode;
    int rc = pack_table(c.table, Mw, true, tp, mode);
    if (rc) return rc;
    const int64_t total = Bn * Cout * Ho * Wo;
    // the word form (conv_v5dw_kernel, conv_tbx.h): E5M2 with the adder wrap, depthwise 3-wide
    // rows, stride 1 / 2; the literal kernel behind it runs only if its gate is raised
    const int64_t nx = Bn * Cin * H * W, nwg = (Wo + TBX_TW - 1) / TBX_TW, items = Bn * Cout * Ho * nwg;
    const size_t awb = align256((size_t)nx * 4);
    const bool v5dw_ok = !g_env.no_v5dw && Mw == 2 && (flags & F_OFUF) && cig == 1 && kw == 3 && kh <= 5 && dw == 1 &&
                         sh == sw && (sw == 1 || sw == 2) && items < (1ll << 31) && Ho * Wo < (1ll << 31) &&
                         workspace != nullptr && workspace_bytes >= FLAG_BYTES + awb + (size_t)(Cout * kh * kw) * 8;
    uint32_t *gate = nullptr;
    ArenaLease lease;  // (gate: a slot of the stream's flag arena, flag_arena)
    // the staged form (conv_v5ds_kernel: both pre-passes fused): depthwise 3 x 3, dilation 1
    DwArgs d{};
    size_t lds = 0;
    if (v5dw_ok && opt(OPT_V5DS) && kh == 3 && kw == 3 && dh == 1 && plan_staged_dw(d, g, sh, false, lds)) {
        if (!dw_lease(s, workspace, workspace_bytes, lease)) return lease_error();
        gate = lease.mine;
        const unsigned gb = (unsigned)(((d.planes + d.PB - 1) / d.PB) * d.nb);
        // (it emits the next convolution's v5 words when fp8a_conv2d_chain asked for them, em.form 2)
        const EmitW emv = em.w && em.form == 2 ? em : EmitW{};
        if (sh == 1)
            conv_v5ds_kernel<1><<<gb, 256, lds, s>>>(x, w, y, d, fq, fqb, fqi, bA, bW, bR, tp, flags, E, gate, ep,
                                                     act, act_lo, act_hi, emv);
        else
            conv_v5ds_kernel<2><<<gb, 256, lds, s>>>(x, w, y, d, fq, fqb, fqi, bA, bW, bR, tp, flags, E, gate, ep,
                                                     act, act_lo, act_hi, emv);
        rc = hip_check("fp8a_conv2d (v5 depthwise, staged)");
        if (rc) return rc;
        if (fq.mx) bA = fqi;
        ++g_paths[PATH_FAST];
    } else if (v5dw_ok) {
        if (em.w && (rc = invalidate_image(em, s))) return rc;  // (no emission here)
        if (!dw_lease(s, workspace, workspace_bytes, lease)) return lease_error();
        gate = lease.mine;
        uint32_t *aw = (uint32_t *)((char *)workspace + FLAG_BYTES);
        uint2 *bwd = (uint2 *)((char *)workspace + FLAG_BYTES + awb);
        // (the input quantizer applied here, its bias written for the kernels after: bA = fqi)
        v5dw_decode_a<<<(unsigned)std::min<int64_t>((nx + 255) / 256, 8192), 256, 0, s>>>(x, nx, aw, E, Mw, bA, fq,
                                                                                           fqb, fqi);
        if (fq.mx) bA = fqi;
        const int64_t nb = Cout * kh * kw;
        v5dw_decode_b<<<(unsigned)std::min<int64_t>((nb + 255) / 256, 1024), 256, 0, s>>>(w, nb, kh * kw, bwd, E, Mw,
                                                                                           bA, bW, bR, tp);
        const TbxArgs ta = tbx_args(g, nwg, items);
        const unsigned gb = (unsigned)std::min<int64_t>((items + 255) / 256, 8 * 1024);
        if (sw == 1)
            conv_v5dw_kernel<1><<<gb, 256, 0, s>>>(aw, bwd, y, ta, bR, flags, E, gate, ep, act, act_lo, act_hi);
        else
            conv_v5dw_kernel<2><<<gb, 256, 0, s>>>(aw, bwd, y, ta, bR, flags, E, gate, ep, act, act_lo, act_hi);
        rc = hip_check("fp8a_conv2d (v5 depthwise, word form)");
        if (rc) return rc;
        ++g_paths[PATH_FAST];
    } else {
        ++g_paths[PATH_EXACT];
        if (em.w && (rc = invalidate_image(em, s))) return rc;  // (no emission here)
        if (fq.mx) {
            fq_bias_kernel<<<1, 1, 0, s>>>(fq, fqb, fqi);
            bA = fqi;
        }
    }
    // (x unquantized when fq is set: the literal kernel applies fq to every loaded value)
    conv_tb_direct_kernel<false><<<std::max((unsigned)std::min<int64_t>((total + 255) / 256, 16384),
                                            clear_blocks(lease)), 256, 0, s>>>(
        x, w, y, Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups, Ho, Wo, E, Mw, bA, bW, bR, tp, flags,
        gate, gate ? (uint32_t *)workspace : nullptr, lease.clr, lease.clr16, ep, act, act_lo, act_hi, fq);
    return hip_check("fp8a_conv2d (v5 depthwise, direct)");
}

// Every other convolution: one implicit GEMM (run_gemm) per group.
static int conv_grouped_gemm(const ConvCall &c) {
    const ConvShape &g = c.g;
    for (int gi = 0; gi < g.groups; ++gi) {
        GemmArgs a = make_args(nullptr, 0, c.w + gi * g.cog * g.Kg, 1, g.Kg, c.y, 0, g.Mrows, g.cog, g.Kg, c.E, c.Mw, c.bA,
                               c.bW + gi * g.cog, 1, c.bR, c.flags & ~F_TB);
        a.nchw = 1;
        a.hw = g.Ho * g.Wo;
        a.ctot = g.Cout;
        a.coff = gi * g.cog;
        a.conv = 1;
        a.X = c.x;
        a.Cin = g.Cin; a.H = g.H; a.W = g.W; a.Ho = g.Ho; a.Wo = g.Wo; a.cbase = gi * g.cig; a.aw_c = g.cig;
        a.kh = g.kh; a.kw = g.kw; a.sh = g.sh; a.sw = g.sw; a.ph = g.ph; a.pw = g.pw; a.dh = g.dh; a.dw = g.dw;
        fastdiv_params((uint32_t)(g.kh * g.kw), a.kk_mul, a.kk_shift);
        fastdiv_params((uint32_t)g.kw, a.kw_mul, a.kw_shift);
        a.ep = reinterpret_cast<const float2 *>(c.bn); a.ep_act = c.act; a.ep_lo = c.act_lo; a.ep_hi = c.act_hi;
        if (c.fq.mx) {
            a.fqin = c.fq;
            a.fq_bias = c.fqb;
            a.fq_ibias = c.fqi;
            a.bA = c.fqi;  // written by the A pre-decode before any kernel reads it
        }
        a.res = c.res; a.post_act = c.post_act; a.post_lo = c.post_lo; a.post_hi = c.post_hi; a.post_fq = c.post_fq;
        a.post_bout = c.post_bout; a.post_ibout = c.post_ibout;
        if (g.groups == 1) {  // (fp8a_conv2d_chain only asks for these on ungrouped convolutions)
            a.in_img = c.in_img;
            a.em = c.em;
        }
        const int rc = run_gemm(a, c.table, c.workspace, c.workspace_bytes, c.s);
        if (rc) return rc;
    }
    return FP8A_OK;
}

// The common prologue of every convolution entry point, then one of the three dispatchers above.
static int conv2d_impl(const ConvCall &call) {
    ConvCall c = call;  // (materialize_input and the word-image checks rewrite x, bA, fq and em)
    ConvShape &g = c.g;
    if (c.bn && (((uintptr_t)c.bn) & 7) != 0) return fail(FP8A_EINVAL, "bn parameters must be 8-byte aligned");
    int rc = check_format(c.E, c.Mw);
    if (!rc) rc = conv_shape(g);
    if (rc) return rc;
    if (g.Mrows == 0) {  // (the output quantizer's bias is still set, as its forward would)
        if (c.post_bout) fq_bias_kernel<<<1, 1, 0, c.s>>>(c.post_fq, c.post_bout, c.post_ibout);
        return c.post_bout ? hip_check("fp8a output-quantizer bias") : FP8A_OK;
    }
    const bool post = c.res || c.post_act || c.post_fq.mx;
    const bool v5_depthwise = (c.flags & F_V5) && g.cog == 1 && !post && g.groups > 1;
    // v5 words (form 2) come from the staged v5 depthwise kernel only: any other launch flags them invalid
    if (c.em.w && (c.em.form == 2) != v5_depthwise) {
        if ((rc = invalidate_image(c.em, c.s))) return rc;
        c.em = EmitW{};
    }
    if (c.res && (c.res == c.y || (((uintptr_t)c.res) & 15) != 0))
        return fail(FP8A_EINVAL, "the residual must be a 16-byte aligned tensor other than the output");
    // v5 never had tensor-bias semantics: its single-output-channel groups take the paths below
    if (g.cog == 1 && !(c.flags & F_V5)) return conv_tensor_bias(c);
    // (a workspace below fp8a_conv2d_workspace_size but holding the flag word runs unsplit)
    if (c.workspace == nullptr || c.workspace_bytes < FLAG_BYTES)
        return fail(FP8A_EINVAL, "conv2d workspace too small");
    if (g.Kg >= (1ll << 31)) return fail(FP8A_EINVAL, "conv2d window too large");
    if (c.fq.mx) {  // fuse into the matrix-core pre-decode only where run_gemm will take that path
        TablePack tp;
        int mode;
        rc = pack_table(c.table, c.Mw, (c.flags & (F_APPROX | F_V5)) != 0, tp, mode);
        if (rc) return rc;
        if (c.flags & F_V5) mode = TM_V5;  // (as run_gemm)
        const WordImage wi = word_image(g.H, g.W, g.ph, g.pw);
        const int64_t a_words = g.Bn * g.cig * wi.H * wi.W;  // as xm_a_words / run_gemm
        const MxPlan mx = mx_plan(c.E, c.Mw, c.flags & ~F_TB, tp, mode, g.Mrows, g.cog, g.Kg, a_words);
        // every matrix-core form applies fq in its A pre-decode (xm_decode_a), so the convolution fuses for all
        // three; the workspace test is the conservative one (the whole size query), where run_gemm's is exact
        const bool fused = mx.any() && mx.fits32 &&
                           c.workspace_bytes >= gemm_workspace_bytes(g.Mrows, g.cog, g.Kg, a_words);
        if (!fused) {
            rc = materialize_input(c);
            if (rc) return rc;
        }
    }
    return v5_depthwise ? conv_v5_depthwise(c) : conv_grouped_gemm(c);
}

// The fields every convolution entry point has, in the public argument order.
static ConvCall conv_call(const float *x, const float *w, float *y, const ConvShape &g, int E, int Mw, const int32_t *bA,
                          const int32_t *bW, const int32_t *bR, const int32_t *table, uint32_t flags, const float *bn,
                          int act, float act_lo, float act_hi, void *workspace, size_t workspace_bytes,
                          fp8a_stream_t stream) {
    ConvCall c{};
    c.g = g;
    c.x = x; c.w = w; c.y = y; c.E = E; c.Mw = Mw; c.bA = bA; c.bW = bW; c.bR = bR; c.table = table; c.flags = flags;
    c.bn = bn; c.act = act; c.act_lo = act_lo; c.act_hi = act_hi;
    c.workspace = workspace; c.workspace_bytes = workspace_bytes; c.s = (hipStream_t)stream;
    return c;
}

int fp8a_conv2d_bn_act(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                       int64_t Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups,
                       int E, int Mw, const int32_t *bA, const int32_t *bW, const int32_t *bR, const int32_t *table,
                       uint32_t flags, const float *bn, int act, float act_lo, float act_hi, void *workspace,
                       size_t workspace_bytes, fp8a_stream_t stream) {
    return conv2d_impl(conv_call(x, w, y, ConvShape{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups}, E, Mw, bA,
                                 bW, bR, table, flags, bn, act, act_lo, act_hi, workspace, workspace_bytes, stream));
}

size_t fp8a_conv2d_qin_workspace_size(int64_t Bn, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int kh, int kw,
                                      int sh, int sw, int ph, int pw, int dh, int dw, int groups) {
    const size_t n = fp8a_conv2d_workspace_size(Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups);
    return n == 0 ? 0 : align256(n) + align256((size_t)(Bn * Cin * H * W) * sizeof(float));
}

int fp8a_conv2d_qin(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                    int64_t Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups, int E,
                    int Mw, const int32_t *bW, const int32_t *bR, const int32_t *table, uint32_t flags,
                    const float *bn, int act, float act_lo, float act_hi, const float *in_maxval, int in_nbits,
                    int in_mbits, int in_sign_bits, float *in_bias_out, int32_t *in_ibias_out, void *workspace,
                    size_t workspace_bytes, fp8a_stream_t stream) {
    if (!in_maxval || !in_bias_out || !in_ibias_out) return fail(FP8A_EINVAL, "null pointer");
    ConvCall c = conv_call(x, w, y, ConvShape{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups}, E, Mw, nullptr,
                           bW, bR, table, flags, bn, act, act_lo, act_hi, workspace, workspace_bytes, stream);
    int rc = fused_quantizer(in_maxval, in_nbits, in_mbits, in_sign_bits, in_bias_out, in_ibias_out, c.fq);
    if (!rc) rc = carve_xq(workspace, workspace_bytes, Bn * Cin * H * W, "conv2d_qin", c.workspace_bytes, c.xq);
    if (rc) return rc;
    c.fqb = in_bias_out;
    c.fqi = in_ibias_out;
    return conv2d_impl(c);
}

size_t fp8a_conv2d_block_workspace_size(int64_t Bn, int64_t Cin, int64_t H, int64_t W, int64_t Cout, int kh,
                                        int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups) {
    return fp8a_conv2d_qin_workspace_size(Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups);
}

// ----------------------------------------------------------------------------- word-image chain
// A convolution's input as the zero-bordered word image of gemm_f8mx_kernel (xm_decode_a's
// layout: [Bn][C][H + 2 ph][W'] with the left border widened for 16-B interior rows), behind a
// 256-B header whose first word is the "invalid" flag (fp8a_conv2d_chain).
size_t fp8a_word_image_bytes(int64_t Bn, int64_t C, int64_t H, int64_t W, int ph, int pw) {
    if (Bn <= 0 || C <= 0 || H <= 0 || W <= 0 || ph < 0 || pw < 0) return 0;
    const WordImage wi = word_image(H, W, ph, pw);
    return FLAG_BYTES + align256((size_t)(Bn * C * wi.H * wi.W) * 4);
}

// The emitting launch's header: [0] valid, [1] the next quantizer's maxval, [2] its float bias,
// [3] its 2^(1 - bias) bit pattern (the grid's min normal), [4] the next convolution's bR; [5] and
// [6] are cleared here and collected by the producers (the words' scale-exponent extreme, and
// "a negative word was emitted": fp8approx_common.h wave_sign_record).
__global__ void emit_prep_kernel(uint32_t *hdr, FqIn fq, const int32_t *bR) {
    const float mx = *fq.mx, fb = fq_bias(mx, fq.E, fq.M);
    hdr[0] = 0u;
    hdr[1] = __float_as_uint(mx);
    hdr[2] = __float_as_uint(fb);
    hdr[3] = (uint32_t)(128 - (int)fb) << 23;
    hdr[4] = (uint32_t)*bR;
    hdr[5] = 0u;  // 255 - the smallest scale exponent of the emitted nonzero words (wave_max_atomic)
    hdr[6] = 0u;  // nonzero: a word with the sign row bit was emitted (wave_sign_record)
}

__global__ void word_image_fill_kernel(uint32_t *img, int64_t words) {
    if (blockIdx.x == 0 && threadIdx.x < 64) img[threadIdx.x] = 0u;  // header: valid
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x)
        img[64 + i] = XM_ZERO_WORD;  // the word of a zero (the border stays so)
}

int fp8a_word_image_init(void *image, int64_t Bn, int64_t C, int64_t H, int64_t W, int ph, int pw,
                         fp8a_stream_t stream) {
    if (image == nullptr || fp8a_word_image_bytes(Bn, C, H, W, ph, pw) == 0) return fail(FP8A_EINVAL, "word image");
    if (((uintptr_t)image & 255) != 0) return fail(FP8A_EINVAL, "word image must be 256-byte aligned");
    const WordImage wi = word_image(H, W, ph, pw);
    // (every word of fp8a_word_image_bytes, the 256-byte rounding's tail included: no kernel reads it, but
    // a caller that compares or copies whole images then sees defined bytes)
    const int64_t words = (int64_t)(align256((size_t)(Bn * C * wi.H * wi.W) * 4) / 4);
    word_image_fill_kernel<<<(unsigned)std::min<int64_t>((words + 255) / 256, 8192), 256, 0, (hipStream_t)stream>>>(
        (uint32_t *)image, words);
    return hip_check("fp8a word image init");
}

// Whether a convolution would read an in_image (fp8a_conv2d_chain): the matrix-core path with its A
// pre-pass (not the fp32-staging form of 1x1 convolutions with few column tiles, not the tile-table
// or VALU kernels), ungrouped, more than one output channel, a fused input quantizer.
int fp8a_conv2d_wants_image(int64_t Cout, int kh, int kw, int ph, int pw, int groups, int E, int Mw,
                            const int32_t *table, uint32_t flags, int sh, int sw, int dh, int dw) {
    if (Cout <= 1 || check_format(E, Mw) != FP8A_OK) return 0;
    TablePack tp;
    int mode;
    if (pack_table(table, Mw, (flags & F_APPROX) != 0, tp, mode) != FP8A_OK) return 0;
    if (groups > 1 && Cout == groups) {  // single-output-channel groups: the table form's words
        // opt-in (FP8A_CHAIN_TBX=1): measured on MobileNetV2 E4M3 the producers' emitting stores cost
        // 1.65 ms per forward for 0.85 ms of gated pre-passes saved (19708 -> 19036 images/s)
        const bool tbx = g_env.chain_tbx && !g_env.no_tbx && ((E == 4 && Mw == 3) || (E == 5 && Mw == 2)) &&
                         xm_table_form(tp, Mw, nullptr) && (flags & F_S2N) && (flags & F_QBMA) &&
                         !(flags & (F_GCLIP | F_V5)) && kw == 3 && dw == 1 && sh == sw && (sw == 1 || sw == 2);
        (void)kh; (void)dh;
        return tbx ? 2 : 0;
    }
    // (the forms only: the shape-dependent part of run_gemm's decision -- offsets, workspace -- is not known here)
    const MxPlan mx = mx_plan(E, Mw, flags & ~F_TB, tp, (flags & F_V5) ? TM_V5 : mode, 0, Cout, 0, 0);
    if (groups != 1 || !mx.on) return 0;
    // the v5 matrix-core form (gemm_v5mx_kernel): its words (v5_word_a) when unpadded (an image's
    // border holds the E4M3 / E5M2 form's zero word, fp8a_word_image_init); emitted by the staged
    // v5 depthwise kernel only (conv_v5ds_kernel) -- every other producer flags the image invalid
    if (flags & F_V5) return (mx.v5mx && ph == 0 && pw == 0) ? 3 : 0;
    if (!mx.f8) return 0;
    if (kh == 1 && kw == 1 && ph == 0 && pw == 0) {  // xm_af32: fp32 staging up to af32_maxct column tiles
        const int64_t bnt = 16 * xm_ncg(Cout), ct = (Cout + bnt - 1) / bnt;
        if (ct <= af32_maxct(sh, sw)) return 0;
    }
    return 1;
}

// fp8a_conv2d_chain's word-image arguments (fp8a_conv2d_block: none).
struct ChainArgs {
    void *in_image, *out_image;
    int next_ph, next_pw;
    const float *next_maxval;
    int next_nbits, next_mbits, next_sign_bits;
    const int32_t *next_bR;
    int next_Mw, next_form;
};

// The header of the word image this launch may emit (valid with the next quantizer's constants, or invalid
// where it cannot emit) and the producers' EmitW.
static int emit_setup(const ConvCall &c, const ChainArgs &n, EmitW &em) {
    ConvShape g = c.g;
    const bool shape_ok = conv_shape(g) == FP8A_OK;  // (a bad shape: conv2d_impl reports it)
    const int qE = n.next_nbits - n.next_sign_bits - n.next_mbits;
    if (!n.next_maxval || !n.next_bR || n.next_mbits < 1 || qE < 1 || !(n.next_Mw == 2 || n.next_Mw == 3) ||
        n.next_ph < 0 || n.next_pw < 0)
        return fail(FP8A_EINVAL, "bad next-convolution parameters for the word image");
    if (n.next_form < 0 || n.next_form > 2) return fail(FP8A_EINVAL, "bad word image form");
    // (the table form's words: the consumer's plain [Bn][C][Ho][Wo] layout, no border)
    const WordImage wi = n.next_form == 1 ? word_image(g.Ho, g.Wo, 0, 0) : word_image(g.Ho, g.Wo, n.next_ph, n.next_pw);
    // (form 2, v5 words: the staged v5 depthwise producer -- conv2d_impl flags the image invalid
    // where that kernel does not run; form 0 / 1: ungrouped producers)
    // (form 0 from a depthwise producer: the staged table-form kernel, round 6)
    const bool dwp = g.groups > 1 && g.Cin == g.groups && g.Cout == g.groups;
    const bool prod = n.next_form == 2 ? (c.flags & F_V5) && dwp
                                       : g.groups == 1 || (n.next_form == 0 && dwp && !(c.flags & F_V5));
    const bool can = prod && g.Cout > 1 && shape_ok && g.Bn * g.Cout * g.Ho * g.Wo < (1ll << 31) &&
                     g.Bn * g.Cout * wi.H * wi.W < (1ll << 30);
    if (!can)
        return dev_fill(n.out_image, 1, sizeof(uint32_t), c.s) != hipSuccess ? hip_check("fp8a word image header") : FP8A_OK;
    const FqIn next_fq{n.next_maxval, qE, n.next_mbits, n.next_sign_bits};
    emit_prep_kernel<<<1, 1, 0, c.s>>>((uint32_t *)n.out_image, next_fq, n.next_bR);
    em.w = (uint32_t *)n.out_image + 64;
    em.invalid = (uint32_t *)n.out_image;
    em.awH = (int)wi.H; em.awW = (int)wi.W; em.awph = wi.ph; em.awpw = wi.pw;
    em.Wo = (int)g.Wo;
    em.hw = (uint32_t)(g.Ho * g.Wo);
    fastdiv_params(em.hw, em.hw_mul, em.hw_shift);
    fastdiv_params((uint32_t)g.Wo, em.wo_mul, em.wo_shift);
    em.fq = next_fq;
    em.bR = n.next_bR;
    em.Mw = n.next_Mw;
    em.form = n.next_form;
    return FP8A_OK;
}

// fp8a_conv2d_block and fp8a_conv2d_chain (name: the entry point's, for its messages): c holds the plain call,
// the residual and the post clamp; the quantizers, the word images and the fake-quant buffer are added here.
static int conv_block(const char *name, ConvCall c, const float *in_maxval, int in_nbits, int in_mbits,
                      int in_sign_bits, float *in_bias_out, int32_t *in_ibias_out, const float *out_maxval, int out_nbits,
                      int out_mbits, int out_sign_bits, float *out_bias_out, int32_t *out_ibias_out, const ChainArgs &n) {
    if (c.post_act != 0 && c.post_act != 1) return fail(FP8A_EINVAL, std::string(name) + ": post_act is 0 or 1");
    if ((n.in_image && ((uintptr_t)n.in_image & 255)) || (n.out_image && ((uintptr_t)n.out_image & 255)))
        return fail(FP8A_EINVAL, "word images must be 256-byte aligned");
    int rc = fused_quantizer(in_maxval, in_nbits, in_mbits, in_sign_bits, in_bias_out, in_ibias_out, c.fq);
    if (rc) return rc;
    if (!c.fq.mx && !c.bA) return fail(FP8A_EINVAL, "null pointer");
    // (the output quantizer's bias: written by the launch's gated exact kernel)
    rc = fused_quantizer(out_maxval, out_nbits, out_mbits, out_sign_bits, out_bias_out, out_ibias_out, c.post_fq);
    if (!rc && n.out_image) rc = emit_setup(c, n, c.em);
    if (!rc) rc = carve_xq(c.workspace, c.workspace_bytes, c.fq.mx ? c.g.Bn * c.g.Cin * c.g.H * c.g.W : -1, name,
                           c.workspace_bytes, c.xq);
    if (rc) return rc;
    if (c.fq.mx) c.bA = nullptr;
    c.fqb = in_bias_out;
    c.fqi = in_ibias_out;
    c.post_bout = c.post_fq.mx ? out_bias_out : nullptr;
    c.post_ibout = c.post_fq.mx ? out_ibias_out : nullptr;
    c.in_img = (const uint32_t *)n.in_image;
    return conv2d_impl(c);
}

int fp8a_conv2d_block(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                      int64_t Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups, int E,
                      int Mw, const int32_t *bA, const int32_t *bW, const int32_t *bR, const int32_t *table,
                      uint32_t flags, const float *bn, int act, float act_lo, float act_hi, const float *in_maxval,
                      int in_nbits, int in_mbits, int in_sign_bits, float *in_bias_out, int32_t *in_ibias_out,
                      const float *res, int post_act, float post_lo, float post_hi, const float *out_maxval,
                      int out_nbits, int out_mbits, int out_sign_bits, float *out_bias_out, int32_t *out_ibias_out,
                      void *workspace, size_t workspace_bytes, fp8a_stream_t stream) {
    ConvCall c = conv_call(x, w, y, ConvShape{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups}, E, Mw, bA, bW,
                           bR, table, flags, bn, act, act_lo, act_hi, workspace, workspace_bytes, stream);
    c.res = res; c.post_act = post_act; c.post_lo = post_lo; c.post_hi = post_hi;
    return conv_block("conv2d_block", c, in_maxval, in_nbits, in_mbits, in_sign_bits, in_bias_out, in_ibias_out,
                      out_maxval, out_nbits, out_mbits, out_sign_bits, out_bias_out, out_ibias_out, ChainArgs{});
}

int fp8a_conv2d_chain(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                      int64_t Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups, int E,
                      int Mw, const int32_t *bA, const int32_t *bW, const int32_t *bR, const int32_t *table,
                      uint32_t flags, const float *bn, int act, float act_lo, float act_hi, const float *in_maxval,
                      int in_nbits, int in_mbits, int in_sign_bits, float *in_bias_out, int32_t *in_ibias_out,
                      const float *res, int post_act, float post_lo, float post_hi, const float *out_maxval,
                      int out_nbits, int out_mbits, int out_sign_bits, float *out_bias_out, int32_t *out_ibias_out,
                      void *in_image, void *out_image, int next_ph, int next_pw, const float *next_maxval,
                      int next_nbits, int next_mbits, int next_sign_bits, const int32_t *next_bR, int next_Mw,
                      int next_form, void *workspace, size_t workspace_bytes, fp8a_stream_t stream) {
    ConvCall c = conv_call(x, w, y, ConvShape{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups}, E, Mw, bA, bW,
                           bR, table, flags, bn, act, act_lo, act_hi, workspace, workspace_bytes, stream);
    c.res = res; c.post_act = post_act; c.post_lo = post_lo; c.post_hi = post_hi;
    return conv_block("conv2d_chain", c, in_maxval, in_nbits, in_mbits, in_sign_bits, in_bias_out, in_ibias_out,
                      out_maxval, out_nbits, out_mbits, out_sign_bits, out_bias_out, out_ibias_out,
                      ChainArgs{in_image, out_image, next_ph, next_pw, next_maxval, next_nbits, next_mbits,
                                next_sign_bits, next_bR, next_Mw, next_form});
}

size_t fp8a_matmul_block_workspace_size(int64_t M, int64_t N, int64_t K) {
    const size_t n = fp8a_matmul_workspace_size_mnk(M, N, K);
    return n == 0 ? 0 : align256(n) + align256((size_t)(M * K) * sizeof(float));
}

// A linear layer with its neighbours fused (QCustomLinearTorch.run_forward + the callers'
// elementwise tails, vit_quantized_approx.py:117-156): C = fq_out(clamp(bn_act(fq_in(A) @ B) + res)).
// Same contract as fp8a_conv2d_block with the row-major matrix operands of fp8a_matmul; with
// in_maxval, A must be dense (lda == K).
int fp8a_matmul_block(const float *A, int64_t lda, const float *B, int64_t sbk, int64_t sbn, float *C, int64_t ldc,
                      int64_t M, int64_t N, int64_t K, int E, int Mw, const int32_t *bA, const int32_t *bB,
                      int64_t bB_stride, const int32_t *bR, const int32_t *table, uint32_t flags, const float *bn,
                      int act, float act_lo, float act_hi, const float *in_maxval, int in_nbits, int in_mbits,
                      int in_sign_bits, float *in_bias_out, int32_t *in_ibias_out, const float *res, int post_act,
                      float post_lo, float post_hi, const float *out_maxval, int out_nbits, int out_mbits,
                      int out_sign_bits, float *out_bias_out, int32_t *out_ibias_out, void *workspace,
                      size_t workspace_bytes, fp8a_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (lda < K || ldc < N) return fail(FP8A_EINVAL, "leading dimension smaller than extent");
    if (flags & (F_TB | F_V5)) return fail(FP8A_EINVAL, "matmul_block: int-bias v9 path only");
    if (post_act < 0 || post_act > 2) return fail(FP8A_EINVAL, "matmul_block: post_act is 0, 1 or 2");
    if (bn && (((uintptr_t)bn) & 7) != 0) return fail(FP8A_EINVAL, "bn parameters must be 8-byte aligned");
    if (res && (res == C || (((uintptr_t)res) & 15) != 0))
        return fail(FP8A_EINVAL, "the residual must be a 16-byte aligned tensor other than the output");
    FqIn fin, fout;
    int rc = fused_quantizer(in_maxval, in_nbits, in_mbits, in_sign_bits, in_bias_out, in_ibias_out, fin);
    if (rc) return rc;
    if (fin.mx && lda != K) return fail(FP8A_EINVAL, "matmul_block: fused input quantization needs a dense A");
    if (!fin.mx && !bA) return fail(FP8A_EINVAL, "null pointer");
    // (the output quantizer's bias: written by the launch's gated exact kernel)
    rc = fused_quantizer(out_maxval, out_nbits, out_mbits, out_sign_bits, out_bias_out, out_ibias_out, fout);
    size_t rest = 0;
    float *xq = nullptr;  // one fake-quant pass into the workspace's end where the quantizer is not fused
    if (!rc) rc = carve_xq(workspace, workspace_bytes, fin.mx ? M * K : -1, "matmul_block", rest, xq);
    if (rc) return rc;
    GemmArgs a = make_args(A, lda, B, sbk, sbn, C, ldc, M, N, K, E, Mw, fin.mx ? in_ibias_out : bA, bB, bB_stride, bR,
                           flags);
    a.ep = reinterpret_cast<const float2 *>(bn); a.ep_act = act; a.ep_lo = act_lo; a.ep_hi = act_hi;
    a.res = res; a.post_act = post_act; a.post_lo = post_lo; a.post_hi = post_hi; a.post_fq = fout;
    if (fout.mx) {
        a.post_bout = out_bias_out;
        a.post_ibout = out_ibias_out;
    }
    if (fin.mx && M > 0 && K > 0) {
        // fuse into the matrix-core pre-decode only where run_gemm will take that path
        TablePack tp;
        int mode;
        rc = check_format(E, Mw);
        if (!rc) rc = pack_table(table, Mw, (flags & F_APPROX) != 0, tp, mode);
        if (rc) return rc;
        const MxPlan mx = mx_plan(E, Mw, flags, tp, mode, M, N, K, M * ((K + BK - 1) / BK * BK));
        // the E4M3 / E5M2 form only (the linear layers' tile-table launches keep the separate fake-quant pass);
        // the conservative workspace test, as conv2d_impl
        const bool fused = mx.f8 && mx.on && mx.fits32 && rest >= gemm_workspace_bytes(M, N, K, 0);
        if (fused) {
            a.fqin = fin;
            a.fq_bias = in_bias_out;
            a.fq_ibias = in_ibias_out;  // written by the A pre-decode before any kernel reads it
        } else {
            const int64_t nx = M * K;
            fp8_quantize_kernel<<<(unsigned)std::max<int64_t>(1, std::min<int64_t>((nx + 255) / 256, 65536)), 256, 0,
                                  s>>>(A, 1, nx, fin.mx, 0, fin.E, fin.M, fin.S, xq, in_bias_out, in_ibias_out);
            rc = hip_check("fp8a input fake-quant");
            if (rc) return rc;
            a.A = xq;
        }
    } else if (fin.mx) {  // empty product: the quantizer's bias is still set, as its forward would
        fq_bias_kernel<<<1, 1, 0, s>>>(fin, in_bias_out, in_ibias_out);
        rc = hip_check("fp8a input-quantizer bias");
        if (rc) return rc;
    }
    return run_gemm(a, table, workspace, rest, s);
}

int fp8a_max_pool2d(const float *x, float *y, int64_t Bn, int64_t C, int64_t H, int64_t W, int kh, int kw, int sh,
                    int sw, int ph, int pw, fp8a_stream_t stream) {
    if (!x || !y) return fail(FP8A_EINVAL, "null pointer");
    if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || ph < 0 || pw < 0 || 2 * ph > kh || 2 * pw > kw)
        return fail(FP8A_EINVAL, "bad pooling window");
    const int64_t Ho = (H + 2 * ph - kh) / sh + 1, Wo = (W + 2 * pw - kw) / sw + 1;
    if (Ho <= 0 || Wo <= 0) return fail(FP8A_EINVAL, "empty pooling output");
    const int64_t total = Bn * C * Ho * Wo;
    if (total == 0) return FP8A_OK;
    if (kh == 3 && kw == 3 && sh == 2 && sw == 2 && ph == 1 && pw == 1 && W % 8 == 0 && H * W < (1ll << 31) &&
        ((uintptr_t)x & 15) == 0 && ((uintptr_t)y & 15) == 0) {
        const int64_t groups = Bn * C * Ho * (W / 8);
        max_pool2d_s2k3_kernel<<<(unsigned)std::min<int64_t>((groups + 255) / 256, 65536), 256, 0, (hipStream_t)stream>>>(
            x, y, Bn * C, (int)H, (int)W, (int)Ho);
        return hip_check("fp8a_max_pool2d");
    }
    max_pool2d_kernel<<<(unsigned)std::min<int64_t>((total + 255) / 256, 65536), 256, 0, (hipStream_t)stream>>>(
        x, y, Bn * C, (int)H, (int)W, (int)Ho, (int)Wo, kh, kw, sh, sw, ph, pw);
    return hip_check("fp8a_max_pool2d");
}

int fp8a_avg_pool2d_plane(const float *x, float *y, int64_t Bn, int64_t C, int64_t H, int64_t W, int kh, int kw,
                          int sh, int sw, fp8a_stream_t stream) {
    if (kh < 1 || kw < 1 || sh < 1 || sw < 1 || kh > H || kw > W || H - kh >= sh || W - kw >= sw)
        return fail(FP8A_EINVAL, "not a one-output-per-plane pooling window");
    if (H * W > 4096) return fail(FP8A_EINVAL, "plane over 4096 values");
    const int64_t planes = Bn * C;
    if (planes == 0) return FP8A_OK;
    if (!x || !y) return fail(FP8A_EINVAL, "null pointer");
    const int hw = (int)(H * W), ps = hw | 1, pb = std::min(128, 8192 / ps);
    avg_pool_plane_kernel<<<(unsigned)((planes + pb - 1) / pb), 128, (size_t)pb * ps * 4, (hipStream_t)stream>>>(
        x, y, planes, pb, (int)W, hw, ps, kh, kw, 1.0f / hw);
    return hip_check("fp8a_avg_pool2d_plane");
}

int fp8a_matmul_qamaa(const float *A, int64_t lda, const float *B, int64_t sbk, int64_t sbn, float *C, int64_t M,
                      int64_t N, int64_t K, const float *maxval, int n_bits, int Mbits, int sign_bits,
                      fp8a_stream_t stream) {
    if (lda < K) return fail(FP8A_EINVAL, "leading dimension smaller than extent");
    if (!A || !B || !C || !maxval) return fail(FP8A_EINVAL, "null pointer");
    GemmArgs a = make_args(A, lda, B, sbk, sbn, C, N, M, N, K, 1, 1, nullptr, nullptr, 0, nullptr, 0);
    a.qmax = maxval;
    a.qM = Mbits;
    a.qE = n_bits - sign_bits - Mbits;
    a.qsign = sign_bits;
    int rc = run_qamaa(a, (hipStream_t)stream);
    if (rc) return rc;
    return fp8a_fp8_quantize(C, 1, M * N, maxval, 0, n_bits, Mbits, sign_bits, C, nullptr, nullptr, stream);
}

int fp8a_conv2d_qamaa(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                      int64_t Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups,
                      const float *maxval, int n_bits, int Mbits, int sign_bits, fp8a_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (!groups_ok(groups, Cin, Cout)) return fail(FP8A_EINVAL, "bad groups");
    if (Cout / groups == 1)
        return fail(FP8A_EINVAL, "single-output-channel groups take the exact product in the reference "
                                 "(approx_calculation.py:810-811): not a qamaa launch");
    ConvShape c{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, groups};
    const int rc0 = conv_shape(c);
    if (rc0) return rc0;
    const int64_t Ho = c.Ho, Wo = c.Wo, cog = c.cog, cig = c.cig, Kg = c.Kg, Mrows = c.Mrows;
    for (int g = 0; g < groups; ++g) {
        GemmArgs a = make_args(nullptr, 0, w + g * cog * Kg, 1, Kg, y, 0, Mrows, cog, Kg, 1, 1, nullptr, nullptr, 0,
                               nullptr, 0);
        a.nchw = 1; a.hw = Ho * Wo; a.ctot = Cout; a.coff = g * cog;
        a.conv = 1; a.X = x;
        a.Cin = Cin; a.H = H; a.W = W; a.Ho = Ho; a.Wo = Wo; a.cbase = g * cig;
        a.kh = kh; a.kw = kw; a.sh = sh; a.sw = sw; a.ph = ph; a.pw = pw; a.dh = dh; a.dw = dw;
        fastdiv_params((uint32_t)(kh * kw), a.kk_mul, a.kk_shift);
        fastdiv_params((uint32_t)kw, a.kw_mul, a.kw_shift);
        a.qmax = maxval; a.qM = Mbits; a.qE = n_bits - sign_bits - Mbits; a.qsign = sign_bits;
        int rc = run_qamaa(a, s);
        if (rc) return rc;
    }
    return fp8a_fp8_quantize(y, 1, Bn * Cout * Ho * Wo, maxval, 0, n_bits, Mbits, sign_bits, y, nullptr, nullptr,
                             stream);
}

int fp8a_fp8_quantize(const float *x, int64_t rows, int64_t inner, const float *maxval, int per_row, int n_bits,
                      int Mbits, int sign_bits, float *out, float *bias_out, int32_t *ibias_out,
                      fp8a_stream_t stream) {
    const int E = n_bits - sign_bits - Mbits;
    if (Mbits < 1 || E < 1) return fail(FP8A_EFORMAT, "bad FP8 quantizer format");
    const int64_t total = rows * inner;
    if (total <= 0) return FP8A_OK;
    const int64_t blocks = std::min<int64_t>((total + 255) / 256, 65536);
    fp8_quantize_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, rows, inner, maxval, per_row, E,
                                                                           Mbits, sign_bits, out, bias_out, ibias_out);
    return hip_check("fp8a_fp8_quantize");
}

// FP8 MSE range search (fq_mse.h).  Workspace: the candidates' MseCand [rows][n_mbits * n_cand], then the
// workgroups' parts, doubles [rows][parts][n_mbits * n_cand].
static bool mse_shape_ok(int64_t rows, int64_t inner, int n_cand, int n_mbits) {
    return rows > 0 && inner > 0 && n_cand > 0 && n_mbits >= 1 && n_mbits <= MSE_MAX_MBITS &&
           (int64_t)n_cand * n_mbits <= MSE_MAX_CANDS && rows <= (int64_t)1 << 24 &&
           inner <= ((int64_t)1 << 62) / rows;
}

size_t fp8a_fp8_mse_workspace_size(int64_t rows, int64_t inner, int n_cand, int n_mbits) {
    if (!mse_shape_ok(rows, inner, n_cand, n_mbits)) return 0;
    const size_t nc = (size_t)n_cand * n_mbits;
    return (size_t)rows * nc * sizeof(MseCand) + (size_t)rows * (size_t)mse_parts(rows, inner) * nc * sizeof(double);
}

int fp8a_fp8_mse_search(const float *x, int64_t rows, int64_t inner, const float *grid, int n_cand,
                        const int32_t *mbits, int n_mbits, int n_bits, int sign_bits, double *sse, void *workspace,
                        size_t workspace_bytes, fp8a_stream_t stream) {
    if (!mse_shape_ok(rows, inner, n_cand, n_mbits)) return fail(FP8A_EINVAL, "bad MSE search shape");
    if (sign_bits < 0 || sign_bits > 1 || n_bits - sign_bits < 1 || n_bits > 16)
        return fail(FP8A_EINVAL, "bad FP8 quantizer format");
    if (mbits == nullptr) return fail(FP8A_EINVAL, "null pointer");
    MseArgs a{};
    for (int m = 0; m < n_mbits; ++m) {
        if (mbits[m] < 1 || mbits[m] > n_bits - sign_bits) return fail(FP8A_EINVAL, "mantissa width outside [1, n_bits - sign_bits]");
        a.mbits[m] = mbits[m];
    }
    if (workspace_bytes < fp8a_fp8_mse_workspace_size(rows, inner, n_cand, n_mbits))
        return fail(FP8A_EINVAL, "workspace too small");
    if (x == nullptr || grid == nullptr || sse == nullptr || workspace == nullptr || ((uintptr_t)workspace & 15) != 0)
        return fail(FP8A_EINVAL, "null or misaligned pointer");
    a.x = x; a.rows = rows; a.inner = inner; a.grid = grid;
    a.n_cand = n_cand; a.n_mbits = n_mbits; a.n_bits = n_bits; a.sign_bits = sign_bits;
    a.parts = mse_parts(rows, inner);
    a.cand = static_cast<MseCand *>(workspace);
    a.part = reinterpret_cast<double *>(a.cand + (size_t)rows * n_cand * n_mbits);
    a.sse = sse;
    launch_mse(a, opt(OPT_MSE_GROUP) != 0, (hipStream_t)stream);
    return hip_check("fp8a_fp8_mse_search");
}

// The fake quantizer's training pair (fq_train.h).  Backward workspace: the workgroups' parts, doubles [rows][parts].
static const char *fqt_shape_bad(int64_t rows, int64_t inner) {
    if (rows <= 0) return "rows must be positive";
    if (inner < 0) return "inner must not be negative";
    if (rows > (int64_t)1 << 24 || inner > ((int64_t)1 << 62) / rows) return "shape too large";
    return nullptr;
}
static int64_t fqt_parts_now(int64_t rows, int64_t inner) { return fqt_parts(rows, inner, opt(OPT_FQT_TARGET_WGS)); }

size_t fp8a_fq_train_workspace_size(int64_t rows, int64_t inner) {
    if (fqt_shape_bad(rows, inner)) return 0;
    return (size_t)rows * (size_t)fqt_parts_now(rows, inner) * sizeof(double);
}

int fp8a_fq_train_forward(const float *x, int64_t rows, int64_t inner, const float *maxval, int n_bits, int Mbits,
                          int sign_bits, float *y, uint8_t *code, float *bias_out, int32_t *ibias_out,
                          fp8a_stream_t stream) {
    if (const char *bad = fqt_shape_bad(rows, inner)) return fail(FP8A_EINVAL, bad);
    const int E = n_bits - sign_bits - Mbits;
    if (Mbits < 1 || E < 1 || sign_bits < 0 || sign_bits > 1) return fail(FP8A_EFORMAT, "bad FP8 quantizer format");
    // (empty rows have no elements to point at: only the biases are written)
    if (maxval == nullptr || (inner > 0 && (x == nullptr || y == nullptr || code == nullptr)))
        return fail(FP8A_EINVAL, "null pointer");
    FqtArgs a{};
    a.rows = rows; a.inner = inner; a.parts = fqt_parts_now(rows, inner);
    a.S = sign_bits; a.E = E; a.M = Mbits; a.fq_fast = opt(OPT_FQ_FAST);
    a.x = x; a.maxval = maxval; a.y = y; a.code = code; a.bias_out = bias_out; a.ibias_out = ibias_out;
    a.vec = (rows == 1 || inner % 4 == 0) && (((uintptr_t)x | (uintptr_t)y) & 15) == 0 && ((uintptr_t)code & 3) == 0;
    launch_fqt_forward(a, (hipStream_t)stream);
    return hip_check("fp8a_fq_train_forward");
}

int fp8a_fq_train_backward(const float *g, const uint8_t *code, int64_t rows, int64_t inner, int sign_bits,
                           float *grad_x, float *grad_maxval, void *workspace, size_t workspace_bytes,
                           fp8a_stream_t stream) {
    if (const char *bad = fqt_shape_bad(rows, inner)) return fail(FP8A_EINVAL, bad);
    if (sign_bits < 0 || sign_bits > 1) return fail(FP8A_EFORMAT, "bad FP8 quantizer format");
    // (empty rows have no elements to point at: only the zero sums are written)
    if (grad_maxval == nullptr || workspace == nullptr || (inner > 0 && (g == nullptr || code == nullptr || grad_x == nullptr)))
        return fail(FP8A_EINVAL, "null pointer");
    if (workspace_bytes < fp8a_fq_train_workspace_size(rows, inner)) return fail(FP8A_EINVAL, "workspace too small");
    if (((uintptr_t)workspace & 7) != 0) return fail(FP8A_EINVAL, "misaligned workspace");
    FqtArgs a{};
    a.rows = rows; a.inner = inner; a.parts = inner == 0 ? 0 : fqt_parts_now(rows, inner);
    a.S = sign_bits;
    a.g = g; a.code = const_cast<uint8_t *>(code); a.gx = grad_x; a.gmax = grad_maxval;
    a.part = static_cast<double *>(workspace);
    a.vec = (rows == 1 || inner % 4 == 0) && (((uintptr_t)g | (uintptr_t)grad_x) & 15) == 0 && ((uintptr_t)code & 3) == 0;
    launch_fqt_backward(a, (hipStream_t)stream);
    return hip_check("fp8a_fq_train_backward");
}

// Training-mode batch norm (bn_train.h).  Workspace: the (S, Q) double pairs [C][parts].
static bool bn_shape_ok(int64_t N, int64_t C, int64_t inner) {
    return N > 0 && C > 0 && inner > 0 && inner < ((int64_t)1 << 31) - BN_TILE && C <= (int64_t)1 << 24 &&
           N <= ((int64_t)1 << 40) / inner && N * inner <= ((int64_t)1 << 60) / C;
}

size_t fp8a_bn_train_workspace_size(int64_t N, int64_t C, int64_t inner) {
    if (!bn_shape_ok(N, C, inner)) return 0;
    return (size_t)C * (size_t)bn_parts(N, C, inner) * sizeof(double2);
}

int fp8a_bn_train(const float *x, float *y, int64_t N, int64_t C, int64_t inner, const float *gamma,
                  const float *beta, float eps, float momentum, float *running_mean, float *running_var,
                  float *save_mean, float *save_var, float *scale_shift, int act, float lo, float hi,
                  const float *q_maxval, int q_n_bits, int q_mbits, int q_sign_bits, float *q_bias, int32_t *q_ibias,
                  void *workspace, size_t workspace_bytes, fp8a_stream_t stream) {
    if (!bn_shape_ok(N, C, inner)) return fail(FP8A_EINVAL, "bad batch-norm shape");
    if (N * inner == 1)  // torch: ValueError
        return fail(FP8A_EFORMAT, "Expected more than 1 value per channel when training");
    if (act != 0 && act != 1) return fail(FP8A_EINVAL, "bn_train: act is 0 or 1");
    BnArgs a{};
    if (q_maxval) {
        const int qE = q_n_bits - q_sign_bits - q_mbits;
        if (q_mbits < 1 || qE < 1 || q_sign_bits < 0 || q_sign_bits > 1) return fail(FP8A_EFORMAT, "bad FP8 quantizer format");
        if (y == nullptr) return fail(FP8A_EINVAL, "bn_train: an output quantizer needs an output");
        a.q = FqIn{q_maxval, qE, q_mbits, q_sign_bits};
    }
    if (workspace_bytes < fp8a_bn_train_workspace_size(N, C, inner)) return fail(FP8A_EINVAL, "workspace too small");
    if (x == nullptr || save_mean == nullptr || save_var == nullptr || scale_shift == nullptr || workspace == nullptr ||
        ((uintptr_t)workspace & 15) != 0 || ((uintptr_t)scale_shift & 7) != 0)
        return fail(FP8A_EINVAL, "null or misaligned pointer");
    a.x = x; a.y = y; a.N = N; a.C = C; a.inner = inner; a.n = N * inner;
    a.parts = bn_parts(N, C, inner);
    a.part = static_cast<double2 *>(workspace);
    a.gamma = gamma; a.beta = beta; a.eps = eps; a.momentum = momentum;
    a.running_mean = running_mean; a.running_var = running_var;
    a.save_mean = save_mean; a.save_var = save_var;
    a.ss = reinterpret_cast<float2 *>(scale_shift);
    a.act = act; a.lo = lo; a.hi = hi;
    a.q_bias = q_bias; a.q_ibias = q_ibias;
    a.vec = inner % 4 == 0 && (((uintptr_t)x | (uintptr_t)y) & 15) == 0;
    launch_bn_train(a, (hipStream_t)stream);
    return hip_check("fp8a_bn_train");
}

// The config-1 layer (approx_flag off) in one launch family: fq_in on the loaded input, the exact
// product (groups = 1: run_dense, the matrix core; groups > 1: dn_group_conv), and per output
// rq -> eval batch norm -> clamp -> fq_out in the store (gemm_dense.h DnFuse).  Each quantizer
// writes its bias (the reference quantizer's custom_bias) like fp8a_conv2d_qin.
int fp8a_dense_conv2d_fused(const float *x, const float *w, float *y, int64_t Bn, int64_t Cin, int64_t H, int64_t W,
                            int64_t Cout, int kh, int kw, int sh, int sw, int ph, int pw, int dh, int dw, int groups,
                            int fmt, const float *w_maxval, int w_per_channel, int w_nbits, int w_mbits,
                            int w_sign_bits, float *w_bias_out, int32_t *w_ibias_out, const float *in_maxval,
                            int in_nbits, int in_mbits, int in_sign_bits, float *in_bias_out, int32_t *in_ibias_out,
                            const float *res_maxval, int res_nbits, int res_mbits, int res_sign_bits,
                            float *res_bias_out, int32_t *res_ibias_out, const float *bn, int act, float act_lo,
                            float act_hi, const float *out_maxval, int out_nbits, int out_mbits, int out_sign_bits,
                            float *out_bias_out, int32_t *out_ibias_out, void *workspace, size_t workspace_bytes,
                            fp8a_stream_t stream) {
    hipStream_t s = (hipStream_t)stream;
    DnFuse fz{};
    int rc = fused_quantizer(w_maxval, w_nbits, w_mbits, w_sign_bits, w_bias_out, w_ibias_out, fz.wq);
    if (!rc) rc = fused_quantizer(in_maxval, in_nbits, in_mbits, in_sign_bits, in_bias_out, in_ibias_out, fz.qin);
    if (!rc) rc = fused_quantizer(res_maxval, res_nbits, res_mbits, res_sign_bits, res_bias_out, res_ibias_out, fz.rq);
    if (!rc) rc = fused_quantizer(out_maxval, out_nbits, out_mbits, out_sign_bits, out_bias_out, out_ibias_out, fz.oq);
    if (rc) return rc;
    fz.wq_row = w_maxval && w_per_channel ? 1 : 0;
    fz.bo[0] = in_bias_out; fz.ibo[0] = in_ibias_out;
    fz.bo[1] = res_bias_out; fz.ibo[1] = res_ibias_out;
    fz.bo[2] = out_bias_out; fz.ibo[2] = out_ibias_out;
    fz.bo[3] = w_bias_out; fz.ibo[3] = w_ibias_out;
    fz.ep = reinterpret_cast<const float2 *>(bn);
    fz.act = act;
    fz.lo = act_lo;
    fz.hi = act_hi;
    if (groups != 1)
        return grouped_conv_impl(x, w, y, Bn, Cin, H, W, Cout, groups, kh, kw, sh, sw, ph, pw, dh, dw, fz, s);
    return dense_conv(ConvShape{Bn, Cin, H, W, Cout, kh, kw, sh, sw, ph, pw, dh, dw, 1}, x, w, y, fmt, fz, workspace,
                      workspace_bytes, s);
}

}  // extern "C"
