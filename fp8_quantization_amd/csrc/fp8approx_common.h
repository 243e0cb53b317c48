// fp8approx_common.h -- definitions shared by the translation units of libfp8approx.so
// (fp8approx.hip: the C-ABI, the host dispatch and the small kernels; k_fast.hip, k_f8mx.hip,
// k_tt.hip, k_v5.hip: the GEMM kernel families; k_check.hip: the fused self-check; k_mse.hip: the MSE
// range search; k_bn.hip: training-mode batch norm -- compiled in parallel by build_native.py).
// Launch arguments, operand decode, the shared epilogue (store_tile) and the word-image emission.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <string>

#include "../../include/fp8approx.h"
#include "fp8approx_device.h"

namespace fp8a {

// ------------------------------------------------------------------------- table packing
// The error table (get_error_table_NN, v9:555-592) is a host constant; it is analysed on the
// host and packed into the launch arguments so the hot loop reads one register per operand:
//   TM_W1U  : entries in {0,1}   -> 1 bit / entry, 2^M bits per row      (E4M3)
//   TM_W2S/U: entries in [-2,1] / [0,3] -> 2 bits / entry, R = 2^M*2/32 words per row
//   TM_LUT  : anything else -> float LUT in LDS (E2M5 no-comp: entries up to 5)
enum TMode : int { TM_NONE = 0, TM_W1U = 1, TM_W2S1 = 2, TM_W2U1 = 3, TM_W2S2 = 4, TM_W2U2 = 5, TM_LUT = 6,
                   TM_QAMAA = 7 /* quantize_after_mult_and_add: term = fq(a*b), no decode */,
                   TM_V5 = 8 /* v5 integer-adder model: code sum + compensation LUT, OF/UF wrap */,
                   TM_F8 = 9 /* E4M3 with s2n + qbma, table in {0,1}: LDS term LUT + hardware fp8 Q_R */ };

struct TablePack {
    uint32_t rows[64][2];  // packed rows for the bit modes (2^M <= 64)
    int8_t raw[1024];      // the full table (2^M x 2^M), row-major; exact path and LUT mode
};

// ------------------------------------------------------------------------- GEMM arguments
// FP8 fake quantizer of the activations (quantize_to_fp8_ste_MM, fp8_quantizer.py:97-173),
// per tensor: the bias from maxval, then clamp / binade step / round.  fp8_quantize_kernel and the
// fused input quantization of the approx ops (fp8a_conv2d_qin) share these, bit for bit.
struct FqIn {
    const float *mx;  // device maxval [1]; nullptr = the input is already quantized
    int E, M, S;      // exponent / mantissa / sign bits of the quantizer
};

__device__ __forceinline__ float fq_bias(float mx, int E, int M) {
    return rintf((float)(1 << E) - log2f(mx) + log2f(2.0f - p2(-M)) - 1.0f);
}

// quantize_to_fp8_ste_MM's forward (fp8_quantizer.py:97-173) on one value, bias = fq_bias(mx):
//   xc = clamp(v), ls = max(floor(log2 |xc|) + bias, 1) (1 for xc = 0), k = ls - M - bias,
//   q = rint(xc / 2^k) 2^k.
// (Round 5 measured a bit-level form -- RNE on the float's bits at or above the smallest normal
// binade -- against this one: 7 % slower on the fake-quant kernel, no faster in the depthwise
// stages or the dense GEMM, so the literal form stays.)
// rint(xc / 2^k) 2^k without the IEEE division: the quotient is exact (a power-of-two scaling) and
// is formed as xc 2^-k, in two exact steps when 2^-k itself overflows (k < -126: then |xc| <= maxval
// is tiny and xc 2^64 cannot overflow); 2^k = 0 (k < -149) leaves the division's (x / 0) * 0 = NaN,
// formed as (x inf) * 0.
__device__ __forceinline__ float fq_step(float xc, int k) {
    const float t = (k >= -126) ? xc * p2(-k) : (xc * 18446744073709551616.0f) * p2(-k - 64);
    const float r = rintf(t) * p2(k);
    return k < -149 ? rintf(xc * __builtin_huge_valf()) * p2(k) : r;  // (x / 0 = x inf: the same NaN)
}
__device__ __forceinline__ float fq_apply_lit(float xc, float bias, int M) {
    int e;
    frexpf(xc, &e);
    const float ls = (xc == 0.0f) ? 1.0f : fmaxf((float)(e - 1) + bias, 1.0f);
    return fq_step(xc, (int)(ls - (float)M - bias));
}
__device__ __forceinline__ float fq_apply(float v, float mx, float bias, int M, int sign_bits) {
    return fq_apply_lit(fminf(fmaxf(v, sign_bits ? -mx : 0.0f), mx), bias, M);
}

// The fast form of fq_apply_lit (option "fq_fast"): the same value, bit for bit, as
//     q = (xc + C) - C,  C = 1.5 * 2^(k + 23),  k = max(floor(log2 |xc|), 1 - bias) - M.
// The float add rounds to nearest-even at bit k (C is an even multiple of 2^k and |xc| < 2^(k+M+1)
// keeps the sum inside C's binade); the subtraction is exact.  C's bits are
//     max(exponent field of xc, emn) + cadd,  emn = bits(2^(1 - bias)),  cadd = (23 - M) << 23 | 0x400000
// (a zero or float-subnormal xc has field 0 and takes emn, as ls = 1 does).  The sum loses the sign
// of a negative xc that rounds to zero, which the literal form keeps (rint(-0.3) = -0.0): xc's sign
// bit is copied onto q.  Six operations (and, max, add, add, sub, bfi) for the literal form's ~30.
// Valid while every reachable k keeps 2^k and 2^(k+24) normal floats and the literal form's own
// arithmetic on bias is exact: fq_fast_ok, a conservative window on the quantizer's constants (wave
// uniform, tested once per launch / epilogue).  Outside it -- the literal form's k < -126 / k < -149
// arms, a NaN or infinite bias (maxval <= 0 or not finite) -- callers keep the literal form.
struct FqFast {
    uint32_t emn, cadd;
    float mx;  // the quantizer's maxval, read once (the literal callers re-read it from memory per value)
};
__device__ __forceinline__ bool fq_fast_ok(float mx, float bias, int M) {
    return bias >= -100.0f && bias <= 120.0f && mx >= 0x1p-100f && mx <= 0x1p64f && M >= 1 && M <= 6;
}
__device__ __forceinline__ FqFast fq_fast_k(float mx, float bias, int M) {  // (fq_fast_ok holds)
    return FqFast{(uint32_t)(128 - (int)bias) << 23, ((uint32_t)(23 - M) << 23) | 0x00400000u, mx};
}
__device__ __forceinline__ float fq_apply_fast(float xc, const FqFast &k) {
    const uint32_t u = __float_as_uint(xc);
    const float C = __uint_as_float(max(u & 0x7F800000u, k.emn) + k.cadd);
    const float q = (xc + C) - C;
    return __uint_as_float((__float_as_uint(q) & 0x7FFFFFFFu) | (u & 0x80000000u));
}
// fq_apply; FQF = true: the fast form where the caller's uniform test allowed it (k.emn != 0; k.mx = maxval
// either way), the literal one else -- one uniform branch per value; false: the literal form only
template <bool FQF>
__device__ __forceinline__ float fq_apply_f(float v, float mx, float bias, int M, int sign_bits, const FqFast &k) {
    if (FQF) {  // (k.emn = 0: the guard failed, uniform)
        const float xc = fminf(fmaxf(v, sign_bits ? -k.mx : 0.0f), k.mx);
        return k.emn ? fq_apply_fast(xc, k) : fq_apply_lit(xc, bias, M);
    }
    return fq_apply_lit(fminf(fmaxf(v, sign_bits ? -mx : 0.0f), mx), bias, M);
}

// Word-image hand-off (round 4, fp8a_conv2d_chain): a convolution's store also writes the NEXT
// convolution's pre-decoded A operand -- its zero-bordered word image (gemm_f8mx.h: the word of
// fq_next(y) for every output element y) -- so the next launch skips its xm_decode_a pass (which
// reads y back and writes the image: 8 B of HBM traffic per element).  Same words as that pass,
// bit for bit: the same fq_apply / xm_word_a on the same float.  An element outside the
// matrix-core window sets the image's header word, and the consumer's gated pre-pass then
// re-decodes its input from y (the fp32 output is always written).
struct EmitW {
    uint32_t *w;        // the image's words [Bn][C][awH][awW] (nullptr: no emission)
    uint32_t *invalid;  // the image's header word
    int awH, awW, awph, awpw;
    int Wo;
    uint32_t hw_mul, hw_shift, wo_mul, wo_shift;  // fastdiv by Ho * Wo and Wo (output index < 2^31)
    uint32_t hw;
    FqIn fq;            // the next convolution's input quantizer (per tensor)
    const int32_t *bR;  // its result bias
    int Mw;             // its mantissa width (3: e4m3 words, 2: e5m2)
    int form;           // 0: gemm_f8mx_kernel's words (zero-bordered image); 1: the tensor-bias table
                        // form's words (conv_tbx.h tbx_decode_a: a depthwise consumer, no border)
};

struct GemmArgs {
    const float *A;
    int64_t lda;
    const float *B;
    int64_t sbk, sbn;
    float *C;
    int64_t ldc;
    int64_t M, N, K;
    int E, Mw;
    uint32_t kexp, kdc;  // 0x7F800000 and (23 - Mw) << 23 as launch arguments: opaque SGPR operands
                         // keep q_fast at one v_and_or_b32 / one v_add_u32 (see make_qc)
    const int32_t *bA;
    const int32_t *bB;
    int64_t bBs;
    const int32_t *bR;
    uint32_t flags;
    // output mapping: rowmajor C[m*ldc + n], or NCHW C[(m/hw)*ctot*hw + (coff+n)*hw + m%hw]
    int nchw;
    int64_t hw, ctot, coff;
    uint32_t *flag;  // device word: set by the fast kernel when the exact kernel must run (FB_* bits);
                     // a slot of the library's flag arena (flag_arena, fp8approx.hip), zero on entry
    // per-unit fallback marks (64 x 64 output units): urow[row unit] / ucol[column unit] for an
    // operand outside the fast path's window, utile[row unit * nuc + column unit] for a tile whose
    // terms left it; the gated exact kernel recomputes only the marked units.  nullptr (a
    // workspace without room for them): any fallback recomputes the whole launch.
    uint8_t *urow, *ucol, *utile;
    int64_t nur, nuc;
    // split-K: block b works on tile b % tiles over k in [s*kchunk, (s+1)*kchunk), s = b / tiles;
    // with splits > 1 it writes its partial tile to part + s*M*N (the output layout with
    // ctot = N, coff = 0, ldc = N) and splitk_reduce_kernel sums the splits in order -- or, with skcnt
    // (option "splitk_fixup", gemm_f8mx_kernel's E4M3 launches), the tile's last-arriving block does, in
    // the same order, inside the launch: skcnt[tile] counts the arrivals (sk_words words after the
    // partials in the workspace, zeroed by xm_decode_b ahead of every launch)
    int splits;
    int xm_wave_rows;  // host side only (launch_shape, k_f8mx.hip; in what was padding): the 128 x 64 "xm_pipe" instances
                       // run with the math loop's waves by rows (option "xm_wave_rows", gemm_f8mx.h WROWS; 0: by columns)
    int64_t kchunk;
    float *part;
    uint32_t *skcnt;
    int64_t sk_words;
    // implicit-GEMM convolution: A(m, k) gathered from NCHW x (no im2col image), m = (b, ho, wo),
    // k = (c, ky, kx) within the group -- the reference's im2col order (approx_calculation.py:745)
    int conv;
    const float *X;
    int64_t Cin, H, W, Ho, Wo, cbase;
    int kh, kw, sh, sw, ph, pw, dh, dw;
    uint32_t kk_mul, kk_shift, kw_mul, kw_shift;  // fast division by kh*kw and by kw
    // qamaa: the res quantizer's FP8 fake quantizer (fp8_quantizer.py:97-173) per product
    const float *qmax;
    int qE, qM, qsign;
    // fused eval-mode BatchNorm + activation epilogue (BNFusedHijacker: F.batch_norm then ReLU /
    // ReLU6 / Hardtanh): per output channel {scale, shift}; ep_act clamps to [ep_lo, ep_hi]
    const float2 *ep;
    int ep_act;
    float ep_lo, ep_hi;
    // pre-decoded operands of the matrix-core E4M3 kernel (gemm_f8mx.h): A words (conv: the
    // group's [Bn][aw_c][H][W] slice; matrix: [M][awld]), B column pairs [Kpad][npad / 2]
    const uint32_t *aw;
    int64_t awld, aw_c;
    int64_t awH, awW;  // conv: the word image's height / width (H + 2 ph, W + 2 pw when zero-padded)
    int awph, awpw;    // conv: x's offset inside the word image (the zero border's width)
    int wfmt;          // pre-decoded operand format: 0 = gemm_f8mx_kernel's, 1 = gemm_tt_kernel's, 2 = gemm_tt16_kernel's,
                       // 4 = gemm_v5mx_kernel's
    int ttf7;          // gemm_tt_kernel: the table has negative entries (the F7 sign rule)
    int af32;          // gemm_f8mx_kernel reads A as fp32 and decodes it while staging (no A pre-pass)
    int xncg;          // gemm_f8mx_kernel's column groups per tile (4: 128 x 64, 2: 128 x 32, 1: 256 x 16)
    int xm_signs;      // gemm_f8mx_kernel builds the negative-sign table rows only when flag[3] says an A word
                       // addresses them (option "xm_sign_rows"; 0: always both halves)
    int fq_fast;       // option "fq_fast": the matrix-core path's quantizers and emitted words take their fast
                       // forms (fq_apply_fast, fq_word) where the uniform guards allow; 0: the literal forms
    const uint2 *bqw;
    const uint32_t *lutw;  // the LDS table image (XM_LUT_WORDS words), written by xm_decode_b
    // E5M2 (gemm_f8mx_kernel XF = 1): per (K-step, 16-column group) the nonzero B elements' exponent
    // range, (max e_b + 128) | (min e_b + 128) << 8 ([kpad][npad / 16]; 0xFF00 when all are zero)
    const uint16_t *ebr;
    int xm_vmin;  // the smallest binade of the table value V' (0: V' >= 1; down to -2M with a custom table, xm_table_form)
    int xm_pipe;  // host side only (launch_shape, k_f8mx.hip): the word-staged E4M3 / E5M2 launches run the instances
                  // whose K loop reads LDS one stage ahead (option "xm_pipe", gemm_f8mx.h PIPE; 0: the loop without it)
    int64_t npad;
    // fused input quantization (fp8a_conv2d_qin): A = fq(X); the quantizer's bias is written to
    // fq_bias / fq_ibias by the A pre-decode, and bA points at fq_ibias
    FqIn fqin;
    float *fq_bias;
    int32_t *fq_ibias;
    // block-output epilogue (fp8a_conv2d_block): after BN / activation, y += res (same index as
    // y), then the post clamp (post_act 1) or GELU (post_act 2), then the block's output quantizer (post_fq)
    const float *res;
    int post_act;
    float post_lo, post_hi;
    FqIn post_fq;
    EmitW em;              // word-image emission for the next convolution (em.w nullptr: off)
    const uint32_t *gate;  // xm_decode_a: run only if *gate != 0 (the input image arrived invalid)
    const uint32_t *in_img; // the input's word image (header + words) a previous launch emitted, or nullptr
    TablePack tab;
    uint32_t *flag_out;  // the caller's workspace word that receives the launch's final flag word
    uint4 *arena_clr;    // the flag arena's other slot, and its 16-byte words to zero (arena_clear)
    uint32_t arena_clr16;
    float *post_bout;    // post_fq's bias outputs (its custom_bias), written by gemm_exact_kernel, or nullptr
    int32_t *post_ibout;
    // gemm_f8mx_kernel's 32-bit tile setup, made once per launch by its launcher (launch_shape, k_f8mx.hip) like
    // kk_mul / kw_mul above; appended, so every earlier field keeps its offset: the tile counts and the fastdiv
    // magics of blockIdx.x / tiles, tile / row tiles, row / (Ho * Wo), pixel / Wo (conv) and row / hw (an NCHW
    // store).  Every dividend is below 2^31 (mx_plan's fits32, fp8approx.hip).  No other kernel reads them.
    uint32_t xm_tiles, xm_num_mt;
    uint32_t xt_mul, xt_shift, xmt_mul, xmt_shift;
    uint32_t ohw_mul, ohw_shift, owo_mul, owo_shift;
    uint32_t shw_mul, shw_shift;
};

// Fallback flag word bits: FB_ANY = some output unit needs the exact kernel, FB_ALL = every
// unit does (a bias outside the exactness window, or no unit marks in the workspace).  (Bits
// 1-4 belong to gemm_tt16_kernel's f16 window, gemm_tt16.h.)
constexpr uint32_t FB_ANY = 1u, FB_ALL = 32u;
// FB_HALF: an E5M2 tile of gemm_f8mx_kernel's plain form met the result grid's top binade and
// asks the halved-block form (XF = 2) to recompute it; its unit marks carry UT_HALF.  Unit mark
// bits: UT_EXACT = recompute in the exact kernel, UT_HALF = recompute in the halved-block form
// (kept set by a halved-block tile that fails, so the tiles sharing the unit still see it).
constexpr uint32_t FB_HALF = 64u;
constexpr uint8_t UT_EXACT = 1u, UT_HALF = 2u;

// Fallback flag value of a block that found a bad operand: FB_ANY once the unit marks are
// written, FB_ALL too without them (or when `all`).
__device__ __forceinline__ uint32_t fb_bits(const GemmArgs &p, bool all = false) {
    return (all || p.urow == nullptr) ? (FB_ANY | FB_ALL) : FB_ANY;
}

// The flag arena (fp8approx.hip: flag_arena) has two slots per stream that launches use in turn:
// a launch finds its slot zero, and its last (gated) kernel zeroes the OTHER slot -- the words the
// previous launch left there, which nothing reads any more -- with every thread of its grid
// (16-byte stores; no fill launch, no counter, no ordering against the launch's own reads).
__device__ __forceinline__ void arena_clear(uint4 *clr, uint32_t n16) {
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += gridDim.x * blockDim.x)
        clr[i] = make_uint4(0u, 0u, 0u, 0u);
}

// Mark the row units of output rows [m_lo, m_hi) / the column unit of column n / the units of
// the output tile (m0 .. m0 + rows - 1, n0 .. n0 + 63) for the exact kernel (plain byte stores:
// every writer stores 1).  The caller raises the flag word (fb_bits).
__device__ __forceinline__ void fb_rows(const GemmArgs &p, int64_t m_lo, int64_t m_hi) {
    if (p.urow == nullptr || m_hi <= m_lo) return;
    for (int64_t u = m_lo >> 6; u <= (m_hi - 1) >> 6; ++u) p.urow[u] = 1;
}
__device__ __forceinline__ void fb_col(const GemmArgs &p, int64_t n) {
    if (p.ucol != nullptr) p.ucol[n >> 6] = 1;
}
__device__ __forceinline__ void fb_tile(const GemmArgs &p, int64_t m0, int64_t rows, int64_t n0,
                                        uint8_t mark = UT_EXACT) {
    if (p.utile == nullptr) return;
    const int64_t hi = min(m0 + rows, p.M);
    for (int64_t u = m0 >> 6; u <= (hi - 1) >> 6; ++u) p.utile[u * p.nuc + (n0 >> 6)] = mark;
}

// The block-output epilogue on one value / four values of the output at index o; pb = the post
// quantizer's bias (post_bias()).
__device__ __forceinline__ float post_bias(const GemmArgs &p) {
    return p.post_fq.mx ? fq_bias(*p.post_fq.mx, p.post_fq.E, p.post_fq.M) : 0.0f;
}

// nn.GELU() (approximate='none') in fp32 as ATen's GeluCUDAKernelImpl evaluates it:
// x * 0.5 * (1 + erf(x * M_SQRT1_2)), left to right, the same device erff (ocml)
__device__ __forceinline__ float gelu_erf(float x) {
    return x * 0.5f * (1.0f + erff(x * (float)M_SQRT1_2));
}

// GELU = false compiles the GELU tail out (the word-emitting store of gemm_f8mx_kernel, whose
// registers are at its occupancy budget; the host never pairs GELU with emission).
// FQF = true: the post quantizer in its fast form where pk says so (pk.emn != 0: StoreCtx, store_ctx tested
// fq_fast_ok), maxval read from pk.mx either way; false: the literal form only.
template <bool GELU = true, bool FQF = false>
__device__ __forceinline__ float post_tail(const GemmArgs &p, float v, float pb, const FqFast &pk = FqFast{}) {
    if (p.post_act == 1) v = fminf(fmaxf(v, p.post_lo), p.post_hi);
    else if (GELU && p.post_act == 2) v = gelu_erf(v);
    if (p.post_fq.mx) v = fq_apply_f<FQF>(v, FQF ? pk.mx : *p.post_fq.mx, pb, p.post_fq.M, p.post_fq.S, pk);
    return v;
}

template <bool GELU = true, bool FQF = false>
__device__ __forceinline__ float post1(const GemmArgs &p, int64_t o, float v, float pb, const FqFast &pk = FqFast{}) {
    if (p.res) v += p.res[o];
    return post_tail<GELU, FQF>(p, v, pb, pk);
}

template <bool GELU = true, bool FQF = false>
__device__ __forceinline__ float4 post4(const GemmArgs &p, int64_t o, float4 v, float pb, const FqFast &pk = FqFast{}) {
    if (p.res) {
        const float4 r = *reinterpret_cast<const float4 *>(p.res + o);
        v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
    }
    return make_float4(post_tail<GELU, FQF>(p, v.x, pb, pk), post_tail<GELU, FQF>(p, v.y, pb, pk),
                       post_tail<GELU, FQF>(p, v.z, pb, pk), post_tail<GELU, FQF>(p, v.w, pb, pk));
}

// y = x * scale + shift with scale = gamma * invstd, shift = beta - mean * scale (ATen's eval
// batch-norm transform), then the activation clamp; c = output channel
__device__ __forceinline__ float epi(float2 e, int act, float lo, float hi, float x) {  // (the channel's pair, loaded)
    const float v = __fmaf_rn(x, e.x, e.y);
    return act ? fminf(fmaxf(v, lo), hi) : v;
}
__device__ __forceinline__ float epi(const float2 *ep, int act, float lo, float hi, int64_t c, float x) {
    if (ep == nullptr) return x;
    return epi(ep[c], act, lo, hi, x);
}

// n / d for 0 <= n < 2^31 via one mulhi: q = (mulhi(n, mul) + n) >> shift (Granlund-Montgomery).
static inline void fastdiv_params(uint32_t d, uint32_t &mul, uint32_t &shift) {
    uint32_t l = 0;
    while ((1ull << l) < d) ++l;
    shift = l;
    mul = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
}

__device__ __forceinline__ uint32_t fastdiv(uint32_t n, uint32_t mul, uint32_t shift) {
    return (__umulhi(n, mul) + n) >> shift;
}

constexpr int BM = 64, BN = 64, BK = 16, TM = 4, TN = 4, NT = 256;
constexpr int AP = BM + 4, BP = BN + 4;

__device__ __forceinline__ uint32_t xm_word_a(float x, int M, int xb, uint32_t emnA, int bR, bool &ok);  // gemm_f8mx.h
__host__ __device__ constexpr int xm_xbias(int Mw);

// A = 0 as an A word of the matrix-core path (gemm_f8mx.h): cvt scale 2^126 (the code is 0), row 0.
// Nonzero words keep se <= 252, so a zero word is the one with se = 253, and the E5M2 halved form's
// se + 1 (254: 2^127) still flushes it to 0.
constexpr uint32_t XM_ZERO_WORD = 253u << 23;
// A word bits 3-6: the tile-table row (8 s_a + m_a) * 8 = its byte offset in a column block
constexpr uint32_t XM_ROW_SHIFT = 3, XM_ROW_MASK = 0x78u;

// Word-image emission (EmitW): one word per final output value at NCHW output index o (< 2^31,
// the host checks).  The next quantizer's constants sit in the image's header (emit_prep_kernel:
// [1] maxval, [2] its float bias, [3] 2^(1 - bias) bits, [4] bR; [5] / [6] collect the emitted words'
// scale-exponent extreme and "a negative word was written", below), made wave-uniform (SGPRs) once
// per epilogue: the matrix-core kernel runs at its 80-VGPR budget, and per-thread copies of them
// (or their recomputation from maxval) in VGPRs made it spill.
struct EmitCtx {
    float mx, fb;
    uint32_t emn;
    int bR;
    FqFast k;   // the fast forms' constants (emit_ctx_fast)
    int kse;
    bool chk;
};
__device__ __forceinline__ EmitCtx emit_ctx(const GemmArgs &p) {
    EmitCtx e{};
    if (p.em.w == nullptr) return e;
    const uint4 h = *reinterpret_cast<const uint4 *>(p.em.invalid);  // header words 0-3 (uniform: SGPRs)
    e.mx = __uint_as_float(__builtin_amdgcn_readfirstlane(h.y));
    e.fb = __uint_as_float(__builtin_amdgcn_readfirstlane(h.z));
    e.emn = __builtin_amdgcn_readfirstlane(h.w);
    e.bR = __builtin_amdgcn_readfirstlane((int)p.em.invalid[4]);
    return e;
}

// xm_word_a(q) (gemm_f8mx.h) for a q that the (M, bias) quantizer just produced, from q's bits: q is on
// the decode's grid by construction when the decode's M and min-normal are the quantizer's (fq_word_ok),
// so the grid test drops out, the scale exponent is kse - (exponent field of q), kse = 254 + xb - bR, and
// the row is q's sign and top M mantissa bits.  What is left of `ok` is the exactness window and the
// scale range; chk = false when the quantizer's reachable exponents -- the smallest subnormal
// 2^(1 - bias - M) up to one binade above maxval's (its rounding can carry) -- lie inside both, and then
// no element is tested (uniform, once per epilogue).  The same word and the same ok as xm_word_a's.
__device__ __forceinline__ bool fq_word_ok(int fqM, float fbias, int Mw, uint32_t emn) {
    return fqM == Mw && emn == ((uint32_t)(128 - (int)fbias) << 23);  // (after fq_fast_ok)
}
__device__ __forceinline__ bool fq_word_chk(float mx, float fbias, int Mw, int kse) {
    const int lo = 128 - (int)fbias - Mw, hi = (int)(__float_as_uint(mx) >> 23) + 1;  // exponent fields
    return !(lo >= max(65, kse - 252) && hi <= min(176, kse - 1));
}
__device__ __forceinline__ uint32_t fq_word(float q, int Mw, int kse, bool chk, bool &ok) {
    const uint32_t u = __float_as_uint(q), ua = u & 0x7FFFFFFFu;
    int se = kse - (int)(ua >> 23);
    if (chk) {
        ok = ua == 0u || (ua >= 0x20800000u && ua <= 0x58800000u && se >= 1 && se <= 252);
        se = min(max(se, 1), 252);
    } else {
        ok = true;
    }
    const uint32_t mc = (ua >> (23 - Mw)) & ((1u << Mw) - 1u);  // row 8 s_a + m_a, as xm_word_a places it
    return ua == 0u ? XM_ZERO_WORD : (((uint32_t)se << 23) | (((u >> 31) * 8u + mc) << XM_ROW_SHIFT));
}
// FQF (emission): the next quantizer passes fq_fast_ok and, for form-0 words, fq_word_ok
__device__ __forceinline__ bool emit_fast_ok(const GemmArgs &p, const EmitCtx &e) {
    return fq_fast_ok(e.mx, e.fb, p.em.fq.M) && (p.em.form != 0 || fq_word_ok(p.em.fq.M, e.fb, p.em.Mw, e.emn));
}
__device__ __forceinline__ void emit_ctx_fast(const GemmArgs &p, EmitCtx &e) {  // (emit_fast_ok holds)
    e.k = fq_fast_k(e.mx, e.fb, p.em.fq.M);
    e.kse = 254 + xm_xbias(p.em.Mw) - e.bR;
    e.chk = fq_word_chk(e.mx, e.fb, p.em.Mw, e.kse);
}
// What a final store needs of its quantizers, computed once per block (wave-uniform): the post
// quantizer's bias, the emission's header constants, and the store's one test (option "fq_fast"): fqf =
// every quantizer the store runs -- the post quantizer, the emitted words' -- passes its guard; then pk /
// ec hold the fast forms' constants, else the store keeps the literal forms throughout.
struct StoreCtx {
    float pb;
    FqFast pk;
    EmitCtx ec;
    bool fqf;
};
template <bool EMIT>
__device__ __forceinline__ StoreCtx store_ctx(const GemmArgs &p, bool fast_allowed = true) {
    StoreCtx c{};
    c.pb = post_bias(p);
    if (EMIT) c.ec = emit_ctx(p);
    const bool emit = EMIT && p.em.w != nullptr;
    const float pmx = p.post_fq.mx ? *p.post_fq.mx : 0.0f;
    c.fqf = fast_allowed && p.fq_fast && (!p.post_fq.mx || fq_fast_ok(pmx, c.pb, p.post_fq.M)) &&
            (!emit || emit_fast_ok(p, c.ec));
    c.pk.mx = pmx;  // (emn = 0: the literal forms, with maxval still read once)
    c.ec.k.mx = c.ec.mx;
    if (c.fqf) {
        if (p.post_fq.mx) c.pk = fq_fast_k(pmx, c.pb, p.post_fq.M);
        if (emit) emit_ctx_fast(p, c.ec);
    }
    return c;
}
template <bool FQF = false>
__device__ __forceinline__ uint32_t emit_word(const GemmArgs &p, const EmitCtx &e, float v, bool &ok) {
    const float q = fq_apply_f<FQF>(v, e.mx, e.fb, p.em.fq.M, p.em.fq.S, e.k);
    if (p.em.form) {  // tbx_decode_a's word of q (a value off the grid / outside the window: invalid)
        const uint32_t u = __float_as_uint(q), ua = u & 0x7FFFFFFFu, M = (uint32_t)p.em.Mw;
        ok = ok && (ua == 0u || ((ua & ((1u << (23 - M)) - 1u)) == 0u && ua >= 0x20800000u && ua <= 0x58800000u));
        return ua == 0u ? 0u : ((u & 0xFF800000u) | (((ua >> (23 - M)) & ((1u << M) - 1u)) << 3));
    }
    if (FQF && e.k.emn) return fq_word(q, p.em.Mw, e.kse, e.chk, ok);
    return xm_word_a(q, p.em.Mw, xm_xbias(p.em.Mw), e.emn, e.bR, ok);
}
// word index of NCHW output index o
__device__ __forceinline__ uint32_t emit_index(const GemmArgs &p, uint32_t uo, uint32_t &wo) {
    const uint32_t plane = fastdiv(uo, p.em.hw_mul, p.em.hw_shift), pix = uo - plane * p.em.hw;
    const uint32_t ho = fastdiv(pix, p.em.wo_mul, p.em.wo_shift);
    wo = pix - ho * (uint32_t)p.em.Wo;
    return (plane * (uint32_t)p.em.awH + ho + (uint32_t)p.em.awph) * (uint32_t)p.em.awW + wo + (uint32_t)p.em.awpw;
}
// Max of v over the wave, then one atomicMax into *dst (v >= 0; 0 records nothing) unless *dst
// already holds at least v -- every wave of a launch records into the same word, and the read
// first keeps the atomics (serialised on one L2 line) to the few waves that raise it.  Every lane
// of the wave must call it.
__device__ __forceinline__ void wave_max_atomic(uint32_t *dst, uint32_t v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off));
    if ((threadIdx.x & 63) == 0 && v != 0u && v > __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        atomicMax(dst, v);
}
// 255 - the scale exponent of a nonzero word (the E5M2 halved-block decision reads the largest,
// gemm_f8mx.h xm_needs_halving; the header's word 5 collects it for the consumer)
__device__ __forceinline__ uint32_t word_sehi(uint32_t w) { return w == XM_ZERO_WORD ? 0u : 255u - (w >> 23); }

// "A negative A word was written": gemm_f8mx_kernel's tile table holds the rows of s_a = 1 (8 + m_a)
// only for launches whose A words address them (word bit 6; a zero's word has row bits 0, -0.0
// included).  Every writer of form-0 words ORs its words into one register and records bit 6 after
// its stores: the A pre-pass into the launch's flag[3], an emitting producer into header word [6] of
// the image (emit_prep_kernel clears it; the consumer's gated pre-pass copies it to flag[3]).  The
// word only ever goes 0 -> 1 within a launch, so the record is a store, not a read-modify-write,
// skipped once the word reads 1 (the read first, as wave_max_atomic).
constexpr uint32_t XM_SIGN_BIT = 0x40u;
// The A pre-pass has up to 8192 blocks that end within microseconds of each other; recording into
// one word, their stores serialise on it (ViT-B/16: +15 us on each of 73 pre-passes).  So its blocks
// spread over flag words XM_SIGN_W0 .. + XM_SIGN_NW - 1 (the second half of the 256-byte flag block,
// zeroed with the rest), and gemm_f8mx_kernel ORs them with flag[3] in its one read.
constexpr int XM_SIGN_W0 = 32, XM_SIGN_NW = 32;
// one thread's record (the exact kernels' emission; a block's or a wave's elected thread)
__device__ __forceinline__ void sign_record(uint32_t *dst, uint32_t words_or) {
    if ((words_or & XM_SIGN_BIT) != 0u && __hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
        __hip_atomic_store(dst, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one ballot per wave, then its first lane's record.  Every lane of the wave must call it.
__device__ __forceinline__ void wave_sign_record(uint32_t *dst, uint32_t words_or) {
    const bool any = __any((words_or & XM_SIGN_BIT) != 0u) != 0;
    if ((threadIdx.x & 63) == 0 && any) sign_record(dst, XM_SIGN_BIT);
}

template <bool FQF = false>
__device__ __forceinline__ void emit1(const GemmArgs &p, const EmitCtx &e, int64_t o, float v, uint32_t &sehi,
                                      uint32_t &neg) {
    uint32_t wo;
    const uint32_t wi = emit_index(p, (uint32_t)o, wo);
    bool ok = true;
    const uint32_t w = emit_word<FQF>(p, e, v, ok);
    p.em.w[wi] = w;
    sehi = max(sehi, word_sehi(w));
    neg |= w;
    if (!ok) atomicOr(p.em.invalid, 1u);
}
// four consecutive outputs (o % 4 == 0 in an NCHW plane of hw % 4 == 0): one 16-B store when
// they sit in one row of the image (Wo % 4 == 0: always; the interior rows start 16-B aligned)
template <bool FQF = false>
__device__ __forceinline__ void emit4(const GemmArgs &p, const EmitCtx &e, int64_t o, float4 v, uint32_t &sehi,
                                      uint32_t &neg) {
    uint32_t wo;
    const uint32_t wi = emit_index(p, (uint32_t)o, wo);
    bool ok0 = true, ok1 = true, ok2 = true, ok3 = true;
    const uint4 w = make_uint4(emit_word<FQF>(p, e, v.x, ok0), emit_word<FQF>(p, e, v.y, ok1),
                               emit_word<FQF>(p, e, v.z, ok2), emit_word<FQF>(p, e, v.w, ok3));
    sehi = max(max(sehi, max(word_sehi(w.x), word_sehi(w.y))), max(word_sehi(w.z), word_sehi(w.w)));
    neg |= (w.x | w.y) | (w.z | w.w);
    if (wo + 3 < (uint32_t)p.em.Wo && (wi & 3u) == 0u) {
        *reinterpret_cast<uint4 *>(p.em.w + wi) = w;
    } else {
        p.em.w[wi] = w.x;
        uint32_t wo1;
        p.em.w[emit_index(p, (uint32_t)o + 1, wo1)] = w.y;
        p.em.w[emit_index(p, (uint32_t)o + 2, wo1)] = w.z;
        p.em.w[emit_index(p, (uint32_t)o + 3, wo1)] = w.w;
    }
    if (!(ok0 && ok1 && ok2 && ok3)) atomicOr(p.em.invalid, 1u);
}

__device__ __forceinline__ int64_t out_index(const GemmArgs &p, int64_t m, int64_t n) {
    if (!p.nchw) return m * p.ldc + n;
    const int64_t img = m / p.hw, pix = m - img * p.hw;
    return (img * p.ctot + p.coff + n) * p.hw + pix;
}

// Fast-path operand decode straight from the float32 bit pattern (int-bias semantics).
//   returns ok: x is exactly a value of the (M, b) grid (any exponent: A/B are decoded with
//               clip_OF=False, v9:58-59) and |x| is 0 or in [2^-62, 2^50] (exactness window:
//               every product and table term a normal float, every Q_R constant finite,
//               DESIGN.md §3).  Otherwise the launch is flagged and the exact kernel reruns it.
//   m        : the M-bit mantissa code = the top M bits of the fp32 mantissa (the s2n scale-up
//               by 2^M, v9:53, leaves the fp32 mantissa untouched)
//   c        : sign(x) * 2^floor(log2|x|): the scale of the error-table term.  Scale-up and
//               scale-back of s2n cancel in it; without s2n a subnormal operand fails the
//               reference's norm mask (v9:87), so c = 0 there, as for zeros.
__device__ __forceinline__ bool stage_decode(float x, int M, uint32_t emn, bool s2n, float &c, uint32_t &m) {
    const uint32_t u = __float_as_uint(x);
    const uint32_t ua = u & 0x7FFFFFFFu;
    const uint32_t ex = ua & 0x7F800000u;
    const bool sub = ua < emn;  // |x| < min_norm = 2^(1-b)
    const uint32_t sh = (uint32_t)(23 - M) + (sub ? ((emn - ex) >> 23) : 0u);
    const bool grid = (sh < 24u) ? ((ua & ((1u << sh) - 1u)) == 0u) : (ua == 0u);
    const bool win = (ua == 0u) || (ua >= 0x20800000u /*2^-62*/ && ua <= 0x58800000u /*2^50*/);
    m = (ua >> (23 - M)) & ((1u << M) - 1u);
    c = (ua == 0u || (!s2n && sub)) ? 0.0f : __uint_as_float(u & 0xFF800000u);
    return grid && win;
}

// Writes one thread's TM x TN outputs (rows m0 + ty*TM + i, columns n0 + tx*TN + j) to the
// output mapping, or to its split-K partial slice (same layout); applies the fused BN/activation
// epilogue when unsplit.
// EMIT = false compiles the word-image emission out (gemm_f8mx_kernel's non-emitting instances:
// the emission code alone pushed that kernel past its 80-VGPR budget).
// GELU = false: the GELU tail compiled out as well (gemm_f8mx_kernel's emitting instances).
// The quantizers and words here are the literal forms (gemm_f8mx_kernel's store_tile_xm has the fast ones).
// sc: the block's StoreCtx (unsplit launches; a split launch stores raw partials and reads none of it).
// -DFP8A_RAW_STORE_DIAG=1 (diagnostic build only, tools/gemm_bench.py --emit: DESIGN.md 3v): the emitting
// instances store the raw fp32 accumulators and nothing else -- no BN / activation, residual, quantizer, word
// or header record -- which bounds what the emitting store can cost.  Its results are wrong; it never ships.
#ifndef FP8A_RAW_STORE_DIAG
#define FP8A_RAW_STORE_DIAG 0
#endif
template <bool EMIT = true, bool GELU = true>
__device__ __forceinline__ void store_tile(const GemmArgs &p, int64_t split, int64_t m0, int64_t n0, int ty, int tx,
                                           float (&acc)[TM][TN], const StoreCtx &sc) {
    constexpr bool RAW = FP8A_RAW_STORE_DIAG && EMIT;
    const bool partial = p.splits > 1;
    float *const C = partial ? p.part + split * p.M * p.N : p.C;
    const int64_t ldc = partial ? p.N : p.ldc, ctot = partial ? p.N : p.ctot, coff = partial ? 0 : p.coff;
    const int64_t nb = n0 + tx * TN;
    if (!partial && !RAW && p.ep != nullptr) {  // fused BN + activation (split-K applies it in the reduction)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int64_t ch = p.coff + min<int64_t>(nb + j, p.N - 1);
#pragma unroll
            for (int i = 0; i < TM; ++i) acc[i][j] = epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, ch, acc[i][j]);
        }
    }
    const float pb = sc.pb;
    const GemmArgs &q = p;
    // word-image emission from each final value (the split-K reduction emits instead)
    const bool emit = EMIT && !RAW && !partial && p.em.w != nullptr;
    const EmitCtx &ec = sc.ec;
    const FqFast &pk = sc.pk;
    uint32_t sehi = 0, neg = 0;
    auto fin1 = [&](int64_t o, float v) {
        if (partial || RAW) return v;
        v = post1<GELU>(q, o, v, pb, pk);
        if (emit) emit1(q, ec, o, v, sehi, neg);
        return v;
    };
    auto fin4 = [&](int64_t o, float4 v) {
        if (partial || RAW) return v;
        v = post4<GELU>(q, o, v, pb, pk);
        if (emit) emit4(q, ec, o, v, sehi, neg);
        return v;
    };
    if (!p.nchw) {
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int64_t m = m0 + ty * TM + i;
            if (m >= p.M) continue;
            if (nb + TN <= p.N && ((ldc & 3) == 0) && ((((uintptr_t)C) & 15) == 0)) {
                *reinterpret_cast<float4 *>(&C[m * ldc + nb]) =
                    fin4(m * ldc + nb, make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]));
            } else {
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    if (nb + j < p.N) C[m * ldc + nb + j] = fin1(m * ldc + nb + j, acc[i][j]);
            }
        }
    } else {
        // NCHW: the thread's 4 rows are 4 consecutive pixels; when they lie in one image and
        // start 16-B aligned, each output channel gets one float4 store.
        const int64_t mb = m0 + ty * TM;
        const int64_t img = mb / p.hw, pix = mb - img * p.hw;
        const bool vec = (pix + TM <= p.hw) && (mb + TM <= p.M) && ((p.hw & 3) == 0) &&
                         ((((uintptr_t)C) & 15) == 0);
        if (vec) {
#pragma unroll
            for (int j = 0; j < TN; ++j)
                if (nb + j < p.N) {
                    const int64_t o = (img * ctot + coff + nb + j) * p.hw + pix;
                    *reinterpret_cast<float4 *>(&C[o]) = fin4(o, make_float4(acc[0][j], acc[1][j], acc[2][j], acc[3][j]));
                }
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int64_t m = mb + i;
                if (m >= p.M) continue;
                const int64_t im = m / p.hw, px = m - im * p.hw;
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    if (nb + j < p.N) {
                        const int64_t o = (im * ctot + coff + nb + j) * p.hw + px;
                        C[o] = fin1(o, acc[i][j]);
                    }
            }
        }
    }
    if (emit) {
        wave_max_atomic(p.em.invalid + 5, sehi);
        wave_sign_record(p.em.invalid + 6, neg);
    }
}

// The final values of a split launch from its partial tiles (layout: row-major [M][N], or [img][N][hw] for an
// NCHW output), at partial index q: the splits summed in split order from slab 0, then BN / activation, the
// block tail and the emission -- four consecutive values (q % 4 == 0, the vector form's conditions:
// splitk_vec) or one.  splitk_reduce_kernel runs them over the whole output, the in-launch sum
// (gemm_f8mx_kernel) over its tile: one definition, so the two give the same bits.
__device__ __forceinline__ bool splitk_vec(const GemmArgs &p) {
    const bool vec = p.nchw ? ((p.hw & 3) == 0) : ((p.N & 3) == 0 && (p.ldc & 3) == 0);
    return vec && ((((uintptr_t)p.C) & 15) == 0) && ((((uintptr_t)p.part) & 15) == 0) && (((p.M * p.N) & 3) == 0) &&
           ((((uintptr_t)p.res) & 15) == 0);
}
template <bool EMIT, bool GELU, bool FQF>
__device__ __forceinline__ void splitk_finish4(const GemmArgs &p, const StoreCtx &sc, int64_t q, uint32_t &sehi,
                                               uint32_t &neg) {
    const int64_t MN = p.M * p.N;
    float4 acc = *reinterpret_cast<const float4 *>(p.part + q);
    for (int sp = 1; sp < p.splits; ++sp) {
        const float4 v = *reinterpret_cast<const float4 *>(p.part + sp * MN + q);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    int64_t o;
    if (p.nchw) {
        const int64_t img = q / (p.N * p.hw), rem = q - img * p.N * p.hw, n = rem / p.hw, pix = rem - n * p.hw;
        o = (img * p.ctot + p.coff + n) * p.hw + pix;
        if (p.ep) {  // the 4 values share channel coff + n (hw % 4 == 0)
            const int64_t ch = p.coff + n;
            acc.x = epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, ch, acc.x);
            acc.y = epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, ch, acc.y);
            acc.z = epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, ch, acc.z);
            acc.w = epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, ch, acc.w);
        }
    } else {
        const int64_t m = q / p.N, n = q - m * p.N;
        o = m * p.ldc + n;
        if (p.ep) {
            acc.x = epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, p.coff + n, acc.x);
            acc.y = epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, p.coff + n + 1, acc.y);
            acc.z = epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, p.coff + n + 2, acc.z);
            acc.w = epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, p.coff + n + 3, acc.w);
        }
    }
    const float4 r = post4<GELU, FQF>(p, o, acc, sc.pb, sc.pk);
    *reinterpret_cast<float4 *>(p.C + o) = r;
    if (EMIT && p.em.w) emit4<FQF>(p, sc.ec, o, r, sehi, neg);
}
template <bool EMIT, bool GELU, bool FQF>
__device__ __forceinline__ void splitk_finish1(const GemmArgs &p, const StoreCtx &sc, int64_t q, uint32_t &sehi,
                                               uint32_t &neg) {
    const int64_t MN = p.M * p.N;
    float acc = p.part[q];
    for (int sp = 1; sp < p.splits; ++sp) acc += p.part[sp * MN + q];
    int64_t o, ch;
    if (p.nchw) {
        const int64_t img = q / (p.N * p.hw), rem = q - img * p.N * p.hw, n = rem / p.hw, pix = rem - n * p.hw;
        o = (img * p.ctot + p.coff + n) * p.hw + pix;
        ch = p.coff + n;
    } else {
        const int64_t m = q / p.N, n = q - m * p.N;
        o = m * p.ldc + n;
        ch = p.coff + n;
    }
    const float r = post1<GELU, FQF>(p, o, epi(p.ep, p.ep_act, p.ep_lo, p.ep_hi, ch, acc), sc.pb, sc.pk);
    p.C[o] = r;
    if (EMIT && p.em.w) emit1<FQF>(p, sc.ec, o, r, sehi, neg);
}
// ... over the BMT x BNT tile at (m0, n0), by the NT threads of its last-arriving block (every thread calls it)
template <bool EMIT, bool GELU, int BMT, int BNT, int NT>
__device__ __forceinline__ void splitk_finish_tile(const GemmArgs &p, int64_t m0, int64_t n0, int tid) {
    const StoreCtx sc = store_ctx<EMIT>(p);
    uint32_t sehi = 0, neg = 0;
    if (splitk_vec(p)) {
        // NCHW: quads of 4 consecutive pixels (rows), lanes along the rows; row-major: quads of 4 columns
#pragma unroll 1
        for (int e = tid; e < BMT * BNT / 4; e += NT) {
            int64_t m, n;
            if (p.nchw) {
                m = m0 + 4 * (e % (BMT / 4));
                n = n0 + e / (BMT / 4);
            } else {
                m = m0 + e / (BNT / 4);
                n = n0 + 4 * (e % (BNT / 4));
            }
            if (m >= p.M || n >= p.N) continue;
            const int64_t img = m / p.hw, pix = m - img * p.hw;
            const int64_t q = p.nchw ? (img * p.N + n) * p.hw + pix : m * p.N + n;
            splitk_finish4<EMIT, GELU, true>(p, sc, q, sehi, neg);
        }
    } else {
#pragma unroll 1
        for (int e = tid; e < BMT * BNT; e += NT) {
            const int64_t m = m0 + (p.nchw ? e % BMT : e / BNT), n = n0 + (p.nchw ? e / BMT : e % BNT);
            if (m >= p.M || n >= p.N) continue;
            const int64_t img = m / p.hw, pix = m - img * p.hw;
            splitk_finish1<EMIT, GELU, true>(p, sc, p.nchw ? (img * p.N + n) * p.hw + pix : m * p.N + n, sehi, neg);
        }
    }
    if (EMIT && p.em.w) {
        wave_max_atomic(p.em.invalid + 5, sehi);
        wave_sign_record(p.em.invalid + 6, neg);
    }
}

// (the context per call.  Kept as a forwarding overload: with the context built inside the function above,
// gemm_fast_kernel's instances came out with two scalar moves in another order)
template <bool EMIT = true, bool GELU = true>
__device__ __forceinline__ void store_tile(const GemmArgs &p, int64_t split, int64_t m0, int64_t n0, int ty, int tx,
                                           float (&acc)[TM][TN]) {
    StoreCtx sc{};
    if (p.splits <= 1) {
        sc.pb = post_bias(p);
        if (EMIT) sc.ec = emit_ctx(p);
    }
    store_tile<EMIT, GELU>(p, split, m0, n0, ty, tx, acc, sc);
}

}  // namespace fp8a
