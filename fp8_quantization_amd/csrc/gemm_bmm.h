// gemm_bmm.h -- the batched approx product (fp8a_bmm, gemm_bmm_kernel): activation x activation, batched
// over two leading dims with two strides per operand, so attention's per-head operands are read straight
// out of [B, S, H*d] buffers; compiled only in k_bmm.hip.
//
// One workgroup owns one 64 x 64 output tile of one batch item.  The per-term arithmetic is
// gemm_fast_kernel's (gemm_fast.h), table mode by table mode -- the same shared helpers (stage_decode,
// make_qc / q_fast, TablePack's modes) and the same k order -- and the TM_F8 form (LDS term LUT + scaled
// hardware conversion as Q_R) also runs E5M2 through the bf8 conversions (BF8).  What differs is the
// off-grid handling: there is no flag arena, no unit mark and no second launch.  A workgroup whose staging
// saw an operand or bias outside the fast forms' window (or, TM_F8, a non-finite sum: a term beyond the
// hardware format's range) recomputes its own tile with exact_term after a workgroup-uniform branch, and
// counts itself in *recount (one atomic per recomputed tile, none otherwise): capture-safe by construction.
#pragma once
#include "fp8approx_common.h"

namespace fp8a {

struct BmmArgs {
    const float *A, *B;
    float *C;
    int64_t nb1;             // the inner batch extent: batch item z = (z / nb1, z % nb1)
    int64_t M, N, K;
    int64_t lda, sa0, sa1;   // A(i0, i1, m, k) = A[i0 sa0 + i1 sa1 + m lda + k]
    int64_t sbk, sbn, sb0, sb1;
    int64_t ldc, sc0, sc1;
    int64_t num_mt, tiles;   // row tiles / tiles per batch item; block b = (tile b % tiles, item b / tiles)
    int E, Mw;
    uint32_t kexp, kdc;      // as GemmArgs: opaque SGPR operands of q_fast
    const int32_t *bA, *bB;
    int64_t bBs;
    const int32_t *bR;
    uint32_t flags;
    unsigned long long *recount;  // tiles recomputed exactly (k_bmm.hip part 0's counter)
    TablePack tab;
};

// k_bmm.hip, part P = 2 * S2N + QBMA (as k_fast.hip): gemm_bmm_kernel<S2N, QBMA, gclip, mode> for the table
// modes TM_NONE .. TM_LUT; part 3 also the TM_F8 forms (E4M3: Mw 3, E5M2: Mw 2; s2n + qbma, no golden clip).
void launch_bmm_p0(int mode, bool gclip, const BmmArgs &a, dim3 grid, hipStream_t s);
void launch_bmm_p1(int mode, bool gclip, const BmmArgs &a, dim3 grid, hipStream_t s);
void launch_bmm_p2(int mode, bool gclip, const BmmArgs &a, dim3 grid, hipStream_t s);
void launch_bmm_p3(int mode, bool gclip, const BmmArgs &a, dim3 grid, hipStream_t s);
// the device address of the recomputed-tile counter (nullptr: the query failed), and its value
unsigned long long *bmm_recount_ptr();
int bmm_recount_read(unsigned long long *v, bool reset);

#if FP8A_OWN_BMM
template <bool S2N, bool QBMA, bool GCLIP, int TMODE, bool BF8>
__global__ __launch_bounds__(NT) void gemm_bmm_kernel(const BmmArgs p) {
    constexpr bool F8 = TMODE == TM_F8;
    constexpr bool TBL = TMODE != TM_NONE && !F8;
    constexpr int R = (TMODE == TM_W2S2 || TMODE == TM_W2U2) ? 2 : 1;
    constexpr bool SGN = (TMODE == TM_W2S1 || TMODE == TM_W2S2 || TMODE == TM_LUT);
    constexpr int FM = BF8 ? 2 : 3;   // TM_F8: the format's mantissa width, 2^FM codes per LUT row
    constexpr int FN = 1 << FM;

    __shared__ __attribute__((aligned(16))) float sA[BK][AP];
    __shared__ __attribute__((aligned(16))) float sB[BK][BP];
    __shared__ __attribute__((aligned(16))) float sAc[TBL ? BK : 1][AP];
    __shared__ __attribute__((aligned(16))) uint32_t sAr[(TBL || F8) ? R * BK : 1][AP];
    __shared__ __attribute__((aligned(16))) float sBc[TBL ? BK : 1][BP];
    __shared__ __attribute__((aligned(16))) uint32_t sBm[(TBL || F8) ? BK : 1][BP];
    // TM_F8: V'(sign a, m_a, m_b), 2 signs x 2^FM codes + a zero row, 16 floats per row (two 8-entry
    // copies on disjoint banks, as gemm_fast_kernel's)
    __shared__ __attribute__((aligned(16))) float sF8[F8 ? (2 * FN + 1) * 16 : 1];
    __shared__ float sLut[TMODE == TM_LUT ? 1024 : 1];
    __shared__ uint32_t sRows[TBL ? 64 * 2 : 1];

    const int tid = threadIdx.x;
    const int ty = tid >> 4, tx = tid & 15;
    const int64_t bid = (int64_t)blockIdx.x % p.tiles, z = (int64_t)blockIdx.x / p.tiles;
    const int64_t m0 = (bid % p.num_mt) * BM;  // consecutive blocks: one batch item, one column tile
    const int64_t n0 = (bid / p.num_mt) * BN;  // (its B panel is shared)
    const int64_t i0 = z / p.nb1, i1 = z - i0 * p.nb1;
    const float *const A = p.A + i0 * p.sa0 + i1 * p.sa1;
    const float *const B = p.B + i0 * p.sb0 + i1 * p.sb1;
    float *const C = p.C + i0 * p.sc0 + i1 * p.sc1;
    const int64_t K = p.K;

    float acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = 0.0f;

    const int M = p.Mw;
    int anybad = 0;
    if (K > 0) {  // (K = 0: the sum over an empty axis, zeros; nothing but C is read)
        const int bA = *p.bA, bR = *p.bR;
        const QC qc = make_qc(p.E, M, bR, p.kexp, p.kdc);
        const uint32_t emnA = (uint32_t)(128 - bA) << 23;
        const float ulpM = p2(-M);
        // TM_F8 Q_R: the result grid of bias bR is the OCP e4m3 (bf8: e5m2) grid scaled by 2^(XB - bR),
        // XB = 7 (15), so Q_R(y) = 2^(XB-bR) cvt(y / 2^(XB-bR)) for y clamped to Q_R's bound (folded into
        // V'); a term beyond the hardware format's range comes back NaN (bf8: infinite) and the tile is
        // recomputed
        constexpr int XB = BF8 ? 15 : 7;
        const float f8S = F8 ? __uint_as_float((uint32_t)min(max(127 + XB - bR, 1), 254) << 23) : 0.0f;
        if (F8) {
            for (int e = tid; e < (2 * FN + 1) * 16; e += NT) {
                const int r = e >> 4, mb = e & (FN - 1);
                float v = 0.0f;
                if (r < 2 * FN) {
                    const int ma = r & (FN - 1);
                    const float u = p2(-FM);
                    const float t = (float)p.tab.raw[ma * FN + mb];
                    v = __fmaf_rn(1.0f + u * ma, 1.0f + u * mb, -t * u);  // exact
                    // Q_R's pre-clamp bound 2^e (2 - 2^-M - 2^-22) (QC::kb)
                    v = fminf(v, __uint_as_float(__float_as_uint(v) & 0x7F800000u) * (2.0f - u - p2(-22)));
                    if (r >= FN) v = -v;
                }
                sF8[e] = v;
            }
            __syncthreads();
        }
        if (TBL) {
            const int n = 1 << M;
            for (int i = tid; i < n * 2; i += NT) sRows[i] = p.tab.rows[i >> 1][i & 1];
            if (TMODE == TM_LUT)
                for (int i = tid; i < n * n; i += NT) sLut[i] = (float)p.tab.raw[i];
            __syncthreads();
        }

        // B staging map: n-contiguous B (V) reads along n, else (K^T: k-contiguous) along k
        const bool b_ncontig = (p.sbn == 1);
        int bcol[4], bkk[4];
        uint32_t emnB[4];
        bool bias_ok = bR >= -100 && bR <= 120 && bA >= -100 && bA <= 120;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = tid + NT * r;
            bcol[r] = b_ncontig ? (e & 63) : (e >> 4);
            bkk[r] = b_ncontig ? (e >> 6) : (e & 15);
            const int64_t n = n0 + bcol[r];
            const int bb = (n < p.N) ? p.bB[n * p.bBs] : 0;
            bias_ok = bias_ok && bb >= -100 && bb <= 120;
            emnB[r] = (uint32_t)(128 - bb) << 23;
        }
        int arow[4], akk[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = tid + NT * r;
            arow[r] = e >> 4;  // lanes along k (row-major A)
            akk[r] = e & 15;
        }
        float xa[4], xb[4];
        // global -> registers for the step at k0 (issued one step ahead of its use); scalar loads, so a
        // ragged K and any alignment of the head views take the same path
        auto load_tile = [&](int64_t k0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t m = m0 + arow[r], k = k0 + akk[r];
                xa[r] = (m < p.M && k < K) ? A[m * p.lda + k] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int64_t n = n0 + bcol[r], k = k0 + bkk[r];
                xb[r] = (n < p.N && k < K) ? B[k * p.sbk + n * p.sbn] : 0.0f;
            }
        };
        load_tile(0);

        for (int64_t k0 = 0; k0 < K; k0 += BK) {
            bool bad = !bias_ok;
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // ---- decode + stage A (64 x 16)
                const int row = arow[r], kk = akk[r];
                const float x = xa[r];
                float c;
                uint32_t mc;
                if (F8) {
                    // cvt scale 2^(XB-bR) / |c| and the byte offset of the LUT row
                    bad |= !stage_decode(x, M, emnA, true, c, mc);
                    const uint32_t cb = __float_as_uint(c);
                    const int se = 254 + XB - bR - (int)((cb >> 23) & 0xFFu);
                    const bool zero = (cb & 0x7FFFFFFFu) == 0u;
                    bad |= !zero && (se < 1 || se > 254);
                    sA[kk][row] = zero ? f8S : __uint_as_float((uint32_t)min(max(se, 1), 254) << 23);
                    const uint32_t rr = zero ? (uint32_t)(2 * FN) : ((cb >> 31) * (uint32_t)FN + mc);
                    sAr[kk][row] = (rr * 16u + (uint32_t)((row >> 2) & 1) * 8u) * 4u;
                    continue;
                }
                bad |= !stage_decode(x, M, emnA, S2N, c, mc);
                sA[kk][row] = x;
                if (TBL) {
                    sAc[kk][row] = c * ulpM;
                    if (TMODE == TM_LUT) {
                        sAr[kk][row] = mc << M;
                    } else {
                        sAr[kk][row] = sRows[mc * 2];
                        if (R == 2) sAr[BK + kk][row] = sRows[mc * 2 + 1];
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {  // ---- decode + stage B (16 x 64)
                const int col = bcol[r], kk = bkk[r];
                const float x = xb[r];
                float c;
                uint32_t mc;
                if (F8) {
                    bad |= !stage_decode(x, M, emnB[r], true, c, mc);
                    sB[kk][col] = c;
                    sBm[kk][col] = mc * 4u;
                    continue;
                }
                bad |= !stage_decode(x, M, emnB[r], S2N, c, mc);
                sB[kk][col] = x;
                if (TBL) {
                    sBc[kk][col] = c;
                    sBm[kk][col] = (TMODE == TM_LUT || TMODE == TM_W1U) ? mc : mc * 2u;
                }
            }
            anybad |= __syncthreads_or(bad ? 1 : 0);
            if (k0 + BK < K) load_tile(k0 + BK);  // the next step's loads fly during this step's math

#pragma unroll 2
            for (int kk = 0; kk < BK; ++kk) {
                const float4 a4 = *reinterpret_cast<const float4 *>(&sA[kk][ty * TM]);
                const float4 b4 = *reinterpret_cast<const float4 *>(&sB[kk][tx * TN]);
                const float a[TM] = {a4.x, a4.y, a4.z, a4.w};
                const float b[TN] = {b4.x, b4.y, b4.z, b4.w};
                if (F8) {
                    const uint4 ia4 = *reinterpret_cast<const uint4 *>(&sAr[kk][ty * TM]);
                    const uint4 ib4 = *reinterpret_cast<const uint4 *>(&sBm[kk][tx * TN]);
                    const uint32_t ia[TM] = {ia4.x, ia4.y, ia4.z, ia4.w};
                    const uint32_t ib[TN] = {ib4.x, ib4.y, ib4.z, ib4.w};
                    const char *lut = reinterpret_cast<const char *>(sF8);
#pragma unroll
                    for (int i = 0; i < TM; ++i) {
                        float xv[TN];
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            xv[j] = *reinterpret_cast<const float *>(lut + (ia[i] + ib[j])) * b[j];
                        typedef short s2 __attribute__((ext_vector_type(2)));
                        s2 code;
                        if (BF8) {
                            code = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32((s2){0, 0}, xv[0], xv[1], a[i], false);
                            code = __builtin_amdgcn_cvt_scalef32_pk_bf8_f32(code, xv[2], xv[3], a[i], true);
                        } else {
                            code = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32((s2){0, 0}, xv[0], xv[1], a[i], false);
                            code = __builtin_amdgcn_cvt_scalef32_pk_fp8_f32(code, xv[2], xv[3], a[i], true);
                        }
                        const uint32_t cu = __builtin_bit_cast(uint32_t, code);
                        const auto lo = BF8 ? __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(cu, f8S, false)
                                            : __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(cu, f8S, false);
                        const auto hi = BF8 ? __builtin_amdgcn_cvt_scalef32_pk_f32_bf8(cu, f8S, true)
                                            : __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(cu, f8S, true);
                        acc[i][0] += lo[0];
                        acc[i][1] += lo[1];
                        acc[i][2] += hi[0];
                        acc[i][3] += hi[1];
                    }
                } else if (!TBL) {
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            const float g = a[i] * b[j];
                            acc[i][j] += QBMA ? q_fast<GCLIP, true>(g, qc) : g;
                        }
                } else {
                    const float4 ac4 = *reinterpret_cast<const float4 *>(&sAc[kk][ty * TM]);
                    const uint4 ar4 = *reinterpret_cast<const uint4 *>(&sAr[kk][ty * TM]);
                    const uint4 ar4h = (R == 2) ? *reinterpret_cast<const uint4 *>(&sAr[BK + kk][ty * TM]) : make_uint4(0, 0, 0, 0);
                    const float4 bc4 = *reinterpret_cast<const float4 *>(&sBc[kk][tx * TN]);
                    const uint4 bm4 = *reinterpret_cast<const uint4 *>(&sBm[kk][tx * TN]);
                    const float ac[TM] = {ac4.x, ac4.y, ac4.z, ac4.w};
                    const uint32_t ar0[TM] = {ar4.x, ar4.y, ar4.z, ar4.w};
                    const uint32_t ar1[TM] = {ar4h.x, ar4h.y, ar4h.z, ar4h.w};
                    const float bc[TN] = {bc4.x, bc4.y, bc4.z, bc4.w};
                    const uint32_t bm[TN] = {bm4.x, bm4.y, bm4.z, bm4.w};
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) {
                            // gemm_fast_kernel's table term: v0 = a b - t cA cB, exactly representable
                            const float cab = ac[i] * bc[j];
                            constexpr bool NEED_G = !S2N || (QBMA && SGN);
                            const float g = NEED_G ? a[i] * b[j] : 0.0f;
                            float v0;
                            if (TMODE == TM_W1U) {
                                const int t = __builtin_amdgcn_sbfe((int)ar0[i], bm[j], 1);
                                const float tc = __uint_as_float(__float_as_uint(cab) & (uint32_t)t);
                                v0 = NEED_G ? g - tc : __fmaf_rn(a[i], b[j], -tc);
                            } else {
                                float tf;
                                if (TMODE == TM_LUT) {
                                    tf = sLut[ar0[i] + bm[j]];
                                } else {
                                    const uint32_t w = (R == 2 && (bm[j] & 32u)) ? ar1[i] : ar0[i];
                                    const int t = SGN ? (int)__builtin_amdgcn_sbfe((int)w, bm[j], 2)
                                                      : (int)__builtin_amdgcn_ubfe(w, bm[j], 2);
                                    tf = (float)t;
                                }
                                v0 = NEED_G ? __fmaf_rn(-tf, cab, g) : __fmaf_rn(a[i], b[j], -(tf * cab));
                            }
                            if (!S2N) v0 = (fabsf(g) >= qc.mnR) ? v0 : g;  // norm mask, v9:87
                            if (S2N && QBMA && SGN) v0 = (g >= -qc.thr) ? fabsf(v0) : v0;  // F7
                            acc[i][j] += QBMA ? q_fast<GCLIP>(v0, qc) : v0;
                        }
                }
            }
            __syncthreads();
        }

        if (F8) {  // a term beyond the hardware format's range: NaN (bf8: +-inf, or their NaN sum)
            bool nf = false;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) nf |= !(fabsf(acc[i][j]) <= 3.0e38f);
            anybad |= __syncthreads_or(nf ? 1 : 0);
        }

        // ---- the tile saw an operand / bias / term outside the fast form's window: its own exact
        // recomputation, the reference's op sequence term by term in the same k order (workgroup-uniform)
        if (anybad) {
            if (tid == 0) atomicAdd(p.recount, 1ull);
            const DFmt fA = dfmt(p.E, M, bA, false), fR = dfmt(p.E, M, bR, false);
#pragma unroll 1
            for (int j = 0; j < TN; ++j) {
                const int64_t n = n0 + tx * TN + j;
                if (n >= p.N) continue;
                const DFmt fB = dfmt(p.E, M, p.bB[n * p.bBs], false);
#pragma unroll 1
                for (int i = 0; i < TM; ++i) {
                    const int64_t m = m0 + ty * TM + i;
                    if (m >= p.M) continue;
                    float s = 0.0f;
                    for (int64_t k = 0; k < K; ++k)
                        s += exact_term(A[m * p.lda + k], B[k * p.sbk + n * p.sbn], fA, fB, fR, p.tab.raw, p.flags);
                    // (a dynamic index: one select chain over the 16 accumulators, off the hot path)
#pragma unroll
                    for (int ii = 0; ii < TM; ++ii)
#pragma unroll
                        for (int jj = 0; jj < TN; ++jj)
                            if (ii == i && jj == j) acc[ii][jj] = s;
                }
            }
        }
    }

    // ---- store: row-major within the item; one 16-B store where the row's four columns allow
    const int64_t nb = n0 + tx * TN;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int64_t m = m0 + ty * TM + i;
        if (m >= p.M) continue;
        float *const row = C + m * p.ldc + nb;
        if (nb + TN <= p.N && (((uintptr_t)row) & 15) == 0) {
            *reinterpret_cast<float4 *>(row) = make_float4(acc[i][0], acc[i][1], acc[i][2], acc[i][3]);
        } else {
#pragma unroll
            for (int j = 0; j < TN; ++j)
                if (nb + j < p.N) row[j] = acc[i][j];
        }
    }
}
#endif  // FP8A_OWN_BMM

}  // namespace fp8a
