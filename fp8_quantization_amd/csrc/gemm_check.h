// gemm_check.h -- the fused self-check (the reference's self_check_mode, approx_matmul_whole_v9.py:
// 119-157): one pass over K that sums, per output (m, n) and in the same k order,
//   C = sum_k v_k    the approx term of Appendix A (exact_term, fp8approx_device.h),
//   G = sum_k g_k    the golden term fl32(a b), through Q_R when quant_btw_mult_accu (v9:30-36),
//   S = sum_k |v_k|  the project's tolerance scale,
// and reduces the error statistics of fp8a_check_stats (include/fp8approx.h) on the device.
//
// A literal kernel on purpose: it shares no code with the production GEMM paths it cross-checks
// (matrix-core, tile-table, depthwise, batched) beyond the element codecs of fp8approx_device.h, and
// G comes from its definition -- any fp32 operand, on the FP8 grid or off it.
//
// One kernel body, gemm_check_kernel, for all three entries (fp8a_matmul_check, fp8a_bmm_check,
// fp8a_conv2d_check): the per-product term is stated here once.  What it walks is a list of units -- the
// one matrix product, the nb0 x nb1 batch items, or the convolution groups -- each an offset into A, B,
// bB and the output (CheckArgs).  The two forms differ in the rows of this table only, and are the two
// instances of template <bool CONV> (one kernel branching at run time measured 1 % slower on attention's
// PV shape than the batched kernel it replaced):
//                   matrix / batched form                        convolution form
//   A               A + u0 sa0 + u1 sa1 + m lda + k,             implicit-im2col rows of the NCHW input,
//                   (u0, u1) = (u / nb1, u % nb1)                input channels from u cig
//   B               B + u0 sb0 + u1 sb1, by sbk, sbn             B + u b_gs, by sbk, sbn
//   bB              every unit alike                             bB + u bb_gs
//   output o        u M N + m ldc + n (items: dense, ldc = N)    (img ctot + u cog + n) hw + pix
//   S index os      (u M + m) N + n                              o
//
// Tiling: a workgroup of 256 threads owns a 64 x 64 output tile of one unit (thread = 4 x 4 outputs,
// three fp32 accumulators each) and walks K in steps of 16; the grid is flat, workgroup b = (unit
// b / tiles, tile b % tiles).  Every step stages 64 x 16 A and 16 x 64 B elements through LDS,
// decoded ONCE per element -- the value, 1 + mant 2^-M and a packed (expo, subnormal flag, mant)
// word -- so a product costs the multiply, the table entry, the scale and the two Q_R, not two
// operand decodes.
//
// Statistics: every workgroup reduces its threads' partials in LDS in a fixed tree order and
// writes CheckPart b to the workspace; check_reduce_kernel (one workgroup) sums the parts in a
// fixed order.  No floating-point atomics anywhere: two runs give identical bytes.
#pragma once
#include <float.h>

#include "fp8approx_common.h"

namespace fp8a {

constexpr int CK_BM = 64, CK_BN = 64, CK_BK = 16, CK_NT = 256, CK_P = 68;  // (CK_P: padded LDS row)

// One workgroup's share of fp8a_check_stats.
struct CheckPart {
    double sum_err, sum_err2, sum_gold2;
    unsigned long long a_norm, b_norm, r_norm;
    float max_err, prod_max_abs, prod_max_rel;
    uint32_t pad;
};

// Everything the check reads (the header's table); fields of the other form stay zero.
struct CheckArgs {
    const float *A, *B;  // A: the matrices, or the convolution's NCHW input
    float *C, *G, *S;    // G: golden sums in C's layout, or nullptr; S: sum_k |v_k| (the workspace's head)
    const float *Cprod;  // the production result in C's layout, or nullptr
    fp8a_check_stats *stats;
    CheckPart *part;     // [units * tiles]
    int64_t units, tiles, tiles_n;  // tiles per unit / its column tiles: tile = tile_m * tiles_n + tile_n
    int64_t M, N, K;     // one unit's extents
    int64_t sbk, sbn;
    // matrix / batched form
    int64_t nb1, lda, sa0, sa1, sb0, sb1, ldc;
    // convolution form
    int conv;
    int64_t b_gs, bb_gs, cig, cog, ctot;
    int64_t Cin, H, W, Ho, Wo;
    int kh, kw, sh, sw, ph, pw, dh, dw;
    int E, Mw;
    const int32_t *bA, *bB;
    int64_t bBs;
    const int32_t *bR;
    uint32_t flags;
    TablePack tab;
};

#if FP8A_OWN_CHECK
// A(m, k) of one unit: A = the unit's matrix, or the input with the unit's channels from cbase.
template <bool CONV>
__device__ __forceinline__ float check_load_A(const CheckArgs &p, const float *A, int64_t cbase, int64_t m, int64_t k) {
    if (!CONV) return A[m * p.lda + k];
    const int64_t hw = p.Ho * p.Wo, img = m / hw, pix = m - img * hw;
    const int64_t ho = pix / p.Wo, wo = pix - ho * p.Wo;
    const int64_t taps = (int64_t)p.kh * p.kw, c = k / taps, t = k - c * taps, ky = t / p.kw, kx = t - ky * p.kw;
    const int64_t hi = ho * p.sh - p.ph + ky * p.dh, wi = wo * p.sw - p.pw + kx * p.dw;
    if (hi < 0 || hi >= p.H || wi < 0 || wi >= p.W) return 0.0f;
    return A[((img * p.Cin + cbase + c) * p.H + hi) * p.W + wi];
}

// The decode of one staged operand element (v9:47-59): the s2n scale-up of a subnormal, then DEC.
// word = expo << 8 | subnormal << 7 | table index of mant;  fac = 1 + mant 2^-M (mult_result_mant's
// factor, v9:182).
__device__ __forceinline__ void check_decode(float x, const DFmt &f, bool s2n, float &fac, int &word, bool &normal) {
    const bool sub = fabsf(x) < f.mn;
    const float x2 = (s2n && sub) ? x * (float)(1 << f.M) : x;
    int e, m;
    exact_dec(x2, f, false, e, m);
    fac = 1.0f + (float)m * p2(-f.M);
    // (a tensor-bias zero decodes to mant = -2^M: the table is indexed as torch indexes, from the end)
    const int idx = m < 0 ? m + (1 << f.M) : m;
    word = (int)(((uint32_t)e << 8) | (sub ? 0x80u : 0u) | ((uint32_t)idx & 0x7Fu));
    normal = !sub;
}

template <typename T, typename Op>
__device__ __forceinline__ T check_block_reduce(T v, T *scratch, Op op) {
    const int t = threadIdx.x;
    __syncthreads();
    scratch[t] = v;
    __syncthreads();
    for (int s = CK_NT / 2; s > 0; s >>= 1) {
        if (t < s) scratch[t] = op(scratch[t], scratch[t + s]);
        __syncthreads();
    }
    return scratch[0];
}

template <bool CONV>
__global__ __launch_bounds__(CK_NT) void gemm_check_kernel(const CheckArgs p) {
    __shared__ float a_val[CK_BK][CK_P], a_fac[CK_BK][CK_P], b_val[CK_BK][CK_P], b_fac[CK_BK][CK_P];
    __shared__ int a_wrd[CK_BK][CK_P], b_wrd[CK_BK][CK_P];
    __shared__ float tabf[1024];  // 2^-M * table entry (the subtrahend of v9:182)
    __shared__ double red[CK_NT];

    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t u = (int64_t)blockIdx.x / p.tiles, tile = (int64_t)blockIdx.x - u * p.tiles;
    const int64_t tile_m = tile / p.tiles_n, tile_n = tile - tile_m * p.tiles_n;
    const int64_t m0 = tile_m * CK_BM, n0 = tile_n * CK_BN;
    // the unit's operands and output (the header's table)
    const int64_t u0 = CONV ? 0 : u / p.nb1, u1 = u - u0 * p.nb1;
    const float *const Au = CONV ? p.A : p.A + u0 * p.sa0 + u1 * p.sa1;
    const float *const Bg = CONV ? p.B + u * p.b_gs : p.B + u0 * p.sb0 + u1 * p.sb1;
    const int32_t *const bBg = p.bB + u * p.bb_gs;  // (bb_gs = 0: every matrix unit alike)
    const int64_t cbase = u * p.cig, coff = u * p.cog, hw = p.Ho * p.Wo;

    const uint32_t flags = p.flags;
    const bool tb = flags & F_TB, s2n = flags & F_S2N, qbma = flags & F_QBMA, gclip = flags & F_GCLIP;
    const bool approx = flags & F_APPROX;
    const int M = p.Mw, nm = 1 << M;
    const DFmt fA = dfmt(p.E, M, *p.bA, tb), fR = dfmt(p.E, M, *p.bR, tb);
    const float scale = (float)nm, ulp = p2(-M);

    for (int i = tid; i < nm * nm; i += CK_NT) tabf[i] = ulp * (float)p.tab.raw[i];

    // this thread's four columns: the exponent offset bA + bB - bR of each (v9:66)
    int bsum[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t n = min(n0 + tx * 4 + j, p.N - 1);
        bsum[j] = fA.b + bBg[n * p.bBs] - fR.b;
    }

    float accC[4][4], accG[4][4], accS[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) accC[i][j] = accG[i][j] = accS[i][j] = 0.0f;
    unsigned long long an = 0, bn = 0, rn = 0;
    // the operand matrices are counted once: A by the first column tile, B by the first row tile
    const bool count_a = tile_n == 0, count_b = tile_m == 0;
    // staging order: the faster thread index runs along the operand's unit-stride dimension
    const bool a_mfast = CONV, b_kfast = p.sbk == 1;

    for (int64_t k0 = 0; k0 < p.K; k0 += CK_BK) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = tid + r * CK_NT;  // 0 .. 1023
            {   // A element (mi, ki)
                const int mi = a_mfast ? (e & 63) : (e >> 4), ki = a_mfast ? (e >> 6) : (e & 15);
                const int64_t m = m0 + mi, k = k0 + ki;
                const bool in = m < p.M && k < p.K;
                const float v = in ? check_load_A<CONV>(p, Au, cbase, m, k) : 0.0f;
                float fac;
                int w;
                bool normal;
                check_decode(v, fA, s2n, fac, w, normal);
                a_val[ki][mi] = v;
                a_fac[ki][mi] = fac;
                a_wrd[ki][mi] = w;
                if (count_a && in && normal) ++an;
            }
            {   // B element (ki, ni)
                const int ni = b_kfast ? (e >> 4) : (e & 63), ki = b_kfast ? (e & 15) : (e >> 6);
                const int64_t n = n0 + ni, k = k0 + ki;
                const bool in = n < p.N && k < p.K;
                const DFmt fB = dfmt(p.E, M, bBg[min(n, p.N - 1) * p.bBs], tb);
                const float v = in ? Bg[k * p.sbk + n * p.sbn] : 0.0f;
                float fac;
                int w;
                bool normal;
                check_decode(v, fB, s2n, fac, w, normal);
                b_val[ki][ni] = v;
                b_fac[ki][ni] = fac;
                b_wrd[ki][ni] = w;
                if (count_b && in && normal) ++bn;
            }
        }
        __syncthreads();
        const int kend = (int)min<int64_t>(CK_BK, p.K - k0);  // (no padded k: a TB zero is not a zero term)
        uint32_t rn_tile = 0;
        for (int kk = 0; kk < kend; ++kk) {
            const float4 av = *reinterpret_cast<const float4 *>(&a_val[kk][ty * 4]);
            const float4 af = *reinterpret_cast<const float4 *>(&a_fac[kk][ty * 4]);
            const int4 aw = *reinterpret_cast<const int4 *>(&a_wrd[kk][ty * 4]);
            const float4 bv = *reinterpret_cast<const float4 *>(&b_val[kk][tx * 4]);
            const float4 bf = *reinterpret_cast<const float4 *>(&b_fac[kk][tx * 4]);
            const int4 bw = *reinterpret_cast<const int4 *>(&b_wrd[kk][tx * 4]);
            const float a4[4] = {av.x, av.y, av.z, av.w}, fa4[4] = {af.x, af.y, af.z, af.w};
            const float b4[4] = {bv.x, bv.y, bv.z, bv.w}, fb4[4] = {bf.x, bf.y, bf.z, bf.w};
            const int wa4[4] = {aw.x, aw.y, aw.z, aw.w}, wb4[4] = {bw.x, bw.y, bw.z, bw.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int eA = wa4[i] >> 8, mA = wa4[i] & 0x7F;
                const bool as = (wa4[i] & 0x80) != 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int eB = wb4[j] >> 8, mB = wb4[j] & 0x7F;
                    const bool bs = (wb4[j] & 0x80) != 0;
                    // golden (v9:30-36)
                    float g = a4[i] * b4[j];
                    const bool zero = (g == 0.0f);
                    if (qbma) g = exact_q(g, fR, gclip);
                    // approx (v9:66-108), exact_term with the operand decodes hoisted
                    const int aexp = eA + eB - bsum[j];
                    const float sgn = (g < 0.0f) ? -1.0f : 1.0f;
                    float mp = fa4[i] * fb4[j];
                    if (approx) mp = mp - tabf[mA * nm + mB];
                    float v;
                    if (s2n) {
                        v = p2(aexp - fR.b) * mp * sgn;
                        if (as) v = v / scale;
                        if (bs) v = v / scale;
                        if (zero) v = 0.0f;
                    } else {
                        const bool norm = (eA > 0) && (eB > 0) && (fabsf(g) >= fR.mn);
                        v = norm ? p2(aexp - fR.b) * mp * sgn : g;
                        const bool inside = (m0 + ty * 4 + i < p.M) && (n0 + tx * 4 + j < p.N);
                        rn_tile += (norm && inside) ? 1u : 0u;
                    }
                    if (qbma) v = exact_q(v, fR, gclip);
                    accC[i][j] += v;
                    accG[i][j] += g;
                    accS[i][j] += fabsf(v);
                }
            }
        }
        rn += rn_tile;
    }

    // stores and this thread's error partials (outputs in (i, j) order)
    double se = 0.0, se2 = 0.0, sg2 = 0.0;
    float me = 0.0f, pa = 0.0f, pr = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int64_t m = m0 + ty * 4 + i;
        if (m >= p.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t n = n0 + tx * 4 + j;
            if (n >= p.N) continue;
            int64_t o, os;  // index in C's layout / in the dense S image
            if (!CONV) {
                os = (u * p.M + m) * p.N + n;
                o = u * p.M * p.N + m * p.ldc + n;  // (ldc = N wherever there is more than one unit)
            } else {
                const int64_t img = m / hw, pix = m - img * hw;
                o = os = (img * p.ctot + coff + n) * hw + pix;
            }
            const float cv = accC[i][j], gv = accG[i][j];
            p.C[o] = cv;
            if (p.G) p.G[o] = gv;
            p.S[os] = accS[i][j];
            const float e = fabsf(gv - cv);  // (fp32, as v9:146)
            me = fmaxf(me, e);
            se += (double)e;
            se2 += (double)e * (double)e;
            sg2 += (double)gv * (double)gv;
            if (p.Cprod) {
                const float d = fabsf(p.Cprod[o] - cv);
                pa = fmaxf(pa, d);
                pr = fmaxf(pr, d / fmaxf(accS[i][j], FLT_MIN));
            }
        }
    }
    auto addd = [](double x, double y) { return x + y; };
    auto addu = [](unsigned long long x, unsigned long long y) { return x + y; };
    auto maxf = [](float x, float y) { return fmaxf(x, y); };
    unsigned long long *const redu = reinterpret_cast<unsigned long long *>(red);
    float *const redf = reinterpret_cast<float *>(red);
    CheckPart out;
    out.sum_err = check_block_reduce(se, red, addd);
    out.sum_err2 = check_block_reduce(se2, red, addd);
    out.sum_gold2 = check_block_reduce(sg2, red, addd);
    out.a_norm = check_block_reduce(an, redu, addu);
    out.b_norm = check_block_reduce(bn, redu, addu);
    out.r_norm = check_block_reduce(rn, redu, addu);
    out.max_err = check_block_reduce(me, redf, maxf);
    out.prod_max_abs = check_block_reduce(pa, redf, maxf);
    out.prod_max_rel = check_block_reduce(pr, redf, maxf);
    out.pad = 0;
    if (tid == 0) p.part[blockIdx.x] = out;
}

// Sums the workgroups' parts in a fixed order (thread t takes parts t, t + 256, ...; then the LDS
// tree) and fills the stats struct.  One workgroup.
__global__ __launch_bounds__(CK_NT) void check_reduce_kernel(const CheckArgs c, int64_t nparts, int64_t M, int64_t N,
                                                             int64_t K, uint32_t flags) {
    __shared__ double red[CK_NT];
    double se = 0.0, se2 = 0.0, sg2 = 0.0;
    unsigned long long an = 0, bn = 0, rn = 0;
    float me = 0.0f, pa = 0.0f, pr = 0.0f;
    for (int64_t i = threadIdx.x; i < nparts; i += CK_NT) {
        const CheckPart q = c.part[i];
        se += q.sum_err;
        se2 += q.sum_err2;
        sg2 += q.sum_gold2;
        an += q.a_norm;
        bn += q.b_norm;
        rn += q.r_norm;
        me = fmaxf(me, q.max_err);
        pa = fmaxf(pa, q.prod_max_abs);
        pr = fmaxf(pr, q.prod_max_rel);
    }
    auto addd = [](double x, double y) { return x + y; };
    auto addu = [](unsigned long long x, unsigned long long y) { return x + y; };
    auto maxf = [](float x, float y) { return fmaxf(x, y); };
    unsigned long long *const redu = reinterpret_cast<unsigned long long *>(red);
    float *const redf = reinterpret_cast<float *>(red);
    se = check_block_reduce(se, red, addd);
    se2 = check_block_reduce(se2, red, addd);
    sg2 = check_block_reduce(sg2, red, addd);
    an = check_block_reduce(an, redu, addu);
    bn = check_block_reduce(bn, redu, addu);
    rn = check_block_reduce(rn, redu, addu);
    me = check_block_reduce(me, redf, maxf);
    pa = check_block_reduce(pa, redf, maxf);
    pr = check_block_reduce(pr, redf, maxf);
    if (threadIdx.x != 0) return;
    const unsigned long long G = (unsigned long long)c.units;
    const bool s2n = flags & F_S2N;
    fp8a_check_stats st;
    st.n_out = G * (unsigned long long)M * (unsigned long long)N;
    st.sum_err = se;
    st.sum_err2 = se2;
    st.sum_gold2 = sg2;
    st.a_norm = an;
    st.a_total = G * (unsigned long long)M * (unsigned long long)K;
    st.b_norm = bn;
    st.b_total = G * (unsigned long long)K * (unsigned long long)N;
    st.r_norm = s2n ? 0ull : rn;
    st.r_total = s2n ? 0ull : G * (unsigned long long)M * (unsigned long long)N * (unsigned long long)K;
    st.max_err = me;
    st.prod_max_abs = pa;
    st.prod_max_rel = pr;
    st.has_prod = c.Cprod != nullptr ? 1u : 0u;
    *c.stats = st;
}

#endif  // FP8A_OWN_CHECK

}  // namespace fp8a
