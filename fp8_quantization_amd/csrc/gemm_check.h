// gemm_check.h -- the fused self-check (the reference's self_check_mode, approx_matmul_whole_v9.py:
// 119-157): one pass over K that sums, per output (m, n) and in the same k order,
//   C = sum_k v_k    the approx term of Appendix A (exact_term, fp8approx_device.h),
//   G = sum_k g_k    the golden term fl32(a b), through Q_R when quant_btw_mult_accu (v9:30-36),
//   S = sum_k |v_k|  the project's tolerance scale,
// and reduces the error statistics of fp8a_check_stats (include/fp8approx.h) on the device.
//
// A literal kernel on purpose: it shares no code with the production GEMM paths it cross-checks
// (matrix-core, tile-table, depthwise) beyond the element codecs of fp8approx_device.h, and G comes
// from its definition -- any fp32 operand, on the FP8 grid or off it.
//
// Tiling: a workgroup of 256 threads owns a 64 x 64 output tile (thread = 4 x 4 outputs, three fp32
// accumulators each) and walks K in steps of 16.  Every step stages 64 x 16 A and 16 x 64 B
// elements through LDS, decoded ONCE per element -- the value, 1 + mant 2^-M and a packed (expo,
// subnormal flag, mant) word -- so a product costs the multiply, the table entry, the scale and the
// two Q_R, not two operand decodes.  A rows are matrix rows or implicit-im2col rows (GemmArgs, as
// load_A reads them); blockIdx.y is the convolution group.
//
// Statistics: every workgroup reduces its threads' partials in LDS in a fixed tree order and
// writes one CheckPart to the workspace; check_reduce_kernel (one workgroup) sums the parts in a
// fixed order.  No floating-point atomics anywhere: two runs give identical bytes.
//
// gemm_bmm_check_kernel (below) is the same pass over fp8a_bmm's batched operands.
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

struct CheckArgs {
    float *G;            // golden sums in C's layout, or nullptr
    float *S;            // sum_k |v_k|, dense in C's index space (workspace)
    const float *Cprod;  // the production result in C's layout, or nullptr
    fp8a_check_stats *stats;
    CheckPart *part;     // [groups * tiles]
    int64_t tiles_n;     // column tiles; blockIdx.x = tile_m * tiles_n + tile_n
    // convolution group g = blockIdx.y: B += g * b_gs, bB += g * bb_gs, input channels from g * cig,
    // output channels from g * cog
    int64_t b_gs, bb_gs, cig, cog;
    int groups;
};

#if FP8A_OWN_CHECK
__device__ __forceinline__ float check_load_A(const GemmArgs &p, int64_t cbase, int64_t m, int64_t k) {
    if (!p.conv) return p.A[m * p.lda + k];
    const int64_t hw = p.Ho * p.Wo, img = m / hw, pix = m - img * hw;
    const int64_t ho = pix / p.Wo, wo = pix - ho * p.Wo;
    const int64_t taps = (int64_t)p.kh * p.kw, c = k / taps, t = k - c * taps, ky = t / p.kw, kx = t - ky * p.kw;
    const int64_t hi = ho * p.sh - p.ph + ky * p.dh, wi = wo * p.sw - p.pw + kx * p.dw;
    if (hi < 0 || hi >= p.H || wi < 0 || wi >= p.W) return 0.0f;
    return p.X[((img * p.Cin + cbase + c) * p.H + hi) * p.W + wi];
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

__global__ __launch_bounds__(CK_NT) void gemm_check_kernel(const GemmArgs p, const CheckArgs c) {
    __shared__ float a_val[CK_BK][CK_P], a_fac[CK_BK][CK_P], b_val[CK_BK][CK_P], b_fac[CK_BK][CK_P];
    __shared__ int a_wrd[CK_BK][CK_P], b_wrd[CK_BK][CK_P];
    __shared__ float tabf[1024];  // 2^-M * table entry (the subtrahend of v9:182)
    __shared__ double red[CK_NT];

    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t grp = blockIdx.y;
    const int64_t tile_m = blockIdx.x / c.tiles_n, tile_n = blockIdx.x - tile_m * c.tiles_n;
    const int64_t m0 = tile_m * CK_BM, n0 = tile_n * CK_BN;
    const float *const Bg = p.B + grp * c.b_gs;
    const int32_t *const bBg = p.bB + grp * c.bb_gs;
    const int64_t cbase = grp * c.cig, coff = grp * c.cog;

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
    const bool a_mfast = p.conv != 0, b_kfast = p.sbk == 1;

    for (int64_t k0 = 0; k0 < p.K; k0 += CK_BK) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = tid + r * CK_NT;  // 0 .. 1023
            {   // A element (mi, ki)
                const int mi = a_mfast ? (e & 63) : (e >> 4), ki = a_mfast ? (e >> 6) : (e & 15);
                const int64_t m = m0 + mi, k = k0 + ki;
                const bool in = m < p.M && k < p.K;
                const float v = in ? check_load_A(p, cbase, m, k) : 0.0f;
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
            if (!p.nchw) {
                o = m * p.ldc + n;
                os = m * p.N + n;
            } else {
                const int64_t img = m / p.hw, pix = m - img * p.hw;
                o = os = (img * p.ctot + coff + n) * p.hw + pix;
            }
            const float cv = accC[i][j], gv = accG[i][j];
            p.C[o] = cv;
            if (c.G) c.G[o] = gv;
            c.S[os] = accS[i][j];
            const float e = fabsf(gv - cv);  // (fp32, as v9:146)
            me = fmaxf(me, e);
            se += (double)e;
            se2 += (double)e * (double)e;
            sg2 += (double)gv * (double)gv;
            if (c.Cprod) {
                const float d = fabsf(c.Cprod[o] - cv);
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
    if (tid == 0) c.part[grp * gridDim.x + blockIdx.x] = out;
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
    const unsigned long long G = (unsigned long long)c.groups;
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

// ------------------------------------------------------------------------- batched form
// gemm_bmm_check_kernel: the same pass over the batched product of fp8a_bmm (gemm_bmm.h) -- nb0 x nb1
// items with two batch strides per operand, read in place; C, G, Cprod and S dense [nb0][nb1][M][N].  One
// workgroup owns one 64 x 64 tile of one item; the grid is flat over (tile, item) in blockIdx.x, and
// part b is workgroup b's, so check_reduce_kernel (groups = items) walks them in the same fixed order.
// Int biases only (no tensor-bias semantics): bA, bR one value, bB shared or per column, every item alike.
struct BmmCheckArgs {
    const float *A, *B;
    float *C, *G, *S;        // G: nullptr or C's layout; S: the workspace's head
    const float *Cprod;      // the production result, dense like C, or nullptr
    CheckPart *part;         // [items * tiles]
    int64_t nb1;             // the inner batch extent: item z = (z / nb1, z % nb1)
    int64_t M, N, K;
    int64_t lda, sa0, sa1;   // A(i0, i1, m, k) = A[i0 sa0 + i1 sa1 + m lda + k]
    int64_t sbk, sbn, sb0, sb1;
    int64_t tiles_n, tiles;  // column tiles / tiles per item; block b = (tile b % tiles, item b / tiles)
    int E, Mw;
    const int32_t *bA, *bB;
    int64_t bBs;
    const int32_t *bR;
    uint32_t flags;
    TablePack tab;
};

// k_check.hip: the kernel over items * a.tiles workgroups, then check_reduce_kernel on c (part, stats, Cprod)
void launch_bmm_check(const BmmCheckArgs &a, const CheckArgs &c, int64_t items, hipStream_t s);

#if FP8A_OWN_CHECK
// One product from its staged decodes (gemm_check_kernel's per-product body, operation for operation):
// the golden term g (v9:30-36) and the approx term v (v9:66-108, before its Q_R).  Returns whether the
// term counts as normal in R_3d (v9:87; never with s2n).
__device__ __forceinline__ bool check_product(float a, float b, float fa, float fb, int wa, int wb, int bsum,
                                              const DFmt &fR, const float *tabf, int nm, float scale, bool approx,
                                              bool s2n, bool qbma, bool gclip, float &g, float &v) {
    const int eA = wa >> 8, mA = wa & 0x7F, eB = wb >> 8, mB = wb & 0x7F;
    const bool as = (wa & 0x80) != 0, bs = (wb & 0x80) != 0;
    g = a * b;
    const bool zero = (g == 0.0f);
    if (qbma) g = exact_q(g, fR, gclip);
    const int aexp = eA + eB - bsum;
    const float sgn = (g < 0.0f) ? -1.0f : 1.0f;
    float mp = fa * fb;
    if (approx) mp = mp - tabf[mA * nm + mB];
    bool norm = false;
    if (s2n) {
        v = p2(aexp - fR.b) * mp * sgn;
        if (as) v = v / scale;
        if (bs) v = v / scale;
        if (zero) v = 0.0f;
    } else {
        norm = (eA > 0) && (eB > 0) && (fabsf(g) >= fR.mn);
        v = norm ? p2(aexp - fR.b) * mp * sgn : g;
    }
    return norm;
}

__global__ __launch_bounds__(CK_NT) void gemm_bmm_check_kernel(const BmmCheckArgs p) {
    __shared__ float a_val[CK_BK][CK_P], a_fac[CK_BK][CK_P], b_val[CK_BK][CK_P], b_fac[CK_BK][CK_P];
    __shared__ int a_wrd[CK_BK][CK_P], b_wrd[CK_BK][CK_P];
    __shared__ float tabf[1024];  // 2^-M * table entry (the subtrahend of v9:182)
    __shared__ double red[CK_NT];

    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    const int64_t z = (int64_t)blockIdx.x / p.tiles, bid = (int64_t)blockIdx.x - z * p.tiles;
    const int64_t tile_m = bid / p.tiles_n, tile_n = bid - tile_m * p.tiles_n;
    const int64_t m0 = tile_m * CK_BM, n0 = tile_n * CK_BN;
    const int64_t i0 = z / p.nb1, i1 = z - i0 * p.nb1;
    const float *const A = p.A + i0 * p.sa0 + i1 * p.sa1;
    const float *const B = p.B + i0 * p.sb0 + i1 * p.sb1;
    const int64_t obase = z * p.M * p.N;  // the item's image in C, G, Cprod and S

    const uint32_t flags = p.flags;
    const bool s2n = flags & F_S2N, qbma = flags & F_QBMA, gclip = flags & F_GCLIP, approx = flags & F_APPROX;
    const int M = p.Mw, nm = 1 << M;
    const DFmt fA = dfmt(p.E, M, *p.bA, false), fR = dfmt(p.E, M, *p.bR, false);
    const float scale = (float)nm, ulp = p2(-M);

    for (int i = tid; i < nm * nm; i += CK_NT) tabf[i] = ulp * (float)p.tab.raw[i];

    // this thread's four columns: the exponent offset bA + bB - bR of each (v9:66)
    int bsum[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t n = min(n0 + tx * 4 + j, p.N - 1);
        bsum[j] = fA.b + p.bB[n * p.bBs] - fR.b;
    }

    float accC[4][4], accG[4][4], accS[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) accC[i][j] = accG[i][j] = accS[i][j] = 0.0f;
    unsigned long long an = 0, bn = 0, rn = 0;
    // every item's operands are counted once: A by the first column tile of each of its row tiles, B by
    // its first row tile
    const bool count_a = tile_n == 0, count_b = tile_m == 0;
    const bool b_kfast = p.sbk == 1;  // (a transposed K: lanes along k)

    for (int64_t k0 = 0; k0 < p.K; k0 += CK_BK) {
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int e = tid + r * CK_NT;  // 0 .. 1023
            {   // A element (mi, ki): lanes along k
                const int mi = e >> 4, ki = e & 15;
                const int64_t m = m0 + mi, k = k0 + ki;
                const bool in = m < p.M && k < p.K;
                const float v = in ? A[m * p.lda + k] : 0.0f;
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
                const DFmt fB = dfmt(p.E, M, p.bB[min(n, p.N - 1) * p.bBs], false);
                const float v = in ? B[k * p.sbk + n * p.sbn] : 0.0f;
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
        const int kend = (int)min<int64_t>(CK_BK, p.K - k0);  // (the K tail is not padded)
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
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float g, v;
                    const bool norm = check_product(a4[i], b4[j], fa4[i], fb4[j], wa4[i], wb4[j], bsum[j], fR, tabf,
                                                    nm, scale, approx, s2n, qbma, gclip, g, v);
                    const bool inside = (m0 + ty * 4 + i < p.M) && (n0 + tx * 4 + j < p.N);
                    rn_tile += (norm && inside) ? 1u : 0u;
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
            const int64_t o = obase + m * p.N + n;
            const float cv = accC[i][j], gv = accG[i][j];
            p.C[o] = cv;
            if (p.G) p.G[o] = gv;
            p.S[o] = accS[i][j];
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
#endif  // FP8A_OWN_CHECK

}  // namespace fp8a
