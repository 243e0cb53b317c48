// gemm_grad_conv.h -- the implicit-GEMM convolution backward (fp8a_grad_conv2d_dgrad / _wgrad):
// gemm_grad.h's arithmetic -- the three-piece bf16 split of the gradient (gr_split), the saved forward operand
// truncated (gr_b_ok), three v_mfma_f32_16x16x32_bf16 per fragment pair and K-step, piece-major, the in-tile
// fp32 recompute for lost elements -- on kernels that address dY, X and W where they lie (dense NCHW / OIHW): no
// im2col image, no dXcol, no fold.  64 x 64 tiles, 256 threads, wave w the rows 16 w .. 16 w + 15, the LDS rows
// of k of gr_block (row stride GR_RS).  Compiled only in k_gradconv.hip.
//
// conv_dgrad_kernel.  dX[b, g Cg + c, iy, ix] = sum over (ky, kx, o) of dY[b, g Og + o, oy, ox] W[g Og + o, c, ky, kx]
// with oy = (iy + ph - ky dh) / sh where that is exact and in range (ox likewise).  Rows are the input pixels of
// one residue class (ry, rx) = (iy mod sh, ix mod sw), in the order (iy / sh, ix / sw): for a class a tap is live
// for every row or for none -- ky is live iff sh divides ry + ph - ky dh, which holds on an arithmetic progression
// ky0, ky0 + py, ... (py = sh / gcd(sh, dh), from the host) -- and on a live tap oy = iy / sh + (ry + ph - ky dh) / sh:
// consecutive rows read consecutive ox whatever the stride.  K walks (live tap, o) on two levels; a row's bounds
// test per tap is the only per-element predicate.  One flattened grid over (row tile, column tile, class, image,
// group), row tile fastest; the row tiles are counted for class (0, 0), the largest, and a workgroup past its own
// class's rows leaves.  A class without a live tap, and pixels no window reaches, get +0 from the zero accumulators.
// The tile goes through LDS once more on its way out, so a wave stores 64 pixels of one channel (ix at stride sw).
//
// conv_wgrad_kernel / conv_wgrad_split_kernel.  dW[g Og + o, c, ky, kx] = sum over (b, oy, ox) of
// dY[b, g Og + o, oy, ox] X[b, g Cg + c, oy sh - ph + ky dh, ox sw - pw + kx dw].  Rows o, columns (c, ky, kx), K =
// (image, output pixel), the group as the batch index.  Staging has its lanes along k: thread (kp, r) = (tid & 15,
// 4 ((tid >> 4) & 3) + (tid >> 6)) takes the k pair 2 kp, 2 kp + 1 of the rows / columns r + 16 i, i < 4, so a
// wave reads four rows of 32 consecutive pixels, and writes one 32-bit word (two bf16 of consecutive k) per row and
// piece: no 2-byte scatter, and the four rows of a wave, 4 apart at 20 words a row, start 16 banks apart.  Its
// columns are decoded into (c, ky, kx) once, k into (b, oy, ox) once per stage.  The split along K is §3ah's:
// parts on 32-k stage boundaries, dense 64 x 64 part tiles at ws + 4096 blockIdx.x, block = (tile, group, part),
// added in index order by grad_reduce_kernel (launch_grad_reduce).
//
// Padding positions and taps that reach no output are not read and not multiplied: they stage +0 against W (a
// non-finite W there is a lost element, and the recompute skips the term as well).
#pragma once
#include "gemm_grad.h"

namespace fp8a {

struct ConvGradArgs {
    const float *dy, *op;    // the gradient [Bn, Cout, Ho, Wo]; the saved operand: W (dgrad) or X (wgrad)
    float *out;              // dX or dW
    int Bn, Cin, H, W, Cout, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw, G, Cg, Og;
    int py, px;              // dgrad: the period of the live ky / kx, s / gcd(s, d)
    int num_mt, num_nt;      // row / column tiles (dgrad: per class, image and group; wgrad: per group)
    uint32_t K;              // wgrad: Bn Ho Wo
    unsigned long long *recount;
};

void launch_conv_dgrad(const ConvGradArgs &a, unsigned blocks, hipStream_t s);
// S == 1: conv_wgrad_kernel over tiles G blocks; else conv_wgrad_split_kernel over tiles G S blocks into ws (per:
// stages per part) and the reduce pass (r: dW as grad_reduce_kernel's C)
void launch_conv_wgrad(const ConvGradArgs &a, const GradArgs &r, int64_t S, int64_t per, float *ws, hipStream_t s);

#if FP8A_OWN_GRAD_CONV
constexpr int GC_LDS = 4 * GR_T * GR_RS;  // sA[3] and sB of gr_block; the dgrad store's [64][65] floats fit

// the MFMA step of gr_block on the staged tile: 3 pieces x 4 column blocks
__device__ __forceinline__ void gc_mfma(const uint8_t *const sA, const uint8_t *const sB, const int wv, const int r16,
                                        const int gq, gr_v4f (&acc)[4]) {
    gr_v8bf af[3], bf[4];
#pragma unroll
    for (int t = 0; t < 3; ++t)
        af[t] = __builtin_bit_cast(gr_v8bf, *reinterpret_cast<const uint4 *>(sA + (t * GR_T + 16 * wv + r16) * GR_RS + 16 * gq));
#pragma unroll
    for (int j = 0; j < 4; ++j)
        bf[j] = __builtin_bit_cast(gr_v8bf, *reinterpret_cast<const uint4 *>(sB + (16 * j + r16) * GR_RS + 16 * gq));
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[t], bf[j], acc[j], 0, 0, 0);
}

// acc[j][r] = s at a dynamic (j, r): one select chain, off the hot path
__device__ __forceinline__ void gc_set(gr_v4f (&acc)[4], const int j, const int r, const float s) {
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
            if (jj == j && rr == r) acc[jj][rr] = s;
}

// ------------------------------------------------------------------------------------------ data gradient
__global__ __launch_bounds__(256) void conv_dgrad_kernel(const ConvGradArgs p) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[GC_LDS];
    uint8_t *const sA = smem, *const sB = smem + 3 * GR_T * GR_RS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, gq = lane >> 4;
    // block = (row tile, column tile, class, image, group), row tile fastest
    uint32_t bid = blockIdx.x;
    const int mt = (int)(bid % (uint32_t)p.num_mt);
    bid /= (uint32_t)p.num_mt;
    const int nt = (int)(bid % (uint32_t)p.num_nt);
    bid /= (uint32_t)p.num_nt;
    const int cls = (int)(bid % (uint32_t)(p.sh * p.sw));
    bid /= (uint32_t)(p.sh * p.sw);
    const int b = (int)(bid % (uint32_t)p.Bn), grp = (int)(bid / (uint32_t)p.Bn);
    const int ry = cls / p.sw, rx = cls - ry * p.sw;
    const int Hc = ry < p.H ? (p.H - ry + p.sh - 1) / p.sh : 0, Wc = rx < p.W ? (p.W - rx + p.sw - 1) / p.sw : 0;
    const int rows = Hc * Wc, m0 = mt * GR_T, n0 = nt * GR_T;
    if (m0 >= rows) return;  // (workgroup-uniform: a smaller class has fewer row tiles than class (0, 0))

    // the live taps of the class: ky = ky0 + jy py, jy < nly (kx likewise); tap t = jy nlx + jx
    int ky0 = p.kh, kx0 = p.kw;
    for (int k = min(p.py, p.kh) - 1; k >= 0; --k)
        if ((ry + p.ph - k * p.dh) % p.sh == 0) ky0 = k;
    for (int k = min(p.px, p.kw) - 1; k >= 0; --k)
        if ((rx + p.pw - k * p.dw) % p.sw == 0) kx0 = k;
    const int nly = ky0 < p.kh ? (p.kh - 1 - ky0) / p.py + 1 : 0, nlx = kx0 < p.kw ? (p.kw - 1 - kx0) / p.px + 1 : 0;
    const int Og = p.Og, L = p.Ho * p.Wo, khw = p.kh * p.kw, wo = p.Cg * khw;  // wo: W's stride over o
    const uint32_t K = (uint32_t)(nly * nlx) * (uint32_t)Og;
    const float *const dyb = p.dy + ((int64_t)b * p.Cout + (int64_t)grp * Og) * L;
    const float *const wb = p.op + (int64_t)grp * Og * wo;

    gr_v4f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (gr_v4f){0.0f, 0.0f, 0.0f, 0.0f};

    // tap t for the row (qy, qx): dY's pixel offset (in: inside dY) and W's tap offset
    auto tap = [&](const int t, const int qy, const int qx, int &aoff, bool &in, int &boff) {
        const int jy = t / nlx, jx = t - jy * nlx;
        const int ky = ky0 + jy * p.py, kx = kx0 + jx * p.px;
        const int oy = qy + (ry + p.ph - ky * p.dh) / p.sh, ox = qx + (rx + p.pw - kx * p.dw) / p.sw;  // exact
        in = (unsigned)oy < (unsigned)p.Ho && (unsigned)ox < (unsigned)p.Wo;
        aoff = oy * p.Wo + ox;
        boff = ky * p.kw + kx;
    };

    if (K > 0u) {
        // staging as gr_block: thread = (row / column sr, k group sg), 8 consecutive k; lanes along the rows
        const int sr = tid & 63, sg = tid >> 6;
        const bool arow = m0 + sr < rows, bcol = n0 + sr < p.Cg;
        const int row = arow ? m0 + sr : 0;
        const int qy = row / Wc, qx = row - qy * Wc;
        const int wc = (bcol ? n0 + sr : 0) * khw;
        float xa[8], xb[8];
        auto load_tile = [&](const uint32_t ks) {
            const uint32_t kb = ks + 8u * (uint32_t)sg;
            int t = (int)(kb / (uint32_t)Og), o = (int)kb - t * Og;
            int aoff = 0, boff = 0;
            bool in = false;
            if (kb < K) tap(t, qy, qx, aoff, in, boff);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool live = kb + (uint32_t)e < K;
                xa[e] = (live && in && arow) ? dyb[o * L + aoff] : 0.0f;
                xb[e] = (live && bcol) ? wb[o * wo + wc + boff] : 0.0f;
                if (++o == Og) {  // the next tap
                    o = 0;
                    ++t;
                    in = false;
                    if (kb + (uint32_t)e + 1u < K) tap(t, qy, qx, aoff, in, boff);
                }
            }
        };
        load_tile(0u);

        int anybad = 0;
        for (uint32_t ks = 0; ks < K; ks += GR_BK) {
            bool bad = false;
            uint32_t w0[4], w1[4], w2[4], wq[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t a0, a1, a2, c0, c1, c2;
                bad |= !gr_split(xa[2 * q], a0, a1, a2);
                bad |= !gr_split(xa[2 * q + 1], c0, c1, c2);
                w0[q] = a0 | (c0 << 16);
                w1[q] = a1 | (c1 << 16);
                w2[q] = a2 | (c2 << 16);
                const uint32_t b0 = __float_as_uint(xb[2 * q]), b1 = __float_as_uint(xb[2 * q + 1]);
                bad |= !gr_b_ok(b0) || !gr_b_ok(b1);
                wq[q] = (b0 >> 16) | (b1 & 0xFFFF0000u);
            }
            *reinterpret_cast<uint4 *>(sA + (0 * GR_T + sr) * GR_RS + 16 * sg) = make_uint4(w0[0], w0[1], w0[2], w0[3]);
            *reinterpret_cast<uint4 *>(sA + (1 * GR_T + sr) * GR_RS + 16 * sg) = make_uint4(w1[0], w1[1], w1[2], w1[3]);
            *reinterpret_cast<uint4 *>(sA + (2 * GR_T + sr) * GR_RS + 16 * sg) = make_uint4(w2[0], w2[1], w2[2], w2[3]);
            *reinterpret_cast<uint4 *>(sB + sr * GR_RS + 16 * sg) = make_uint4(wq[0], wq[1], wq[2], wq[3]);
            anybad |= __syncthreads_or(bad ? 1 : 0);
            if (ks + GR_BK < K) load_tile(ks + GR_BK);  // the next stage's loads fly during the MFMAs
            gc_mfma(sA, sB, wv, r16, gq, acc);
            __syncthreads();
        }

        // ---- a lost element was staged: the tile's own fp32 recomputation in the same (tap, o) order; a tap
        // outside dY for the row is skipped, as its +0 terms were
        if (anybad) {
            if (tid == 0) atomicAdd(p.recount, 1ull);
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const int c = n0 + 16 * j + r16;
#pragma unroll 1
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + 16 * wv + 4 * gq + r;
                    float s = 0.0f;
                    if (m < rows && c < p.Cg) {
                        const int my = m / Wc, mx = m - my * Wc;
                        for (int t = 0; t < nly * nlx; ++t) {
                            int aoff, boff;
                            bool in;
                            tap(t, my, mx, aoff, in, boff);
                            if (!in) continue;
                            for (int o = 0; o < Og; ++o) s = __fmaf_rn(dyb[o * L + aoff], wb[o * wo + c * khw + boff], s);
                        }
                    }
                    gc_set(acc, j, r, s);
                }
            }
        }
    }

    // ---- store: through LDS as [column][row] (65 floats a column: lanes r16 write 65 words apart), then thread =
    // (row, column group): a wave stores 64 consecutive rows of one channel
    float *const tile = reinterpret_cast<float *>(smem);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) tile[(16 * j + r16) * (GR_T + 1) + 16 * wv + 4 * gq + r] = acc[j][r];
    __syncthreads();
    const int orow = m0 + (tid & 63);
    if (orow < rows) {
        const int qy = orow / Wc, qx = orow - qy * Wc;
        const int HW = p.H * p.W;
        float *const dx = p.out + ((int64_t)b * p.Cin + (int64_t)grp * p.Cg) * HW + (ry + qy * p.sh) * p.W + rx + qx * p.sw;
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int col = (tid >> 6) + 4 * i;
            if (n0 + col < p.Cg) dx[(n0 + col) * HW] = tile[col * (GR_T + 1) + (tid & 63)];
        }
    }
}

// ------------------------------------------------------------------------------------------ weight gradient
template <bool SPLIT>
__device__ __forceinline__ void gc_wgrad_block(const ConvGradArgs &p, float *const ws, const uint32_t kper) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[GC_LDS];
    uint8_t *const sA = smem, *const sB = smem + 3 * GR_T * GR_RS;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, gq = lane >> 4;
    const uint32_t tiles = (uint32_t)(p.num_mt * p.num_nt);
    const uint32_t bid = blockIdx.x % tiles, zs = blockIdx.x / tiles;
    const int grp = (int)(SPLIT ? zs % (uint32_t)p.G : zs);
    const uint32_t part = SPLIT ? zs / (uint32_t)p.G : 0u;
    const int m0 = (int)(bid % (uint32_t)p.num_mt) * GR_T, n0 = (int)(bid / (uint32_t)p.num_mt) * GR_T;
    const int Og = p.Og, Wo = p.Wo, L = p.Ho * p.Wo, HW = p.H * p.W, khw = p.kh * p.kw, Kg = p.Cg * khw;
    const int dyi = p.Cout * L, xi = p.Cin * HW;  // the image strides
    const float *const dyb = p.dy + (int64_t)grp * Og * L;
    const float *const xb_ = p.op + (int64_t)grp * p.Cg * HW;
    const uint64_t kpast = (uint64_t)kper * (uint64_t)(part + 1u);
    const uint32_t kbeg = SPLIT ? kper * part : 0u;
    const uint32_t K = SPLIT && kpast < p.K ? (uint32_t)kpast : p.K;

    gr_v4f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (gr_v4f){0.0f, 0.0f, 0.0f, 0.0f};

    // column n = (c, ky, kx): X's offset from the window's origin pixel, and the tap's displacement
    auto column = [&](const int n, int &off, int &ty, int &tx) {
        const int c = n / khw, rem = n - c * khw, ky = rem / p.kw, kx = rem - ky * p.kw;
        ty = ky * p.dh - p.ph;
        tx = kx * p.dw - p.pw;
        off = c * HW + ty * p.W + tx;
    };

    if (K > kbeg) {
        // staging: thread = (k pair kp, row / column sr + 16 i): lanes along k
        const int kp = tid & 15, sr = 4 * ((tid >> 4) & 3) + (tid >> 6);
        bool arow[4], bcol[4];
        int ao[4], bo[4], ty[4], tx[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            arow[i] = m0 + sr + 16 * i < Og;
            ao[i] = (arow[i] ? m0 + sr + 16 * i : 0) * L;
            bcol[i] = n0 + sr + 16 * i < Kg;
            column(bcol[i] ? n0 + sr + 16 * i : 0, bo[i], ty[i], tx[i]);
        }
        float xa[8], xb[8];  // [2 i + h]: row i, k 2 kp + h
        auto load_tile = [&](const uint32_t ks) {
            const uint32_t k = ks + 2u * (uint32_t)kp;
            int b = (int)(k / (uint32_t)L), pix = (int)k - b * L;
            int oy = pix / Wo, ox = pix - oy * Wo;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bool live = k + (uint32_t)h < K;
                const int da = b * dyi + pix, y0 = oy * p.sh, x0 = ox * p.sw, dx = b * xi + y0 * p.W + x0;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    xa[2 * i + h] = (live && arow[i]) ? dyb[da + ao[i]] : 0.0f;
                    const bool in = live && bcol[i] && (unsigned)(y0 + ty[i]) < (unsigned)p.H &&
                                    (unsigned)(x0 + tx[i]) < (unsigned)p.W;
                    xb[2 * i + h] = in ? xb_[dx + bo[i]] : 0.0f;
                }
                ++pix;
                if (++ox == Wo) {
                    ox = 0;
                    if (++oy == p.Ho) {
                        oy = 0;
                        pix = 0;
                        ++b;
                    }
                }
            }
        };
        load_tile(kbeg);

        int anybad = 0;
        for (uint32_t ks = kbeg; ks < K; ks += GR_BK) {
            bool bad = false;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                uint32_t a0, a1, a2, c0, c1, c2;
                bad |= !gr_split(xa[2 * i], a0, a1, a2);
                bad |= !gr_split(xa[2 * i + 1], c0, c1, c2);
                const uint32_t b0 = __float_as_uint(xb[2 * i]), b1 = __float_as_uint(xb[2 * i + 1]);
                bad |= !gr_b_ok(b0) || !gr_b_ok(b1);
                const int at = (sr + 16 * i) * GR_RS + 4 * kp;
                *reinterpret_cast<uint32_t *>(sA + 0 * GR_T * GR_RS + at) = a0 | (c0 << 16);
                *reinterpret_cast<uint32_t *>(sA + 1 * GR_T * GR_RS + at) = a1 | (c1 << 16);
                *reinterpret_cast<uint32_t *>(sA + 2 * GR_T * GR_RS + at) = a2 | (c2 << 16);
                *reinterpret_cast<uint32_t *>(sB + at) = (b0 >> 16) | (b1 & 0xFFFF0000u);
            }
            anybad |= __syncthreads_or(bad ? 1 : 0);
            if (ks + GR_BK < K) load_tile(ks + GR_BK);  // the next stage's loads fly during the MFMAs
            gc_mfma(sA, sB, wv, r16, gq, acc);
            __syncthreads();
        }

        // ---- a lost element was staged: this (tile, part)'s own fp32 recomputation, k ascending, positions
        // outside X skipped
        if (anybad) {
            if (tid == 0) atomicAdd(p.recount, 1ull);
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + 16 * j + r16;
                int off = 0, cy = 0, cx = 0;
                if (n < Kg) column(n, off, cy, cx);
#pragma unroll 1
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + 16 * wv + 4 * gq + r;
                    float s = 0.0f;
                    if (m < Og && n < Kg) {
                        int b = (int)(kbeg / (uint32_t)L), pix = (int)kbeg - b * L;
                        int oy = pix / Wo, ox = pix - oy * Wo;
                        for (uint32_t k = kbeg; k < K; ++k) {
                            const int y0 = oy * p.sh, x0 = ox * p.sw;
                            if ((unsigned)(y0 + cy) < (unsigned)p.H && (unsigned)(x0 + cx) < (unsigned)p.W)
                                s = __fmaf_rn(dyb[b * dyi + m * L + pix], xb_[b * xi + y0 * p.W + x0 + off], s);
                            ++pix;
                            if (++ox == Wo) {
                                ox = 0;
                                if (++oy == p.Ho) {
                                    oy = 0;
                                    pix = 0;
                                    ++b;
                                }
                            }
                        }
                    }
                    gc_set(acc, j, r, s);
                }
            }
        }
    }

    // ---- store: lane (r16, gq) holds rows 4 gq + r of its wave's 16, column r16 of block j
    if constexpr (SPLIT) {
        float *const W = ws + (int64_t)blockIdx.x * (GR_T * GR_T);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) W[GR_T * (16 * wv + 4 * gq + r) + 16 * j + r16] = acc[j][r];
        return;
    }
    float *const dw = p.out + (int64_t)grp * Og * Kg;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + 16 * j + r16;
        if (n >= Kg) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + 16 * wv + 4 * gq + r;
            if (m < Og) dw[m * Kg + n] = acc[j][r];
        }
    }
}

__global__ __launch_bounds__(256) void conv_wgrad_kernel(const ConvGradArgs p) { gc_wgrad_block<false>(p, nullptr, 0u); }

__global__ __launch_bounds__(256) void conv_wgrad_split_kernel(const ConvGradArgs p, float *const ws, const uint32_t kper) {
    gc_wgrad_block<true>(p, ws, kper);
}
#endif  // FP8A_OWN_GRAD_CONV

}  // namespace fp8a
