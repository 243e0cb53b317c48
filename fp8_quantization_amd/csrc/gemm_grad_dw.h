// gemm_grad_dw.h -- the depthwise convolution backward (fp8a_grad_dwconv2d_dgrad / _wgrad): direct
// fp32 kernels for groups == Cin == Cout, where a 64 x 64 matrix-core gradient tile holds one useful column.  A
// depthwise gradient is kh kw multiply-adds per element: plain __fmaf_rn on dy, x and w where they lie (dense NCHW,
// [C, 1, kh, kw]), one rounding per term, any float32 operand on the one path -- no three-piece split, no
// bf16-exactness test, no recompute, the recomputed-tile counter never touched.  Compiled only in k_graddw.hip.
//
// The tap rule (include/fp8approx.h): a padding position, or a tap that reaches no output, is neither read nor
// multiplied -- every term sits under its own bounds predicate; nothing relies on a zero halo times the operand.
// Every output element is written (+0 where nothing contributes); no float atomics, no arrival order.
//
// dwconv_dgrad_kernel<K, S>.  dx[b, c, iy, ix] = sum_{ky, kx} dy[b, c, oy, ox] w[c, 0, ky, kx], oy = (iy + ph -
// ky dh) / sh where exact and in range.  Work is counted in quotient pixels (qy, qx) = (iy / sh, ix / sw): a thread
// computes the sh x sw block of dX of its quotient pixel, one pixel per residue class (ry, rx), so a class's live
// taps are the same for every thread and a live tap reads dY at (qy + ey, qx + ex) with ey = (ry + ph - ky dh) / sh
// fixed per (class, tap): straight-line code, no divergence on parity.  The planes (b, c) of a dense NCHW tensor are
// consecutive, P = b C + c.  Two workgroup shapes, chosen by the host from the geometry:
//   tile mode    a workgroup owns a 32 x 64 quotient tile of one plane, qx along the lanes (wave w the rows w + 4 i).
//                The tile's dY footprint -- FH x FW = (32 + ey1 - ey0) x (64 + ex1 - ex0), the host's exact range of
//                live offsets -- is staged once by LDS-DMA, one 4-byte global_load_lds per lane and row piece
//                (lane = column: coalesced rows; positions outside dY are not loaded).
//   plane mode   a plane of at most 1024 quotient pixels would leave that tile mostly idle: the workgroup takes PB
//                consecutive planes, whose dY is one contiguous range, copied raw by 16-byte global_load_lds as the
//                staged depthwise forward kernels do (gemm_dense.h's dn_dw3g_kernel: from the 16-byte-aligned start,
//                the tensor's first / last chunk per float), and its threads walk the flattened (plane, qy, qx).
// The kh kw weights of the workgroup's planes go to LDS once; the 3 x 3 instances keep a plane's nine in registers.
// Instances: <3, 1> and <3, 2> (3 x 3, dilation 1, padding 1, stride (1, 1) / (2, 2): the live taps unrolled
// constants, 9 at stride 1, 4 / 2 / 2 / 1 at stride 2) and <0, 0>, the runtime geometry (kh, kw <= 7, (k - 1) d <= 32).
// The grid is flat over (tile, plane) or plane groups; in-tile indices are 32-bit, the plane's base 64-bit, once.
//
// dwconv_wgrad_kernel<KH, KW, FIXED> / dwconv_wgrad_reduce_kernel.  dw[c, 0, ky, kx] = sum_{b, oy, ox} dy[b, c, oy,
// ox] x[b, c, oy sh - ph + ky dh, ox sw - pw + kx dw].  A workgroup is (channel, part); the split's unit is an output
// row (b, oy): R = Bn Ho, per = ceil(R / splits), S = ceil(R / per), part s the rows [per s, min(per (s + 1), R)).
// It walks its rows in chunks of CR rows x CW columns (about 1024 pixels; rows run on across images), lanes along
// the chunk's flattened pixel index, so a 7-wide plane still fills its waves.  Per chunk the X footprint -- one slab
// of FHx x FWx per image the chunk touches -- is staged by the same per-row LDS-DMA, so X comes from HBM about
// once; a thread reads its dY value once and feeds all kh kw partial sums, which live in registers (FIXED: KH x KW is
// the kernel; else kh <= KH, kw <= KW under uniform predicates).  The partials combine in a fixed order: a xor
// butterfly inside the wave, the waves through LDS in wave-index order.  S == 1 stores dw; else part s stores at
// ws[(c S + s) kh kw ..] and dwconv_wgrad_reduce_kernel adds P_0 + P_1 + ... in index order.
#pragma once
#include "fp8approx_common.h"

namespace fp8a {

constexpr int DWG_QH = 32, DWG_QW = 64;   // the data gradient's quotient tile
constexpr int DWG_PIX = DWG_QH * DWG_QW;
constexpr int DWG_KMAX = 7;               // the runtime-geometry instances: kh, kw <= 7,
constexpr int DWG_EXT = 32;               // (kh - 1) dh, (kw - 1) dw <= 32
constexpr int DWG_CHUNK = 1024;           // the weight gradient's pixels per chunk
constexpr int DWG_LDS = 48 << 10;         // the most LDS a plan may take

struct DwGradArgs {
    const float *dy, *op;  // the gradient [Bn, C, Ho, Wo]; the saved operand: w (dgrad) or x (wgrad)
    float *out;            // dx or dw
    int Bn, C, H, W, Ho, Wo, kh, kw, sh, sw, ph, pw, dh, dw;
    int64_t ndy;           // dgrad: dy's elements (the raw copy never reads outside them)
    // dgrad
    int64_t planes;        // Bn C
    int Hq, Wq;            // the quotient plane: ceil(H / sh) x ceil(W / sw)
    int ey0, ex0, FH, FW;  // tile mode: the smallest live offsets and the footprint
    int nty, ntx;          // tile mode: tiles per plane
    int PB;                // plane mode: planes per workgroup (0: tile mode)
    int nimg;              // LDS floats of the staged dY / X image (the weights follow it)
    // wgrad
    int R, per, S;         // output rows, rows per part, parts
    int CR, CW;            // chunk rows / columns
    int FHx, FWx;          // one image's slab
    unsigned lds;          // dynamic LDS bytes
};

void launch_dw_dgrad(const DwGradArgs &a, unsigned blocks, hipStream_t s);
void launch_dw_wgrad(const DwGradArgs &a, float *ws, hipStream_t s);

#if FP8A_OWN_GRAD_DW
extern __shared__ float dwg_sm[];

// ------------------------------------------------------------------------------------------ data gradient
// the sh x sw block of dX of the quotient pixel (qy, qx): img[base + oy RS + ox] is dY(oy, ox) of its plane, wp the
// plane's weights in LDS, o the plane of dX
template <int K, int S>
__device__ __forceinline__ void dwg_pixel(const DwGradArgs &p, const float *const img, const int base, const int RS,
                                          const float *const wp, float *const o, const int qy, const int qx) {
    if constexpr (K == 3) {
        constexpr int E0 = S == 1 ? -1 : 0, NE = S == 1 ? 3 : 2;  // the live offsets: E0 .. E0 + NE - 1
        float w[9], v[NE][NE];
        bool ok[NE][NE];
#pragma unroll
        for (int t = 0; t < 9; ++t) w[t] = wp[t];
#pragma unroll
        for (int a = 0; a < NE; ++a)
#pragma unroll
            for (int b = 0; b < NE; ++b) {
                const int oy = qy + E0 + a, ox = qx + E0 + b;
                ok[a][b] = (unsigned)oy < (unsigned)p.Ho && (unsigned)ox < (unsigned)p.Wo;
                v[a][b] = 0.0f;
                if (ok[a][b]) v[a][b] = img[base + oy * RS + ox];
            }
#pragma unroll
        for (int ry = 0; ry < S; ++ry)
#pragma unroll
            for (int rx = 0; rx < S; ++rx) {
                float acc = 0.0f;
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) {
                        const int ty = ry + 1 - ky, tx = rx + 1 - kx;  // (compile-time after unrolling)
                        if (ty % S != 0 || tx % S != 0) continue;
                        const int a = ty / S - E0, b = tx / S - E0;
                        acc = ok[a][b] ? __fmaf_rn(v[a][b], w[3 * ky + kx], acc) : acc;  // skipped, not 0 * w
                    }
                const int iy = qy * S + ry, ix = qx * S + rx;
                if (iy < p.H && ix < p.W) o[iy * p.W + ix] = acc;
            }
    } else {
        for (int ry = 0; ry < p.sh && qy * p.sh + ry < p.H; ++ry)
            for (int rx = 0; rx < p.sw && qx * p.sw + rx < p.W; ++rx) {
                float acc = 0.0f;
                for (int ky = 0; ky < p.kh; ++ky) {
                    const int ty = ry + p.ph - ky * p.dh;
                    if (ty % p.sh != 0) continue;
                    const int oy = qy + ty / p.sh;
                    if ((unsigned)oy >= (unsigned)p.Ho) continue;
                    for (int kx = 0; kx < p.kw; ++kx) {
                        const int tx = rx + p.pw - kx * p.dw;
                        if (tx % p.sw != 0) continue;
                        const int ox = qx + tx / p.sw;
                        if ((unsigned)ox < (unsigned)p.Wo) acc = __fmaf_rn(img[base + oy * RS + ox], wp[ky * p.kw + kx], acc);
                    }
                }
                o[(qy * p.sh + ry) * p.W + qx * p.sw + rx] = acc;
            }
    }
}

template <int K, int S>
__global__ __launch_bounds__(256) void dwconv_dgrad_kernel(const DwGradArgs p) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int khw = K ? K * K : p.kh * p.kw, HoWo = p.Ho * p.Wo, HW = p.H * p.W;
    const bool plane_mode = p.PB > 0;
    int64_t P0;
    int npl = 1, qy0 = 0, qx0 = 0;
    if (plane_mode) {
        P0 = (int64_t)blockIdx.x * p.PB;
        npl = (int)min((int64_t)p.PB, p.planes - P0);
    } else {  // block = (tile, plane), tile fastest
        const unsigned tiles = (unsigned)(p.nty * p.ntx), t = blockIdx.x % tiles;
        P0 = blockIdx.x / tiles;
        qy0 = (int)(t / (unsigned)p.ntx) * DWG_QH;
        qx0 = (int)(t % (unsigned)p.ntx) * DWG_QW;
    }
    const float *const dyp = p.dy + P0 * HoWo;  // (the 64-bit bases, once)
    float *const dxp = p.out + P0 * HW;
    float *img = dwg_sm, *wsm = dwg_sm + p.nimg;

    int RS, org;  // dY(pl, oy, ox) of the workgroup's plane pl is img[org + pl HoWo + oy RS + ox]
    if (plane_mode) {
        // the planes' contiguous range, raw, in 16-byte chunks from its 16-byte-aligned start
        const int lead = (int)(((uintptr_t)dyp & 15u) >> 2), nq = (lead + npl * HoWo + 3) >> 2;
        const float *const src = dyp - lead;
        const uintptr_t lo = (uintptr_t)p.dy, hi = (uintptr_t)(p.dy + p.ndy);
        for (int q0 = 0; q0 < nq; q0 += 256) {
            const int q = q0 + tid;
            if (q < nq) {
                const uintptr_t s4 = (uintptr_t)(src + 4 * q);
                if (s4 >= lo && s4 + 16u <= hi) {
                    __builtin_amdgcn_global_load_lds(src + 4 * q, img + 4 * (q0 + 64 * wv), 16, 0, 0);
                } else {  // (the tensor's first / last floats: never read outside dy)
                    for (int e = 0; e < 4; ++e)
                        if (s4 + 4u * e >= lo && s4 + 4u * e < hi) img[4 * q + e] = src[4 * q + e];
                }
            }
        }
        RS = p.Wo;
        org = lead;
    } else {
        // the tile's footprint, a row piece of 64 columns per wave and instruction; outside dY: not loaded
        const int oy_lo = qy0 + p.ey0, ox_lo = qx0 + p.ex0;
        for (int r = wv; r < p.FH; r += 4) {
            const int oy = oy_lo + r;
            if ((unsigned)oy >= (unsigned)p.Ho) continue;
            for (int j = 0; j < p.FW; j += 64) {
                const int cc = j + lane, ox = ox_lo + cc;
                if (cc < p.FW && (unsigned)ox < (unsigned)p.Wo)
                    __builtin_amdgcn_global_load_lds(dyp + oy * p.Wo + ox, img + r * p.FW + j, 4, 0, 0);
            }
        }
        RS = p.FW;
        org = -(oy_lo * p.FW + ox_lo);
    }
    const int c0 = (int)(P0 % p.C);
    for (int d = tid; d < npl * khw; d += 256) {
        const int pl = d / khw;
        wsm[d] = p.op[((c0 + pl) % p.C) * khw + (d - pl * khw)];
    }
    __syncthreads();  // (waits for the LDS-DMA: vmcnt(0) before the barrier)

    if (plane_mode) {
        const int HWq = p.Hq * p.Wq;
        for (int e = tid; e < npl * HWq; e += 256) {
            const int pl = e / HWq, rem = e - pl * HWq, qy = rem / p.Wq, qx = rem - qy * p.Wq;
            dwg_pixel<K, S>(p, img, org + pl * HoWo, RS, wsm + pl * khw, dxp + pl * HW, qy, qx);
        }
    } else {
        const int qx = qx0 + lane;
        if (qx < p.Wq)
            for (int i = 0; i < DWG_QH / 4; ++i) {
                const int qy = qy0 + wv + 4 * i;
                if (qy < p.Hq) dwg_pixel<K, S>(p, img, org, RS, wsm, dxp, qy, qx);
            }
    }
}

// ------------------------------------------------------------------------------------------ weight gradient
template <int KH, int KW, bool FIXED>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const DwGradArgs p, float *const ws) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = (int)(blockIdx.x / (unsigned)p.S), part = (int)(blockIdx.x - (unsigned)c * (unsigned)p.S);
    const int r0 = part * p.per, r1 = min(r0 + p.per, p.R);
    const int kh = FIXED ? KH : p.kh, kw = FIXED ? KW : p.kw;
    const int HoWo = p.Ho * p.Wo, HW = p.H * p.W, ci = p.C * HoWo, xi = p.C * HW, slab = p.FHx * p.FWx;
    const float *const dyc = p.dy + (int64_t)c * HoWo;  // (the 64-bit bases, once)
    const float *const xc = p.op + (int64_t)c * HW;
    float *img = dwg_sm;
    const int rstep = p.dh * p.FWx;

    float acc[KH * KW];
#pragma unroll
    for (int t = 0; t < KH * KW; ++t) acc[t] = 0.0f;

    for (int ra = r0; ra < r1; ra += p.CR) {
        const int rb = min(ra + p.CR, r1);
        const int ba = ra / p.Ho, oya = ra - ba * p.Ho, nim = (rb - 1) / p.Ho - ba + 1;
        for (int xa = 0; xa < p.Wo; xa += p.CW) {
            const int cw = min(p.CW, p.Wo - xa), x0 = xa * p.sw - p.pw;
            __syncthreads();  // (the chunk before is read)
            // slab i = image ba + i: the rows of X from its first output row's first tap down, columns from x0
            for (int u = wv; u < nim * p.FHx; u += 4) {
                const int i = u / p.FHx, fr = u - i * p.FHx, b = ba + i;
                const int oylo = i == 0 ? oya : 0, oyhi = min(rb - b * p.Ho, p.Ho) - 1;
                const int iy = oylo * p.sh - p.ph + fr;
                if (fr > (oyhi - oylo) * p.sh + (kh - 1) * p.dh || (unsigned)iy >= (unsigned)p.H) continue;
                for (int j = 0; j < p.FWx; j += 64) {
                    const int cc = j + lane, ix = x0 + cc;
                    if (cc < p.FWx && (unsigned)ix < (unsigned)p.W)
                        __builtin_amdgcn_global_load_lds(xc + b * xi + iy * p.W + ix, img + u * p.FWx + j, 4, 0, 0);
                }
            }
            __syncthreads();  // (waits for the LDS-DMA)
            const int npx = (rb - ra) * cw;
            for (int e = tid; e < npx; e += 256) {
                const int j = e / cw, col = e - j * cw, r = ra + j, b = r / p.Ho, oy = r - b * p.Ho, ox = xa + col;
                const float g = dyc[b * ci + oy * p.Wo + ox];
                const int i = b - ba, oylo = i == 0 ? oya : 0;
                const int base = i * slab + (oy - oylo) * p.sh * p.FWx + col * p.sw;
                const int iy0 = oy * p.sh - p.ph, ix0 = ox * p.sw - p.pw;
                unsigned cm = 0u;  // the columns inside X, one bit per kx
#pragma unroll
                for (int kx = 0; kx < KW; ++kx)
                    cm |= (unsigned)((FIXED || kx < kw) && (unsigned)(ix0 + kx * p.dw) < (unsigned)p.W) << kx;
                int row = base;
#pragma unroll
                for (int ky = 0; ky < KH; ++ky, row += rstep) {
                    if ((!FIXED && ky >= kh) || (unsigned)(iy0 + ky * p.dh) >= (unsigned)p.H) continue;
                    int at = row;
#pragma unroll
                    for (int kx = 0; kx < KW; ++kx, at += p.dw)
                        if ((cm >> kx) & 1u)  // outside X: skipped, not dy * 0
                            acc[ky * KW + kx] = __fmaf_rn(g, img[at], acc[ky * KW + kx]);
                }
            }
        }
    }

    // the workgroup's partials: a xor butterfly in the wave, then the waves in index order
    __syncthreads();
#pragma unroll
    for (int t = 0; t < KH * KW; ++t) {
        float v = acc[t];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_xor(v, off, 64);
        if (lane == 0) img[wv * (KH * KW) + t] = v;
    }
    __syncthreads();
    if (tid < kh * kw) {
        const int ky = tid / kw, t = ky * KW + (tid - ky * kw);
        const float s = ((img[t] + img[KH * KW + t]) + img[2 * KH * KW + t]) + img[3 * KH * KW + t];
        if (p.S == 1) p.out[(int64_t)c * (kh * kw) + tid] = s;
        else ws[((int64_t)c * p.S + part) * (kh * kw) + tid] = s;
    }
}

// dw[i] = P_0[i] + P_1[i] + ... in index order; i = (c, tap), part s of channel c at ws[(c S + s) khw ..]
__global__ __launch_bounds__(256) void dwconv_wgrad_reduce_kernel(const float *const ws, float *const dw, const int n,
                                                                  const int khw, const int S) {
    const int i = (int)(blockIdx.x * 256u + threadIdx.x);
    if (i >= n) return;
    const int c = i / khw, t = i - c * khw;
    const float *const q = ws + (int64_t)c * S * khw + t;
    float s = q[0];
    for (int k = 1; k < S; ++k) s = s + q[(int64_t)k * khw];
    dw[i] = s;
}
#endif  // FP8A_OWN_GRAD_DW

}  // namespace fp8a
