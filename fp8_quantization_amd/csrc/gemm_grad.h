// gemm_grad.h -- the gradient GEMM of the straight-through backward (fp8a_grad_bmm, gemm_grad_kernel): an
// arbitrary fp32 operand A (the incoming gradient) times a bf16-exact operand B (a saved forward operand on
// its FP8 grid: <= 8 significant bits, as gemm_dense.h relies on), batched, with K addressed on two levels in
// both operands so a convolution's weight gradient reduces over (image, pixel) in one launch; compiled only
// in k_grad.hip.
//
// The split.  An fp32 value x is the sum of three bf16 pieces, each the truncation of what the previous
// ones left:  p0 = trunc16(x), p1 = trunc16(x - p0), p2 = x - p0 - p1  (8 + 8 + 8 significand bits; both
// subtractions are exact, and what is left after two truncations has at most 8 bits, so p2 is a bf16).  A
// piece times a bf16-exact b has at most 16 significant bits: exact in fp32.  Three
// v_mfma_f32_16x16x32_bf16 per K-step against the same B fragment therefore accumulate exactly the terms
// the fp32 product sums, at the bf16 matrix-core rate.  bf16 subnormals are not relied on: a piece (or a B
// element) with a zero exponent field counts as lost, so an A element is split exactly iff it is zero or
// finite with exponent field >= 24 (|x| >= 2^-103: its last bit is worth 2^-126 or more, so every piece is
// zero or normal).
//
// One workgroup owns one 64 x 64 output tile of one batch item; wave w the rows 16 w .. 16 w + 15 of all
// four 16-column blocks.  Per 32-k stage the tile's A (split while it is staged: no piece image in HBM) and B
// (truncated) go to LDS as bf16 rows of k, and a wave issues 3 pieces x 4 column blocks = 12 MFMAs.  A fixed
// k order per output, no float atomics, no split along K: two calls give the same bytes.
// A tile whose staging saw a B element that is not bf16-exact, or an A element the split loses (above; inf /
// NaN included), recomputes itself with fp32 FMAs in the same k order after a workgroup-uniform branch and
// counts itself in *recount (one atomic per recomputed tile, none otherwise), as gemm_bmm_kernel does.
//
// The split along K (fp8a_grad_bmm_split) is two more kernels around the same tile body:
// gemm_grad_split_kernel gives each (tile, batch item, part) a workgroup that runs the part's stages and stores
// its accumulator tile in a workspace, grad_reduce_kernel adds an output's parts in index order.  Two launches,
// no flags or atomics between workgroups: as deterministic as the unsplit kernel.
#pragma once
#include "fp8approx_common.h"

namespace fp8a {

struct GradArgs {
    const float *A, *B;
    float *C;
    int64_t M, N;
    uint32_t K0, K1, K;      // K = K0 K1 < 2^31; k = k0 K1 + k1
    int64_t sa_i, sa_m, sa_k0, sa_k1;   // A(i, m, k0, k1) = A[i sa_i + m sa_m + k0 sa_k0 + k1 sa_k1]
    int64_t sb_i, sb_k0, sb_k1, sb_n;   // B(i, k0, k1, n)
    int64_t sc_i, sc_m, sc_n;           // C(i, m, n)
    int64_t num_mt, tiles;   // row tiles / tiles per batch item; block b = (tile b % tiles, item b / tiles)
    unsigned long long *recount;  // tiles recomputed in fp32 (k_grad.hip's counter)
};

void launch_grad(const GradArgs &a, dim3 grid, hipStream_t s);
// the split along K: gemm_grad_split_kernel over tiles nb S blocks into ws (S dense [nb][tiles][64][64] fp32
// images), then grad_reduce_kernel over (tiles nb, 16) blocks; per: stages per part
void launch_grad_split(const GradArgs &a, int64_t nb, int64_t S, int64_t per, float *ws, hipStream_t s);
unsigned long long *grad_recount_ptr();  // nullptr: the address query failed
int grad_recount_read(unsigned long long *v, bool reset);

constexpr int GR_T = 64;          // tile edge
constexpr int GR_BK = 32;         // k per stage = one MFMA K-step
constexpr int GR_RS = 2 * GR_BK + 16;  // LDS row stride, bytes (bf16 rows of k)

#if FP8A_OWN_GRAD
typedef __bf16 gr_v8bf __attribute__((ext_vector_type(8)));
typedef float gr_v4f __attribute__((ext_vector_type(4)));

// B's test: exact in bf16 and not a bf16 subnormal
__device__ __forceinline__ bool gr_b_ok(uint32_t u) {
    const uint32_t e = u & 0x7F800000u;
    return (u & 0xFFFFu) == 0u && e != 0x7F800000u && (e != 0u || (u & 0x7FFFFFFFu) == 0u);
}
// A's split: the three pieces' bf16 bit patterns; false when the pieces lose x (header)
__device__ __forceinline__ bool gr_split(float x, uint32_t &h0, uint32_t &h1, uint32_t &h2) {
    const uint32_t u = __float_as_uint(x), e = (u >> 23) & 0xFFu;
    const bool ok = (u & 0x7FFFFFFFu) == 0u || (e >= 24u && e != 0xFFu);
    const float p0 = __uint_as_float(u & 0xFFFF0000u);
    const float r1 = ok ? x - p0 : 0.0f;  // exact
    const uint32_t u1 = __float_as_uint(r1);
    const float r2 = r1 - __uint_as_float(u1 & 0xFFFF0000u);  // exact, <= 8 significant bits
    h0 = ok ? u >> 16 : 0u;
    h1 = u1 >> 16;
    h2 = __float_as_uint(r2) >> 16;
    return ok;
}

// One workgroup's work, shared by the two product kernels.  SPLIT = false is gemm_grad_kernel: block = (tile,
// item), the k range [0, K), the tile stored through C's strides.  SPLIT = true is gemm_grad_split_kernel: block =
// (tile, item, part), part slowest; part s owns the stages [s per, (s + 1) per) -- kper = 32 per flat k -- runs the
// same staged loads, piece splits and 12-MFMA steps on them from zero accumulators, and stores its whole 64 x 64
// accumulator tile, dense and row-major, at ws + 4096 blockIdx.x: rows and columns beyond M and N hold the zeros
// their zero-filled staging sums to, so grad_reduce_kernel reads nothing that was not written.  A block that
// staged a lost element recomputes its own k range and counts itself once.
template <bool SPLIT>
__device__ __forceinline__ void gr_block(const GradArgs &p, float *const ws, const int64_t nb, const uint32_t kper) {
    __shared__ __attribute__((aligned(16))) uint8_t sA[3][GR_T][GR_RS];
    __shared__ __attribute__((aligned(16))) uint8_t sB[GR_T][GR_RS];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int64_t bid = (int64_t)blockIdx.x % p.tiles, zs = (int64_t)blockIdx.x / p.tiles;
    const int64_t z = SPLIT ? zs % nb : zs, part = SPLIT ? zs / nb : 0;
    const int64_t m0 = (bid % p.num_mt) * GR_T, n0 = (bid / p.num_mt) * GR_T;
    const float *const A = p.A + z * p.sa_i;
    const float *const B = p.B + z * p.sb_i;
    float *const C = p.C + z * p.sc_i;
    // the flat k range [kbeg, K) of this block (K: where its walk ends)
    const uint64_t kpast = (uint64_t)kper * (uint64_t)(part + 1);
    const uint32_t kbeg = SPLIT ? kper * (uint32_t)part : 0u;
    const uint32_t K = SPLIT && kpast < p.K ? (uint32_t)kpast : p.K, K1 = p.K1;

    gr_v4f acc[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] = (gr_v4f){0.0f, 0.0f, 0.0f, 0.0f};

    if (K > kbeg) {  // (an empty range: the sum over an empty axis, zeros; nothing but C is touched)
        // staging: thread = (row / column sr, k group sg): 8 consecutive k of the stage.  Lanes run along
        // the rows, so an operand with unit m (n) stride loads full lines and one with unit k stride 32
        // contiguous bytes per lane.
        const int sr = tid & 63, sg = tid >> 6;
        const bool arow = m0 + sr < p.M, bcol = n0 + sr < p.N;
        const float *const Ar = A + (arow ? m0 + sr : 0) * p.sa_m;
        const float *const Br = B + (bcol ? n0 + sr : 0) * p.sb_n;
        float xa[8], xb[8];
        auto load_tile = [&](uint32_t ks) {
            const uint32_t kb = ks + 8u * (uint32_t)sg;
            uint32_t q0 = kb / K1, q1 = kb - q0 * K1;
            int64_t oa = (int64_t)q0 * p.sa_k0 + (int64_t)q1 * p.sa_k1;
            int64_t ob = (int64_t)q0 * p.sb_k0 + (int64_t)q1 * p.sb_k1;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const bool in = kb + (uint32_t)e < K;
                xa[e] = (in && arow) ? Ar[oa] : 0.0f;
                xb[e] = (in && bcol) ? Br[ob] : 0.0f;
                oa += p.sa_k1;
                ob += p.sb_k1;
                if (++q1 == K1) {  // the next k0: back over the K1 steps taken, one k0 step on
                    q1 = 0;
                    oa += p.sa_k0 - (int64_t)K1 * p.sa_k1;
                    ob += p.sb_k0 - (int64_t)K1 * p.sb_k1;
                }
            }
        };
        load_tile(kbeg);

        int anybad = 0;
        for (uint32_t ks = kbeg; ks < K; ks += GR_BK) {
            bool bad = false;
            uint32_t w0[4], w1[4], w2[4], wb[4];
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
                wb[q] = (b0 >> 16) | (b1 & 0xFFFF0000u);
            }
            *reinterpret_cast<uint4 *>(&sA[0][sr][16 * sg]) = make_uint4(w0[0], w0[1], w0[2], w0[3]);
            *reinterpret_cast<uint4 *>(&sA[1][sr][16 * sg]) = make_uint4(w1[0], w1[1], w1[2], w1[3]);
            *reinterpret_cast<uint4 *>(&sA[2][sr][16 * sg]) = make_uint4(w2[0], w2[1], w2[2], w2[3]);
            *reinterpret_cast<uint4 *>(&sB[sr][16 * sg]) = make_uint4(wb[0], wb[1], wb[2], wb[3]);
            anybad |= __syncthreads_or(bad ? 1 : 0);
            if (ks + GR_BK < K) load_tile(ks + GR_BK);  // the next stage's loads fly during the MFMAs

            // lane (r16, g): row / column r16 of its block, k 8 g .. 8 g + 7 of the step
            gr_v8bf af[3], bf[4];
#pragma unroll
            for (int t = 0; t < 3; ++t)
                af[t] = __builtin_bit_cast(gr_v8bf, *reinterpret_cast<const uint4 *>(&sA[t][16 * wv + r16][16 * g]));
#pragma unroll
            for (int j = 0; j < 4; ++j)
                bf[j] = __builtin_bit_cast(gr_v8bf, *reinterpret_cast<const uint4 *>(&sB[16 * j + r16][16 * g]));
#pragma unroll
            for (int t = 0; t < 3; ++t)  // (piece-major: four independent accumulators between dependent MFMAs)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[t], bf[j], acc[j], 0, 0, 0);
            __syncthreads();
        }

        // ---- the tile saw an element the bf16 forms lose: its own fp32 recomputation, FMAs in the same k
        // order (workgroup-uniform).  Thread (wv, r16, g) owns rows 16 wv + 4 g + r, columns 16 j + r16.
        if (anybad) {
            if (tid == 0) atomicAdd(p.recount, 1ull);
#pragma unroll 1
            for (int j = 0; j < 4; ++j) {
                const int64_t n = n0 + 16 * j + r16;
#pragma unroll 1
                for (int r = 0; r < 4; ++r) {
                    const int64_t m = m0 + 16 * wv + 4 * g + r;
                    float s = 0.0f;
                    if (m < p.M && n < p.N) {
                        const float *const ap = A + m * p.sa_m;
                        const float *const bp = B + n * p.sb_n;
                        if constexpr (!SPLIT) {  // [0, K0 K1): the two levels as they are
                            for (uint32_t k0 = 0; k0 < p.K0; ++k0)
                                for (uint32_t k1 = 0; k1 < K1; ++k1)
                                    s = __fmaf_rn(ap[(int64_t)k0 * p.sa_k0 + (int64_t)k1 * p.sa_k1],
                                                  bp[(int64_t)k0 * p.sb_k0 + (int64_t)k1 * p.sb_k1], s);
                        } else {  // a part may begin and end inside a k0 row: the flat walk of load_tile
                            uint32_t q1 = kbeg % K1;
                            int64_t oa = (int64_t)(kbeg / K1) * p.sa_k0 + (int64_t)q1 * p.sa_k1;
                            int64_t ob = (int64_t)(kbeg / K1) * p.sb_k0 + (int64_t)q1 * p.sb_k1;
                            for (uint32_t k = kbeg; k < K; ++k) {
                                s = __fmaf_rn(ap[oa], bp[ob], s);
                                oa += p.sa_k1;
                                ob += p.sb_k1;
                                if (++q1 == K1) {
                                    q1 = 0;
                                    oa += p.sa_k0 - (int64_t)K1 * p.sa_k1;
                                    ob += p.sb_k0 - (int64_t)K1 * p.sb_k1;
                                }
                            }
                        }
                    }
                    // (a dynamic index: one select chain over the 16 accumulators, off the hot path)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
                        for (int rr = 0; rr < 4; ++rr)
                            if (jj == j && rr == r) acc[jj][rr] = s;
                }
            }
        }
    }

    // ---- store: D[m][n], lane (r16, g) holds rows 4 g + r of its wave's 16, column r16 of block j
    if constexpr (SPLIT) {
        float *const W = ws + (int64_t)blockIdx.x * (GR_T * GR_T);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) W[GR_T * (16 * wv + 4 * g + r) + 16 * j + r16] = acc[j][r];
        return;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int64_t n = n0 + 16 * j + r16;
        if (n >= p.N) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t m = m0 + 16 * wv + 4 * g + r;
            if (m < p.M) C[m * p.sc_m + n * p.sc_n] = acc[j][r];
        }
    }
}

__global__ __launch_bounds__(256) void gemm_grad_kernel(const GradArgs p) { gr_block<false>(p, nullptr, 1, 0u); }

__global__ __launch_bounds__(256) void gemm_grad_split_kernel(const GradArgs p, float *const ws, const int64_t nb,
                                                              const uint32_t kper) {
    gr_block<true>(p, ws, nb, kper);
}

// The reduce pass: one thread per output element, block = four rows of one (item, tile), blockIdx.y the row
// group; lane = column, so every workspace read is a full 256-byte row.  The parts are added in index order
// from P_0 (not from +0: a sum of negative zeros stays negative), plain fp32 adds; stored through C's strides.
__global__ __launch_bounds__(256) void grad_reduce_kernel(const GradArgs p, const float *const ws, const int64_t nb,
                                                          const int S) {
    const int col = threadIdx.x & 63, row = 4 * (int)blockIdx.y + (int)(threadIdx.x >> 6);
    const int64_t bid = (int64_t)blockIdx.x % p.tiles, z = (int64_t)blockIdx.x / p.tiles;
    const int64_t m = (bid % p.num_mt) * GR_T + row, n = (bid / p.num_mt) * GR_T + col;
    if (m >= p.M || n >= p.N) return;
    const int64_t part = nb * p.tiles * (GR_T * GR_T);
    const float *w = ws + (int64_t)blockIdx.x * (GR_T * GR_T) + GR_T * row + col;
    float acc = *w;
#pragma unroll 4
    for (int s = 1; s < S; ++s) {
        w += part;
        acc = acc + *w;
    }
    p.C[z * p.sc_i + m * p.sc_m + n * p.sc_n] = acc;
}
#endif  // FP8A_OWN_GRAD

}  // namespace fp8a
