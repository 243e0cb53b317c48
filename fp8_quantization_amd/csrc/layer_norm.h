// layer_norm.h -- QuantLayerNorm's block in one pass each way: the input's fake quantizer, the
// normalisation over the last dimension and the affine map forward; from the output's gradient to the gradients of the
// input, gamma and beta backward, in one pass over the activation plus a small combine.  Nothing is kept between the two
// but x, mean and rstd.
//
// x is [rows][n] float32, contiguous, 1 <= n <= 4096; gamma and beta [n] (gamma already weight-quantized); the input
// quantizer (optional, per tensor) is maxval on the device with E / M / S exponent, mantissa and sign bits.
//
// Arithmetic of one row (ln_q and ln_xhat: the ONE definition of q_j and xhat_j, called by both directions, so the
// backward's xhat is the forward's bit for bit):
//   q_j    = fq_apply(x_j)             as fp8a_fp8_quantize computes it -- the fq_fast form where fq_fast_ok holds and
//                                      option "fq_fast" is on (the same value bit for bit); no quantizer: q_j = x_j
//   mean   = (float)(sum_j (double)q_j / (double)n)
//   d_j    = q_j - mean                one fp32 subtraction
//   var    = (float)(sum_j (double)(d_j * d_j) / (double)n)    two-pass, from the registers: the fp32 product widened
//   rstd   = 1.0f / sqrtf(var + eps)   one fp32 add, IEEE sqrtf, IEEE division (no approximate rsqrt)
//   xhat_j = d_j * rstd                one fp32 multiply
//   y_j    = fmaf(xhat_j, gamma_j, beta_j)      the only fused operation (the unit is built with -ffp-contract=off)
// The forward writes mean[rows], rstd[rows]; thread 0 of workgroup 0 writes the quantizer's float and int32 bias, as
// fqt_write_bias does.
// Backward, from x, g, gamma, mean, rstd:
//   w_j    = the clamp weight of fq_train.h -- fqt_weights(fqt_code(x_j, lo, maxval, S)): 1 inside (lo, maxval), 1/2 on
//            a bound, 0 outside (and for a NaN); 1 without a quantizer
//   gy_j   = g_j * gamma_j
//   c1     = sum_j (double)gy_j / (double)n,  c2 = sum_j (double)(gy_j * xhat_j) / (double)n      both stay in double
//   dq_j   = rstd * (float)(((double)gy_j - c1) - (double)xhat_j * c2)      the bracket in double (subtract, multiply,
//            subtract), rounded to fp32 ONCE, then one fp32 multiply.  The row constants are not rounded to fp32 and
//            the bracket's two cancelling differences are not rounded one by one: on a short row with an outlier
//            (12 values, one at 4 sigma) the all-fp32 form of this line was 2 ulp of the row's largest dx off.
//   dx_j   = w_j * dq_j                                a multiplication, as fq_train.h's (no quantizer: dx_j = dq_j)
//   dbeta_j = sum_rows (double)g_j,  dgamma_j = sum_rows (double)(g_j * xhat_j),  each rounded to fp32 once
//   dx may alias g: a thread reads its elements of g before it writes the same elements of dx.
// n = 1: mean = q, d = 0, xhat = 0, y = beta; c1 = gy, c2 = 0, dx = 0 exactly.  A constant row whose sum is exact in
// double (any fp32 constant: n <= 4096 < 2^29) has d = 0 and y = beta bit for bit.
//
// Accumulation types.  Every sum is in double, of fp32 values (or fp32 products) widened: a row's values span a few
// binades around an offset of several sigma, so an fp32 sum's error in mean (~ n^(1/2) ulp of the offset) would reach
// every xhat of the row at full size, while a double sum of at most 4096 (rows: 2^31) fp32 terms is exact to far
// below an fp32 ulp of the result and is rounded ONCE.  It also makes the result independent of the precision of the
// order (the order is still fixed, below).  The cost is two v_cvt + v_add_f64 per value in a kernel that waits on HBM.
//
// The fixed order of every sum: a thread adds its own values in index order; the 64 lanes of a wave are summed by the
// xor butterfly (offsets 32, 16, ..., 1: every lane ends with the same bits); the waves of a workgroup-wide row are
// added in wave order.  dgamma / dbeta: a workgroup owns a run of ln_run(rows) consecutive rows and writes ONE double
// partial per column and output into the workspace part[2][parts][n]; ln_combine_kernel adds a column's partials in
// workgroup order -- 16 slices of consecutive workgroups, each in order, then the 16 slice sums in slice order -- and
// rounds to fp32 once.  No floating-point atomics.  The partition depends on rows alone, the form on n and on the
// 16-byte alignment of the pointers alone: two calls return identical bytes.
//
// Forms (ln_form), each in a scalar and a float4 version (n % 4 == 0 and x, g, out, gamma, beta 16-byte aligned: every
// row then starts on 16 bytes):
//   1 <= n <= 1024     WAVE PER ROW.  A workgroup of 256 threads owns its run of rows, wave w rows r0 + w, r0 + w + 4,
//                      ...  float4: lane l holds the float4s l, l + 64, ... of the row, V = 1 .. 4 of them (ViT-B/16's
//                      n = 768 is V = 3: three 16-byte loads per lane and tensor); scalar: elements l, l + 64, ..., V =
//                      1, 2, 4, 8 or 16.  Lanes own fixed columns, so gamma (and beta) are read once per wave and the
//                      wave's dgamma / dbeta partials stay in registers over all its rows; the row's sums are
//                      butterflies.  LDS only once at the end: waves 1 .. 3 hand their partials to wave 0, which adds
//                      them in wave order (dgamma, then dbeta through the same array).
//   1024 < n <= 4096   WORKGROUP PER ROW.  256 threads x 16 values (4 float4s), the row resident in registers as
//                      bn_bwd_resident_kernel keeps a channel; the workgroup walks its run of rows, a thread owns its
//                      columns' partials and writes them itself.  A row's two sums go through one LDS array each (so a
//                      barrier per sum is enough, also from one row to the next: a wave that rewrites the first array
//                      has passed the second sum's barrier, which every wave reaches after reading the first).
// All element offsets are 64-bit.
#pragma once
#include "fp8approx_common.h"
#include "fq_train.h"

namespace fp8a {

constexpr int LN_NT = 256;               // threads per workgroup
constexpr int LN_WAVES = LN_NT / 64;
constexpr int LN_WAVE_MAX = 1024;        // longest row of the wave form
constexpr int LN_MAX = 4096;             // longest row at all (256 threads x 16 values)
constexpr int LN_RUN_MIN = 8;            // a workgroup's run of rows: the smallest power of two in [8, 64] that
constexpr int LN_RUN_MAX = 64;           //   leaves at most LN_WG_TARGET workgroups (64 beyond that)
constexpr int LN_WG_TARGET = 1024;
constexpr int LN_CB_COLS = 16;           // ln_combine_kernel: columns and slices per workgroup
constexpr int LN_CB_SLICES = LN_NT / LN_CB_COLS;

struct LnArgs {
    int64_t rows;
    int n, run, parts, vec;
    float eps;
    const float *x, *gamma, *beta;
    const float *g;            // backward: the gradient of y
    float *out;                // forward: y; backward: dx (may be g)
    float *mean_out, *rstd_out;         // forward
    const float *mean, *rstd;           // backward
    const float *maxval;       // device [1]; nullptr: no quantizer
    int E, M, S, fq_fast;
    float *bias_out;           // forward, or nullptr
    int32_t *ibias_out;
    double *part;              // backward: [2][parts][n], dgamma's partials then dbeta's
    float *dgamma, *dbeta;
};

static inline int ln_run(int64_t rows) {
    int r = LN_RUN_MIN;
    while (r < LN_RUN_MAX && (rows + r - 1) / r > LN_WG_TARGET) r *= 2;
    return r;
}
static inline int64_t ln_parts(int64_t rows) { return (rows + ln_run(rows) - 1) / ln_run(rows); }

// the wave form's V (float4s or elements per lane); 0: the workgroup form
static inline int ln_form(int64_t n, bool vec) {
    if (n > LN_WAVE_MAX) return 0;
    if (vec) return (int)((n + 255) / 256);
    int v = 1;
    while (64 * v < n) v *= 2;
    return v;
}

#if FP8A_OWN_LN
// The quantizer's constants (uniform); q.on = false: none.
struct LnQ {
    bool on;
    float mx, lo, bias;
    int M, S;
    FqFast k;
};
__device__ __forceinline__ LnQ ln_q_consts(const LnArgs &a) {
    LnQ q{};
    q.on = a.maxval != nullptr;
    q.M = a.M;
    q.S = a.S;
    if (q.on) {
        q.mx = *a.maxval;
        q.lo = a.S ? -q.mx : 0.0f;
        q.bias = fq_bias(q.mx, a.E, a.M);
        q.k = a.fq_fast && fq_fast_ok(q.mx, q.bias, a.M) ? fq_fast_k(q.mx, q.bias, a.M) : FqFast{0u, 0u, q.mx};
    }
    return q;
}
__device__ __forceinline__ void ln_write_bias(const LnArgs &a, const LnQ &q) {
    if (q.on && blockIdx.x == 0 && threadIdx.x == 0) {
        if (a.bias_out) a.bias_out[0] = q.bias;
        if (a.ibias_out) a.ibias_out[0] = (int32_t)q.bias;
    }
}

// q_j and xhat_j of the header: both directions call these two and nothing else for them.
__device__ __forceinline__ float ln_q(const LnQ &q, float x) {
    return q.on ? fq_apply_f<true>(x, q.mx, q.bias, q.M, q.S, q.k) : x;
}
__device__ __forceinline__ float ln_xhat(float qj, float mean, float rstd) {
    const float d = qj - mean;
    return d * rstd;
}

// The wave's butterfly, then (W > 1) the workgroup's waves in wave order through lds[W].  Every thread returns the
// same bits.
template <int W>
__device__ __forceinline__ double ln_reduce(double v, double *lds) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (W > 1) {
        if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
        __syncthreads();
        v = lds[0];
#pragma unroll
        for (int w = 1; w < W; ++w) v += lds[w];
    }
    return v;
}

// Slot k = j VEC + c of thread t (of T per row) is element (t + j T) VEC + c; slot j's VEC elements are live
// together (VEC = 4 only where n % 4 == 0).
template <int VEC, int T>
__device__ __forceinline__ bool ln_live(int n, int t, int j) { return (t + j * T) * VEC < n; }

template <int V, int VEC, int T, typename F>
__device__ __forceinline__ void ln_load(const F *p, int n, int t, F (&v)[V * VEC]) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int e = (t + j * T) * VEC;
        if constexpr (VEC == 4) {
            const float4 f = e < n ? *reinterpret_cast<const float4 *>(p + e) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            v[4 * j] = f.x; v[4 * j + 1] = f.y; v[4 * j + 2] = f.z; v[4 * j + 3] = f.w;
        } else {
            v[j] = e < n ? p[e] : 0.0f;
        }
    }
}
template <int V, int VEC, int T>
__device__ __forceinline__ void ln_store(float *p, int n, int t, const float (&v)[V * VEC]) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int e = (t + j * T) * VEC;
        if (e < n) {
            if constexpr (VEC == 4) *reinterpret_cast<float4 *>(p + e) = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
            else p[e] = v[j];
        }
    }
}
template <int V, int VEC, int T>
__device__ __forceinline__ void ln_store_part(double *p, int n, int t, const double (&v)[V * VEC]) {
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int e = (t + j * T) * VEC;
        if (e < n) {
#pragma unroll
            for (int c = 0; c < VEC; ++c) p[e + c] = v[j * VEC + c];
        }
    }
}

template <int V, int VEC, int W>
__device__ __forceinline__ void ln_forward_row(const LnArgs &a, const LnQ &q, int64_t r, int t,
                                               const float (&gam)[V * VEC], const float (&bet)[V * VEC], double *l0,
                                               double *l1) {
    constexpr int T = 64 * W;
    float v[V * VEC];
    ln_load<V, VEC, T>(a.x + r * a.n, a.n, t, v);
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            v[j * VEC + c] = ln_q(q, v[j * VEC + c]);
            if (ln_live<VEC, T>(a.n, t, j)) s += (double)v[j * VEC + c];
        }
    }
    const float mean = (float)(ln_reduce<W>(s, l0) / (double)a.n);
    double s2 = 0.0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            const float d = v[j * VEC + c] - mean;
            if (ln_live<VEC, T>(a.n, t, j)) s2 += (double)(d * d);
        }
    }
    const float var = (float)(ln_reduce<W>(s2, l1) / (double)a.n);
    const float rstd = 1.0f / sqrtf(var + a.eps);
#pragma unroll
    for (int k = 0; k < V * VEC; ++k) v[k] = fmaf(ln_xhat(v[k], mean, rstd), gam[k], bet[k]);
    ln_store<V, VEC, T>(a.out + r * a.n, a.n, t, v);
    if (t == 0) {
        a.mean_out[r] = mean;
        a.rstd_out[r] = rstd;
    }
}

// One row of the backward; dgam / dbet: the thread's partial sums of its columns over the rows it walks.
template <int V, int VEC, int W>
__device__ __forceinline__ void ln_backward_row(const LnArgs &a, const LnQ &q, int64_t r, int t,
                                                const float (&gam)[V * VEC], double (&dgam)[V * VEC],
                                                double (&dbet)[V * VEC], double *l0, double *l1) {
    constexpr int T = 64 * W;
    float xh[V * VEC], gy[V * VEC], w[V * VEC];
    ln_load<V, VEC, T>(a.x + r * a.n, a.n, t, xh);
    ln_load<V, VEC, T>(a.g + r * a.n, a.n, t, gy);
    const float mean = a.mean[r], rstd = a.rstd[r];
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
#pragma unroll
        for (int c = 0; c < VEC; ++c) {
            const int k = j * VEC + c;
            w[k] = 1.0f;
            if (q.on) {
                float wm;
                fqt_weights(fqt_code(xh[k], q.lo, q.mx, q.S), q.S, w[k], wm);
            }
            xh[k] = ln_xhat(ln_q(q, xh[k]), mean, rstd);
            if (ln_live<VEC, T>(a.n, t, j)) {
                dgam[k] += (double)(gy[k] * xh[k]);
                dbet[k] += (double)gy[k];
                gy[k] = gy[k] * gam[k];
                s1 += (double)gy[k];
                s2 += (double)(gy[k] * xh[k]);
            }
        }
    }
    const double c1 = ln_reduce<W>(s1, l0) / (double)a.n;
    const double c2 = ln_reduce<W>(s2, l1) / (double)a.n;
#pragma unroll
    for (int k = 0; k < V * VEC; ++k) {
        const float dq = rstd * (float)(((double)gy[k] - c1) - (double)xh[k] * c2);
        gy[k] = q.on ? w[k] * dq : dq;
    }
    ln_store<V, VEC, T>(a.out + r * a.n, a.n, t, gy);
}

// Wave per row: n <= 64 V VEC.
template <int V, int VEC, bool BWD>
__global__ __launch_bounds__(LN_NT) void ln_wave_kernel(const LnArgs a) {
    constexpr int N = V * VEC;
    __shared__ double lds[BWD ? (LN_WAVES - 1) * N * 64 : 1];
    const LnQ q = ln_q_consts(a);
    if (!BWD) ln_write_bias(a, q);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * a.run;
    const int64_t r1 = r0 + a.run < a.rows ? r0 + a.run : a.rows;
    float gam[N];
    ln_load<V, VEC, 64>(a.gamma, a.n, lane, gam);
    if constexpr (!BWD) {
        float bet[N];
        ln_load<V, VEC, 64>(a.beta, a.n, lane, bet);
        for (int64_t r = r0 + wave; r < r1; r += LN_WAVES) ln_forward_row<V, VEC, 1>(a, q, r, lane, gam, bet, nullptr, nullptr);
    } else {
        double dgam[N], dbet[N];
#pragma unroll
        for (int k = 0; k < N; ++k) dgam[k] = dbet[k] = 0.0;
        for (int64_t r = r0 + wave; r < r1; r += LN_WAVES)
            ln_backward_row<V, VEC, 1>(a, q, r, lane, gam, dgam, dbet, nullptr, nullptr);
        // the four waves' partials in wave order: dgamma (pass 0), then dbeta through the same array
#pragma unroll
        for (int pass = 0; pass < 2; ++pass) {
            double(&acc)[N] = pass ? dbet : dgam;
            if (wave > 0) {
#pragma unroll
                for (int k = 0; k < N; ++k) lds[((wave - 1) * N + k) * 64 + lane] = acc[k];
            }
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int k = 0; k < N; ++k) {
#pragma unroll
                    for (int u = 0; u < LN_WAVES - 1; ++u) acc[k] += lds[(u * N + k) * 64 + lane];
                }
                ln_store_part<V, VEC, 64>(a.part + ((int64_t)pass * a.parts + blockIdx.x) * a.n, a.n, lane, acc);
            }
            __syncthreads();
        }
    }
}

// Workgroup per row: n <= 4096.
template <int VEC, bool BWD>
__global__ __launch_bounds__(LN_NT) void ln_row_kernel(const LnArgs a) {
    constexpr int N = LN_MAX / LN_NT, V = N / VEC;
    __shared__ double l0[LN_WAVES], l1[LN_WAVES];
    const LnQ q = ln_q_consts(a);
    if (!BWD) ln_write_bias(a, q);
    const int t = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * a.run;
    const int64_t r1 = r0 + a.run < a.rows ? r0 + a.run : a.rows;
    float gam[N];
    ln_load<V, VEC, LN_NT>(a.gamma, a.n, t, gam);
    if constexpr (!BWD) {
        float bet[N];
        ln_load<V, VEC, LN_NT>(a.beta, a.n, t, bet);
        for (int64_t r = r0; r < r1; ++r) ln_forward_row<V, VEC, LN_WAVES>(a, q, r, t, gam, bet, l0, l1);
    } else {
        double dgam[N], dbet[N];
#pragma unroll
        for (int k = 0; k < N; ++k) dgam[k] = dbet[k] = 0.0;
        for (int64_t r = r0; r < r1; ++r) ln_backward_row<V, VEC, LN_WAVES>(a, q, r, t, gam, dgam, dbet, l0, l1);
        ln_store_part<V, VEC, LN_NT>(a.part + (int64_t)blockIdx.x * a.n, a.n, t, dgam);
        ln_store_part<V, VEC, LN_NT>(a.part + ((int64_t)a.parts + blockIdx.x) * a.n, a.n, t, dbet);
    }
}

// dgamma / dbeta from the workgroups' partials: thread (slice s, column c) adds the partials of slice s's
// consecutive workgroups in order, thread (0, c) the 16 slice sums in slice order, rounding once.
__global__ __launch_bounds__(LN_NT) void ln_combine_kernel(const LnArgs a) {
    __shared__ double lg[LN_CB_SLICES][LN_CB_COLS], lb[LN_CB_SLICES][LN_CB_COLS];
    const int c = threadIdx.x % LN_CB_COLS, s = threadIdx.x / LN_CB_COLS;
    const int col = blockIdx.x * LN_CB_COLS + c;
    const int chunk = (a.parts + LN_CB_SLICES - 1) / LN_CB_SLICES;
    const int p0 = s * chunk < a.parts ? s * chunk : a.parts;
    const int p1 = p0 + chunk < a.parts ? p0 + chunk : a.parts;
    double sg = 0.0, sb = 0.0;
    if (col < a.n) {
        for (int p = p0; p < p1; ++p) {
            sg += a.part[(int64_t)p * a.n + col];
            sb += a.part[((int64_t)a.parts + p) * a.n + col];
        }
    }
    lg[s][c] = sg;
    lb[s][c] = sb;
    __syncthreads();
    if (s == 0 && col < a.n) {
#pragma unroll
        for (int u = 1; u < LN_CB_SLICES; ++u) {
            sg += lg[u][c];
            sb += lb[u][c];
        }
        a.dgamma[col] = (float)sg;
        a.dbeta[col] = (float)sb;
    }
}
#endif  // FP8A_OWN_LN

}  // namespace fp8a
