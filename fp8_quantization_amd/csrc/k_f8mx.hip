// k_f8mx.hip -- gemm_f8mx_kernel (gemm_f8mx.h), one translation unit per result-grid form XF
// (-DFP8A_XF_PART=0 / 1 / 2, compiled in parallel by build_native.py); part 0 also holds the
// operand pre-passes xm_decode_a / xm_decode_b.  Launchers: fp8approx_launch.h.
#ifndef FP8A_XF_PART
#error "k_f8mx.hip is compiled once per part: -DFP8A_XF_PART=0..2"
#endif
#define FP8A_OWN_F8MX 1
#define FP8A_OWN_F8MX_DECODE (FP8A_XF_PART == 0)
#include "fp8approx_launch.h"
#include "gemm_f8mx.h"
#include <type_traits>

namespace fp8a {

// f(std::true_type) where b holds and the build allows the `true` form, else f(std::false_type): a runtime
// boolean as a template argument
template <bool ALLOWED, class F>
static void with_bool(bool b, F &&f) {
    if constexpr (ALLOWED) {
        if (b) return f(std::true_type{});
    }
    f(std::false_type{});
}

template <int NCG, int RB, int XF>
static void launch_shape(const GemmArgs &a0, hipStream_t s) {
    using Cf = XmCfg<NCG, RB>;
    const int64_t num_mt = (a0.M + Cf::BMT - 1) / Cf::BMT, xt = num_mt * ((a0.N + Cf::BNT - 1) / Cf::BNT);
    const dim3 g((unsigned)(xt * a0.splits));
    // the kernel's 32-bit tile setup: its divisors' magics, once per launch (xt * splits < 2^31: mx_plan)
    GemmArgs a = a0;
    a.xm_tiles = (uint32_t)xt;
    a.xm_num_mt = (uint32_t)num_mt;
    fastdiv_params(a.xm_tiles, a.xt_mul, a.xt_shift);
    fastdiv_params(a.xm_num_mt, a.xmt_mul, a.xmt_shift);
    if (a.conv) {
        fastdiv_params((uint32_t)(a.Ho * a.Wo), a.ohw_mul, a.ohw_shift);
        fastdiv_params((uint32_t)a.Wo, a.owo_mul, a.owo_shift);
    }
    if (a.nchw) fastdiv_params((uint32_t)a.hw, a.shw_mul, a.shw_shift);
    // Which instance a launch runs -- the one place that says which of gemm_f8mx_kernel's template arguments go
    // together (gemm_f8mx.h explains each):
    //   EMIT  = the launch writes the next convolution's word image from its own store (fp8a_conv2d_chain):
    //           a.em.w, unsplit or split with the in-launch sum
    //   AF32  = a.af32, A staged from fp32
    //   FIX   = the in-launch split-K sum, a.skcnt: E4M3 (XF 0) only
    //   piped = option "xm_pipe" on a word-staged plain form: XF != 2, not AF32
    //   PIPE  = piped ? XmPipe<NCG, EMIT, FIX> : 0  (XmPipe 0, the 256 x 16 split-sum tiles: the unpiped instance)
    //   WROWS = option "xm_wave_rows" on a piped 128 x 64 (NCG 4) instance without FIX
    // A combination the rule excludes is never instantiated (with_bool<false> compiles the `false` arm alone).
    const bool emit = a.em.w != nullptr && (a.splits == 1 || a.skcnt != nullptr);
    // (The nesting, `true` arm first, is also the order of the kernels in the code object.)
    with_bool<XF != 2>(a.xm_pipe && !a.af32, [&](auto piped) {
        with_bool<XF == 0>(a.skcnt != nullptr, [&](auto fix) {
            constexpr bool PIPED = decltype(piped)::value, FIX = decltype(fix)::value;
            with_bool<PIPED && !FIX && NCG == 4>(a.xm_wave_rows != 0, [&](auto wrows) {
                with_bool<!PIPED>(a.af32 != 0, [&](auto af32) {
                    with_bool<true>(emit, [&](auto em) {
                        constexpr bool EMIT = decltype(em)::value;
                        constexpr int PIPE = PIPED ? XmPipe<NCG, EMIT, FIX>::value : 0;
                        gemm_f8mx_kernel<NCG, RB, decltype(af32)::value, XF, EMIT, FIX, PIPE, decltype(wrows)::value>
                            <<<g, Cf::NT, 0, s>>>(a);
                    });
                });
            });
        });
    });
}

template <int XF>
static void launch_xf(const GemmArgs &a, hipStream_t s) {
    if (a.xncg == 1) {
        launch_shape<1, 4, XF>(a, s);
    } else if constexpr (XF == 2) {
        launch_shape<2, 4, XF>(a, s);  // (the halved-block form: at most 32 columns, gemm_f8mx.h)
    } else {
        if (a.xncg == 2) launch_shape<2, 4, XF>(a, s);
        else launch_shape<4, 8, XF>(a, s);
    }
}

static int clock_read(unsigned long long *v, bool reset) {
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_clk), 6 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[6] = {0, 0, 0, 0, 0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_clk), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}

static int signs_read(unsigned long long *v, bool reset) {
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_xm_sign), 2 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z[2] = {0, 0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_xm_sign), z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}

// launch_f8mx_xfN / f8mx_clock_xfN / f8mx_signs_xfN of this unit's part N (fp8approx_launch.h)
#define XF_NAME2(name, part) name##part
#define XF_NAME(name, part) XF_NAME2(name, part)
void XF_NAME(launch_f8mx_xf, FP8A_XF_PART)(const GemmArgs &a, hipStream_t s) { launch_xf<FP8A_XF_PART>(a, s); }
int XF_NAME(f8mx_clock_xf, FP8A_XF_PART)(unsigned long long *v, bool reset) { return clock_read(v, reset); }
int XF_NAME(f8mx_signs_xf, FP8A_XF_PART)(unsigned long long *v, bool reset) { return signs_read(v, reset); }

}  // namespace fp8a
