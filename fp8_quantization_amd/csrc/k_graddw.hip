// k_graddw.hip -- the depthwise convolution backward (gemm_grad_dw.h: dwconv_dgrad_kernel of
// fp8a_grad_dwconv2d_dgrad, dwconv_wgrad_kernel / dwconv_wgrad_reduce_kernel of fp8a_grad_dwconv2d_wgrad) in its own
// translation unit.
#define FP8A_OWN_GRAD_DW 1
#include "gemm_grad_dw.h"

namespace fp8a {

void launch_dw_dgrad(const DwGradArgs &a, unsigned blocks, hipStream_t s) {
    const bool k3 = a.kh == 3 && a.kw == 3 && a.dh == 1 && a.dw == 1 && a.ph == 1 && a.pw == 1 && a.sh == a.sw;
    if (k3 && a.sh == 1) dwconv_dgrad_kernel<3, 1><<<dim3(blocks), 256, a.lds, s>>>(a);
    else if (k3 && a.sh == 2) dwconv_dgrad_kernel<3, 2><<<dim3(blocks), 256, a.lds, s>>>(a);
    else dwconv_dgrad_kernel<0, 0><<<dim3(blocks), 256, a.lds, s>>>(a);
}

void launch_dw_wgrad(const DwGradArgs &a, float *ws, hipStream_t s) {
    const unsigned blocks = (unsigned)((int64_t)a.C * a.S);
    if (a.kh == 3 && a.kw == 3) dwconv_wgrad_kernel<3, 3, true><<<dim3(blocks), 256, a.lds, s>>>(a, ws);
    else dwconv_wgrad_kernel<DWG_KMAX, DWG_KMAX, false><<<dim3(blocks), 256, a.lds, s>>>(a, ws);
    if (a.S > 1) {
        const int n = a.C * a.kh * a.kw;
        dwconv_wgrad_reduce_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, s>>>(ws, a.out, n, a.kh * a.kw, a.S);
    }
}

}  // namespace fp8a
