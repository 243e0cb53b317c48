// k_gradconv.hip -- the implicit-GEMM convolution backward (gemm_grad_conv.h: conv_dgrad_kernel of
// fp8a_grad_conv2d_dgrad, conv_wgrad_kernel / conv_wgrad_split_kernel of fp8a_grad_conv2d_wgrad) in its own
// translation unit; the reduce pass and the recomputed-tile counter are k_grad.hip's.
#define FP8A_OWN_GRAD_CONV 1
#include "gemm_grad_conv.h"

namespace fp8a {

void launch_conv_dgrad(const ConvGradArgs &a, unsigned blocks, hipStream_t s) {
    conv_dgrad_kernel<<<dim3(blocks), 256, 0, s>>>(a);
}

void launch_conv_wgrad(const ConvGradArgs &a, const GradArgs &r, int64_t S, int64_t per, float *ws, hipStream_t s) {
    const int64_t blocks = (int64_t)a.num_mt * a.num_nt * a.G;
    if (S == 1) {
        conv_wgrad_kernel<<<dim3((unsigned)blocks), 256, 0, s>>>(a);
        return;
    }
    conv_wgrad_split_kernel<<<dim3((unsigned)(blocks * S)), 256, 0, s>>>(a, ws, (uint32_t)(per * GR_BK));
    launch_grad_reduce(r, a.G, S, ws, s);
}

}  // namespace fp8a
