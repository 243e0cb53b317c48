// k_grad.hip -- gemm_grad_kernel (gemm_grad.h: the gradient GEMM of fp8a_grad_bmm) and the two passes of its
// split along K (gemm_grad_split_kernel, grad_reduce_kernel: fp8a_grad_bmm_split) in their own translation
// unit, with the recomputed-tile counter.
#define FP8A_OWN_GRAD 1
#include "gemm_grad.h"

namespace fp8a {

__device__ unsigned long long g_grad_recomputed;

unsigned long long *grad_recount_ptr() {
    static unsigned long long *ptr = [] {
        void *q = nullptr;
        if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_grad_recomputed)) != hipSuccess) {
            (void)hipGetLastError();
            q = nullptr;
        }
        return (unsigned long long *)q;
    }();
    return ptr;
}

int grad_recount_read(unsigned long long *v, bool reset) {
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_grad_recomputed), sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_grad_recomputed), &z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}

void launch_grad(const GradArgs &a, dim3 grid, hipStream_t s) { gemm_grad_kernel<<<grid, 256, 0, s>>>(a); }

void launch_grad_split(const GradArgs &a, int64_t nb, int64_t S, int64_t per, float *ws, hipStream_t s) {
    gemm_grad_split_kernel<<<dim3((unsigned)(a.tiles * nb * S)), 256, 0, s>>>(a, ws, nb, (uint32_t)(per * GR_BK));
    grad_reduce_kernel<<<dim3((unsigned)(a.tiles * nb), GR_T / 4), 256, 0, s>>>(a, ws, nb, (int)S);
}

}  // namespace fp8a
