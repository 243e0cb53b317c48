// k_bmm.hip -- gemm_bmm_kernel (gemm_bmm.h: the batched approx product of fp8a_bmm), one translation unit
// per part P = 2 * S2N + QBMA (build_native.py compiles it four times with -DFP8A_BMM_PART=P, in
// parallel).  Part 0 also owns the recomputed-tile counter.
#define FP8A_OWN_BMM 1
#include "gemm_bmm.h"

#ifndef FP8A_BMM_PART
#error "k_bmm.hip is compiled once per part: -DFP8A_BMM_PART=0..3"
#endif

namespace fp8a {

template <bool S2N, bool QBMA, bool GCLIP>
static void launch_bmm_modes(int mode, const BmmArgs &a, dim3 grid, hipStream_t s) {
    switch (mode) {
        case TM_NONE: gemm_bmm_kernel<S2N, QBMA, GCLIP, TM_NONE, false><<<grid, NT, 0, s>>>(a); break;
        case TM_W1U: gemm_bmm_kernel<S2N, QBMA, GCLIP, TM_W1U, false><<<grid, NT, 0, s>>>(a); break;
        case TM_W2S1: gemm_bmm_kernel<S2N, QBMA, GCLIP, TM_W2S1, false><<<grid, NT, 0, s>>>(a); break;
        case TM_W2U1: gemm_bmm_kernel<S2N, QBMA, GCLIP, TM_W2U1, false><<<grid, NT, 0, s>>>(a); break;
        case TM_W2S2: gemm_bmm_kernel<S2N, QBMA, GCLIP, TM_W2S2, false><<<grid, NT, 0, s>>>(a); break;
        case TM_W2U2: gemm_bmm_kernel<S2N, QBMA, GCLIP, TM_W2U2, false><<<grid, NT, 0, s>>>(a); break;
        default: gemm_bmm_kernel<S2N, QBMA, GCLIP, TM_LUT, false><<<grid, NT, 0, s>>>(a); break;
    }
}

#if FP8A_BMM_PART == 0
__device__ unsigned long long g_bmm_recomputed;

unsigned long long *bmm_recount_ptr() {
    static unsigned long long *ptr = [] {
        void *q = nullptr;
        if (hipGetSymbolAddress(&q, HIP_SYMBOL(g_bmm_recomputed)) != hipSuccess) {
            (void)hipGetLastError();
            q = nullptr;
        }
        return (unsigned long long *)q;
    }();
    return ptr;
}

int bmm_recount_read(unsigned long long *v, bool reset) {
    if (hipMemcpyFromSymbol(v, HIP_SYMBOL(g_bmm_recomputed), sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        const unsigned long long z = 0;
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_bmm_recomputed), &z, sizeof(z)) != hipSuccess) return -1;
    }
    return 0;
}

void launch_bmm_p0(int mode, bool gclip, const BmmArgs &a, dim3 grid, hipStream_t s) {
    if (gclip) launch_bmm_modes<false, false, true>(mode, a, grid, s);
    else launch_bmm_modes<false, false, false>(mode, a, grid, s);
}
#elif FP8A_BMM_PART == 1
void launch_bmm_p1(int mode, bool gclip, const BmmArgs &a, dim3 grid, hipStream_t s) {
    if (gclip) launch_bmm_modes<false, true, true>(mode, a, grid, s);
    else launch_bmm_modes<false, true, false>(mode, a, grid, s);
}
#elif FP8A_BMM_PART == 2
void launch_bmm_p2(int mode, bool gclip, const BmmArgs &a, dim3 grid, hipStream_t s) {
    if (gclip) launch_bmm_modes<true, false, true>(mode, a, grid, s);
    else launch_bmm_modes<true, false, false>(mode, a, grid, s);
}
#else
void launch_bmm_p3(int mode, bool gclip, const BmmArgs &a, dim3 grid, hipStream_t s) {
    if (mode == TM_F8) {
        if (a.Mw == 2) gemm_bmm_kernel<true, true, false, TM_F8, true><<<grid, NT, 0, s>>>(a);
        else gemm_bmm_kernel<true, true, false, TM_F8, false><<<grid, NT, 0, s>>>(a);
    } else if (gclip) launch_bmm_modes<true, true, true>(mode, a, grid, s);
    else launch_bmm_modes<true, true, false>(mode, a, grid, s);
}
#endif

}  // namespace fp8a
