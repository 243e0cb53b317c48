// k_mse.hip -- the FP8 MSE candidate-search kernels (fq_mse.h) in their own translation unit.
// Launcher: fp8approx_launch.h.
#define FP8A_OWN_MSE 1
#include "fp8approx_launch.h"
#include "fq_mse.h"

namespace fp8a {

void launch_mse(const MseArgs &a, bool group, hipStream_t s) {
    const int nc = a.n_mbits * a.n_cand;
    const int64_t total = a.rows * nc;
    const unsigned small = (unsigned)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 65536));
    const size_t lds = (size_t)nc * (MSE_WAVES * sizeof(double) + sizeof(MseCand));
    const unsigned wgs = (unsigned)(a.rows * a.parts);
    mse_prep_kernel<<<small, 256, 0, s>>>(a);
    if (group) mse_search_kernel<true><<<wgs, MSE_NT, lds, s>>>(a);
    else mse_search_kernel<false><<<wgs, MSE_NT, lds, s>>>(a);
    mse_reduce_kernel<<<small, 256, 0, s>>>(a);
}

}  // namespace fp8a
