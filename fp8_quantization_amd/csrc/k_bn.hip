// k_bn.hip -- the training-mode batch-norm kernels (bn_train.h) in their own translation unit.
// Launcher: fp8approx_launch.h.
#define FP8A_OWN_BN 1
#include "fp8approx_launch.h"
#include "bn_train.h"

namespace fp8a {

void launch_bn_train(const BnArgs &a, hipStream_t s) {
    if (bn_lin(a.inner))
        bn_stats_lin_kernel<<<(unsigned)(((a.C + 63) / 64) * a.parts), BN_NT, 0, s>>>(a);
    else
        bn_stats_kernel<<<(unsigned)(a.C * a.parts), BN_NT, 0, s>>>(a);
    bn_finalize_kernel<<<(unsigned)((a.C + 255) / 256), 256, 0, s>>>(a);
    if (a.y == nullptr) return;
    const int64_t total = a.N * a.C * a.inner, work = a.vec ? total / 4 : total;
    const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 2048));
    if (total < ((int64_t)1 << 31)) bn_apply_kernel<uint32_t><<<blocks, 256, 0, s>>>(a);
    else bn_apply_kernel<uint64_t><<<blocks, 256, 0, s>>>(a);
}

}  // namespace fp8a
