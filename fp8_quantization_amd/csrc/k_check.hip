// k_check.hip -- the fused self-check kernels (gemm_check.h: gemm_check_kernel, the one body of the
// matrix, batched and convolution entries in its two instances, and the one-workgroup stats reduction)
// in their own translation unit.  Launcher: fp8approx_launch.h.
#define FP8A_OWN_CHECK 1
#include "fp8approx_launch.h"
#include "gemm_check.h"

namespace fp8a {

size_t check_part_bytes(int64_t parts) { return (size_t)parts * sizeof(CheckPart); }

void launch_check(const CheckArgs &c, hipStream_t s) {
    const int64_t parts = c.units * c.tiles;  // workgroup b: unit b / tiles, tile b % tiles, part b
    if (c.conv) gemm_check_kernel<true><<<dim3((unsigned)parts), CK_NT, 0, s>>>(c);
    else gemm_check_kernel<false><<<dim3((unsigned)parts), CK_NT, 0, s>>>(c);
    check_reduce_kernel<<<1, CK_NT, 0, s>>>(c, parts, c.M, c.N, c.K, c.flags);
}

}  // namespace fp8a
