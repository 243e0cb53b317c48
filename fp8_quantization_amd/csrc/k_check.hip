// k_check.hip -- the fused self-check kernels (gemm_check.h: gemm_check_kernel, its batched form
// gemm_bmm_check_kernel and the one-workgroup stats reduction) in their own translation unit.
// Launchers: fp8approx_launch.h, gemm_check.h.
#define FP8A_OWN_CHECK 1
#include "fp8approx_launch.h"
#include "gemm_check.h"

namespace fp8a {

size_t check_part_bytes(int64_t parts) { return (size_t)parts * sizeof(CheckPart); }

void launch_check(const GemmArgs &a, const CheckArgs &c, hipStream_t s) {
    const int64_t tiles = ((a.M + CK_BM - 1) / CK_BM) * c.tiles_n;
    gemm_check_kernel<<<dim3((unsigned)tiles, (unsigned)c.groups), CK_NT, 0, s>>>(a, c);
    check_reduce_kernel<<<1, CK_NT, 0, s>>>(c, tiles * c.groups, a.M, a.N, a.K, a.flags);
}

void launch_bmm_check(const BmmCheckArgs &a, const CheckArgs &c, int64_t items, hipStream_t s) {
    gemm_bmm_check_kernel<<<dim3((unsigned)(a.tiles * items)), CK_NT, 0, s>>>(a);
    // (c.groups = items: the totals are items x M N, M K, K N, M N K)
    check_reduce_kernel<<<1, CK_NT, 0, s>>>(c, a.tiles * items, a.M, a.N, a.K, a.flags);
}

}  // namespace fp8a
