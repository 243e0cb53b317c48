// k_fqt.hip -- the FP8 fake quantizer's training forward / backward kernels (fq_train.h) in their own
// translation unit.  Launchers: fp8approx_launch.h.
#define FP8A_OWN_FQT 1
#include "fp8approx_launch.h"
#include "fq_train.h"

namespace fp8a {

static unsigned fqt_row_blocks(const FqtArgs &a) { return (unsigned)((a.rows + FQT_NT - 1) / FQT_NT); }

void launch_fqt_forward(const FqtArgs &a, hipStream_t s) {
    if (fqt_short(a.inner)) fqt_forward_rows_kernel<<<fqt_row_blocks(a), FQT_NT, 0, s>>>(a);
    else fqt_forward_kernel<<<(unsigned)(a.rows * a.parts), FQT_NT, 0, s>>>(a);
}

// a.parts = 0: an empty row, only the (zero) sums are written
void launch_fqt_backward(const FqtArgs &a, hipStream_t s) {
    if (a.parts > 0) {
        if (fqt_short(a.inner)) fqt_backward_rows_kernel<<<fqt_row_blocks(a), FQT_NT, 0, s>>>(a);
        else fqt_backward_kernel<<<(unsigned)(a.rows * a.parts), FQT_NT, 0, s>>>(a);
    }
    if (fqt_reduce_by_wave(a.parts))
        fqt_reduce_wave_kernel<<<(unsigned)((a.rows + FQT_WAVES - 1) / FQT_WAVES), FQT_NT, 0, s>>>(a);
    else
        fqt_reduce_kernel<<<fqt_row_blocks(a), FQT_NT, 0, s>>>(a);
}

}  // namespace fp8a
