// k_attn.hip -- the attention softmax block's forward / backward kernels (attn_softmax.h) in their own translation
// unit.  Launcher: fp8approx_launch.h.
#define FP8A_OWN_ATTN 1
#include "fp8approx_launch.h"
#include "attn_softmax.h"

namespace fp8a {

template <bool BWD>
static void launch_attn(const AttnArgs &a, hipStream_t s) {
    const unsigned wave_blocks = (unsigned)((a.rows + ATTN_WAVES - 1) / ATTN_WAVES);
    switch (attn_form(a.n)) {
    case 1: attn_wave_kernel<1, BWD><<<wave_blocks, ATTN_NT, 0, s>>>(a); break;
    case 2: attn_wave_kernel<2, BWD><<<wave_blocks, ATTN_NT, 0, s>>>(a); break;
    case 4: attn_wave_kernel<4, BWD><<<wave_blocks, ATTN_NT, 0, s>>>(a); break;
    case 8: attn_wave_kernel<8, BWD><<<wave_blocks, ATTN_NT, 0, s>>>(a); break;
    case 16: attn_wave_kernel<16, BWD><<<wave_blocks, ATTN_NT, 0, s>>>(a); break;
    default: attn_row_kernel<BWD><<<(unsigned)a.rows, ATTN_NT, 0, s>>>(a); break;
    }
}

void launch_attn_softmax(const AttnArgs &a, bool backward, hipStream_t s) {
    if (backward) launch_attn<true>(a, s);
    else launch_attn<false>(a, s);
}

}  // namespace fp8a
