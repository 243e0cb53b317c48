// k_ln.hip -- the layer norm block's forward / backward kernels (layer_norm.h) in their own translation unit.
// Launcher: fp8approx_launch.h.
#define FP8A_OWN_LN 1
#include "fp8approx_launch.h"
#include "layer_norm.h"

namespace fp8a {

template <bool BWD>
static void launch_ln(const LnArgs &a, hipStream_t s) {
    const unsigned grid = (unsigned)a.parts;
    const int v = ln_form(a.n, a.vec != 0);
    if (a.vec) {
        switch (v) {
        case 1: ln_wave_kernel<1, 4, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        case 2: ln_wave_kernel<2, 4, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        case 3: ln_wave_kernel<3, 4, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        case 4: ln_wave_kernel<4, 4, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        default: ln_row_kernel<4, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        }
    } else {
        switch (v) {
        case 1: ln_wave_kernel<1, 1, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        case 2: ln_wave_kernel<2, 1, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        case 4: ln_wave_kernel<4, 1, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        case 8: ln_wave_kernel<8, 1, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        case 16: ln_wave_kernel<16, 1, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        default: ln_row_kernel<1, BWD><<<grid, LN_NT, 0, s>>>(a); break;
        }
    }
}

void launch_layer_norm(const LnArgs &a, bool backward, hipStream_t s) {
    if (!backward) {
        launch_ln<false>(a, s);
        return;
    }
    launch_ln<true>(a, s);
    ln_combine_kernel<<<(unsigned)((a.n + LN_CB_COLS - 1) / LN_CB_COLS), LN_NT, 0, s>>>(a);
}

}  // namespace fp8a
