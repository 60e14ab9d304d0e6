// pt_adaptive_select.h — the per-round rules of adaptive sampling (include/pt_adaptive.h): the convergence test of a pixel and
// the keep rule (dilation by the 3x3 neighbourhood), as PT_HD functions that the engine's mark / keep kernels (pt_engine.hip) and the host emulation
// of the tests compile from the same text.
#ifndef PT_ADAPTIVE_SELECT_H
#define PT_ADAPTIVE_SELECT_H
#include <stdint.h>

#include "../../include/pt_numerics.h"

namespace ptd {

// A pixel of n samples whose Y terms sum to s1 (and their squares to s2, both in f64) is NOT converged unless
//   (n * s2 - s1 * s1) <= (n - 1) * M * M,   M = max(rel_error * s1, abs_error * n).
// Multiplies, subtracts and a max only — no sqrt, no division —, so the decision is exact and a numpy restatement gets it bit for bit.
// A NaN makes the comparison false: such a pixel runs to max_samples.
PT_HD bool adaptive_unconverged(uint32_t n, double s1, double s2, float rel_error, float abs_error) {
    const double nd = (double)n;
    const double a = (double)rel_error * s1, b = (double)abs_error * nd;
    const double m = a > b ? a : b;
    const double lhs = nd * s2 - s1 * s1;
    const double rhs = (nd - 1.0) * m * m;
    return !(lhs <= rhs);
}

// A pixel of the current list (n samples) goes on to the next round when n < max_samples and some pixel of its 3x3 neighbourhood inside the film
// (itself included) is marked in `unconverged` — the byte image that holds 1 exactly for the pixels of the current list that are not converged.
PT_HD bool adaptive_keep(const uint8_t* unconverged, uint32_t width, uint32_t height, uint32_t pixel, uint32_t n, uint32_t max_samples) {
    if (n >= max_samples) return false;
    const uint32_t x = pixel % width, y = pixel / width;
    const uint32_t x0 = x > 0u ? x - 1u : 0u, x1 = x + 1u < width ? x + 1u : x;
    const uint32_t y0 = y > 0u ? y - 1u : 0u, y1 = y + 1u < height ? y + 1u : y;
    bool any = false;
    for (uint32_t yy = y0; yy <= y1; ++yy)
        for (uint32_t xx = x0; xx <= x1; ++xx) any = any || unconverged[yy * width + xx] != 0u;
    return any;
}

}  // namespace ptd
#endif
