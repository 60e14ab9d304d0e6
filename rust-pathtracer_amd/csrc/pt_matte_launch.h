// pt_matte_launch.h — launchers of the ID-matte kernels (pt_matte.hip) for the entries of pt_engine.hip and the host-array extract of pt_matte.hip.
#ifndef PT_MATTE_LAUNCH_H
#define PT_MATTE_LAUNCH_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pt_api.h"

namespace ptk {

// The slot table of a matte render: ranks planes of n_pixels 8-byte (key, count) words, slot r of pixel p at word r * n_pixels + p, and behind them the
// overflow plane of n_pixels uint32.
inline size_t matte_table_bytes(uint32_t n_pixels, uint32_t ranks) { return (size_t)n_pixels * (8u * (size_t)ranks + 4u); }
inline uint32_t* matte_table_overflow(void* table, uint32_t n_pixels, uint32_t ranks) {
    return reinterpret_cast<uint32_t*>(static_cast<char*>(table) + 8u * (size_t)ranks * n_pixels);
}

// One sample index of every pixel folded into the table: hits[p] is pixel p's closest hit of that sample (launch_probe_intersect's output).  `first`: the
// table is initialised instead of read.  1 <= ranks <= 8, key_kind PT_MATTE_KEY_*.
hipError_t launch_matte_fold(hipStream_t stream, uint32_t n_pixels, uint32_t ranks, uint32_t key_kind, const pt_hit* hits, void* table, bool first);
// The table sorted and divided: keys and coverage are ranks planes of n_pixels, overflow one plane (any of the three on the device).
hipError_t launch_matte_finish(hipStream_t stream, uint32_t n_pixels, uint32_t ranks, uint32_t samples, const void* table, uint32_t* keys, float* coverage, uint32_t* overflow);
// out (set_count planes of n_pixels floats) from keys and coverage (ranks planes each) and the selections on the device: offsets[set_count + 1] into
// selected, every set sorted ascending without duplicates; set_count <= 16, offsets[set_count] <= 1024 (the callers' argument checks).
hipError_t launch_matte_extract(int grid, hipStream_t stream, uint32_t n_pixels, uint32_t ranks, const uint32_t* keys, const float* coverage, uint32_t set_count,
                                const uint32_t* offsets, const uint32_t* selected, float* out);
// The grid of the extract: one workgroup per 256 pixels, at most 8 per compute unit (the grid-stride loop takes the rest)
inline int matte_extract_grid(int compute_units, uint32_t n_pixels) {
    const uint32_t need = (n_pixels + 255u) / 256u, cap = (uint32_t)(compute_units > 0 ? compute_units : 1) * 8u;
    return (int)(need < cap ? need : cap);
}
// offsets and selected behind each other in one device buffer: the words of that buffer, and where the output planes may start behind it
constexpr uint32_t kMatteSelectionWords = 1088;   // 17 offsets + 1024 keys, rounded up to 256 bytes

}  // namespace ptk
#endif
