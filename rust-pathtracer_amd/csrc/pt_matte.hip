// pt_matte.hip — ID mattes (include/pt_denoise.h) on gfx950: k_matte_fold, k_matte_finish, k_matte_extract, the host-array entry
// pt_matte_extract and the host-only pt_cryptomatte_hash.  The render and the resident entries are pt_engine.hip's (the probes and the resident planes are the
// scene's); they launch these kernels.  The per-pixel rules are pt_matte_rules.h's, the text the host emulation compiles.
//
// All three kernels are one lane per pixel, 256 lanes.  The slot table is plane-major, slot r of pixel p one 8-byte word at r * n + p: the 64 lanes of a wave
// read and write 512 contiguous bytes per slot.  The number of ranks R is a template constant (1 .. 8) and every loop over the slots is unrolled, so the slots
// are registers: an array indexed by a run-time r would go to scratch.
//   fold     reads valid, instance and material of the lane's hit record, reads its R slots, and writes back the one slot the sample changes (or adds one to
//            the lane's overflow word).  The launch of sample 0 writes the whole table instead of reading it, so nothing is cleared beforehand.
//   finish   sorts the slots as 64-bit words (the count's complement above the key) through a 19-exchange network at fixed positions, divides, and writes the
//            keys, the coverage and the overflow plane.
//   extract  loads the lane's R keys and coverages once; the block stages the sorted selections in LDS once (at most 1024 keys and 17 offsets, 4164 bytes);
//            every (set, rank) is a binary search there, and a lane writes one value per set.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/pt_denoise.h"
#include "pt_error.h"
#include "pt_matte_launch.h"
#include "pt_matte_rules.h"
#include "pt_plan.h"

using namespace ptd;

namespace {

constexpr int kBlock = 256;
static_assert(MATTE_SKY == PT_MATTE_SKY && MATTE_NONE == PT_MATTE_NONE && MATTE_RANKS_MAX == PT_MATTE_RANKS_MAX, "the rules' constants are the header's");
static_assert(MATTE_KEY_INSTANCE == (uint32_t)PT_MATTE_KEY_INSTANCE && MATTE_KEY_MATERIAL == (uint32_t)PT_MATTE_KEY_MATERIAL, "the rules' key kinds are the header's");
static_assert(sizeof(MatteSlot) == 8, "a slot is one 8-byte word");
static_assert(ptk::kMatteSelectionWords >= MATTE_SETS_MAX + 1u + MATTE_SELECTED_MAX, "the selection buffer holds the offsets and the keys");

pt_status mfail(pt_status st, const std::string& m) { pt_set_error(m); return st; }

}  // namespace

namespace ptk {

template <int R>
__global__ void __launch_bounds__(kBlock) k_matte_fold(uint32_t n, uint32_t key_kind, const pt_hit* __restrict__ hits, MatteSlot* __restrict__ slots,
                                                      uint32_t* __restrict__ overflow, int first) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const pt_hit* h = hits + p;
    const uint32_t key = matte_sample_key(h->valid, h->instance, h->material, key_kind);
    if (first) {
        slots[p] = MatteSlot{key, 1u};
#pragma unroll
        for (int r = 1; r < R; ++r) slots[(size_t)r * n + p] = MatteSlot{0u, 0u};
        overflow[p] = 0u;
        return;
    }
    MatteSlot s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = slots[(size_t)r * n + p];
    const int slot = matte_fold_slot<R>(s, key);
    if (slot == R) overflow[p] = overflow[p] + 1u;
    else slots[(size_t)slot * n + p] = matte_fold_value<R>(s, slot, key);
}

template <int R>
__global__ void __launch_bounds__(kBlock) k_matte_finish(uint32_t n, uint32_t samples, const MatteSlot* __restrict__ slots, const uint32_t* __restrict__ overflow_in,
                                                        uint32_t* __restrict__ keys, float* __restrict__ coverage, uint32_t* __restrict__ overflow) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    MatteSlot s[R];
#pragma unroll
    for (int r = 0; r < R; ++r) s[r] = slots[(size_t)r * n + p];
    uint32_t k[R];
    float c[R];
    matte_finish_pixel<R>(s, samples, k, c);
#pragma unroll
    for (int r = 0; r < R; ++r) { keys[(size_t)r * n + p] = k[r]; coverage[(size_t)r * n + p] = c[r]; }
    overflow[p] = overflow_in[p];
}

template <int R>
__global__ void __launch_bounds__(kBlock) k_matte_extract(uint32_t n, const uint32_t* __restrict__ keys, const float* __restrict__ coverage, uint32_t set_count,
                                                         const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ selected, float* __restrict__ out) {
    __shared__ uint32_t s_selected[MATTE_SELECTED_MAX];
    __shared__ uint32_t s_offsets[MATTE_SETS_MAX + 1u];
    // (the launcher refuses more sets; the clamps keep a bad table of offsets inside the two arrays)
    const uint32_t sets = set_count < MATTE_SETS_MAX ? set_count : MATTE_SETS_MAX;
    const uint32_t total = offsets[sets] < MATTE_SELECTED_MAX ? offsets[sets] : MATTE_SELECTED_MAX;
    for (uint32_t i = threadIdx.x; i <= sets; i += blockDim.x) s_offsets[i] = offsets[i] < total ? offsets[i] : total;
    for (uint32_t i = threadIdx.x; i < total; i += blockDim.x) s_selected[i] = selected[i];
    __syncthreads();
    for (uint32_t p = blockIdx.x * blockDim.x + threadIdx.x; p < n; p += gridDim.x * blockDim.x) {
        uint32_t k[R];
        float c[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { k[r] = keys[(size_t)r * n + p]; c[r] = coverage[(size_t)r * n + p]; }
        for (uint32_t m = 0; m < sets; ++m) out[(size_t)m * n + p] = matte_extract_pixel<R>(k, c, s_selected, s_offsets[m], s_offsets[m + 1u]);
    }
}

}  // namespace ptk

namespace {

// the kernel of a family for a run-time number of ranks
#define PT_MATTE_RANKS(call) \
    switch (ranks) { \
        case 1: call(1); break; case 2: call(2); break; case 3: call(3); break; case 4: call(4); break; \
        case 5: call(5); break; case 6: call(6); break; case 7: call(7); break; default: call(8); break; \
    }

bool launchable(uint32_t n_pixels, uint32_t ranks) { return n_pixels != 0 && n_pixels <= 0x7fffffffu && ranks != 0 && ranks <= (uint32_t)MATTE_RANKS_MAX; }
dim3 pixel_grid(uint32_t n_pixels) { return dim3((n_pixels + (uint32_t)kBlock - 1u) / (uint32_t)kBlock); }

struct Dev {
    void* p = nullptr;
    Dev() = default;
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    ~Dev() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 4); }
    template <typename T> T* as() const { return static_cast<T*>(p); }
};

}  // namespace

namespace ptk {

hipError_t launch_matte_fold(hipStream_t stream, uint32_t n_pixels, uint32_t ranks, uint32_t key_kind, const pt_hit* hits, void* table, bool first) {
    if (!launchable(n_pixels, ranks) || key_kind > MATTE_KEY_MATERIAL) return hipErrorInvalidValue;
    MatteSlot* slots = static_cast<MatteSlot*>(table);
    uint32_t* overflow = matte_table_overflow(table, n_pixels, ranks);
#define PT_MATTE_FOLD(R) hipLaunchKernelGGL(k_matte_fold<R>, pixel_grid(n_pixels), dim3(kBlock), 0, stream, n_pixels, key_kind, hits, slots, overflow, first ? 1 : 0)
    PT_MATTE_RANKS(PT_MATTE_FOLD)
#undef PT_MATTE_FOLD
    return hipGetLastError();
}

hipError_t launch_matte_finish(hipStream_t stream, uint32_t n_pixels, uint32_t ranks, uint32_t samples, const void* table, uint32_t* keys, float* coverage, uint32_t* overflow) {
    if (!launchable(n_pixels, ranks) || samples == 0 || samples > MATTE_SAMPLES_MAX) return hipErrorInvalidValue;
    const MatteSlot* slots = static_cast<const MatteSlot*>(table);
    const uint32_t* overflow_in = matte_table_overflow(const_cast<void*>(table), n_pixels, ranks);
#define PT_MATTE_FINISH(R) hipLaunchKernelGGL(k_matte_finish<R>, pixel_grid(n_pixels), dim3(kBlock), 0, stream, n_pixels, samples, slots, overflow_in, keys, coverage, overflow)
    PT_MATTE_RANKS(PT_MATTE_FINISH)
#undef PT_MATTE_FINISH
    return hipGetLastError();
}

hipError_t launch_matte_extract(int grid, hipStream_t stream, uint32_t n_pixels, uint32_t ranks, const uint32_t* keys, const float* coverage, uint32_t set_count,
                                const uint32_t* offsets, const uint32_t* selected, float* out) {
    if (!launchable(n_pixels, ranks) || set_count == 0 || set_count > MATTE_SETS_MAX || grid <= 0) return hipErrorInvalidValue;
#define PT_MATTE_EXTRACT(R) hipLaunchKernelGGL(k_matte_extract<R>, dim3(grid), dim3(kBlock), 0, stream, n_pixels, keys, coverage, set_count, offsets, selected, out)
    PT_MATTE_RANKS(PT_MATTE_EXTRACT)
#undef PT_MATTE_EXTRACT
    return hipGetLastError();
}

}  // namespace ptk

extern "C" pt_status pt_cryptomatte_hash(const char* name, uint32_t* hash, float* id) {
    if (!name) return mfail(PT_ERR_INVALID_ARGUMENT, "name is null");
    const uint32_t h = matte_murmur3_32(reinterpret_cast<const uint8_t*>(name), strlen(name), 0u);
    if (hash) *hash = h;
    if (id) { const uint32_t bits = matte_id_bits(h); memcpy(id, &bits, 4); }
    return PT_OK;
}

extern "C" pt_status pt_matte_extract(uint32_t width, uint32_t height, uint32_t ranks, const uint32_t* keys, const float* coverage, uint32_t set_count,
                                      const uint32_t* offsets, const uint32_t* selected, uint32_t device, float* out) {
    std::string err;
    const pt_status st = pth::check_matte_extract_args(width, height, ranks, keys, coverage, set_count, offsets, selected, out, &err);
    if (st != PT_OK) return mfail(st, err);
    if (set_count == 0) return PT_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return mfail(PT_ERR_NO_DEVICE, "no HIP device available: the product path has no CPU fallback");
    if (device >= (uint32_t)ndev) return mfail(PT_ERR_INVALID_ARGUMENT, "device: no such HIP device");
    std::vector<uint32_t> selection;
    pth::matte_selection_words(set_count, offsets, selected, &selection);
#define MT_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return mfail(e_ == hipErrorOutOfMemory ? PT_ERR_OUT_OF_MEMORY : PT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)
    MT_TRY(hipSetDevice((int)device));
    int cus = 0;
    MT_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, (int)device));
    const size_t np = (size_t)width * height;
    Dev d_selection, d_keys, d_coverage, d_out;
    MT_TRY(d_selection.alloc(4 * selection.size())); MT_TRY(d_keys.alloc(4 * ranks * np)); MT_TRY(d_coverage.alloc(4 * ranks * np)); MT_TRY(d_out.alloc(4 * set_count * np));
    MT_TRY(hipMemcpy(d_selection.p, selection.data(), 4 * selection.size(), hipMemcpyHostToDevice));
    MT_TRY(hipMemcpy(d_keys.p, keys, 4 * ranks * np, hipMemcpyHostToDevice));
    MT_TRY(hipMemcpy(d_coverage.p, coverage, 4 * ranks * np, hipMemcpyHostToDevice));
    MT_TRY(ptk::launch_matte_extract(ptk::matte_extract_grid(cus, (uint32_t)np), nullptr, (uint32_t)np, ranks, d_keys.as<uint32_t>(), d_coverage.as<float>(), set_count,
                                     d_selection.as<uint32_t>(), d_selection.as<uint32_t>() + MATTE_SETS_MAX + 1u, d_out.as<float>()));
    MT_TRY(hipDeviceSynchronize());
    MT_TRY(hipMemcpy(out, d_out.p, 4 * set_count * np, hipMemcpyDeviceToHost));
#undef MT_TRY
    return PT_OK;
}
