// glv_launch_util.h -- the host logic every launcher of glv_misc.hip and glv_bars.hip shares: how many workgroups, how a table's rounds are split
// over blockIdx.y, the dynamic-LDS opt-in, and a rows kernel's dispatch over the LDS rings it is built for.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>

#include "glv_launch.h"

namespace glv {

// Workgroups of a grid-stride kernel: one per `per_wg` items up to `cap`, the kernel's loop takes what lies beyond.  No items give 0: a caller that
// launches all the same asks for at least 1 itself.
constexpr size_t kGridCap = 256 * 8;       // 256 CUs x 8 resident 256-thread blocks
inline unsigned capped_grid(size_t items, size_t per_wg, size_t cap) {
    const size_t g = (items + per_wg - 1) / per_wg;
    return (unsigned) (g < cap ? g : cap);
}

// The > 64 KiB dynamic-LDS opt-in of KERNEL, set at most once per device: by the first launch that needs it, or ahead of it by a prepare_* call (the
// launchers' nrows == 0 form), so that a process call is a plain launch.
template <auto KERNEL>
inline hipError_t lds_opt_in(size_t bytes) {
    static std::atomic<bool> done[64] = {};
    if (bytes <= 64 * 1024) return hipSuccess;
    int dev = 0;
    (void) hipGetDevice(&dev);
    if (dev >= 0 && dev < 64 && done[dev].load(std::memory_order_acquire)) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int) bytes);
    if (e != hipSuccess) return e;
    if (dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
    return hipSuccess;
}

// The rows kernels: xb workgroups of rows in x, ranges of a table's rounds in y -- 512 workgroups = two per CU, once (a range start refills the whole
// ring; glv_bars_rows_kernel at N = 4096, ms with 1 / 2 / 4 / 8 / 16 ranges: 32 K rows 0.321 / 0.328 / 0.337 / 0.351 / 0.370, 8 K rows 0.213 / 0.137 /
// 0.093 / 0.099 / 0.102, 2 K rows 0.206 / 0.131 / 0.072 / 0.048 / 0.045)
struct RoundSplit { uint32_t yb, rounds_per_wg; };
inline RoundSplit split_rounds(uint32_t xb, uint32_t nrounds) {
    uint32_t yb = xb >= 512 ? 1 : (512 + xb - 1) / xb;
#if defined(GLV_TUNE_BUILD)
    if (const char* o = std::getenv("GLV_ROWS_YB")) yb = (uint32_t) atoi(o);       // tools/rows_bench: the split of the rounds over blockIdx.y
#endif
    if (yb > nrounds) yb = nrounds;
    const uint32_t rpw = (nrounds + yb - 1) / yb;
    return {(nrounds + rpw - 1) / rpw, rpw};
}

// A rows kernel's ring dispatcher (glv_bars.hip with_rows_ring, with_rows_i8_ring) hands its caller a ring the kernel is built for and the rows of a
// workgroup as compile-time constants, and answers `none` for any other ring
template <int S, int RB> struct RingRows { static constexpr int bins = S, rows = RB; };

}  // namespace glv
