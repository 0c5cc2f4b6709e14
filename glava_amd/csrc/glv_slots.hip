// glv_slots.hip -- the lifecycle of chosen streams of a batch (glv_batch_reset_streams / _save_streams / _load_streams): one kernel that zeroes the state of
// listed streams, gathers it into blobs in the portable form, or scatters blobs back.
//
// The portable form of a stream (include/glv_spectrum.h) is its bytes in the batch's state arrays with the host-kept positions rotated out: the regions
// of SlotTable in order, each the stream's part of one array, each cut into `chan_bytes` blocks of `mod` units of 2^log_unit bytes -- portable unit u of a
// block is array unit (u + pos) mod `mod` of the same block.  The gravity rows: one unit per row, no rotation.  The average ring: a block per channel
// row, a unit per ring slot (a row of n elements), pos = head.  A PCM ring: one block, a unit per frame (4 or 8 bytes), pos = the ring's write position.
//
//   glv_slots_kernel<KIND>   work item [listed stream j][16-byte piece p of the stream's bytes in portable order]
//
// A workgroup takes 256 consecutive pieces of ONE listed stream per trip, so d_idx[j] is one uniform load per trip and both sides of the copy are 4 KiB
// runs (a run breaks only where the rotation wraps).  Units of 16 bytes or more rotate whole pieces.  Frames are smaller: the piece's place in the ring
// may begin off 16 bytes or straddle the wrap, so -- the rule of glv_wave_kernel / glv_decimate_kernel -- the ring side is one 16-byte access where its
// first byte is 16-byte aligned (the ring's bytes are a multiple of 16: an aligned piece never wraps) and naturally aligned frames else, each wrapped on
// its own; the blob side is always one 16-byte access.  Plain vector loads and stores, no LDS, no atomics.
// Bounds: an entry of d_idx >= streams is skipped where it is read, with its blob; p < pieces; the host's pos < mod, so a rotated unit stays in its block.
#include <hip/hip_runtime.h>

#include "glv_launch.h"
#include "glv_launch_util.h"

namespace glv {

typedef uint32_t glv_su4 __attribute__((ext_vector_type(4)));
typedef uint32_t glv_su2 __attribute__((ext_vector_type(2)));

template <int KIND>
__global__ void __launch_bounds__(256) glv_slots_kernel(const SlotTable t, const uint32_t chunks, const uint32_t step_j, const uint32_t step_c, const uint64_t items) {
    const uint32_t pieces = t.bytes >> 4;
    // item = j * chunks + c, advanced by gridDim.x = step_j * chunks + step_c per trip without a division
    uint32_t j = blockIdx.x / chunks, c = blockIdx.x - j * chunks;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t s = t.idx[j];                                             // uniform: one listed stream per workgroup and trip
        const uint32_t p = c * 256u + threadIdx.x;
        if (s < t.streams && p < pieces) {
            const uint32_t o = p << 4;                                           // the piece's first byte in the stream's portable form
            // the region that holds it (regions lie back to back: the last whose start is <= o), by selects over the by-value table
            SlotRegion r = t.r[0];
#pragma unroll
            for (int q = 1; q < kSlotRegions; ++q)
                if ((uint32_t) q < t.nregions && o >= t.r[q].start) r = t.r[q];
            uint32_t in = o - r.start;                                           // ... and within the region: block, unit, byte of the unit
            const uint32_t block = in >= r.chan_bytes ? r.chan_bytes : 0u;       // (at most two blocks: the channel rows)
            in -= block;
            const uint32_t unit = in >> r.log_unit, within = in & ((1u << r.log_unit) - 1u);
            char* const arr = r.base + (uint64_t) s * r.stream_bytes + block;    // 64-bit: the ring of a large batch passes 2^32 bytes
            glv_su4* const blob = reinterpret_cast<glv_su4*>(static_cast<char*>(t.blob) + (uint64_t) j * t.bytes + o);
            uint32_t u = unit + r.pos;
            if (u >= r.mod) u -= r.mod;
            const uint32_t at = (u << r.log_unit) + within;                      // byte of the block
            if (r.log_unit >= 4u || (at & 15u) == 0u) {
                glv_su4* const a = reinterpret_cast<glv_su4*>(arr + at);
                if constexpr (KIND == SLOT_ZERO) *a = glv_su4{0u, 0u, 0u, 0u};
                else if constexpr (KIND == SLOT_GATHER) *blob = *a;
                else *a = *blob;
            } else if (r.log_unit == 3u) {                                       // two float frames, each where the rotation puts it
                uint32_t u1 = u + 1u;
                if (u1 >= r.mod) u1 -= r.mod;
                glv_su2* const a0 = reinterpret_cast<glv_su2*>(arr + ((size_t) u << 3));
                glv_su2* const a1 = reinterpret_cast<glv_su2*>(arr + ((size_t) u1 << 3));
                if constexpr (KIND == SLOT_ZERO) { *a0 = glv_su2{0u, 0u}; *a1 = glv_su2{0u, 0u}; }
                else if constexpr (KIND == SLOT_GATHER) { const glv_su2 x = *a0, y = *a1; *blob = glv_su4{x.x, x.y, y.x, y.y}; }
                else { const glv_su4 v = *blob; *a0 = glv_su2{v.x, v.y}; *a1 = glv_su2{v.z, v.w}; }
            } else {                                                             // four s16 frames
                uint32_t* a[4];
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    uint32_t uq = u + (uint32_t) q;
                    if (uq >= r.mod) uq -= r.mod;
                    a[q] = reinterpret_cast<uint32_t*>(arr + ((size_t) uq << 2));
                }
                if constexpr (KIND == SLOT_ZERO) { *a[0] = 0u; *a[1] = 0u; *a[2] = 0u; *a[3] = 0u; }
                else if constexpr (KIND == SLOT_GATHER) *blob = glv_su4{*a[0], *a[1], *a[2], *a[3]};
                else { const glv_su4 v = *blob; *a[0] = v.x; *a[1] = v.y; *a[2] = v.z; *a[3] = v.w; }
            }
        }
        j += step_j; c += step_c;
        if (c >= chunks) { c -= chunks; ++j; }
    }
}

// Vets the table as far as the host can (every count the kernel's bounds rest on) and launches one grid: a workgroup per 256 pieces of a listed stream up
// to the cap, the kernel's loop takes what lies beyond.  SLOT_ZERO needs no blob.
hipError_t launch_slots(int kind, const SlotTable& t, hipStream_t st) {
    if (!t.idx || t.count == 0 || t.streams == 0 || t.nregions == 0 || t.nregions > (uint32_t) kSlotRegions || t.bytes == 0 || (t.bytes & 15u)) return hipErrorInvalidValue;
    if (kind != SLOT_ZERO && (!t.blob || (reinterpret_cast<uintptr_t>(t.blob) & 15u))) return hipErrorInvalidValue;
    uint32_t start = 0;
    for (uint32_t q = 0; q < t.nregions; ++q) {
        const SlotRegion& r = t.r[q];
        const uint64_t unit = (uint64_t) 1 << r.log_unit;
        if (!r.base || (reinterpret_cast<uintptr_t>(r.base) & 15u) || r.start != start || r.log_unit < 2u || r.log_unit > 24u || r.mod == 0 || r.pos >= r.mod) return hipErrorInvalidValue;
        if ((uint64_t) r.chan_bytes != unit * r.mod || (r.chan_bytes & 15u) || (r.stream_bytes != r.chan_bytes && r.stream_bytes != 2u * r.chan_bytes)) return hipErrorInvalidValue;
        if (r.log_unit < 4u && (r.mod & ((16u >> r.log_unit) - 1u))) return hipErrorInvalidValue;       // whole pieces per ring: an aligned piece never wraps
        start += r.stream_bytes;
    }
    if (start != t.bytes) return hipErrorInvalidValue;
    const uint32_t chunks = ((t.bytes >> 4) + 255u) / 256u;
    const uint64_t items = (uint64_t) t.count * chunks;
    const unsigned grid = capped_grid((size_t) items, 1, kSlotsGridCap);
    const uint32_t step_j = grid / chunks, step_c = grid % chunks;
    if (kind == SLOT_ZERO) hipLaunchKernelGGL((glv_slots_kernel<SLOT_ZERO>), dim3(grid), dim3(256), 0, st, t, chunks, step_j, step_c, items);
    else if (kind == SLOT_GATHER) hipLaunchKernelGGL((glv_slots_kernel<SLOT_GATHER>), dim3(grid), dim3(256), 0, st, t, chunks, step_j, step_c, items);
    else if (kind == SLOT_SCATTER) hipLaunchKernelGGL((glv_slots_kernel<SLOT_SCATTER>), dim3(grid), dim3(256), 0, st, t, chunks, step_j, step_c, items);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace glv
