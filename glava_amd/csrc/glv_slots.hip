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
//
//   glv_slot_copy_kernel     work item [pair j][16-byte piece p], as above (glv_batch_copy_streams): the piece of stream src_idx[j] of one batch straight into
//                            stream dst_idx[j] of another (or of the same one), no blob between
//
// Two region tables, the same regions in the same order (the launcher holds them to that), each with its own bases and positions: portable piece p is read
// where the source's positions put it and written where the destination's do, each side by the ring rule above on its own -- so a PCM ring has four forms
// (one access or single frames on either side), and units of 16 bytes or more are whole pieces on both.  A pair with either entry >= its batch's streams is
// skipped where it is read.  With both tables of ONE batch a pair (i, i) rewrites what it read; a stream that is source and destination of different
// pairs is the caller's error (the contents of the named destinations are then unspecified, nothing else is touched).
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

// where portable piece `in` (bytes into the region, block taken off) of a region lies in its block: the rotated unit and the byte
struct SlotPlace { uint32_t u, at; };
__device__ __forceinline__ SlotPlace slot_place(const SlotRegion& r, uint32_t in) {
    uint32_t u = (in >> r.log_unit) + r.pos;
    if (u >= r.mod) u -= r.mod;
    return SlotPlace{u, (u << r.log_unit) + (in & ((1u << r.log_unit) - 1u))};
}
// frame u + q of a ring of r.mod frames, wrapped on its own
__device__ __forceinline__ uint32_t slot_frame(const SlotRegion& r, uint32_t u, uint32_t q) {
    uint32_t uq = u + q;
    if (uq >= r.mod) uq -= r.mod;
    return uq;
}

__global__ void __launch_bounds__(256) glv_slot_copy_kernel(const SlotTable src, const SlotTable dst, const uint32_t chunks, const uint32_t step_j, const uint32_t step_c,
                                                            const uint64_t items) {
    const uint32_t pieces = dst.bytes >> 4;
    uint32_t j = blockIdx.x / chunks, c = blockIdx.x - j * chunks;              // item = j * chunks + c, as in glv_slots_kernel
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t ss = src.idx[j], sd = dst.idx[j];                         // uniform: one pair per workgroup and trip
        const uint32_t p = c * 256u + threadIdx.x;
        if (ss < src.streams && sd < dst.streams && p < pieces) {
            const uint32_t o = p << 4;
            SlotRegion rs = src.r[0], rd = dst.r[0];                             // the region of both tables that holds the piece (the same index: same starts)
#pragma unroll
            for (int q = 1; q < kSlotRegions; ++q)
                if ((uint32_t) q < dst.nregions && o >= dst.r[q].start) { rs = src.r[q]; rd = dst.r[q]; }
            uint32_t in = o - rd.start;
            const uint32_t block = in >= rd.chan_bytes ? rd.chan_bytes : 0u;
            in -= block;
            const char* const from = rs.base + (uint64_t) ss * rs.stream_bytes + block;      // 64-bit, as in glv_slots_kernel
            char* const to = rd.base + (uint64_t) sd * rd.stream_bytes + block;
            const SlotPlace a = slot_place(rs, in), b = slot_place(rd, in);
            glv_su4 v;
            if (rs.log_unit >= 4u || (a.at & 15u) == 0u) v = *reinterpret_cast<const glv_su4*>(from + a.at);
            else if (rs.log_unit == 3u) {
                const glv_su2 x = *reinterpret_cast<const glv_su2*>(from + ((size_t) a.u << 3));
                const glv_su2 y = *reinterpret_cast<const glv_su2*>(from + ((size_t) slot_frame(rs, a.u, 1u) << 3));
                v = glv_su4{x.x, x.y, y.x, y.y};
            } else {
                v.x = *reinterpret_cast<const uint32_t*>(from + ((size_t) a.u << 2));
                v.y = *reinterpret_cast<const uint32_t*>(from + ((size_t) slot_frame(rs, a.u, 1u) << 2));
                v.z = *reinterpret_cast<const uint32_t*>(from + ((size_t) slot_frame(rs, a.u, 2u) << 2));
                v.w = *reinterpret_cast<const uint32_t*>(from + ((size_t) slot_frame(rs, a.u, 3u) << 2));
            }
            if (rd.log_unit >= 4u || (b.at & 15u) == 0u) *reinterpret_cast<glv_su4*>(to + b.at) = v;
            else if (rd.log_unit == 3u) {
                *reinterpret_cast<glv_su2*>(to + ((size_t) b.u << 3)) = glv_su2{v.x, v.y};
                *reinterpret_cast<glv_su2*>(to + ((size_t) slot_frame(rd, b.u, 1u) << 3)) = glv_su2{v.z, v.w};
            } else {
                *reinterpret_cast<uint32_t*>(to + ((size_t) b.u << 2)) = v.x;
                *reinterpret_cast<uint32_t*>(to + ((size_t) slot_frame(rd, b.u, 1u) << 2)) = v.y;
                *reinterpret_cast<uint32_t*>(to + ((size_t) slot_frame(rd, b.u, 2u) << 2)) = v.z;
                *reinterpret_cast<uint32_t*>(to + ((size_t) slot_frame(rd, b.u, 3u) << 2)) = v.w;
            }
        }
        j += step_j; c += step_c;
        if (c >= chunks) { c -= chunks; ++j; }
    }
}

// every count of a table that the kernels' bounds rest on
static bool slot_table_ok(const SlotTable& t) {
    if (!t.idx || t.count == 0 || t.streams == 0 || t.nregions == 0 || t.nregions > (uint32_t) kSlotRegions || t.bytes == 0 || (t.bytes & 15u)) return false;
    uint32_t start = 0;
    for (uint32_t q = 0; q < t.nregions; ++q) {
        const SlotRegion& r = t.r[q];
        const uint64_t unit = (uint64_t) 1 << r.log_unit;
        if (!r.base || (reinterpret_cast<uintptr_t>(r.base) & 15u) || r.start != start || r.log_unit < 2u || r.log_unit > 24u || r.mod == 0 || r.pos >= r.mod) return false;
        if ((uint64_t) r.chan_bytes != unit * r.mod || (r.chan_bytes & 15u) || (r.stream_bytes != r.chan_bytes && r.stream_bytes != 2u * r.chan_bytes)) return false;
        if (r.log_unit < 4u && (r.mod & ((16u >> r.log_unit) - 1u))) return false;       // whole pieces per ring: an aligned piece never wraps
        start += r.stream_bytes;
    }
    return start == t.bytes;
}

// Vets the table as far as the host can (every count the kernel's bounds rest on) and launches one grid: a workgroup per 256 pieces of a listed stream up
// to the cap, the kernel's loop takes what lies beyond.  SLOT_ZERO needs no blob.
hipError_t launch_slots(int kind, const SlotTable& t, hipStream_t st) {
    if (!slot_table_ok(t)) return hipErrorInvalidValue;
    if (kind != SLOT_ZERO && (!t.blob || (reinterpret_cast<uintptr_t>(t.blob) & 15u))) return hipErrorInvalidValue;
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

// ... and the copy from slot to slot: both tables vetted as above and held to the same regions (start, sizes, unit and ring length; bases and positions are each
// side's own), the same count; then glv_slots_kernel's grid.
hipError_t launch_slot_copy(const SlotTable& src, const SlotTable& dst, hipStream_t st) {
    if (!slot_table_ok(src) || !slot_table_ok(dst) || src.nregions != dst.nregions || src.bytes != dst.bytes || src.count != dst.count) return hipErrorInvalidValue;
    for (uint32_t q = 0; q < dst.nregions; ++q) {
        const SlotRegion &a = src.r[q], &b = dst.r[q];
        if (a.start != b.start || a.stream_bytes != b.stream_bytes || a.chan_bytes != b.chan_bytes || a.log_unit != b.log_unit || a.mod != b.mod) return hipErrorInvalidValue;
    }
    const uint32_t chunks = ((dst.bytes >> 4) + 255u) / 256u;
    const uint64_t items = (uint64_t) dst.count * chunks;
    const unsigned grid = capped_grid((size_t) items, 1, kSlotsGridCap);
    hipLaunchKernelGGL(glv_slot_copy_kernel, dim3(grid), dim3(256), 0, st, src, dst, chunks, grid / chunks, grid % chunks, items);
    return hipGetLastError();
}

}  // namespace glv
