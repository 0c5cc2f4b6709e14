// glv_ring_each.hip -- the two copies of a per-stream ring track call (glv_batch_ring_track_each_s16 / _f32): stream s of a ring batch takes c_s of the
// call's `updates` ring updates, c_s = min(counts[s], updates) read on the device (counts null: everybody takes all of them).
//
//   glv_ring_stage_each_kernel<LOG_FB>   work item [stream s][16-byte piece p of the stream's staged recording]
//   glv_ring_keep_each_kernel<LOG_FB>    work item [stream s][16-byte piece p of the stream's ring]
//
// The layout is glv_ring_track.hip's: frames of 2^LOG_FB bytes (4: interleaved s16, 8: interleaved f32), a piece is 4 or 2 of them; the staged recording of
// stream s is `pitch` frames (a multiple of 4, so every stream starts on 16 bytes): its ring read oldest frame first -- frame f < n is ring frame (f + pos)
// mod n -- followed by its FIRST c_s * new_frames new frames and zeros up to the pitch.  The new frames lie [streams][updates * new_frames] whatever the
// counts are; those of a stream at and beyond c_s * new_frames are never read.  The stage kernel also writes the per-stream call's table of window starts,
// starts[s][t] = (t + 1) * new_frames for every t < updates: the windows behind a count lie inside the staged region (they read the stream's last frames
// and zeros), and the scan discards what the transform makes of them.  The keep kernel writes frames [c_s * new_frames, c_s * new_frames + n) of the staged
// recording -- the last n of the stream's OWN n + c_s * new_frames frames -- back as the ring, oldest frame at 0: the host sets the batch's one ring position to
// 0, which is then right for every stream, and a stream with c_s = 0 keeps its ring (read oldest first) bit for bit.
//
// A workgroup takes 256 consecutive pieces of ONE stream per trip (glv_ring_stage_kernel's scheme, with its division-free advance), so the stream and its
// count are uniform for the workgroup: one scalar load per trip.  The stage side and the ring as the keep kernel writes it are always one 16-byte access.
// The other side follows the ring rule: one 16-byte access where the piece's first byte is 16-byte aligned and the piece lies wholly inside (n is a multiple
// of 4 frames, so an aligned piece of the ring never wraps; a piece of the new frames must end at or before c_s * new_frames), naturally aligned frames else,
// each wrapped or bounded on its own.  The keep kernel's source offset differs per stream, so its alignment does too.  Plain vector loads and stores, no LDS,
// no atomics.  Bounds: p < pieces of the stream; a ring frame index is < n; a new frame index is < c_s * new_frames <= updates * new_frames; a staged frame
// index is < c_s * new_frames + n <= pitch; a table index is < streams * updates.  Offsets are 64-bit.
#include <hip/hip_runtime.h>

#include "glv_launch.h"
#include "glv_launch_util.h"

namespace glv {

typedef uint32_t glv_eu4 __attribute__((ext_vector_type(4)));
typedef uint32_t glv_eu2 __attribute__((ext_vector_type(2)));

// frame i of the frames at `base` as frame q of the piece v
template <int LOG_FB>
__device__ __forceinline__ void ring_each_frame(const char* base, uint64_t i, glv_eu4& v, int q) {
    if constexpr (LOG_FB == 2) {
        const uint32_t x = *reinterpret_cast<const uint32_t*>(base + (i << 2));
        if (q == 0) v.x = x; else if (q == 1) v.y = x; else if (q == 2) v.z = x; else v.w = x;
    } else {
        const glv_eu2 x = *reinterpret_cast<const glv_eu2*>(base + (i << 3));
        if (q == 0) { v.x = x.x; v.y = x.y; } else { v.z = x.x; v.w = x.y; }
    }
}

// the updates stream j takes: its count clamped to the call's (j is uniform for the workgroup: a scalar load)
__device__ __forceinline__ uint32_t ring_each_count(const RingTrackEach& e, uint32_t j) {
    const uint32_t c = e.counts ? e.counts[j] : e.r.updates;
    return c < e.r.updates ? c : e.r.updates;
}

template <int LOG_FB>
__global__ void __launch_bounds__(256) glv_ring_stage_each_kernel(const RingTrackEach e, const uint32_t chunks, const uint32_t step_j, const uint32_t step_c, const uint64_t items) {
    constexpr uint32_t FPP = 16u >> LOG_FB;                                      // frames per piece
    const RingTrack& r = e.r;
    const uint32_t pieces = r.pitch / FPP, added = r.updates * r.new_frames;     // (the launcher: added <= pitch - n, so it fits 32 bits)
    const uint32_t entries = r.streams * r.updates;                              // (the launcher: fits 32 bits)
    for (uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x; t < entries; t += (uint64_t) gridDim.x * 256u)
        r.starts[t] = ((uint32_t) t % r.updates + 1u) * r.new_frames;            // <= added <= pitch - n, behind a count too
    // item = j * chunks + c, advanced by gridDim.x = step_j * chunks + step_c per trip without a division
    uint32_t j = blockIdx.x / chunks, c = blockIdx.x - j * chunks;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t p = c * 256u + threadIdx.x;
        if (j < r.streams) {
            const uint32_t own = ring_each_count(e, j) * r.new_frames;           // the stream's own new frames: <= added
            if (p < pieces) {
                const uint32_t f = p * FPP;                                      // the piece's first frame of the staged recording: f + FPP <= pitch
                glv_eu4 v = glv_eu4{0u, 0u, 0u, 0u};
                if (f < r.n) {                                                   // n is a multiple of FPP: the whole piece is ring
                    const char* const ring = static_cast<const char*>(r.ring) + (((uint64_t) j * r.n) << LOG_FB);
                    uint32_t u = f + r.pos;
                    if (u >= r.n) u -= r.n;
                    if ((u & (FPP - 1u)) == 0u) v = *reinterpret_cast<const glv_eu4*>(ring + ((uint64_t) u << LOG_FB));
                    else {
#pragma unroll
                        for (int q = 0; q < (int) FPP; ++q) {
                            uint32_t uq = u + (uint32_t) q;
                            if (uq >= r.n) uq -= r.n;
                            ring_each_frame<LOG_FB>(ring, uq, v, q);
                        }
                    }
                } else if (r.fresh && f - r.n < own) {
                    const uint32_t i = f - r.n;                                  // the piece's first new frame; those at and beyond `own` are zeros and are not read
                    const char* const src = static_cast<const char*>(r.fresh) + (((uint64_t) j * added) << LOG_FB);
                    const char* const at = src + ((uint64_t) i << LOG_FB);
                    if (i + FPP <= own && (reinterpret_cast<uintptr_t>(at) & 15u) == 0u) v = *reinterpret_cast<const glv_eu4*>(at);
                    else {
#pragma unroll
                        for (int q = 0; q < (int) FPP; ++q)
                            if (i + (uint32_t) q < own) ring_each_frame<LOG_FB>(src, (uint64_t) i + (uint32_t) q, v, q);
                    }
                }
                *reinterpret_cast<glv_eu4*>(static_cast<char*>(r.stage) + ((((uint64_t) j * r.pitch) + f) << LOG_FB)) = v;
            }
        }
        j += step_j; c += step_c;
        if (c >= chunks) { c -= chunks; ++j; }
    }
}

template <int LOG_FB>
__global__ void __launch_bounds__(256) glv_ring_keep_each_kernel(const RingTrackEach e, const uint32_t chunks, const uint32_t step_j, const uint32_t step_c, const uint64_t items) {
    constexpr uint32_t FPP = 16u >> LOG_FB;
    const RingTrack& r = e.r;
    const uint32_t pieces = r.n / FPP;
    uint32_t j = blockIdx.x / chunks, c = blockIdx.x - j * chunks;               // item = j * chunks + c, as in glv_ring_stage_each_kernel
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t p = c * 256u + threadIdx.x;
        if (j < r.streams) {
            const uint32_t own = ring_each_count(e, j) * r.new_frames;           // <= updates * new_frames <= pitch - n
            if (p < pieces) {
                const uint32_t f = p * FPP;                                      // ring frame f <- staged frame own + f; own + f + FPP <= own + n <= pitch
                const char* const src = static_cast<const char*>(r.stage) + (((uint64_t) j * r.pitch) << LOG_FB);
                const char* const at = src + (((uint64_t) own + f) << LOG_FB);
                glv_eu4 v = glv_eu4{0u, 0u, 0u, 0u};
                if ((reinterpret_cast<uintptr_t>(at) & 15u) == 0u) v = *reinterpret_cast<const glv_eu4*>(at);
                else {
#pragma unroll
                    for (int q = 0; q < (int) FPP; ++q) ring_each_frame<LOG_FB>(src, (uint64_t) own + f + (uint32_t) q, v, q);
                }
                *reinterpret_cast<glv_eu4*>(static_cast<char*>(r.ring) + ((((uint64_t) j * r.n) + f) << LOG_FB)) = v;
            }
        }
        j += step_j; c += step_c;
        if (c >= chunks) { c -= chunks; ++j; }
    }
}

// every count the kernels' bounds rest on (the counts themselves are device memory: the kernels clamp them)
static bool ring_each_ok(bool f32, const RingTrackEach& e) {
    const RingTrack& r = e.r;
    if (!r.ring || !r.stage || !r.starts || r.streams == 0 || r.updates == 0 || r.new_frames == 0 || r.new_frames > r.n) return false;
    if (r.n < 4u || (r.n & 3u) || r.pos >= r.n || (r.pitch & 3u)) return false;
    if ((uint64_t) r.updates * r.new_frames + r.n > (uint64_t) r.pitch) return false;                  // (so updates * new_frames fits 32 bits)
    if ((uint64_t) r.streams * r.updates > 0xffffffffull) return false;                                // the table's entries
    if ((reinterpret_cast<uintptr_t>(r.ring) | reinterpret_cast<uintptr_t>(r.stage)) & 15u) return false;
    if ((reinterpret_cast<uintptr_t>(r.starts) | reinterpret_cast<uintptr_t>(e.counts)) & 3u) return false;
    if (reinterpret_cast<uintptr_t>(r.fresh) & (f32 ? 7u : 3u)) return false;
    return true;
}

// One grid each: a workgroup per 256 pieces of a stream up to the cap, the kernel's loop takes what lies beyond.
hipError_t launch_ring_each_stage(bool f32, const RingTrackEach& e, hipStream_t st) {
    if (!ring_each_ok(f32, e)) return hipErrorInvalidValue;
    const uint32_t pieces = e.r.pitch / (f32 ? 2u : 4u), chunks = (pieces + 255u) / 256u;
    const uint64_t items = (uint64_t) e.r.streams * chunks;
    const unsigned grid = capped_grid((size_t) items, 1, kRingTrackGridCap);
    if (f32) hipLaunchKernelGGL((glv_ring_stage_each_kernel<3>), dim3(grid), dim3(256), 0, st, e, chunks, grid / chunks, grid % chunks, items);
    else hipLaunchKernelGGL((glv_ring_stage_each_kernel<2>), dim3(grid), dim3(256), 0, st, e, chunks, grid / chunks, grid % chunks, items);
    return hipGetLastError();
}

hipError_t launch_ring_each_keep(bool f32, const RingTrackEach& e, hipStream_t st) {
    if (!ring_each_ok(f32, e)) return hipErrorInvalidValue;
    const uint32_t pieces = e.r.n / (f32 ? 2u : 4u), chunks = (pieces + 255u) / 256u;
    const uint64_t items = (uint64_t) e.r.streams * chunks;
    const unsigned grid = capped_grid((size_t) items, 1, kRingTrackGridCap);
    if (f32) hipLaunchKernelGGL((glv_ring_keep_each_kernel<3>), dim3(grid), dim3(256), 0, st, e, chunks, grid / chunks, grid % chunks, items);
    else hipLaunchKernelGGL((glv_ring_keep_each_kernel<2>), dim3(grid), dim3(256), 0, st, e, chunks, grid / chunks, grid % chunks, items);
    return hipGetLastError();
}

}  // namespace glv
