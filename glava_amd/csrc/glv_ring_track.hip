// glv_ring_track.hip -- the two copies of a ring track call (glv_batch_ring_track_s16 / _f32): several updates of a ring batch in one call.
//
//   glv_ring_stage_kernel<LOG_FB>   work item [stream s][16-byte piece p of the stream's staged recording]
//   glv_ring_keep_kernel<LOG_FB>    work item [stream s][16-byte piece p of the stream's ring]
//
// Frames are 2^LOG_FB bytes: 4 (interleaved s16) or 8 (interleaved f32); a piece is 4 or 2 of them.  The staged recording of stream s (RingTrack::stage,
// `pitch` frames, a multiple of 4, so every stream starts on 16 bytes) is its ring read oldest frame first -- frame f < n is ring frame (f + pos) mod n --
// followed by its updates * new_frames new frames (zeros where RingTrack::fresh is null: the s16 entry's zero fill) and up to 3 frames of zeros
// that no window reads.  The track executor then runs on it as on any recording.  The stage kernel also writes the table of window starts, (t + 1) *
// new_frames for update t, so that the call allocates nothing.  The keep kernel writes the last n of those n + updates * new_frames frames back as the ring, oldest frame
// at frame 0: the host sets the ring's position to 0.
//
// A workgroup takes 256 consecutive pieces of ONE stream per trip (glv_slots_kernel's scheme: both sides are 4 KiB runs, no division in the loop).  The
// stage side and the ring as the keep kernel writes it are always one 16-byte access.  The other side follows the ring rule of glv_slots.hip: one 16-byte
// access where the piece's first byte is 16-byte aligned (n is a multiple of 4 frames, so an aligned piece of the ring never wraps; a piece of the new frames
// must also lie wholly within them), naturally aligned frames else, each wrapped or bounded on its own.  Plain vector loads and stores, no LDS, no atomics.
// Bounds: p < pieces of the stream; a ring frame index is < n; a new frame index is < updates * new_frames; a staged frame index is < pitch.  Offsets are 64-bit.
#include <hip/hip_runtime.h>

#include "glv_launch.h"
#include "glv_launch_util.h"

namespace glv {

typedef uint32_t glv_ru4 __attribute__((ext_vector_type(4)));
typedef uint32_t glv_ru2 __attribute__((ext_vector_type(2)));

// frame i of the frames at `base` (null: zeros) as frame q of the piece v
template <int LOG_FB>
__device__ __forceinline__ void ring_track_frame(const char* base, uint64_t i, glv_ru4& v, int q) {
    if constexpr (LOG_FB == 2) {
        const uint32_t x = base ? *reinterpret_cast<const uint32_t*>(base + (i << 2)) : 0u;
        if (q == 0) v.x = x; else if (q == 1) v.y = x; else if (q == 2) v.z = x; else v.w = x;
    } else {
        const glv_ru2 x = base ? *reinterpret_cast<const glv_ru2*>(base + (i << 3)) : glv_ru2{0u, 0u};
        if (q == 0) { v.x = x.x; v.y = x.y; } else { v.z = x.x; v.w = x.y; }
    }
}

template <int LOG_FB>
__global__ void __launch_bounds__(256) glv_ring_stage_kernel(const RingTrack r, const uint32_t chunks, const uint32_t step_j, const uint32_t step_c, const uint64_t items) {
    constexpr uint32_t FPP = 16u >> LOG_FB;                                      // frames per piece
    const uint32_t pieces = r.pitch / FPP, added = r.updates * r.new_frames;     // (the launcher: added <= pitch - n, so it fits 32 bits)
    for (uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x; t < r.updates; t += (uint64_t) gridDim.x * 256u)
        r.starts[t] = ((uint32_t) t + 1u) * r.new_frames;                        // <= added
    // item = j * chunks + c, advanced by gridDim.x = step_j * chunks + step_c per trip without a division
    uint32_t j = blockIdx.x / chunks, c = blockIdx.x - j * chunks;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t p = c * 256u + threadIdx.x;
        if (j < r.streams && p < pieces) {
            const uint32_t f = p * FPP;                                          // the piece's first frame of the staged recording: f + FPP <= pitch
            glv_ru4 v = glv_ru4{0u, 0u, 0u, 0u};
            if (f < r.n) {                                                       // n is a multiple of FPP: the whole piece is ring
                const char* const ring = static_cast<const char*>(r.ring) + (((uint64_t) j * r.n) << LOG_FB);
                uint32_t u = f + r.pos;
                if (u >= r.n) u -= r.n;
                if ((u & (FPP - 1u)) == 0u) v = *reinterpret_cast<const glv_ru4*>(ring + ((uint64_t) u << LOG_FB));
                else {
#pragma unroll
                    for (int q = 0; q < (int) FPP; ++q) {
                        uint32_t uq = u + (uint32_t) q;
                        if (uq >= r.n) uq -= r.n;
                        ring_track_frame<LOG_FB>(ring, uq, v, q);
                    }
                }
            } else if (r.fresh) {
                const uint32_t i = f - r.n;                                      // the piece's first new frame; those at and beyond `added` are the pad: zeros
                const char* const src = static_cast<const char*>(r.fresh) + (((uint64_t) j * added) << LOG_FB);
                const char* const at = src + ((uint64_t) i << LOG_FB);
                if (i + FPP <= added && (reinterpret_cast<uintptr_t>(at) & 15u) == 0u) v = *reinterpret_cast<const glv_ru4*>(at);
                else {
#pragma unroll
                    for (int q = 0; q < (int) FPP; ++q)
                        if (i + (uint32_t) q < added) ring_track_frame<LOG_FB>(src, (uint64_t) i + (uint32_t) q, v, q);
                }
            }
            *reinterpret_cast<glv_ru4*>(static_cast<char*>(r.stage) + ((((uint64_t) j * r.pitch) + f) << LOG_FB)) = v;
        }
        j += step_j; c += step_c;
        if (c >= chunks) { c -= chunks; ++j; }
    }
}

template <int LOG_FB>
__global__ void __launch_bounds__(256) glv_ring_keep_kernel(const RingTrack r, const uint32_t chunks, const uint32_t step_j, const uint32_t step_c, const uint64_t items) {
    constexpr uint32_t FPP = 16u >> LOG_FB;
    const uint32_t pieces = r.n / FPP, added = r.updates * r.new_frames;
    uint32_t j = blockIdx.x / chunks, c = blockIdx.x - j * chunks;               // item = j * chunks + c, as in glv_ring_stage_kernel
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t p = c * 256u + threadIdx.x;
        if (j < r.streams && p < pieces) {
            const uint32_t f = p * FPP;                                          // ring frame f <- staged frame added + f; added + f + FPP <= added + n <= pitch
            const char* const src = static_cast<const char*>(r.stage) + (((uint64_t) j * r.pitch) << LOG_FB);
            const char* const at = src + (((uint64_t) added + f) << LOG_FB);
            glv_ru4 v = glv_ru4{0u, 0u, 0u, 0u};
            if ((reinterpret_cast<uintptr_t>(at) & 15u) == 0u) v = *reinterpret_cast<const glv_ru4*>(at);
            else {
#pragma unroll
                for (int q = 0; q < (int) FPP; ++q) ring_track_frame<LOG_FB>(src, (uint64_t) added + f + (uint32_t) q, v, q);
            }
            *reinterpret_cast<glv_ru4*>(static_cast<char*>(r.ring) + ((((uint64_t) j * r.n) + f) << LOG_FB)) = v;
        }
        j += step_j; c += step_c;
        if (c >= chunks) { c -= chunks; ++j; }
    }
}

// every count the kernels' bounds rest on
static bool ring_track_ok(bool f32, const RingTrack& r) {
    if (!r.ring || !r.stage || !r.starts || r.streams == 0 || r.updates == 0 || r.new_frames == 0 || r.new_frames > r.n) return false;
    if (r.n < 4u || (r.n & 3u) || r.pos >= r.n || (r.pitch & 3u)) return false;
    if ((uint64_t) r.updates * r.new_frames + r.n > (uint64_t) r.pitch) return false;                  // (so updates * new_frames fits 32 bits)
    if ((reinterpret_cast<uintptr_t>(r.ring) | reinterpret_cast<uintptr_t>(r.stage)) & 15u) return false;
    if ((reinterpret_cast<uintptr_t>(r.starts) & 3u) || (reinterpret_cast<uintptr_t>(r.fresh) & (f32 ? 7u : 3u))) return false;
    return true;
}

// One grid each: a workgroup per 256 pieces of a stream up to the cap, the kernel's loop takes what lies beyond.
hipError_t launch_ring_track_stage(bool f32, const RingTrack& r, hipStream_t st) {
    if (!ring_track_ok(f32, r)) return hipErrorInvalidValue;
    const uint32_t pieces = r.pitch / (f32 ? 2u : 4u), chunks = (pieces + 255u) / 256u;
    const uint64_t items = (uint64_t) r.streams * chunks;
    const unsigned grid = capped_grid((size_t) items, 1, kRingTrackGridCap);
    if (f32) hipLaunchKernelGGL((glv_ring_stage_kernel<3>), dim3(grid), dim3(256), 0, st, r, chunks, grid / chunks, grid % chunks, items);
    else hipLaunchKernelGGL((glv_ring_stage_kernel<2>), dim3(grid), dim3(256), 0, st, r, chunks, grid / chunks, grid % chunks, items);
    return hipGetLastError();
}

hipError_t launch_ring_track_keep(bool f32, const RingTrack& r, hipStream_t st) {
    if (!ring_track_ok(f32, r)) return hipErrorInvalidValue;
    const uint32_t pieces = r.n / (f32 ? 2u : 4u), chunks = (pieces + 255u) / 256u;
    const uint64_t items = (uint64_t) r.streams * chunks;
    const unsigned grid = capped_grid((size_t) items, 1, kRingTrackGridCap);
    if (f32) hipLaunchKernelGGL((glv_ring_keep_kernel<3>), dim3(grid), dim3(256), 0, st, r, chunks, grid / chunks, grid % chunks, items);
    else hipLaunchKernelGGL((glv_ring_keep_kernel<2>), dim3(grid), dim3(256), 0, st, r, chunks, grid / chunks, grid % chunks, items);
    return hipGetLastError();
}

}  // namespace glv
