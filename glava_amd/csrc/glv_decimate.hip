// glv_decimate.hip -- `setbufscale k` on the batched layer (glv_batch_set_bufscale): rd_update's box decimation (render.c:1765-1790) of every window of a
// process or track call in one launch, from the frames where they lie into planar float rows of n = bufsize / k samples.
//
//   glv_decimate_kernel<KIND>   out[t] = (((0.0F + x[t k]) + x[t k + 1]) + ... + x[t k + k - 1]) / (float) k   per channel row
//
// x is the backend's unpack of the frame (unpack_s16 / unpack_s16_mono, fifo.c:94-110; a float frame's samples or (l + r) / 2, pulse_input.c:167) -- or, for the
// planar kind, the caller's lb / rb rows themselves.  Every addition and the one division are float32 operations of their own in that order: the unit is
// compiled without contraction, the sum starts from +0.0F (a window whose first sample is -0.0F gives +0.0F, as the reference's accumulator does), nothing is
// pre-summed as integers and nothing is multiplied by a reciprocal.  glv_bufscale_kernel (glv_misc.hip: glv_prelude_bufscale, float rows) stays as it is.
#include <hip/hip_runtime.h>

#include "glv_core.h"
#include "glv_launch.h"
#include "glv_launch_util.h"

namespace glv {

typedef float glv_f4 __attribute__((ext_vector_type(4)));
typedef float glv_f2 __attribute__((ext_vector_type(2)));
typedef uint32_t glv_u4 __attribute__((ext_vector_type(4)));

// Four consecutive frames of a lane's span, both channels.  `aligned`: the lane's first byte lies on 16 bytes, and so does every group of four frames behind
// it (16 bytes of s16 frames, 32 of float frames, 16 of each planar row) -- 16-byte loads; else naturally aligned loads of one frame (4 bytes of s16, 8 of
// floats) or one sample (planar).  A track window begins at any frame, so s16 recordings promise 4 bytes and float ones 8.  The planar track kind's windows
// begin at any sample of a row and the second row lies pitch_frames floats on, any number: each row takes the 16-byte load where ITS first byte lies on 16.
template <int KIND>
__device__ __forceinline__ void decimate_group(const void* lane, const uint64_t row_pitch, const uint32_t g, const bool aligned, const int mono, float (&l)[4], float (&r)[4]) {
    if constexpr (KIND == DEC_S16) {
        const uint32_t* const src = static_cast<const uint32_t*>(lane) + (size_t) g * 4u;
        uint32_t f[4];
        if (aligned) {
            const glv_u4 v = *reinterpret_cast<const glv_u4*>(src);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x = (int16_t) (f[q] & 0xffffu), y = (int16_t) (f[q] >> 16);
            if (mono) { l[q] = unpack_s16_mono(x, y); r[q] = l[q]; } else { l[q] = unpack_s16(x); r[q] = unpack_s16(y); }
        }
    } else if constexpr (KIND == DEC_F32) {
        const glv_f2* const src = static_cast<const glv_f2*>(lane) + (size_t) g * 4u;
        glv_f2 f[4];
        if (aligned) {
            const glv_f4 lo = *reinterpret_cast<const glv_f4*>(src), hi = *reinterpret_cast<const glv_f4*>(src + 2);
            f[0] = glv_f2{lo.x, lo.y}; f[1] = glv_f2{lo.z, lo.w}; f[2] = glv_f2{hi.x, hi.y}; f[3] = glv_f2{hi.z, hi.w};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (mono) { l[q] = (f[q].x + f[q].y) / 2.0f; r[q] = l[q]; } else { l[q] = f[q].x; r[q] = f[q].y; }      // pulse_input.c:167
        }
    } else {
        const float* const a = static_cast<const float*>(lane) + (size_t) g * 4u;
        const float* const b = a + row_pitch;
        if constexpr (KIND == DEC_F32_PLANAR_TRACK) {
            if (aligned) { const glv_f4 va = *reinterpret_cast<const glv_f4*>(a); l[0] = va.x; l[1] = va.y; l[2] = va.z; l[3] = va.w; }
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q) l[q] = a[q];
            }
            if ((reinterpret_cast<uintptr_t>(b) & 15u) == 0u) { const glv_f4 vb = *reinterpret_cast<const glv_f4*>(b); r[0] = vb.x; r[1] = vb.y; r[2] = vb.z; r[3] = vb.w; }
            else {
#pragma unroll
                for (int q = 0; q < 4; ++q) r[q] = b[q];
            }
        } else
        if (aligned) {
            const glv_f4 va = *reinterpret_cast<const glv_f4*>(a), vb = *reinterpret_cast<const glv_f4*>(b);
            l[0] = va.x; l[1] = va.y; l[2] = va.z; l[3] = va.w; r[0] = vb.x; r[1] = vb.y; r[2] = vb.z; r[3] = vb.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) { l[q] = a[q]; r[q] = b[q]; }
        }
    }
}

// One lane owns four consecutive output samples of a window's row pair: the 4 k consecutive frames [4 k i, 4 k (i + 1)) of the window, walked as k groups of
// four with the running sums of both channels in registers.  k is a run-time bound; a sum is finished every k frames, which falls on the same frame in every
// lane (the counters depend on k alone: scalar registers), and the finished mean goes into its place among the lane's four by selects -- no indexed
// register, no scratch.  Work items are [window f = s * steps + t][group of four samples], 256 lanes a workgroup, looped beyond the grid.
// Bounded reads: 4 k (i + 1) <= k n and a window's start is at most start_max = pitch_frames - k n behind its stream's first frame (a table's entry is clamped
// where it is read: track_window_start), so whatever a table holds a lane reads inside the recording of a stream < streams; the table is read in [0, steps).
// The planar kind (a process call's lb / rb rows, [streams][2][k n]) has no table and no hop: window s is rows 2 s and 2 s + 1.
// The planar track kind (glv_batch_track_at_f32_planar under bufscale: [streams][2][pitch_frames]) cuts window t of stream s out of rows 2 s and 2 s + 1 by the
// interleaved kinds' rules -- the same start within each row, the same clamp, the same output row -- with no mix, as the planar kind.
template <int KIND>
__global__ void __launch_bounds__(256) glv_decimate_kernel(const Decimate d, const uint32_t log_quads, const uint64_t items) {
    const float fk = (float) d.k;
    const uint64_t span = (uint64_t) d.k * d.n;                              // frames of a window
    for (uint64_t item = (uint64_t) blockIdx.x * 256u + threadIdx.x; item < items; item += (uint64_t) gridDim.x * 256u) {
        const uint32_t f = (uint32_t) (item >> log_quads);                   // (< 2^31 windows: the host counted them)
        const uint32_t i = (uint32_t) item & ((1u << log_quads) - 1u);
        const uint32_t s = f / d.w.steps, t = f - s * d.w.steps;
        const uint64_t lead = (uint64_t) i * 4u * d.k;                       // the lane's first frame within its window
        const void* lane;
        if constexpr (KIND == DEC_F32_PLANAR) lane = static_cast<const float*>(d.in) + ((uint64_t) 2u * f * span + lead);
        else {
            // (per-stream rows, table_len = windows: entry t of row s is entry f -- glv_frame.h track_table_entry, f < windows; uniform across the launch)
            const bool rows = d.w.starts && d.w.table_len != d.w.steps;
            const uint64_t first = (rows ? track_window_start(d.w, s, t, track_table_entry(d.w, f))
                                         : track_window_start(d.w, s, t, d.w.starts ? d.w.starts[t] : 0u)) + lead;      // 64-bit: a recording may pass 2^32 frames
            if constexpr (KIND == DEC_S16) lane = static_cast<const uint32_t*>(d.in) + first;
            else if constexpr (KIND == DEC_F32) lane = static_cast<const glv_f2*>(d.in) + first;
            else lane = static_cast<const float*>(d.in) + (first + (uint64_t) s * d.w.pitch_frames);      // (a stream is two rows of pitch_frames floats: its channel-0 row)
        }
        const bool aligned = (reinterpret_cast<uintptr_t>(lane) & 15u) == 0u;      // (planar: the second row lies k n floats on, a multiple of 16 bytes)
        float suml = 0.0f, sumr = 0.0f, outl[4], outr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { outl[q] = 0.0f; outr[q] = 0.0f; }
        uint32_t count = 0, slot = 0;
        for (uint32_t g = 0; g < d.k; ++g) {
            float l[4], r[4];
            decimate_group<KIND>(lane, KIND == DEC_F32_PLANAR_TRACK ? d.w.pitch_frames : span, g, aligned, (int) d.mono, l, r);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                suml = suml + l[q]; sumr = sumr + r[q];                      // render.c:1774, in index order
                if (++count == d.k) {
                    const float ml = suml / fk, mr = sumr / fk;              // render.c:1776
#pragma unroll
                    for (int o = 0; o < 4; ++o) { outl[o] = slot == (uint32_t) o ? ml : outl[o]; outr[o] = slot == (uint32_t) o ? mr : outr[o]; }
                    ++slot; count = 0; suml = 0.0f; sumr = 0.0f;
                }
            }
        }
        float* const row = d.out + (KIND == DEC_F32_PLANAR ? (uint64_t) 2u * f : track_window_row(d.w, s, t)) * d.n + (uint64_t) i * 4u;
        *reinterpret_cast<glv_f4*>(row) = glv_f4{outl[0], outl[1], outl[2], outl[3]};
        *reinterpret_cast<glv_f4*>(row + d.n) = glv_f4{outr[0], outr[1], outr[2], outr[3]};
    }
}

hipError_t launch_decimate(int kind, const Decimate& d, hipStream_t st) {
    if (!d.in || !d.out || d.k < 2u || d.k > 16u || d.n < 256u || (d.n & (d.n - 1u)) || d.w.steps == 0 || d.w.streams == 0) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(d.out) & 15u) || (reinterpret_cast<uintptr_t>(d.in) & (kind == DEC_F32 ? 7u : 3u))) return hipErrorInvalidValue;
    const uint64_t span = (uint64_t) d.k * d.n, windows = (uint64_t) d.w.steps * d.w.streams;
    if (windows > 0x7fffffffull) return hipErrorInvalidValue;
    if (d.w.starts && d.w.table_len != d.w.steps && (uint64_t) d.w.table_len != windows) return hipErrorInvalidValue;      // a table is one row, or a row per stream
    if (kind == DEC_F32_PLANAR) { if (d.w.steps != 1u || d.w.starts) return hipErrorInvalidValue; }
    else if (d.w.pitch_frames < span || (d.w.starts ? (uint64_t) d.w.start_max != d.w.pitch_frames - span
                                                    : (uint64_t) (d.w.steps - 1u) * d.w.hop > d.w.pitch_frames - span)) return hipErrorInvalidValue;
    uint32_t log_quads = 0;
    while ((4u << log_quads) < d.n) ++log_quads;
    const uint64_t items = windows << log_quads;
    const unsigned grid = capped_grid((size_t) items, 256, kDecimateGridCap);
    if (kind == DEC_S16) hipLaunchKernelGGL((glv_decimate_kernel<DEC_S16>), dim3(grid), dim3(256), 0, st, d, log_quads, items);
    else if (kind == DEC_F32) hipLaunchKernelGGL((glv_decimate_kernel<DEC_F32>), dim3(grid), dim3(256), 0, st, d, log_quads, items);
    else if (kind == DEC_F32_PLANAR) hipLaunchKernelGGL((glv_decimate_kernel<DEC_F32_PLANAR>), dim3(grid), dim3(256), 0, st, d, log_quads, items);
    else if (kind == DEC_F32_PLANAR_TRACK) hipLaunchKernelGGL((glv_decimate_kernel<DEC_F32_PLANAR_TRACK>), dim3(grid), dim3(256), 0, st, d, log_quads, items);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace glv
