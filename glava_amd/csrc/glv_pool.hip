// glv_pool.hip -- a pool call's small kernels (glv_batch_track_pool_s16 / _f32 / _f32_planar): the stages in front of the transform that read PCM, over ONE
// buffer of recordings that every stream reads through a span of its own.
//
//   glv_decimate_pool_kernel<KIND>   glv_decimate_kernel's three track kinds (glv_decimate.hip): `setbufscale k`, windows of k n frames
//   glv_wave_pool_kernel<KIND, R16>  glv_wave_kernel's window kinds 3, 4 and 5 (glv_misc.hip): GLV_OP_WAVE, unpack -> wrange -> GL_R16
//
// Kernels of their own, so that those two keep their code byte for byte; the arithmetic is theirs line by line (the unit is compiled without contraction, as
// they are), and what differs is where a window begins: pool_window_start (glv_frame.h) of the stream's span, the entry of its table row, the pool's frames and
// the window's k n.  The span is one 16-byte load per lane and window, uniform across the lanes of a window, from a table of `streams` records that sits in L2.
// Bounded reads: pool_window_start is at most pool.frames - k n whatever span and table hold, and a lane reads inside [start, start + k n) as in the kernels these
// are copies of -- inside the pool (the planar kinds: inside each of its two rows, pool.frames floats apart).  The launchers refuse a pool below one window.
#include <hip/hip_runtime.h>

#include "glv_core.h"
#include "glv_launch.h"
#include "glv_launch_util.h"

namespace glv {

typedef float glv_pool_f4 __attribute__((ext_vector_type(4)));
typedef float glv_pool_f2 __attribute__((ext_vector_type(2)));
typedef uint32_t glv_pool_u4 __attribute__((ext_vector_type(4)));

// window (s, entry)'s first frame in the pool: the span of stream s, one 16-byte load
static __device__ __forceinline__ uint64_t pool_start(const TrackPool& pool, uint32_t s, uint32_t entry, uint64_t window) {
    const glv_pool_u4 v = *reinterpret_cast<const glv_pool_u4*>(pool.spans + s);
    return pool_window_start((uint64_t) v.x | (uint64_t) v.y << 32, v.z, entry, pool.frames, window);
}

// ---- bufscale: decimate_group of glv_decimate.hip for the three track kinds (four consecutive frames of a lane's span, both channels) ------------------------
template <int KIND>
__device__ __forceinline__ void pool_decimate_group(const void* lane, const uint64_t row_pitch, const uint32_t g, const bool aligned, const int mono, float (&l)[4], float (&r)[4]) {
    if constexpr (KIND == DEC_S16) {
        const uint32_t* const src = static_cast<const uint32_t*>(lane) + (size_t) g * 4u;
        uint32_t f[4];
        if (aligned) {
            const glv_pool_u4 v = *reinterpret_cast<const glv_pool_u4*>(src);
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
        const glv_pool_f2* const src = static_cast<const glv_pool_f2*>(lane) + (size_t) g * 4u;
        glv_pool_f2 f[4];
        if (aligned) {
            const glv_pool_f4 lo = *reinterpret_cast<const glv_pool_f4*>(src), hi = *reinterpret_cast<const glv_pool_f4*>(src + 2);
            f[0] = glv_pool_f2{lo.x, lo.y}; f[1] = glv_pool_f2{lo.z, lo.w}; f[2] = glv_pool_f2{hi.x, hi.y}; f[3] = glv_pool_f2{hi.z, hi.w};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (mono) { l[q] = (f[q].x + f[q].y) / 2.0f; r[q] = l[q]; } else { l[q] = f[q].x; r[q] = f[q].y; }      // pulse_input.c:167
        }
    } else {
        static_assert(KIND == DEC_F32_PLANAR_TRACK, "a pool call has the three track kinds");
        const float* const a = static_cast<const float*>(lane) + (size_t) g * 4u;
        const float* const b = a + row_pitch;
        if (aligned) { const glv_pool_f4 va = *reinterpret_cast<const glv_pool_f4*>(a); l[0] = va.x; l[1] = va.y; l[2] = va.z; l[3] = va.w; }
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) l[q] = a[q];
        }
        if ((reinterpret_cast<uintptr_t>(b) & 15u) == 0u) { const glv_pool_f4 vb = *reinterpret_cast<const glv_pool_f4*>(b); r[0] = vb.x; r[1] = vb.y; r[2] = vb.z; r[3] = vb.w; }
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = b[q];
        }
    }
}

// glv_decimate_kernel's walk (one lane: four consecutive output samples of a window's row pair, k groups of four frames, sums from +0.0F in index order, one
// division) with the lane's first frame at pool_start + lead.  d.w: steps, streams, step_major, the per-stream rows of the table (table_len = steps * streams);
// its pitch_frames is the planar kind's channel stride, pool.frames.
template <int KIND>
__global__ void __launch_bounds__(256) glv_decimate_pool_kernel(const Decimate d, const TrackPool pool, const uint32_t log_quads, const uint64_t items) {
    const float fk = (float) d.k;
    const uint64_t span = (uint64_t) d.k * d.n;                              // frames of a window
    for (uint64_t item = (uint64_t) blockIdx.x * 256u + threadIdx.x; item < items; item += (uint64_t) gridDim.x * 256u) {
        const uint32_t f = (uint32_t) (item >> log_quads);                   // (< 2^31 windows: the host counted them)
        const uint32_t i = (uint32_t) item & ((1u << log_quads) - 1u);
        const uint32_t s = f / d.w.steps, t = f - s * d.w.steps;
        const uint64_t lead = (uint64_t) i * 4u * d.k;                       // the lane's first frame within its window
        const uint64_t first = pool_start(pool, s, track_table_entry(d.w, f), span) + lead;      // (f < windows = table_len: entry t of row s)
        const void* lane;
        if constexpr (KIND == DEC_S16) lane = static_cast<const uint32_t*>(d.in) + first;
        else if constexpr (KIND == DEC_F32) lane = static_cast<const glv_pool_f2*>(d.in) + first;
        else lane = static_cast<const float*>(d.in) + first;                 // (the pool's channel-0 row; channel 1 lies pool.frames floats on)
        const bool aligned = (reinterpret_cast<uintptr_t>(lane) & 15u) == 0u;
        float suml = 0.0f, sumr = 0.0f, outl[4], outr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) { outl[q] = 0.0f; outr[q] = 0.0f; }
        uint32_t count = 0, slot = 0;
        for (uint32_t g = 0; g < d.k; ++g) {
            float l[4], r[4];
            pool_decimate_group<KIND>(lane, pool.frames, g, aligned, (int) d.mono, l, r);
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
        float* const row = d.out + track_window_row(d.w, s, t) * d.n + (uint64_t) i * 4u;
        *reinterpret_cast<glv_pool_f4*>(row) = glv_pool_f4{outl[0], outl[1], outl[2], outl[3]};
        *reinterpret_cast<glv_pool_f4*>(row + d.n) = glv_pool_f4{outr[0], outr[1], outr[2], outr[3]};
    }
}

// what both launchers ask of a pool: a span table to load 16 bytes at a time from, and one whole window
static bool pool_ok(const TrackPool& pool, uint64_t window) {
    return pool.spans && (reinterpret_cast<uintptr_t>(pool.spans) & 15u) == 0u && window != 0 && pool.frames >= window;      // (pool_window_start subtracts the window)
}

hipError_t launch_decimate_pool(int kind, const Decimate& d, const TrackPool& pool, hipStream_t st) {
    if (!d.in || !d.out || d.k < 2u || d.k > 16u || d.n < 256u || (d.n & (d.n - 1u)) || d.w.steps == 0 || d.w.streams == 0) return hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(d.out) & 15u) || (reinterpret_cast<uintptr_t>(d.in) & (kind == DEC_F32 ? 7u : 3u))) return hipErrorInvalidValue;
    const uint64_t span = (uint64_t) d.k * d.n, windows = (uint64_t) d.w.steps * d.w.streams;
    if (windows > 0x7fffffffull || !pool_ok(pool, span)) return hipErrorInvalidValue;
    if (!d.w.starts || (uint64_t) d.w.table_len != windows) return hipErrorInvalidValue;      // a pool call's table has a row per stream
    uint32_t log_quads = 0;
    while ((4u << log_quads) < d.n) ++log_quads;
    const uint64_t items = windows << log_quads;
    const unsigned grid = capped_grid((size_t) items, 256, kDecimateGridCap);
    if (kind == DEC_S16) hipLaunchKernelGGL((glv_decimate_pool_kernel<DEC_S16>), dim3(grid), dim3(256), 0, st, d, pool, log_quads, items);
    else if (kind == DEC_F32) hipLaunchKernelGGL((glv_decimate_pool_kernel<DEC_F32>), dim3(grid), dim3(256), 0, st, d, pool, log_quads, items);
    else if (kind == DEC_F32_PLANAR_TRACK) hipLaunchKernelGGL((glv_decimate_pool_kernel<DEC_F32_PLANAR_TRACK>), dim3(grid), dim3(256), 0, st, d, pool, log_quads, items);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

// ---- GLV_OP_WAVE: glv_wave_kernel's window kinds over the pool (KIND 3: s16 frames, 4: interleaved float frames, 5: planar float rows) ----------------------
// One lane takes 8 frames of a window: `s` counts windows step-major (window t * streams + stream), the group's first frame is pool_start + t, a group that
// does not lie on 16 bytes takes its frames one naturally aligned load at a time, and both channel rows' 8 values leave as texels (R16) or as the floats
// c / 65535.  w: units, steps and the per-stream rows of the table (w.hop = steps: the entries between two streams' rows).
template <int KIND, bool R16>
__global__ void __launch_bounds__(256) glv_wave_pool_kernel(const void* __restrict__ in, void* __restrict__ out, size_t groups_total, uint32_t n, uint32_t limit, int mono,
                                                            const WaveWindows w, const TrackPool pool) {
    static_assert(KIND >= 3 && KIND <= 5, "a pool call has the three window kinds");
    const uint32_t gpr = limit / 8u;                                     // groups of 8 samples per window
    auto emit = [&](size_t row, uint32_t t, const float (&x)[8]) {
        uint32_t c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float p0 = x[2 * q] + 1.0f, p1 = x[2 * q + 1] + 1.0f;  // render.c:777-778
            c[q] = pack_unorm16(p0 / 2.0f, p1 / 2.0f);                   // render.c:521-524
        }
        if constexpr (R16) {
            st<glv_pool_u4>(static_cast<uint16_t*>(out) + row * n, t * 2u, glv_pool_u4{c[0], c[1], c[2], c[3]});
        } else {
            BarW4 lo, hi;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                lo.w[2 * q] = unorm16_to_float(c[q] & 0xffffu); lo.w[2 * q + 1] = unorm16_to_float(c[q] >> 16);
                hi.w[2 * q] = unorm16_to_float(c[2 + q] & 0xffffu); hi.w[2 * q + 1] = unorm16_to_float(c[2 + q] >> 16);
            }
            st<BarW4>(static_cast<float*>(out) + row * n, t * 4u, lo);
            st<BarW4>(static_cast<float*>(out) + row * n, t * 4u + 16u, hi);
        }
    };
    const uint32_t streams = w.units / 2u;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < groups_total; i += (size_t) gridDim.x * blockDim.x) {
        const size_t s = i / gpr;                                        // window
        const uint32_t t = (uint32_t) (i % gpr) * 8u;
        const uint32_t step = (uint32_t) (s / streams);
        const uint32_t stream = (uint32_t) (s % streams);
        const uint64_t first = pool_start(pool, stream, w.starts[(size_t) stream * w.hop + step], n) + t;      // the group's first frame
        if constexpr (KIND == 3) {
            const uint32_t* src = static_cast<const uint32_t*>(in) + first;
            uint32_t f[8];
            if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {
                const glv_pool_u4 a = ld<glv_pool_u4>(src, 0u), b = ld<glv_pool_u4>(src, 16u);
                f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 8; ++q) f[q] = src[q];
            }
            float l[8], r[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int a = (int16_t) (f[q] & 0xffffu), b = (int16_t) (f[q] >> 16);
                if (mono) { l[q] = unpack_s16_mono(a, b); r[q] = l[q]; } else { l[q] = unpack_s16(a); r[q] = unpack_s16(b); }
            }
            emit(2 * s, t, l);                                           // (row t' * units + 2 stream + c = 2 s + c)
            emit(2 * s + 1, t, r);
        } else if constexpr (KIND == 4) {
            const cf* src = static_cast<const cf*>(in) + first;
            cf f[8];
            if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {
#pragma unroll
                for (uint32_t q = 0; q < 4; ++q) {
                    const BarW4 a = ld<BarW4>(src, q * 16u);
                    f[2 * q] = cf{a.w[0], a.w[1]}; f[2 * q + 1] = cf{a.w[2], a.w[3]};
                }
            } else {
#pragma unroll
                for (uint32_t q = 0; q < 8; ++q) f[q] = src[q];
            }
            float l[8], r[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                if (mono) { l[q] = (f[q].x + f[q].y) / 2; r[q] = l[q]; } else { l[q] = f[q].x; r[q] = f[q].y; }     // pulse_input.c:167
            }
            emit(2 * s, t, l);
            emit(2 * s + 1, t, r);
        } else {
            const float* src = static_cast<const float*>(in) + first;
#pragma unroll
            for (uint32_t c = 0; c < 2u; ++c, src += pool.frames) {       // channel c of the group: the same 8 samples of the row pool.frames floats on
                float x[8];
                if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {
                    const BarW4 a = ld<BarW4>(src, 0u), b = ld<BarW4>(src, 16u);
                    x[0] = a.w[0]; x[1] = a.w[1]; x[2] = a.w[2]; x[3] = a.w[3]; x[4] = b.w[0]; x[5] = b.w[1]; x[6] = b.w[2]; x[7] = b.w[3];
                } else {
#pragma unroll
                    for (uint32_t q = 0; q < 8; ++q) x[q] = src[q];
                }
                emit(2 * s + c, t, x);
            }
        }
    }
}

hipError_t launch_wave_track_pool(const void* pool_pcm, bool f32, const WaveWindows& w, const TrackPool& pool, bool mono, uint32_t n, void* out, bool r16, uint32_t limit,
                                  hipStream_t st) {
    if (limit == 0 || limit > n || (limit & 7u) || w.units == 0 || (w.units & 1u) || w.steps == 0) return hipErrorInvalidValue;
    if (!pool_pcm || !out || !w.starts || w.hop != w.steps || !pool_ok(pool, n)) return hipErrorInvalidValue;      // a pool call's table has a row per stream
    if (w.planar && !f32) return hipErrorInvalidValue;
    const size_t total = (size_t) w.steps * (w.units / 2u) * (limit / 8u);
    const unsigned grid = capped_grid(total, 256, kGridCap);      // (total >= 1: glv_misc.hip grid_256's grid for glv_wave_kernel)
    const int m = mono && !w.planar ? 1 : 0;
#define GLV_WAVE_POOL_LAUNCH(KIND) \
    do { if (r16) hipLaunchKernelGGL((glv_wave_pool_kernel<KIND, true>), dim3(grid), dim3(256), 0, st, pool_pcm, out, total, n, limit, m, w, pool); \
         else hipLaunchKernelGGL((glv_wave_pool_kernel<KIND, false>), dim3(grid), dim3(256), 0, st, pool_pcm, out, total, n, limit, m, w, pool); } while (0)
    if (w.planar) GLV_WAVE_POOL_LAUNCH(5);
    else if (f32) GLV_WAVE_POOL_LAUNCH(4);
    else GLV_WAVE_POOL_LAUNCH(3);
#undef GLV_WAVE_POOL_LAUNCH
    return hipGetLastError();
}

}  // namespace glv
