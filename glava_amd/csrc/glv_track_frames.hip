// glv_track_frames.hip -- the render frames of a track call on gl_storage 3 (glv_batch_track_frames_s16 / _f32): keyframe interpolation and the GL_R16
// upload of every frame's buffer in one launch, and the keyframes a next call starts from in another.
//
//   glv_track_frames_kernel   frame j of row r = unorm16(s + ((e - s) * mod[j])) of keyframes from[j] and to[j] (render.c:1792-1809, :2185, :521-524)
//   glv_track_keys_kernel     d_keys[0] <- keyframe keep_from, d_keys[1] <- keyframe keep_to (render.c:2347-2353 as it stands after the last frame)
//   glv_track_frames_each_kernel / glv_track_keys_each_kernel   both with a row of tables, a count of steps, a count of frames and a keep pair per stream
//                             (glv_batch_track_each_frames_* / glv_batch_track_pool_frames_*)
// ... and of a wave track call on any gl_storage (glv_batch_track_wave_frames_s16 / _f32), whose keyframes are read from the recording:
//   glv_wave_frames_kernel    the same frame from keyframes (u + 1.0F) / 2.0F of the unpacked window of step k - 2 (render.c:777-778), as texels or their floats
//   glv_wave_keys_kernel      the same write-back, as floats
//   glv_wave_frames_planar_kernel / glv_wave_keys_planar_kernel   both from a planar float recording (glv_batch_track_wave_frames_f32_planar)
//   glv_wave_frames_each_kernel / glv_wave_keys_each_kernel   both with a row of tables and of starts, a count of steps, a count of frames and a keep pair per stream,
//                             from recordings or through a span of a pool (glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_*)
#include <hip/hip_runtime.h>

#include "glv_core.h"
#include "glv_launch.h"
#include "glv_launch_util.h"

namespace glv {

typedef float glv_f4 __attribute__((ext_vector_type(4)));
typedef uint32_t glv_u2 __attribute__((ext_vector_type(2)));

// Keyframe k of a call is row block k of `keys` for k < 2 and the finished float rows of step k - 2 beyond: every index a table holds is clamped to
// steps + 1 here, so whatever the tables hold nothing outside the two arrays is read.
// One lane owns four consecutive bins of one channel row (a 16-byte keyframe load, an 8-byte texel store) and walks the frames of one segment with both
// keyframes in registers: a keyframe is loaded when its index changes and taken from the other register where a push moved it there (`from` of a frame is
// `to` of its predecessor whenever an update was pushed between them), so a segment of a live session's tables reads each keyframe row about once instead of
// twice per frame.  The tables hold absolute indices: no frame depends on another, a segment starts anywhere, and the work items are
// [segment][row][group of 256 bins] -- a workgroup is one wave and takes the items blockIdx.x, blockIdx.x + gridDim.x, ... of however many there are.
// The table entries of the frame kFramesDepth ahead are requested with the frame being computed (uniform across the workgroup, inside [0, frames) only), as
// glv_track_scan_kernel requests its rates.
// `limit`: the bins of a row that are written, a multiple of 4 -- the row where the texels are the result, what the bars kernel of the next launch reads else.
// The lerp is the three float operations of render.c:1806 in its order, compiled without contraction; from == to is the keyframe's own bits, no arithmetic
// (render.c:2185 with interpolation off).  The quantiser is pack_unorm16, the upload every gl_storage 3 class applies.
constexpr int kFramesLanes = 64;
constexpr int kFramesDepth = 4;
constexpr size_t kFramesGridCap = 256 * 32;           // 256 CUs x 32 resident waves

__global__ void __launch_bounds__(kFramesLanes) glv_track_frames_kernel(const TrackFrames t, const uint32_t groups, const uint64_t items) {
    const uint32_t last_key = t.steps + 1u;
    uint16_t* const out = static_cast<uint16_t*>(t.out);
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t group = (uint32_t) (item % groups);
        const uint64_t rest = item / groups;
        const uint32_t row = (uint32_t) (rest % t.units);
        const uint32_t seg = (uint32_t) (rest / t.units);
        const uint32_t bin = (group * (uint32_t) kFramesLanes + threadIdx.x) * 4u;
        if (bin >= t.limit) continue;                                       // the last group of a row: nothing of these lanes is read or written
        const uint32_t j0 = seg * t.segment;                                // (< frames: the host counted the segments)
        const uint32_t j1 = t.frames - j0 > t.segment ? j0 + t.segment : t.frames;
        auto key = [&](uint32_t k) -> glv_f4 {
            const float* const base = k < 2u ? t.keys + ((size_t) k * t.units + row) * t.n : t.rows + ((size_t) (k - 2u) * t.units + row) * t.n;
            return *reinterpret_cast<const glv_f4*>(base + bin);
        };
        uint32_t from[kFramesDepth], to[kFramesDepth];
        float mod[kFramesDepth];
#pragma unroll
        for (int d = 0; d < kFramesDepth; ++d) {
            const bool in = (uint32_t) d < j1 - j0;
            from[d] = in ? t.from[j0 + (uint32_t) d] : 0u; to[d] = in ? t.to[j0 + (uint32_t) d] : 0u; mod[d] = in ? t.mod[j0 + (uint32_t) d] : 0.0f;
        }
        uint32_t ks = 0xffffffffu, ke = 0xffffffffu;                         // the keyframes in s and e: none yet (no clamped index is this)
        glv_f4 s = { 0.0f, 0.0f, 0.0f, 0.0f }, e = s;
        for (uint32_t jb = j0; jb < j1; jb += (uint32_t) kFramesDepth) {
#pragma unroll
            for (int d = 0; d < kFramesDepth; ++d) {
                const uint32_t j = jb + (uint32_t) d;
                if (j >= j1) break;
                const uint32_t kf = from[d] < last_key ? from[d] : last_key, kt = to[d] < last_key ? to[d] : last_key;
                const float m = mod[d];
                if (j1 - j > (uint32_t) kFramesDepth) {
                    from[d] = t.from[j + (uint32_t) kFramesDepth]; to[d] = t.to[j + (uint32_t) kFramesDepth]; mod[d] = t.mod[j + (uint32_t) kFramesDepth];
                }
                glv_f4 ns = s;
                if (kf != ks) ns = kf == ke ? e : key(kf);
                if (kt != ke) e = kt == ks ? s : key(kt);
                s = ns; ks = kf; ke = kt;
                glv_f4 w = s;
                if (kf != kt) w = s + ((e - s) * m);                        // render.c:1806
                const glv_u2 c = { pack_unorm16(w.x, w.y), pack_unorm16(w.z, w.w) };    // render.c:521-524
                *reinterpret_cast<glv_u2*>(out + ((size_t) j * t.units + row) * t.n + bin) = c;
            }
        }
    }
}

// Element i of both kept keyframes is read before element i of either destination is written, and no other lane touches element i: the pairs the host
// accepts -- (0, 1), (1, k), (k, k') with 2 <= k < k' -- never read what another lane has written.
__global__ void __launch_bounds__(256) glv_track_keys_kernel(float* keys, const float* rows, const size_t quads, const uint32_t keep_from, const uint32_t keep_to) {
    glv_f4* const k0 = reinterpret_cast<glv_f4*>(keys);
    glv_f4* const k1 = k0 + quads;
    const glv_f4* const steps = reinterpret_cast<const glv_f4*>(rows);
    const glv_f4* const a = keep_from < 2u ? k0 + (size_t) keep_from * quads : steps + (size_t) (keep_from - 2u) * quads;
    const glv_f4* const b = keep_to < 2u ? k0 + (size_t) keep_to * quads : steps + (size_t) (keep_to - 2u) * quads;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += (size_t) gridDim.x * blockDim.x) {
        const glv_f4 va = a[i], vb = b[i];
        k0[i] = va; k1[i] = vb;
    }
}

// The frames stage of a per-stream frames call (glv_batch_track_each_frames_* / glv_batch_track_pool_frames_*): glv_track_frames_kernel's walk with a row of the three
// tables per stream.  What differs, and nothing else: the table base of a work item is (row >> 1) * frames; `last_key` is c_s + 1 of the item's stream,
// c_s = min(counts[s], steps) -- the clamp that stream's one-stream call applies, so no stream reads the zero rows the scan wrote behind its count; the walk
// stops at f_s = min(frame_counts[s], frames), the rest of the segment is stored as zero texels, and no table entry at j >= f_s is requested.
// Both counts are loaded once per item.  Every address the tables and the counts are read at derives from blockIdx.x and the kernel's arguments alone: the tables
// and counts are separate __restrict__ arguments, never written here, so the loads are uniform (scalar memory loads, counted apart from the vector memory counter
// that the chain of 512-byte stores in front of them fills).
__global__ void __launch_bounds__(kFramesLanes) glv_track_frames_each_kernel(const TrackFrames t, const uint32_t* __restrict__ tfrom, const uint32_t* __restrict__ tto,
                                                                             const float* __restrict__ tmod, const uint32_t* __restrict__ frame_counts,
                                                                             const uint32_t* __restrict__ counts, const uint32_t groups, const uint64_t items) {
    uint16_t* const out = static_cast<uint16_t*>(t.out);
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t group = (uint32_t) (item % groups);
        const uint64_t rest = item / groups;
        const uint32_t row = (uint32_t) (rest % t.units);
        const uint32_t seg = (uint32_t) (rest / t.units);
        const uint32_t bin = (group * (uint32_t) kFramesLanes + threadIdx.x) * 4u;
        if (bin >= t.limit) continue;                                       // the last group of a row: nothing of these lanes is read or written
        const uint32_t stream = row >> 1;                                   // (< units / 2: the tables and the counts have a row for it)
        uint32_t c = t.steps, f = t.frames;
        if (counts) { const uint32_t v = counts[stream]; c = v < c ? v : c; }
        if (frame_counts) { const uint32_t v = frame_counts[stream]; f = v < f ? v : f; }
        const uint32_t last_key = c + 1u;                                   // (<= steps + 1)
        const uint32_t j0 = seg * t.segment;                                // (< frames: the host counted the segments)
        const uint32_t j1 = t.frames - j0 > t.segment ? j0 + t.segment : t.frames;
        const uint32_t jw = f <= j0 ? j0 : f < j1 ? f : j1;                 // the walk's end: frames [jw, j1) of the segment lie behind the stream's count
        const uint32_t* const from_s = tfrom + (size_t) stream * t.frames;
        const uint32_t* const to_s = tto + (size_t) stream * t.frames;
        const float* const mod_s = tmod + (size_t) stream * t.frames;
        auto key = [&](uint32_t k) -> glv_f4 {
            const float* const base = k < 2u ? t.keys + ((size_t) k * t.units + row) * t.n : t.rows + ((size_t) (k - 2u) * t.units + row) * t.n;
            return *reinterpret_cast<const glv_f4*>(base + bin);
        };
        uint32_t from[kFramesDepth], to[kFramesDepth];
        float mod[kFramesDepth];
#pragma unroll
        for (int d = 0; d < kFramesDepth; ++d) {
            const bool in = (uint32_t) d < jw - j0;
            from[d] = in ? from_s[j0 + (uint32_t) d] : 0u; to[d] = in ? to_s[j0 + (uint32_t) d] : 0u; mod[d] = in ? mod_s[j0 + (uint32_t) d] : 0.0f;
        }
        uint32_t ks = 0xffffffffu, ke = 0xffffffffu;                         // the keyframes in s and e: none yet (no clamped index is this)
        glv_f4 s = { 0.0f, 0.0f, 0.0f, 0.0f }, e = s;
        for (uint32_t jb = j0; jb < jw; jb += (uint32_t) kFramesDepth) {
#pragma unroll
            for (int d = 0; d < kFramesDepth; ++d) {
                const uint32_t j = jb + (uint32_t) d;
                if (j >= jw) break;
                const uint32_t kf = from[d] < last_key ? from[d] : last_key, kt = to[d] < last_key ? to[d] : last_key;
                const float m = mod[d];
                if (jw - j > (uint32_t) kFramesDepth) {
                    from[d] = from_s[j + (uint32_t) kFramesDepth]; to[d] = to_s[j + (uint32_t) kFramesDepth]; mod[d] = mod_s[j + (uint32_t) kFramesDepth];
                }
                glv_f4 ns = s;
                if (kf != ks) ns = kf == ke ? e : key(kf);
                if (kt != ke) e = kt == ks ? s : key(kt);
                s = ns; ks = kf; ke = kt;
                glv_f4 w = s;
                if (kf != kt) w = s + ((e - s) * m);                        // render.c:1806
                const glv_u2 c2 = { pack_unorm16(w.x, w.y), pack_unorm16(w.z, w.w) };    // render.c:521-524
                *reinterpret_cast<glv_u2*>(out + ((size_t) j * t.units + row) * t.n + bin) = c2;
            }
        }
        for (uint32_t j = jw; j < j1; ++j) *reinterpret_cast<glv_u2*>(out + ((size_t) j * t.units + row) * t.n + bin) = glv_u2{ 0u, 0u };
    }
}

// The write-back of a per-stream frames call: glv_track_keys_kernel's with the pair taken per stream from `keep` (uint32 [streams][2]) and clamped to c_s + 1.  A lane
// reads element i of both kept keyframes before it writes element i of either destination, and no other lane touches element i: any pair is safe.
// per_stream: the quads of one stream's two rows, 2 * n / 4.
__global__ void __launch_bounds__(256) glv_track_keys_each_kernel(float* keys, const float* rows, const size_t quads, const uint32_t per_stream, const uint32_t steps,
                                                                  const uint32_t* __restrict__ counts, const uint32_t* __restrict__ keep) {
    glv_f4* const k0 = reinterpret_cast<glv_f4*>(keys);
    glv_f4* const k1 = k0 + quads;
    const glv_f4* const step_rows = reinterpret_cast<const glv_f4*>(rows);
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < quads; i += (size_t) gridDim.x * blockDim.x) {
        const size_t stream = i / per_stream;
        uint32_t c = steps;
        if (counts) { const uint32_t v = counts[stream]; c = v < c ? v : c; }
        const uint32_t last_key = c + 1u;
        uint32_t kf = keep[2u * stream], kt = keep[2u * stream + 1u];
        kf = kf < last_key ? kf : last_key; kt = kt < last_key ? kt : last_key;
        const glv_f4* const a = kf < 2u ? k0 + (size_t) kf * quads : step_rows + (size_t) (kf - 2u) * quads;
        const glv_f4* const b = kt < 2u ? k0 + (size_t) kt * quads : step_rows + (size_t) (kt - 2u) * quads;
        const glv_f4 va = a[i], vb = b[i];
        k0[i] = va; k1[i] = vb;
    }
}

// The frames of a segment where the caller names none: long enough that a keyframe serves several frames, short enough that a single stream's call still
// fills the chip -- two rounds of the 8192 resident waves where frames * units * groups allow them (a wave's walk is a chain of 512-byte stores: with one
// segment, 64 streams x 3426 frames of N = 4096 ran on 2048 waves and wrote 2.3 TB/s, profiles/r19/track_frames.txt).
constexpr uint64_t kFramesWaves = 2u * kFramesGridCap;
uint32_t track_frames_segment(uint32_t frames, uint32_t units, uint32_t limit) {
    const uint64_t per_segment = (uint64_t) units * ((limit / 4u + (uint32_t) kFramesLanes - 1u) / (uint32_t) kFramesLanes);
    const uint64_t wanted = per_segment >= kFramesWaves ? 1u : (kFramesWaves + per_segment - 1u) / per_segment;
    const uint64_t len = ((uint64_t) frames + wanted - 1u) / wanted;
    return (uint32_t) (len < 8u ? 8u : len);
}

hipError_t launch_track_frames(const TrackFrames& t, hipStream_t st) {
    if (!t.from || !t.to || !t.mod || !t.keys || !t.rows || !t.out) return hipErrorInvalidValue;
    if (t.frames == 0 || t.steps == 0 || t.units == 0 || t.segment == 0 || t.limit == 0 || t.limit > t.n || (t.limit & 3u) || (t.n & 3u) || t.steps > 0xfffffffdu)
        return hipErrorInvalidValue;
    const uint32_t groups = (t.limit / 4u + (uint32_t) kFramesLanes - 1u) / (uint32_t) kFramesLanes;
    const uint64_t segments = ((uint64_t) t.frames + t.segment - 1u) / t.segment;
    const uint64_t items = segments * t.units * groups;                      // (< 2^32 * 2^32 / 4: no overflow)
    const unsigned grid = capped_grid((size_t) items, 1, kFramesGridCap);
    hipLaunchKernelGGL(glv_track_frames_kernel, dim3(grid), dim3(kFramesLanes), 0, st, t, groups, items);
    return hipGetLastError();
}

hipError_t launch_track_keys(float* keys, const float* rows, uint32_t units, uint32_t n, uint32_t keep_from, uint32_t keep_to, hipStream_t st) {
    if (!keys || !rows || units == 0 || n == 0 || (n & 3u)) return hipErrorInvalidValue;
    const size_t quads = (size_t) units * (n / 4u);
    hipLaunchKernelGGL(glv_track_keys_kernel, dim3(capped_grid(quads, 256, kGridCap)), dim3(256), 0, st, keys, rows, quads, keep_from, keep_to);
    return hipGetLastError();
}

hipError_t launch_track_frames_each(const TrackFramesEach& e, hipStream_t st) {
    const TrackFrames& t = e.t;
    if (!t.from || !t.to || !t.mod || !t.keys || !t.rows || !t.out) return hipErrorInvalidValue;
    if (t.frames == 0 || t.steps == 0 || t.units == 0 || (t.units & 1u) || t.segment == 0 || t.limit == 0 || t.limit > t.n || (t.limit & 3u) || (t.n & 3u) || t.steps > 0xfffffffdu)
        return hipErrorInvalidValue;
    const uint32_t groups = (t.limit / 4u + (uint32_t) kFramesLanes - 1u) / (uint32_t) kFramesLanes;
    const uint64_t segments = ((uint64_t) t.frames + t.segment - 1u) / t.segment;
    const uint64_t items = segments * t.units * groups;                      // (< 2^32 * 2^32 / 4: no overflow)
    const unsigned grid = capped_grid((size_t) items, 1, kFramesGridCap);
    hipLaunchKernelGGL(glv_track_frames_each_kernel, dim3(grid), dim3(kFramesLanes), 0, st, t, t.from, t.to, t.mod, e.frame_counts, e.counts, groups, items);
    return hipGetLastError();
}

hipError_t launch_track_keys_each(float* keys, const float* rows, uint32_t units, uint32_t n, uint32_t steps, const uint32_t* counts, const uint32_t* keep, hipStream_t st) {
    if (!keys || !rows || !keep || units == 0 || (units & 1u) || n == 0 || (n & 3u) || steps == 0 || steps > 0xfffffffdu) return hipErrorInvalidValue;
    const size_t quads = (size_t) units * (n / 4u);
    hipLaunchKernelGGL(glv_track_keys_each_kernel, dim3(capped_grid(quads, 256, kGridCap)), dim3(256), 0, st, keys, rows, quads, 2u * (n / 4u), steps, counts, keep);
    return hipGetLastError();
}

// ---- the wave module's render frames (glv_batch_track_wave_frames_s16 / _f32) -----------------------------------------------------------------------------
// A wave keyframe is a trivial function of the recording -- the backend's unpack, wrange's + 1.0F and / 2.0F (render.c:777-778) -- so the steps' float rows never
// exist: keyframe 2 + t is read from the window of step t where it lies, as glv_wave_kernel's kinds 3 and 4 read it (the same helpers, the same clamp of the
// table's entry, the same rule for a group that is not 16-byte aligned), and keyframes 0 and 1 from the caller's d_keys.
// One lane owns FOUR consecutive frames of one stream, both channel rows: 16 bytes of s16 or 32 bytes of floats from the recording, two 16-byte loads from d_keys.
// Bounded reads: i + 4 <= limit <= n and the start is clamped to pitch_frames - n, so a lane reads frames [i, i + 4) of a window inside the recording of a
// stream < streams; a table index is clamped to steps + 1 before it is used, and the starts are read in [0, steps) only.
typedef float glv_f2 __attribute__((ext_vector_type(2)));
typedef uint32_t glv_u4 __attribute__((ext_vector_type(4)));

// KIND: 0 s16 frames, 1 interleaved float frames (the kernels' F32_IN), 2 planar float rows [streams][2][pitch_frames] (WaveWindows::planar;
// glv_batch_track_wave_frames_f32_planar): a lane's four frames of a channel are 16 contiguous bytes of that channel's row, taken as they are -- one 16-byte load
// where they begin on 16 bytes, four dwords else, each row by its own address (pitch_frames is any number).
template <int KIND>
__device__ __forceinline__ void wave_key(const void* pcm, const WaveWindows& w, const int mono, const float* keys, const uint32_t n, const uint32_t k,
                                         const uint32_t stream, const uint32_t i, glv_f4& l, glv_f4& r) {
    if (k < 2u) {
        const float* const base = keys + ((size_t) k * w.units + 2u * stream) * n + i;
        l = *reinterpret_cast<const glv_f4*>(base);
        r = *reinterpret_cast<const glv_f4*>(base + n);
        return;
    }
    const uint32_t step = k - 2u;                                               // (< steps: k was clamped to steps + 1)
    const uint64_t first = wave_window_start(w, stream, step, w.starts[step]) + i;      // the lane's first frame, in 64-bit arithmetic
    float a[4], b[4];
    if constexpr (KIND == 2) {
        const float* const src = static_cast<const float*>(pcm) + (first + (uint64_t) stream * w.pitch_frames);      // (a stream is two rows: its channel-0 row)
        const float* const sib = src + w.pitch_frames;
        if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) { const glv_f4 v = *reinterpret_cast<const glv_f4*>(src); a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = src[q];
        }
        if ((reinterpret_cast<uintptr_t>(sib) & 15u) == 0u) { const glv_f4 v = *reinterpret_cast<const glv_f4*>(sib); b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w; }
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = sib[q];
        }
    } else if constexpr (KIND == 1) {
        const glv_f2* const src = static_cast<const glv_f2*>(pcm) + first;
        glv_f2 f[4];
        if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {
            const glv_f4 lo = *reinterpret_cast<const glv_f4*>(src), hi = *reinterpret_cast<const glv_f4*>(src + 2);
            f[0] = glv_f2{lo.x, lo.y}; f[1] = glv_f2{lo.z, lo.w}; f[2] = glv_f2{hi.x, hi.y}; f[3] = glv_f2{hi.z, hi.w};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (mono) { a[q] = (f[q].x + f[q].y) / 2; b[q] = a[q]; } else { a[q] = f[q].x; b[q] = f[q].y; }     // pulse_input.c:167
        }
    } else {
        const uint32_t* const src = static_cast<const uint32_t*>(pcm) + first;
        uint32_t f[4];
        if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {
            const glv_u4 v = *reinterpret_cast<const glv_u4*>(src);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x = (int16_t) (f[q] & 0xffffu), y = (int16_t) (f[q] >> 16);
            if (mono) { a[q] = unpack_s16_mono(x, y); b[q] = a[q]; } else { a[q] = unpack_s16(x); b[q] = unpack_s16(y); }
        }
    }
    l = glv_f4{(a[0] + 1.0f) / 2.0f, (a[1] + 1.0f) / 2.0f, (a[2] + 1.0f) / 2.0f, (a[3] + 1.0f) / 2.0f};       // render.c:777-778
    r = glv_f4{(b[0] + 1.0f) / 2.0f, (b[1] + 1.0f) / 2.0f, (b[2] + 1.0f) / 2.0f, (b[3] + 1.0f) / 2.0f};
}

// glv_track_frames_kernel's walk with a stream's two channel rows in one lane: `s` and `e` are four float4, a keyframe is loaded when its index changes and taken
// from the other pair of registers where a push moved it there, table entries are requested kFramesDepth ahead.  The work items are
// [segment][stream][group of 256 frames], one wave each, looped beyond the grid.  R16_OUT: the upload's texels, 8 bytes per channel row and frame; else their
// floats c / 65535 (what texelFetch returns: glv_wave_kernel's float form), 16 bytes.
template <bool F32_IN, bool R16_OUT>
__global__ void __launch_bounds__(kFramesLanes) glv_wave_frames_kernel(const void* pcm, const WaveWindows w, const int mono, const WaveFrames t, const uint32_t groups,
                                                                       const uint64_t items) {
    const uint32_t last_key = w.steps + 1u;
    const uint32_t streams = w.units / 2u;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t group = (uint32_t) (item % groups);
        const uint64_t rest = item / groups;
        const uint32_t stream = (uint32_t) (rest % streams);
        const uint32_t seg = (uint32_t) (rest / streams);
        const uint32_t i = (group * (uint32_t) kFramesLanes + threadIdx.x) * 4u;
        if (i >= t.limit) continue;                                         // the last group of a row: nothing of these lanes is read or written
        const uint32_t j0 = seg * t.segment;                                // (< frames: the host counted the segments)
        const uint32_t j1 = t.frames - j0 > t.segment ? j0 + t.segment : t.frames;
        auto emit = [&](uint32_t j, uint32_t c, const glv_f4 v) {
            const uint32_t lo = pack_unorm16(v.x, v.y), hi = pack_unorm16(v.z, v.w);      // render.c:521-524
            const size_t at = ((size_t) j * w.units + 2u * stream + c) * t.n + i;
            if constexpr (R16_OUT) *reinterpret_cast<glv_u2*>(static_cast<uint16_t*>(t.out) + at) = glv_u2{lo, hi};
            else *reinterpret_cast<glv_f4*>(static_cast<float*>(t.out) + at) =
                     glv_f4{unorm16_to_float(lo & 0xffffu), unorm16_to_float(lo >> 16), unorm16_to_float(hi & 0xffffu), unorm16_to_float(hi >> 16)};
        };
        uint32_t from[kFramesDepth], to[kFramesDepth];
        float mod[kFramesDepth];
#pragma unroll
        for (int d = 0; d < kFramesDepth; ++d) {
            const bool in = (uint32_t) d < j1 - j0;
            from[d] = in ? t.from[j0 + (uint32_t) d] : 0u; to[d] = in ? t.to[j0 + (uint32_t) d] : 0u; mod[d] = in ? t.mod[j0 + (uint32_t) d] : 0.0f;
        }
        uint32_t ks = 0xffffffffu, ke = 0xffffffffu;                         // the keyframes in s and e: none yet (no clamped index is this)
        glv_f4 sl = { 0.0f, 0.0f, 0.0f, 0.0f }, sr = sl, el = sl, er = sl;
        for (uint32_t jb = j0; jb < j1; jb += (uint32_t) kFramesDepth) {
#pragma unroll
            for (int d = 0; d < kFramesDepth; ++d) {
                const uint32_t j = jb + (uint32_t) d;
                if (j >= j1) break;
                const uint32_t kf = from[d] < last_key ? from[d] : last_key, kt = to[d] < last_key ? to[d] : last_key;
                const float m = mod[d];
                if (j1 - j > (uint32_t) kFramesDepth) {
                    from[d] = t.from[j + (uint32_t) kFramesDepth]; to[d] = t.to[j + (uint32_t) kFramesDepth]; mod[d] = t.mod[j + (uint32_t) kFramesDepth];
                }
                glv_f4 nl = sl, nr = sr;
                if (kf != ks) { if (kf == ke) { nl = el; nr = er; } else wave_key<F32_IN>(pcm, w, mono, t.keys, t.n, kf, stream, i, nl, nr); }
                if (kt != ke) { if (kt == ks) { el = sl; er = sr; } else wave_key<F32_IN>(pcm, w, mono, t.keys, t.n, kt, stream, i, el, er); }
                sl = nl; sr = nr; ks = kf; ke = kt;
                glv_f4 wl = sl, wr = sr;
                if (kf != kt) { wl = sl + ((el - sl) * m); wr = sr + ((er - sr) * m); }      // render.c:1806
                emit(j, 0u, wl);
                emit(j, 1u, wr);
            }
        }
    }
}

// Element i of both kept keyframes is read before element i of either destination is written, and no other lane touches element i (glv_track_keys_kernel's
// rule); a keyframe beyond the caller's two comes from the recording, which no lane writes.
template <bool F32_IN>
__global__ void __launch_bounds__(256) glv_wave_keys_kernel(const void* pcm, const WaveWindows w, const int mono, float* keys, const uint32_t n, const size_t quads,
                                                            const uint32_t keep_from, const uint32_t keep_to) {
    const uint32_t per_stream = n / 4u;
    for (size_t q = (size_t) blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t) gridDim.x * blockDim.x) {
        const uint32_t stream = (uint32_t) (q / per_stream), i = (uint32_t) (q % per_stream) * 4u;
        glv_f4 al, ar, bl, br;
        wave_key<F32_IN>(pcm, w, mono, keys, n, keep_from, stream, i, al, ar);
        wave_key<F32_IN>(pcm, w, mono, keys, n, keep_to, stream, i, bl, br);
        float* const k0 = keys + (size_t) 2u * stream * n + i;
        float* const k1 = k0 + (size_t) w.units * n;
        *reinterpret_cast<glv_f4*>(k0) = al; *reinterpret_cast<glv_f4*>(k0 + n) = ar;
        *reinterpret_cast<glv_f4*>(k1) = bl; *reinterpret_cast<glv_f4*>(k1 + n) = br;
    }
}

// The planar kinds of both kernels (glv_batch_track_wave_frames_f32_planar): glv_wave_frames_kernel's walk and glv_wave_keys_kernel's write-back over wave_key<2>, word for
// word -- kernels of their own, so that the s16 and float kinds above keep their names and their code (the kinds are template constants, and a third value of a bool
// is another symbol).  `mono` is handed on and never read: planar rows are taken as they are.
template <bool R16_OUT>
__global__ void __launch_bounds__(kFramesLanes) glv_wave_frames_planar_kernel(const void* pcm, const WaveWindows w, const int mono, const WaveFrames t, const uint32_t groups,
                                                                       const uint64_t items) {
    const uint32_t last_key = w.steps + 1u;
    const uint32_t streams = w.units / 2u;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t group = (uint32_t) (item % groups);
        const uint64_t rest = item / groups;
        const uint32_t stream = (uint32_t) (rest % streams);
        const uint32_t seg = (uint32_t) (rest / streams);
        const uint32_t i = (group * (uint32_t) kFramesLanes + threadIdx.x) * 4u;
        if (i >= t.limit) continue;                                         // the last group of a row: nothing of these lanes is read or written
        const uint32_t j0 = seg * t.segment;                                // (< frames: the host counted the segments)
        const uint32_t j1 = t.frames - j0 > t.segment ? j0 + t.segment : t.frames;
        auto emit = [&](uint32_t j, uint32_t c, const glv_f4 v) {
            const uint32_t lo = pack_unorm16(v.x, v.y), hi = pack_unorm16(v.z, v.w);      // render.c:521-524
            const size_t at = ((size_t) j * w.units + 2u * stream + c) * t.n + i;
            if constexpr (R16_OUT) *reinterpret_cast<glv_u2*>(static_cast<uint16_t*>(t.out) + at) = glv_u2{lo, hi};
            else *reinterpret_cast<glv_f4*>(static_cast<float*>(t.out) + at) =
                     glv_f4{unorm16_to_float(lo & 0xffffu), unorm16_to_float(lo >> 16), unorm16_to_float(hi & 0xffffu), unorm16_to_float(hi >> 16)};
        };
        uint32_t from[kFramesDepth], to[kFramesDepth];
        float mod[kFramesDepth];
#pragma unroll
        for (int d = 0; d < kFramesDepth; ++d) {
            const bool in = (uint32_t) d < j1 - j0;
            from[d] = in ? t.from[j0 + (uint32_t) d] : 0u; to[d] = in ? t.to[j0 + (uint32_t) d] : 0u; mod[d] = in ? t.mod[j0 + (uint32_t) d] : 0.0f;
        }
        uint32_t ks = 0xffffffffu, ke = 0xffffffffu;                         // the keyframes in s and e: none yet (no clamped index is this)
        glv_f4 sl = { 0.0f, 0.0f, 0.0f, 0.0f }, sr = sl, el = sl, er = sl;
        for (uint32_t jb = j0; jb < j1; jb += (uint32_t) kFramesDepth) {
#pragma unroll
            for (int d = 0; d < kFramesDepth; ++d) {
                const uint32_t j = jb + (uint32_t) d;
                if (j >= j1) break;
                const uint32_t kf = from[d] < last_key ? from[d] : last_key, kt = to[d] < last_key ? to[d] : last_key;
                const float m = mod[d];
                if (j1 - j > (uint32_t) kFramesDepth) {
                    from[d] = t.from[j + (uint32_t) kFramesDepth]; to[d] = t.to[j + (uint32_t) kFramesDepth]; mod[d] = t.mod[j + (uint32_t) kFramesDepth];
                }
                glv_f4 nl = sl, nr = sr;
                if (kf != ks) { if (kf == ke) { nl = el; nr = er; } else wave_key<2>(pcm, w, mono, t.keys, t.n, kf, stream, i, nl, nr); }
                if (kt != ke) { if (kt == ks) { el = sl; er = sr; } else wave_key<2>(pcm, w, mono, t.keys, t.n, kt, stream, i, el, er); }
                sl = nl; sr = nr; ks = kf; ke = kt;
                glv_f4 wl = sl, wr = sr;
                if (kf != kt) { wl = sl + ((el - sl) * m); wr = sr + ((er - sr) * m); }      // render.c:1806
                emit(j, 0u, wl);
                emit(j, 1u, wr);
            }
        }
    }
}

__global__ void __launch_bounds__(256) glv_wave_keys_planar_kernel(const void* pcm, const WaveWindows w, const int mono, float* keys, const uint32_t n, const size_t quads,
                                                            const uint32_t keep_from, const uint32_t keep_to) {
    const uint32_t per_stream = n / 4u;
    for (size_t q = (size_t) blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t) gridDim.x * blockDim.x) {
        const uint32_t stream = (uint32_t) (q / per_stream), i = (uint32_t) (q % per_stream) * 4u;
        glv_f4 al, ar, bl, br;
        wave_key<2>(pcm, w, mono, keys, n, keep_from, stream, i, al, ar);
        wave_key<2>(pcm, w, mono, keys, n, keep_to, stream, i, bl, br);
        float* const k0 = keys + (size_t) 2u * stream * n + i;
        float* const k1 = k0 + (size_t) w.units * n;
        *reinterpret_cast<glv_f4*>(k0) = al; *reinterpret_cast<glv_f4*>(k0 + n) = ar;
        *reinterpret_cast<glv_f4*>(k1) = bl; *reinterpret_cast<glv_f4*>(k1 + n) = br;
    }
}

hipError_t launch_wave_frames(const void* pcm, bool f32, const WaveWindows& w, bool mono, const WaveFrames& t, bool r16, hipStream_t st) {
    if (!pcm || !w.starts || !t.from || !t.to || !t.mod || !t.keys || !t.out) return hipErrorInvalidValue;
    if (t.frames == 0 || w.steps == 0 || w.steps > 0xfffffffdu || w.units == 0 || (w.units & 1u) || t.segment == 0 || t.limit == 0 || t.limit > t.n || (t.limit & 3u) ||
        (t.n & 3u) || w.pitch_frames < t.n || w.start_max != w.pitch_frames - t.n)
        return hipErrorInvalidValue;
    const uint32_t groups = (t.limit / 4u + (uint32_t) kFramesLanes - 1u) / (uint32_t) kFramesLanes;
    const uint64_t segments = ((uint64_t) t.frames + t.segment - 1u) / t.segment;
    const uint64_t items = segments * (w.units / 2u) * groups;              // (< 2^32 * 2^31 / 4: no overflow)
    const unsigned grid = capped_grid((size_t) items, 1, kFramesGridCap);
    const int m = mono ? 1 : 0;
    if (w.planar) {
        if (!f32) return hipErrorInvalidValue;
        if (r16) hipLaunchKernelGGL((glv_wave_frames_planar_kernel<true>), dim3(grid), dim3(kFramesLanes), 0, st, pcm, w, 0, t, groups, items);
        else hipLaunchKernelGGL((glv_wave_frames_planar_kernel<false>), dim3(grid), dim3(kFramesLanes), 0, st, pcm, w, 0, t, groups, items);
    } else
    if (f32) {
        if (r16) hipLaunchKernelGGL((glv_wave_frames_kernel<true, true>), dim3(grid), dim3(kFramesLanes), 0, st, pcm, w, m, t, groups, items);
        else hipLaunchKernelGGL((glv_wave_frames_kernel<true, false>), dim3(grid), dim3(kFramesLanes), 0, st, pcm, w, m, t, groups, items);
    } else {
        if (r16) hipLaunchKernelGGL((glv_wave_frames_kernel<false, true>), dim3(grid), dim3(kFramesLanes), 0, st, pcm, w, m, t, groups, items);
        else hipLaunchKernelGGL((glv_wave_frames_kernel<false, false>), dim3(grid), dim3(kFramesLanes), 0, st, pcm, w, m, t, groups, items);
    }
    return hipGetLastError();
}

hipError_t launch_wave_keys(const void* pcm, bool f32, const WaveWindows& w, bool mono, float* keys, uint32_t n, uint32_t keep_from, uint32_t keep_to, hipStream_t st) {
    if (!pcm || !w.starts || !keys || n == 0 || (n & 3u) || w.units == 0 || (w.units & 1u) || w.steps == 0 || w.pitch_frames < n || w.start_max != w.pitch_frames - n)
        return hipErrorInvalidValue;
    if ((uint64_t) keep_from >= (uint64_t) w.steps + 2u || (uint64_t) keep_to >= (uint64_t) w.steps + 2u) return hipErrorInvalidValue;
    const size_t quads = (size_t) (w.units / 2u) * (n / 4u);
    const int m = mono ? 1 : 0;
    if (w.planar) {
        if (!f32) return hipErrorInvalidValue;
        hipLaunchKernelGGL(glv_wave_keys_planar_kernel, dim3(capped_grid(quads, 256, kGridCap)), dim3(256), 0, st, pcm, w, 0, keys, n, quads, keep_from, keep_to);
    } else
    if (f32) hipLaunchKernelGGL((glv_wave_keys_kernel<true>), dim3(capped_grid(quads, 256, kGridCap)), dim3(256), 0, st, pcm, w, m, keys, n, quads, keep_from, keep_to);
    else hipLaunchKernelGGL((glv_wave_keys_kernel<false>), dim3(capped_grid(quads, 256, kGridCap)), dim3(256), 0, st, pcm, w, m, keys, n, quads, keep_from, keep_to);
    return hipGetLastError();
}

// ---- the wave module's render frames per stream (glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_*) ------------------------------------
// Both wave kernels above with what glv_track_frames_each_kernel added to its lockstep sibling: a row of the frame tables, a row of the starts, a count of steps, a
// count of frames and a keep pair per stream -- and, for a pool call, the stream's span.  Kernels and a key helper of their own, so that the lockstep kernels and
// wave_key keep their code; the arithmetic is theirs, line for line.
//
// wave_key with the window of step k - 2 of stream s where the per-stream and the pool calls put it: the entry is starts[s * steps + k - 2]; !POOL: wave_window_start's
// clamp of it into the stream's recording, POOL: pool_window_start (glv_frame.h) of the stream's span, one 16-byte load, in 64-bit arithmetic.  Neither the starts
// nor the span is read for k < 2, so a stream without steps (whose every index is clamped to 1) reads its two carried keyframes only.
// KIND as wave_key's; the planar kind's channel rows lie w.pitch_frames floats apart -- the pool's frames in a pool call, whose one pair of rows every stream shares.
// Bounded reads: k - 2 < c_s <= steps (the callers clamp k to c_s + 1), i + 4 <= n, and a window begins at most pitch_frames - n into a recording or pool_frames - n
// into the pool whatever entry and span hold.
template <int KIND, bool POOL>
__device__ __forceinline__ void wave_each_key(const void* pcm, const WaveWindows& w, const int mono, const float* keys, const uint32_t n, const uint32_t k,
                                              const uint32_t stream, const uint32_t i, const uint32_t* __restrict__ starts, const TrackSpan* __restrict__ spans,
                                              const uint64_t pool_frames, glv_f4& l, glv_f4& r) {
    if (k < 2u) {
        const float* const base = keys + ((size_t) k * w.units + 2u * stream) * n + i;
        l = *reinterpret_cast<const glv_f4*>(base);
        r = *reinterpret_cast<const glv_f4*>(base + n);
        return;
    }
    const uint32_t step = k - 2u;                                               // (< c_s <= steps: k was clamped to c_s + 1)
    const uint32_t entry = starts[(size_t) stream * w.steps + step];
    uint64_t first;                                                             // the lane's first frame, in 64-bit arithmetic
    if constexpr (POOL) {
        const glv_u4 v = *reinterpret_cast<const glv_u4*>(spans + stream);
        first = pool_window_start((uint64_t) v.x | (uint64_t) v.y << 32, v.z, entry, pool_frames, (uint64_t) n) + i;
    } else first = wave_window_start(w, stream, step, entry) + i;
    float a[4], b[4];
    if constexpr (KIND == 2) {
        if constexpr (!POOL) first += (uint64_t) stream * w.pitch_frames;      // (a stream is two rows: its channel-0 row)
        const float* const src = static_cast<const float*>(pcm) + first;
        const float* const sib = src + w.pitch_frames;
        if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) { const glv_f4 v = *reinterpret_cast<const glv_f4*>(src); a[0] = v.x; a[1] = v.y; a[2] = v.z; a[3] = v.w; }
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) a[q] = src[q];
        }
        if ((reinterpret_cast<uintptr_t>(sib) & 15u) == 0u) { const glv_f4 v = *reinterpret_cast<const glv_f4*>(sib); b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w; }
        else {
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = sib[q];
        }
    } else if constexpr (KIND == 1) {
        const glv_f2* const src = static_cast<const glv_f2*>(pcm) + first;
        glv_f2 f[4];
        if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {
            const glv_f4 lo = *reinterpret_cast<const glv_f4*>(src), hi = *reinterpret_cast<const glv_f4*>(src + 2);
            f[0] = glv_f2{lo.x, lo.y}; f[1] = glv_f2{lo.z, lo.w}; f[2] = glv_f2{hi.x, hi.y}; f[3] = glv_f2{hi.z, hi.w};
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (mono) { a[q] = (f[q].x + f[q].y) / 2; b[q] = a[q]; } else { a[q] = f[q].x; b[q] = f[q].y; }     // pulse_input.c:167
        }
    } else {
        const uint32_t* const src = static_cast<const uint32_t*>(pcm) + first;
        uint32_t f[4];
        if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {
            const glv_u4 v = *reinterpret_cast<const glv_u4*>(src);
            f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q) f[q] = src[q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int x = (int16_t) (f[q] & 0xffffu), y = (int16_t) (f[q] >> 16);
            if (mono) { a[q] = unpack_s16_mono(x, y); b[q] = a[q]; } else { a[q] = unpack_s16(x); b[q] = unpack_s16(y); }
        }
    }
    l = glv_f4{(a[0] + 1.0f) / 2.0f, (a[1] + 1.0f) / 2.0f, (a[2] + 1.0f) / 2.0f, (a[3] + 1.0f) / 2.0f};       // render.c:777-778
    r = glv_f4{(b[0] + 1.0f) / 2.0f, (b[1] + 1.0f) / 2.0f, (b[2] + 1.0f) / 2.0f, (b[3] + 1.0f) / 2.0f};
}

// glv_wave_frames_kernel's walk over a row of the tables per stream.  What differs, and nothing else (glv_track_frames_each_kernel's list): the table base of a work
// item is stream * frames; `last_key` is c_s + 1 of the item's stream, c_s = min(counts[s], steps), so a keyframe index never names a window behind the stream's
// count; the walk stops at f_s = min(frame_counts[s], frames), the rest of the segment is stored as zero texels (R16_OUT) or their floats 0.0f, and no table entry
// at j >= f_s is requested.  Both counts are loaded once per item.  The frame tables, the counts, the starts and the spans are separate __restrict__ arguments,
// never written here, and every address they are read at derives from blockIdx.x, the kernel's arguments and a uniform table entry: uniform loads, counted apart
// from the vector memory counter that the chain of stores fills.
template <int KIND, bool POOL, bool R16_OUT>
__global__ void __launch_bounds__(kFramesLanes) glv_wave_frames_each_kernel(const void* pcm, const WaveWindows w, const int mono, const WaveFrames t,
                                                                            const uint32_t* __restrict__ tfrom, const uint32_t* __restrict__ tto,
                                                                            const float* __restrict__ tmod, const uint32_t* __restrict__ frame_counts,
                                                                            const uint32_t* __restrict__ counts, const uint32_t* __restrict__ starts,
                                                                            const TrackSpan* __restrict__ spans, const uint64_t pool_frames, const uint32_t groups,
                                                                            const uint64_t items) {
    const uint32_t streams = w.units / 2u;
    for (uint64_t item = blockIdx.x; item < items; item += gridDim.x) {
        const uint32_t group = (uint32_t) (item % groups);
        const uint64_t rest = item / groups;
        const uint32_t stream = (uint32_t) (rest % streams);                // (< streams: the tables, the counts and the spans have a row for it)
        const uint32_t seg = (uint32_t) (rest / streams);
        const uint32_t i = (group * (uint32_t) kFramesLanes + threadIdx.x) * 4u;
        if (i >= t.limit) continue;                                         // the last group of a row: nothing of these lanes is read or written
        uint32_t c = w.steps, f = t.frames;
        if (counts) { const uint32_t v = counts[stream]; c = v < c ? v : c; }
        if (frame_counts) { const uint32_t v = frame_counts[stream]; f = v < f ? v : f; }
        const uint32_t last_key = c + 1u;                                   // (<= steps + 1)
        const uint32_t j0 = seg * t.segment;                                // (< frames: the host counted the segments)
        const uint32_t j1 = t.frames - j0 > t.segment ? j0 + t.segment : t.frames;
        const uint32_t jw = f <= j0 ? j0 : f < j1 ? f : j1;                 // the walk's end: frames [jw, j1) of the segment lie behind the stream's count
        const uint32_t* const from_s = tfrom + (size_t) stream * t.frames;
        const uint32_t* const to_s = tto + (size_t) stream * t.frames;
        const float* const mod_s = tmod + (size_t) stream * t.frames;
        auto key = [&](uint32_t k, glv_f4& l, glv_f4& r) { wave_each_key<KIND, POOL>(pcm, w, mono, t.keys, t.n, k, stream, i, starts, spans, pool_frames, l, r); };
        auto emit = [&](uint32_t j, uint32_t ch, const glv_f4 v) {
            const uint32_t lo = pack_unorm16(v.x, v.y), hi = pack_unorm16(v.z, v.w);      // render.c:521-524
            const size_t at = ((size_t) j * w.units + 2u * stream + ch) * t.n + i;
            if constexpr (R16_OUT) *reinterpret_cast<glv_u2*>(static_cast<uint16_t*>(t.out) + at) = glv_u2{lo, hi};
            else *reinterpret_cast<glv_f4*>(static_cast<float*>(t.out) + at) =
                     glv_f4{unorm16_to_float(lo & 0xffffu), unorm16_to_float(lo >> 16), unorm16_to_float(hi & 0xffffu), unorm16_to_float(hi >> 16)};
        };
        uint32_t from[kFramesDepth], to[kFramesDepth];
        float mod[kFramesDepth];
#pragma unroll
        for (int d = 0; d < kFramesDepth; ++d) {
            const bool in = (uint32_t) d < jw - j0;
            from[d] = in ? from_s[j0 + (uint32_t) d] : 0u; to[d] = in ? to_s[j0 + (uint32_t) d] : 0u; mod[d] = in ? mod_s[j0 + (uint32_t) d] : 0.0f;
        }
        uint32_t ks = 0xffffffffu, ke = 0xffffffffu;                         // the keyframes in s and e: none yet (no clamped index is this)
        glv_f4 sl = { 0.0f, 0.0f, 0.0f, 0.0f }, sr = sl, el = sl, er = sl;
        for (uint32_t jb = j0; jb < jw; jb += (uint32_t) kFramesDepth) {
#pragma unroll
            for (int d = 0; d < kFramesDepth; ++d) {
                const uint32_t j = jb + (uint32_t) d;
                if (j >= jw) break;
                const uint32_t kf = from[d] < last_key ? from[d] : last_key, kt = to[d] < last_key ? to[d] : last_key;
                const float m = mod[d];
                if (jw - j > (uint32_t) kFramesDepth) {
                    from[d] = from_s[j + (uint32_t) kFramesDepth]; to[d] = to_s[j + (uint32_t) kFramesDepth]; mod[d] = mod_s[j + (uint32_t) kFramesDepth];
                }
                glv_f4 nl = sl, nr = sr;
                if (kf != ks) { if (kf == ke) { nl = el; nr = er; } else key(kf, nl, nr); }
                if (kt != ke) { if (kt == ks) { el = sl; er = sr; } else key(kt, el, er); }
                sl = nl; sr = nr; ks = kf; ke = kt;
                glv_f4 wl = sl, wr = sr;
                if (kf != kt) { wl = sl + ((el - sl) * m); wr = sr + ((er - sr) * m); }      // render.c:1806
                emit(j, 0u, wl);
                emit(j, 1u, wr);
            }
        }
        for (uint32_t j = jw; j < j1; ++j) {                                // zero texels: pack_unorm16 of them is 0, and 0 / 65535 is 0.0f
            const size_t at = ((size_t) j * w.units + 2u * stream) * t.n + i;
            if constexpr (R16_OUT) {
                *reinterpret_cast<glv_u2*>(static_cast<uint16_t*>(t.out) + at) = glv_u2{ 0u, 0u };
                *reinterpret_cast<glv_u2*>(static_cast<uint16_t*>(t.out) + at + t.n) = glv_u2{ 0u, 0u };
            } else {
                *reinterpret_cast<glv_f4*>(static_cast<float*>(t.out) + at) = glv_f4{ 0.0f, 0.0f, 0.0f, 0.0f };
                *reinterpret_cast<glv_f4*>(static_cast<float*>(t.out) + at + t.n) = glv_f4{ 0.0f, 0.0f, 0.0f, 0.0f };
            }
        }
    }
}

// glv_wave_keys_kernel's body with the pair taken per stream from `keep` (uint32 [streams][2]) and clamped to c_s + 1: element i of both kept keyframes is read before
// element i of either destination is written, and no other lane touches element i -- any pair is safe.
template <int KIND, bool POOL>
__global__ void __launch_bounds__(256) glv_wave_keys_each_kernel(const void* pcm, const WaveWindows w, const int mono, float* keys, const uint32_t n, const size_t quads,
                                                                 const uint32_t* __restrict__ counts, const uint32_t* __restrict__ keep,
                                                                 const uint32_t* __restrict__ starts, const TrackSpan* __restrict__ spans, const uint64_t pool_frames) {
    const uint32_t per_stream = n / 4u;
    for (size_t q = (size_t) blockIdx.x * blockDim.x + threadIdx.x; q < quads; q += (size_t) gridDim.x * blockDim.x) {
        const uint32_t stream = (uint32_t) (q / per_stream), i = (uint32_t) (q % per_stream) * 4u;
        uint32_t c = w.steps;
        if (counts) { const uint32_t v = counts[stream]; c = v < c ? v : c; }
        const uint32_t last_key = c + 1u;
        uint32_t kf = keep[2u * stream], kt = keep[2u * stream + 1u];
        kf = kf < last_key ? kf : last_key; kt = kt < last_key ? kt : last_key;
        glv_f4 al, ar, bl, br;
        wave_each_key<KIND, POOL>(pcm, w, mono, keys, n, kf, stream, i, starts, spans, pool_frames, al, ar);
        wave_each_key<KIND, POOL>(pcm, w, mono, keys, n, kt, stream, i, starts, spans, pool_frames, bl, br);
        float* const k0 = keys + (size_t) 2u * stream * n + i;
        float* const k1 = k0 + (size_t) w.units * n;
        *reinterpret_cast<glv_f4*>(k0) = al; *reinterpret_cast<glv_f4*>(k0 + n) = ar;
        *reinterpret_cast<glv_f4*>(k1) = bl; *reinterpret_cast<glv_f4*>(k1 + n) = br;
    }
}

// what both launchers ask of the windows: a table with a row per stream, and a recording (or a pool behind an aligned span table) that holds one window
static bool wave_each_ok(const void* pcm, int kind, const WaveWindows& w, const TrackPool& pool, uint32_t n) {
    if (!pcm || !w.starts || kind < 0 || kind > 2 || (w.planar != 0u) != (kind == 2)) return false;
    if (n == 0 || (n & 3u) || w.units == 0 || (w.units & 1u) || w.steps == 0 || w.steps > 0xfffffffdu) return false;
    if (pool.spans) return (reinterpret_cast<uintptr_t>(pool.spans) & 15u) == 0u && pool.frames >= n && w.pitch_frames == pool.frames;      // (pool_window_start subtracts the window)
    return w.pitch_frames >= n && w.start_max == w.pitch_frames - n;
}

#define GLV_WAVE_EACH_KINDS(GO) \
    do { \
        if (pooled) { if (kind == 2) GO(2, true); else if (kind == 1) GO(1, true); else GO(0, true); } \
        else { if (kind == 2) GO(2, false); else if (kind == 1) GO(1, false); else GO(0, false); } \
    } while (0)

hipError_t launch_wave_each_frames(const void* pcm, int kind, const WaveWindows& w, bool mono, const WaveFramesEach& e, bool r16, hipStream_t st) {
    const WaveFrames& t = e.t;
    if (!wave_each_ok(pcm, kind, w, e.pool, t.n) || !t.from || !t.to || !t.mod || !t.keys || !t.out) return hipErrorInvalidValue;
    if (t.frames == 0 || t.segment == 0 || t.limit == 0 || t.limit > t.n || (t.limit & 3u)) return hipErrorInvalidValue;
    const uint32_t groups = (t.limit / 4u + (uint32_t) kFramesLanes - 1u) / (uint32_t) kFramesLanes;
    const uint64_t segments = ((uint64_t) t.frames + t.segment - 1u) / t.segment;
    const uint64_t items = segments * (w.units / 2u) * groups;              // (< 2^32 * 2^31 / 4: no overflow)
    const unsigned grid = capped_grid((size_t) items, 1, kFramesGridCap);
    const int m = mono && kind != 2 ? 1 : 0;
    const bool pooled = e.pool.spans != nullptr;
#define GLV_WAVE_EACH_FRAMES(KIND, POOL) \
    do { if (r16) hipLaunchKernelGGL((glv_wave_frames_each_kernel<KIND, POOL, true>), dim3(grid), dim3(kFramesLanes), 0, st, pcm, w, m, t, t.from, t.to, t.mod, \
                                     e.frame_counts, e.counts, w.starts, e.pool.spans, e.pool.frames, groups, items); \
         else hipLaunchKernelGGL((glv_wave_frames_each_kernel<KIND, POOL, false>), dim3(grid), dim3(kFramesLanes), 0, st, pcm, w, m, t, t.from, t.to, t.mod, \
                                 e.frame_counts, e.counts, w.starts, e.pool.spans, e.pool.frames, groups, items); } while (0)
    GLV_WAVE_EACH_KINDS(GLV_WAVE_EACH_FRAMES);
#undef GLV_WAVE_EACH_FRAMES
    return hipGetLastError();
}

hipError_t launch_wave_each_keys(const void* pcm, int kind, const WaveWindows& w, bool mono, const WaveKeysEach& k, hipStream_t st) {
    if (!wave_each_ok(pcm, kind, w, k.pool, k.n) || !k.keys || !k.keep) return hipErrorInvalidValue;
    const size_t quads = (size_t) (w.units / 2u) * (k.n / 4u);
    const unsigned grid = capped_grid(quads, 256, kGridCap);
    const int m = mono && kind != 2 ? 1 : 0;
    const bool pooled = k.pool.spans != nullptr;
#define GLV_WAVE_EACH_KEYS(KIND, POOL) \
    hipLaunchKernelGGL((glv_wave_keys_each_kernel<KIND, POOL>), dim3(grid), dim3(256), 0, st, pcm, w, m, k.keys, k.n, quads, k.counts, k.keep, w.starts, k.pool.spans, \
                       k.pool.frames)
    GLV_WAVE_EACH_KINDS(GLV_WAVE_EACH_KEYS);
#undef GLV_WAVE_EACH_KEYS
    return hipGetLastError();
}
#undef GLV_WAVE_EACH_KINDS

}  // namespace glv
