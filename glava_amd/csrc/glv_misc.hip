// glv_misc.hip -- the small kernels and the size dispatch (the bars passes of a second launch: glv_bars.hip).
//
//   glv_post_kernel         gravity / average / wrange on spectra already in HBM (the single-op
//                           drop-ins glv_gravity, glv_average, glv_wrange; glava/render.c:720-781) and
//                           the magnitude stage alone (glv_magnitude; render.c:842-846)
//   glv_track_scan_kernel   the scan over time of a track call
//   glv_unpack_kernel       s16 interleaved -> planar f32 (glv_unpack_s16; glava/fifo.c:94-110)
//   glv_ring_planar_kernel  the device rings as the reference's backends publish them
//   glv_wave_kernel         GLV_OP_WAVE: unpack -> wrange -> GL_R16 upload
//   glv_bufscale_kernel, glv_lerp_kernel          the rd_update prelude
//   glv_smooth_kernel, glv_smooth_ring_kernel     the CPU path's transform_smooth
//   launch_window_split, launch_window_split_check   the s16 window as float pairs (glv_winsplit.h)
//   launch_frame, frame_variants, frame_variant_ok, frame_geometry   the frame kernel by size (glv_inst.hip)
#include <hip/hip_runtime.h>

#include <type_traits>

#include "glv_frame.h"
#include "glv_launch.h"
#include "glv_launch_util.h"
#include "glv_winsplit.h"

namespace glv {

// One lane owns one pair of floats (8 B) of a row and runs the same state machine as the
// fused epilogue (apply_state).
__global__ void __launch_bounds__(256) glv_post_kernel(const FrameArgs a, const uint32_t n) {
    const size_t pairs_per_row = n / 2;
    const size_t total = (size_t) a.units * pairs_per_row;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t) gridDim.x * blockDim.x) {
        const size_t row = i / pairs_per_row;
        const uint32_t off = (uint32_t) (i % pairs_per_row) * 8u;     // byte offset of the pair in its row
        cf val = ld<cf>(static_cast<const float*>(a.in) + row * n, off);
        if (a.ops & OP_MAGNITUDE) {                                               // render.c:842-846
            const float y0 = __builtin_fabsf(val.x) + 1.0f, y1 = __builtin_fabsf(val.y) + 1.0f;
            const cf tl = ld<cf>(a.tilt, off);
            if (a.log_mode == 0)      { val.x = log_third_nf<0, true>(y0, a.logtab) * tl.x; val.y = log_third_nf<0, true>(y1, a.logtab) * tl.y; }
            else if (a.log_mode == 1) { val.x = log_third<1>(y0, a.logtab, kLogTabMaxBits) * tl.x; val.y = log_third<1>(y1, a.logtab, kLogTabMaxBits) * tl.y; }
            else                      { val.x = log_third<2>(y0, a.logtab, kLogTabMaxBits) * tl.x; val.y = log_third<2>(y1, a.logtab, kLogTabMaxBits) * tl.y; }
        }
        if (a.ops & OP_WRANGE) {                                                  // render.c:777-779
            const float p = val.x + 1.0f, q = val.y + 1.0f;
            val.x = p / 2.0f; val.y = q / 2.0f;
        }
        val = apply_state(val, off, row, n, a);
        if (a.out) {
            if (a.ops & OP_R16) st<uint32_t>(reinterpret_cast<uint16_t*>(a.out) + row * n, off / 2u, pack_unorm16(val.x, val.y));   // render.c:521-524
            else st<cf>(a.out + row * n, off, val);
        }
    }
}

// ---- the scan over time of a track call (glv_batch_track_s16) ---------------------------------------------------------------------
// The transform launches left every window of every stream as one finished row (texels where the chain's first act is the GL_R16 upload,
// IN16; floats else).  gravity and the average are a recurrence over time per bin: one lane owns one float pair / texel pair of one channel
// row, like glv_post_kernel, and walks the `steps` updates with the gravity value in a register and the F-slot ring in LDS -- [F][lanes],
// lane-contiguous: every access of a wave is 64 consecutive words.  The batch's state arrays are read once before the first step and
// written once after the last, in the layout `steps` sequential calls would have left (the ring by slot: the host advances the head).
// A lane touches its own column of the ring only: no barrier anywhere.  The step is apply_state's / apply_state_r16's, helper by helper.
// The row of a step does not depend on the state: kTrackDepth steps' loads are in flight ahead of the one being computed (a register ring,
// indices compile-time) -- at few streams the loop is a chain of HBM round trips otherwise.
// A live track call (glv_batch_track_live_s16 / _f32) walks the kept bins only, TrackGeometry::kept of every row's n: units * ceil(kept / 128) workgroups, and
// a lane whose pair lies at or beyond kept / 2 leaves before it touches state, rows or LDS.
// Window t of stream s starts at frame s * pitch + t * hop = (s * hops_per_pitch + t) * hop of the whole sequence: with q = n / hop it is row
// k = h >> log_q of the residue launch r = h & (q - 1), whose rows start at r * residue_rows.
constexpr int kTrackLanes = 64;          // one wave per workgroup: with few streams the lanes of a row spread over n / 128 CUs
constexpr int kTrackDepth = 8;
// The rates kind (RATES; glv_batch_track_rates_s16 / _f32): gravity's step changes from update to update, as a live GLava's measured gl->ur does -- step tt
// applies g = gravity_step * (1.0F / ur[tt]) (render.c:728: a correctly rounded division, then a separate multiply; the units are compiled without contraction),
// evaluated here because the host cannot see a table in device memory without a synchronise.  The entry of step tt + kTrackDepth is requested with that step's
// row, in a register ring beside ahead[]: uniform across the workgroup, in [0, steps) only, and like the row never in the dependent chain of a step.  Texel
// state takes the float expression the pass is defined by at every step (gravity_r16_flt): the host accepts the packed integer step only after checking it
// against this very expression for all 65 536 texel values (glv_tables.h gravity_r16_integer_step), so the bits are those of the sequential calls whichever
// arm each of them took.  The other kinds' code has no table in it.
template <bool IN16, bool RATES = false>
__global__ void __launch_bounds__(kTrackLanes) glv_track_scan_kernel(const FrameArgs a, const TrackGeometry t) {
    using V = typename std::conditional<IN16, uint32_t, cf>::type;         // one lane's element of a row: a texel pair / a float pair
    extern __shared__ __attribute__((aligned(8))) unsigned char track_lds[];
    V* const ring = reinterpret_cast<V*>(track_lds) + threadIdx.x;          // slot f of this lane: ring[f * kTrackLanes]
    const uint32_t blocks_per_row = (t.kept + 2u * (uint32_t) kTrackLanes - 1u) / (2u * (uint32_t) kTrackLanes);   // (kept: a multiple of 64 bins; n for every call but a live track call's)
    const uint32_t row = blockIdx.x / blocks_per_row;                       // uniform: a workgroup lies inside one channel row
    const uint32_t pair = (blockIdx.x % blocks_per_row) * (uint32_t) kTrackLanes + threadIdx.x;
    if (pair >= t.kept / 2u) return;                                        // the last workgroup's upper half-wave where kept is an odd multiple of 64: nothing of it is read or written
    const uint32_t off = pair * (uint32_t) sizeof(V);                       // byte offset in an input / state row
    const size_t row_bytes = (size_t) t.n * (sizeof(V) / 2u);
    const uint32_t F = a.F;
    const bool grav = (a.ops & OP_GRAVITY) != 0, avg = (a.ops & OP_AVERAGE) != 0, windowed = a.avg_window != 0;
    const bool out16 = t.out_texels != 0;
    // ---- the lane's slice of the state, once
    V gs = V();
    if (avg) {
        const char* h = reinterpret_cast<const char*>(a.hist) + (size_t) row * F * row_bytes;
        for (uint32_t f = 0; f < F; ++f) ring[f * kTrackLanes] = ld<V>(h + (size_t) f * row_bytes, off);
    } else if (grav) gs = ld<V>(reinterpret_cast<const char*>(a.grav) + (size_t) row * row_bytes, off);
    uint32_t head = a.head;
    // ---- where step tt's row lies, and where its result goes (uniform arithmetic)
    const uint64_t h0 = (uint64_t) (row >> 1) * t.hops_per_pitch;
    const uint32_t q_mask = (1u << t.log_q) - 1u;
    const char* const in = static_cast<const char*>(a.in);
    auto fetch = [&](uint32_t tt) -> V {
        const uint64_t h = h0 + tt;
        const uint64_t in_row = (uint64_t) ((uint32_t) h & q_mask) * t.residue_rows + 2u * (h >> t.log_q) + (row & 1u);
        return ld<V>(in + in_row * row_bytes, off);
    };
    char* const out = reinterpret_cast<char*>(a.out);
    const size_t out_row_bytes = (size_t) t.n * (out16 ? 2u : 4u);
    const uint32_t out_off = pair * (out16 ? 4u : 8u);
    auto step = [&](V x, uint32_t tt, float g) {
        char* const o = out + ((size_t) tt * a.units + row) * out_row_bytes;
        if constexpr (IN16) {
            uint32_t tex = x;                                               // apply_state_r16
            if (grav) {
                const uint32_t store = avg ? ring[(F == 1 ? head : ring_slot(head, F - 2, F)) * kTrackLanes] : gs;
                if constexpr (RATES) tex = gravity_r16_flt(tex, store, g);
                else tex = gravity_r16(tex, store, a.g, a.grav_sub, a.grav_int);
                if (!avg) gs = tex;
            }
            if (avg) {
                cf acc = { 0.0f, 0.0f };
                for (uint32_t f = 0; f + 1 < F; ++f) weighted_texels(acc, ring[ring_slot(head, f, F) * kTrackLanes], a.wts32[f], windowed);
                ring[head * kTrackLanes] = tex;
                if (F > 1) {
                    weighted_texels(acc, tex, a.wts32[F - 1], windowed);
                    tex = pack_unorm16(div_frames(acc.x, a.F_as_float, a.F_rcp), div_frames(acc.y, a.F_as_float, a.F_rcp));
                }
                head = head + 1u == F ? 0u : head + 1u;
            }
            if (out16) st<uint32_t>(o, out_off, tex);
            else st<cf>(o, out_off, texels_to_float(tex));
        } else {
            cf val = x;                                                     // apply_state, the float chain
            if (avg) {
                cf acc = { 0.0f, 0.0f }, prev = { 0.0f, 0.0f };
                if (F == 1) prev = ring[head * kTrackLanes];
                for (uint32_t f = 0; f + 1 < F; ++f) {
                    prev = ring[ring_slot(head, f, F) * kTrackLanes];
                    average_add(acc, prev, a.wts[f], windowed);
                }
                if (grav) { val.x = gravity(val.x, prev.x, g); val.y = gravity(val.y, prev.y, g); }
                ring[head * kTrackLanes] = val;
                average_add(acc, val, a.wts[F - 1], windowed);
                val = average_end(acc, a.F_as_float);
                head = head + 1u == F ? 0u : head + 1u;
            } else if (grav) {
                val.x = gravity(val.x, gs.x, g); val.y = gravity(val.y, gs.y, g);
                gs = val;
            }
            if (out16) st<uint32_t>(o, out_off, pack_unorm16(val.x, val.y));    // render.c:521-524
            else st<cf>(o, out_off, val);
        }
    };
    // ---- the walk
    V ahead[kTrackDepth];
    float rate[RATES ? kTrackDepth : 1];                                    // the rates kind: ur of the steps whose rows are in flight
#pragma unroll
    for (int j = 0; j < kTrackDepth; ++j) {
        ahead[j] = (uint32_t) j < t.steps ? fetch((uint32_t) j) : V();
        if constexpr (RATES) rate[j] = (uint32_t) j < t.steps ? t.ur[j] : 1.0f;
    }
    for (uint32_t t0 = 0; t0 < t.steps; t0 += (uint32_t) kTrackDepth) {
#pragma unroll
        for (int j = 0; j < kTrackDepth; ++j) {
            const uint32_t tt = t0 + (uint32_t) j;
            if (tt >= t.steps) break;
            const V x = ahead[j];
            float g = a.g;
            if constexpr (RATES) g = t.gravity_step * (1.0F / rate[j]);    // render.c:728
            if (tt + (uint32_t) kTrackDepth < t.steps) {
                ahead[j] = fetch(tt + (uint32_t) kTrackDepth);
                if constexpr (RATES) rate[j] = t.ur[tt + (uint32_t) kTrackDepth];
            }
            step(x, tt, g);
        }
    }
    // ---- the state the sequential calls would have left
    if (avg) {
        char* h = reinterpret_cast<char*>(a.hist) + (size_t) row * F * row_bytes;
        for (uint32_t f = 0; f < F; ++f) st<V>(h + (size_t) f * row_bytes, off, ring[f * kTrackLanes]);
    } else if (grav) st<V>(reinterpret_cast<char*>(a.grav_w) + (size_t) row * row_bytes, off, gs);
}

// ---- the scan of a per-stream track call (glv_batch_track_each_s16 / _f32 / _f32_planar) ------------------------------------------------------------------
// glv_track_scan_kernel's walk with what a stream of its own needs, in a kernel of its own: the kinds above keep their code and their arguments.
// Counts: stream s = row >> 1 takes c = min(counts[s], steps) steps (uniform per workgroup: a workgroup lies inside one channel row; loaded once; no table: all
// steps).  The walk, the look-ahead ring and the rate requests are bounded by c, so no row and no rate at or beyond step c is asked for; the output rows of steps
// [c, steps) receive zeros -- the finished row of a step that did not run, which the call's last stage (bars, columns) turns into what it makes of a zero row.
// Rates (RATES): step tt of stream s applies g = gravity_step * (1.0F / ur[s * steps + tt]), the rates kind's expression on the stream's own row; texel state then
// takes the float form at every step, as there.  !RATES: FrameArgs::g and the packed integer texel step (gravity_r16), exactly as the plain kinds -- a call with
// counts alone on texel state keeps the integer arm wherever the sequential calls take it.
// State afterwards: the batch's head advances by `steps` for every stream (the host cannot see the counts), this stream's own by c.  The ring was loaded slot by
// slot under the batch's head and walked under the stream's; slot p is written back to slot (p + steps - c) % F, so the row of age j under the stream's head sits
// where age j sits under (head + steps) % F -- what the next call reads.  c = 0: the ring turned by steps % F and the gravity row as it was, every age in place.
template <bool IN16, bool RATES>
__global__ void __launch_bounds__(kTrackLanes) glv_track_each_scan_kernel(const FrameArgs a, const TrackGeometry t, const TrackEach e) {
    using V = typename std::conditional<IN16, uint32_t, cf>::type;
    extern __shared__ __attribute__((aligned(8))) unsigned char track_each_lds[];
    V* const ring = reinterpret_cast<V*>(track_each_lds) + threadIdx.x;     // slot f of this lane: ring[f * kTrackLanes]
    const uint32_t blocks_per_row = (t.kept + 2u * (uint32_t) kTrackLanes - 1u) / (2u * (uint32_t) kTrackLanes);
    const uint32_t row = blockIdx.x / blocks_per_row;                       // uniform
    const uint32_t pair = (blockIdx.x % blocks_per_row) * (uint32_t) kTrackLanes + threadIdx.x;
    if (pair >= t.kept / 2u) return;
    const uint32_t off = pair * (uint32_t) sizeof(V);
    const size_t row_bytes = (size_t) t.n * (sizeof(V) / 2u);
    const uint32_t F = a.F;
    const bool grav = (a.ops & OP_GRAVITY) != 0, avg = (a.ops & OP_AVERAGE) != 0, windowed = a.avg_window != 0;
    const bool out16 = t.out_texels != 0;
    const uint32_t stream = row >> 1;
    uint32_t c = t.steps;                                                   // the stream's steps: uniform
    if (e.counts) { const uint32_t own = e.counts[stream]; c = own < t.steps ? own : t.steps; }
    const float* const ur = RATES ? e.ur + (size_t) stream * t.steps : nullptr;      // the stream's row of the rate table, read in [0, c)
    // ---- the lane's slice of the state, once
    V gs = V();
    if (avg) {
        const char* h = reinterpret_cast<const char*>(a.hist) + (size_t) row * F * row_bytes;
        for (uint32_t f = 0; f < F; ++f) ring[f * kTrackLanes] = ld<V>(h + (size_t) f * row_bytes, off);
    } else if (grav) gs = ld<V>(reinterpret_cast<const char*>(a.grav) + (size_t) row * row_bytes, off);
    uint32_t head = a.head;
    // ---- where step tt's row lies (the windows form: row (stream * steps + tt) * 2 + channel), and where its result goes
    const char* const in = static_cast<const char*>(a.in);
    auto fetch = [&](uint32_t tt) -> V { return ld<V>(in + (((uint64_t) stream * t.steps + tt) * 2u + (row & 1u)) * row_bytes, off); };
    char* const out = reinterpret_cast<char*>(a.out);
    const size_t out_row_bytes = (size_t) t.n * (out16 ? 2u : 4u);
    const uint32_t out_off = pair * (out16 ? 4u : 8u);
    auto step = [&](V x, uint32_t tt, float g) {
        char* const o = out + ((size_t) tt * a.units + row) * out_row_bytes;
        if constexpr (IN16) {
            uint32_t tex = x;                                               // apply_state_r16
            if (grav) {
                const uint32_t store = avg ? ring[(F == 1 ? head : ring_slot(head, F - 2, F)) * kTrackLanes] : gs;
                if constexpr (RATES) tex = gravity_r16_flt(tex, store, g);
                else tex = gravity_r16(tex, store, a.g, a.grav_sub, a.grav_int);
                if (!avg) gs = tex;
            }
            if (avg) {
                cf acc = { 0.0f, 0.0f };
                for (uint32_t f = 0; f + 1 < F; ++f) weighted_texels(acc, ring[ring_slot(head, f, F) * kTrackLanes], a.wts32[f], windowed);
                ring[head * kTrackLanes] = tex;
                if (F > 1) {
                    weighted_texels(acc, tex, a.wts32[F - 1], windowed);
                    tex = pack_unorm16(div_frames(acc.x, a.F_as_float, a.F_rcp), div_frames(acc.y, a.F_as_float, a.F_rcp));
                }
                head = head + 1u == F ? 0u : head + 1u;
            }
            if (out16) st<uint32_t>(o, out_off, tex);
            else st<cf>(o, out_off, texels_to_float(tex));
        } else {
            cf val = x;                                                     // apply_state, the float chain
            if (avg) {
                cf acc = { 0.0f, 0.0f }, prev = { 0.0f, 0.0f };
                if (F == 1) prev = ring[head * kTrackLanes];
                for (uint32_t f = 0; f + 1 < F; ++f) {
                    prev = ring[ring_slot(head, f, F) * kTrackLanes];
                    average_add(acc, prev, a.wts[f], windowed);
                }
                if (grav) { val.x = gravity(val.x, prev.x, g); val.y = gravity(val.y, prev.y, g); }
                ring[head * kTrackLanes] = val;
                average_add(acc, val, a.wts[F - 1], windowed);
                val = average_end(acc, a.F_as_float);
                head = head + 1u == F ? 0u : head + 1u;
            } else if (grav) {
                val.x = gravity(val.x, gs.x, g); val.y = gravity(val.y, gs.y, g);
                gs = val;
            }
            if (out16) st<uint32_t>(o, out_off, pack_unorm16(val.x, val.y));    // render.c:521-524
            else st<cf>(o, out_off, val);
        }
    };
    // ---- the walk over the stream's own steps [0, c)
    V ahead[kTrackDepth];
    float rate[RATES ? kTrackDepth : 1];
#pragma unroll
    for (int j = 0; j < kTrackDepth; ++j) {
        ahead[j] = (uint32_t) j < c ? fetch((uint32_t) j) : V();
        if constexpr (RATES) rate[j] = (uint32_t) j < c ? ur[j] : 1.0f;
    }
    for (uint32_t t0 = 0; t0 < c; t0 += (uint32_t) kTrackDepth) {
#pragma unroll
        for (int j = 0; j < kTrackDepth; ++j) {
            const uint32_t tt = t0 + (uint32_t) j;
            if (tt >= c) break;
            const V x = ahead[j];
            float g = a.g;
            if constexpr (RATES) g = t.gravity_step * (1.0F / rate[j]);    // render.c:728
            if (tt + (uint32_t) kTrackDepth < c) {
                ahead[j] = fetch(tt + (uint32_t) kTrackDepth);
                if constexpr (RATES) rate[j] = ur[tt + (uint32_t) kTrackDepth];
            }
            step(x, tt, g);
        }
    }
    // ---- the steps behind the count: a finished row of zeros each
    for (uint32_t tt = c; tt < t.steps; ++tt) {
        char* const o = out + ((size_t) tt * a.units + row) * out_row_bytes;
        if (out16) st<uint32_t>(o, out_off, 0u);
        else st<cf>(o, out_off, cf{0.0f, 0.0f});
    }
    // ---- the state c sequential calls would have left, presented at the batch's new head
    if (avg) {
        char* h = reinterpret_cast<char*>(a.hist) + (size_t) row * F * row_bytes;
        const uint32_t turn = (t.steps - c) % F;
        for (uint32_t f = 0; f < F; ++f) {
            const uint32_t to = f + turn >= F ? f + turn - F : f + turn;
            st<V>(h + (size_t) to * row_bytes, off, ring[f * kTrackLanes]);
        }
    } else if (grav) st<V>(reinterpret_cast<char*>(a.grav_w) + (size_t) row * row_bytes, off, gs);
}

__global__ void __launch_bounds__(256) glv_unpack_kernel(const int16_t* __restrict__ pcm, size_t frames, int mono,
                                                         float* __restrict__ l, float* __restrict__ r) {
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < frames; i += (size_t) gridDim.x * blockDim.x) {
        const uint32_t u = reinterpret_cast<const uint32_t*>(pcm)[i];
        const int a = (int16_t) (u & 0xffffu), b = (int16_t) (u >> 16);
        if (mono) { const float s = unpack_s16_mono(a, b); l[i] = s; r[i] = s; }
        else { l[i] = unpack_s16(a); r[i] = unpack_s16(b); }
    }
}

// The device rings as the reference's backends publish them in audio_out_l / audio_out_r (glava/fifo.h:9-20): planar f32,
// oldest sample first (fifo.c:91-92 / pulse_input.c:155-156 keep that order by memmove; the device rings are circular and
// `rot` is the index of their oldest frame).  s16 ring: the unpack of fifo.c:94-110; f32 ring: the deinterleave of
// pulse_input.c:159-176; mono: the respective (L + R) / 2 into both outputs.
__global__ void __launch_bounds__(256) glv_ring_planar_kernel(const void* __restrict__ ring, int is_f32, uint32_t n, uint32_t rot, int mono,
                                                              size_t streams, float* __restrict__ out) {
    const size_t total = streams * n;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t) gridDim.x * blockDim.x) {
        const size_t s = i / n;
        const uint32_t t = (uint32_t) (i % n);
        const size_t src = s * n + ((t + rot) & (n - 1));
        float l, r;
        if (is_f32) {
            const cf u = static_cast<const cf*>(ring)[src];
            if (mono) { l = (u.x + u.y) / 2; r = l; } else { l = u.x; r = u.y; }              // pulse_input.c:167
        } else {
            const uint32_t u = static_cast<const uint32_t*>(ring)[src];
            const int a = (int16_t) (u & 0xffffu), b = (int16_t) (u >> 16);
            if (mono) { l = unpack_s16_mono(a, b); r = l; } else { l = unpack_s16(a); r = unpack_s16(b); }
        }
        out[(s * 2) * n + t] = l;
        out[(s * 2 + 1) * n + t] = r;
    }
}

// ---- GLV_OP_WAVE: the wave module's bind (shaders/glava/wave/1.frag:7-9: window, wrange) ---------------
// Per channel row: the backend's unpack (fifo.c:94-110 / pulse_input.c:155-178; mono: the mix into both rows), transform_wrange (render.c:773-781:
// b += 1.0F; b /= 2.0F) and the GL_R16 upload (render.c:521-524), written as the texels c (R16) or as the floats c / 65535 texelFetch returns.
// KIND 0 / 1: interleaved s16 / f32 frames -- one lane takes 8 frames of a stream (two 16-byte loads of s16, four of f32) and stores both channel
// rows' 8 values (one 16-byte store of texels per row, two of floats): 4 n bytes in and 4 n (8 n) out per s16 stereo frame.  `rot` is the index of
// the oldest frame of a device ring (0 for frames); a rotation that is not a multiple of 8 frames can wrap inside a group and takes the frames one
// by one.  KIND 2: planar f32 rows, taken as they are (the lb / rb snapshot is already unpacked), 8 samples per lane.  Only the first `limit` samples
// of a row (a multiple of 8) are produced -- in front of the bars kernel that is what the bars sample; out rows keep their pitch of n.
typedef unsigned int glv_wave_u4 __attribute__((ext_vector_type(4)));
// KIND 3 (glv_batch_track_wave_s16): KIND 0's arithmetic over every window of a track call -- `s` counts windows, step-major (window t * streams + stream),
// whose frames start at stream * pitch_frames + t * hop of the recordings (WaveWindows; the other kinds never read it).  A window starts at any frame:
// frames are dwords, so a group whose first frame is not 16-byte aligned takes its 8 frames one naturally aligned dword at a time.
// KIND 4 (glv_batch_track_wave_f32): KIND 1's unpack over the same windows of float recordings, 8 bytes per frame.  A group's first frame is 8-byte
// aligned and no more: 16-byte aligned it takes KIND 1's four 16-byte loads, otherwise its 8 frames one naturally aligned 8-byte load at a time.
// KIND 5 (glv_batch_track_at_f32_planar): the same windows of PLANAR float recordings, float [streams][2][pitch_frames] (WaveWindows::planar) -- KIND 2's rows taken
// as they are, no mix, each channel's 8 samples from its own row: two 16-byte loads where the group's first float of THAT row lies on 16 bytes, else 8 dwords
// (a window begins at any sample and pitch_frames is any number, so the two rows of a stream may differ).  Bounded as KIND 3 and 4, within row 2 stream + c.
// Bounded reads (KIND 3 and 4): s < steps * streams and t + 8 <= limit <= n, so a lane reads frames [t, t + 8) of a window the call names and no others.
// A table call (WaveWindows::starts): the window of step t' begins min(starts[t'], pitch_frames - n) frames into the recording -- one lookup per lane and group
// of 8 frames, t' < steps, from a table that sits in L2; the clamp keeps the window inside the recording whatever the table holds.  With per-stream rows
// (with a table WaveWindows::hop is the table's: steps between two streams' rows, glv_batch_track_each_*; 0 for one shared row) the entry is starts[stream * steps + t'], stream < streams: inside uint32 [streams][steps].
template <int KIND, bool R16>
__global__ void __launch_bounds__(256) glv_wave_kernel(const void* __restrict__ in, void* __restrict__ out, size_t groups_total, uint32_t n, uint32_t limit,
                                                       uint32_t rot, int mono, const WaveWindows w) {
    const uint32_t gpr = limit / 8u;                                     // groups of 8 samples per row (KIND 2) / per stream (window)
    auto emit = [&](size_t row, uint32_t t, const float (&x)[8]) {
        uint32_t c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float p0 = x[2 * q] + 1.0f, p1 = x[2 * q + 1] + 1.0f;  // render.c:777-778
            c[q] = pack_unorm16(p0 / 2.0f, p1 / 2.0f);                   // render.c:521-524
        }
        if constexpr (R16) {
            st<glv_wave_u4>(static_cast<uint16_t*>(out) + row * n, t * 2u, glv_wave_u4{c[0], c[1], c[2], c[3]});
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
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < groups_total; i += (size_t) gridDim.x * blockDim.x) {
        const size_t s = i / gpr;                                        // stream (KIND 0 / 1) or row (KIND 2)
        const uint32_t t = (uint32_t) (i % gpr) * 8u;
        if constexpr (KIND == 2) {
            const float* src = static_cast<const float*>(in) + s * n;
            const BarW4 a = ld<BarW4>(src, t * 4u), b = ld<BarW4>(src, t * 4u + 16u);
            const float x[8] = {a.w[0], a.w[1], a.w[2], a.w[3], b.w[0], b.w[1], b.w[2], b.w[3]};
            emit(s, t, x);
        } else if constexpr (KIND == 3) {
            const uint32_t streams = w.units / 2u;
            const uint32_t step = (uint32_t) (s / streams);
            const uint32_t stream = (uint32_t) (s % streams);
            const uint64_t first = wave_window_start(w, stream, step, w.starts ? w.starts[(size_t) stream * w.hop + step] : 0u) + t;      // the group's first frame
            const uint32_t* src = static_cast<const uint32_t*>(in) + first;
            uint32_t f[8];
            if ((reinterpret_cast<uintptr_t>(src) & 15u) == 0u) {
                const glv_wave_u4 a = ld<glv_wave_u4>(src, 0u), b = ld<glv_wave_u4>(src, 16u);
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
            const uint32_t streams = w.units / 2u;
            const uint32_t step = (uint32_t) (s / streams);
            const uint32_t stream = (uint32_t) (s % streams);
            const uint64_t first = wave_window_start(w, stream, step, w.starts ? w.starts[(size_t) stream * w.hop + step] : 0u) + t;      // the group's first frame
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
        } else if constexpr (KIND == 5) {
            const uint32_t streams = w.units / 2u;
            const uint32_t step = (uint32_t) (s / streams);
            const uint32_t stream = (uint32_t) (s % streams);
            const float* src = static_cast<const float*>(in) + (wave_planar_start(w, stream, step, w.starts ? w.starts[(size_t) stream * w.hop + step] : 0u) + t);
#pragma unroll
            for (uint32_t c = 0; c < 2u; ++c, src += w.pitch_frames) {     // channel c of the group: the same 8 samples of the row pitch_frames floats on
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
        } else {
            float l[8], r[8];
            const bool whole = (rot & 7u) == 0u;                         // (uniform) bin and rot multiples of 8: the group does not wrap
            const uint32_t pos = (t + rot) & (n - 1u);
            if constexpr (KIND == 0) {
                const uint32_t* src = static_cast<const uint32_t*>(in) + s * n;
                uint32_t f[8];
                if (whole) {
                    const glv_wave_u4 a = ld<glv_wave_u4>(src, pos * 4u), b = ld<glv_wave_u4>(src, pos * 4u + 16u);
                    f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w; f[4] = b.x; f[5] = b.y; f[6] = b.z; f[7] = b.w;
                } else {
#pragma unroll
                    for (uint32_t q = 0; q < 8; ++q) f[q] = src[(t + q + rot) & (n - 1u)];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const int a = (int16_t) (f[q] & 0xffffu), b = (int16_t) (f[q] >> 16);
                    if (mono) { l[q] = unpack_s16_mono(a, b); r[q] = l[q]; } else { l[q] = unpack_s16(a); r[q] = unpack_s16(b); }
                }
            } else {
                const cf* src = static_cast<const cf*>(in) + s * n;
                cf f[8];
                if (whole) {
#pragma unroll
                    for (uint32_t q = 0; q < 4; ++q) {
                        const BarW4 a = ld<BarW4>(src, pos * 8u + q * 16u);
                        f[2 * q] = cf{a.w[0], a.w[1]}; f[2 * q + 1] = cf{a.w[2], a.w[3]};
                    }
                } else {
#pragma unroll
                    for (uint32_t q = 0; q < 8; ++q) f[q] = src[(t + q + rot) & (n - 1u)];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    if (mono) { l[q] = (f[q].x + f[q].y) / 2; r[q] = l[q]; } else { l[q] = f[q].x; r[q] = f[q].y; }     // pulse_input.c:167
                }
            }
            emit(2 * s, t, l);
            emit(2 * s + 1, t, r);
        }
    }
}

// ---- rd_update prelude (glava/render.c:1765-1809) ------------------------------------------------
// bufscale: mean of k consecutive samples, float accumulation in index order, one float division
__global__ void __launch_bounds__(256) glv_bufscale_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                           size_t total_out, uint32_t k) {
    const float fk = (float) k;
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < total_out; i += (size_t) gridDim.x * blockDim.x) {
        float accum = 0.0f;
        for (uint32_t a = 0; a < k; ++a) accum = accum + in[i * k + a];     // rows are n_out*k long: i*k stays inside the row
        out[i] = accum / fk;
    }
}
// keyframe interpolation: s + (e - s) * mod, mod = min(uratio * kcounter, 1) computed on the host
__global__ void __launch_bounds__(256) glv_lerp_kernel(const float* __restrict__ s0, const float* __restrict__ e0,
                                                       float* __restrict__ out, size_t total, float mod) {
    for (size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t) gridDim.x * blockDim.x) {
        const float d = e0[i] - s0[i];
        const float p = d * mod;
        out[i] = s0[i] + p;
    }
}

// ---- CPU-path transform_smooth (glava/render.c:694-718) --------------------------------------------
// In place and sequentially dependent inside a row (output t reads inputs that earlier outputs already
// replaced), so one lane walks one row; rows are independent.  smin/smax depend only on t and come from
// the host (powf/log/floor/ceil of the reference's libm, glv_tables.h).
//
// The walk only ever touches the first `reach` floats of a row (reach = max smax + 1, about 1.01 n / smooth_ratio) and
// writes the first `asz`.  A workgroup (one wave) therefore stages that prefix of R rows in LDS with coalesced loads --
// row j at float offset j * stride, stride odd, so the 64 lanes' accesses to the same index of their own rows fall in
// different banks --, lanes 0..R-1 walk their rows there (every tap an LDS read instead of a strided global one: round 2
// measured 29 ms for 131 072 rows of N=4096 with the walk in global memory, every lane on its own cache line), and the
// first asz floats of each row go back coalesced.  R = as many rows as fit the workgroup's LDS (host: launch_smooth).
__global__ void __launch_bounds__(64) glv_smooth_kernel(float* __restrict__ rows, size_t nrows, uint32_t n,
                                                        const int* __restrict__ smin, const int* __restrict__ smax, uint32_t asz,
                                                        uint32_t reach, uint32_t rows_per_wg) {
    extern __shared__ float smooth_lds[];
    const uint32_t stride = reach | 1u;
    const uint32_t lane = threadIdx.x;
    const size_t row0 = (size_t) blockIdx.x * rows_per_wg;
    if (row0 >= nrows) return;
    const uint32_t R = (uint32_t) (nrows - row0 < rows_per_wg ? nrows - row0 : rows_per_wg);
    // staging: eight loads of a lane in flight before the first is parked in LDS (one at a time, every 256-byte piece
    // of a row was its own exposed HBM round trip)
    for (uint32_t j = 0; j < R; ++j) {
        const float* src = rows + (row0 + j) * n;
        float* dst = smooth_lds + (size_t) j * stride;
        for (uint32_t i0 = lane; i0 < reach; i0 += 64 * 8) {
            float tmp[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) tmp[k] = i0 + 64u * k < reach ? src[i0 + 64u * k] : 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) if (i0 + 64u * k < reach) dst[i0 + 64u * k] = tmp[k];
        }
    }
    __syncthreads();
    if (lane < R) {
        float* b = smooth_lds + (size_t) lane * stride;
        // the bounds of eight steps are fetched together (uniform: scalar loads) -- one memory round trip per eight
        // outputs instead of two per output, which is what a step of the first LDS version waited for
        for (uint32_t t0 = 0; t0 < asz; t0 += 8) {
            int lo[8], hi[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t t = t0 + k < asz ? t0 + k : asz - 1;
                lo[k] = smin[t]; hi[k] = smax[t];
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                if (t0 + k >= asz) break;
                float avg = 0.0f;
                int count = 0;
                const int q1 = hi[k];
                // eight taps per trip, read together; taps past smax read as 0, which the reference's `if (b[s])` skips anyway
                for (int q0 = lo[k]; q0 <= q1; q0 += 8) {
                    float x[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) x[i] = q0 + i <= q1 ? b[q0 + i] : 0.0f;
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (x[i] != 0.0f) { avg = avg + x[i]; ++count; }   // `if (b[s])`: NaN counts, +-0 does not
                }
                b[t0 + k] = avg / (float) count;                    // 0/0 = NaN at t = 0, as in the reference
            }
        }
    }
    __syncthreads();
    for (uint32_t j = 0; j < R; ++j) {
        float* dst = rows + (row0 + j) * n;
        const float* src = smooth_lds + (size_t) j * stride;
        for (uint32_t i = lane; i < asz; i += 64) dst[i] = src[i];
    }
}

// The same walk for many rows at once: a wave takes 64 rows, one per lane, and keeps only a sliding window of each in LDS
// -- a ring of W floats per lane (position q lives in slot q mod W; lane stride W + 1, odd: the lanes' accesses to the
// same slot of their own rows hit different banks).  Inputs enter in chunks of kSmoothChunk positions (coalesced: half a
// wave reads one row's chunk), finished outputs leave in chunks of the same size, the walk in between reads and writes
// LDS only.  W >= (largest window) + 2 chunks: a slot is reused for position p + W only after p has left every later
// window (smin is monotone) and, being a finished output, has been written back.  33 KiB of LDS per wave at W = 128
// (the defaults at N=4096: largest window 23 taps) instead of one 4 KiB row prefix per lane: 4 waves = 256 rows in
// flight per CU against 30, which is what a latency-bound dependent walk needs.
constexpr uint32_t kSmoothChunk = 32;
template <uint32_t W>
__global__ void __launch_bounds__(64) glv_smooth_ring_kernel(float* __restrict__ rows, size_t nrows, uint32_t n,
                                                             const int* __restrict__ smin, const int* __restrict__ smax, uint32_t asz,
                                                             uint32_t reach) {
    extern __shared__ float smooth_lds[];
    constexpr uint32_t LS = W + 1;                         // lane stride (floats)
    constexpr uint32_t CH = kSmoothChunk;
    const uint32_t lane = threadIdx.x;
    const size_t row0 = (size_t) blockIdx.x * 64;
    if (row0 >= nrows) return;
    const uint32_t R = (uint32_t) (nrows - row0 < 64 ? nrows - row0 : 64);
    const uint32_t sub = lane & (CH - 1), half = lane / CH;           // two rows per load / store instruction
    uint32_t loaded = 0, written = 0;
    // positions [c0, c1) (c1 - c0 <= CH) of every row: HBM -> ring, eight row pairs in flight
    auto load_chunk = [&](uint32_t c0, uint32_t c1) {
        const uint32_t pos = c0 + sub;
        for (uint32_t j0 = 0; j0 < R; j0 += 16) {
            float tmp[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t j = j0 + 2u * k + half;
                tmp[k] = (j < R && pos < c1) ? rows[(row0 + j) * n + pos] : 0.0f;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t j = j0 + 2u * k + half;
                if (j < R && pos < c1) smooth_lds[j * LS + (pos & (W - 1))] = tmp[k];
            }
        }
    };
    // finished outputs [c0, c1) of every row: ring -> HBM
    auto store_chunk = [&](uint32_t c0, uint32_t c1) {
        const uint32_t pos = c0 + sub;
        for (uint32_t j0 = 0; j0 < R; j0 += 2) {
            const uint32_t j = j0 + half;
            if (j < R && pos < c1) rows[(row0 + j) * n + pos] = smooth_lds[j * LS + (pos & (W - 1))];
        }
    };
    auto wave_sync = [&]() {                               // the workgroup is one wave: LDS is in order, the compiler must be too
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
    };
    float* b = smooth_lds + (size_t) lane * LS;
    for (uint32_t t0 = 0; t0 < asz; t0 += 8) {
        int lo[8], hi[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t t = t0 + k < asz ? t0 + k : asz - 1;
            lo[k] = smin[t]; hi[k] = smax[t];
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t t = t0 + k;
            if (t >= asz) break;
            // outputs that are complete chunks leave first (they also free the slots the next inputs take)
            while (t - written >= CH) { wave_sync(); store_chunk(written, written + CH); written += CH; }
            // inputs up to this step's last tap
            // ... and up to t itself: the output takes position t's slot, which no later chunk may then overwrite
            uint32_t need = hi[k] + 1 > (int) t + 1 ? (uint32_t) (hi[k] + 1) : t + 1;
            need = need < reach ? need : reach;
            while (loaded < need) {
                const uint32_t c1 = loaded + CH < reach ? loaded + CH : reach;
                wave_sync();
                load_chunk(loaded, c1);
                loaded = c1;
            }
            wave_sync();
            if (lane < R) {
                float avg = 0.0f;
                int count = 0;
                const int q1 = hi[k];
                for (int q0 = lo[k]; q0 <= q1; q0 += 8) {
                    float x[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) x[i] = q0 + i <= q1 ? b[(uint32_t) (q0 + i) & (W - 1)] : 0.0f;
#pragma unroll
                    for (int i = 0; i < 8; ++i)
                        if (x[i] != 0.0f) { avg = avg + x[i]; ++count; }   // `if (b[s])`: NaN counts, +-0 does not
                }
                b[t & (W - 1)] = avg / (float) count;                   // 0/0 = NaN at t = 0, as in the reference
            }
        }
    }
    wave_sync();
    while (written < asz) { const uint32_t c1 = written + CH < asz ? written + CH : asz; store_chunk(written, c1); written = c1; }
}

// the s16 window as float pairs: glv_winsplit.h (shared with the knob-sweep harness glv_tune.hip)
hipError_t launch_window_split(const double* w_tab, float* split, uint32_t n, int* d_fail_shifted, hipStream_t st) {
    return launch_window_split_impl(w_tab, split, n, d_fail_shifted, st);
}
hipError_t launch_window_split_check(const double* w_tab, const float* split, uint32_t n, unsigned long long* d_mismatches, hipStream_t st) {
    return launch_window_split_check_impl(w_tab, split, n, d_mismatches, st);
}

// one 256-thread workgroup per 256 items, grid-stride beyond the cap; at least one
static unsigned grid_256(size_t items) {
    const unsigned g = capped_grid(items, 256, kGridCap);
    return g ? g : 1u;
}

hipError_t launch_post(const FrameArgs& a, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(glv_post_kernel, dim3(grid_256((size_t) a.units * (n / 2))), dim3(256), 0, st, a, n);
    return hipGetLastError();
}

hipError_t launch_track_scan(const FrameArgs& a, const TrackGeometry& t, bool rows_texels, hipStream_t st) {
    const uint64_t blocks = (uint64_t) a.units * ((t.kept + 2u * (uint32_t) kTrackLanes - 1u) / (2u * (uint32_t) kTrackLanes));
    if (t.n < 2u * (uint32_t) kTrackLanes || t.kept == 0 || t.kept > t.n || t.kept % 64u != 0 || t.steps == 0 || blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    const size_t lds = (a.ops & OP_AVERAGE) ? (size_t) a.F * kTrackLanes * (rows_texels ? sizeof(uint32_t) : sizeof(cf)) : 0;   // <= 32 KiB (F <= 64)
    if (t.ur) {                                                             // the rates kind: a table without gravity has no reader
        if (!(a.ops & OP_GRAVITY)) return hipErrorInvalidValue;
        if (rows_texels) hipLaunchKernelGGL((glv_track_scan_kernel<true, true>), dim3((uint32_t) blocks), dim3(kTrackLanes), lds, st, a, t);
        else hipLaunchKernelGGL((glv_track_scan_kernel<false, true>), dim3((uint32_t) blocks), dim3(kTrackLanes), lds, st, a, t);
        return hipGetLastError();
    }
    if (rows_texels) hipLaunchKernelGGL((glv_track_scan_kernel<true>), dim3((uint32_t) blocks), dim3(kTrackLanes), lds, st, a, t);
    else hipLaunchKernelGGL((glv_track_scan_kernel<false>), dim3((uint32_t) blocks), dim3(kTrackLanes), lds, st, a, t);
    return hipGetLastError();
}

hipError_t launch_track_each_scan(const FrameArgs& a, const TrackGeometry& t, const TrackEach& e, bool rows_texels, hipStream_t st) {
    const uint64_t blocks = (uint64_t) a.units * ((t.kept + 2u * (uint32_t) kTrackLanes - 1u) / (2u * (uint32_t) kTrackLanes));
    if (t.n < 2u * (uint32_t) kTrackLanes || t.kept == 0 || t.kept > t.n || t.kept % 64u != 0 || t.steps == 0 || blocks == 0 || blocks > 0x7fffffffull) return hipErrorInvalidValue;
    if (t.log_q != 0 || t.hops_per_pitch != t.steps || t.ur || (a.units & 1u)) return hipErrorInvalidValue;      // the windows form's rows; the rates are TrackEach's
    if (!(a.ops & (OP_GRAVITY | OP_AVERAGE)) || (e.ur && !(a.ops & OP_GRAVITY))) return hipErrorInvalidValue;     // counts protect state, rates are gravity's
    const size_t lds = (a.ops & OP_AVERAGE) ? (size_t) a.F * kTrackLanes * (rows_texels ? sizeof(uint32_t) : sizeof(cf)) : 0;   // <= 32 KiB (F <= 64)
    if (e.ur) {
        if (rows_texels) hipLaunchKernelGGL((glv_track_each_scan_kernel<true, true>), dim3((uint32_t) blocks), dim3(kTrackLanes), lds, st, a, t, e);
        else hipLaunchKernelGGL((glv_track_each_scan_kernel<false, true>), dim3((uint32_t) blocks), dim3(kTrackLanes), lds, st, a, t, e);
        return hipGetLastError();
    }
    if (rows_texels) hipLaunchKernelGGL((glv_track_each_scan_kernel<true, false>), dim3((uint32_t) blocks), dim3(kTrackLanes), lds, st, a, t, e);
    else hipLaunchKernelGGL((glv_track_each_scan_kernel<false, false>), dim3((uint32_t) blocks), dim3(kTrackLanes), lds, st, a, t, e);
    return hipGetLastError();
}

hipError_t launch_unpack(const int16_t* pcm, size_t frames, int mono, float* l, float* r, hipStream_t st) {
    hipLaunchKernelGGL(glv_unpack_kernel, dim3(grid_256(frames)), dim3(256), 0, st, pcm, frames, mono, l, r);
    return hipGetLastError();
}

hipError_t launch_ring_planar(const void* ring, int is_f32, uint32_t n, uint32_t rot, int mono, size_t streams, float* out, hipStream_t st) {
    hipLaunchKernelGGL(glv_ring_planar_kernel, dim3(grid_256(streams * n)), dim3(256), 0, st, ring, is_f32, n, rot, mono, streams, out);
    return hipGetLastError();
}

hipError_t launch_wave(const void* in, int in_mode, bool mono, uint32_t n, uint32_t rot, size_t units, void* out, bool r16, uint32_t limit, hipStream_t st) {
    if (limit == 0 || limit > n || (limit & 7u) || rot >= n) return hipErrorInvalidValue;
    const bool planar = in_mode == IN_F32_PLANAR;
    if (!planar && (units & 1u)) return hipErrorInvalidValue;           // interleaved frames: whole streams
    const size_t total = (planar ? units : units / 2) * (limit / 8u);
    if (total == 0) return hipSuccess;
    const unsigned grid = grid_256(total);
    const int m = mono ? 1 : 0;
#define GLV_WAVE_LAUNCH(KIND) \
    do { if (r16) hipLaunchKernelGGL((glv_wave_kernel<KIND, true>), dim3(grid), dim3(256), 0, st, in, out, total, n, limit, rot, m, WaveWindows()); \
         else hipLaunchKernelGGL((glv_wave_kernel<KIND, false>), dim3(grid), dim3(256), 0, st, in, out, total, n, limit, rot, m, WaveWindows()); } while (0)
    if (planar) GLV_WAVE_LAUNCH(2);
    else if (in_mode == IN_S16_STEREO || in_mode == IN_S16_RING) GLV_WAVE_LAUNCH(0);
    else GLV_WAVE_LAUNCH(1);
#undef GLV_WAVE_LAUNCH
    return hipGetLastError();
}
hipError_t launch_wave_track(const void* pcm, bool f32, const WaveWindows& w, bool mono, uint32_t n, void* out, bool r16, uint32_t limit, hipStream_t st) {
    if (limit == 0 || limit > n || (limit & 7u) || w.units == 0 || (w.units & 1u) || w.steps == 0 || (w.hop == 0 && !w.starts)) return hipErrorInvalidValue;
    if (w.starts && w.hop != 0 && w.hop != w.steps) return hipErrorInvalidValue;      // a table: one shared row (0), or uint32 [streams][steps] (steps), nothing else
    const size_t total = (size_t) w.steps * (w.units / 2u) * (limit / 8u);
    const unsigned grid = grid_256(total);
    if (w.planar) {
        if (!f32 || !w.starts) return hipErrorInvalidValue;      // (planar float rows, a table call's only)
        if (r16) hipLaunchKernelGGL((glv_wave_kernel<5, true>), dim3(grid), dim3(256), 0, st, pcm, out, total, n, limit, 0u, 0, w);
        else hipLaunchKernelGGL((glv_wave_kernel<5, false>), dim3(grid), dim3(256), 0, st, pcm, out, total, n, limit, 0u, 0, w);
        return hipGetLastError();
    }
    if (f32) {
        if (r16) hipLaunchKernelGGL((glv_wave_kernel<4, true>), dim3(grid), dim3(256), 0, st, pcm, out, total, n, limit, 0u, mono ? 1 : 0, w);
        else hipLaunchKernelGGL((glv_wave_kernel<4, false>), dim3(grid), dim3(256), 0, st, pcm, out, total, n, limit, 0u, mono ? 1 : 0, w);
        return hipGetLastError();
    }
    if (r16) hipLaunchKernelGGL((glv_wave_kernel<3, true>), dim3(grid), dim3(256), 0, st, pcm, out, total, n, limit, 0u, mono ? 1 : 0, w);
    else hipLaunchKernelGGL((glv_wave_kernel<3, false>), dim3(grid), dim3(256), 0, st, pcm, out, total, n, limit, 0u, mono ? 1 : 0, w);
    return hipGetLastError();
}
hipError_t launch_bufscale(const float* in, float* out, size_t total_out, uint32_t k, hipStream_t st) {
    hipLaunchKernelGGL(glv_bufscale_kernel, dim3(grid_256(total_out)), dim3(256), 0, st, in, out, total_out, k);
    return hipGetLastError();
}
hipError_t launch_lerp(const float* s0, const float* e0, float* out, size_t total, float mod, hipStream_t st) {
    hipLaunchKernelGGL(glv_lerp_kernel, dim3(grid_256(total)), dim3(256), 0, st, s0, e0, out, total, mod);
    return hipGetLastError();
}
hipError_t launch_smooth(float* rows, size_t nrows, uint32_t n, const int* smin, const int* smax, uint32_t asz, uint32_t reach,
                         uint32_t max_window, hipStream_t st) {
    // (the dynamic-LDS opt-in is set per call, not through lds_opt_in: the bytes follow the call's arguments)
    // ring kernel: 64 rows per wave, W >= largest window + 2 chunks (glv_smooth_ring_kernel); few rows or huge windows:
    // the row-prefix kernel
    const uint32_t need_w = max_window + 2 * kSmoothChunk;
    if (nrows >= 64 && need_w <= 512) {
        const unsigned wgs = (unsigned) ((nrows + 63) / 64);
#define GLV_RING(WW)                                                                                                           \
        do {                                                                                                                   \
            const size_t lds = sizeof(float) * 64 * (WW + 1);                                                                  \
            if (lds > 64 * 1024) {                                                                                             \
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(glv_smooth_ring_kernel<WW>),                  \
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);                     \
                if (e != hipSuccess) return e;                                                                                 \
            }                                                                                                                  \
            hipLaunchKernelGGL(glv_smooth_ring_kernel<WW>, dim3(wgs), dim3(64), lds, st, rows, nrows, n, smin, smax, asz, reach); \
            return hipGetLastError();                                                                                          \
        } while (0)
        if (need_w <= 128) GLV_RING(128);
        if (need_w <= 256) GLV_RING(256);
        GLV_RING(512);
#undef GLV_RING
    }
    // rows per workgroup: what fits 64 KiB of LDS (two workgroups per CU), at most one row per lane, at least one
    // (reach <= n <= 32768 floats = 128 KiB: a row always fits the 160 KiB of a CU once the limit is raised)
    const size_t row_bytes = sizeof(float) * (size_t) (reach | 1u);
    size_t budget = 64 * 1024;
    if (row_bytes > budget) {
        budget = row_bytes;
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(glv_smooth_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int) budget);
        if (e != hipSuccess) return e;
    }
    size_t rpw = budget / row_bytes;
    if (rpw > 64) rpw = 64;
    const size_t wgs = (nrows + rpw - 1) / rpw;
    hipLaunchKernelGGL(glv_smooth_kernel, dim3((unsigned) wgs), dim3(64), rpw * row_bytes, st, rows, nrows, n, smin, smax, asz, reach, (uint32_t) rpw);
    return hipGetLastError();
}

#define GLV_BY_SIZE(log_nn, CALL, DEFAULT)                                                                            \
    switch (log_nn) {                                                                                                   \
        case 7: return CALL(7); case 8: return CALL(8); case 9: return CALL(9); case 10: return CALL(10);               \
        case 11: return CALL(11); case 12: return CALL(12); case 13: return CALL(13); case 14: return CALL(14);         \
    }                                                                                                                   \
    return DEFAULT

hipError_t launch_frame(int log_nn, int in_mode, int log_mode, int variant, FrameClass cls, const FrameArgs& a, int grid, hipStream_t st) {
#define GLV_CALL(K) launch_frame_##K(in_mode, log_mode, variant, cls, a, grid, st)
    GLV_BY_SIZE(log_nn, GLV_CALL, hipErrorInvalidValue);
#undef GLV_CALL
}
int frame_variants(int log_nn) {
#define GLV_CALL(K) frame_variants_##K()
    GLV_BY_SIZE(log_nn, GLV_CALL, 1);
#undef GLV_CALL
}
bool frame_variant_ok(int log_nn, int in_mode, int log_mode, int variant) {
#define GLV_CALL(K) frame_variant_ok_##K(in_mode, log_mode, variant) != 0
    GLV_BY_SIZE(log_nn, GLV_CALL, false);
#undef GLV_CALL
}
FrameGeometry frame_geometry(int log_nn, int variant) {
#define GLV_CALL(K) frame_geometry_##K(variant)
    GLV_BY_SIZE(log_nn, GLV_CALL, FrameGeometry{});
#undef GLV_CALL
}
#undef GLV_BY_SIZE

}  // namespace glv
