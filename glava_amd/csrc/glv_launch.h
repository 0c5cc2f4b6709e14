// glv_launch.h -- host-visible launch entry points of the kernel translation units.
#pragma once

#include <hip/hip_runtime.h>

#include "glv_frame.h"

namespace glv {

// what the host needs to know about one kernel configuration of one size (glv_inst.hip Tuned<K, V>)
struct FrameGeometry {
    int lanes;          // lanes cooperating on one row
    int resident;       // workgroups that fit one CU
    int rounds;         // rounds of resident workgroups a large launch is cut into
    int rows_per_trip;  // channel rows one workgroup takes per trip of its persistent loop
    int bar_batch;      // steps per batch of the fused GLV_OP_BARS loop: its work lists are padded to multiples of this
    int lds_bytes, log_e, slots, twreg, winlds;   // for diagnostics / the wisdom file's comments
    int nbuf;           // exchange regions per row (0: split exchange -- no room to park a finished row: bars are a second launch)
    int live_points;    // complex points [0, live_points) of a row are what the GLV_OP_BARS_ONLY kernel class of this configuration keeps alive (a compile-time
                        // share of the last pass's blocks, glv_frame.h LIVE_RBLOCKS): the host takes that class only when the bars sample nothing beyond
};

// per-size production launchers, one translation unit each (glv_inst.hip -DGLV_LOG_NN=k)
#define GLV_DECL_INST(K) \
    hipError_t launch_frame_##K(int in_mode, int log_mode, int variant, FrameClass cls, const FrameArgs& a, int grid, hipStream_t st); \
    int frame_variants_##K(); \
    int frame_variant_ok_##K(int in_mode, int log_mode, int variant); \
    FrameGeometry frame_geometry_##K(int variant);
GLV_DECL_INST(7) GLV_DECL_INST(8) GLV_DECL_INST(9) GLV_DECL_INST(10) GLV_DECL_INST(11) GLV_DECL_INST(12) GLV_DECL_INST(13) GLV_DECL_INST(14)
#undef GLV_DECL_INST

// glv_misc.hip (the bars launchers below: glv_bars.hip)
hipError_t launch_frame(int log_nn, int in_mode, int log_mode, int variant, FrameClass cls, const FrameArgs& a, int grid, hipStream_t st);
int frame_variants(int log_nn);                                        // kernel configurations built for this size (>= 1)
bool frame_variant_ok(int log_nn, int in_mode, int log_mode, int variant);   // is `variant` built for this input / log mode
FrameGeometry frame_geometry(int log_nn, int variant);
hipError_t launch_post(const FrameArgs& a, uint32_t n, hipStream_t st);
// the scan over time of a track call (glv_track_scan_kernel): a.in = the residue launches' rows, a.units = channel rows of one update, a.out = the
// results step-major ([steps][units][n]), state pointers / head / weights as for launch_post.  Where window t of stream s lies among the rows:
struct TrackGeometry {
    uint32_t n, steps;
    uint32_t hops_per_pitch;   // pitch_frames / hop: window t of stream s starts at hop (s * hops_per_pitch + t) frames = h hops
    uint32_t log_q;            // log2(n / hop): the window is row h >> log_q of residue launch h & (n / hop - 1)
    uint32_t residue_rows;     // channel rows between the first rows of two residue launches
    uint32_t out_texels;       // results as GL_R16 texels (uint16 rows) instead of floats
    uint32_t kept;             // bins [0, kept) of every row are walked, loaded and stored, state included: n, or a live track call's kept bins (a multiple of 64)
    float gravity_step;        // a rates call (glv_batch_track_rates_s16 / _f32): step t applies gravity with gravity_step * (1.0F / ur[t]), render.c:728 evaluated in the
    const float* ur;           //   kernel's rates kind -- float [steps] in device memory, read in [0, steps) only; nullptr: every other call, FrameArgs::g / grav_sub as they are
};
hipError_t launch_track_scan(const FrameArgs& a, const TrackGeometry& t, bool rows_texels, hipStream_t st);
// The scan of a per-stream track call (glv_track_each_scan_kernel; glv_batch_track_each_*): the windows form's geometry (log_q = 0, hops_per_pitch = steps) with a
// row of the rate table and a count of steps per stream.  Stream s = channel row >> 1 walks its first c_s = min(counts[s], steps) steps (counts == nullptr: all) with
// gravity's step from ur[s * steps + t] (ur == nullptr: FrameArgs::g / grav_sub as they are, the packed integer texel step included), writes zeros to the output
// rows of the steps behind c_s, and leaves its ring where the BATCH's head will point: slot p of the stream's own walk is stored to slot (p + steps - c_s) % F.
// Both tables are device memory, read when the kernel runs: counts in [0, streams), ur in [s * steps, s * steps + c_s) only.  TrackGeometry::ur stays null.
struct TrackEach {
    const uint32_t* counts;
    const float* ur;
};
hipError_t launch_track_each_scan(const FrameArgs& a, const TrackGeometry& t, const TrackEach& e, bool rows_texels, hipStream_t st);
// The render frames of a track call on gl_storage 3 (glv_track_frames.hip; glv_batch_track_frames_s16 / _f32).  Keyframe k of the call is block k of `keys`
// (float [2][units][n]) for k < 2 and the finished float rows of step k - 2 in `rows` (float [steps][units][n]) beyond; frame j of row r is the GL_R16 upload
// of keyframe from[j] itself where from[j] == to[j], of s + ((e - s) * mod[j]) of keyframes from[j] and to[j] else (render.c:1806, :2185).  The tables are
// device memory, read in [0, frames) only, every index clamped to steps + 1 in the kernel.  out: uint16 [frames][units][n], rows at pitch n of which bins
// [0, limit) are written (limit a multiple of 4); segment: the frames one lane walks with its keyframes in registers (track_frames_segment: the default).
struct TrackFrames {
    const uint32_t* from; const uint32_t* to; const float* mod;
    const float* keys; const float* rows;
    void* out;
    uint32_t frames, steps, units, n, limit, segment;
};
uint32_t track_frames_segment(uint32_t frames, uint32_t units, uint32_t limit);
hipError_t launch_track_frames(const TrackFrames& t, hipStream_t st);
// ... and the keyframes the next call starts from: keys[0] <- keyframe keep_from, keys[1] <- keyframe keep_to, element by element, both read before either is
// written (the pairs (0, 1), (1, k >= 2) and (k, k') with 2 <= k < k': the host vets them)
hipError_t launch_track_keys(float* keys, const float* rows, uint32_t units, uint32_t n, uint32_t keep_from, uint32_t keep_to, hipStream_t st);
// The render frames of a per-stream frames call (glv_track_frames_each_kernel; glv_batch_track_each_frames_* / glv_batch_track_pool_frames_*): TrackFrames with
// t.from / t.to / t.mod holding a row per stream, [units / 2][frames] -- row s is stream s's -- and t.steps the call's.  Stream s = channel row >> 1 clamps every
// index to c_s + 1, c_s = min(counts[s], steps) (counts == nullptr: steps), walks its first f_s = min(frame_counts[s], frames) frames (nullptr: all) and stores
// zero texels for the rest; no table entry at j >= f_s is read.  All device memory, read when the kernel runs.  A structure of its own: TrackFrames keeps its
// size and offsets, and glv_track_frames_kernel its code.
struct TrackFramesEach {
    TrackFrames t;
    const uint32_t* frame_counts;
    const uint32_t* counts;
};
hipError_t launch_track_frames_each(const TrackFramesEach& e, hipStream_t st);
// ... and its write-back: keys[0] <- keyframe keep[2 s], keys[1] <- keyframe keep[2 s + 1] of stream s, each clamped to c_s + 1 in the kernel (any pair is
// safe: a lane reads and writes element i only)
hipError_t launch_track_keys_each(float* keys, const float* rows, uint32_t units, uint32_t n, uint32_t steps, const uint32_t* counts, const uint32_t* keep, hipStream_t st);
// Where the windows of the track sources of GLV_OP_WAVE lie (glv_wave_kernel, glv_bars_rows_i8_kernel).  A process call's windows lie back to back -- the
// identity geometry, which those kernels' existing kinds have built in and never read from here.  A track call (glv_batch_track_wave_s16) cuts them
// out of [streams][pitch_frames][2] recordings: output row r = t * units + 2 s + c is channel c of the n frames from s * pitch_frames + t * hop on,
// in 64-bit arithmetic.  by_steps (the one-launch form): a workgroup of the bars kernel takes RB consecutive steps of ONE channel row, whose windows
// overlap and meet in L2, instead of RB consecutive rows r.
// A table call (glv_batch_track_at_s16 / _f32, glv_wave_kernel only): `starts` is uint32 [steps] in device memory and window t of every stream begins
// min(starts[t], start_max) frames into its recording, start_max = pitch_frames - n (glv_frame.h TrackWindows: the same table, the same clamp, in the kernel).
// starts == nullptr: t * hop.
// With a table nothing walks at a hop, and `hop` carries the table's own: the entries between the table rows of two streams -- 0: one row shared by all streams;
// `steps`: uint32 [streams][steps], row s is stream s's (glv_batch_track_each_*), and the entry of window (s, t) is starts[s * hop + t] (glv_wave_kernel's window
// kinds 3, 4, 5 only).  The structure keeps its size and every offset, so every kernel that takes one and does not read a table keeps its code.
struct WaveWindows {
    uint32_t units = 0, steps = 0, hop = 0, by_steps = 0;
    uint64_t pitch_frames = 0;
    const uint32_t* starts = nullptr;
    uint32_t start_max = 0, planar = 0;      // planar (the f32 kinds of a table call only): the recordings are float [streams][2][pitch_frames], channel rows apart, taken as they are
};
// (planar: the result counts floats into row 2 s of the recording, whose sibling 2 s + 1 lies pitch_frames floats on -- wave_planar_start)
GLV_HD constexpr uint64_t wave_window_start(const WaveWindows& w, uint32_t s, uint32_t t, uint32_t entry = 0) {
    return (uint64_t) s * w.pitch_frames + (w.starts ? (uint64_t) (entry < w.start_max ? entry : w.start_max) : (uint64_t) t * w.hop);
}
GLV_HD constexpr uint64_t wave_planar_start(const WaveWindows& w, uint32_t s, uint32_t t, uint32_t entry) {
    return wave_window_start(w, s, t, entry) + (uint64_t) s * w.pitch_frames;
}
hipError_t launch_bufscale(const float* in, float* out, size_t total_out, uint32_t k, hipStream_t st);
// `setbufscale k` on the batched layer (glv_decimate.hip; glv_batch_set_bufscale): every window of a call is k * n frames and becomes a pair of planar float rows
// of n samples, out[t] = (x[t k] + ... + x[t k + k - 1]) / (float) k summed from +0.0F in index order (render.c:1765-1790).  Kinds: interleaved s16 frames,
// interleaved float frames (both unpacked as the backend does, `mono`: channels == 1), and a process call's planar rows float [streams][2][k n] (no mix).
// The interleaved kinds cut their windows out of [streams][pitch_frames][2] recordings by TrackWindows' rules with k n in the place of n: window t of stream s
// begins track_window_start(w, s, t, starts[t]) frames in, w.start_max = w.pitch_frames - k n where a table is set, and its rows go to row
// track_window_row(w, s, t) of `out` -- where the transform that reads them as IN_F32_PLANAR writes its own.  A process call: steps 1, hop 0, pitch k n.
// ... and a track call's planar recording float [streams][2][pitch_frames] (no mix either): the interleaved kinds' windows, cut out of rows 2 s and 2 s + 1
enum DecimateKind { DEC_S16 = 0, DEC_F32 = 1, DEC_F32_PLANAR = 2, DEC_F32_PLANAR_TRACK = 3 };
struct Decimate {
    const void* in; float* out;
    uint32_t n, k, mono, pad;
    TrackWindows w;
};
constexpr size_t kDecimateGridCap = 256 * 8;       // 256 CUs x 8 resident 256-lane workgroups; the kernel's loop takes what lies beyond
hipError_t launch_decimate(int kind, const Decimate& d, hipStream_t st);
// A pool call (glv_pool.hip; glv_batch_track_pool_s16 / _f32 / _f32_planar): the three track kinds of the decimation and the three window kinds of the waveform
// kernel over ONE buffer of pool.frames frames, each stream through its span -- window (s, t) begins pool_window_start(spans[s].first, spans[s].frames, entry,
// pool.frames, k n) frames into the pool (glv_frame.h: clamped into the span, and into the pool whatever the span holds), entry = starts[s * steps + t] of per-stream
// rows.  The pool is an argument of its own: Decimate, TrackWindows and WaveWindows keep their size and offsets, and their pitch_frames is the planar kinds' channel
// stride, pool.frames.  Kernels of their own beside glv_decimate_kernel and glv_wave_kernel, which keep their code; the arithmetic is theirs, line by line.
// Refused: a null or misaligned span table, pool.frames below a window, a table that is not a row per stream, DEC_F32_PLANAR (a process call's kind).
hipError_t launch_decimate_pool(int kind, const Decimate& d, const TrackPool& pool, hipStream_t st);
hipError_t launch_wave_track_pool(const void* pool_pcm, bool f32, const WaveWindows& w, const TrackPool& pool, bool mono, uint32_t n, void* out, bool r16, uint32_t limit, hipStream_t st);
// Chosen streams of a batch (glv_slots.hip; glv_batch_reset_streams / _save_streams / _load_streams): zero their state, gather it into blobs in the portable
// form, or scatter blobs back -- one launch each.  A stream's portable bytes are the regions below back to back (`start` = the sum of the stream_bytes before);
// a region is the stream's stream_bytes of one device array, one or two blocks of chan_bytes = mod << log_unit bytes, and portable unit u of a block is array
// unit (u + pos) mod `mod` of that block (pos < mod; units below 16 bytes are a PCM ring's frames).  idx: uint32 [count] in device memory, read when the kernel
// runs, an entry >= streams skipped with its blob; blob: count * bytes bytes, 16-byte aligned (SLOT_ZERO: unused).
enum SlotKind { SLOT_ZERO = 0, SLOT_GATHER = 1, SLOT_SCATTER = 2 };
constexpr int kSlotRegions = 4;
struct SlotRegion {
    char* base;
    uint32_t start, stream_bytes, chan_bytes, log_unit, pos, mod;
};
struct SlotTable {
    SlotRegion r[kSlotRegions];
    const uint32_t* idx; void* blob;
    uint32_t nregions, streams, count, bytes;      // bytes: of one stream's portable form (a multiple of 16)
};
constexpr size_t kSlotsGridCap = 256 * 8;          // 256 CUs x 8 resident 256-lane workgroups of 256 pieces each; the kernel's loop takes what lies beyond
hipError_t launch_slots(int kind, const SlotTable& t, hipStream_t st);
// ... and straight from slot to slot (glv_slot_copy_kernel; glv_batch_copy_streams): stream src.idx[j] of one batch into stream dst.idx[j] of another, or of the same
// one -- two tables of the same regions in the same order, each with its own bases, positions and streams (blob unused), count pairs; a pair with either entry
// >= its side's streams is skipped where it is read.  Tables that differ in a region's start, sizes, unit or ring length are refused, like every malformed one.
hipError_t launch_slot_copy(const SlotTable& src, const SlotTable& dst, hipStream_t st);
// The two copies of a ring track call (glv_ring_track.hip; glv_batch_ring_track_s16 / _f32).  launch_ring_track_stage (glv_ring_stage_kernel) writes every stream's
// ring, oldest frame first, and its updates * new_frames new frames behind it into `stage` -- [streams][pitch] frames of 4 (s16) or 8 (f32) bytes, pitch a multiple of
// 4 and >= n + updates * new_frames, the frames beyond those zeros -- and (t + 1) * new_frames into starts[t], t < updates.  fresh: [streams][updates * new_frames]
// frames, frame aligned; null: zeros.  launch_ring_track_keep (glv_ring_keep_kernel) writes frames [updates * new_frames, updates * new_frames + n) of every staged
// stream back as its ring, oldest frame at 0.  ring and stage 16-byte aligned, n a multiple of 4, pos < n: anything else is refused.
struct RingTrack {
    void* ring; const void* fresh; void* stage; uint32_t* starts;
    uint32_t n, pos, new_frames, updates, pitch, streams;
};
constexpr size_t kRingTrackGridCap = 256 * 8;      // 256 CUs x 8 resident 256-lane workgroups of 256 pieces each; the kernels' loops take what lies beyond
hipError_t launch_ring_track_stage(bool f32, const RingTrack& r, hipStream_t st);
hipError_t launch_ring_track_keep(bool f32, const RingTrack& r, hipStream_t st);
// ... of a per-stream ring track call (glv_ring_each.hip; glv_batch_ring_track_each_s16 / _f32): stream s takes c_s = min(counts[s], updates) of the updates, read
// on the device (counts null: everybody takes all).  launch_ring_each_stage (glv_ring_stage_each_kernel) writes every stream's ring, oldest frame first, and the
// FIRST c_s * new_frames of its new frames behind it into `stage`, zeros beyond them up to the pitch -- `fresh` is [streams][updates * new_frames] frames whatever
// the counts are, and nothing of a stream at or beyond c_s * new_frames is read -- and (t + 1) * new_frames into starts[s * updates + t] for every s < streams,
// t < updates: uint32 [streams][updates], the per-stream table call's rows.  launch_ring_each_keep (glv_ring_keep_each_kernel) writes frames [c_s * new_frames,
// c_s * new_frames + n) of every staged stream back as its ring, oldest frame at 0.  What RingTrack's launchers refuse is refused, and counts off 4 bytes and more
// than 2^32 - 1 table entries.
struct RingTrackEach {
    RingTrack r;
    const uint32_t* counts;
};
hipError_t launch_ring_each_stage(bool f32, const RingTrackEach& e, hipStream_t st);
hipError_t launch_ring_each_keep(bool f32, const RingTrackEach& e, hipStream_t st);
hipError_t launch_lerp(const float* s0, const float* e0, float* out, size_t total, float mod, hipStream_t st);
hipError_t launch_smooth(float* rows, size_t nrows, uint32_t n, const int* smin, const int* smax, uint32_t asz, uint32_t reach,
                         uint32_t max_window, hipStream_t st);
// the s16 window table as float pairs (glv_core.h WinSplit): split = float [n/2][4]; d_fail_shifted = int [2], zeroed by the caller
hipError_t launch_window_split(const double* w_tab, float* split, uint32_t n, int* d_fail_shifted, hipStream_t st);
hipError_t launch_window_split_check(const double* w_tab, const float* split, uint32_t n, unsigned long long* d_mismatches, hipStream_t st);
// The matrix-core kernels of the many-bars pass (glv_bars.hip glv_bars_rows_kernel over float rows, glv_bars_rows_i8_kernel over texel rows): kRowsWaves
// waves per workgroup, one tile of a round each, and the LDS rings (bins) each kernel is built for, smallest first -- the host cuts a table's rounds for the
// first ring that takes them.  (The rows a workgroup takes with each ring: the kernels' dispatchers, which a static_assert holds to these lists.)
constexpr int kRowsWaves = 4;
constexpr uint32_t kRowsRings[] = {160, 288, 448, 832};
constexpr uint32_t kRowsI8Rings[] = {160, 288, 448, 832, 1600};
// rt: the tables of the many-bars kernels (>= 256 bars; glv_tables.h make_bar_mtiles): tiles of 32 bars with their weights, the bars'
// weight sums, and -- when they could be cut -- the rounds of the matrix-core kernel for an LDS ring of ring_bins bins (one of kRowsRings)
// mode != 0 (glv_params.sample_mode maximum / hybrid): the block-transposed weights of glv_bars_mode_kernel (glv_tables.h make_bar_mode_blocks) and the
// bins of a row its bars sample; the other tables are then unused.  rows_texels (mode != 0 only): `spec` is uint16 [nrows][n], GL_R16 texels c -- the kernel's
// texel-row kind takes x = c / 65535 correctly rounded (unorm16_to_float: what texelFetch returns) and walks as over floats
struct BarRowsTables {
    const BarMTile* mtiles; uint32_t ntiles; const float* wt; const float* wsum;
    const BarTile* rounds; uint32_t nrounds, ring_bins;
    uint32_t mode = 0; float hybrid_weight = 0.65f; const BarModeBlock* mblocks = nullptr; uint32_t nmblocks = 0; const float* mw = nullptr; uint32_t mode_bins = 0;
    uint32_t rows_texels = 0;
};
hipError_t launch_bars(const float* spec, float* bars_out, size_t nrows, uint32_t n, uint32_t bars, uint32_t nsteps,
                       const BarItem* items, const BarDesc* desc, const float* tap_w, hipStream_t st, bool r16 = false, const BarRowsTables* rt = nullptr);
hipError_t prepare_bars_rows(uint32_t n, const BarRowsTables* rt);      // function attributes of the kernel launch_bars would pick
// the tables of the i8 matrix-core kernel for texel rows (glv_tables.h make_bar_itiles): tiles (origin a multiple of 16 bins, steps of 32),
// the digit planes of the integer weights in operand layout, per bar the rounding constant and shift, the rounds for a ring of ring_bins bins (one of kRowsI8Rings)
struct BarIRowsTables {
    const BarMTile* tiles; uint32_t ntiles; const void* wq; const BarIFin* fin;
    const BarTile* rounds; uint32_t nrounds, ring_bins;
};
hipError_t launch_bars_i8(const void* rows, bool rows_f32, void* bars_out, size_t nrows, uint32_t n, uint32_t bars, const BarIRowsTables* rt, hipStream_t st, bool r16);
hipError_t prepare_bars_i8(uint32_t n, const BarIRowsTables* rt);     // function attributes of the kernels launch_bars_i8 / launch_bars_i8_pcm would pick
// the same pass straight from interleaved s16 frames (GLV_OP_WAVE | GLV_OP_BARS in one launch): pcm int16 [nrows / 2][n][2], row 2 s + c is channel c of
// stream s; the kernel unpacks, applies wrange and quantises the frames it parks.  rot: index of the oldest frame (the device ring; 0 for frames)
hipError_t launch_bars_i8_pcm(const void* pcm, uint32_t rot, bool mono, void* bars_out, size_t nrows, uint32_t n, uint32_t bars, const BarIRowsTables* rt, hipStream_t st, bool r16);
// GLV_OP_WAVE without bars / the first of its two launches (glv_wave_kernel): unpack -> wrange -> GL_R16 texels (r16) or their floats c / 65535, for the
// first `limit` samples (a multiple of 8) of every row; out rows keep a pitch of n.  in_mode: glv_frame.h InMode; units: channel rows
hipError_t launch_wave(const void* in, int in_mode, bool mono, uint32_t n, uint32_t rot, size_t units, void* out, bool r16, uint32_t limit, hipStream_t st);
// ... and both over every window of a track call (interleaved s16 recordings, any window start): out / bars_out hold w.steps * w.units rows, step-major.
// launch_wave_track with f32: the recordings are interleaved stereo floats, 8 bytes per frame (pcm 8-byte aligned).
// launch_bars_i8_pcm_track needs window starts on groups of 8 frames (pcm 32-byte aligned, hop and pitch multiples of 8) and refuses others (a table call never reaches it: the host cannot know where a table's windows lie)
hipError_t launch_wave_track(const void* pcm, bool f32, const WaveWindows& w, bool mono, uint32_t n, void* out, bool r16, uint32_t limit, hipStream_t st);
hipError_t launch_bars_i8_pcm_track(const void* pcm, const WaveWindows& w, bool mono, void* bars_out, uint32_t n, uint32_t bars, const BarIRowsTables* rt, hipStream_t st,
                                    bool r16);
// The render frames of a wave track call (glv_track_frames.hip; glv_batch_track_wave_frames_s16 / _f32): TrackFrames' tables and arithmetic with the keyframes
// beyond the caller's two read from the recording where they lie.  Keyframe k < 2 is block k of `keys` (float [2][w.units][n]); keyframe 2 + t of row 2 s + c and
// sample i is (u + 1.0F) / 2.0F of the unpack u of frame wave_window_start(w, s, t, w.starts[t]) + i (w.starts is required: a table call's windows), every index
// clamped to w.steps + 1 in the kernel.  out: rows [frames][w.units] at pitch n of which samples [0, limit) are written (limit a multiple of 4) -- the upload's
// texels (r16) or their floats c / 65535; segment: as TrackFrames', with the streams as its rows (a lane owns both channel rows of its four frames).
struct WaveFrames {
    const uint32_t* from; const uint32_t* to; const float* mod;
    float* keys;
    void* out;
    uint32_t frames, n, limit, segment;
};
hipError_t launch_wave_frames(const void* pcm, bool f32, const WaveWindows& w, bool mono, const WaveFrames& t, bool r16, hipStream_t st);
// ... and the keyframes the next call starts from, as floats: keys[0] <- keyframe keep_from, keys[1] <- keyframe keep_to (launch_track_keys' pairs, vetted by the host)
hipError_t launch_wave_keys(const void* pcm, bool f32, const WaveWindows& w, bool mono, float* keys, uint32_t n, uint32_t keep_from, uint32_t keep_to, hipStream_t st);
// The render frames of a per-stream wave frames call (glv_wave_frames_each_kernel; glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_*): WaveFrames
// with t.from / t.to / t.mod holding a row per stream, [w.units / 2][frames], and w.starts a row per stream, uint32 [w.units / 2][w.steps].  Stream s clamps every
// index to c_s + 1, c_s = min(counts[s], w.steps) (counts == nullptr: w.steps), walks its first f_s = min(frame_counts[s], frames) frames (nullptr: all) and stores
// zero texels (or their floats) for the rest; no table entry at j >= f_s is read, and a stream with c_s == 0 reads neither starts, span nor recording.  Keyframe
// 2 + t of stream s is read from the window that begins wave_window_start(w, s, t, starts[s * steps + t]) frames in (w.pitch_frames, w.start_max: the recordings'),
// or with pool.spans set pool_window_start(spans[s].first, spans[s].frames, that entry, pool.frames, n) frames into the ONE buffer `pcm` (w.pitch_frames ==
// pool.frames: the planar kind's channel stride).  kind: 0 s16 frames, 1 interleaved float frames, 2 planar float rows (w.planar set; no mono mix).  All device
// memory, read when the kernel runs.  Structures of their own: WaveFrames and WaveWindows keep their size and offsets, the lockstep kernels their code.
struct WaveFramesEach {
    WaveFrames t;
    const uint32_t* frame_counts;
    const uint32_t* counts;
    TrackPool pool;             // spans == nullptr: a recording per stream
};
hipError_t launch_wave_each_frames(const void* pcm, int kind, const WaveWindows& w, bool mono, const WaveFramesEach& e, bool r16, hipStream_t st);
// ... and its write-back (glv_wave_keys_each_kernel): keys[0] <- keyframe keep[2 s], keys[1] <- keyframe keep[2 s + 1] of stream s, each clamped to c_s + 1 in the
// kernel (any pair is safe: a lane reads and writes its own elements only)
struct WaveKeysEach {
    float* keys;                // float [2][w.units][n]
    uint32_t n;
    const uint32_t* counts;
    const uint32_t* keep;       // uint32 [w.units / 2][2]
    TrackPool pool;
};
hipError_t launch_wave_each_keys(const void* pcm, int kind, const WaveWindows& w, bool mono, const WaveKeysEach& k, hipStream_t st);
// bars at texels of the pre-smoothing pass (glv_batch_set_bar_texels) over texel rows: uint16, or floats c / 65535 (rows_f32); one lane per bar and row
hipError_t launch_bars_snap(const void* rows, bool rows_f32, void* bars_out, size_t nrows, uint32_t n, uint32_t bars, const BarDesc* desc, const uint32_t* wi,
                            hipStream_t st, bool r16);
// columns = means of three texels of the pre-smoothing pass (glv_batch_set_column_texels) over a GL chain's rows as floats c / 65535: ntex distinct texels
// (desc, tap_w: W' as float bits for mode 0 with work lists `items` for 256 / bar_lanes_of(n) groups; float weights in tap order for modes 1 / 2), cols columns
hipError_t launch_columns(const float* rows, float* cols_out, size_t nrows, uint32_t n, uint32_t ntex, uint32_t cols, uint32_t nsteps, const BarItem* items,
                          const BarDesc* desc, const float* tap_w, const ColumnMap* map, uint32_t mode, float hybrid_weight, hipStream_t st);
// ... and over a GL chain's rows as the texels themselves (uint16 [nrows][n]: the scan results of glv_batch_track_columns_s16 / _f32)
hipError_t launch_columns_texels(const uint16_t* rows, float* cols_out, size_t nrows, uint32_t n, uint32_t ntex, uint32_t cols, uint32_t nsteps,
                                 const BarItem* items, const BarDesc* desc, const float* tap_w, const ColumnMap* map, uint32_t mode, float hybrid_weight, hipStream_t st);
hipError_t launch_ring_planar(const void* ring, int is_f32, uint32_t n, uint32_t rot, int mono, size_t streams, float* out, hipStream_t st);
hipError_t launch_unpack(const int16_t* pcm, size_t frames, int mono, float* l, float* r, hipStream_t st);

}  // namespace glv
