// glv_track.cpp -- track mode: every update of a recording in one call.  The plans of the five entries, the executor of the FFT forms with its
// stages, the wave module's form, and the C entries with their sizing queries.
#include "glv_host.h"
#include "glv_tables.h"       // kBarSeqMin

namespace {
// ---- track mode: `steps` consecutive updates of every stream from one long buffer (glv_batch_track_s16, glv_batch_track_windows_s16 / _f32) -----
// One executor (`track`) carries out a TrackPlan in three stages, kernels only.  (1) The transform, with the stateless frame kernels as they are, in
// one of two forms.  Residues (plan_track: hop a power of two, track_residues): the whole [streams * pitch] frame sequence is cut into
// back-to-back windows of n frames q = n / hop times, launch r starting r * hop frames in -- window t of stream s, which starts at a multiple h of
// hop, is row h / q of launch h % q.  Windows (plan_track_windows: any hop, track_windows): ONE launch in the kernel's IN_S16_TRACK mode -- IN_F32_TRACK
// for a float recording (TrackPlan::f32, the one thing the float entry adds: every stage after the transform sees rows, not samples) -- over
// the steps * streams windows the call names, each read where it lies (glv_frame.h TrackWindows) -- rows step-major straight into d_out (a stateless
// chain without bars: nothing else runs), step-major into the workspace (stateless with bars), or stream-major into the workspace for the scan, whose
// geometry with one residue (log_q = 0) and hops_per_pitch = steps IS [stream][step][channel].  Either way the rows are texels where the chain's
// first act is the GL_R16 upload.  (2) glv_track_scan_kernel (track_scan) walks the steps per bin with the state on chip and writes every
// step's result -- into d_out, or with GLV_OP_BARS into the workspace's second region in the row format the bars kernel takes.  (3) The bars of a
// second launch over steps * streams * 2 finished rows -- or, for a batch with column texels set (plan_track_columns: the windows form, a GL chain), the
// graph module's columns: glv_columns_kernel's texel-row kind over the scan's texels.
// A GLV_OP_BARS_ONLY batch (plan_track_live: the windows form, bars or columns as the batch has them) keeps TrackPlan::kept bins of every row from the
// scan on: the transform finishes whole rows (live classes for it were built and measured level with the full-row ones at 64 streams,
// profiles/r15/track_live_rule.txt, and taken out again), the scan walks the kept bins (TrackGeometry::kept), the bars and columns kernels never read
// beyond them -- the rest of every row of the workspace's second region is not written.
// A table call (glv_batch_track_at_s16 / _f32, plan_track_at: TrackPlan::at) is whichever of the windows, columns and live forms the batch takes, with the
// windows where a table in device memory says: the transform runs in the kernel kinds that read it (IN_S16_TRACK_AT / IN_F32_TRACK_AT), nothing else differs.
// A rates call (glv_batch_track_rates_s16 / _f32, track_rates: TrackPlan::ur) is a table call whose scan runs in the kernel's rates kind: gravity's step of
// update t comes from a second table in device memory, gravity_step * (1.0F / ur[t]) -- the plan, the workspace, the launches and the batch's own ur are the table call's.
// A batch with bufscale k > 1 (glv_batch_set_bufscale) runs the windows form and everything built on it with windows of k * n frames: stage (1) is then two launches --
// glv_decimate_kernel writes every window's decimated rows, steps * streams * 2 rows of n floats, into a region in FRONT of the workspace's others (TrackPlan::dec_bytes),
// each at the row index the transform's result takes, and the stateless transform runs once over them as IN_F32_PLANAR -- and the stages behind it see no difference.
// The residue form (whose trick rests on back-to-back windows of n frames) and the wave forms refuse such a batch.
// What a recording holds, the one thing an entry adds to its plan: s16 frames, interleaved stereo float frames, or planar float rows float [streams][2][pitch_frames]
// (the _f32_planar entries: table calls only).  True where it holds floats, so `f32 ? ... : ...` reads as it did while this was a boolean; a bool converts.
struct TrackInput {
    enum Kind { S16 = 0, F32 = 1, F32_PLANAR = 2 } kind;
    bool rows = false;      // the call's tables have a row per stream (glv_batch_track_each_*: set by track_each, read where the wave form's windows are laid out)
    const glv_track_frames_each* frames = nullptr;      // a per-stream frames call (glv_batch_track_each_frames_* / _pool_frames_*: set by track_each_frames_call; the wave module's: by track_each_wave_frames_call): its render frames, read by track_at, or by track_wave
    const uint32_t* counts = nullptr;      // ... of the wave form (glv_batch_track_each_wave_frames_* / _pool_wave_frames_*): its steps per stream, uint32 [streams] or none (set by track_each)
    glv::TrackPool pool = {nullptr, 0};      // a pool call (glv_batch_track_pool_*: set by track_pool): d_pcm is ONE buffer of pool.frames frames, stream s reads it through pool.spans[s]
    TrackInput(bool f32 = false) : kind(f32 ? F32 : S16) {}
    TrackInput(Kind k) : kind(k) {}
    explicit operator bool() const { return kind != S16; }
    bool planar() const { return kind == F32_PLANAR; }
};
struct TrackPlan {
    uint32_t q = 0, log_q = 0;          // residue launches
    uint64_t frames = 0;                // frames of the sequence the windows cover: the last window of the last stream ends here
    uint64_t k0 = 0;                    // windows of launch 0 (launch r: (frames - r * hop) / n, k0 or k0 - 1)
    bool windows = false;               // stage (1) is the one launch over the windows where they lie, else the q residue launches
    TrackInput f32;                     // the recording is interleaved stereo f32 (8 bytes per frame) or planar f32 rows (f32.planar()), else s16; set by the entry, windows form only
    bool to_out = false;                // stage (1) writes d_out and nothing else runs, else it writes the start of the workspace
    bool scan = false;                  // stage (2) runs: the chain keeps state, or stage (1) left residues (which only the scan puts in step order)
    uint32_t hops_per_pitch = 0, residue_rows = 0;   // TrackGeometry, with log_q: where the scan finds window t of stream s among stage (1)'s rows
    bool state = false;                 // the chain keeps gravity / average state
    bool in16 = false;                  // the transform's rows are GL_R16 texels (kernel class FC_R16), else floats (FC_PLAIN)
    bool out16 = false;                 // the scan's results are texels
    ChainPlan::Bars bars = ChainPlan::NO_BARS;
    uint64_t rows_bytes = 0, work_bytes = 0;   // the transform's region of the workspace (a multiple of 256 bytes), and all of it
    uint64_t out_rows = 0;              // steps * streams * 2
    bool at = false;                    // the windows lie where a table in device memory says (glv_batch_track_at_s16 / _f32), not every `hop` frames; set before the plan
    const uint32_t* starts = nullptr;   // ... and the table, uint32 [steps]; set by the entry as f32 is (the sizing query has none), windows form only
    const float* ur = nullptr;          // a rates call's table of update rates, float [steps]; set by track_at as starts is, read by the scan alone
    bool each = false;                  // a per-stream call (glv_batch_track_each_*): `starts` and `ur` are [streams][steps], row s is stream s's; set by track_at with them
    const uint32_t* counts = nullptr;   // ... and its steps per stream, uint32 [streams] or none; read by the scan alone, on the device
    bool live = false;                  // the entry is the live form (glv_batch_track_live_s16 / _f32)
    uint32_t kept = 0;                  // the live form's kept bins K, a multiple of 64 below n (kept_bins); 0: every bin -- the other entries, and the live form's full-row form
    const glv_track_frames* fr = nullptr;   // a frames call (glv_batch_track_frames_s16 / _f32): its render frames; set before the plan (the sizing query's holds `frames` alone)
    const glv_track_frames_each* fe = nullptr;   // ... of a per-stream frames call (glv_batch_track_each_frames_* / _pool_frames_*): a row of tables, a count of frames and a keep pair
                                        //     per stream; set by track_at beside an `fr` that holds its `frames` and d_keys -- all the plan needs; track_frames picks its launchers by it
    uint64_t frame_rows = 0;            // ... fr->frames * streams * 2: the rows the frames kernel writes and the bars run over
    uint64_t frames_off = 0;            // ... and where its texel rows lie in the workspace when bars follow: behind the transform's region and the scan's
    uint64_t dec_bytes = 0;             // bufscale > 1: the decimated rows' region at the very start of the workspace (a multiple of 256 bytes); every other region lies behind it
};
// frames of a window: n, or the k * n that bufscale k decimates to n
uint64_t window_frames(const glv_batch* b) { return (uint64_t) b->bufscale * b->p.n; }
// What the two track entries (glv_batch_track_s16, glv_batch_track_windows_s16) share, written once so that they cannot disagree: the refusals that are
// not about hop or pitch, and what the chain's stages carry.  In the order the checks have always run: (1) the arguments ...
// live: the entry is the live form, whose batches keep state only where bars sample -- bars and a state operator are part of the call
int track_args(unsigned ops, uint32_t steps, bool live = false) {
    if (!(ops & GLV_OP_FFT)) return fail(GLV_ERR_INVALID, "a track call transforms: GLV_OP_FFT is required (ops 0x%x)", ops);
    if (live && (!(ops & GLV_OP_BARS) || !(ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE))))
        return fail(GLV_ERR_INVALID, "a live track call takes GLV_OP_FFT | GLV_OP_BARS with GLV_OP_GRAVITY and / or GLV_OP_AVERAGE (ops 0x%x)", ops);
    const unsigned allowed = GLV_OP_FFT | GLV_OP_GRAVITY | GLV_OP_AVERAGE | GLV_OP_BARS | GLV_OP_R16 | GLV_OP_PRIVATE_STATE;
    if (ops & ~allowed)
        return fail(GLV_ERR_INVALID, "a track call takes GLV_OP_FFT with GLV_OP_GRAVITY / AVERAGE / BARS / R16 only (no RAW, SMOOTH, WAVE, WRANGE, MAGNITUDE, OUTPUT_IS_STATE; ops 0x%x)", ops);
    if (steps == 0) return fail(GLV_ERR_INVALID, "steps must be > 0");
    return GLV_OK;
}
// ... (2) each entry's own hop and pitch rules, then (3) the batch, the rows of the output, and the decisions
// The kept bins of a live track call: the smallest multiple of 64 that covers the live bins and every bin the call's last kernel can READ, multiplied by a
// zero weight or not -- where that is less than a row and no more than the live share of every kernel configuration; else 0, the full-row form (the
// bars sample too far or the chain has no live class: live_bins() is 0; float rows in front of a kernel whose reads are not bounded here).  Texel rows: the
// integer pass, the snapped bars and the columns never touch what lies beyond their taps, and a texel nobody wrote is a number.  Float rows: the chunked
// work lists read whole chunks past a bar's last tap and multiply them by +0 (plan_wave draws the same line) -- an unwritten float could be a NaN.
uint32_t kept_bins(const glv_batch* b, const TrackPlan& tp) {
    const uint32_t L = b->live_bins();
    if (L == 0) return 0;
    uint32_t reach = L;
    if (!tp.out16) {
        if (tp.bars != ChainPlan::BARS_F32 || b->p.sample_mode != GLV_SAMPLE_AVERAGE || b->p.bars >= glv::kBarSeqMin) return 0;
        reach = b->bar_x.chunk_reach;
    }
    const uint32_t K = glv::track_kept_bins(L, reach);
    if (K >= b->p.n) return 0;
    for (int v = 0; v < glv::frame_variants(b->log_nn); ++v)
        if (K > 2u * (uint32_t) glv::frame_geometry(b->log_nn, v).live_points) return 0;
    return K;
}
// columns: the entry is the columns form (glv_batch_track_columns_*), which takes exactly the batches the other entries refuse for their column texels
// live: the entry is the live form (glv_batch_track_live_*), which takes exactly the batches the other entries refuse for their GLV_OP_BARS_ONLY -- bars, bar
// texels or columns, whichever the batch has set
int track_chain(const glv_batch* b, uint32_t pitch_frames, uint32_t steps, unsigned ops, TrackPlan& tp, bool columns = false, bool live = false) {
    static const float some_output = 0.0f;       // (check_ops asks whether an output exists: the caller's is vetted by the entry)
    if (b->p.gl_storage == 2) return fail(GLV_ERR_STATE, "gl_storage 2 is the pass-by-pass checker form: a track call runs on gl_storage 0 and 1");
    if (live) {
        if (!(b->ops_mask & GLV_OP_BARS_ONLY))
            return fail(GLV_ERR_STATE, "the batch was not created with GLV_OP_BARS_ONLY: its track entries are glv_batch_track_windows_* / glv_batch_track_columns_*");
        columns = b->columns();
    } else if (b->ops_mask & GLV_OP_BARS_ONLY)
        return fail(GLV_ERR_STATE, "the batch was created with GLV_OP_BARS_ONLY: its state beyond the live bins does not exist, which the scan over time would read");
    if (b->columns() && !columns) return fail(GLV_ERR_STATE, "column texels are set (glv_batch_set_column_texels): a track call has no columns form");
    if (columns && !b->columns())
        return fail(GLV_ERR_STATE, "no column texels are set (glv_batch_set_column_texels): bars and bar texels are tracked by glv_batch_track_windows_s16 / _f32");
    if (b->single_row) return fail(GLV_ERR_STATE, "a track call needs a batch of stereo streams");
    if (int rc = check_ops(b, ops, &some_output)) return rc;
    tp.out_rows = (uint64_t) steps * b->streams * 2u;
    if (tp.out_rows > 0xffffffffull)                              // (the transform and the scan count their rows in FrameArgs::units, a uint32_t)
        return fail(GLV_ERR_INVALID, "steps=%u of %u streams at pitch_frames=%u: more than 2^32 rows in one call, cut the track into chunks", steps, b->streams, pitch_frames);
    tp.state = (ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE)) != 0;
    tp.live = live;
    if (upload_storage(b->p)) {
        // gl_storage 3: the float chain (float rows into the scan, float state) whose results leave as the upload's texels wherever bars follow -- from the
        // scan's float-state form, or from a stateless transform directly; the bars of a second launch as plan_chain picks them (check_ops vetted them)
        const bool with_bars = (ops & GLV_OP_BARS) != 0, averaging = b->p.sample_mode == GLV_SAMPLE_AVERAGE;
        tp.bars = !with_bars ? ChainPlan::NO_BARS
                  : b->snapped() ? (b->columns() ? ChainPlan::BARS_COLUMNS_TEXELS : averaging ? ChainPlan::BARS_SNAP : ChainPlan::BARS_SNAP_MODE_TEXELS)
                                 : (averaging ? ChainPlan::BARS_I8 : ChainPlan::BARS_MODE_TEXELS);
        // (a frames call: every step's finished rows stay floats -- they are the keyframes; the upload is the frames kernel's)
        tp.out16 = !tp.fr && (with_bars || (ops & GLV_OP_R16) != 0);
        tp.in16 = !tp.state && tp.out16;
        return GLV_OK;                  // (live: such a batch has no live bins -- tp.kept stays 0, the full-row form)
    }
    if (columns) {      // (check_ops: GLV_OP_BARS on a GL chain with state, no GLV_OP_R16; gl_storage 2 went above -- texel state, texel rows all the way)
        tp.bars = ChainPlan::BARS_COLUMNS_TEXELS; tp.in16 = tp.out16 = true;
        if (live) tp.kept = kept_bins(b, tp);
        return GLV_OK;
    }
    const bool gl = tp.state && b->state16;                       // the GL_R16 chain, texel state (log_mode 2: its passes one by one -- the same texels)
    const bool snap = (ops & GLV_OP_BARS) && b->snapped();        // (check_ops: a GL chain's texel rows)
    // the bars of a second launch, as plan_chain picks them for a chain whose transform kernel does not take them
    if (!(ops & GLV_OP_BARS)) tp.bars = ChainPlan::NO_BARS;
    else if (snap) tp.bars = b->p.sample_mode != GLV_SAMPLE_AVERAGE ? ChainPlan::BARS_SNAP_MODE : b->p.log_mode != 2 ? ChainPlan::BARS_SNAP : ChainPlan::BARS_SNAP_FLOATS;
    else if (gl && b->p.bars >= glv::kBarSeqMin && b->bar_x.i8()) tp.bars = b->p.log_mode != 2 ? ChainPlan::BARS_I8 : ChainPlan::BARS_I8_FLOATS;
    else tp.bars = ChainPlan::BARS_F32;
    tp.in16 = tp.state ? gl : ((ops & GLV_OP_R16) && !(ops & GLV_OP_BARS));
    // with bars the texel conversion applies to the bars: the rows stay floats, unless the bars kernel takes texel rows
    tp.out16 = (ops & GLV_OP_BARS) ? (tp.bars == ChainPlan::BARS_I8 || tp.bars == ChainPlan::BARS_SNAP) : (ops & GLV_OP_R16) != 0;
    if (live) tp.kept = kept_bins(b, tp);
    return GLV_OK;
}
uint64_t up256(uint64_t v) { return (v + 255u) & ~(uint64_t) 255u; }
bool pitch_too_short(uint64_t n, uint32_t pitch_frames, uint32_t hop, uint32_t steps) {
    if ((uint64_t) pitch_frames >= n + (uint64_t) (steps - 1) * hop) return false;
    (void) fail(GLV_ERR_INVALID, "pitch_frames=%u holds fewer than steps=%u windows of n=%llu frames every hop=%u", pitch_frames, steps, (unsigned long long) n, hop);
    return true;
}
// Everything about a track call that does not depend on its pointers or on what the batch did before: refusals, geometry, workspace.
int plan_track(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops, TrackPlan& tp) {
    const uint32_t n = b->p.n;
    if (int rc = refuse_bufscale(b, "glv_batch_track_s16 (its residue launches rest on back-to-back windows of n frames; glv_batch_track_windows_s16 takes any hop)")) return rc;
    if (int rc = track_args(ops, steps)) return rc;
    const int lh = log2_exact(hop);
    if (lh < 2 || hop > n) return fail(GLV_ERR_INVALID, "hop=%u: must be a power of two in [4, n=%u]", hop, n);
    if (pitch_frames % hop != 0) return fail(GLV_ERR_INVALID, "pitch_frames=%u is not a multiple of hop=%u", pitch_frames, hop);
    if (pitch_too_short(n, pitch_frames, hop, steps)) return GLV_ERR_INVALID;
    if (int rc = track_chain(b, pitch_frames, steps, ops, tp)) return rc;
    tp.q = n / hop; tp.log_q = (uint32_t) log2_exact(tp.q);
    tp.frames = (uint64_t) (b->streams - 1) * pitch_frames + (uint64_t) (steps - 1) * hop + n;
    tp.k0 = tp.frames / n;
    if (2u * tp.k0 > 0xffffffffull || (uint64_t) b->streams * (pitch_frames / hop) + steps > 0xffffffffull)
        return fail(GLV_ERR_INVALID, "steps=%u of %u streams at pitch_frames=%u: more than 2^32 rows in one call, cut the track into chunks", steps, b->streams, pitch_frames);
    tp.scan = true; tp.hops_per_pitch = pitch_frames / hop; tp.residue_rows = (uint32_t) (2u * tp.k0);
    tp.rows_bytes = up256((uint64_t) tp.q * 2u * tp.k0 * n * (tp.in16 ? 2u : 4u));
    tp.work_bytes = tp.rows_bytes + ((ops & GLV_OP_BARS) ? up256(tp.out_rows * n * (tp.out16 ? 2u : 4u)) : 0u);
    return GLV_OK;
}
// glv_batch_track_windows_s16 / _f32: any hop >= 1, any pitch that holds the windows.  One transform launch over exactly the windows asked for, so its region of the
// workspace is steps * streams * 2 rows; a stateless chain without bars writes d_out directly and needs none (256: 0 stays "refused").  The scan's region
// exists where a scan runs AND bars follow it.
// The hop and pitch rule of every form whose windows are read where they lie, written once.  at: a table call -- the kernels clamp every entry to pitch_frames - n
// (glv_frame.h TrackWindows), so the recording has to hold ONE window and `hop` is not looked at.
// n: the frames of a window (window_frames: k * n on a batch with bufscale k)
int windows_args(uint64_t n, uint32_t pitch_frames, uint32_t hop, uint32_t steps, bool at) {
    if (at) return pitch_frames >= n ? GLV_OK : fail(GLV_ERR_INVALID, "pitch_frames=%u holds no window of n=%llu frames", pitch_frames, (unsigned long long) n);
    if (hop == 0) return fail(GLV_ERR_INVALID, "hop must be > 0");
    return pitch_too_short(n, pitch_frames, hop, steps) ? GLV_ERR_INVALID : GLV_OK;
}
void windows_geometry(const glv_batch* b, uint32_t steps, unsigned ops, TrackPlan& tp) {
    const uint32_t n = b->p.n;
    tp.windows = true; tp.scan = tp.state; tp.hops_per_pitch = steps;      // (one residue: log_q and residue_rows stay 0)
    tp.to_out = !tp.state && !(ops & GLV_OP_BARS) && !tp.fr;
    tp.dec_bytes = b->bufscale > 1u ? up256(tp.out_rows * n * 4u) : 0u;      // (offsets below are counted from behind it: `track` moves its base)
    if (tp.to_out) { tp.rows_bytes = 0; tp.work_bytes = tp.dec_bytes != 0 ? tp.dec_bytes : 256; return; }
    tp.rows_bytes = up256(tp.out_rows * n * (tp.in16 ? 2u : 4u));
    tp.frames_off = tp.rows_bytes + (tp.state && ((ops & GLV_OP_BARS) || tp.fr) ? up256(tp.out_rows * n * (tp.out16 ? 2u : 4u)) : 0u);
    tp.work_bytes = tp.dec_bytes + tp.frames_off + (tp.fr && (ops & GLV_OP_BARS) ? up256(tp.frame_rows * n * 2u) : 0u);      // a frames call with bars: the frames' texel rows
}
int plan_track_windows(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops, TrackPlan& tp) {
    if (int rc = track_args(ops, steps)) return rc;
    if (int rc = windows_args(window_frames(b), pitch_frames, hop, steps, tp.at)) return rc;
    if (int rc = track_chain(b, pitch_frames, steps, ops, tp)) return rc;
    windows_geometry(b, steps, ops, tp);
    return GLV_OK;
}
// glv_batch_track_columns_s16 / _f32: the windows form of a GL chain with state (track_chain sees to that), texel rows in both regions of the workspace, and
// the columns as the third stage.  (The scan stores every bin of a step, though the columns read only those below the last tap of any distinct texel: a
// store limit was built and measured level with full stores at 64 streams, profiles/r14/track_columns.txt, and taken out again.)
int plan_track_columns(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops, TrackPlan& tp) {
    if (int rc = track_args(ops, steps)) return rc;
    if (!(ops & GLV_OP_BARS)) return fail(GLV_ERR_INVALID, "a columns track call samples: GLV_OP_BARS is required (ops 0x%x)", ops);
    if (int rc = windows_args(window_frames(b), pitch_frames, hop, steps, tp.at)) return rc;
    if (int rc = track_chain(b, pitch_frames, steps, ops, tp, true)) return rc;
    windows_geometry(b, steps, ops, tp);
    return GLV_OK;
}
// glv_batch_track_live_s16 / _f32: the windows form on a GLV_OP_BARS_ONLY batch, bars or columns as the batch has them (track_chain), over the kept bins
// (TrackPlan::kept).  The workspace keeps the windows and columns queries' layout and size: rows at pitch n, of which the kept bins are written.
int plan_track_live(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops, TrackPlan& tp) {
    if (int rc = track_args(ops, steps, true)) return rc;
    if (int rc = windows_args(window_frames(b), pitch_frames, hop, steps, tp.at)) return rc;
    if (int rc = track_chain(b, pitch_frames, steps, ops, tp, false, true)) return rc;
    windows_geometry(b, steps, ops, tp);
    return GLV_OK;
}
// glv_batch_track_at_s16 / _f32 on an FFT chain: the form a caller of the hop entries would have to pick for the batch -- live, columns or windows -- with the
// table's rule for hop and pitch (windows_args).  Everything else is that form's plan: what it refuses, its stages, its workspace.  (`hop` is not looked at.)
int plan_track_at(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops, TrackPlan& tp) {
    tp.at = true;
    if (b->ops_mask & GLV_OP_BARS_ONLY) return plan_track_live(b, pitch_frames, hop, steps, ops, tp);
    if (b->columns()) return plan_track_columns(b, pitch_frames, hop, steps, ops, tp);
    return plan_track_windows(b, pitch_frames, hop, steps, ops, tp);
}
// glv_batch_track_frames_s16 / _f32: what the frames ask of the ops and the batch, then the table call's plan with tp.fr set -- float rows out of its last float
// stage (track_chain), parked in the workspace (windows_geometry), the frames' texel rows behind them where bars follow.
int plan_track_frames(const glv_batch* b, uint32_t pitch_frames, uint32_t steps, unsigned ops, TrackPlan& tp) {
    if (tp.fr->frames == 0) return fail(GLV_ERR_INVALID, "frames must be > 0");
    if (ops & GLV_OP_WAVE) return fail(GLV_ERR_INVALID, "GLV_OP_WAVE keeps no keyframes: a frames track call takes an FFT chain (ops 0x%x)", ops);
    if (!(ops & (GLV_OP_R16 | GLV_OP_BARS)))
        return fail(GLV_ERR_INVALID, "a frames track call's result is a texture: GLV_OP_R16 (the upload's texels) and / or GLV_OP_BARS (ops 0x%x)", ops);
    if (!upload_storage(b->p))
        return fail(GLV_ERR_STATE, "gl_storage=%u: keyframes are interpolated in front of the GL_R16 upload of gl_storage 3 (0 has no upload, on 1 the reference forces interpolation off)",
                    b->p.gl_storage);
    if (b->single_row) return fail(GLV_ERR_STATE, "a track call needs a batch of stereo streams");
    tp.frame_rows = (uint64_t) tp.fr->frames * b->streams * 2u;
    if (tp.frame_rows > 0xffffffffull)
        return fail(GLV_ERR_INVALID, "frames=%u of %u streams: more than 2^32 - 1 rows in one call, cut the frames into chunks", tp.fr->frames, b->streams);
    return plan_track_at(b, pitch_frames, 0u, steps, ops, tp);
}

int refuse_track_pointers(const void* d_pcm, TrackInput f32, const void* d_out, const void* d_work) {
    if (!d_pcm || !d_out || !d_work) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (f32.planar()) { if (reinterpret_cast<uintptr_t>(d_pcm) & 3u) return fail(GLV_ERR_INVALID, "d_rows must be aligned like a float: 4 bytes"); }
    else if (f32 && (reinterpret_cast<uintptr_t>(d_pcm) & 7u)) return fail(GLV_ERR_INVALID, "d_pcm must be aligned like a float frame: 8 bytes");
    if (reinterpret_cast<uintptr_t>(d_work) & 255u) return fail(GLV_ERR_INVALID, "d_work must be 256-byte aligned");
    return GLV_OK;
}
// (1) as residues: q launches of the stateless kernel class, each over back-to-back windows -- the only loop of launches on the track path
int track_residues(glv_batch* b, const TrackPlan& tp, glv::FrameArgs& a, glv::FrameClass cls, const int16_t* d_pcm, uint32_t hop, char* work, hipStream_t st) {
    const uint32_t n = b->p.n;
    for (uint32_t r = 0; r < tp.q; ++r) {
        const uint64_t k_r = (tp.frames - (uint64_t) r * hop) / n;            // k0 or k0 - 1; never past the last window any step reads
        if (k_r == 0) continue;                                                // (counted all the same: the launch count is n / hop)
        a.in = d_pcm + (size_t) r * hop * 2u;
        a.out = reinterpret_cast<float*>(work + (size_t) r * 2u * tp.k0 * n * (tp.in16 ? 2u : 4u));
        a.units = (uint32_t) (2u * k_r);
        int variant = 0, grid = 0;
        launch_plan(b, a.units, glv::IN_S16_STEREO, a.ops, &variant, &grid);
        b->last_grid = grid; b->last_variant = variant;
        const hipError_t e = glv::launch_frame(b->log_nn, glv::IN_S16_STEREO, (int) b->p.log_mode, variant, cls, a, grid, st);
        if (e != hipSuccess) return fail(GLV_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    }
    b->last_launches += (int) tp.q;
    return GLV_OK;
}
// (1) as windows: every window of the call where it lies, one launch, into `rows`
// dec: bufscale > 1 -- the decimated rows' region, which glv_decimate_kernel fills from the windows of k * n frames and the transform then reads as planar rows
int track_windows(glv_batch* b, const TrackPlan& tp, glv::FrameArgs& a, glv::FrameClass cls, const void* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps,
                        float* rows, float* dec, hipStream_t st) {
    a.in = d_pcm; a.out = rows; a.units = (uint32_t) tp.out_rows;
    a.trk.pitch_frames = pitch_frames; a.trk.hop = hop; a.trk.steps = steps; a.trk.streams = b->streams; a.trk.step_major = tp.state ? 0u : 1u;
    a.trk.table_len = tp.each ? steps * b->streams : steps;      // (a row per stream, or one row for all; out_rows = 2 * steps * streams fits 32 bits)
    a.trk.starts = tp.starts; a.trk.start_max = pitch_frames - b->p.n * b->bufscale; a.trk.pad2 = 0;      // (both plans' pitch rule: pitch_frames >= a window)
    int hop_mode = tp.f32 ? glv::IN_F32_TRACK : glv::IN_S16_TRACK;
    int mode = !tp.starts ? hop_mode : tp.f32 ? glv::IN_F32_TRACK_AT : glv::IN_S16_TRACK_AT;      // a table call: the kernel kinds that read it, planned as the hop kinds
    if (tp.f32.planar()) { hop_mode = glv::IN_F32_PLANAR; mode = glv::IN_F32_PLANAR_TRACK_AT; }      // planar rows (a table call: track_at): the planar pipeline's plan and wisdom
    if (tp.each) mode = tp.f32.planar() ? glv::IN_F32_PLANAR_TRACK_EACH : tp.f32 ? glv::IN_F32_TRACK_EACH : glv::IN_S16_TRACK_EACH;      // a table row per stream: the kinds that index it, planned as their siblings
    const glv::TrackPool& pool = tp.f32.pool;
    if (pool.spans) {      // a pool call (a per-stream call: track_pool): the pool's frames where the pitch was -- the planar kind's channel stride -- and the spans where no table call has a hop
        a.trk.pitch_frames = pool.frames; a.trk.hop = (uint64_t) reinterpret_cast<uintptr_t>(pool.spans); a.trk.start_max = 0;
        mode = tp.f32.planar() ? glv::IN_F32_PLANAR_TRACK_POOL : tp.f32 ? glv::IN_F32_TRACK_POOL : glv::IN_S16_TRACK_POOL;
    }
    if (dec) {
        glv::Decimate d = {};
        d.in = d_pcm; d.out = dec; d.n = b->p.n; d.k = b->bufscale; d.mono = b->p.channels == 1 && !tp.f32.planar() ? 1u : 0u; d.w = a.trk;      // (planar rows are taken as they are)
        const int kind = tp.f32.planar() ? glv::DEC_F32_PLANAR_TRACK : tp.f32 ? glv::DEC_F32 : glv::DEC_S16;
        const hipError_t e = pool.spans ? glv::launch_decimate_pool(kind, d, pool, st) : glv::launch_decimate(kind, d, st); ++b->last_launches;
        if (e != hipSuccess) return fail(GLV_ERR_HIP, "bufscale launch failed: %s", hipGetErrorString(e));
        a.in = dec; hop_mode = mode = glv::IN_F32_PLANAR;      // row r of the region becomes row r of `rows`: the index the windows kinds give window (s, t)
    }
    int variant = 0, grid = 0;
    launch_plan(b, a.units, hop_mode, a.ops, &variant, &grid);
    b->last_grid = grid; b->last_variant = variant;
    const hipError_t e = glv::launch_frame(b->log_nn, mode, (int) b->p.log_mode, variant, cls, a, grid, st); ++b->last_launches;
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    b->kernel_name = "glv_frame_kernel";
    return GLV_OK;
}
// (2) the scan over time, from stage (1)'s rows at the start of the workspace into `out`
int track_scan(glv_batch* b, const TrackPlan& tp, glv::FrameArgs& a, uint32_t steps, const char* work, float* out, unsigned ops, hipStream_t st) {
    a.in = work; a.out = out;
    a.units = b->streams * 2u; a.ops = ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE);
    a.grav = b->grav_cur; a.grav_w = b->d_grav; a.hist = b->d_hist; a.head = b->head;
    a.grav_sub = b->grav_sub; a.grav_int = b->grav_int ? 1u : 0u; a.gl_storage = tp.in16 && tp.state ? 1u : 0u;
    glv::TrackGeometry g;
    g.n = b->p.n; g.steps = steps; g.hops_per_pitch = tp.hops_per_pitch; g.log_q = tp.log_q; g.residue_rows = tp.residue_rows; g.out_texels = tp.out16 ? 1u : 0u;
    g.kept = tp.kept != 0 ? tp.kept : b->p.n;
    g.gravity_step = b->p.gravity_step; g.ur = tp.ur;
    glv::TrackEach rows;                // a per-stream call: the counts and the rate rows go to the scan kernel of that call, and `g` keeps a null rate table
    rows.counts = tp.counts; rows.ur = tp.each ? tp.ur : nullptr;
    if (tp.each) g.ur = nullptr;
    const hipError_t e = tp.each ? glv::launch_track_each_scan(a, g, rows, tp.in16, st) : glv::launch_track_scan(a, g, tp.in16, st); ++b->last_launches;
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "scan launch failed: %s", hipGetErrorString(e));
    b->kernel_name = tp.each ? "glv_track_each_scan_kernel" : "glv_track_scan_kernel";
    // A per-stream call: the head advances by `steps` all the same -- it is the batch's, and the counts are the device's; the kernel wrote every stream's ring
    // where that head puts it.  Otherwise the state as `steps` sequential calls leave it: the ring's slots were written where the head implies, the gravity store is the batch's own
    if (ops & GLV_OP_AVERAGE) b->head = (uint32_t) (((uint64_t) b->head + steps) % b->p.avg_frames);
    if ((ops & GLV_OP_GRAVITY) && !(ops & GLV_OP_AVERAGE)) b->grav_cur = b->d_grav;
    return GLV_OK;
}
// (3) for a batch with column texels: the columns of every step's row, from the scan's texels
int track_columns(glv_batch* b, const float* rows, size_t units, float* out, hipStream_t st) {
    const hipError_t e = glv::launch_columns_texels(reinterpret_cast<const uint16_t*>(rows), out, units, b->p.n,
                                                    (uint32_t) b->snap_x.tex.size(), b->p.bars, b->snap_x.col_nsteps, b->snap_x.col_items, b->snap.desc, b->snap.w,
                                                    b->snap_x.col_map, b->p.sample_mode, shape_hybrid(b->p), st);
    ++b->last_launches;
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "columns launch failed: %s", hipGetErrorString(e));
    b->kernel_name = "glv_columns_kernel";
    return GLV_OK;
}
// A frames call, between (2) and (3): every render frame's buffer as the upload's texels (glv_track_frames_kernel), from the keyframes the caller carries and the
// steps' finished float rows -- into d_out, or with bars behind those rows in the workspace, where only the bins the bars kernel reads are written (plan_chain's
// limit for the same kernels on this storage).  Then the keyframes the next call starts from.  `rows`: the steps' rows in, the rows stage (3) reads out.
int track_frames(glv_batch* b, const TrackPlan& tp, float*& rows, uint32_t steps, char* work, float* out, unsigned ops, hipStream_t st) {
    const glv_track_frames& fr = *tp.fr;
    const bool bars = (ops & GLV_OP_BARS) != 0;
    glv::TrackFrames t;
    t.from = fr.d_from; t.to = fr.d_to; t.mod = fr.d_mod; t.keys = fr.d_keys; t.rows = rows;
    t.out = bars ? static_cast<void*>(work + tp.frames_off) : static_cast<void*>(out);
    t.frames = fr.frames; t.steps = steps; t.units = b->streams * 2u; t.n = b->p.n; t.limit = b->p.n;
    const uint32_t bins = b->snapped() ? b->snap.bins : b->bar_x.bins_needed;
    if (bars && bins != 0 && bins < b->p.n) t.limit = (bins + 3u) & ~3u;
    t.segment = b->track_frames_segment != 0 ? b->track_frames_segment : glv::track_frames_segment(t.frames, t.units, t.limit);
    hipError_t e;
    if (tp.fe) {      // a per-stream frames call: stream s's rows of the tables, its count of steps (the scan's: tp.counts) and of frames, all read on the device
        t.from = tp.fe->d_from; t.to = tp.fe->d_to; t.mod = tp.fe->d_mod;
        const glv::TrackFramesEach each = {t, tp.fe->d_frame_counts, tp.counts};
        e = glv::launch_track_frames_each(each, st);
    } else e = glv::launch_track_frames(t, st);
    ++b->last_launches;
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "frames launch failed: %s", hipGetErrorString(e));
    e = tp.fe ? glv::launch_track_keys_each(fr.d_keys, rows, t.units, t.n, steps, tp.counts, tp.fe->d_keep, st)
              : glv::launch_track_keys(fr.d_keys, rows, t.units, t.n, fr.keep_from, fr.keep_to, st);
    ++b->last_launches;
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "keyframe write-back launch failed: %s", hipGetErrorString(e));
    if (bars) rows = static_cast<float*>(t.out);
    return GLV_OK;
}
// the kernel (family) of stage (3), which a live track call names (the other entries have always named the scan)
const char* bars_kernel_name(const glv_batch* b, ChainPlan::Bars bars) {
    switch (bars) {
        case ChainPlan::BARS_I8: case ChainPlan::BARS_I8_FLOATS: return "glv_bars_rows_i8_kernel";
        case ChainPlan::BARS_SNAP: case ChainPlan::BARS_SNAP_FLOATS: return "glv_bars_snap_kernel";
        case ChainPlan::BARS_SNAP_MODE: case ChainPlan::BARS_SNAP_MODE_TEXELS: case ChainPlan::BARS_MODE_TEXELS: return "glv_bars_mode_kernel";
        default: return b->p.sample_mode != GLV_SAMPLE_AVERAGE ? "glv_bars_mode_kernel" : b->p.bars >= glv::kBarSeqMin ? "glv_bars_rows_kernel" : "glv_bars_kernel";
    }
}
// Carries a plan out: what the plan could not know (the pointers, what the batch did before), then the stages.  A refused call leaves the batch untouched.
int track(glv_batch* b, const TrackPlan& tp, const void* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work, unsigned ops, hipStream_t st) {
    if (int rc = refuse_track_pointers(d_pcm, tp.f32, d_out, d_work)) return rc;
    if (int rc = refuse_gravity_mix(b, ops)) return rc;
    if (int rc = refuse_stale_tilt(b)) return rc;
    b->last_launches = 0;
    HIP_TRY(hipSetDevice(b->device));
    commit_gravity_form(b, ops);
    char* const work = static_cast<char*>(d_work) + tp.dec_bytes;      // (bufscale > 1: the decimated rows come first, every other region behind them)
    float* const out = static_cast<float*>(d_out);
    if (int rc = timed_launch_begin(b, st)) return rc;
    glv::FrameArgs a;
    fill_common(a, b->p, b->tab);
    a.ops = GLV_OP_FFT | (tp.in16 ? (unsigned) GLV_OP_R16 : 0u); a.log_mode = b->p.log_mode;
    const glv::FrameClass cls = glv::frame_class(false, false, false, a.ops);
    if (tp.kept != 0) b->ran_live_over(tp.kept);      // the live form over the kept bins: the scan leaves the state at and beyond bin `kept` as it finds it
    if (int rc = tp.windows ? track_windows(b, tp, a, cls, d_pcm, pitch_frames, hop, steps, tp.to_out ? out : reinterpret_cast<float*>(work),
                                            tp.dec_bytes != 0 ? static_cast<float*>(d_work) : nullptr, st)
                            : track_residues(b, tp, a, cls, static_cast<const int16_t*>(d_pcm), hop, work, st)) return rc;
    ChainPlan pl;
    pl.bars = tp.bars;
    pl.rows = reinterpret_cast<float*>(work + (tp.scan ? tp.rows_bytes : 0u));       // what the bars read: the scan's results, or a stateless transform's rows
    const bool parked = (ops & GLV_OP_BARS) || tp.fr;      // the steps' finished rows stay in the workspace: the bars read them, or a frames call's frames kernel
    if (tp.scan) if (int rc = track_scan(b, tp, a, steps, work, parked ? pl.rows : out, ops, st)) return rc;
    size_t units = (size_t) tp.out_rows;
    if (tp.fr) { if (int rc = track_frames(b, tp, pl.rows, steps, work, out, ops, st)) return rc; units = (size_t) tp.frame_rows; }
    // (3) the bars of every step's rows (a frames call: of every frame's), or the columns
    if (tp.bars == ChainPlan::BARS_COLUMNS_TEXELS) { if (int rc = track_columns(b, pl.rows, units, out, st)) return rc; }
    else if (int rc = launch_bars_pass(b, pl, out, units, (ops & GLV_OP_R16) != 0, st)) return rc;
    else if (tp.live) b->kernel_name = bars_kernel_name(b, tp.bars);
    if (tp.fr) b->kernel_name = tp.fe ? "glv_track_frames_each_kernel" : "glv_track_frames_kernel";      // (a frames call names its own kernel, whatever follows it)
    return timed_launch_end(b, st);
}

// ---- track mode for the wave module: the texture of every update of a recording in one call (glv_batch_track_wave_s16 / _f32) ------
// GLV_OP_WAVE is stateless and transforms nothing: a call is plan_wave's one or two launches over steps * streams * 2 rows instead of streams * 2,
// the kernels' windows cut out of the recordings by glv::WaveWindows.  The bars arithmetic, what the waveform kernel writes and how much of a row are
// plan_wave's own choices (track and process cannot disagree); the rows between two launches live in the caller's workspace, not in the scratch rows
// (sized for one update).
struct TrackWavePlan {
    TrackInput f32;                 // the recording is interleaved stereo f32 or planar f32 rows, else s16; set before the plan is made (the sizing query's is s16: the same bytes)
    bool at = false;                // the windows lie where a table in device memory says (glv_batch_track_at_s16 / _f32); set before the plan is made
    ChainPlan pl;                   // the one or two launches of windows that start at any frame
    bool one_launch = false;        // with bars: plan_wave fuses where hop and pitch keep every window on a group of 8 frames -- of a 32-byte aligned d_pcm, which
                                    // only the call sees: on any other it runs `pl`.  Never from floats: the integer pass reads s16 frames, as in a process call
    uint64_t rows = 0;              // steps * streams * 2
    uint64_t work_bytes = 256;      // (without bars there is no second launch and nothing to park: the convention keeps 0 for "refused")
    const glv_track_frames* render = nullptr;   // a frames call (glv_batch_track_wave_frames_s16 / _f32): its render frames; set before the plan (the sizing query's holds `frames` alone)
    uint64_t frame_rows = 0;        // ... render->frames * streams * 2: the rows the frames kernel writes and the bars run over -- nothing is computed per step
};
int plan_track_wave(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops, TrackWavePlan& tp) {
    static const float some_output = 0.0f;       // (check_ops asks whether an output exists: the caller's is vetted by track_wave)
    const uint32_t n = b->p.n;
    if (!(ops & GLV_OP_WAVE)) return fail(GLV_ERR_INVALID, "a wave track call needs GLV_OP_WAVE (ops 0x%x; GLV_OP_FFT chains: glv_batch_track_s16)", ops);
    if (ops & ~(unsigned) (GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16))
        return fail(GLV_ERR_INVALID, "a wave track call takes GLV_OP_WAVE with GLV_OP_BARS / GLV_OP_R16 only (ops 0x%x)", ops);
    if (steps == 0) return fail(GLV_ERR_INVALID, "steps must be > 0");
    if (int rc = windows_args(n, pitch_frames, hop, steps, tp.at)) return rc;
    if (b->single_row) return fail(GLV_ERR_STATE, "a track call needs a batch of stereo streams");
    if (int rc = refuse_bufscale(b, tp.render ? "glv_batch_track_wave_frames_s16 / _f32" : "a wave track call (glv_batch_track_wave_s16 / _f32, GLV_OP_WAVE in a table call)")) return rc;
    tp.rows = (uint64_t) steps * b->streams * 2u;
    if (tp.rows > 0x100000000ull)                 // (a COUNT of rows, steps * units, which the launchers take as a size_t: exactly 2^32 rows pass)
        return fail(GLV_ERR_INVALID, "steps=%u of %u streams: more than 2^32 rows in one call, cut the track into chunks", steps, b->streams);
    if (int rc = check_ops(b, ops, &some_output)) return rc;
    // The sizing query does not see d_pcm, so with bars the workspace is always what the two launches need: plan_wave is asked twice, for windows that
    // start anywhere (the plan every call can fall back on) and for this call's hop and pitch.  A table call always runs the former: the one-launch pass needs every
    // window on a group of 8 frames, which the host cannot know of a table in device memory.
    const int in_mode = tp.f32 ? glv::IN_F32_STEREO : glv::IN_S16_STEREO;
    if (int rc = plan_wave(b, in_mode, ops, 0, nullptr, tp.pl, false)) return rc;
    if (ops & GLV_OP_BARS) {
        ChainPlan grouped;
        if (int rc = plan_wave(b, in_mode, ops, 0, nullptr, grouped, !tp.at && hop % 8u == 0u && pitch_frames % 8u == 0u)) return rc;
        tp.one_launch = grouped.wave_fused;
        tp.work_bytes = up256(tp.rows * n * (tp.pl.wave_r16 ? 2u : 4u));
    }
    if (!tp.render) return GLV_OK;
    // A frames call: a table call whose rows are the render frames' -- the lerp sits between the unpack and the upload, so the pass never runs from the s16 frames
    // in one launch, and what is parked for the bars is the frames' rows in plan_wave's format.
    if (tp.render->frames == 0) return fail(GLV_ERR_INVALID, "frames must be > 0");
    tp.frame_rows = (uint64_t) tp.render->frames * b->streams * 2u;
    if (tp.frame_rows > 0xffffffffull)
        return fail(GLV_ERR_INVALID, "frames=%u of %u streams: more than 2^32 - 1 rows in one call, cut the frames into chunks", tp.render->frames, b->streams);
    tp.one_launch = false;
    if (ops & GLV_OP_BARS) tp.work_bytes = up256(tp.frame_rows * n * (tp.pl.wave_r16 ? 2u : 4u));
    return GLV_OK;
}

// The two launches of a frames call in place of the waveform kernel's one: every render frame's rows (glv_wave_frames_kernel) -- into d_out, or with bars into the
// workspace in the format and up to the limit plan_wave chose for the waveform kernel's rows -- then the keyframes the next call starts from.
int track_wave_frames(glv_batch* b, const TrackWavePlan& tp, const void* d_pcm, const glv::WaveWindows& w, void* rows, hipStream_t st) {
    const glv_track_frames& fr = *tp.render;
    const bool mono = b->p.channels == 1 && !w.planar;
    glv::WaveFrames t;
    t.from = fr.d_from; t.to = fr.d_to; t.mod = fr.d_mod; t.keys = fr.d_keys; t.out = rows;
    t.frames = fr.frames; t.n = b->p.n; t.limit = (tp.pl.wave_limit + 3u) & ~3u;      // (a lane owns four frames; n is a multiple of 4)
    t.segment = b->track_frames_segment != 0 ? b->track_frames_segment : glv::track_frames_segment(t.frames, b->streams, t.limit);
    hipError_t e = glv::launch_wave_frames(d_pcm, (bool) tp.f32, w, mono, t, tp.pl.wave_r16, st); ++b->last_launches;
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "frames launch failed: %s", hipGetErrorString(e));
    e = glv::launch_wave_keys(d_pcm, (bool) tp.f32, w, mono, fr.d_keys, t.n, fr.keep_from, fr.keep_to, st); ++b->last_launches;
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "keyframe write-back launch failed: %s", hipGetErrorString(e));
    return GLV_OK;
}
// ... of a per-stream wave frames call (glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_*): the same two launches with stream s's rows of the
// tables and of the starts, its count of steps and of frames and its keep pair, all read on the device (glv_wave_frames_each_kernel, glv_wave_keys_each_kernel) --
// from the recordings, or with in.pool set through the spans of the one buffer.  The row format, the limit and the segment are track_wave_frames' own.
int track_wave_each_frames(glv_batch* b, const TrackWavePlan& tp, const void* d_pcm, const glv::WaveWindows& w, const TrackInput& in, void* rows, hipStream_t st) {
    const glv_track_frames_each& fe = *in.frames;
    const bool mono = b->p.channels == 1 && !w.planar;
    glv::WaveFramesEach e;
    glv::WaveFrames& t = e.t;
    t.from = fe.d_from; t.to = fe.d_to; t.mod = fe.d_mod; t.keys = fe.d_keys; t.out = rows;
    t.frames = fe.frames; t.n = b->p.n; t.limit = (tp.pl.wave_limit + 3u) & ~3u;      // (a lane owns four frames; n is a multiple of 4)
    t.segment = b->track_frames_segment != 0 ? b->track_frames_segment : glv::track_frames_segment(t.frames, b->streams, t.limit);
    e.frame_counts = fe.d_frame_counts; e.counts = in.counts; e.pool = in.pool;
    hipError_t err = glv::launch_wave_each_frames(d_pcm, (int) in.kind, w, mono, e, tp.pl.wave_r16, st); ++b->last_launches;
    if (err != hipSuccess) return fail(GLV_ERR_HIP, "frames launch failed: %s", hipGetErrorString(err));
    const glv::WaveKeysEach k = {fe.d_keys, t.n, in.counts, fe.d_keep, in.pool};
    err = glv::launch_wave_each_keys(d_pcm, (int) in.kind, w, mono, k, st); ++b->last_launches;
    if (err != hipSuccess) return fail(GLV_ERR_HIP, "keyframe write-back launch failed: %s", hipGetErrorString(err));
    return GLV_OK;
}
// fr: the render frames of a frames call (track_frames_call has vetted them; a table call, so d_starts is set); nullptr: every other call
// f32.frames: the render frames of a per-stream wave frames call (track_each_wave_frames_call has vetted them; `fr` is not set): the plan sees the longest row
// d_starts: the table of a table call (its entry has vetted the pointer), and `hop` is not looked at; nullptr: every `hop` frames
int track_wave(glv_batch* b, const void* d_pcm, TrackInput f32, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work, unsigned ops, hipStream_t st,
               const glv_track_frames* fr = nullptr, const uint32_t* d_starts = nullptr) {
    if (int rc = refuse_track_pointers(d_pcm, f32, d_out, d_work)) return rc;
    glv_track_frames shape = {};      // what the plan reads of a per-stream frames call through `fr`: the longest row (track_at's device for the FFT form)
    if (f32.frames) { shape.frames = f32.frames->frames; shape.d_keys = f32.frames->d_keys; fr = &shape; }
    TrackWavePlan tp;
    tp.f32 = f32; tp.at = d_starts != nullptr; tp.render = fr;
    if (int rc = plan_track_wave(b, pitch_frames, hop, steps, ops, tp)) return rc;
    ChainPlan& pl = tp.pl;
    const bool fused = tp.one_launch && (reinterpret_cast<uintptr_t>(d_pcm) & 31u) == 0u;
    b->last_launches = 0;
    HIP_TRY(hipSetDevice(b->device));
    const bool mono = b->p.channels == 1 && !f32.planar(), r16 = (ops & GLV_OP_R16) != 0;      // (planar rows are taken as they are)
    glv::WaveWindows w;
    w.units = b->streams * 2u; w.steps = steps; w.hop = hop; w.pitch_frames = pitch_frames;
    w.starts = d_starts; w.start_max = pitch_frames - b->p.n; w.planar = f32.planar() ? 1u : 0u;
    if (f32.rows) w.hop = steps;      // a per-stream call: with a table `hop` is the table's own -- uint32 [streams][steps], row s is stream s's
    if (f32.pool.spans) { w.pitch_frames = f32.pool.frames; w.start_max = 0; }      // a pool call: the planar kind's channel stride; the clamp is the span's and the pool's
    // (a store's 32-bit lane offset spans 4 rows of the workgroup: `units` rows apart by steps)
    w.by_steps = b->track_wave_by_steps && (4ull * w.units + 2u) * b->p.bars * 4u <= 0xffffffffull ? 1u : 0u;
    if (int rc = timed_launch_begin(b, st)) return rc;
    hipError_t e;
    if (fr) {
        if (ops & GLV_OP_BARS) pl.out = pl.rows = static_cast<float*>(d_work);
        else pl.out = static_cast<float*>(d_out);
        if (int rc = f32.frames ? track_wave_each_frames(b, tp, d_pcm, w, f32, pl.out, st) : track_wave_frames(b, tp, d_pcm, w, pl.out, st)) return rc;
        if (int rc = launch_bars_pass(b, pl, static_cast<float*>(d_out), (size_t) tp.frame_rows, r16, st)) return rc;
        b->kernel_name = f32.frames ? "glv_wave_frames_each_kernel" : "glv_wave_frames_kernel";      // (a frames call names its own kernel, whatever follows it)
        return timed_launch_end(b, st);
    }
    if (fused) {
        const glv::BarIRowsTables irt = b->bar_x.irows_tables();
        e = glv::launch_bars_i8_pcm_track(d_pcm, w, mono, d_out, b->p.n, b->p.bars, &irt, st, r16);
        b->kernel_name = "glv_bars_rows_i8_kernel";
    } else {
        if (ops & GLV_OP_BARS) pl.out = pl.rows = static_cast<float*>(d_work);
        else pl.out = static_cast<float*>(d_out);
        e = f32.pool.spans ? glv::launch_wave_track_pool(d_pcm, (bool) f32, w, f32.pool, mono, b->p.n, pl.out, pl.wave_r16, pl.wave_limit, st)
                           : glv::launch_wave_track(d_pcm, (bool) f32, w, mono, b->p.n, pl.out, pl.wave_r16, pl.wave_limit, st);
        b->kernel_name = "glv_wave_kernel";
    }
    ++b->last_launches;
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    if (!fused) if (int rc = launch_bars_pass(b, pl, static_cast<float*>(d_out), (size_t) tp.rows, r16, st)) return rc;
    return timed_launch_end(b, st);
}

// The sizing query of a track entry: its plan's workspace, or 0 where the plan refuses (no return code to carry it: the message names the code).
template <class Plan>
uint64_t planned_work_bytes(const glv_batch* b, int (*plan)(const glv_batch*, uint32_t, uint32_t, uint32_t, unsigned, Plan&), uint32_t pitch_frames, uint32_t hop, uint32_t steps,
                            unsigned ops, bool at = false) {
    if (!b) { (void) fail(GLV_ERR_INVALID, "batch is NULL"); return 0; }
    Plan tp;
    tp.at = at;
    if (const int rc = plan(b, pitch_frames, hop, steps, ops, tp)) {
        g_err = std::string(rc == GLV_ERR_STATE ? "GLV_ERR_STATE: " : "GLV_ERR_INVALID: ") + g_err;
        return 0;
    }
    return tp.work_bytes;
}
// glv_batch_track_at_s16 / _f32: the table's own refusals, then the form the ops and the batch select -- the wave form's executor, or the FFT forms'.
// d_ur: the second table of a rates call (track_rates has vetted it, and that the ops have the gravity that reads it); nullptr: the batch's own ur
// fr: the render frames of a frames call (track_frames_call has vetted them and the ops); nullptr: every other call
// each: the tables of a per-stream call (track_each has vetted them: d_starts and d_ur are its rows, [streams][steps]); nullptr: one row for all streams
// f32.frames: the render frames of a per-stream frames call (track_each_frames_call has vetted them and refused GLV_OP_WAVE; `each` is set, `fr` is not)
int track_at(glv_batch* b, const void* d_pcm, TrackInput f32, uint32_t pitch_frames, const uint32_t* d_starts, uint32_t steps, void* d_out, void* d_work, unsigned ops, hipStream_t st,
             const glv_track_frames* fr = nullptr, const glv_track_tables* each = nullptr, const float* d_ur = nullptr) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!d_starts) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (reinterpret_cast<uintptr_t>(d_starts) & 3u) return fail(GLV_ERR_INVALID, "d_starts must be 4-byte aligned");
    if (ops & GLV_OP_WAVE) return track_wave(b, d_pcm, f32, pitch_frames, 0u, steps, d_out, d_work, ops, st, fr, d_starts);
    glv_track_frames shape = {};      // what the plan and the frames stage read of a per-stream frames call through `fr`: the longest row and the keyframes
    const glv_track_frames_each* const fe = f32.frames;
    if (fe) { shape.frames = fe->frames; shape.d_keys = fe->d_keys; fr = &shape; }
    TrackPlan tp;
    tp.fr = fr; tp.fe = fe;
    if (int rc = fr ? plan_track_frames(b, pitch_frames, steps, ops, tp) : plan_track_at(b, pitch_frames, 0u, steps, ops, tp)) return rc;
    tp.f32 = f32; tp.starts = d_starts; tp.ur = d_ur;
    if (each) { tp.each = true; tp.counts = each->d_counts; }
    return track(b, tp, d_pcm, pitch_frames, 0u, steps, d_out, d_work, ops, st);
}
// glv_batch_track_rates_s16 / _f32: the rate table's own refusals, then the table call.  The wave form keeps no state and applies no gravity, and a chain
// without gravity would leave the table unread: both are the caller's mistake, not a call that quietly ignores an argument.
int track_rates(glv_batch* b, const void* d_pcm, TrackInput f32, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur, uint32_t steps, void* d_out, void* d_work,
                unsigned ops, hipStream_t st, const glv_track_frames* fr = nullptr) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!d_ur) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (reinterpret_cast<uintptr_t>(d_ur) & 3u) return fail(GLV_ERR_INVALID, "d_ur must be 4-byte aligned");
    if (ops & GLV_OP_WAVE) return fail(GLV_ERR_INVALID, "GLV_OP_WAVE is stateless: no gravity reads the rate table (glv_batch_track_at_s16 / _f32; ops 0x%x)", ops);
    if (!(ops & GLV_OP_GRAVITY)) return fail(GLV_ERR_INVALID, "a rates track call needs GLV_OP_GRAVITY, which reads the rate table (ops 0x%x)", ops);
    return track_at(b, d_pcm, f32, pitch_frames, d_where, steps, d_out, d_work, ops, st, fr, nullptr, d_ur);
}
// glv_batch_track_each_s16 / _f32 / _f32_planar: a table call whose tables have a row per stream, and a count of steps per stream.  What can be said of the three
// tables without the batch's plan -- the pointers, and which chains have a reader for the rates and state for the counts to protect -- then the table call with the
// rows handed on: its plan, its workspace, its refusals in its words.  Nothing here launches.
int track_each(glv_batch* b, const void* d_pcm, TrackInput f32, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, void* d_out, void* d_work, unsigned ops,
               hipStream_t st) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!tb) return fail(GLV_ERR_INVALID, "tb is NULL");
    if (reinterpret_cast<uintptr_t>(tb) & (alignof(glv_track_tables) - 1u)) return fail(GLV_ERR_INVALID, "tb must be aligned like a pointer: %u bytes", (unsigned) alignof(glv_track_tables));
    if (reinterpret_cast<uintptr_t>(tb->d_ur) & 3u) return fail(GLV_ERR_INVALID, "d_ur must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(tb->d_counts) & 3u) return fail(GLV_ERR_INVALID, "d_counts must be 4-byte aligned");
    if (tb->d_ur) {
        if (ops & GLV_OP_WAVE) return fail(GLV_ERR_INVALID, "GLV_OP_WAVE is stateless: no gravity reads the rate table (glv_batch_track_at_s16 / _f32; ops 0x%x)", ops);
        if (!(ops & GLV_OP_GRAVITY)) return fail(GLV_ERR_INVALID, "a rates track call needs GLV_OP_GRAVITY, which reads the rate table (ops 0x%x)", ops);
    }
    const bool wave_frames = f32.frames && (ops & GLV_OP_WAVE);      // (track_each_wave_frames_call's: the counts bound the keyframes a stream contributes)
    if (tb->d_counts && !wave_frames && ((ops & GLV_OP_WAVE) || !(ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE))))
        return fail(GLV_ERR_INVALID, "the chain keeps no state for d_counts to protect: counts need GLV_OP_GRAVITY and / or GLV_OP_AVERAGE and no GLV_OP_WAVE (ops 0x%x)", ops);
    f32.rows = true; f32.counts = tb->d_counts;
    return track_at(b, d_pcm, f32, pitch_frames, tb->d_starts, steps, d_out, d_work, ops, st, nullptr, tb, tb->d_ur);
}
// glv_batch_track_pool_s16 / _f32 / _f32_planar: a per-stream call over ONE buffer of pool_frames frames, stream s through d_spans[s].  What can be said of the pool
// without the batch's plan -- the pointers, and that it holds one window -- then the per-stream call, and through it the table call, with the pool handed on in
// TrackInput: their plan, their workspace, their refusals in their words.  With a pool the pitch rule is pool_frames >= k n and nothing else is asked: the plans
// see pool_frames where they saw pitch_frames, saturated (their own rule for a table call is the same one: a recording holds a window).  Nothing here launches.
static_assert(sizeof(glv_track_span) == sizeof(glv::TrackSpan) && offsetof(glv_track_span, first) == offsetof(glv::TrackSpan, first)
              && offsetof(glv_track_span, frames) == offsetof(glv::TrackSpan, frames), "the kernels read the header's record");
int track_pool(glv_batch* b, const void* d_pool, TrackInput f32, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, void* d_out,
               void* d_work, unsigned ops, hipStream_t st) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!d_pool || !d_spans) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (reinterpret_cast<uintptr_t>(d_spans) & 15u) return fail(GLV_ERR_INVALID, "d_spans must be 16-byte aligned");
    if (pool_frames < window_frames(b))
        return fail(GLV_ERR_INVALID, "pool_frames=%llu holds no window of n=%llu frames", (unsigned long long) pool_frames, (unsigned long long) window_frames(b));
    f32.pool.spans = reinterpret_cast<const glv::TrackSpan*>(d_spans); f32.pool.frames = pool_frames;
    return track_each(b, d_pool, f32, pool_frames > 0xffffffffull ? 0xffffffffu : (uint32_t) pool_frames, tb, steps, d_out, d_work, ops, st);
}
// glv_batch_track_frames_s16 / _f32: what can be said of the frames without the batch's plan -- the pointers and the pair of keyframes kept -- then the rates call
// or the table call with the frames handed on.  Nothing here launches; a refusal below (plan_track_frames, the table call's own) leaves the batch as untouched.
// wave: the entry is the wave form (glv_batch_track_wave_frames_s16 / _f32), whose keyframes are read from the recording -- the table call's wave executor, no rates
int track_frames_call(glv_batch* b, const void* d_pcm, TrackInput f32, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur, uint32_t steps, const glv_track_frames* fr,
                      void* d_out, void* d_work, unsigned ops, hipStream_t st, bool wave = false) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!fr) return fail(GLV_ERR_INVALID, "fr is NULL");
    if (!wave && (ops & GLV_OP_WAVE)) return fail(GLV_ERR_INVALID, "GLV_OP_WAVE keeps no keyframes: a frames track call takes an FFT chain (ops 0x%x)", ops);
    if (wave && !(ops & GLV_OP_WAVE)) return fail(GLV_ERR_INVALID, "a wave frames track call needs GLV_OP_WAVE (ops 0x%x; GLV_OP_FFT chains: glv_batch_track_frames_s16)", ops);
    if (!fr->d_from || !fr->d_to || !fr->d_mod || !fr->d_keys) return fail(GLV_ERR_INVALID, "NULL device pointer in glv_track_frames");
    if ((reinterpret_cast<uintptr_t>(fr->d_from) | reinterpret_cast<uintptr_t>(fr->d_to) | reinterpret_cast<uintptr_t>(fr->d_mod)) & 3u)
        return fail(GLV_ERR_INVALID, "d_from, d_to and d_mod must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(fr->d_keys) & 15u) return fail(GLV_ERR_INVALID, "d_keys must be 16-byte aligned");
    const uint32_t kf = fr->keep_from, kt = fr->keep_to;
    if (!((kf == 0u && kt == 1u) || (kf == 1u && kt >= 2u) || (kf >= 2u && kt > kf)) || (uint64_t) kt >= (uint64_t) steps + 2u)
        return fail(GLV_ERR_INVALID, "keep_from=%u, keep_to=%u: the keyframes kept are (0, 1), (1, k) or (k, k') with 2 <= k < k' < steps + 2 = %llu", kf, kt,
                    (unsigned long long) steps + 2u);
    if (d_ur) return track_rates(b, d_pcm, f32, pitch_frames, d_where, d_ur, steps, d_out, d_work, ops, st, fr);
    return track_at(b, d_pcm, f32, pitch_frames, d_where, steps, d_out, d_work, ops, st, fr);
}
// glv_batch_track_each_frames_* / glv_batch_track_pool_frames_*: what can be said of the per-stream frames without the batch's plan -- the structure, its pointers
// and their alignment, and that the wave form has no per-stream frames -- then the pool call (d_spans set) or the per-stream call with the frames handed on: their
// refusals in their words, then plan_track_frames' through track_at.  The keep pairs and the counts are device memory: the kernels clamp them.  Nothing here launches.
int track_each_frames_call(glv_batch* b, const void* d_pcm, TrackInput f32, uint64_t frames_held, const glv_track_span* d_spans, bool pool, const glv_track_tables* tb,
                           uint32_t steps, const glv_track_frames_each* fe, void* d_out, void* d_work, unsigned ops, hipStream_t st) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!fe) return fail(GLV_ERR_INVALID, "fe is NULL");
    if (reinterpret_cast<uintptr_t>(fe) & (alignof(glv_track_frames_each) - 1u))
        return fail(GLV_ERR_INVALID, "fe must be aligned like a pointer: %u bytes", (unsigned) alignof(glv_track_frames_each));
    if (ops & GLV_OP_WAVE)
        return fail(GLV_ERR_INVALID, "GLV_OP_WAVE keeps no keyframes: a frames track call takes an FFT chain (ops 0x%x; the wave module: glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_*)", ops);
    if (!fe->d_from || !fe->d_to || !fe->d_mod || !fe->d_keep || !fe->d_keys) return fail(GLV_ERR_INVALID, "NULL device pointer in glv_track_frames_each");
    if ((reinterpret_cast<uintptr_t>(fe->d_from) | reinterpret_cast<uintptr_t>(fe->d_to) | reinterpret_cast<uintptr_t>(fe->d_mod) | reinterpret_cast<uintptr_t>(fe->d_frame_counts)
         | reinterpret_cast<uintptr_t>(fe->d_keep)) & 3u)
        return fail(GLV_ERR_INVALID, "d_from, d_to, d_mod, d_frame_counts and d_keep must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(fe->d_keys) & 15u) return fail(GLV_ERR_INVALID, "d_keys must be 16-byte aligned");
    if (fe->frames == 0) return fail(GLV_ERR_INVALID, "frames must be > 0");
    f32.frames = fe;
    if (pool) return track_pool(b, d_pcm, f32, frames_held, d_spans, tb, steps, d_out, d_work, ops, st);
    return track_each(b, d_pcm, f32, (uint32_t) frames_held, tb, steps, d_out, d_work, ops, st);
}
// glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_*: track_each_frames_call's vetting for the wave form -- the structure, its pointers and their
// alignment, and that the ops name the wave module -- then the pool call (d_spans set) or the per-stream call with the frames handed on: their refusals in their
// words (a rate table among them), then plan_track_wave's through the table call's wave executor.  The keep pairs and the counts are device memory: the kernels
// clamp them.  Nothing here launches.
int track_each_wave_frames_call(glv_batch* b, const void* d_pcm, TrackInput f32, uint64_t frames_held, const glv_track_span* d_spans, bool pool, const glv_track_tables* tb,
                                uint32_t steps, const glv_track_frames_each* fe, void* d_out, void* d_work, unsigned ops, hipStream_t st) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!fe) return fail(GLV_ERR_INVALID, "fe is NULL");
    if (reinterpret_cast<uintptr_t>(fe) & (alignof(glv_track_frames_each) - 1u))
        return fail(GLV_ERR_INVALID, "fe must be aligned like a pointer: %u bytes", (unsigned) alignof(glv_track_frames_each));
    if (!(ops & GLV_OP_WAVE))
        return fail(GLV_ERR_INVALID, "a per-stream wave frames track call needs GLV_OP_WAVE (ops 0x%x; GLV_OP_FFT chains: glv_batch_track_each_frames_* / glv_batch_track_pool_frames_*)", ops);
    if (!fe->d_from || !fe->d_to || !fe->d_mod || !fe->d_keep || !fe->d_keys) return fail(GLV_ERR_INVALID, "NULL device pointer in glv_track_frames_each");
    if ((reinterpret_cast<uintptr_t>(fe->d_from) | reinterpret_cast<uintptr_t>(fe->d_to) | reinterpret_cast<uintptr_t>(fe->d_mod) | reinterpret_cast<uintptr_t>(fe->d_frame_counts)
         | reinterpret_cast<uintptr_t>(fe->d_keep)) & 3u)
        return fail(GLV_ERR_INVALID, "d_from, d_to, d_mod, d_frame_counts and d_keep must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(fe->d_keys) & 15u) return fail(GLV_ERR_INVALID, "d_keys must be 16-byte aligned");
    if (fe->frames == 0) return fail(GLV_ERR_INVALID, "frames must be > 0");
    f32.frames = fe;
    if (pool) return track_pool(b, d_pcm, f32, frames_held, d_spans, tb, steps, d_out, d_work, ops, st);
    return track_each(b, d_pcm, f32, (uint32_t) frames_held, tb, steps, d_out, d_work, ops, st);
}

// ---- track mode for ring batches: `updates` ring updates in one call (glv_batch_ring_track_s16 / _f32) -------------------------------------------
// A ring batch's stream is a recording the library holds the last n frames of.  The call stages, per stream, those n frames oldest first with the updates *
// new_frames new ones behind them in a region in FRONT of the workspace (glv_ring_stage_kernel, which also writes the table of window starts (t + 1) *
// new_frames behind that region), runs the table call on the staged recordings -- its plan, its stages, its refusals in its words, its workspace behind the two
// new regions -- and writes each stream's last n staged frames back as its ring (glv_ring_keep_kernel), oldest frame at 0.  Nothing of the batch moves before
// every refusal has had its say; the ring and its position move last.
struct RingTrackPlan {
    uint32_t pitch = 0;                 // frames of a staged recording: n + updates * new_frames, rounded up to 4 frames (every stream starts on 16 bytes)
    uint64_t stage_bytes = 0;           // the staged recordings, at the frame size of the widest ring the batch has: one query sizes both entries
    uint64_t starts_bytes = 0;          // the table of window starts behind them
    uint64_t work_bytes = 0;            // both and the table call's own workspace
};
// f32: the ring the call reads -- 0 s16, 1 f32; -1: the sizing query, which asks for any ring
int plan_ring_track(const glv_batch* b, int f32, uint32_t new_frames, uint32_t updates, unsigned ops, RingTrackPlan& rp) {
    const uint32_t n = b->p.n;
    if (new_frames == 0 || new_frames > n) return fail(GLV_ERR_INVALID, "new_frames=%u: must be in [1, n=%u]", new_frames, n);
    if (updates == 0) return fail(GLV_ERR_INVALID, "updates must be > 0");
    const bool has_s16 = b->d_ring.get() != nullptr, has_f32 = b->d_ring_f32.get() != nullptr;
    if (f32 < 0 ? !has_s16 && !has_f32 : f32 ? !has_f32 : !has_s16)
        return fail(GLV_ERR_STATE, "the batch was created without GLV_OP_RING_%s in its ops_mask (rings are allocated at creation, a ring track call never allocates)",
                    f32 < 0 ? "S16 / GLV_OP_RING_F32" : f32 ? "F32" : "S16");
    if ((uint64_t) updates * new_frames > 0xffffffffull - 3u - n)
        return fail(GLV_ERR_INVALID, "updates=%u of new_frames=%u: more than 2^32 frames in one call, cut the updates into chunks", updates, new_frames);
    rp.pitch = (n + updates * new_frames + 3u) & ~3u;
    uint64_t inner = 0;
    if (ops & GLV_OP_WAVE) {
        TrackWavePlan tp;
        tp.at = true;
        if (int rc = plan_track_wave(b, rp.pitch, 0u, updates, ops, tp)) return rc;
        inner = tp.work_bytes;
    } else {
        TrackPlan tp;
        if (int rc = plan_track_at(b, rp.pitch, 0u, updates, ops, tp)) return rc;
        inner = tp.work_bytes;
    }
    rp.stage_bytes = up256((uint64_t) b->streams * rp.pitch * (has_f32 ? 8u : 4u));
    rp.starts_bytes = up256((uint64_t) updates * 4u);
    rp.work_bytes = rp.stage_bytes + rp.starts_bytes + inner;
    return GLV_OK;
}
int ring_track(glv_batch* b, bool f32, const void* d_new, uint32_t new_frames, uint32_t updates, void* d_out, void* d_work, unsigned ops, hipStream_t st) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    RingTrackPlan rp;
    if (int rc = plan_ring_track(b, f32 ? 1 : 0, new_frames, updates, ops, rp)) return rc;
    if (!d_out || !d_work) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (f32 && !d_new) return fail(GLV_ERR_INVALID, "d_new is NULL (the PulseAudio backend has no zero-fill path)");
    if (reinterpret_cast<uintptr_t>(d_new) & (f32 ? 7u : 3u)) return fail(GLV_ERR_INVALID, "d_new must be aligned like a frame: %u bytes", f32 ? 8u : 4u);
    if (reinterpret_cast<uintptr_t>(d_work) & 255u) return fail(GLV_ERR_INVALID, "d_work must be 256-byte aligned");
    if (!(ops & GLV_OP_WAVE)) {      // what the executor of the FFT forms asks of the batch's past: said here, before the first launch
        if (int rc = refuse_gravity_mix(b, ops)) return rc;
        if (int rc = refuse_stale_tilt(b)) return rc;
    }
    HIP_TRY(hipSetDevice(b->device));
    uint32_t* const pos = f32 ? &b->ring_pos_f32 : &b->ring_pos;
    char* const work = static_cast<char*>(d_work);
    glv::RingTrack r;
    r.ring = f32 ? static_cast<void*>(b->d_ring_f32.get()) : static_cast<void*>(b->d_ring.get());
    r.fresh = d_new; r.stage = work; r.starts = reinterpret_cast<uint32_t*>(work + rp.stage_bytes);
    r.n = b->p.n; r.pos = *pos; r.new_frames = new_frames; r.updates = updates; r.pitch = rp.pitch; r.streams = b->streams;
    hipError_t e = glv::launch_ring_track_stage(f32, r, st);
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "ring staging launch failed: %s", hipGetErrorString(e));
    // (a launch that fails behind this point leaves the ring and its position alone; head and the gravity form go back to what the caller saw)
    const uint32_t head = b->head; const float* const grav_cur = b->grav_cur; const int grav_mode = b->grav_mode; const bool ran_live = b->ran_live; const uint32_t kept_live = b->kept_live;
    int rc = track_at(b, r.stage, f32, rp.pitch, r.starts, updates, d_out, work + rp.stage_bytes + rp.starts_bytes, ops, st);
    if (rc == GLV_OK) {
        e = glv::launch_ring_track_keep(f32, r, st);
        if (e != hipSuccess) rc = fail(GLV_ERR_HIP, "ring write-back launch failed: %s", hipGetErrorString(e));
    }
    if (rc != GLV_OK) { b->head = head; b->grav_cur = grav_cur; b->grav_mode = grav_mode; b->ran_live = ran_live; b->kept_live = kept_live; return rc; }
    *pos = 0;                           // the oldest frame sits at frame 0 of every ring
    b->last_launches += 2;              // the two copies around the table call's launches
    return GLV_OK;
}

// ---- ... per stream: stream s takes c_s = min(d_counts[s], updates) of the updates, update t of it at ur = d_ur[s][t] (glv_batch_ring_track_each_s16 / _f32) ----
// The ring track call with the per-stream table call in the place of the table call.  The write-back rewrites every ring oldest frame first whatever the stream
// took, so a stream that took c_s updates keeps the last n of ITS n + c_s * new_frames frames and the batch's one ring position, 0, is right for all of them: the
// staging puts a stream's first c_s * new_frames new frames behind its ring and zeros behind those (glv_ring_stage_each_kernel, which also writes a row of starts
// (t + 1) * new_frames per stream), the write-back reads from c_s * new_frames on (glv_ring_keep_each_kernel).  Windows behind a count lie in the staged region and
// the scan discards their rows.  The wave form keeps no state, takes no rates and has no meaning for a count: the lockstep entries take it.
// The plan: the lockstep call's (new_frames, updates, the ring, the 2^32 bounds, then plan_track_at's refusals and workspace), with a row of starts per stream.
int plan_ring_track_each(const glv_batch* b, int f32, uint32_t new_frames, uint32_t updates, unsigned ops, RingTrackPlan& rp) {
    if (ops & GLV_OP_WAVE)
        return fail(GLV_ERR_INVALID, "GLV_OP_WAVE keeps no state for a count or a rate to act on: the wave form takes glv_batch_ring_track_s16 / _f32 (ops 0x%x)", ops);
    if (int rc = plan_ring_track(b, f32, new_frames, updates, ops, rp)) return rc;
    const uint64_t rows = up256((uint64_t) b->streams * updates * 4u);      // (rows of the output <= 2^32: no overflow)
    rp.work_bytes += rows - rp.starts_bytes;
    rp.starts_bytes = rows;
    return GLV_OK;
}
int ring_track_each(glv_batch* b, bool f32, const void* d_new, uint32_t new_frames, uint32_t updates, const float* d_ur, const uint32_t* d_counts, void* d_out, void* d_work,
                    unsigned ops, hipStream_t st) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    RingTrackPlan rp;
    if (int rc = plan_ring_track_each(b, f32 ? 1 : 0, new_frames, updates, ops, rp)) return rc;
    if (!d_out || !d_work) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (f32 && !d_new) return fail(GLV_ERR_INVALID, "d_new is NULL (the PulseAudio backend has no zero-fill path)");
    if (reinterpret_cast<uintptr_t>(d_new) & (f32 ? 7u : 3u)) return fail(GLV_ERR_INVALID, "d_new must be aligned like a frame: %u bytes", f32 ? 8u : 4u);
    if (reinterpret_cast<uintptr_t>(d_work) & 255u) return fail(GLV_ERR_INVALID, "d_work must be 256-byte aligned");
    // what the per-stream call says of the two tables, in its words, and what the executor of the FFT forms asks of the batch's past: said here, before the first launch
    if (reinterpret_cast<uintptr_t>(d_ur) & 3u) return fail(GLV_ERR_INVALID, "d_ur must be 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_counts) & 3u) return fail(GLV_ERR_INVALID, "d_counts must be 4-byte aligned");
    if (d_ur && !(ops & GLV_OP_GRAVITY)) return fail(GLV_ERR_INVALID, "a rates track call needs GLV_OP_GRAVITY, which reads the rate table (ops 0x%x)", ops);
    if (d_counts && !(ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE)))
        return fail(GLV_ERR_INVALID, "the chain keeps no state for d_counts to protect: counts need GLV_OP_GRAVITY and / or GLV_OP_AVERAGE and no GLV_OP_WAVE (ops 0x%x)", ops);
    if (int rc = refuse_gravity_mix(b, ops)) return rc;
    if (int rc = refuse_stale_tilt(b)) return rc;
    HIP_TRY(hipSetDevice(b->device));
    uint32_t* const pos = f32 ? &b->ring_pos_f32 : &b->ring_pos;
    char* const work = static_cast<char*>(d_work);
    glv::RingTrackEach e;
    e.r.ring = f32 ? static_cast<void*>(b->d_ring_f32.get()) : static_cast<void*>(b->d_ring.get());
    e.r.fresh = d_new; e.r.stage = work; e.r.starts = reinterpret_cast<uint32_t*>(work + rp.stage_bytes);
    e.r.n = b->p.n; e.r.pos = *pos; e.r.new_frames = new_frames; e.r.updates = updates; e.r.pitch = rp.pitch; e.r.streams = b->streams;
    e.counts = d_counts;
    hipError_t err = glv::launch_ring_each_stage(f32, e, st);
    if (err != hipSuccess) return fail(GLV_ERR_HIP, "ring staging launch failed: %s", hipGetErrorString(err));
    // (a launch that fails behind this point leaves the ring and its position alone; head and the gravity form go back to what the caller saw)
    const uint32_t head = b->head; const float* const grav_cur = b->grav_cur; const int grav_mode = b->grav_mode; const bool ran_live = b->ran_live; const uint32_t kept_live = b->kept_live;
    const glv_track_tables tb = {e.r.starts, d_ur, d_counts};
    int rc = track_each(b, e.r.stage, f32, rp.pitch, &tb, updates, d_out, work + rp.stage_bytes + rp.starts_bytes, ops, st);
    if (rc == GLV_OK) {
        err = glv::launch_ring_each_keep(f32, e, st);
        if (err != hipSuccess) rc = fail(GLV_ERR_HIP, "ring write-back launch failed: %s", hipGetErrorString(err));
    }
    if (rc != GLV_OK) { b->head = head; b->grav_cur = grav_cur; b->grav_mode = grav_mode; b->ran_live = ran_live; b->kept_live = kept_live; return rc; }
    *pos = 0;                           // the oldest frame sits at frame 0 of every ring, whatever its stream took
    b->last_launches += 2;              // the two copies around the per-stream table call's launches
    return GLV_OK;
}
}  // namespace

extern "C" {
uint64_t glv_batch_track_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops) {
    return planned_work_bytes(b, plan_track, pitch_frames, hop, steps, ops);
}

int glv_batch_track_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                        unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    TrackPlan tp;
    if (int rc = plan_track(b, pitch_frames, hop, steps, ops, tp)) return rc;
    return track(b, tp, d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// (the workspace holds the transform's rows and the scan's: neither depends on the recording's type, one query for glv_batch_track_windows_s16 and _f32)
uint64_t glv_batch_track_windows_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops) {
    return planned_work_bytes(b, plan_track_windows, pitch_frames, hop, steps, ops);
}

int glv_batch_track_windows_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                                unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    TrackPlan tp;
    if (int rc = plan_track_windows(b, pitch_frames, hop, steps, ops, tp)) return rc;
    return track(b, tp, d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// (texel rows in both regions of the workspace, whatever the recording's type: one query for glv_batch_track_columns_s16 and _f32)
uint64_t glv_batch_track_columns_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops) {
    return planned_work_bytes(b, plan_track_columns, pitch_frames, hop, steps, ops);
}

int glv_batch_track_columns_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                                unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    TrackPlan tp;
    if (int rc = plan_track_columns(b, pitch_frames, hop, steps, ops, tp)) return rc;
    return track(b, tp, d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_columns_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                                unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    TrackPlan tp;
    if (int rc = plan_track_columns(b, pitch_frames, hop, steps, ops, tp)) return rc;
    tp.f32 = true;
    return track(b, tp, d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// (the workspace of the windows or the columns query, whichever form the batch takes: one query for glv_batch_track_live_s16 and _f32)
uint64_t glv_batch_track_live_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops) {
    return planned_work_bytes(b, plan_track_live, pitch_frames, hop, steps, ops);
}

int glv_batch_track_live_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                             unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    TrackPlan tp;
    if (int rc = plan_track_live(b, pitch_frames, hop, steps, ops, tp)) return rc;
    return track(b, tp, d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_live_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                             unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    TrackPlan tp;
    if (int rc = plan_track_live(b, pitch_frames, hop, steps, ops, tp)) return rc;
    tp.f32 = true;
    return track(b, tp, d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// (the rows between the two launches are texels or floats of the waveform, whatever the recording's type: one query for glv_batch_track_wave_s16 and _f32)
uint64_t glv_batch_track_wave_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops) {
    return planned_work_bytes(b, plan_track_wave, pitch_frames, hop, steps, ops);
}

int glv_batch_track_wave_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                             unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    return track_wave(b, d_pcm, false, pitch_frames, hop, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_windows_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                                unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    TrackPlan tp;
    if (int rc = plan_track_windows(b, pitch_frames, hop, steps, ops, tp)) return rc;
    tp.f32 = true;
    return track(b, tp, d_pcm, pitch_frames, hop, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_wave_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                             unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    return track_wave(b, d_pcm, true, pitch_frames, hop, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// (one query for glv_batch_track_at_s16 and _f32, every form: the workspace of the form's own query for the same steps -- none of them depends on hop or pitch
// where the windows are read where they lie; asked with the shortest recording a call takes, one window)
uint64_t glv_batch_track_at_work_bytes(const glv_batch* b, uint32_t steps, unsigned ops) {
    if (!b) { (void) fail(GLV_ERR_INVALID, "batch is NULL"); return 0; }
    if (ops & GLV_OP_WAVE) return planned_work_bytes(b, plan_track_wave, b->p.n, 0u, steps, ops, true);
    return planned_work_bytes(b, plan_track_at, (uint32_t) window_frames(b), 0u, steps, ops, true);
}

int glv_batch_track_at_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const uint32_t* d_starts, uint32_t steps, void* d_out, void* d_work,
                           unsigned ops, void* hip_stream) {
    return track_at(b, d_pcm, false, pitch_frames, d_starts, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_at_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const uint32_t* d_starts, uint32_t steps, void* d_out, void* d_work,
                           unsigned ops, void* hip_stream) {
    return track_at(b, d_pcm, true, pitch_frames, d_starts, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// From a planar float recording, float [streams][2][pitch_frames]: the table call with the recording's type and nothing else (sized by glv_batch_track_at_work_bytes)
int glv_batch_track_at_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const uint32_t* d_starts, uint32_t steps, void* d_out, void* d_work,
                                  unsigned ops, void* hip_stream) {
    return track_at(b, d_rows, TrackInput::F32_PLANAR, pitch_frames, d_starts, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// (sized by glv_batch_track_at_work_bytes: the rate table adds no region.  d_where is the header's d_starts, handed on whole: tests/test_track_at_host.py pins
// every entry named glv_batch_track_<form>_s16 / _f32 other than the `at` pair to a body that names no table of starts)
int glv_batch_track_rates_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur, uint32_t steps, void* d_out, void* d_work,
                              unsigned ops, void* hip_stream) {
    return track_rates(b, d_pcm, false, pitch_frames, d_where, d_ur, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_rates_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur, uint32_t steps, void* d_out, void* d_work,
                              unsigned ops, void* hip_stream) {
    return track_rates(b, d_pcm, true, pitch_frames, d_where, d_ur, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_rates_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur, uint32_t steps, void* d_out,
                                     void* d_work, unsigned ops, void* hip_stream) {
    return track_rates(b, d_rows, TrackInput::F32_PLANAR, pitch_frames, d_where, d_ur, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// A table row per stream, and a count of steps per stream (sized by glv_batch_track_at_work_bytes: the rows add no region).  The tables are handed on whole.
int glv_batch_track_each_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, void* d_out, void* d_work, unsigned ops,
                             void* hip_stream) {
    return track_each(b, d_pcm, false, pitch_frames, tb, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_each_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, void* d_out, void* d_work, unsigned ops,
                             void* hip_stream) {
    return track_each(b, d_pcm, true, pitch_frames, tb, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_each_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, void* d_out, void* d_work, unsigned ops,
                                    void* hip_stream) {
    return track_each(b, d_rows, TrackInput::F32_PLANAR, pitch_frames, tb, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// One pool of recordings, a span per stream (sized by glv_batch_track_at_work_bytes, as the per-stream call is).  Pool, spans and tables are handed on whole.
int glv_batch_track_pool_s16(glv_batch* b, const int16_t* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, void* d_out,
                             void* d_work, unsigned ops, void* hip_stream) {
    return track_pool(b, d_pool, false, pool_frames, d_spans, tb, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_pool_f32(glv_batch* b, const float* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, void* d_out,
                             void* d_work, unsigned ops, void* hip_stream) {
    return track_pool(b, d_pool, true, pool_frames, d_spans, tb, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_pool_f32_planar(glv_batch* b, const float* d_rows, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps,
                                    void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_pool(b, d_rows, TrackInput::F32_PLANAR, pool_frames, d_spans, tb, steps, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// (one query for glv_batch_track_frames_s16 and _f32: the table call's regions with float rows in both, and with bars the frames' texel rows behind them; asked, like
// glv_batch_track_at_work_bytes, with the shortest recording a call takes)
uint64_t glv_batch_track_frames_work_bytes(const glv_batch* b, uint32_t steps, uint32_t frames, unsigned ops) {
    if (!b) { (void) fail(GLV_ERR_INVALID, "batch is NULL"); return 0; }
    glv_track_frames shape = {};
    shape.frames = frames;
    TrackPlan tp;
    tp.fr = &shape;
    if (const int rc = plan_track_frames(b, (uint32_t) window_frames(b), steps, ops, tp)) {
        g_err = std::string(rc == GLV_ERR_STATE ? "GLV_ERR_STATE: " : "GLV_ERR_INVALID: ") + g_err;
        return 0;
    }
    return tp.work_bytes;
}

int glv_batch_track_frames_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur, uint32_t steps, const glv_track_frames* fr,
                               void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_frames_call(b, d_pcm, false, pitch_frames, d_where, d_ur, steps, fr, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_frames_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur, uint32_t steps, const glv_track_frames* fr,
                               void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_frames_call(b, d_pcm, true, pitch_frames, d_where, d_ur, steps, fr, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_frames_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur, uint32_t steps,
                                      const glv_track_frames* fr, void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_frames_call(b, d_rows, TrackInput::F32_PLANAR, pitch_frames, d_where, d_ur, steps, fr, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// A row of frame tables, a count of frames and a keep pair per stream, on the per-stream call's updates (sized by glv_batch_track_frames_work_bytes with the longest row:
// the rows add no region).  Tables and frames are handed on whole.
int glv_batch_track_each_frames_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
                                    void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_frames_call(b, d_pcm, false, pitch_frames, nullptr, false, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_each_frames_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
                                    void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_frames_call(b, d_pcm, true, pitch_frames, nullptr, false, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_each_frames_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
                                           void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_frames_call(b, d_rows, TrackInput::F32_PLANAR, pitch_frames, nullptr, false, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// ... and on the pool call's: one buffer of recordings, a span per stream
int glv_batch_track_pool_frames_s16(glv_batch* b, const int16_t* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps,
                                    const glv_track_frames_each* fe, void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_frames_call(b, d_pool, false, pool_frames, d_spans, true, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_pool_frames_f32(glv_batch* b, const float* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps,
                                    const glv_track_frames_each* fe, void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_frames_call(b, d_pool, true, pool_frames, d_spans, true, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_pool_frames_f32_planar(glv_batch* b, const float* d_rows, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps,
                                           const glv_track_frames_each* fe, void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_frames_call(b, d_rows, TrackInput::F32_PLANAR, pool_frames, d_spans, true, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// (one query for glv_batch_track_wave_frames_s16 and _f32: 256 without bars, else the frames' rows in the format plan_wave gives the bars kernel; asked, like
// glv_batch_track_at_work_bytes, with the shortest recording a call takes)
uint64_t glv_batch_track_wave_frames_work_bytes(const glv_batch* b, uint32_t steps, uint32_t frames, unsigned ops) {
    if (!b) { (void) fail(GLV_ERR_INVALID, "batch is NULL"); return 0; }
    glv_track_frames shape = {};
    shape.frames = frames;
    TrackWavePlan tp;
    tp.at = true; tp.render = &shape;
    if (const int rc = plan_track_wave(b, b->p.n, 0u, steps, ops, tp)) {
        g_err = std::string(rc == GLV_ERR_STATE ? "GLV_ERR_STATE: " : "GLV_ERR_INVALID: ") + g_err;
        return 0;
    }
    return tp.work_bytes;
}

int glv_batch_track_wave_frames_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const uint32_t* d_where, uint32_t steps, const glv_track_frames* fr,
                                    void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_frames_call(b, d_pcm, false, pitch_frames, d_where, nullptr, steps, fr, d_out, d_work, ops, (hipStream_t) hip_stream, true);
}

int glv_batch_track_wave_frames_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const uint32_t* d_where, uint32_t steps, const glv_track_frames* fr,
                                    void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_frames_call(b, d_pcm, true, pitch_frames, d_where, nullptr, steps, fr, d_out, d_work, ops, (hipStream_t) hip_stream, true);
}

int glv_batch_track_wave_frames_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const uint32_t* d_where, uint32_t steps, const glv_track_frames* fr,
                                           void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_frames_call(b, d_rows, TrackInput::F32_PLANAR, pitch_frames, d_where, nullptr, steps, fr, d_out, d_work, ops, (hipStream_t) hip_stream, true);
}

// The wave module's render frames per stream (sized by glv_batch_track_wave_frames_work_bytes with the longest row: the rows add no region).  Tables and frames are
// handed on whole.
int glv_batch_track_each_wave_frames_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
                                         void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_wave_frames_call(b, d_pcm, false, pitch_frames, nullptr, false, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_each_wave_frames_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
                                         void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_wave_frames_call(b, d_pcm, true, pitch_frames, nullptr, false, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_each_wave_frames_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps,
                                                const glv_track_frames_each* fe, void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_wave_frames_call(b, d_rows, TrackInput::F32_PLANAR, pitch_frames, nullptr, false, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// ... and over one buffer of recordings, a span per stream
int glv_batch_track_pool_wave_frames_s16(glv_batch* b, const int16_t* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps,
                                         const glv_track_frames_each* fe, void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_wave_frames_call(b, d_pool, false, pool_frames, d_spans, true, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_pool_wave_frames_f32(glv_batch* b, const float* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps,
                                         const glv_track_frames_each* fe, void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_wave_frames_call(b, d_pool, true, pool_frames, d_spans, true, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_track_pool_wave_frames_f32_planar(glv_batch* b, const float* d_rows, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps,
                                                const glv_track_frames_each* fe, void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return track_each_wave_frames_call(b, d_rows, TrackInput::F32_PLANAR, pool_frames, d_spans, true, tb, steps, fe, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// (one query for glv_batch_ring_track_s16 and _f32: the staged recordings at the frame size of the widest ring the batch has, the table of starts, and behind
// them what glv_batch_track_at_work_bytes answers for the same updates and ops)
uint64_t glv_batch_ring_track_work_bytes(const glv_batch* b, uint32_t new_frames, uint32_t updates, unsigned ops) {
    if (!b) { (void) fail(GLV_ERR_INVALID, "batch is NULL"); return 0; }
    RingTrackPlan rp;
    if (const int rc = plan_ring_track(b, -1, new_frames, updates, ops, rp)) {
        g_err = std::string(rc == GLV_ERR_STATE ? "GLV_ERR_STATE: " : "GLV_ERR_INVALID: ") + g_err;
        return 0;
    }
    return rp.work_bytes;
}

int glv_batch_ring_track_s16(glv_batch* b, const int16_t* d_new, uint32_t new_frames, uint32_t updates, void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return ring_track(b, false, d_new, new_frames, updates, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_ring_track_f32(glv_batch* b, const float* d_new, uint32_t new_frames, uint32_t updates, void* d_out, void* d_work, unsigned ops, void* hip_stream) {
    return ring_track(b, true, d_new, new_frames, updates, d_out, d_work, ops, (hipStream_t) hip_stream);
}

// (one query for glv_batch_ring_track_each_s16 and _f32: the lockstep query's regions with a row of starts per stream in the place of its one row)
uint64_t glv_batch_ring_track_each_work_bytes(const glv_batch* b, uint32_t new_frames, uint32_t updates, unsigned ops) {
    if (!b) { (void) fail(GLV_ERR_INVALID, "batch is NULL"); return 0; }
    RingTrackPlan rp;
    if (const int rc = plan_ring_track_each(b, -1, new_frames, updates, ops, rp)) {
        g_err = std::string(rc == GLV_ERR_STATE ? "GLV_ERR_STATE: " : "GLV_ERR_INVALID: ") + g_err;
        return 0;
    }
    return rp.work_bytes;
}

int glv_batch_ring_track_each_s16(glv_batch* b, const int16_t* d_new, uint32_t new_frames, uint32_t updates, const float* d_ur, const uint32_t* d_counts, void* d_out,
                                  void* d_work, unsigned ops, void* hip_stream) {
    return ring_track_each(b, false, d_new, new_frames, updates, d_ur, d_counts, d_out, d_work, ops, (hipStream_t) hip_stream);
}

int glv_batch_ring_track_each_f32(glv_batch* b, const float* d_new, uint32_t new_frames, uint32_t updates, const float* d_ur, const uint32_t* d_counts, void* d_out,
                                  void* d_work, unsigned ops, void* hip_stream) {
    return ring_track_each(b, true, d_new, new_frames, updates, d_ur, d_counts, d_out, d_work, ops, (hipStream_t) hip_stream);
}
}  // extern "C"
