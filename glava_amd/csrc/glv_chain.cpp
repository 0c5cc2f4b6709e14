// glv_chain.cpp -- one process call: what it needs prepared (batch_prepare), its argument checks, its plan (ChainPlan: route, kernel class, where
// the rows go, which bars launch follows) and the launches that carry the plan out.
#include <cstring>

#include "glv_host.h"
#include "glv_tables.h"       // make_frame_weights, gravity_r16_integer_step, kBarSeqMin

namespace glvh __attribute__((visibility("hidden"))) {
// does `ops` run as the fused GL_R16 kernel?  (gl_storage 1, an FFT chain with state; RAW / SMOOTH / the audit log take the passes one by one)
bool gl_fused_chain(const glv_batch* b, unsigned ops) {
    return b->p.gl_storage == 1 && (ops & GLV_OP_FFT) && (ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE)) && !(ops & (GLV_OP_RAW | GLV_OP_SMOOTH)) && b->p.log_mode != 2;
}
}  // namespace glvh
namespace {
// ... or the GL passes one by one (gl_storage 2; RAW / SMOOTH / the audit log of 1)?  (gl_storage 3 is the float chain: no GL pass)
bool gl_passes_chain(const glv_batch* b, unsigned ops) {
    return b->p.gl_storage != 0 && !upload_storage(b->p) && (ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE)) && !gl_fused_chain(b, ops);
}
}  // namespace
namespace glvh __attribute__((visibility("hidden"))) {
// the operators of an FFT chain the frame kernel runs: the GL passes one by one leave it the transform alone (GLV_OP_RAW: the passes then
// run on the raw values)
unsigned frame_ops(const glv_batch* b, unsigned ops) { return gl_passes_chain(b, ops) ? GLV_OP_FFT | (ops & GLV_OP_RAW) : ops; }

void fill_common(glv::FrameArgs& a, const glv_params& p, const Tables& t) {
    std::memset(&a, 0, sizeof(a));
    a.tw = t.d_tw; a.win = t.d_win; a.win_split = t.d_win_split; a.logtab = t.d_log; a.tilt = t.d_tilt;
    a.F = p.avg_frames; a.mono = p.channels == 1; a.avg_window = p.avg_window != 0;
    a.inv_n = 1.0f / (float) p.n;
    a.fft_scale = p.fft_scale;
    a.one_minus_cutoff = 1.0F - p.fft_cutoff;                  // render.c:845
    a.g = p.gravity_step * (1.0F / p.ur);                      // render.c:728
    a.F_as_float = (float) p.avg_frames;                       // render.c:761
    a.F_rcp = 1.0F / (float) p.avg_frames;
    glv::make_frame_weights(a.wts, p.avg_frames, p.avg_window != 0, (int) p.avg_window_kind);
    for (uint32_t f = 0; f < p.avg_frames; ++f) a.wts32[f] = (float) a.wts[f];
}

int timed_launch_begin(glv_batch* b, hipStream_t st) {
    if (!b->timing) return GLV_OK;
    if (b->ev_used + 2 > b->ev.size()) {
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        b->ev.push_back(e0); b->ev.push_back(e1);
    }
    HIP_TRY(hipEventRecord(b->ev[b->ev_used], st));
    return GLV_OK;
}
int timed_launch_end(glv_batch* b, hipStream_t st) {
    if (!b->timing) return GLV_OK;
    HIP_TRY(hipEventRecord(b->ev[b->ev_used + 1], st));
    b->ev_used += 2;
    b->launches += 1;
    return GLV_OK;
}

// the gravity step on texels (only the GL_R16 state needs it: 65 536 evaluations on the host whenever g changes -- for the
// single-stream drop-ins that is whenever the host's measured `ur` changes, i.e. every frame)
void update_gravity_step(glv_batch* b) {
    const float g = b->p.gravity_step * (1.0F / b->p.ur);                      // render.c:728
    if (b->state16 && (!b->grav_known || std::memcmp(&g, &b->grav_g, sizeof(g)) != 0)) {
        b->grav_int = glv::gravity_r16_integer_step(g, &b->grav_sub);
        b->grav_g = g; b->grav_known = true;
    }
}

// Everything the process calls need besides the state arrays, made from b->p: tilt table, the gravity step on texels, and -- as
// announced by the creation mask -- bar tables, smooth bounds, the internal spectra rows.  Called by creation and by
// glv_batch_set_params (and by the single-stream drop-ins when their caller changes a knob): the ONLY place that allocates or
// copies synchronously; glv_batch_process_* / ring updates never do (tests/test_stream_order.py greps for it).
int batch_prepare(glv_batch* b) {
    if (int rc = b->tab.set_tilt(b->p.fft_scale, b->p.fft_cutoff, b->p.log_mode == 1)) return rc;
    update_gravity_step(b);
    // Tables are cheap and always made (an operator the creation mask did not announce only fails to get them when its
    // parameters are unusable: a later call of that operator is then refused); buffers of spectrum size are made for announced
    // operators only.
    // (an unannounced operator's unusable parameters are not this call's error: glv_last_error keeps what it said before)
    {
        const std::string said = g_err;
        const int rc = ensure_smooth_tables(b);
        if (rc != GLV_OK) { if (b->ops_mask & GLV_OP_SMOOTH) return rc; g_err = said; }
    }
    {
        const std::string said = g_err;
        const int rc = ensure_bar_tables(b);
        if (rc != GLV_OK) { if (b->ops_mask & GLV_OP_BARS) return rc; g_err = said; }
    }
    if (b->ops_mask & GLV_OP_BARS) {
        // the internal spectra rows: needed whenever bars are not computed inside the transform's launch from a row in LDS and no state
        // array holds the spectra -- unless every chain the creation mask announces fuses its bars in every kernel configuration
        // (bars_fusable: 16384 stereo streams of N = 4096 would hold 512 MiB nothing reads).  The mask's R16 bit is the hint that a float
        // chain's bars are wanted as GL_R16 texels (they leave through glv_bars_kernel, from the scratch rows); gravity-only chains read the
        // state.
        // GLV_OP_WAVE | GLV_OP_BARS in two launches: the waveform kernel's texels (or their floats) wait for the bars kernel in the same rows
        if (bars_need_rows(b, b->bar) || (b->ops_mask & GLV_OP_WAVE)) if (int rc = ensure_scratch(b)) return rc;
        if (int rc = ensure_snap_tables(b)) return rc;
        b->update_live_bins();
    }
    // function attributes (the > 64 KiB dynamic-LDS opt-in) of every frame kernel this batch can launch: set here, once per device
    // and instantiation, so that a process call is a plain launch (launch_variant with grid 0 = attribute only; classes a
    // configuration is not built for answer hipErrorInvalidValue, which is not an error here)
    if (b->attr_log_mode != (int) b->p.log_mode) {
        b->attr_log_mode = (int) b->p.log_mode;
        glv::FrameArgs a;
        std::memset(&a, 0, sizeof(a));
        for (int in_mode = 0; in_mode < glv::kFrameKinds + glv::kPlanarTrackKinds + glv::kEachTrackKinds + glv::kPoolTrackKinds; ++in_mode)      // (InMode and a table call's kinds, the planar one, the per-stream ones and the pool ones behind them)
            for (int v = 0; v < glv::frame_variants(b->log_nn); ++v)
                for (int c = 0; c < glv::kFrameClasses; ++c)
                    (void) glv::launch_frame(b->log_nn, in_mode, (int) b->p.log_mode, v, (glv::FrameClass) c, a, 0, nullptr);
        (void) hipGetLastError();
    }
    // the pass-by-pass GL chain parks the transform's f32 spectra when the caller's buffer cannot take them (texel / bar outputs)
    if (b->p.gl_storage == 2 && (b->ops_mask & (GLV_OP_GRAVITY | GLV_OP_AVERAGE)) && !b->single_row) return ensure_scratch(b);
    return GLV_OK;
}

// Argument checks shared by every batched entry point (ring updates run them BEFORE touching the ring, so that a
// rejected call leaves the ring where the caller saw it).
int check_ops(const glv_batch* b, unsigned ops, const float* d_out) {
    // gravity's output IS its new state (render.c:733-734): a chain that ends in gravity can leave the
    // spectra in the state buffer (glv_batch_gravity_state) instead of writing them a second time
    const bool state_is_output = (ops & GLV_OP_GRAVITY) && !(ops & (GLV_OP_AVERAGE | GLV_OP_SMOOTH | GLV_OP_RAW));
    if (!d_out && !(state_is_output && !(ops & GLV_OP_BARS) && !b->state16))
        return fail(GLV_ERR_INVALID, "NULL output pointer (allowed only for f32-state chains ending in gravity, see glv_batch_gravity_state)");
    if (ops & GLV_OP_WAVE) {
        // the wave module's bind is the unpack, wrange and the upload and nothing else (wave/1.frag:7-9); with GLV_OP_BARS the pre-smoothing pass over it
        if (ops & (GLV_OP_FFT | GLV_OP_GRAVITY | GLV_OP_AVERAGE | GLV_OP_RAW | GLV_OP_WRANGE | GLV_OP_MAGNITUDE | GLV_OP_SMOOTH | GLV_OP_OUTPUT_IS_STATE))
            return fail(GLV_ERR_INVALID, "GLV_OP_WAVE combines with GLV_OP_BARS and GLV_OP_R16 only (it includes wrange and is stateless; ops 0x%x)", ops);
        if (ops & GLV_OP_BARS) {
            if (b->p.gl_storage == 0)
                return fail(GLV_ERR_STATE, "GLV_OP_WAVE | GLV_OP_BARS: gl_storage 0 -- a float chain has no texel rows for the pre-smoothing pass to sample");
            if ((b->ops_mask & (GLV_OP_WAVE | GLV_OP_BARS)) != (unsigned) (GLV_OP_WAVE | GLV_OP_BARS))
                return fail(GLV_ERR_STATE, "GLV_OP_WAVE | GLV_OP_BARS needs both bits in glv_batch_create's ops_mask (0x%x): the rows between its two launches are made at creation", b->ops_mask);
        }
        // (with or without bars: a batch whose bars are the graph module's columns is not the wave module's)
        if (b->columns())
            return fail(GLV_ERR_STATE, "GLV_OP_WAVE with column texels set (glv_batch_set_column_texels): the wave shader does not average three texels (wave/1.frag:17-23)");
    }
    const unsigned stateful = ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE);
    if (stateful & ~b->ops_mask)
        return fail(GLV_ERR_STATE, "ops 0x%x need state the batch was not created with (ops_mask 0x%x)", ops, b->ops_mask);
    if (stateful && b->state16 != (b->p.gl_storage == 1))
        return fail(GLV_ERR_STATE, "gl_storage=%u: the state of this batch was created as %s", b->p.gl_storage, b->state16 ? "GL_R16 texels (gl_storage 1)" : "floats (gl_storage 0 / 2 / 3)");
    if ((b->ops_mask & GLV_OP_BARS_ONLY) && stateful && !(ops & GLV_OP_BARS))
        return fail(GLV_ERR_STATE, "the batch was created with GLV_OP_BARS_ONLY: its state lives only below the bins the bars sample, a stateful call must ask for GLV_OP_BARS (ops 0x%x)", ops);
    if ((ops & GLV_OP_WRANGE) && (ops & GLV_OP_FFT)) return fail(GLV_ERR_INVALID, "GLV_OP_WRANGE excludes GLV_OP_FFT");
    if ((ops & GLV_OP_RAW) && !(ops & GLV_OP_FFT)) return fail(GLV_ERR_INVALID, "GLV_OP_RAW needs GLV_OP_FFT");
    if ((ops & GLV_OP_MAGNITUDE) && (ops & (GLV_OP_FFT | GLV_OP_WRANGE))) return fail(GLV_ERR_INVALID, "GLV_OP_MAGNITUDE excludes GLV_OP_FFT and GLV_OP_WRANGE");
    if (!(ops & (GLV_OP_FFT | GLV_OP_GRAVITY | GLV_OP_AVERAGE | GLV_OP_WRANGE | GLV_OP_SMOOTH | GLV_OP_MAGNITUDE | GLV_OP_R16 | GLV_OP_WAVE))) return fail(GLV_ERR_INVALID, "empty ops");
    if ((ops & GLV_OP_R16) && (ops & (GLV_OP_RAW | GLV_OP_SMOOTH))) return fail(GLV_ERR_INVALID, "GLV_OP_R16 excludes GLV_OP_RAW and GLV_OP_SMOOTH");
    if ((ops & GLV_OP_R16) && !d_out) return fail(GLV_ERR_INVALID, "GLV_OP_R16 needs an output buffer");
    if ((ops & GLV_OP_OUTPUT_IS_STATE) && (!state_is_output || !d_out || (ops & (GLV_OP_BARS | GLV_OP_R16)) || (b->p.gl_storage && !upload_storage(b->p))))
        return fail(GLV_ERR_INVALID, "GLV_OP_OUTPUT_IS_STATE needs a chain that ends in gravity with f32 rows out (no AVERAGE / SMOOTH / RAW / BARS / R16, gl_storage 0)");
    if ((ops & GLV_OP_BARS) && !b->bar.desc)
        return fail(GLV_ERR_STATE, "GLV_OP_BARS: the batch has no bar tables (bars / smooth_factor / bar_phase were unusable when it was created; tables are built at creation and by glv_batch_set_params, process calls never allocate)");
    if ((ops & GLV_OP_BARS) && (b->bar_x.count != b->p.bars || b->bar_x.factor != b->p.smooth_factor || b->bar_x.phase != b->p.bar_phase || !same_shape(b->bar_x.shape_of, b->p)))
        return fail(GLV_ERR_STATE, "GLV_OP_BARS: bar parameters changed without glv_batch_set_params");
    if ((ops & GLV_OP_BARS) && !(ops & GLV_OP_WAVE) && upload_storage(b->p)) {
        // gl_storage 3: the bars sample the GL_R16 upload of the finished float buffer (render.c:2185, :2276-2303) -- an FFT chain's, with or without state;
        // what is offered is what the shipped `setsmoothpass true` configuration runs, in the exact forms the GL chains have
        if (!(ops & GLV_OP_FFT) || (ops & (GLV_OP_SMOOTH | GLV_OP_RAW)))
            return fail(GLV_ERR_STATE, "GLV_OP_BARS on gl_storage 3 samples the upload of an FFT chain's finished rows: GLV_OP_FFT is required, GLV_OP_SMOOTH / GLV_OP_RAW are "
                                       "not offered with it (ops 0x%x)", ops);
        if (!b->snapped() && b->p.sample_mode == GLV_SAMPLE_AVERAGE && !(b->p.bars >= glv::kBarSeqMin && b->bar_x.i8()))
            return fail(GLV_ERR_STATE, "GLV_OP_BARS on gl_storage 3: unsnapped averaging bars run as the exact integer pass only (bars=%u: 256 or more, with integer tables); the "
                                       "modules' bars come from glv_batch_set_bar_texels / glv_batch_set_column_texels", b->p.bars);
    }
    if ((ops & GLV_OP_BARS) && b->snapped()) {
        // bars at texels of the pre-smoothing pass: the chain's rows must be what that pass samples -- a GL chain's texels, not smoothed
        // (... or the wave texture's: GLV_OP_WAVE | GLV_OP_BARS, vetted above; or the upload of gl_storage 3, vetted above)
        if (!(ops & GLV_OP_WAVE) && !upload_storage(b->p) && (!(ops & GLV_OP_FFT) || !(gl_fused_chain(b, ops) || gl_passes_chain(b, ops)) || (ops & GLV_OP_SMOOTH)))
            return fail(GLV_ERR_STATE, "GLV_OP_BARS with bar texels set (glv_batch_set_bar_texels) needs a GL chain's texel rows: GLV_OP_FFT with gravity / average on "
                                       "gl_storage 1 or 2, without GLV_OP_SMOOTH (ops 0x%x)", ops);
        if (!snap_current(b)) return fail(GLV_ERR_STATE, "GLV_OP_BARS: bar parameters changed without glv_batch_set_params");
        if (b->columns() && (ops & GLV_OP_R16))
            return fail(GLV_ERR_STATE, "GLV_OP_R16 with column texels set (glv_batch_set_column_texels): a mean of three texels is not a texel, the columns are floats");
    }
    if ((ops & GLV_OP_SMOOTH) && (!b->d_smin || b->smooth_d != b->p.smooth_distance || b->smooth_r != b->p.smooth_ratio))
        return fail(GLV_ERR_STATE, "GLV_OP_SMOOTH: the batch has no window bounds for these parameters (unusable smooth_ratio at creation, or changed without glv_batch_set_params)");
    return GLV_OK;
}

// GLV_OP_WAVE (check_ops vetted the call).  Without bars: the waveform kernel into the caller's buffer.  With bars the pre-smoothing pass runs over the
// upload's texels in the arithmetic of the GL_R16 chain's second launch: GLV_BARS_I8_EXACT straight from s16 frames / the s16 ring in one launch; every
// other form -- f32 inputs, a ring rotated by a number of frames that is not a multiple of 8, maximum / hybrid, fewer than 256 bars, bar texels, no integer tables, the single-stream drop-in, GLV_UNFUSED_WAVE -- as
// the waveform kernel into the scratch rows (texels where the bars kernel takes texels, their floats else; only what the bars sample), then the bars kernel.
// whole_groups: every window the call reads starts on a group of 8 frames of a 32-byte aligned buffer (a process call's windows do; a track call says)
int plan_wave(const glv_batch* b, int in_mode, unsigned ops, uint32_t rot, float* d_out, ChainPlan& pl, bool whole_groups = true) {
    pl.route = ChainPlan::WAVE; pl.ops = ops; pl.out = d_out; pl.bars = ChainPlan::NO_BARS;
    pl.wave_r16 = (ops & GLV_OP_R16) != 0; pl.wave_limit = b->p.n;
    if (!(ops & GLV_OP_BARS)) return GLV_OK;
    const bool averaging = b->p.sample_mode == GLV_SAMPLE_AVERAGE;
    if (b->snapped()) pl.bars = averaging ? ChainPlan::BARS_SNAP : ChainPlan::BARS_SNAP_MODE;
    else if (averaging && b->p.bars >= glv::kBarSeqMin && b->bar_x.i8()) pl.bars = ChainPlan::BARS_I8;
    else pl.bars = ChainPlan::BARS_F32;
    // (the integer pass parks groups of 8 frames: a ring whose oldest frame is not at a multiple of 8 -- an update of a sample_sz / 4 that is not one -- would wrap inside a group)
    pl.wave_fused = pl.bars == ChainPlan::BARS_I8 && (in_mode == glv::IN_S16_STEREO || in_mode == glv::IN_S16_RING) && (rot & 7u) == 0u && whole_groups && !b->unfused_wave && !b->single_row;
    if (pl.wave_fused) return GLV_OK;
    if (!b->d_scratch) return fail(GLV_ERR_STATE, "GLV_OP_WAVE | GLV_OP_BARS needs the internal rows: announce both bits in glv_batch_create's ops_mask");
    pl.out = pl.rows = b->d_scratch;
    pl.wave_r16 = pl.bars == ChainPlan::BARS_I8 || pl.bars == ChainPlan::BARS_SNAP;
    // what the bars do not sample is not produced -- where the bars kernel never multiplies what lies beyond (integer weights of 0, taps, staged bins)
    const uint32_t bins = b->snapped() ? b->snap.bins : b->bar_x.bins_needed;
    if ((pl.bars != ChainPlan::BARS_F32 || !averaging) && bins != 0 && bins < b->p.n) pl.wave_limit = bins;
    return GLV_OK;
}

// the second bars launch of a chain (ChainPlan::bars) over its finished rows
int launch_bars_pass(glv_batch* b, const ChainPlan& pl, float* d_bars, size_t units, bool r16, hipStream_t st) {
    hipError_t e;
    if (pl.bars == ChainPlan::NO_BARS) return GLV_OK;
    if (pl.bars == ChainPlan::BARS_F32 || pl.bars == ChainPlan::BARS_MODE_TEXELS) {
        glv::BarRowsTables rt = rows_tables(b->p, b->bar_x, b->bar);
        rt.rows_texels = pl.bars == ChainPlan::BARS_MODE_TEXELS ? 1u : 0u;
        e = glv::launch_bars(pl.rows, d_bars, units, b->p.n, b->p.bars, b->bar_x.nsteps, b->bar_x.items, b->bar.desc, b->bar.w, st, r16, &rt);
    } else if (pl.bars == ChainPlan::BARS_SNAP || pl.bars == ChainPlan::BARS_SNAP_FLOATS) {
        e = glv::launch_bars_snap(pl.rows, pl.bars == ChainPlan::BARS_SNAP_FLOATS, d_bars, units, b->p.n, b->p.bars, b->snap.desc, reinterpret_cast<const uint32_t*>(b->snap.w.get()), st, r16);
    } else if (pl.bars == ChainPlan::BARS_COLUMNS) {
        e = glv::launch_columns(pl.rows, d_bars, units, b->p.n, (uint32_t) b->snap_x.tex.size(), b->p.bars, b->snap_x.col_nsteps, b->snap_x.col_items, b->snap.desc,
                                b->snap.w, b->snap_x.col_map, b->p.sample_mode, shape_hybrid(b->p), st);
    } else if (pl.bars == ChainPlan::BARS_COLUMNS_TEXELS) {
        e = glv::launch_columns_texels(reinterpret_cast<const uint16_t*>(pl.rows), d_bars, units, b->p.n, (uint32_t) b->snap_x.tex.size(), b->p.bars, b->snap_x.col_nsteps,
                                       b->snap_x.col_items, b->snap.desc, b->snap.w, b->snap_x.col_map, b->p.sample_mode, shape_hybrid(b->p), st);
    } else if (pl.bars == ChainPlan::BARS_SNAP_MODE || pl.bars == ChainPlan::BARS_SNAP_MODE_TEXELS) {
        glv::BarRowsTables rt = rows_tables(b->p, b->bar_x, b->snap);
        rt.rows_texels = pl.bars == ChainPlan::BARS_SNAP_MODE_TEXELS ? 1u : 0u;
        e = glv::launch_bars(pl.rows, d_bars, units, b->p.n, b->p.bars, 0, nullptr, b->snap.desc, nullptr, st, r16, &rt);
    } else {
        const glv::BarIRowsTables irt = b->bar_x.irows_tables();
        e = glv::launch_bars_i8(pl.rows, pl.bars == ChainPlan::BARS_I8_FLOATS, d_bars, units, b->p.n, b->p.bars, &irt, st, r16);
    }
    ++b->last_launches;
    return e == hipSuccess ? GLV_OK : fail(GLV_ERR_HIP, "bars launch failed: %s", hipGetErrorString(e));
}
}  // namespace glvh
namespace {
int plan_chain(glv_batch* b, int in_mode, unsigned ops, uint32_t units, uint32_t rot, float* d_out, ChainPlan& pl) {
    if (ops & GLV_OP_WAVE) return plan_wave(b, in_mode, ops, rot, d_out, pl);
    const bool gl_passes = gl_passes_chain(b, ops);
    if (gl_fused_chain(b, ops)) pl.route = ChainPlan::GL_FUSED;
    else if (ops & GLV_OP_FFT) pl.route = gl_passes ? ChainPlan::GL_PASSES : ChainPlan::FRAME;
    else pl.route = (ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE | GLV_OP_WRANGE | GLV_OP_MAGNITUDE | GLV_OP_R16)) ? ChainPlan::POST : ChainPlan::COPY;
    // which kernel configuration of this size runs, on how many workgroups (wisdom, overrides, defaults)
    if (ops & GLV_OP_FFT) launch_plan(b, units, in_mode, ops, &pl.variant, &pl.grid);
    // GLV_OP_BARS: d_out receives the bars.  Stateful FFT chains whose rows are owned by whole waves compute
    // them inside the frame kernel from the finished row in LDS (the spectra never reach HBM, apart from
    // the state the operators keep anyway); otherwise the spectra stay internal -- in the gravity state
    // when the chain ends in gravity, in the scratch rows else -- and a bars kernel runs after.
    const bool snap = (ops & GLV_OP_BARS) && b->snapped();      // (check_ops: a GL chain's texel rows)
    pl.fused_bars = (ops & GLV_OP_BARS) && (ops & GLV_OP_FFT) && !gl_passes && bars_fusable(b, ops) && pl.variant < kMaxVariants
                    && (snap ? b->snap : b->bar).fusable[pl.variant];
    pl.out = d_out;
    if (ops & GLV_OP_BARS) {
        const bool state_is_output = (ops & GLV_OP_GRAVITY) && !(ops & (GLV_OP_AVERAGE | GLV_OP_SMOOTH | GLV_OP_RAW));
        if (pl.fused_bars || (state_is_output && !b->p.gl_storage)) pl.out = nullptr;
        else {
            if (!b->d_scratch) return fail(GLV_ERR_STATE, "this GLV_OP_BARS chain needs the internal spectra rows: announce it in glv_batch_create's ops_mask (GLV_OP_BARS together with the chain's other operators; GLV_OP_R16 too when a float chain's bars are wanted as texels)");
            pl.out = b->d_scratch;
        }
    }
    if (pl.route == ChainPlan::GL_PASSES) {
        // the frame kernel delivers the float spectra into the caller's buffer when that is what it will hold in the end, else into the
        // scratch rows; the GL passes write the caller's buffer (NULL: the state is the output), or the same rows when bars sample them
        pl.out = d_out && !(ops & (GLV_OP_BARS | GLV_OP_R16)) ? d_out : b->d_scratch;
        pl.rows = (ops & GLV_OP_BARS) ? pl.out : d_out;
    } else pl.rows = pl.out ? pl.out : b->d_grav;           // no rows out: a chain that ends in gravity, whose state is its output
    // many bars of texel rows: the integer matrix-core pass -- on the GL_R16 chain's texels, or on the texel values of the GL passes
    // gl_storage 3: the float chain writes the upload's texels (FC_R16 / FC_STATE_R16) and every second launch runs its texel-row kind (check_ops vetted the bars)
    const bool upload = (ops & GLV_OP_BARS) && upload_storage(b->p);
    const bool averaging = b->p.sample_mode == GLV_SAMPLE_AVERAGE;
    if (!(ops & GLV_OP_BARS) || pl.fused_bars) pl.bars = ChainPlan::NO_BARS;
    else if (upload) pl.bars = snap ? (b->columns() ? ChainPlan::BARS_COLUMNS_TEXELS : averaging ? ChainPlan::BARS_SNAP : ChainPlan::BARS_SNAP_MODE_TEXELS)
                                    : (averaging ? ChainPlan::BARS_I8 : ChainPlan::BARS_MODE_TEXELS);
    else if (snap && b->columns()) pl.bars = ChainPlan::BARS_COLUMNS;
    else if (snap) pl.bars = b->p.sample_mode != GLV_SAMPLE_AVERAGE ? ChainPlan::BARS_SNAP_MODE : pl.route == ChainPlan::GL_FUSED ? ChainPlan::BARS_SNAP : ChainPlan::BARS_SNAP_FLOATS;
    else if (b->p.bars >= glv::kBarSeqMin && b->bar_x.i8() && (pl.route == ChainPlan::GL_FUSED || (gl_passes && !(ops & GLV_OP_SMOOTH))))
        pl.bars = pl.route == ChainPlan::GL_FUSED ? ChainPlan::BARS_I8 : ChainPlan::BARS_I8_FLOATS;
    else pl.bars = ChainPlan::BARS_F32;
    if (pl.route == ChainPlan::GL_PASSES) pl.ops = frame_ops(b, ops);
    else {
        pl.ops = ops & ~(unsigned) (GLV_OP_PRIVATE_STATE | GLV_OP_OUTPUT_IS_STATE);
        if (ops & GLV_OP_BARS) pl.ops &= ~(unsigned) GLV_OP_R16;     // with bars the texel conversion applies to the bars, the spectra stay f32
        if (pl.bars == ChainPlan::BARS_I8 || pl.bars == ChainPlan::BARS_SNAP) pl.ops |= glv::OP_R16;   // ... but the GL_R16 chain hands the integer pass its rows as 16-bit texels
        if (upload && pl.bars != ChainPlan::NO_BARS) pl.ops |= glv::OP_R16;                            // ... and gl_storage 3 every second launch: the upload's texels
    }
    // the GL_R16 chain's rows go to the bars of a second launch and nowhere else (the scratch rows): what those bars do not sample is not stored
    // (gl_storage 3 likewise: the texel rows of the float-state classes)
    const uint32_t bins_needed = snap ? b->snap.bins : b->bar_x.bins_needed;
    if ((pl.route == ChainPlan::GL_FUSED || upload) && pl.bars != ChainPlan::NO_BARS && bins_needed != 0 && bins_needed < b->p.n)
        pl.out_limit = bins_needed * 4u;
    // GLV_OP_BARS_ONLY: ... and what they do not sample is not computed, nor is its state kept -- the GL_R16 chain, and a float chain with
    // the bars fused (check_ops vetted the call)
    if (b->live_bins() != 0 && (pl.route == ChainPlan::GL_FUSED || pl.fused_bars)) pl.live_points = b->live_bins() / 2u;
    pl.cls = glv::frame_class(pl.route == ChainPlan::GL_FUSED, pl.fused_bars, pl.live_points != 0, pl.ops, snap, snap && b->columns());
    return GLV_OK;
}

// bufscale > 1, the first launch of a process call: the caller's windows of k * n frames into the batch's staging rows (ChainPlan::dec_in; glv_decimate_kernel),
// which the chain then reads as planar rows.  A process call's windows lie back to back: one step, pitch k * n.
int decimate_stage(glv_batch* b, const ChainPlan& pl, hipStream_t st) {
    if (!pl.dec_in) return GLV_OK;
    glv::Decimate d = {};
    d.in = pl.dec_in; d.out = b->d_decim; d.n = b->p.n; d.k = b->bufscale; d.mono = b->p.channels == 1 ? 1u : 0u;
    d.w.pitch_frames = (uint64_t) b->bufscale * b->p.n; d.w.steps = 1; d.w.streams = pl.dec_streams;
    const hipError_t e = glv::launch_decimate(pl.dec_kind, d, st); ++b->last_launches;
    return e == hipSuccess ? GLV_OK : fail(GLV_ERR_HIP, "bufscale launch failed: %s", hipGetErrorString(e));
}

// Carries out a WAVE plan: one HIP-event window around its one or two launches; stream-ordered, nothing is allocated.
int run_wave(glv_batch* b, const ChainPlan& pl, const void* d_in, int in_mode, float* d_out, unsigned ops, uint32_t units, uint32_t rot, hipStream_t st) {
    const bool mono = b->p.channels == 1;
    if (int rc = timed_launch_begin(b, st)) return rc;
    if (int rc = decimate_stage(b, pl, st)) return rc;
    hipError_t e;
    if (pl.wave_fused) {
        const glv::BarIRowsTables irt = b->bar_x.irows_tables();
        e = glv::launch_bars_i8_pcm(d_in, rot, mono, d_out, units, b->p.n, b->p.bars, &irt, st, (ops & GLV_OP_R16) != 0);
        b->kernel_name = "glv_bars_rows_i8_kernel";
    } else {
        e = glv::launch_wave(d_in, in_mode, mono, b->p.n, rot, units, pl.out, pl.wave_r16, pl.wave_limit, st);
        b->kernel_name = "glv_wave_kernel";
    }
    ++b->last_launches;
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    if (!pl.wave_fused) if (int rc = launch_bars_pass(b, pl, d_out, units, (ops & GLV_OP_R16) != 0, st)) return rc;
    return timed_launch_end(b, st);
}

// Carries out a plan: the first kernel (and the GL passes), the batch's state bookkeeping, the smooth pass, the second bars launch --
// one HIP-event window around every launch of the chain.  Stream-ordered: launches and asynchronous device-to-device copies only.
int run_chain(glv_batch* b, const ChainPlan& pl, const void* d_in, int in_mode, float* d_out, unsigned ops, uint32_t units, uint32_t rot,
              hipStream_t st) {
    glv::FrameArgs a;
    fill_common(a, b->p, b->tab);
    a.in = d_in; a.out = pl.out; a.grav = b->grav_cur; a.grav_w = b->d_grav; a.hist = b->d_hist;
    a.units = units; a.ops = pl.ops; a.head = b->head; a.rot = rot; a.log_mode = b->p.log_mode;
    a.grav_sub = b->grav_sub; a.grav_int = b->grav_int ? 1u : 0u;
    a.bars_r16 = (ops & GLV_OP_BARS) && (ops & GLV_OP_R16) ? 1u : 0u;
    a.out_limit = pl.out_limit;
    // GLV_OP_OUTPUT_IS_STATE: a chain that ends in gravity writes ONE copy of its result (SURVEY 8d row B, 20 N bytes per frame) --
    // transform_gravity stores the same value to its `applied` array and to the buffer (render.c:733-734), so the caller's output
    // buffer can BE the state the next update reads.  Opt-in: the caller promises to leave the buffer alone until then.
    const bool gravity_only = (ops & GLV_OP_GRAVITY) && !(ops & GLV_OP_AVERAGE);
    const bool out_is_state = (ops & GLV_OP_OUTPUT_IS_STATE) != 0;           // check_ops vetted the chain
    if (out_is_state) {
        if ((const void*) d_out == d_in) return fail(GLV_ERR_INVALID, "GLV_OP_OUTPUT_IS_STATE: the output buffer must not be the input");
        a.grav_w = d_out; a.out = nullptr;
    }
    const float* grav_next = gravity_only ? (out_is_state ? d_out : b->d_grav) : b->grav_cur;
    if (pl.fused_bars) {
        const BarTableSet& t = b->snapped() ? b->snap : b->bar;   // (snapped: the uint32 weights W' travel as the bits of float weights; kernel class FC_GL16_SNAP*)
        a.bar_desc = t.desc; a.bar_items = t.fitems[pl.variant]; a.bar_nsteps = t.fnsteps[pl.variant]; a.bar_w = t.w;
        a.bars = b->p.bars; a.bars_out = d_out; a.col_map = b->snap_x.col_map;      // (NULL unless column texels are set)
    }
    if (pl.route == ChainPlan::GL_FUSED) a.gl_storage = 1;
    if (pl.route == ChainPlan::POST && (ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE))) a.gl_storage = upload_storage(b->p) ? 0u : b->p.gl_storage;   // the post kernel models it directly (3: the float operators)
    if (pl.route == ChainPlan::GL_PASSES && !pl.out)
        return fail(GLV_ERR_STATE, "this gl_storage chain needs the internal spectra rows (created for gl_storage 2 batches with state, and with GLV_OP_BARS in the ops_mask)");
    if (pl.live_points != 0) { a.live_points = pl.live_points; b->ran_live_over(b->live_bins()); }

    if (int rc = timed_launch_begin(b, st)) return rc;
    if (int rc = decimate_stage(b, pl, st)) return rc;
    hipError_t e = hipSuccess;
    if (pl.route == ChainPlan::POST || pl.route == ChainPlan::COPY) {
        if (in_mode != glv::IN_F32_PLANAR) return fail(GLV_ERR_INVALID, "operators without GLV_OP_FFT take planar f32 input");
        if (pl.route == ChainPlan::POST) { e = glv::launch_post(a, b->p.n, st); ++b->last_launches; }
        else if ((const void*) pl.out != d_in) e = hipMemcpyAsync(pl.out, d_in, sizeof(float) * (size_t) units * b->p.n, hipMemcpyDeviceToDevice, st);
        b->kernel_name = pl.route == ChainPlan::POST ? "glv_post_kernel" : "glv_smooth_kernel";
    } else {
        b->last_grid = pl.grid; b->last_variant = pl.variant;
        e = glv::launch_frame(b->log_nn, in_mode, (int) b->p.log_mode, pl.variant, pl.cls, a, pl.grid, st); ++b->last_launches;
        if (pl.route == ChainPlan::FRAME) b->kernel_name = "glv_frame_kernel";     // (the GL routes name it once every launch went through)
    }
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "kernel launch failed: %s", hipGetErrorString(e));
    if (pl.route == ChainPlan::GL_PASSES) {
        // the GL twin's pass structure (render.c:2188-2265): gravity / average as their own pass over GL_R16-quantised values
        // (glv_frame.h apply_state; state as floats with gl_storage 2, as texels with 1)
        glv::FrameArgs a2 = a;
        a2.in = pl.out; a2.ops = ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE | ((ops & GLV_OP_BARS) ? 0u : (unsigned) GLV_OP_R16)); a2.gl_storage = b->p.gl_storage;
        a2.out = pl.rows;
        e = glv::launch_post(a2, b->p.n, st); ++b->last_launches;
        if (e != hipSuccess) return fail(GLV_ERR_HIP, "GL-storage pass launch failed: %s", hipGetErrorString(e));
    }
    if (pl.route == ChainPlan::GL_FUSED || pl.route == ChainPlan::GL_PASSES) b->kernel_name = "glv_frame_kernel";
    if (ops & GLV_OP_AVERAGE) b->head = (b->head + 1) % b->p.avg_frames;
    b->grav_cur = grav_next;
    if (ops & GLV_OP_SMOOTH) {                     // render.c:694-718, in place on the finished rows (a SMOOTH chain always has them)
        e = glv::launch_smooth(pl.rows, units, b->p.n, b->d_smin, b->d_smax, b->smooth_asz, b->smooth_reach, b->smooth_window, st); ++b->last_launches;
        if (e != hipSuccess) return fail(GLV_ERR_HIP, "smooth launch failed: %s", hipGetErrorString(e));
    }
    if (int rc = launch_bars_pass(b, pl, d_out, units, (ops & GLV_OP_R16) != 0, st)) return rc;
    return timed_launch_end(b, st);
}

// What a call asks of the state the batch's earlier calls and glv_batch_set_params left, written once for process and the track executor.
// transform_gravity keeps ONE `applied` buffer per slot (render.c:724).  Here it lives in d_grav when gravity runs
// without average and in the newest ring slot when both run fused; a batch that mixed the two forms would silently
// continue from a stale state, so that is refused (reset the batch, or use one batch per operator chain).
int gravity_form(unsigned ops) { return !(ops & GLV_OP_GRAVITY) ? 0 : (ops & GLV_OP_AVERAGE) ? 2 : 1; }
}  // namespace
namespace glvh __attribute__((visibility("hidden"))) {
int refuse_gravity_mix(const glv_batch* b, unsigned ops) {
    const int mode = gravity_form(ops);
    if (mode == 0 || b->grav_mode == 0 || b->grav_mode == mode) return GLV_OK;
    return fail(GLV_ERR_STATE, "gravity was last applied %s average on this batch and is now requested %s it: the two forms keep "
                               "their state in different buffers (glv_batch_reset, or one batch per chain)",
                b->grav_mode == 2 ? "fused with" : "without", mode == 2 ? "fused with" : "without");
}
// ... committed once nothing can refuse the call any more
void commit_gravity_form(glv_batch* b, unsigned ops) {
    if (ops & GLV_OP_GRAVITY) b->grav_mode = gravity_form(ops);
}
int refuse_stale_tilt(const glv_batch* b) {
    if (b->tab.tilt_scale == b->p.fft_scale && b->tab.tilt_cutoff == b->p.fft_cutoff && b->tab.tilt_fold == (b->p.log_mode == 1)) return GLV_OK;
    return fail(GLV_ERR_STATE, "fft_scale / fft_cutoff / log_mode changed without glv_batch_set_params");
}

// One update of `units` channel rows through the fused kernel (or the post kernel when no FFT is asked).
// dec_in: bufscale > 1 -- d_in is the batch's staging rows, which the chain's first launch makes from the windows at dec_in (process_windows)
int process(glv_batch* b, const void* d_in, int in_mode, float* d_out, unsigned ops, uint32_t units,
            uint32_t rot, hipStream_t st, const void* dec_in, int dec_kind) {
    if (!d_in) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (int rc = check_ops(b, ops, d_out)) return rc;
    if (int rc = refuse_gravity_mix(b, ops)) return rc;
    b->last_launches = 0;
    HIP_TRY(hipSetDevice(b->device));
    ChainPlan pl;
    if (int rc = plan_chain(b, in_mode, ops, units, rot, d_out, pl)) return rc;
    if (int rc = refuse_stale_tilt(b)) return rc;
    pl.dec_in = dec_in; pl.dec_kind = dec_kind; pl.dec_streams = units / 2u;
    commit_gravity_form(b, ops);
    if (pl.route == ChainPlan::WAVE) return run_wave(b, pl, d_in, in_mode, d_out, ops, units, rot, st);
    return run_chain(b, pl, d_in, in_mode, d_out, ops, units, rot, st);
}

// The three process entries: the call as it has always run, or with bufscale > 1 the chain glv_batch_process_f32 plans on this batch for the same ops, over the
// staging rows its first launch decimates the caller's windows of k * n frames into.  Whatever the planar entry refuses is refused in its words, before anything
// is launched.
int process_windows(glv_batch* b, const void* d_in, int in_mode, int dec_kind, float* d_out, unsigned ops, hipStream_t st) {
    if (b->bufscale == 1u) return process(b, d_in, in_mode, d_out, ops, b->streams * 2, 0, st);
    if (!d_in) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (reinterpret_cast<uintptr_t>(d_in) & (dec_kind == glv::DEC_F32 ? 7u : 3u))
        return fail(GLV_ERR_INVALID, "the input must be aligned like its frames: %d bytes", dec_kind == glv::DEC_F32 ? 8 : 4);
    return process(b, b->d_decim, glv::IN_F32_PLANAR, d_out, ops, b->streams * 2, 0, st, d_in, dec_kind);
}
// ... and the three glv_batch_process_first_* entries: the same call on streams [0, count) -- 2 * count channel rows where process_windows passes all of the batch's.
// Every kernel takes its rows from the call (the grid is planned for them, a tuned grid clamped to them), so the rows behind are neither read nor written; head,
// the gravity form and the live flag are the batch's own and advance as for a full call.
int refuse_prefix(const glv_batch* b, const char* entry, uint32_t count) {
    if (count == 0 || count > b->streams) return fail(GLV_ERR_INVALID, "%s: count=%u: must be in [1, streams=%u]", entry, count, b->streams);
    if (b->single_row) return fail(GLV_ERR_STATE, "%s: a single-row batch (the drop-ins') has no streams to choose among", entry);
    return GLV_OK;
}
int process_first(glv_batch* b, uint32_t count, const void* d_in, int in_mode, int dec_kind, float* d_out, unsigned ops, hipStream_t st) {
    if (b->bufscale == 1u) return process(b, d_in, in_mode, d_out, ops, 2 * count, 0, st);
    if (!d_in) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (reinterpret_cast<uintptr_t>(d_in) & (dec_kind == glv::DEC_F32 ? 7u : 3u))
        return fail(GLV_ERR_INVALID, "the input must be aligned like its frames: %d bytes", dec_kind == glv::DEC_F32 ? 8 : 4);
    return process(b, b->d_decim, glv::IN_F32_PLANAR, d_out, ops, 2 * count, 0, st, d_in, dec_kind);
}
// What does not honour `setbufscale`: refused while k > 1, in the setter's name
int refuse_bufscale(const glv_batch* b, const char* entry) {
    if (b->bufscale == 1u) return GLV_OK;
    return fail(GLV_ERR_STATE, "%s does not take a batch with bufscale k=%u (glv_batch_set_bufscale): set k = 1, or use a batch of its own", entry, b->bufscale);
}
}  // namespace glvh
