/*
 * glv_spectrum.h -- C ABI of the MI355X-native GLava audio-spectrum path.
 *
 * Drop-in boundary for GLava's  fifo/pulse_input -> window -> FFT -> magnitude ->
 * gravity/average  pipeline.  Plain C: pointers, sizes, int status
 * returns.  No exceptions, no exit(), no torch/HIP types (a HIP stream is passed as
 * `void*`).  Every entry point names the reference interface it replaces; paths are
 * relative to the jarcode-foss/glava tree.
 *
 * The library is libglvspectrum.so (glava_amd/csrc), hand-written HIP for gfx950.  There
 * is NO CPU fallback: without a usable HIP device every compute entry point returns
 * GLV_ERR_NO_DEVICE and glv_last_error() says why.
 */
#ifndef GLV_SPECTRUM_H
#define GLV_SPECTRUM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GLV_ABI_VERSION 7      /* 5 (round 5): + glv_gl_texture; GLV_OP_BARS over texel rows (gl_storage != 0, 256 bars or more) is the exact integer mean
                                  6 (round 6): + GLV_OP_BARS_ONLY, glv_batch_live_bins, glv_batch_bars_arithmetic, glv_batch_tune_placement; GLV_OP_R16 in a creation mask is a hint
                                  7 (round 6): glv_params grew smooth_audio()'s shape -- round_formula, sample_mode, sample_hybrid_weight, sample_scale, sample_range
                                               (appended; all-zero == the shipped shape, so a caller that zero-fills the tail keeps ABI 6's results); GLV_BARS_F32_SEQ
                                  7, added without a version change: glv_batch_set_bar_texels (bars at texels of the pre-smoothing pass; detect it by the symbol),
                                               glv_batch_set_column_texels (the graph module's columns: means of three such texels; likewise),
                                               GLV_OP_WAVE and glv_wave_texture (the wave module's bind on the device; likewise) */

/* status codes (0 = ok).  The reference has no error channel: it prints and calls
 * glava_abort() (glava/glava.h:17, glava/render.c passim); the in-tree shim maps any
 * non-zero status to that. */
enum {
    GLV_OK = 0,
    GLV_ERR_INVALID = 1,     /* bad argument (n not a power of two in [256,32768], NULL, ...) */
    GLV_ERR_NO_DEVICE = 2,   /* no HIP device / kernels for gfx950 not loadable */
    GLV_ERR_HIP = 3,         /* a HIP runtime call failed; see glv_last_error() */
    GLV_ERR_NOMEM = 4,
    GLV_ERR_STATE = 5        /* operator used on a batch/state that lacks the required buffers */
};

/* Operator selection for the batched calls (bit set).  The order of application is
 * fixed and is the reference's: fft -> gravity -> average (glava/render.c:2140-2156). */
enum {
    GLV_OP_FFT      = 1u << 0,  /* window + FFT + abs/log/tilt   == transform_fft     render.c:783-847 */
    GLV_OP_GRAVITY  = 1u << 1,  /*                               == transform_gravity render.c:720-736 */
    GLV_OP_AVERAGE  = 1u << 2,  /*                               == transform_average render.c:738-771 */
    GLV_OP_RAW      = 1u << 3,  /* testing aid: with GLV_OP_FFT, skip abs/log/tilt and emit the raw
                                   interleaved (Re,Im) FFT output, which must be bit-identical to the
                                   reference's data[] at render.c:840 */
    GLV_OP_WRANGE   = 1u << 4,  /* (b+1)/2                       == transform_wrange  render.c:773-781;
                                   exclusive with GLV_OP_FFT (the wave module requests window,wrange) */
    GLV_OP_BARS     = 1u << 5,  /* smooth_audio() bin averaging + bar lookup (shaders/glava/util/
                                   smooth.glsl:13-64, radial/1.frag:58-70): emit `bars` values per
                                   channel instead of n bins; d_out is float [streams][2][bars].
                                   Inputs are clamped to [0, 1] (NaN -> 0) like the GL_R16 texels the shader
                                   samples; the taps' products are summed in a documented, fixed order (below 256
                                   bars: chunks of 16 / 32 / 64 taps by n, fused multiply-add chains; from 256 bars up -- the
                                   pre-smoothing pass, bars = n -- ONE fused multiply-add chain per bar in bin order, which the
                                   matrix cores compute: glava_amd/csrc/glv_frame.h "GLV_OP_BARS arithmetic";
                                   oracle/glv_oracle.c glvo_bars_chunked restates both) -- within 2e-4 relative of the
                                   shader's tap-by-tap loop, identical bits on every device path.  A bar whose weights
                                   sum to 0 is 0 / 0 as in the shader.  These are the `setsmoothpass false` bars (smooth_audio()
                                   averaging the spectrum at the bar positions); the shipped default's bars are texels of
                                   the pre-smoothed texture: glv_batch_set_bar_texels.
                                   Inside the GL chains (gl_storage != 0, gravity / average in the chain: the rows the bars sample are
                                   GL_R16 TEXELS, as in the reference's pre-smoothing pass, render.c:2277-2303) 256 bars or more are computed
                                   EXACTLY (ABI 5): per bar the shader's float weights w_j become integers W_j = llrint(w_j 2^P / sum w) with the
                                   first largest taking the residue so that sum W_j == 2^P (P = max(17, 21 + ceil(log2 sum w))), and
                                   texel = floor(sum W_j c_j / 2^P + 1/2) on the 16-bit texels c_j; without GLV_OP_R16 the float
                                   (float) ((double) sum W_j c_j 2^-P / 65535).  Integer arithmetic on the i8 matrix cores: no summation order,
                                   within 0.03 texel steps of the mean with the float weights in exact arithmetic
                                   (glava_amd/csrc/glv_tables.h make_bar_itiles; oracle/glv_oracle.c glvo_bars_int_at restates it) */
    GLV_OP_SMOOTH   = 1u << 6,  /* CPU-path log-window mean  == transform_smooth   render.c:694-718;
                                   applied last, in place on each row (after fft/gravity/average) */
    GLV_OP_MAGNITUDE = 1u << 7, /* the magnitude stage alone: b = (float)(log(|b| + 1.0f) / 3) * tilt(i),
                                   the tail of transform_fft (render.c:842-846) on planar f32 rows that
                                   already hold FFT output; exclusive with GLV_OP_FFT (which includes it);
                                   runs before gravity/average when combined with them */
    GLV_OP_R16      = 1u << 8,  /* output as GL_R16 texels: d_out is uint16 [streams][2][n] with
                                   texel = round_to_nearest_even(clamp(x, 0, 1) * 65535) -- what the only consumer of
                                   the spectra makes of them (handle_audio uploads every finished buffer with
                                   glTexImage1D(GL_TEXTURE_1D, 0, GL_R16, sz, 0, GL_RED, GL_FLOAT, buf), render.c:521-524).
                                   Applied last, to the output only: gravity / average state stays f32.  Halves the
                                   write side of the pass (8n instead of 12n bytes per s16 frame).  Alone (no other
                                   op) it quantises planar f32 rows.  With GLV_OP_BARS the bars are what is quantised (d_out:
                                   uint16 [streams][2][bars]; the spectra feeding them stay f32): with gl_storage = 1, bars = n and
                                   bar_phase = 0.5 that is the texture every stock module samples -- upload, gravity, average and
                                   pre-smoothing pass of render.c:2188-2303 in one call.  Excludes GLV_OP_RAW, GLV_OP_SMOOTH.
                                   In glv_batch_create's ops_mask (ABI 6) the bit is a HINT and nothing else: a FLOAT chain (gl_storage 0)
                                   with GLV_OP_BARS whose bars the transform kernel can compute itself gets the internal spectra rows --
                                   which only its bars AS TEXELS need (they leave through a second launch) -- only when the mask carries
                                   GLV_OP_R16 too; without it such a call is refused (GLV_ERR_STATE), with it nothing else changes. */
    GLV_OP_PRIVATE_STATE = 1u << 9, /* (ABI 3 flag, accepted and ignored since ABI 4: a batch-owned gravity state is the default again) */
    GLV_OP_RING_S16 = 1u << 10, /* glv_batch_create's ops_mask only: allocate (and zero, == the calloc'd rings of
                                   glava.c:487-494) the s16 device ring of glv_batch_ring_update_s16 / _append_s16; ring calls on
                                   a batch created without it are refused (GLV_ERR_STATE: nothing is allocated after creation) */
    GLV_OP_RING_F32 = 1u << 11, /* the same for the interleaved f32 ring of glv_batch_ring_update_f32 */
    GLV_OP_BARS_ONLY = 1u << 13, /* glv_batch_create's ops_mask only (ABI 6), with GLV_OP_BARS: the caller promises that every stateful call on this
                                   batch asks for GLV_OP_BARS -- the bars are all that is ever looked at (GLava's shipped pipeline: the modules sample
                                   the pre-smoothed texture and nothing else, smooth.glsl:62; BASELINE configs[2]: the radial module's bars).
                                   smooth_audio() samples bins below scale_audio(1) * n plus half a window (0.288 n with the shipped
                                   SAMPLE_RANGE 0.9 / SAMPLE_SCALE 8; glv_params.sample_range / sample_scale), so what the reference's passes compute beyond that is dead: the chain then keeps its gravity
                                   store and ring, and computes magnitude / upload / gravity / average, only for a compile-time share of the row
                                   that covers the bins the bars sample (3/8 of it; glv_batch_live_bins tells whether the batch runs that way) --
                                   15 n instead of 28 n bytes per frame at n = 4096, F = 5 on GL_R16 state.  Live kernel classes exist for the
                                   GL_R16 chains (gl_storage 1: bars in a second launch or fused) and for float chains whose bars the transform
                                   kernel computes itself (fewer than 256 bars, every kernel configuration of the size fusable); any other
                                   batch (and log_mode 2) runs the full chain: the bars are bit-identical either way (no smooth_factor makes a
                                   bar sample further: smooth_audio() clamps its positions to [0, 1]).  A stateful call without GLV_OP_BARS and glv_batch_gravity_state are refused
                                   (GLV_ERR_STATE); so is a glv_batch_set_params (or a texel table) that would take a batch which has run its live class to the
                                   full chain or to live bins beyond what its live calls have kept (glv_stream_state_desc.kept_bins: the state beyond
                                   was never kept; shrinking and growing back within it are accepted) -- until glv_batch_reset */
    GLV_OP_WAVE     = 1u << 14, /* the wave module's bind (shaders/glava/wave/1.frag:7-9 requests `window`, `wrange`; `window` has no CPU stage,
                                   render.c:850): per channel row the backend's unpack (fifo.c:94-110 / pulse_input.c:155-178; channels == 1: the mono mix
                                   into both rows; planar f32 rows are taken as they are), transform_wrange (render.c:773-781: b += 1.0F; b /= 2.0F) and
                                   the GL_R16 upload (render.c:521-524, :2185) -- from EVERY input entry point (s16 / f32 interleaved frames, planar f32,
                                   both device rings, oldest frame first), stateless.  Outputs:
                                     GLV_OP_WAVE | GLV_OP_R16     uint16 [streams][2][n]: the upload's texels c
                                     GLV_OP_WAVE                  float  [streams][2][n]: c / 65535 correctly rounded -- what texelFetch returns, the texture the
                                                                  module samples with `setsmoothpass false`
                                     GLV_OP_WAVE | GLV_OP_BARS [| GLV_OP_R16]   the pre-smoothing pass over those texels (audio is true for SRC_AUDIO_L/R,
                                                                  render.c:2325-2326, so handle_audio runs it on the waveform too: render.c:2276-2303,
                                                                  util/smooth_pass.frag): arithmetic and outputs exactly what GLV_OP_BARS documents for the
                                                                  GL_R16 chain -- GLV_BARS_I8_EXACT for sample_mode average at 256 bars or more,
                                                                  GLV_BARS_F32_SEQ for maximum / hybrid (glv_batch_bars_arithmetic reports it).  With bars = n,
                                                                  bar_phase = 0.5 and GLV_OP_R16 that is the texture the shipped wave module samples
                                                                  (wave/1.frag:17-23).  From s16 frames and the s16 ring (its oldest frame at a multiple of 8), GLV_BARS_I8_EXACT runs as ONE launch:
                                                                  the integer pass unpacks, applies wrange and quantises the frames as it parks them in LDS,
                                                                  reading only the frames its bars sample; every other form is the waveform kernel into rows
                                                                  made at creation, then the bars kernel (glv_batch_last_launches reports which;
                                                                  GLV_UNFUSED_WAVE in the environment at creation forces two launches: diagnostics).
                                                                  Measured (tools/wave_texture_bench.py, profiles/r09/wave_texture.txt: one MI355X, 65536
                                                                  streams, N = 4096, HIP events around every launch, medians of 7 rounds of 20 calls): one
                                                                  launch 0.724 ms per call, two launches 0.723 ms (90.5 / 90.6 M frames/s) -- no difference
                                                                  beyond the spread (0.046 / 0.003 ms); for orientation the GL chain's pre-smoothing launch over
                                                                  the same 131072 rows is 0.48 ms.  The one-launch form stays the default: it is no slower and
                                                                  needs no rows between launches.  glv_batch_track_wave_s16 inherits it.
                                   A new bit: every call without it is what it was.  Refused: with GLV_OP_FFT / GRAVITY / AVERAGE / RAW / WRANGE / MAGNITUDE /
                                   SMOOTH / OUTPUT_IS_STATE (GLV_ERR_INVALID); GLV_OP_WAVE | GLV_OP_BARS on a gl_storage 0 batch (GLV_ERR_STATE: a float chain has
                                   no texel rows -- true of 0, the operators alone; gl_storage 3 adds the upload and takes the call exactly as 1 does), on a batch whose ops_mask lacked either bit (GLV_ERR_STATE: the rows between the two launches are made at
                                   creation); any GLV_OP_WAVE call, with or without bars, while column texels are set (GLV_ERR_STATE: the wave shader does not average three texels).  With bar texels set
                                   (glv_batch_set_bar_texels) GLV_OP_WAVE | GLV_OP_BARS gives the texels of the pass at the table's positions */
    GLV_OP_OUTPUT_IS_STATE = 1u << 12 /* opt-in, with a chain that ENDS in gravity (GLV_OP_GRAVITY without AVERAGE / SMOOTH / RAW, f32
                                   rows out, no gl_storage): transform_gravity stores every value twice, to its `applied` array and to
                                   the buffer (render.c:733-734) -- with this flag ONE array is kept: the call writes the spectra
                                   once, into d_out, and the NEXT update of the batch reads its `applied` values from there.  The
                                   caller promises to leave that buffer intact until the next update has been issued (the same
                                   buffer every time, or several in rotation; stream order is all the synchronisation needed) and
                                   not to alias it with the input.  The chain then moves SURVEY 8d row B's 20 n bytes per frame
                                   instead of 28 n.  Without the flag the state lives in a buffer the batch owns (the default: a
                                   caller may post-process, reuse or free d_out at will) */
};
/* Bits glv_batch_create's ops_mask understands: GLV_OP_GRAVITY / GLV_OP_AVERAGE (state arrays), GLV_OP_BARS (the internal
 * spectra rows, where the announced chain cannot compute its bars inside the transform's launch), GLV_OP_SMOOTH, GLV_OP_RING_S16 /
 * GLV_OP_RING_F32 (device rings).  The tables are cheap and always made at creation (tilt, bar taps and work lists, smooth
 * bounds: an operator the mask did not announce only goes without them when its parameters are unusable); buffers of spectrum
 * size are made for announced operators only.  The process calls themselves never allocate, never copy synchronously, change no
 * function attribute, and can be captured into a hipGraph from the first one on; an operator whose buffers the batch was not
 * created with is refused with GLV_ERR_STATE. */

/* Mirrors the fields of the private `struct gl_data` that the path reads
 * (glava/render.c:166-207) and of `struct audio_data` (glava/fifo.h:9-20). */
typedef struct glv_params {
    uint32_t n;             /* audio_buf_sz / bsz: real samples per channel; power of two in [256, 32768]
                               (#request setbufsize, render.c:1176).  Complex FFT length is n/2 (render.c:786) */
    uint32_t channels;      /* 2 = stereo, 1 = mirror/mono mix (fifo.c:98-102, setmirror render.c:1053) */
    float fft_scale;        /* render.c:845, default 10.2 (render.c:930) */
    float fft_cutoff;       /* render.c:845, default 0.3  (render.c:931) */
    float gravity_step;     /* render.c:728, default 4.2  (render.c:911) */
    float ur;               /* updates per second used by gravity (render.c:728); the reference measures it
                               (render.c:2387); ideal value rate/(sample_sz/4).  Like the reference, any value is
                               taken: 0 (an interval without updates) makes the step infinite and the output -inf.
                               The reference starts at 1.0F (render.c:906) and replaces it by ucounter / tcounter each time a
                               second of frame durations has passed (render.c:2379-2399): a live GLava never runs at the
                               ideal value.  A track call that follows it: glv_batch_track_rates_s16 / _f32 */
    uint32_t avg_frames;    /* F, render.c:743; 1..GLV_MAX_AVG_FRAMES */
    uint32_t avg_window;    /* bool, render.c:745/765 */
    uint32_t avg_window_kind; /* 0: CPU twin 0.6/0.4, oldest-first (render.c:661,751-766)
                                 1: GL twin 0.53836/0.46164, newest-first (common.glsl:13, average_pass.frag:19-45,
                                    render.c:2247-2256) */
    uint32_t log_mode;      /* render.c:844 evaluates log() in fp64 and divides by 3 in fp64, then rounds to float:
                               1: (default) hardware log2 * (ln2/3 * tilt) in fp32: <= 1.8e-7 relative error
                                  against the reference's float on EVERY float input of the stage (exhaustive
                                  test, tests/test_gpu_parity.py::test_magnitude_stage_every_float; bar 1e-5).  At n >= 16384
                                  the factor ln2/3 * tilt itself comes from one fused multiply-add per value (<= 4.5e-7 from
                                  the reference's thrice-rounded product): <= 6.3e-7 in total
                               0: bit-faithful: fp64 table-driven log (rel. error ~2^-50) and fp64 /3 -- the
                                  reference's float result on every input of the same exhaustive test
                               2: audit: device libm fp64 log + true fp64 division (slow) */
    /* GLV_OP_BARS parameters (shaders/glava/smooth_parameters.glsl) */
    uint32_t bars;          /* bars per channel (radial.glsl:9 NBARS 160 => 80) */
    float smooth_factor;    /* SMOOTH_FACTOR, smooth_parameters.glsl:72, default 0.025 */
    /* GLV_OP_SMOOTH parameters (render.c:917-918, #request setsmooth / setsmoothratio render.c:1201-1206) */
    float smooth_distance;  /* default 0.01 */
    float smooth_ratio;     /* default 4 */
    uint32_t gl_storage;    /* 0 (default): gravity / average keep float state, like the CPU operators (render.c:720-771).
                               1: the storage of the GL passes is modelled (render.c:2188-2265 with setaccelfft, GLava's shipped
                               default rc.glsl:211: every intermediate is a GL_R16 texture, render.c:523, :1718): the uploaded
                               buffer, the gravity store after each step and the average are clamped to [0, 1] and quantised to 16
                               bits; no averaging pass when avg_frames == 1 (render.c:2230).  Usually combined with
                               avg_window_kind = 1.  The state IS kept as 16-bit texels (uint16 store and ring) and an FFT chain
                               runs as ONE launch: upload quantisation, GL_MAX + gravity pass, ring copy and average pass are the
                               transform kernel's epilogue (with GLV_OP_BARS, where a row's bars fit, also the bars); the output is
                               GL_R16 texels (GLV_OP_R16) or their floats c / 65535.  28 n bytes per frame at avg_frames = 5.
                               2: the same values, pass by pass as the reference runs them: the transform writes f32 spectra, a
                               second kernel applies gravity / average on f32 state (every value a float c / 65535).  Bit-identical
                               to 1 on every input; kept as the checker of 1 and for the chains 1 does not fuse.
                               3 (added within ABI 7; detect it by glv_batch_create accepting the value): GLava with `setaccelfft false`.
                               The CPU operators on float state exactly as with 0 -- float rows out, GLV_OP_R16 texels out and the
                               state afterwards are gl_storage 0's in every bit (render.c:2149-2155) -- and then the GL_R16 upload of
                               the finished buffer (render.c:2185, :521-524), which is what GLV_OP_BARS samples: with c[i] =
                               unorm16(row[i]) the texels of the finished float row of an FFT chain (with or without gravity /
                               average), the call's output is what the GL chains define over texel rows c in the arithmetic
                               glv_batch_bars_arithmetic reports -- sample_mode average at 256 bars or more: GLV_BARS_I8_EXACT
                               (with bars = n, bar_phase 0.5 the pre-smoothing pass of render.c:2276-2303); bar texels
                               (glv_batch_set_bar_texels) and column texels (glv_batch_set_column_texels): the texels / the
                               column_mean of three texels of that pass over the same rows; sample_mode maximum / hybrid:
                               GLV_BARS_F32_SEQ over x = c / 65535, with or without a table, at any bar count.  GLV_OP_WAVE |
                               GLV_OP_BARS as with 1.  Not offered (the non-shipped `setsmoothpass false` / `setsmooth` corners,
                               GLV_ERR_STATE): unsnapped averaging bars below 256 (or without integer tables), GLV_OP_SMOOTH or
                               GLV_OP_RAW together with GLV_OP_BARS, GLV_OP_BARS without GLV_OP_FFT, and glv_batch_bars on
                               caller's rows; without GLV_OP_BARS, GLV_OP_SMOOTH is what it is on 0.  A GLV_OP_BARS_ONLY batch has
                               no live bins (glv_batch_live_bins 0) and runs the full chain with the same results.  Routes
                               (glv_batch_last_launches): bar texels and columns in ONE launch where the GL_R16 chain fuses them
                               (kernel classes FC_STATE_SNAP / FC_STATE_COLS: the finished float row in LDS is sampled through the
                               upload's quantiser), else two: the float-state kernel writes the upload's texels of the bins the
                               bars sample into the internal rows, then glv_bars_rows_i8_kernel / glv_bars_snap_kernel /
                               glv_columns_kernel / glv_bars_mode_kernel (texel-row kinds) run on them.
                               The storage class (1 vs 0 / 2 / 3) is fixed when a batch or state is created. */
    float bar_phase;        /* GLV_OP_BARS evaluates smooth_audio() at idx = (k + bar_phase) / bars, k = 0 .. bars-1.
                               0 (default): the bar positions of the modules (radial/1.frag:58-70: pos = k / (NBARS / 2)) with the
                               `setsmoothpass false` semantics -- smooth_audio() averaging the spectrum at those positions.  With
                               setsmoothpass true (GLava's default) the shipped modules fetch texels of the pre-smoothed texture
                               instead: those bars come from glv_batch_set_bar_texels (bar_phase is then ignored).
                               0.5 with bars == n: the texel centres of the reference's pre-smoothing pass
                               (util/smooth_pass.frag: smooth_audio(tex, sz, gl_FragCoord.x / w), render.c:2277-2303) -- the
                               texture every stock module samples when setsmoothpass is on (the default) */
    /* smooth_audio()'s SHAPE (ABI 7): the GLSL `#define`s of shaders/glava/smooth_parameters.glsl:17-42, which a user overrides in
     * ~/.config/glava/smooth_parameters.glsl or a module's config (the reference re-defines them textually, glsl_ext.c:143-157).  0 in every
     * field is the shipped shape.  GLV_OP_BARS evaluates exactly this smooth_audio(); integration/glava_hip_shim.c reads the defines out of
     * the processed shader text the host compiles. */
    uint32_t round_formula; /* ROUND_FORMULA (smooth_parameters.glsl:17, the macros of util/common.glsl:17-22):
                               GLV_ROUND_SINUSOIDAL 0 (shipped), GLV_ROUND_CIRCULAR 1, GLV_ROUND_LINEAR 2 */
    uint32_t sample_mode;   /* SAMPLE_MODE (smooth_parameters.glsl:28; smooth.glsl:9-11, :32-59):
                               GLV_SAMPLE_AVERAGE 0 (shipped): the weighted mean over s = smin; s <= smax -- every arithmetic GLV_OP_BARS documents above;
                               GLV_SAMPLE_MAXIMUM 1: max over s = smin; s < smax of fl(x_j * w_j), from +0 (order-free: bit-exact by construction);
                               GLV_SAMPLE_HYBRID  2: fl(fl(vmax * fl(1 - H)) + fl(fl(avg / weight) * H)) with v_j = fl(x_j * w_j), vmax their maximum,
                                  avg = ONE chain of float additions of the v_j in bin order from +0 (the shader's loop as written, no fused
                                  multiply-add), weight the tap-order float sum of the w_j; s < smax.
                               Modes 1 and 2 run one lane per bar and row (glv_bars_mode_kernel), never inside the transform's launch and never on the
                               matrix cores (a maximum is not a matrix product); texel rows (gl_storage != 0) enter as x = c / 65535 in float (what
                               texelFetch returns) and leave, with GLV_OP_R16, as round_to_nearest_even(clamp(bar, 0, 1) * 65535) */
    float sample_hybrid_weight; /* SAMPLE_HYBRID_WEIGHT, smooth_parameters.glsl:31; 0 = the shipped 0.65; (0, 1] */
    float sample_scale;     /* SAMPLE_SCALE, smooth_parameters.glsl:35; 0 = the shipped 8 */
    float sample_range;     /* SAMPLE_RANGE, smooth_parameters.glsl:40; 0 = the shipped 0.9.  scale_audio(1) = -log(1 - range) / scale must not
                               exceed 1 (the shader would fetch texels beyond the texture: undefined in GL, GLV_ERR_INVALID here) */
} glv_params;
enum { GLV_ROUND_SINUSOIDAL = 0, GLV_ROUND_CIRCULAR = 1, GLV_ROUND_LINEAR = 2 };
enum { GLV_SAMPLE_AVERAGE = 0, GLV_SAMPLE_MAXIMUM = 1, GLV_SAMPLE_HYBRID = 2 };

#define GLV_MAX_AVG_FRAMES 64

/* Fill `p` with the shipped defaults (shaders/glava/rc.glsl:181-211,
 * shaders/glava/smooth_parameters.glsl:46-67): n=4096, stereo, 10.2/0.3, 4.2,
 * ur = 22050/256, F=5 windowed. */
void glv_params_default(glv_params* p);

/* Version / diagnostics. */
int         glv_abi_version(void);
const char* glv_last_error(void);          /* thread-local, never NULL */
int         glv_device_count(void);        /* 0 when no HIP device is usable */

/* ------------------------------------------------------------------------------------
 * 1. Single-stream drop-ins (host pointers, in place).  Same shape as the reference's
 *    operator seam  void apply(struct gl_data*, void** udata, void* data)
 *    (glava/render.c:106-118, table at :849-856).  `glv_state` replaces the `*udata`
 *    slot (lazily calloc'd by the reference, render.c:662-666, and free()d by
 *    rd_destroy, render.c:2463-2469); here it is created/destroyed explicitly.
 * ------------------------------------------------------------------------------------ */
typedef struct glv_state glv_state;   /* per (channel, stream) device-side gravity + history state */

int glv_state_create(const glv_params* p, int device, glv_state** out);
int glv_state_reset(glv_state* s);            /* zero gravity/history (== fresh calloc) */
int glv_state_destroy(glv_state* s);

/* == transform_fft(gl, _, &(struct gl_sampler_data){buf, p->n})   glava/render.c:783-847 */
int glv_fft(const glv_params* p, glv_state* s, float* buf);
/* == transform_gravity                                             glava/render.c:720-736 */
int glv_gravity(const glv_params* p, glv_state* s, float* buf);
/* == transform_average                                             glava/render.c:738-771 */
int glv_average(const glv_params* p, glv_state* s, float* buf);
/* == transform_wrange                                              glava/render.c:773-781 */
int glv_wrange(const glv_params* p, glv_state* s, float* buf);
/* == transform_smooth                                              glava/render.c:694-718 */
int glv_smooth(const glv_params* p, glv_state* s, float* buf);
/* == the magnitude tail of transform_fft alone (abs, +1, log/3, tilt) glava/render.c:842-846 */
int glv_magnitude(const glv_params* p, glv_state* s, float* buf);
/* fft -> gravity -> average in one launch (what handle_audio does per bind, render.c:2140-2156) */
int glv_fft_gravity_average(const glv_params* p, glv_state* s, float* buf);
/* the GL_R16 texels glTexImage1D(..., GL_R16, ..., GL_FLOAT, buf) stores for buf[0..n) (render.c:521-524):
 * texels[i] = round_to_nearest_even(clamp(buf[i], 0, 1) * 65535); buf is not modified */
int glv_texels_r16(const glv_params* p, glv_state* s, const float* buf, uint16_t* texels);
/* == the accel_fft branch of handle_audio, from the per-frame transform_fft to the texture the module samples (glava/render.c:2176-2303,
 * GLava's shipped configuration: rc.glsl:211 setaccelfft true, smooth_parameters.glsl:78 setsmoothpass true): transform_fft of the n samples
 * in buf (not modified), the GL_R16 upload (:521-524), GL_MAX store + gravity pass (:2199-2228), ring copy + average pass (:2230-2265; none
 * when avg_frames == 1) and -- smooth_pass != 0 -- the pre-smoothing pass (:2277-2303, util/smooth_pass.frag) on 16-bit state: one launch
 * (+ one for the pre-smoothing pass).  texels: the n GL_R16 texels the last pass's render target holds -- upload them with
 * glTexImage1D(GL_TEXTURE_1D, 0, GL_R16, n, 0, GL_RED, GL_UNSIGNED_SHORT, texels).  The state must have been created with gl_storage = 1
 * (normally avg_window_kind = 1; for the pre-smoothing pass bars = n and bar_phase = 0.5); it holds the gravity store and the ring like
 * the reference's gr_store / gr.out textures do.  integration/render_hip.patch binds this into handle_audio. */
int glv_gl_texture(const glv_params* p, glv_state* s, const float* buf, int smooth_pass, uint16_t* texels);
/* == handle_audio for a bind whose transforms are `window`, `wrange` -- the wave module's (shaders/glava/wave/1.frag:7-9) --, from the CPU transform
 * to the texture the module samples (glava/render.c:2113-2309): transform_wrange of the n floats in buf (lb / rb; not modified; render.c:773-781),
 * the GL_R16 upload (:521-524, :2185) and -- smooth_pass != 0, the shipped default (smooth_parameters.glsl:78) -- the pre-smoothing pass
 * (:2276-2303) in its exact integer form (GLV_OP_BARS, GLV_BARS_I8_EXACT).  texels: the n GL_R16 texels of the upload or of the pass; the module
 * reads them with texture(audio_l, (gl_FragCoord.x + o) / screen.x), o in {-1, 0, 1}, GL_NEAREST / GL_REPEAT (wave/1.frag:17-23, render.c:1714-1717;
 * glava_amd.bar_positions.wave_column_texels restates the mapping).  GLV_OP_WAVE [| GLV_OP_BARS] | GLV_OP_R16 on one row.  The pass needs a state
 * created with gl_storage = 1, bars = n and bar_phase = 0.5 (GLV_ERR_STATE / GLV_ERR_INVALID otherwise); smooth_pass == 0 works on any state.
 * Added within ABI 7 without a version change: detect it by the symbol.  integration/render_hip.patch does not bind it yet. */
int glv_wave_texture(const glv_params* p, glv_state* s, const float* buf, int smooth_pass, uint16_t* texels);

/* == the unpack loop of the FIFO backend, glava/fifo.c:94-110 (and :67-79 when pcm == NULL):
 * `frames` interleaved stereo s16 frames -> planar f32.  Runs on the device (the bit-exactness
 * of int16 -> f32 /65535f is part of the parity contract). */
int glv_unpack_s16(int device, const int16_t* pcm, size_t frames, int channels, float* l, float* r);

/* rd_update prelude on device buffers (glava/render.c:1765-1809); stream-ordered, no state:
 *   bufscale  d_out[r][t] = mean(d_in[r][t*k .. t*k+k-1]), float accumulation (render.c:1768-1781)
 *   lerp      d_out = d_start + (d_end - d_start) * min(uratio * kcounter, 1)   (render.c:1794-1809) */
int glv_prelude_bufscale(int device, const float* d_in, float* d_out, size_t rows, uint32_t n_out, uint32_t k, void* hip_stream);
int glv_prelude_lerp(int device, const float* d_start, const float* d_end, float* d_out, size_t count,
                     float uratio, int kcounter, void* hip_stream);

/* ------------------------------------------------------------------------------------
 * 2. Batched extension (device pointers, stream-ordered).  No reference counterpart:
 *    B independent stereo streams, one update ("frame") of every stream per call.
 *    Layouts (row-major):
 *      d_pcm   int16 [streams][n][2]     interleaved LRLR, exactly the bytes a FIFO delivers
 *      d_f32   float [streams][2][n]     planar, what glava.c:528-537 snapshots into lb/rb
 *      d_spec  float [streams][2][n]     out; index 2k = |Re Z_k| path, 2k+1 = |Im Z_k| path
 *      d_bars  float [streams][2][bars]  out when GLV_OP_BARS
 *    State (gravity [streams][2][n], history ring [streams][2][F][n]) is owned by the
 *    batch and allocated according to `ops_mask` given at creation.
 * ------------------------------------------------------------------------------------ */
/* device memory for C hosts that do not want the HIP headers (the audio backend of INTEGRATION.md section 2):
 * thin wrappers over hipMalloc / hipFree / hipMemcpyAsync on `device`; copies are ordered on hip_stream
 * (NULL = the default stream) and glv_device_sync waits for it. */
int glv_device_malloc(int device, size_t bytes, void** d_ptr);
int glv_device_free(int device, void* d_ptr);
int glv_device_upload(int device, void* d_dst, const void* h_src, size_t bytes, void* hip_stream);
int glv_device_download(int device, void* h_dst, const void* d_src, size_t bytes, void* hip_stream);
int glv_device_sync(int device, void* hip_stream);

typedef struct glv_batch glv_batch;

int glv_batch_create(const glv_params* p, uint32_t streams, unsigned ops_mask, int device, glv_batch** out);
/* Change the scalar knobs of a batch (fft_scale, fft_cutoff, gravity_step, ur, avg_window*, log_mode, channels, bars,
 * smooth_*, bar_phase, gl_storage among 0, 2 and 3): regenerates and uploads whatever tables depend on them -- synchronously; this is the
 * only place besides creation that allocates or copies.  n, avg_frames and the state's storage class (gl_storage == 1 or not)
 * are fixed at creation (GLV_ERR_STATE: moving to or from 1).  State (gravity, history, rings) is kept. */
int glv_batch_set_params(glv_batch* b, const glv_params* p);
int glv_batch_reset(glv_batch* b);
int glv_batch_destroy(glv_batch* b);

/* one update of every stream from s16 PCM already resident in HBM.  Stream-ordered: nothing is allocated, nothing is copied
 * synchronously; the call can be captured into a hipGraph.
 *
 * Chains that end in gravity (GLV_OP_GRAVITY without AVERAGE / SMOOTH / RAW): the state lives in a buffer the batch owns and
 * d_out receives a copy (28 n bytes per frame); d_out may be NULL -- the spectra are then left in the state buffer only, read
 * them through glv_batch_gravity_state (20 n).  With GLV_OP_OUTPUT_IS_STATE d_out itself becomes the state (20 n; see the flag
 * for what the caller promises).  (With GLV_OP_BARS a chain ending in gravity keeps the spectra in the state internally.) */
/* (every input entry point -- this one, _f32, _f32_stereo and the two ring updates -- takes GLV_OP_FFT chains or GLV_OP_WAVE; planar f32 also the operators
 * without a transform) */
int glv_batch_process_s16(glv_batch* b, const int16_t* d_pcm, float* d_out, unsigned ops, void* hip_stream);
/* Track mode: `steps` consecutive updates of every stream in ONE call, from a recording whose every hop is already in HBM -- the time axis as the
 * parallel one.  Added within ABI 7 without a version change: detect it by the symbol.
 *   d_pcm   int16 [streams][pitch_frames][2]; window t of stream s = its frames [t * hop, t * hop + n)
 *   d_out   step-major: d_out + t * (bytes one glv_batch_process_s16 call with these ops writes) is EXACTLY what call t would have written
 *   d_work  caller-owned workspace of at least glv_batch_track_work_bytes(...) bytes, 256-byte aligned; its contents mean nothing between calls
 * Contract: the output of step t and the batch's state afterwards -- gravity store, history ring, ring head, which gravity form the batch is in -- are
 * bit for bit what `steps` consecutive glv_batch_process_s16(b, window_t, out_t, ops, st) calls produce and leave behind.  So a track may be cut into
 * chunks (track(4) then track(7) == track(11)), track calls mix with process / ring calls on the same batch, and the state a call starts from is
 * whatever the batch holds.
 * Accepted: GLV_OP_FFT (required; alone it is a spectrogram) with GLV_OP_GRAVITY / AVERAGE / BARS / R16 in the combinations glv_batch_process_s16 takes,
 * on gl_storage 0 and 1, channels 1 and 2, every log_mode, GLV_OP_BARS with and without a bar-texel table (glv_batch_set_bar_texels).
 * gl_storage 3 (added within ABI 7): every track entry -- this one, glv_batch_track_windows_*, _columns_*, _live_* (the full-row form: such a batch has no live
 * bins), _at_*, _rates_* and the wave entries -- takes such a batch under its own contract, word for word: the stateless transform writes float rows (texel
 * rows where no state follows and bars do), the scan runs its float-state form and writes the upload's texels for GLV_OP_BARS, and the texel-row bars /
 * snap / columns / mode kernel follows; the workspace queries follow those element sizes (float rows in the first region, texel rows in the second).
 * Refused: GLV_ERR_INVALID -- GLV_OP_RAW / SMOOTH / WAVE / WRANGE / MAGNITUDE / OUTPUT_IS_STATE, steps == 0, hop not a power of two in [4, n],
 * pitch_frames % hop != 0, pitch_frames < n + (steps - 1) * hop, a NULL pointer, a workspace that is not 256-byte aligned, more than 2^32 rows in one
 * call; GLV_ERR_STATE -- gl_storage 2 (the checker form), a batch created with GLV_OP_BARS_ONLY (its state beyond the live bins does not exist),
 * column texels set, and everything glv_batch_process_s16 refuses (the gravity form mix, unannounced state, parameters changed without
 * glv_batch_set_params).  A refused call leaves the batch untouched.
 * Stream-ordered: kernels and nothing else -- nothing is allocated or synchronised, the first call can be captured into a hipGraph.  Three stages:
 *   1. n / hop launches of the stateless transform kernel.  The frame sequence [0, (streams - 1) * pitch_frames + (steps - 1) * hop + n) is taken as one:
 *      launch r transforms the back-to-back windows that start at r * hop + k * n, so window (s, t), which starts at s * pitch_frames + t * hop, is row
 *      k = start / n of launch r = (start % n) / hop.  Windows that straddle two streams, and those between a stream's last step and the next stream, are
 *      computed and never read: the transform's work follows streams * pitch_frames, not streams * steps -- give a multi-stream recording a pitch close
 *      to what the call consumes.  No launch reads past the last window of the last stream.
 *   2. glv_track_scan_kernel (glv_batch_kernel_name): one lane per bin pair walks the steps with the gravity value in a register and the F-slot ring
 *      in LDS; the batch's state arrays are read once before the first step and written once after the last.
 *   3. with GLV_OP_BARS the bars kernel of a second launch over steps * streams * 2 finished rows (identical bits on every device path).
 * glv_batch_last_launches: n / hop + 1, + 1 with GLV_OP_BARS.
 * Measured against the same updates issued one by one (tools/track_bench.py; profiles/r10/track.txt: one MI355X, N = 4096, hop 256, the GL chain with
 * F = 5 and the pre-smoothing pass, texels out, 2048 steps; a host clock around the calls and the synchronise that ends them): 1 stream 2.10 ms against
 * 41.3 ms (19.7 x), 8 streams 2.60 against 44.6 ms (17.1 x), 64 streams 6.00 against 46.1 ms (7.7 x); 1024 streams, 256 steps, 8.42 against 10.7 ms
 * (1.27 x).  The one-by-one form costs ~20 us per update whatever it carries until the chip fills; the two forms had not crossed at 1024 streams, the
 * largest count measured -- beyond it nothing is known, and the workspace (8 GiB there) grows with streams * steps. */
uint64_t glv_batch_track_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops);   /* 0 on arguments the call refuses: glv_last_error then starts with the code's name, "GLV_ERR_INVALID: " or "GLV_ERR_STATE: " */
int glv_batch_track_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                        unsigned ops, void* hip_stream);
/* Track mode at ANY hop: the transform reads each window where it lies in the recording.  Added within ABI 7 without a version change: detect them by
 * the symbol.  glv_batch_track_s16 above is unchanged.
 *   d_pcm   int16 [streams][pitch_frames][2], aligned like any int16 frame pointer (4 bytes: a seek to an odd frame of a recording is a valid argument);
 *           window t of stream s = its frames [t * hop, t * hop + n).  hop is ANY value >= 1 (a renderer's is rate / fps: 735 at 44.1 kHz and 60 fps, 1470,
 *           800), hop > n included; pitch_frames >= n + (steps - 1) * hop and nothing else is asked of it.
 *   d_out, d_work, ops: as for glv_batch_track_s16.
 * Contract: glv_batch_track_s16's, word for word -- the output of step t and the batch's state afterwards (gravity store, history ring, ring head, which
 * gravity form the batch is in) are bit for bit what `steps` consecutive glv_batch_process_s16(b, window_t, out_t, ops, st) calls produce and leave behind.
 * So chunks compose, calls mix with process / ring / glv_batch_track_s16 calls on the same batch, and at a hop both entries take the two produce identical
 * output and state.
 * Accepted: what glv_batch_track_s16 accepts (GLV_OP_FFT required, with GLV_OP_GRAVITY / AVERAGE / BARS / R16 / PRIVATE_STATE; gl_storage 0 and 1, channels
 * 1 and 2, every log_mode, a bar-texel table honoured).  Refused: what it refuses minus its two hop / pitch rules, plus hop == 0 -- GLV_ERR_INVALID: other
 * operator bits, steps == 0, hop == 0, pitch_frames < n + (steps - 1) * hop, a NULL pointer, a workspace that is not 256-byte aligned,
 * steps * streams * 2 > 2^32 - 1 rows; GLV_ERR_STATE: gl_storage 2, a GLV_OP_BARS_ONLY batch, column texels set, a single-row (drop-in) batch, and everything
 * glv_batch_process_s16 refuses (the gravity form mix, unannounced state, parameters changed without glv_batch_set_params).  A refused call launches
 * nothing and leaves the batch untouched; the query then returns 0 with the code's name at the front of glv_last_error.
 * Stream-ordered: kernels and nothing else -- nothing is allocated or synchronised, the first call can be captured, glv_batch_timing_* covers it.
 * Launches (glv_batch_last_launches):
 *   1  a stateless chain without bars (GLV_OP_FFT [| GLV_OP_R16], a spectrogram): the transform kernel (glv_batch_kernel_name: glv_frame_kernel) takes every
 *      window of the call in ONE launch and writes step-major rows straight into d_out.  The workspace is never touched; the query reports 256.
 *   2  stateless with bars: the transform writes step-major rows into the workspace, the bars kernel follows.
 *   2  with state: the transform writes rows [stream][step][channel] into the workspace, glv_track_scan_kernel (glv_batch_kernel_name) walks them as in
 *      glv_batch_track_s16; 3 with bars.
 * The transform enumerates windows stream by stream, so the overlapping windows of one stream are in flight together and their overlap meets in L1 / L2; a
 * window whose first byte is 8-byte aligned is read with 8-byte loads, any other as pairs of dwords (all are aligned when d_pcm is 8-byte aligned and hop and
 * pitch_frames are even).  No launch reads a byte outside the windows the call names.
 * Workspace (R = steps * streams * 2 rows, sizes rounded up to 256 bytes): 256 for the one-launch form; else R * n * (2 for a GL_R16 chain's texel rows, 4
 * for floats) for the transform, plus, with state AND bars, R * n * (2 | 4) for the scan's results as glv_batch_track_s16 sizes them.  Never more than
 * glv_batch_track_s16 needs for the same call (its transform region is (n / hop) * 2 * floor(frames / n) rows, frames = (streams - 1) * pitch_frames +
 * (steps - 1) * hop + n: at least R, and growing with the pitch).
 * Measured (tools/track_windows_bench.py; profiles/r12/track_windows.txt: one MI355X, N = 4096, the GL chain with F = 5 and the pre-smoothing pass, texels
 * out; a host clock around the calls and the synchronise that ends them, medians of 7 alternating rounds; 1 / 8 / 64 streams x 2048 steps, 1024 x 256):
 *   hop 735 against the same windows through glv_batch_process_s16 one by one: 2.02 against 41.6 ms (20.6 x), 2.54 against 44.7 (17.6 x), 5.55 against 46.2
 *   (8.3 x), 7.68 against 10.7 (1.40 x).  Hop 736, whose windows are all 8-byte aligned: 2.02 / 2.58 / 5.50 / 7.74 ms, and hop 735 from a d_pcm one frame on:
 *   2.03 / 2.54 / 5.53 / 7.70 -- inside the round-to-round spread of hop 735 at every point: the dword loads cost nothing measurable.
 *   hop 256 against glv_batch_track_s16 in the same library (3 launches against 18): tight pitch 1.99 against 2.10 ms, 2.53 against 2.58, 5.20 against 5.78,
 *   7.63 against 8.32 -- ahead at 1 and at 1024 streams, inside the spread (none) at 8 and 64; pitch of twice what the call consumes 1.98 against 2.10,
 *   2.54 against 2.75, 5.19 against 6.65 (1.28 x), 7.65 against 10.6 (1.39 x), with 8 against 12.5 GiB of workspace at 1024 streams.
 * Which entry for a power-of-two hop: this one, at every stream count measured (1 to 1024) -- it was behind at none, its time and workspace do not grow with
 * the pitch, and from 64 streams on a recording with slack behind its windows runs 1.3-1.4 x faster.  Neither entry delegates to the other. */
uint64_t glv_batch_track_windows_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops);   /* 0: refused; also sizes glv_batch_track_windows_f32 */
int glv_batch_track_windows_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                                unsigned ops, void* hip_stream);
/* Track mode for the wave module: the texture of every update of a recording in ONE call (glv_batch_track_s16 refuses GLV_OP_WAVE; these are the entry
 * points that take it).  Added within ABI 7 without a version change: detect them by the symbol.
 *   d_pcm   int16 [streams][pitch_frames][2]; window t of stream s = its frames [t * hop, t * hop + n).  hop is ANY value >= 1 (a renderer's is
 *           rate / fps, e.g. 735), hop > n included; pitch_frames >= n + (steps - 1) * hop and nothing else is asked of it.
 *   ops     GLV_OP_WAVE [| GLV_OP_BARS] [| GLV_OP_R16], the combinations glv_batch_process_s16 takes for GLV_OP_WAVE; channels 1 and 2; a bar-texel
 *           table (glv_batch_set_bar_texels) is honoured as there.
 *   d_out   step-major: d_out + t * (bytes one glv_batch_process_s16 call with these ops writes) is bit for bit what that call on window t would have
 *           written -- texels, floats c / 65535, pass texels, pass floats.
 *   d_work  caller-owned, 256-byte aligned, at least glv_batch_track_wave_work_bytes(...) bytes (0: refused, glv_last_error starts with the code's
 *           name).  Without GLV_OP_BARS none is needed: the query reports 256, the pointer must still be non-NULL and aligned and is never touched.
 *           With GLV_OP_BARS the query reports what the two launches need -- steps * streams * 2 rows of n texels or floats -- for every hop and pitch:
 *           it does not see d_pcm, whose alignment decides between one launch and two.  A call that runs in one launch never touches d_work.
 * Stateless: the batch's state, rings and heads are untouched.  Stream-ordered: kernels and nothing else -- nothing is allocated or synchronised, the
 * first call can be captured into a hipGraph, glv_batch_timing_* covers it.
 * Refused: GLV_ERR_INVALID -- any bit besides the three, no GLV_OP_WAVE, steps == 0, hop == 0, pitch_frames too short, a NULL pointer, an unaligned
 * workspace, steps * streams * 2 > 2^32 rows; GLV_ERR_STATE -- what a GLV_OP_WAVE process call is refused for (gl_storage 0 with bars, a creation mask
 * without both bits, column texels set, bar parameters changed without glv_batch_set_params) and a single-row (drop-in) batch.  A refused call
 * launches nothing.
 * Launches (glv_batch_last_launches; glv_batch_kernel_name as for the process call): 1 without bars (glv_wave_kernel over every window).  With bars 1
 * (glv_bars_rows_i8_kernel straight from the frames) where the process call fuses -- GLV_BARS_I8_EXACT, averaging sample mode, no bar-texel table, no
 * GLV_UNFUSED_WAVE -- AND every window starts on a group of 8 frames: d_pcm 32-byte aligned, hop % 8 == 0, pitch_frames % 8 == 0.  With bars in every
 * other case 2 -- a d_pcm that is not 32-byte aligned (a seek to any frame of a recording) included: the waveform kernel writes the samples the bars
 * read into the workspace, the bars kernel of the process call's second launch runs over all of them.
 * Which rows share a workgroup of the one-launch form -- 64 consecutive output rows, or 64 consecutive steps of one channel row, whose windows overlap --
 * changes no bit; the first is the default (GLV_TRACK_WAVE_ORDER=rows|steps in the environment at creation: diagnostics).
 * Measured against the same windows through glv_batch_process_s16 one by one, timed with a library built from the commit before these entry points (this
 * one's build: the same times), the window cutting and upload that form needs NOT counted (tools/track_wave_bench.py; profiles/r11/track_wave.txt: one
 * MI355X, N = 4096, gl_storage 1, bars = n, bar_phase 0.5, GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16; a host clock around the calls and the synchronise that ends
 * them, medians of 7): hop 256, 2048 steps -- 1 stream 0.066 ms against 22.3 ms (338 x), 8 streams 0.207 against 23.2 ms (112 x), 64 streams 1.38 against
 * 23.5 ms (17.0 x); 1024 streams, 256 steps, 2.47 against 5.98 ms (2.4 x); hop 735 (two launches, 32 MiB of workspace), 1 stream, 2048 steps, 0.064 against
 * 22.4 ms (349 x).  The one-by-one form costs ~11 us per update until the chip fills; the track call was the faster at every point measured.  By steps
 * instead of by rows: 0.048 / 0.178 / 1.43 / 2.65 ms at 1 / 8 / 64 / 1024 streams -- ahead at few streams, behind at many, by about the round-to-round
 * spread either way (the hop-735 point, where the order plays no part, shows the same 0.064 / 0.044 between the two batches). */
uint64_t glv_batch_track_wave_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops);   /* also sizes glv_batch_track_wave_f32 */
int glv_batch_track_wave_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                             unsigned ops, void* hip_stream);
/* Track mode from float recordings: glv_batch_track_windows_s16 and glv_batch_track_wave_s16 for the layout a PulseAudio source or an audio decoder
 * delivers.  Added within ABI 7 without a version change: detect them by the symbol.
 *   d_pcm   float [streams][pitch_frames][2], interleaved L R (glv_batch_process_f32_stereo's frames), aligned like a float frame: 8 bytes, anything
 *           less is GLV_ERR_INVALID.  Window t of stream s = its frames [t * hop, t * hop + n); any hop >= 1, hop > n included; any
 *           pitch_frames >= n + (steps - 1) * hop.  A seek to any frame of a 16-byte aligned recording is a valid d_pcm: windows start 8-byte aligned
 *           and no more.
 * Contract: that of the s16 entry of the same name with glv_batch_process_f32_stereo as the sequential side.  The output of step t -- and for
 * glv_batch_track_windows_f32 the batch's state afterwards: gravity store, history ring, ring head, gravity form -- is bit for bit what `steps` consecutive
 * glv_batch_process_f32_stereo(b, window_t, out_t, ops, stream) calls produce and leave, -0 / Inf / NaN / denormal samples included; channels == 1 mixes
 * (L + R) / 2 in float as that call does.  Chunks compose; calls mix with process, ring and s16 track calls on the same batch.  Accepted and refused ops,
 * the GLV_ERR_STATE cases and "a refused call launches nothing" are those of glv_batch_track_windows_s16 / glv_batch_track_wave_s16.  Stream-ordered:
 * kernels and nothing else -- nothing is allocated or synchronised, the first call can be captured, glv_batch_timing_* covers it.
 * Workspace: glv_batch_track_windows_work_bytes / glv_batch_track_wave_work_bytes, the queries of the s16 entries -- the rows between launches do not
 * depend on the input's type.
 * Launches (glv_batch_last_launches, glv_batch_kernel_name as for the s16 entries): glv_batch_track_windows_f32 1 for a stateless chain without bars, 2
 * with bars or with state, 3 with both.  glv_batch_track_wave_f32 1 without bars; with bars ALWAYS 2 (glv_wave_kernel, then the bars kernel): the integer
 * pass reads s16 frames only, as in the float process call -- the query already reports the two-launch size.
 * The transform reads a window whose first byte is 16-byte aligned with the loads of a back-to-back frame, any other in naturally aligned 8-byte (mono and
 * N >= 16384) or 4-byte pieces; no launch reads a byte outside the windows the call names.  There is no float twin of glv_batch_track_s16 (the residue
 * form): the windows entry is the recommended one at every hop.
 * Measured (tools/track_f32_bench.py; profiles/r13/track_f32.txt: one MI355X, N = 4096, hop 735, an odd pitch; a host clock around the calls and the synchronise
 * that ends them, medians of 7 alternating rounds; 1 / 8 / 64 streams x 2048 steps, 1024 x 256), each float track call against the same windows through
 * glv_batch_process_f32_stereo one by one (window cutting not counted) and against the s16 entry on an s16 recording of the same shape:
 *   glv_batch_track_windows_f32, the GL chain with F = 5 and the pre-smoothing pass, texels out: 1.99 against 44.9 ms one by one (22.6 x) and 1.99 ms from
 *   s16; 2.58 against 47.1 (18.3 x) and 2.56; 5.83 against 48.3 (8.3 x) and 5.52; 8.46 against 12.7 (1.50 x) and 7.79.
 *   glv_batch_track_wave_f32, GLV_OP_WAVE | GLV_OP_BARS | GLV_OP_R16 (two launches in both forms at this hop): 0.045 against 18.3 ms one by one (409 x) and 0.054 ms
 *   from s16; 0.213 against 20.5 (96 x) and 0.212; 1.57 against 22.0 (14.1 x) and 1.38; 3.01 against 6.36 (2.1 x) and 2.81.
 * Ahead of the one-by-one form at every point.  Against the s16 form: inside the round-to-round spread at 1 and 8 streams, where the scan and the launches
 * dominate; BEHIND it at 64 and 1024 streams, by 6 % and 9 % (FFT chains) and 13 % and 7 % (wave), more than the spread: there the first launch is bound by
 * the input it reads, and a float recording is twice the bytes. */
int glv_batch_track_windows_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                                unsigned ops, void* hip_stream);
int glv_batch_track_wave_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                             unsigned ops, void* hip_stream);
/* Track mode for the graph module: the columns of every update of a recording in ONE call (the other track entries refuse a batch with column texels
 * set; these are the entry points that take it).  Added within ABI 7; detect by the symbol.
 *   d_pcm, pitch_frames, hop, steps: as for glv_batch_track_windows_s16 / _f32 -- any hop >= 1 (hop > n too), any pitch_frames >= n + (steps - 1) * hop; the
 *           s16 recording 4-byte aligned, the f32 one 8-byte aligned.  There is no residue-form twin.
 *   batch   gl_storage 1, created with GLV_OP_BARS and the chain's state bits, a column table set (glv_batch_set_column_texels).
 *   ops     GLV_OP_FFT | GLV_OP_BARS with GLV_OP_GRAVITY and / or GLV_OP_AVERAGE (GLV_OP_PRIVATE_STATE is ignored): the GL chains for which a process call takes
 *           columns.  Every log_mode, channels 1 and 2, every sample_mode.
 *   d_out   float [steps][streams][2][cols]: the block at d_out + t * streams * 2 * cols * 4 is what process call t writes.
 *   d_work  caller-owned, 256-byte aligned, at least glv_batch_track_columns_work_bytes(...) bytes (0: refused, glv_last_error starts with the code's name).
 * Contract: glv_batch_track_windows_s16's with columns as the output -- step t's columns and the batch's state afterwards (gravity store, history ring, ring
 * head, gravity form, over ALL n bins) are bit for bit what `steps` consecutive glv_batch_process_s16 (_f32: glv_batch_process_f32_stereo) calls with the same
 * table produce and leave behind.  Chunks compose; calls mix with process and ring calls on the same batch, and with the other track calls once the table
 * is cleared.  Stream-ordered: kernels only, nothing allocated or synchronised; the first call can be captured into a hipGraph; glv_batch_timing_* covers it.
 * Refused, launching nothing and leaving the batch untouched -- GLV_ERR_INVALID: any other ops bit, no GLV_OP_FFT or no GLV_OP_BARS, steps or hop 0, a pitch
 * too short, a NULL pointer, a workspace not 256-byte aligned, an f32 d_pcm not 8-byte aligned, more than 2^32 - 1 rows.  GLV_ERR_STATE: no column table set
 * (glv_batch_track_windows_* takes bars), GLV_OP_R16 (the columns are floats, as in a process call), gl_storage 0 or 2, a GLV_OP_BARS_ONLY batch, a
 * single-row batch, a chain without state, and whatever the process call refuses (the gravity form mix, unannounced state, stale parameters).
 * Launches (glv_batch_last_launches 3, glv_batch_kernel_name "glv_columns_kernel"): the transform over the windows where they lie, texel rows
 * [stream][step][channel] into the workspace; glv_track_scan_kernel, every step's texels into the workspace's second region; glv_columns_kernel in its
 * texel-row kind over steps * streams * 2 rows -- sample_mode average: the exact integer sums over the table's work lists; maximum / hybrid: x = c / 65535
 * correctly rounded, then the float walk of the process call.  The texels between launches are half the bytes of the floats c / 65535 the process call's
 * second launch reads.
 * Workspace: R = steps * streams * 2 rows; R * n * 2 bytes for the transform's texels and R * n * 2 for the scan's, each rounded up to 256.
 * Measured (tools/track_columns_bench.py; profiles/r14/track_columns.txt: one MI355X, N = 4096, hop 735, an odd pitch, the GL chain with F = 5; a host clock
 * around the calls and the synchronise that ends them, medians of 7 alternating rounds; 1 / 8 / 64 streams x 2048 steps, 1024 x 256) against the same windows
 * through glv_batch_process_s16 one by one with the same table (window cutting not counted):
 *   an 800-pixel window (401 columns over 801 texels; one by one two launches): 2.23 against 54.4 ms (24.4 x), 4.71 against 61.1 (13.0 x), 22.6 against 63.3
 *   (2.8 x); at 1024 streams BEHIND, 41.8 against 19.8 ms (0.47 x).
 *   a 320-pixel window (161 columns over 321 texels; one by one one launch): 2.09 against 51.7 ms (24.8 x), 3.45 against 54.6 (15.8 x), 12.9 against 56.1
 *   (4.3 x); at 1024 streams BEHIND, 22.5 against 10.9 ms (0.48 x).
 * From 64 streams on the call's time is the columns kernel's, whose texel-row kind reads a lane's eight taps with eight 2-byte loads: once the chip is full
 * the one-by-one form, which never takes its rows through HBM where it fuses, is the faster -- cut such a track into fewer streams per call, or use
 * process calls there.
 * A store limit for the scan (only the bins the columns read, about 0.29 n, in whole 128-bin workgroups) was built with a creation-time switch and measured
 * in the same file (`full` = every bin stored): full / limit 0.99 and 0.99 at 1 stream, 0.98 and 1.01 at 8, 1.006 and 1.000 at 64 (spread 0.3 and 0.7 ms of
 * 22.6 and 12.9), 1.03 and 1.05 at 1024 (spread 2.4 and 0.4 ms of 41.8 and 22.5).  Not faster by more than the spread at 64 streams: the limit and its
 * switch were deleted, the scan stores every bin. */
uint64_t glv_batch_track_columns_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops);   /* 0: refused; sizes both entries */
int glv_batch_track_columns_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                                unsigned ops, void* hip_stream);
int glv_batch_track_columns_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                                unsigned ops, void* hip_stream);
/* Track mode for GLV_OP_BARS_ONLY batches: every update of a recording in ONE call, over the live bins only (the other track entries refuse such a
 * batch -- its state beyond the live bins is not kept; these are the entry points that take it).  Added within ABI 7; detect by the symbol.
 *   d_pcm, pitch_frames, hop, steps: as for glv_batch_track_windows_s16 / _f32 -- any hop >= 1, any pitch_frames >= n + (steps - 1) * hop; the s16
 *           recording 4-byte aligned, the f32 one 8-byte aligned.
 *   batch   created with GLV_OP_BARS_ONLY, gl_storage 0 or 1, channels 1 or 2; bars, bar texels (glv_batch_set_bar_texels) or columns
 *           (glv_batch_set_column_texels), whichever is set.
 *   ops     GLV_OP_FFT | GLV_OP_BARS with GLV_OP_GRAVITY and / or GLV_OP_AVERAGE; GLV_OP_R16 and GLV_OP_PRIVATE_STATE wherever the process call takes them.
 *   d_out   step-major, what the process call writes: bars, bar texels or columns of [steps][streams][2].
 *   d_work  caller-owned, 256-byte aligned, at least glv_batch_track_live_work_bytes(...) bytes (0: refused, glv_last_error starts with the code's name):
 *           the value, and the layout, of the windows (columns) query of the same batch without the flag -- two regions of steps * streams * 2 rows at pitch n.
 * Contract: step t of d_out is bit for bit what the t-th of `steps` consecutive glv_batch_process_s16 (_f32: glv_batch_process_f32_stereo) calls on window t
 * writes on this batch; afterwards the ring head, the gravity form and the state of every bin below glv_batch_live_bins(b) are those the sequential calls
 * leave.  The state at and beyond the live bins is unspecified, as after a live process call (and the batch counts as having run live: glv_batch_set_params
 * and glv_batch_set_bar_texels guard it the same way).  Chunks compose; calls mix with process and ring calls on the same batch.  Stream-ordered: kernels
 * only, nothing allocated or synchronised; the first call can be captured into a hipGraph; glv_batch_timing_* covers it.
 * Refused, launching nothing and leaving the batch untouched -- GLV_ERR_INVALID: no GLV_OP_FFT, no GLV_OP_BARS, no state operator, any other ops bit, steps
 * or hop 0, a pitch too short, a NULL pointer, a workspace not 256-byte aligned, an f32 d_pcm not 8-byte aligned, more than 2^32 - 1 rows.  GLV_ERR_STATE: a
 * batch without GLV_OP_BARS_ONLY (glv_batch_track_windows_* / glv_batch_track_columns_* take it), gl_storage 2, a single-row batch, and whatever the
 * process call refuses.
 * Launches (glv_batch_last_launches 3; glv_batch_kernel_name names the third): the transform over the windows where they lie, whole rows into the
 * workspace; glv_track_scan_kernel over the kept bins K of every row; the bars or columns kernel.  K is the smallest multiple of 64 that covers the live bins
 * and every bin the third kernel can read (the chunked float bars read whole chunks past a bar's last tap, with weights of +0).  Nothing at or beyond bin K
 * of any row of the workspace's second region is written, and the state there is left as the call finds it.  Where the batch has no live bins (the bars
 * sample too far, log_mode 2) or K exceeds a kernel configuration's live share, the scan walks full rows: the same results, every bin's state kept.
 * Measured (tools/track_live_bench.py; profiles/r15/track_live_rule.txt, column (d) -- the form that ships -- and profiles/r15/track_live.txt: one MI355X, N = 4096, hop 735, an odd pitch, the shipped pipeline with texels out, F = 5;
 * a host clock around the call and the synchronise that ends it, medians of 7 alternating rounds; 1 / 8 / 64 streams x 2048 steps, 1024 x 256):
 *   2.02 / 2.46 / 4.76 / 5.58 ms, against glv_batch_track_windows_s16 on an unflagged batch (the library before this entry) 1.99 / 2.56 / 5.46 / 7.90 ms and
 *   against the same windows through glv_batch_process_s16 one by one on the flagged batch 35.2 / 37.0 / 38.7 / 9.10 ms.
 * Level with the unflagged track call at one stream (the difference is inside the spread of 0.08 ms), ahead of it by 4 % at 8 streams, 13 % at 64 and 29 % at
 * 1024; ahead of the one-by-one live calls at every point, 17 x, 15 x, 8.1 x and 1.63 x.  A caller with a flagged batch takes this entry at every stream count.
 * Live classes for the transform (magnitude, log, tilt and quantisation for the live register slots only, stores below K) were built behind a creation-time
 * switch and measured in profiles/r15/track_live_rule.txt: ahead of the full-row classes by 0.115 ms of 4.65 at 64 streams, inside the spread of 0.200 ms, and
 * by 0.492 ms of 5.09 at 1024 streams (spread 0.400 ms).  Not ahead by more than the spread at both, so by the rule set beforehand the classes, the switch and
 * their tests were taken out; the transform is the one of glv_batch_track_windows_*. */
uint64_t glv_batch_track_live_work_bytes(const glv_batch* b, uint32_t pitch_frames, uint32_t hop, uint32_t steps, unsigned ops);   /* 0: refused; sizes both entries */
int glv_batch_track_live_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                             unsigned ops, void* hip_stream);
int glv_batch_track_live_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, uint32_t hop, uint32_t steps, void* d_out, void* d_work,
                             unsigned ops, void* hip_stream);
/* Track mode at given window starts: every entry above places window t at t * hop, one integer hop per call.  These take a TABLE of positions instead -- a
 * renderer at a rate the frame rate does not divide (the shipped 22050 Hz at 60 fps: 367.5 frames per step), the windows a live GLava would have shown
 * (updates every sample_sz / 4 frames, the latest complete one per render frame), variable frame rates (with the gravity those run at:
 * glv_batch_track_rates_s16 / _f32 below), scrubbing, cue lists.  Added within ABI 7; detect by the symbol.  The ten entries above keep their signatures and behaviour; the residue form (glv_batch_track_s16) has no table twin.
 *   d_pcm, pitch_frames: as for glv_batch_track_windows_s16 / _f32, with pitch_frames >= n as the only rule (the s16 recording 4-byte aligned, the f32 one 8).
 *   d_starts  uint32 [steps] in DEVICE memory, 4-byte aligned, shared by all streams.  Window t of stream s is the n frames of that stream's recording
 *           from min(d_starts[t], pitch_frames - n) on.  Entries may come in any order; repeats and backward jumps are valid.
 *   d_out, d_work, ops: those of the form the call takes --
 *           ops with GLV_OP_WAVE: the wave form (glv_batch_track_wave_*); else a GLV_OP_BARS_ONLY batch: the live form (glv_batch_track_live_*); else a batch
 *           with column texels set: the columns form (glv_batch_track_columns_*); anything else: the windows form (glv_batch_track_windows_*).
 *           Each form accepts and refuses what its uniform-hop entry does, minus the hop rules.
 * The clamp is done in the kernels, because the host cannot see the table without a synchronise: whatever the table holds, no launch reads a byte outside the
 * recordings the call names ([d_pcm + s * pitch_frames, + pitch_frames) frames for s < streams) nor a table entry outside d_starts[0, steps).
 * Contract: the existing one, word for word -- step t of d_out, and afterwards the batch's state (gravity store, history ring, ring head, gravity form; on a
 * live batch the state below glv_batch_live_bins), are bit for bit what `steps` consecutive glv_batch_process_s16 / glv_batch_process_f32_stereo calls on
 * those windows produce and leave behind.  Chunks compose: a call on d_starts + k continues a call that ended at step k.  Calls mix with every other
 * process, ring and track call.  Stream-ordered: kernels only, nothing allocated or synchronised; the first call can be captured into a hipGraph.
 * The table is read when the kernels run, not when the call is made: rewriting d_starts (in stream order) between replays re-aims a captured call.
 * Refused, launching nothing and leaving the batch untouched -- GLV_ERR_INVALID: pitch_frames < n, steps 0, a NULL pointer (d_starts included), a d_starts
 * not 4-byte aligned, a d_work not 256-byte aligned, an f32 d_pcm not 8-byte aligned, the row-count limits and the ops rules of the form.  GLV_ERR_STATE:
 * gl_storage 2, a single-row batch, whatever the process call refuses.
 * Launches: the FFT forms 1 (stateless, no bars), 2 or 3 as for glv_batch_track_windows_*; the wave form 1 without bars and ALWAYS 2 with bars (the
 * one-launch integer pass needs every window on a group of 8 frames, which the host cannot know of a table in device memory).
 * Workspace: glv_batch_track_at_work_bytes, which is the form's own query for the same steps (none depends on hop or pitch where windows are read where
 * they lie); 256 where nothing is parked; 0: refused, glv_last_error starts with the code's name.
 * Kernels: the transform of glv_batch_track_windows_* with the table's entry in place of t * hop (glv_frame.h TrackWindows).  The entry of a frame is
 * requested one frame ahead, with the previous frame's samples, so that no load whose value an address depends on is issued behind a row's stores.
 * Measured (tools/track_at_bench.py, profiles/r16/track_at.txt: one MI355X, N = 4096, the GL chain with F = 5 and the pre-smoothing pass, texels out; a host clock
 * around the call and the synchronise that ends it, medians of 7 alternating rounds, spread = max - min; 1 / 8 / 64 streams x 2048 steps, 1024 x 256):
 *   (a) the table t * 735 against glv_batch_track_windows_s16 at hop 735, same library: 1.980 against 1.979 ms (spreads 0.023 / 0.070), 2.538 against 2.529
 *       (0.014 / 0.019), 5.427 against 5.363 (0.146 / 0.112), 7.959 against 7.741 (0.212 / 0.421) -- 0.1 to 2.8 % behind, inside the spread at every point;
 *       the float entries 1.980 against 1.986, 2.580 against 2.576, 5.617 against 5.626, 8.398 against 8.346 ms: level.
 *   (b) glv_batch_track_windows_s16 at hop 735 in this library against the parent commit's: 1.975 / 2.535 / 5.262 / 7.663 against 1.975 / 2.530 / 5.274 /
 *       7.852 ms, inside the spread at every point (the hop kinds' kernels have the parent's registers and scratch, 152 of 152: profiles/r16/track_at_isa.txt).
 *   (c) the 22050 Hz / 60 fps table against the same windows through glv_batch_process_s16 one by one: 1.983 against 41.4 ms (20.9 x), 2.542 against 44.6
 *       (17.6 x), 5.588 against 46.2 (8.3 x), 7.918 against 10.7 (1.35 x).
 * The table kinds hold 1-2 more VGPRs than the hop kinds at N = 4096 and no scratch.  At other sizes 45 of their 152 kernels have scratch their hop kind lacks
 * (68-88 bytes a lane at N <= 1024, 12-20 at 2048 and 8192, 168-224 at 16384 and 32768: profiles/r16/track_at_isa.txt) -- the entry carried across the
 * transform and a second division; those sizes have not been timed. */
uint64_t glv_batch_track_at_work_bytes(const glv_batch* b, uint32_t steps, unsigned ops);   /* 0: refused, glv_last_error starts with the code's name; sizes both entries */
int glv_batch_track_at_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const uint32_t* d_starts, uint32_t steps,
                           void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_at_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const uint32_t* d_starts, uint32_t steps,
                           void* d_out, void* d_work, unsigned ops, void* hip_stream);
/* Track mode with a per-step update rate: every track entry above applies gravity with ONE step for the whole call, g = gravity_step * (1.0F / ur) from the
 * batch's glv_params.  The reference measures ur as it runs (render.c:906, :2379-2399) and both gravity paths read it at every update (render.c:728, :2224): at
 * 22050 Hz, 60 fps and updates of 256 frames a live GLava's first 59 updates run at ur = 1.0, the next 60 at 59.0, the rest at 60.0 -- never at 22050 / 256.  These
 * entries take that sequence as a second table.  Added within ABI 7; detect by the symbol.
 *   Everything except d_ur is glv_batch_track_at_s16 / _f32, word for word: the form the batch selects (a GLV_OP_BARS_ONLY batch: live; column texels set: columns;
 *   anything else: windows), the clamp of d_starts[t], d_out, the launches, the kernel glv_batch_kernel_name reports, and the workspace -- sized by
 *   glv_batch_track_at_work_bytes(b, steps, ops): the rate table adds no region.  A uniform hop is the table t * hop.
 *   d_ur    float [steps] in DEVICE memory, 4-byte aligned, shared by all streams.  Step t applies gravity with g_t = gravity_step * (1.0F / d_ur[t]): the host's
 *           expression (render.c:728), a correctly rounded division and then a separate multiply, evaluated in the scan kernel because the host cannot see the
 *           table without a synchronise.  No entry outside d_ur[0, steps) is read.  0, -0, negative, tiny and huge entries are taken as the reference takes them.
 * Contract: step t of d_out, and afterwards the batch's state (gravity store, history ring, ring head, gravity form; on a live batch the state below
 * glv_batch_live_bins), are bit for bit what `steps` consecutive glv_batch_process_s16 / glv_batch_process_f32_stereo calls produce and leave behind when each is
 * preceded by glv_batch_set_params with ur = d_ur[t].  The batch's own ur is NOT changed: the next process or track call uses it.  Chunks compose (a call on
 * d_starts + k, d_ur + k continues one that ended at step k); calls mix with every other process, ring and track call.  Stream-ordered: kernels only, nothing
 * allocated or synchronised, the first call can be captured; both tables are read when the kernels run, so rewriting d_ur in stream order re-aims a captured call.
 * A NaN entry is outside the contract (glv_batch_set_params refuses a NaN ur): that step and those after it are unspecified, but no launch reads or writes out
 * of bounds whatever the table holds.
 * Refused, launching nothing and leaving the batch untouched -- GLV_ERR_INVALID: a NULL d_ur or one not 4-byte aligned, ops without GLV_OP_GRAVITY (nothing
 * would read the table), ops with GLV_OP_WAVE (stateless), and everything glv_batch_track_at_* refuses with this code; GLV_ERR_STATE: as glv_batch_track_at_*.
 * Kernel: the rates kind of glv_track_scan_kernel (glv_misc.hip).  The entry of step t + 8 is requested with that step's row, so no load a step depends on sits
 * in its dependent chain.  Texel state (a GL chain) evaluates the float expression the gravity pass is defined by at every step: the host's packed integer step
 * is accepted only after being checked against that expression for all 65 536 texel values, so the bits are the sequential calls' either way.  The two existing
 * kinds of the scan kept their registers and scratch (profiles/r17/track_rates_isa.txt).
 * Python: glava_amd.track_starts.live_session_rates(rate, fps, frames, update_frames) gives (starts, step_of_frame, ur) of a live session whose every frame
 * meets its target and whose updates arrive on the audio clock; wall-clock jitter is not modelled.
 * Measured (tools/track_rates_bench.py, profiles/r17/track_rates.txt; the protocol of profiles/r16/track_at.txt: one MI355X, N = 4096, the GL chain with F = 5 and
 * the pre-smoothing pass, texels out, medians of 7 alternating rounds, spread = max - min; 1 / 8 / 64 streams x 2048 steps, 1024 x 256):
 *   (a) the rates entry with every d_ur[t] = the batch's ur against glv_batch_track_at_s16 on the same table t * 735, same library: 2.044 against 1.979 ms (spreads
 *       0.006 / 0.060), 2.602 against 2.527 (0.022 / 0.028), 5.669 against 5.388 (0.145 / 0.174), 8.164 against 7.887 (0.392 / 0.437) -- 3.0 to 5.2 % BEHIND, and
 *       beyond the spread at 1, 8 and 64 streams (0.065, 0.075 and 0.281 ms), inside it at 1024.  That is what the division and the float form of the texel step
 *       cost in every wave and step: 21 more VALU instructions a step than the packed integer step (profiles/r17/track_rates_isa.txt).  A per-step integer form on
 *       the device was not built; a caller whose rate never changes takes glv_batch_track_at_*.
 *   (b) glv_batch_track_at_s16 in this library against the parent commit's: 1.975 / 2.538 / 5.391 / 7.928 against 1.976 / 2.533 / 5.340 / 7.908 ms (spreads 0.011 /
 *       0.021 / 0.218 / 0.288 and 0.019 / 0.014 / 0.169 / 0.532), inside the spread at every point; bench.py level (101.4 / 101.1 against 100.4 M frames/s).
 *   (c) the tables of live_session_rates(22050, 60, ..., 256) against the same windows through glv_batch_process_s16 one by one with glv_batch_set_params between
 *       the calls: 2.054 against 68.4 ms (33.3 x), 2.621 against 72.2 (27.5 x), 5.910 against 73.0 (12.3 x), 8.358 against 14.4 (1.72 x). */
int glv_batch_track_rates_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const uint32_t* d_starts, const float* d_ur, uint32_t steps,
                              void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_rates_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const uint32_t* d_starts, const float* d_ur, uint32_t steps,
                              void* d_out, void* d_work, unsigned ops, void* hip_stream);
/* Track mode at render frames: the entries above give one result per UPDATE.  With `setinterpolate true` on `setaccelfft false` (gl_storage 3) the texture a
 * module samples on a render frame is not the latest finished spectrum but start + (end - start) * min(uratio * kcounter, 1) of the last two finished rows
 * (render.c:1760-1763, :1792-1809; the upload picks that buffer, :2185; the pre-smoothing pass runs over the upload, :2276-2303; the keyframes are pushed at
 * :2347-2353, the counters kept at :2379-2383) -- whenever the update rate is below 0.9 of the frame rate: a 144 Hz display, `setsamplesize 4096`.  These
 * entries run the updates of a recording AND give every render frame's texture, bars, bar texels or columns in one call.  Added within ABI 7; detect by the symbol.
 *   Updates: d_where / d_ur / steps are glv_batch_track_at_* 's d_starts and glv_batch_track_rates_* 's d_ur, word for word (d_ur NULL: the batch's own ur, the
 *   table call; else the rates call with its refusals).  The `steps` updates run through those calls' executor, and afterwards the batch's state (gravity store,
 *   history ring, ring head, gravity form) is bit for bit what they leave.
 *   Keyframes: keyframe k of a call is d_keys[k] for k < 2 -- `start` and `end` as the previous call left them -- and for k >= 2 the finished FLOAT row of step
 *   k - 2, what the same call on a gl_storage 0 batch writes as floats.  Every index a table holds is clamped to steps + 1 in the kernel: whatever the tables
 *   hold, no launch reads outside d_keys, the steps' rows, or the tables' [0, frames).
 *   Frame j, per row and bin: d_from[j] == d_to[j] -- that keyframe's own bits, no arithmetic (a frame whose uratio > 0.9 or with interpolation off: render.c:2185
 *   uploads the buffer); else w = s + ((e - s) * d_mod[j]) of keyframes s = d_from[j], e = d_to[j]: three separate IEEE float operations in the order of
 *   render.c:1806, no fused multiply-add, d_mod[j] applied as given (the host's min(uratio * kcounter, 1.0F)).  Then the upload's quantiser c = unorm16(w), the
 *   function every gl_storage 3 class applies (NaN and -0 give 0).
 *   d_out, frame-major: block j is what a gl_storage 3 process call with these ops would write if its finished float row were w_j.  GLV_OP_R16 without
 *   GLV_OP_BARS: the upload's texels, uint16 [frames][streams][2][n].  With GLV_OP_BARS the bars kernel follows over frames * streams * 2 texel rows -- the integer
 *   pass at 256 bars or more, bar texels, column texels (floats), maximum / hybrid, each in the arithmetic glv_batch_bars_arithmetic reports, as texels with
 *   GLV_OP_R16 -- [frames][streams][2][bars].
 *   Write-back: after the last frame d_keys[0] <- keyframe keep_from and d_keys[1] <- keyframe keep_to, both read before either is written; the pairs are (0, 1),
 *   (1, k >= 2) and (k, k') with 2 <= k < k'.  So chunks compose: a session cut into calls, each starting from the d_keys its predecessor left, gives the frames of
 *   the uncut session.  d_keys is zero-filled before a session's first call: the reference mallocs its keyframe buffers (render.c:1682) and shows garbage until two
 *   updates have passed; zero is this library's definition (integration/nullgl_harness.c does the same).
 *   Workspace: glv_batch_track_frames_work_bytes(b, steps, frames, ops) bytes, 256-byte aligned: the steps' float rows from the transform, the scan's where the
 *   chain keeps state, and with GLV_OP_BARS the frames' texel rows (each region rounded up to 256 bytes).
 * Launches (glv_batch_last_launches): the table call's for the float chain without bars (1 stateless, 2 with state), + 1 (glv_track_frames_kernel), + 1 (the
 * write-back), + 1 with GLV_OP_BARS.  Stream-ordered: kernels only, nothing allocated or synchronised, the first call can be captured; all tables are read when
 * the kernels run, so rewriting d_mod in stream order re-aims a captured call.  glv_batch_kernel_name reports "glv_track_frames_kernel", whatever follows it.
 * Refused, launching nothing and leaving the batch untouched -- GLV_ERR_STATE: any gl_storage but 3 (on 1 the reference forces interpolation off,
 * render.c:2161-2168; 0 has no upload), a single-row batch, and everything the underlying table call refuses with this code; GLV_ERR_INVALID: fr NULL or any of
 * its pointers NULL, frames == 0, d_keys not 16-byte aligned or a table not 4-byte aligned, a keep pair outside the list above or >= steps + 2, ops without
 * GLV_OP_R16 or GLV_OP_BARS (the result is a texture), GLV_OP_WAVE, frames * streams * 2 > 2^32 - 1, and everything the table call refuses with this code.
 * Kernel (glv_track_frames.hip): one lane owns four consecutive bins of a row (16-byte keyframe loads, 8-byte texel stores) and walks a segment of frames with
 * both keyframes in registers, reloading one only when its index changes -- a live session's tables advance monotonically, so a keyframe row is read about once per
 * segment, not twice per frame; table entries are requested 4 frames ahead; the grid is segments x rows x groups of 256 bins, looped over beyond 8192 workgroups,
 * the segment at least 8 frames and as long as still leaves 16384 workgroups.  With GLV_OP_BARS only the bins the bars kernel reads are written, the limit of
 * gl_storage 3's two-launch process route.  The scan, frame and bars kernels kept their code.
 * Python: glava_amd.track_starts.keyframe_tables(modified, on, uratio) gives (from, to, mod, keep_from, keep_to) from a session's per-frame record;
 * live_session_frames(rate, fps, frames, update_frames) the whole session's tables with gl->fr measured as the reference measures it (wall-clock jitter is not
 * modelled).
 * Measured (tools/track_frames_bench.py, profiles/r19/track_frames.txt; the protocol of profiles/r17/track_rates.txt: one MI355X, N = 4096, gl_storage 3, F = 5, the
 * pre-smoothing pass, texels out, the tables of live_session_frames(22050, 144, ..., 256), medians of 7 alternating rounds, spread = max - min; 1 / 8 / 64 streams x
 * 2048 steps = 3426 frames, 1024 streams x 256 steps = 430 frames):
 *   (a) the frames call against glv_batch_track_rates_s16 on the same batch and steps: 1.569 against 1.529 ms, 2.133 against 1.934, 7.019 against 5.584, 11.561
 *       against 8.694 (spreads 0.01 / 0.02 / 0.18 / 0.13) -- 1.67 times the rows through the bars kernel, and the frames stage;
 *   (b) the frames stage alone (frames kernel and write-back, texels out, by difference of HIP-event times): 0.030 / 0.210 / 1.556 / 3.219 ms, i.e. 4.8 / 4.8 / 5.1 /
 *       5.0 TB/s of texels written and keyframe rows read, beside the 5.47 TB/s of profiles/stream_ceiling.json's read-write mix (4.0-6.2 TB/s for pure writes).
 *       With one segment at 64 streams (the default as first built: 2048 workgroups) the same stage took 3.460 ms, 2.3 TB/s;
 *   (c) glv_batch_track_at_s16 on the shipped GL chain in this library against the parent commit's: 1.967 / 2.532 / 5.419 / 8.152 against 1.971 / 2.527 / 5.444 /
 *       7.997 ms (spreads 0.020 / 0.026 / 0.227 / 0.385 and 0.055 / 0.032 / 0.112 / 0.337), inside the spread at every point; bench.py 103.8 / 102.1 against
 *       103.9 / 103.3 M frames/s alternating (profiles/r19/bench_compare.txt), inside the run-to-run spread.  The device code of every object both trees have is the
 *       parent's byte for byte (tools/track_frames_isa.py, profiles/r19/track_frames_isa.txt). */
typedef struct glv_track_frames {
    const uint32_t* d_from;   /* uint32 [frames], device: keyframe index of `start` for render frame j            */
    const uint32_t* d_to;     /* uint32 [frames], device: keyframe index of `end`                                   */
    const float*    d_mod;    /* float  [frames], device: the host's min(uratio * kcounter, 1.0F), applied as given */
    uint32_t        frames;   /* render frames of this call, >= 1                                                   */
    float*          d_keys;   /* float [2][streams][2][n], device, caller-owned, 16-byte aligned: keyframes 0 and 1 */
    uint32_t        keep_from, keep_to;   /* keyframe indices written back to d_keys[0] / d_keys[1] after the call  */
} glv_track_frames;
uint64_t glv_batch_track_frames_work_bytes(const glv_batch* b, uint32_t steps, uint32_t frames, unsigned ops);   /* 0: refused, glv_last_error starts with the code's name; sizes both entries */
int glv_batch_track_frames_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur /* NULL: the batch's ur */,
                               uint32_t steps, const glv_track_frames* fr, void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_frames_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur /* NULL: the batch's ur */,
                               uint32_t steps, const glv_track_frames* fr, void* d_out, void* d_work, unsigned ops, void* hip_stream);
/* Track mode at render frames for the wave module.  The reference forces interpolation off only when a bind with an `fft` transform is pushed to the GL
 * (render.c:2131-2135, :2161-2168); the wave module's bind requests `window` and `wrange` and nothing else (wave/1.frag:7-9), so with `setinterpolate true` every
 * render frame whose uratio <= 0.9 uploads s + ((e - s) * min(uratio * kcounter, 1)) of the last two wrange'd buffers (render.c:1792-1809; a wave bind uploads
 * `ilb`, :2185), runs the pre-smoothing pass over that upload (:2276-2303) and pushes the keyframes (:2347-2353) -- on ANY gl_storage, under the shipped
 * `setaccelfft true` too.  The entries above refuse GLV_OP_WAVE; these give every render frame's wave texture.  Added within ABI 7; detect by the symbol.
 *   Steps: d_where is glv_batch_track_at_* 's d_starts -- uint32 [steps] in device memory, shared by all streams, window t begins min(d_where[t], pitch_frames - n)
 *   frames into each recording (a fixed hop is the table t * hop).  `steps` is the number of keyframes the recording contributes: nothing is computed per step.
 *   Keyframes: keyframe k < 2 is d_keys[k], float [streams][2][n]; keyframe 2 + t of row 2 s + c and sample i is (u + 1.0F) / 2.0F (render.c:777-778), u the
 *   backend's unpack of frame min(d_where[t], pitch_frames - n) + i of stream s: s16 v / 65535, mono ((l + r) / 2) / 65535 in C int arithmetic (fifo.c:94-110);
 *   floats the sample itself, mono (l + r) / 2 (pulse_input.c:155-178) -- glv_wave_kernel's helpers.  The float keyframes exist nowhere else: no entry returns
 *   them (GLV_OP_WAVE without GLV_OP_R16 gives c / 65535).  Every index a table holds is clamped to steps + 1 in the kernel: whatever the tables hold, nothing
 *   outside d_pcm's recordings, d_keys and the tables' [0, frames) / [0, steps) is read.  d_keys is zero-filled before a session's first call.
 *   Frame j: d_from[j] == d_to[j] -- that keyframe's own bits; else w = s + ((e - s) * d_mod[j]), three float operations in the order of render.c:1806.  Then the
 *   upload's quantiser c = unorm16(w), then what a GLV_OP_WAVE process call with the same ops does on this batch: texels c (GLV_OP_R16), floats c / 65535
 *   (neither GLV_OP_R16 nor GLV_OP_BARS), or with GLV_OP_BARS the pre-smoothing pass / bar texels / maximum / hybrid over frames * streams * 2 rows.
 *   ops: GLV_OP_WAVE [| GLV_OP_BARS] [| GLV_OP_R16], exactly what glv_batch_track_wave_* takes, on every batch it takes them on (channels 1 and 2, bar texels,
 *   fewer than 256 bars, maximum / hybrid) and refused where it refuses, with its codes (column texels set, gl_storage 0 with bars, a creation mask without both
 *   bits, a single-row batch).  fr: glv_track_frames as above, with every refusal glv_batch_track_frames_* makes about it.
 *   d_out, frame-major: [frames][streams][2][w], w = n or bars.  Write-back: d_keys[0] <- keyframe keep_from, d_keys[1] <- keyframe keep_to as floats, both read
 *   before either is written; chunks compose as above.
 *   Workspace: glv_batch_track_wave_frames_work_bytes(b, steps, frames, ops): 256 without bars; with bars the frames' rows, frames * streams * 2 * n texels or
 *   floats (as the bars kernel takes them), rounded up to 256 bytes.  256-byte aligned.
 * Launches: 2 (glv_wave_frames_kernel, the write-back glv_wave_keys_kernel), 3 with GLV_OP_BARS.  There is no transform launch and there are no step rows.  Kernels
 * only: nothing allocated or synchronised, the first call can be captured, the tables are read when the kernels run.  glv_batch_kernel_name reports
 * "glv_wave_frames_kernel".  The batch's state is not touched.
 * Kernel (glv_track_frames.hip): one lane owns four consecutive frames of one stream, both channel rows -- a keyframe is 16 bytes of s16 or 32 bytes of floats from
 * the recording (wide loads where the group is 16-byte aligned, naturally aligned dword / 8-byte loads else: a window starts at any frame), or two 16-byte loads
 * from d_keys -- and walks a segment of frames with both keyframes in registers, as glv_track_frames_kernel does; the work items are segments x streams x groups
 * of 256 frames, one wave each, looped beyond 8192 workgroups. */
uint64_t glv_batch_track_wave_frames_work_bytes(const glv_batch* b, uint32_t steps, uint32_t frames, unsigned ops);   /* 0: refused, glv_last_error starts with the code's name; sizes both entries */
int glv_batch_track_wave_frames_s16(glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const uint32_t* d_where, uint32_t steps, const glv_track_frames* fr,
                                    void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_wave_frames_f32(glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const uint32_t* d_where, uint32_t steps, const glv_track_frames* fr,
                                    void* d_out, void* d_work, unsigned ops, void* hip_stream);
/* Track mode from PLANAR float recordings (added within ABI 7: detect them by the symbol).  The table, rates, frames and wave-frames calls above from the third
 * layout a recording comes in: d_rows float [streams][2][pitch_frames] -- the lb / rb rows glv_batch_process_f32 takes ([streams][2][n]), as one long buffer per
 * channel: a torch tensor [streams, channels, frames], a decoder that emits planar float, a host built around GLava's main loop.  Window t of stream s, channel c,
 * is the w = bufscale * n floats that begin min(d_starts[t], pitch_frames - w) floats into row 2 s + c; the clamp is the kernels', whatever the table holds no
 * launch reads outside the rows.  d_rows is 4-byte aligned and no more: a window begins at any sample, pitch_frames is any number >= w (the kernels take wide
 * loads where a row's window lies on them and naturally aligned dwords elsewhere, row by row).
 * NO MONO MIX: the rows are taken as they are, whatever glv_params.channels says -- glv_batch_process_f32's rule, the backend has already mixed lb / rb.  Step t
 * is therefore bit for bit what glv_batch_process_f32 on the window's two rows would have written, and with channels == 2 bit for bit what the interleaved _f32
 * sibling writes from the interleaved copy of the same samples, output and state.
 * In every other respect each entry IS its _f32 sibling: the form the ops and the batch select (windows, live, columns, wave), the refusals in the same words before
 * anything runs (under bufscale > 1 the wave forms refuse as theirs do), the state written back, kernels only on hip_stream, capturable into a hipGraph and
 * re-aimed by rewriting the tables.  Workspace: the siblings' queries size these entries too -- glv_batch_track_at_work_bytes for the table and rates calls,
 * glv_batch_track_frames_work_bytes and glv_batch_track_wave_frames_work_bytes for the frames calls; the layout of the recording changes no region.
 * There are no hop entries: a table of t * hop (glava_amd.track_starts.hop_starts) is the hop form, and measured inside its spread.
 * GLV_ERR_INVALID as the siblings, with d_rows misaligned for a float (4 bytes) in the place of their 8-byte rule. */
int glv_batch_track_at_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const uint32_t* d_starts, uint32_t steps,
                                  void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_rates_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const uint32_t* d_starts, const float* d_ur, uint32_t steps,
                                     void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_frames_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const uint32_t* d_where, const float* d_ur /* NULL: the batch's ur */,
                                      uint32_t steps, const glv_track_frames* fr, void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_wave_frames_f32_planar(glv_batch* b, const float* d_rows, uint32_t pitch_frames, const uint32_t* d_where, uint32_t steps, const glv_track_frames* fr,
                                           void* d_out, void* d_work, unsigned ops, void* hip_stream);
/* Track mode PER STREAM: the table, rates and planar calls above move every stream of a batch in lockstep -- one row of window starts, one row of rates and one
 * number of steps for all of them.  Listeners of a service sit at different positions of different recordings, drop different frames, end at different lengths,
 * and one that seeks has to catch up while the others stand still.  These entries take tables with ONE ROW PER STREAM and a count of steps per stream; stream s
 * then behaves as if it were alone in a batch with its own table for its own number of updates, bit for bit.  Added within ABI 7; detect by the symbol.
 * Everything not said here is glv_batch_track_at_s16 / _f32 / _f32_planar: d_pcm / d_rows, d_out and d_work and their layouts, the form the ops and the batch
 * select, the launches.  Sized by glv_batch_track_at_work_bytes(b, steps, ops): the rows add no region, and there is no other query.
 *   Windows.  Window t of stream s begins min(d_starts[s * steps + t], pitch_frames - k n) frames into that stream's recording, k the batch's bufscale.  The clamp
 *           is the kernels', so no launch reads outside the recordings whatever any table holds.  The tables are read when the kernels run: rewriting them in
 *           stream order re-aims a captured hipGraph.
 *   Rates.  With d_ur set, step t of stream s applies gravity with gravity_step * (1.0F / d_ur[s * steps + t]) -- the rates call's expression, row by row.  A
 *           non-NULL d_ur is refused (GLV_ERR_INVALID) with GLV_OP_WAVE or without GLV_OP_GRAVITY, as glv_batch_track_rates_* refuses it.  With d_ur NULL the
 *           batch's own ur applies at every step, in the arithmetic of the table call (texel state: the packed integer step wherever the host accepted it).
 *   Counts. c_s = min(d_counts[s], steps), evaluated on the device.  For t < c_s the output of step t of stream s is bit for bit what glv_batch_track_rates_* /
 *           _at_* writes for that step on a one-stream batch that holds stream s's state, recording and table row.  For t >= c_s the row of d_out is what the
 *           call's last stage produces from a finished row of all zeros: zeros without bars, and the bars, texels or columns of a zero row with them -- defined,
 *           so nothing stale is left behind.  A non-NULL d_counts is refused (GLV_ERR_INVALID) on a chain without state (neither GLV_OP_GRAVITY nor
 *           GLV_OP_AVERAGE, or GLV_OP_WAVE): there is nothing to protect, and the caller ignores the rows it does not want.
 *   State afterwards.  The batch's head advances by `steps` -- the host cannot see the counts, and the head is the batch's.  Stream s's gravity row and average
 *           ring are those of c_s sequential updates of that stream, presented at the batch's new head: the ring slot that holds the row of age j under the
 *           stream's own head sits where age j sits under (head + steps) % F.  The next process, ring or track call on the batch therefore continues every
 *           stream bit for bit, glv_batch_save_streams returns for stream s the blob a one-stream batch returns after c_s updates, and a stream with c_s == 0
 *           keeps its state bit for bit (its ring turned, every age in place).
 *   Forms.  All three FFT forms the table call selects (windows; live on GLV_OP_BARS_ONLY batches; columns), gl_storage 0, 1 and 3, channels 1 and 2 (planar: no
 *           mix), bufscale up to 16; and the wave form (GLV_OP_WAVE [| BARS] [| R16], two launches with bars as a table call's), which takes d_starts alone.
 *   Refused, launching nothing and leaving the batch untouched: everything glv_batch_track_at_* refuses, in the same words and with the same codes; and with
 *           GLV_ERR_INVALID a NULL tb or one not aligned for its pointers, a NULL or misaligned d_starts, and a d_ur or d_counts not 4-byte aligned.
 * Cost of a count: the transform stage still computes the windows of steps t >= c_s (clamped, therefore safe) and only the scan skips them -- a skip in the
 * transform would have to live in the frame kernel and is left for later.  A batch of listeners of very different lengths pays for the longest in stage (1).
 * Kernels: the transform in per-stream table kinds of the frame kernel (glv_frame.h in_track_each: the table kinds with the entry read at f % (streams * steps);
 * kinds of their own, because the index operand costs 58 of their 228 kernels registers or scratch beside the shared-table twins -- every frame kernel that
 * existed is byte for byte the parent's), glv_decimate_kernel's three track kinds and glv_wave_kernel's three window kinds, which CHANGED (one uniform test, one
 * index: registers and instruction counts in profiles/r25/track_each_isa.txt, which lists every object and kernel that is identical and every one that is not),
 * and glv_track_each_scan_kernel (glv_misc.hip), which glv_batch_kernel_name reports where the table call reports glv_track_scan_kernel: the walk bounded by the
 * stream's count (the look-ahead of 8 steps asks for no row and no rate at or beyond it), zeros behind it, and the ring written back turned by steps - c_s.
 * Python: glava_amd.track_starts.stack_tables(rows) pads per-stream (starts, ur) pairs of any lengths to the longest and returns the three arrays. */
typedef struct glv_track_tables {
    const uint32_t* d_starts;  /* uint32 [streams][steps], device memory, 4-byte aligned: row s is stream s's table */
    const float*    d_ur;      /* float  [streams][steps] or NULL: the batch's own ur at every step             */
    const uint32_t* d_counts;  /* uint32 [streams] or NULL: every stream takes all `steps` steps                */
} glv_track_tables;
int glv_batch_track_each_s16
    (glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_each_f32
    (glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_each_f32_planar
    (glv_batch* b, const float* d_rows, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, void* d_out, void* d_work, unsigned ops, void* hip_stream);
/* Track mode over a POOL of recordings: the per-stream entries above take [streams][pitch_frames], a private copy of a recording per stream, each padded to the
 * longest -- 1024 listeners of one five-minute recording hold it 1024 times, and a listener that joins, leaves or switches recordings costs a staging copy.
 * These entries take ONE buffer of pool_frames frames and a span per stream: where that stream's recording begins in the pool and how long it is.  Any number of
 * streams may name the same span, overlapping spans or disjoint ones; join, leave and switch are writes to d_spans and the tables.  Added within ABI 7; detect
 * by the symbol.  Everything not said here is glv_batch_track_each_s16 / _f32 / _f32_planar, word for word: glv_track_tables (rates, counts, the NULL rules), the
 * forms the ops and the batch select (windows; live on GLV_OP_BARS_ONLY batches; columns; the wave form), gl_storage 0, 1 and 3, channels 1 and 2, bufscale up to
 * 16, d_out, and d_work sized by glv_batch_track_at_work_bytes(b, steps, ops) -- there is no other query.  Capturable from the first call; nothing is allocated
 * or synchronised.
 *   Pool.    d_pool holds pool_frames frames: int16 [pool_frames][2], float [pool_frames][2], or for the planar entry float [2][pool_frames] -- channel c of frame
 *            i is d_rows[c * pool_frames + i], any pool_frames, no mono mix.  Aligned as the recordings of the per-stream entries are: 4, 8 and 4 bytes.  The pool
 *            may exceed 2^32 frames, which is why `first` is 64-bit and travels to the kernels in the span and not through the 32-bit tables.
 *   Windows. With k the batch's bufscale, window t of stream s begins at pool frame
 *                ext = frames[s] >= k n ? frames[s] - k n : 0
 *                w   = min(first[s] + min(d_starts[s * steps + t], ext), pool_frames - k n)
 *            evaluated in the kernels, in 64-bit arithmetic.  With well-formed spans (frames >= k n, first + frames <= pool_frames) the outer min never binds and
 *            no table can make a listener read another listener's recording: the guarantee is per stream, not per buffer.  With malformed spans no launch reads
 *            outside the pool.  The spans and the tables are read when the kernels run: rewriting them in stream order re-aims a captured hipGraph.
 *   Contract. Output, state afterwards, head, launches, glv_batch_last_launches and glv_batch_kernel_name are bit for bit those of glv_batch_track_each_* on the
 *            materialised copy d_pcm[s][i] = pool[first[s] + i], i < frames[s], at pitch_frames = max frames[s], with table entries pre-clamped to
 *            frames[s] - k n.
 *   Refused, launching nothing and leaving the batch untouched: what glv_batch_track_each_* refuses, in its words (a message that names pitch_frames shows
 *            pool_frames, saturated at 2^32 - 1); and with GLV_ERR_INVALID a NULL d_pool or d_spans, spans not 16-byte aligned, and pool_frames < k n.
 * Kernels: the transform in pool kinds of the frame kernel (glv_frame.h in_track_pool: the per-stream kinds with the stream's 16-byte span loaded where the table
 * entry is, one frame ahead of the address that needs it, and the start rule above -- glv_frame.h pool_window_start, which the tests mirror); under bufscale and in
 * the wave form glv_decimate_pool_kernel and glv_wave_pool_kernel (glv_pool.hip), the arithmetic of glv_decimate_kernel's track kinds and glv_wave_kernel's window
 * kinds behind the same rule.  The scan, bars, columns and slot kernels read no PCM and are the per-stream call's.  Every kernel that existed keeps its device
 * code byte for byte; registers, scratch and instruction counts of the new kinds beside their siblings: profiles/r26/track_pool_isa.txt.
 * Python: glava_amd.track_starts.pool_spans(lengths) packs recordings into a pool, each on a group of 8 frames, and returns the `first` offsets. */
typedef struct glv_track_span {
    uint64_t first;     /* first frame of the stream's recording, counted from the pool's first frame */
    uint32_t frames;    /* its length in frames */
    uint32_t reserved;  /* never read */
} glv_track_span;       /* one per stream, device memory, 16-byte aligned records */
int glv_batch_track_pool_s16
    (glv_batch* b, const int16_t* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, void* d_out, void* d_work,
     unsigned ops, void* hip_stream);
int glv_batch_track_pool_f32
    (glv_batch* b, const float* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, void* d_out, void* d_work,
     unsigned ops, void* hip_stream);
int glv_batch_track_pool_f32_planar
    (glv_batch* b, const float* d_rows, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, void* d_out, void* d_work,
     unsigned ops, void* hip_stream);
/* Track mode at render frames PER STREAM: glv_batch_track_frames_* takes one row of frame tables, one frame count and one keep pair for the whole batch, and
 * cannot reach the per-stream or pool updates.  Listeners at a 60 Hz and a 144 Hz display of the same recording have different frame counts, different d_mod
 * rows and different keep pairs (glava_amd.track_starts.live_session_frames(22050, 60, ...) against (22050, 144, ...)).  These entries give every stream its own
 * rows of the three frame tables, its own number of frames and its own keep pair, on the updates of glv_batch_track_each_* or glv_batch_track_pool_*; stream s
 * then behaves as if it were alone in a one-stream batch running glv_batch_track_frames_*, bit for bit.  Added within ABI 7; detect by the symbol.
 * Sized by glv_batch_track_frames_work_bytes(b, steps, frames, ops) with frames the longest row: the rows add no region, and there is no other query.
 *   Updates.   tb, steps, d_pcm / d_rows and pitch_frames, or d_pool, pool_frames and d_spans, are glv_batch_track_each_* / _pool_* 's arguments, word for word:
 *              their refusals in their words, and the batch's state afterwards, the head and the ring turned by steps - c_s exactly what those calls leave;
 *              c_s = min(d_counts[s], steps), or steps where d_counts is NULL.
 *   Keyframes. Keyframe k < 2 of stream s is d_keys[k]'s rows of stream s, keyframe k >= 2 the finished float row of that stream's step k - 2.  Every index read
 *              from d_from, d_to or d_keep is clamped in the kernel to c_s + 1 -- the clamp that stream's one-stream call applies -- so no launch reads outside
 *              d_keys, the steps' rows or the tables whatever they hold, and no stream sees a zero row written behind its count.  A stream with c_s == 0 lerps
 *              between its two carried keyframes only.
 *   Frames.    f_s = min(d_frame_counts[s], frames), evaluated on the device (NULL: frames).  For j < f_s rows 2 s and 2 s + 1 of block j of d_out follow
 *              glv_batch_track_frames_* 's rule with stream s's entries d_from[s * frames + j], d_to[...], d_mod[...]: from == to gives that keyframe's own bits,
 *              else s + ((e - s) * mod) in three float operations without contraction, then the upload's quantiser; the stage the ops select then runs over
 *              frames * streams * 2 rows.  For j >= f_s the frames stage writes zero texels and the output row is what the last stage makes of a zero texel
 *              row -- defined, nothing stale.  No table entry at j >= f_s is read.  d_out stays frame-major: [frames][streams][2][w].
 *   Write-back. d_keys[0] of stream s <- keyframe d_keep[2 s], d_keys[1] <- keyframe d_keep[2 s + 1], both read before either is written.  Any pair is safe (a
 *              lane reads and writes element i only): the host's rule (0, 1), (1, k), (k, k') cannot be checked for a table in device memory and is not
 *              imposed.  (0, 1) leaves a stream's keys as they were.  Chunks compose per stream, as the lockstep call's do.
 *   Equivalence. For every stream with c_s >= 1 and f_s >= 1 its rows of blocks j < f_s and its d_keys afterwards are bit for bit what glv_batch_track_frames_*
 *              gives on a one-stream batch that holds the stream's state and recording (pool entries: its materialised span with pre-clamped entries), with
 *              steps = c_s, frames = f_s, the stream's rows, and its keep pair where the host accepts that pair.  With equal rows for all streams, NULL counts
 *              and equal keep pairs the call is bit for bit glv_batch_track_frames_*.
 *   Refused, launching nothing and leaving the batch untouched: everything glv_batch_track_frames_* refuses about ops, storage and frames, everything the
 *              per-stream or pool call refuses, and with GLV_ERR_INVALID fe NULL or not aligned like a pointer, any of its pointers NULL except
 *              d_frame_counts, a table not 4-byte aligned, d_keys not 16-byte aligned, frames == 0.  GLV_OP_WAVE is refused: the wave form per stream has entries
 *              of its own, glv_batch_track_each_wave_frames_* / glv_batch_track_pool_wave_frames_* below.
 * Launches (glv_batch_last_launches): the per-stream call's without bars, + 2 (glv_track_frames_each_kernel, glv_track_keys_each_kernel), + 1 with GLV_OP_BARS.
 * Stream-ordered and capturable from the first call; all tables, counts and keep pairs are read when the kernels run, so rewriting them re-aims a captured
 * graph.  glv_batch_kernel_name reports "glv_track_frames_each_kernel".
 * Kernels (glv_track_frames.hip): glv_track_frames_kernel's walk -- four bins a lane, both keyframes in registers, table entries 4 frames ahead, one wave a
 * workgroup looping over [segment][row][group] items -- with the table base (row >> 1) * frames, last_key from the stream's count, the walk stopped at f_s and
 * zeros behind it.  The tables and counts are read through uniform (scalar) loads, which do not queue behind the chain of 512-byte stores.  Every kernel that
 * existed keeps its source.
 * Python: glava_amd.track_starts.stack_frame_tables(rows) pads per-stream (from, to, mod, keep_from, keep_to) tuples to the longest and returns the three
 * tables, the frame counts and the keep array. */
typedef struct glv_track_frames_each {
    const uint32_t* d_from;          /* uint32 [streams][frames], device, 4-byte aligned: row s is stream s's table   */
    const uint32_t* d_to;            /* uint32 [streams][frames]                                                       */
    const float*    d_mod;           /* float  [streams][frames], applied as given                                     */
    const uint32_t* d_frame_counts;  /* uint32 [streams] or NULL: every stream takes all `frames` frames               */
    const uint32_t* d_keep;          /* uint32 [streams][2], device: the keyframes written back to d_keys[0] / [1]     */
    uint32_t        frames;          /* longest row, >= 1                                                              */
    float*          d_keys;          /* float [2][streams][2][n], caller-owned, 16-byte aligned                        */
} glv_track_frames_each;
int glv_batch_track_each_frames_s16
    (glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe, void* d_out, void* d_work,
     unsigned ops, void* hip_stream);
int glv_batch_track_each_frames_f32
    (glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe, void* d_out, void* d_work,
     unsigned ops, void* hip_stream);
int glv_batch_track_each_frames_f32_planar
    (glv_batch* b, const float* d_rows, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe, void* d_out, void* d_work,
     unsigned ops, void* hip_stream);
int glv_batch_track_pool_frames_s16
    (glv_batch* b, const int16_t* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
     void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_pool_frames_f32
    (glv_batch* b, const float* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
     void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_pool_frames_f32_planar
    (glv_batch* b, const float* d_rows, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
     void* d_out, void* d_work, unsigned ops, void* hip_stream);
/* Track mode at render frames per stream FOR THE WAVE MODULE: the reference switches interpolation off only for binds that carry an fft transform (render.c:2131-2135,
 * :2161-2168), so the wave module lerps on every gl_storage, the shipped `setaccelfft true` included -- listeners at 60 Hz and 144 Hz displays of shared
 * recordings are its ordinary case.  These entries are glv_batch_track_wave_frames_* with everything per stream: the argument lists of
 * glv_batch_track_each_frames_* / glv_batch_track_pool_frames_*, the same two structures, no new sizing query.  Added within ABI 7; detect by the symbol.
 * Sized by glv_batch_track_wave_frames_work_bytes(b, steps, fe->frames, ops) with frames the longest row: 256 without bars, the frames' rows with bars.
 *   ops.       GLV_OP_WAVE [| GLV_OP_BARS] [| GLV_OP_R16], on every batch glv_batch_track_wave_frames_* takes them on: any gl_storage, channels 1 and 2, the
 *              pre-smoothing pass, bar texels, fewer than 256 bars, maximum / hybrid.  The planar kinds do no mono mix.
 *   Steps.     tb->d_starts is uint32 [streams][steps]; tb->d_ur must be NULL (GLV_ERR_INVALID in the per-stream call's words: no gravity reads a rate table).
 *              tb->d_counts is ACCEPTED here, unlike in glv_batch_track_each_* 's wave form: c_s = min(d_counts[s], steps) is the number of keyframes stream s
 *              contributes, NULL means steps.  Nothing is computed per step.
 *   Keyframes. Keyframe k < 2 of stream s is rows 2 s, 2 s + 1 of d_keys[k]; keyframe k >= 2 is (u + 1.0F) / 2.0F of the backend's unpack u of the window of
 *              step k - 2, which begins min(d_starts[s * steps + k - 2], pitch_frames - n) frames into the stream's recording, or for the pool entries at pool frame
 *              min(first[s] + min(entry, frames[s] - n or 0), pool_frames - n) of its span, evaluated in the kernel in 64-bit arithmetic (glv_batch_track_pool_* 's
 *              rule).  Every index read from d_from, d_to or d_keep is clamped in the kernels to c_s + 1.  A stream with c_s == 0 lerps between its two carried
 *              keyframes and reads neither its recording, its span nor its row of d_starts.  Whatever tables, counts and spans hold, no launch reads outside the
 *              recordings or the pool, d_keys, [0, steps) of a stream's starts row, or [0, f_s) of its frame rows.
 *   Frames.    f_s = min(d_frame_counts[s], frames), NULL: frames.  For j < f_s: from == to gives the keyframe's own bits, otherwise s + ((e - s) * mod) in three
 *              float operations without contraction; then the upload's quantiser, then what a GLV_OP_WAVE process call with these ops does.  For j >= f_s the
 *              frames stage writes zero texels and the output row is what the last stage makes of a zero texel row: 0 texels, 0.0f, or the bars of a zero row.
 *              No table entry at j >= f_s is read.  d_out stays frame-major: [frames][streams][2][w].
 *   Write-back. Per stream d_keys[0] <- keyframe d_keep[2 s], d_keys[1] <- keyframe d_keep[2 s + 1], both clamped, both read before either is written; any pair
 *              is safe (a lane reads and writes its own elements only).  Chunks compose per stream.
 *   Equivalence. A stream with c_s >= 1 and f_s >= 1 is bit for bit glv_batch_track_wave_frames_* on a one-stream batch with its recording (pool entries: its
 *              materialised span with entries pre-clamped), steps = c_s, frames = f_s, its rows, its rows of d_keys, and its keep pair where the host accepts that
 *              pair.  With equal rows, NULL counts and equal keep pairs the call is bit for bit the lockstep call.  The batch's state is not touched.
 *   Refused, launching nothing: everything glv_batch_track_wave_frames_* refuses about ops, batch and frames (bufscale > 1 among it, as every wave form);
 *              everything the vetting of glv_track_frames_each refuses (fe NULL or not aligned like a pointer, any of its pointers NULL except d_frame_counts, a
 *              table not 4-byte aligned, d_keys not 16-byte aligned, frames == 0); the per-stream and pool calls' refusals about tb, d_starts, d_spans and
 *              pool_frames; ops without GLV_OP_WAVE (FFT chains: glv_batch_track_each_frames_* / glv_batch_track_pool_frames_*).
 * Launches (glv_batch_last_launches): 2 (glv_wave_frames_each_kernel, glv_wave_keys_each_kernel), 3 with GLV_OP_BARS.  Kernels only: nothing is allocated or
 * synchronised, and the first call is capturable; all tables, counts, keep pairs and spans are read when the kernels run, so rewriting them re-aims a captured
 * graph.  glv_batch_kernel_name reports "glv_wave_frames_each_kernel".
 * Kernels (glv_track_frames.hip): glv_wave_frames_kernel's walk -- four frames of both channel rows a lane, both keyframes in registers, table entries 4 frames
 * ahead, one wave a workgroup looping over [segment][stream][group] items -- with the table base stream * frames, last_key from the stream's count, the walk
 * stopped at f_s and zeros behind it; tables, counts, starts and spans are read through uniform (scalar) loads.  Every kernel that existed keeps its device code
 * byte for byte; registers, scratch and instruction counts of the new kernels beside their lockstep siblings: profiles/r28/track_wave_frames_each_isa.txt.
 * Python: the tables are glava_amd.track_starts.stack_tables, stack_frame_tables and pool_spans, as for the FFT entries. */
int glv_batch_track_each_wave_frames_s16
    (glv_batch* b, const int16_t* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe, void* d_out, void* d_work,
     unsigned ops, void* hip_stream);
int glv_batch_track_each_wave_frames_f32
    (glv_batch* b, const float* d_pcm, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe, void* d_out, void* d_work,
     unsigned ops, void* hip_stream);
int glv_batch_track_each_wave_frames_f32_planar
    (glv_batch* b, const float* d_rows, uint32_t pitch_frames, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe, void* d_out, void* d_work,
     unsigned ops, void* hip_stream);
int glv_batch_track_pool_wave_frames_s16
    (glv_batch* b, const int16_t* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
     void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_pool_wave_frames_f32
    (glv_batch* b, const float* d_pool, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
     void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_track_pool_wave_frames_f32_planar
    (glv_batch* b, const float* d_rows, uint64_t pool_frames, const glv_track_span* d_spans, const glv_track_tables* tb, uint32_t steps, const glv_track_frames_each* fe,
     void* d_out, void* d_work, unsigned ops, void* hip_stream);
/* device pointer to the gravity state float [streams][2][n] == the latest output of a chain ending in gravity: the
 * batch-owned buffer, or the caller's d_out of the latest call when that doubles as the state (GLV_OP_OUTPUT_IS_STATE).
 * GLV_ERR_STATE if the batch was created without GLV_OP_GRAVITY, after fused gravity + average calls (the state is
 * then the newest slot of the history ring, float [rows][F][n] -- not an array of this shape), and with gl_storage == 1 (the
 * state is uint16 texels). */
int glv_batch_gravity_state(glv_batch* b, const float** d_state);
/* same from planar f32 (the lb/rb snapshot) */
int glv_batch_process_f32(glv_batch* b, const float* d_f32, float* d_out, unsigned ops, void* hip_stream);

/* same from interleaved stereo f32 frames, float [streams][n][2] -- the layout the PulseAudio backend
 * receives (glava/pulse_input.c:155-178); channels == 1 mixes (L + R) / 2 in float (pulse_input.c:167) */
int glv_batch_process_f32_stereo(glv_batch* b, const float* d_pcm, float* d_out, unsigned ops, void* hip_stream);

/* `setbufscale k` of rc.glsl (rd_update's box decimation, render.c:1765-1790) for a batch.  Added within ABI 7: detect it by the symbol.  With transform
 * size n and bufscale k a window of every call below is k * n frames (GLava's bufsize), and channel sample t of it is
 *     acc = 0.0F; for a in 0..k-1: acc = acc + x[t*k + a]; acc = acc / (float) k
 * of the backend's unpack x of the frames (s16: v / 65535.0F, channels == 1: ((l + r) / 2) / 65535.0F in C integer arithmetic, fifo.c:94-110; f32: the sample,
 * channels == 1: (l + r) / 2.0F) -- every addition and the one division rounded float32 operations in that order, no fused multiply-add, no reciprocal, no
 * integer pre-sum; a window whose first sample is -0.0F gives +0.0F.  Everything behind it is what the library computes from planar float rows of n samples.
 *   glv_batch_set_bufscale   k = 1: off, the default; 2..GLV_MAX_BUFSCALE.  Like glv_batch_set_params it is synchronous and the only place the feature
 *       allocates: a batch-owned staging array of streams * 2 * n floats (k = 1 frees it; on failure the batch stays as it was).  State, head, tables, bar and
 *       column texels are kept; glv_batch_set_params and glv_batch_reset keep k.  GLV_ERR_INVALID: k = 0, k > GLV_MAX_BUFSCALE, k * n > 2^21.  GLV_ERR_STATE: a
 *       single-row batch (the drop-ins'), a batch created with GLV_OP_RING_S16 / GLV_OP_RING_F32.  With k = 1 every entry runs the code path it has always run.
 *   Process calls while k > 1: glv_batch_process_s16 and glv_batch_process_f32_stereo read [streams][k*n][2], glv_batch_process_f32 reads planar
 *       [streams][2][k*n] (the lb / rb rd_update itself decimates: no mix).  One launch (glv_decimate_kernel) writes the staging rows, then the chain
 *       glv_batch_process_f32 plans on this batch for the same ops runs on them; what that entry refuses is refused in its words.  glv_batch_last_launches and
 *       the timing pair count the extra launch.  The calls never allocate and can be captured into a hipGraph from the first one on.
 *   Track calls on FFT chains while k > 1 (glv_batch_track_windows_*, _columns_*, _live_*, _at_*, _rates_*, _frames_*, s16 and f32): window t of a stream is
 *       the k * n frames from t * hop, or from min(starts[t], pitch_frames - k * n) for a table call -- the pitch rules and the kernel's clamp use k * n, no launch
 *       reads outside the recordings whatever a table holds.  One launch writes every window's decimated rows, steps * streams * 2 * n floats, into a new FIRST
 *       region of the workspace (the *_work_bytes queries answer for the batch as it is; a stateless chain without bars needs the workspace for these rows
 *       alone), the stateless transform runs once over them, and the scan, bars, columns, frames and key write-back stages run unchanged.  Keyframes of a frames
 *       call are rows of n, as the reference's interpolate_buf of bufsize / bufscale is (render.c:1681); the tables and d_keys do not change.
 *   GLV_ERR_STATE while k > 1, each naming glv_batch_set_bufscale: glv_batch_track_s16 (its residues rest on back-to-back windows of n frames),
 *       glv_batch_track_wave_* and glv_batch_track_wave_frames_*, the ring entries, glv_batch_autotune and glv_batch_tune_placement. */
#define GLV_MAX_BUFSCALE 16
int      glv_batch_set_bufscale(glv_batch* b, uint32_t k);
uint32_t glv_batch_bufscale(const glv_batch* b);

/* FIFO ring mode (glava/fifo.c:91-112): the batch keeps an n-frame s16 ring per stream in
 * HBM; each call appends `new_frames` (= sample_sz/4, fifo.c:38,91) stereo frames per
 * stream (d_new int16 [streams][new_frames][2]; NULL => poll-timeout zero fill,
 * fifo.c:67-79), then transforms the whole window. */
int glv_batch_ring_update_s16(glv_batch* b, const int16_t* d_new, uint32_t new_frames, float* d_out,
                              unsigned ops, void* hip_stream);
/* the same ring kept in interleaved f32 frames -- the PulseAudio backend's update (glava/pulse_input.c:
 * 155-178: shift both rings left by sample_sz/4, append sample_sz/4 stereo f32 frames; channels == 1 mixes
 * (L + R) / 2 in float).  d_new: float [streams][new_frames][2]; no zero-fill path (pa_simple_read blocks). */
int glv_batch_ring_update_f32(glv_batch* b, const float* d_new, uint32_t new_frames, float* d_out, unsigned ops,
                              void* hip_stream);

/* The rings on their own (the audio-backend seam, glava/fifo.h:9-20): append an update without transforming, and read the
 * rings the way the reference's backends publish them in audio_out_l / audio_out_r -- planar f32, oldest sample first
 * (fifo.c:91-110: memmove + unpack; pulse_input.c:155-176: memmove + deinterleave; channels == 1: the mono mix in both).
 * d_planar: float [streams][2][n].  f32_ring: 0 = the s16 ring, 1 = the interleaved f32 ring.  A backend that keeps
 * struct audio_data's contract downloads this; one that publishes spectra calls glv_batch_ring_update_* instead. */
int glv_batch_ring_append_s16(glv_batch* b, const int16_t* d_new /* NULL = zero fill, fifo.c:67-79 */, uint32_t new_frames, void* hip_stream);
int glv_batch_ring_append_f32(glv_batch* b, const float* d_new, uint32_t new_frames, void* hip_stream);
int glv_batch_ring_planar(glv_batch* b, int f32_ring, float* d_planar, void* hip_stream);

/* Ring batches in track mode: SEVERAL updates of a live stream in one call.  Added within ABI 7: detect them by the symbol.  A packet or a decoder block holds
 * several updates' worth of frames, and a host that stalled has several to catch up; these entries run `updates` ring updates of new_frames frames each as one
 * track call instead of a loop of glv_batch_ring_update_* calls.
 *   d_new   [streams][updates * new_frames][2], each stream's new frames back to back: int16, 4-byte aligned (NULL: zero fill, as glv_batch_ring_update_s16), or
 *           float, 8-byte aligned (NULL is refused, as by glv_batch_ring_update_f32).
 *   d_out   the layout of glv_batch_track_at_s16 / _f32 on the same batch and ops: [updates][streams * 2][row], step-major -- floats, GL_R16 texels, bars, bar
 *           texels or columns, as the ops and the batch's settings select.
 *   d_work  glv_batch_ring_track_work_bytes(b, new_frames, updates, ops) bytes, 256-byte aligned; one query sizes both entries.
 * Contract.  Let R_s be stream s's ring read oldest frame first (n frames) followed by its updates * new_frames new frames.  Update t (from 0) transforms frames
 * [(t + 1) * new_frames, (t + 1) * new_frames + n) of R_s -- the window the t-th of `updates` sequential glv_batch_ring_update_* calls sees -- and every output
 * row, the gravity and average state, head and the rings (read oldest first; where the library puts the ring's write position is its own business) are bit for
 * bit those of the sequential calls.  updates * new_frames may be smaller than n, equal to it or larger.  The call is also bit for bit glv_batch_track_at_s16 /
 * _f32 on the materialised R_s with starts[t] = (t + 1) * new_frames, and takes every form that entry selects on the batch (windows, live, columns, GLV_OP_WAVE;
 * with and without GLV_OP_BARS / GLV_OP_R16; gl_storage 0, 1 and 3; channels 1 and 2); what that entry refuses for the batch and the ops is refused here in its
 * words, before anything moves.
 * Workspace, in order, each region a multiple of 256 bytes: the staged R_s, streams * pitch frames with pitch = n + updates * new_frames rounded up to 4 frames
 * (at the frame size of the widest ring the batch has); the table of starts, updates * 4 bytes; then what glv_batch_track_at_work_bytes(b, updates, ops) answers.
 * Launches (glv_batch_last_launches): the table call's for the form, plus 2 -- one that stages R_s and writes the table (glv_ring_stage_kernel) in front and one
 * that writes the last n frames of every R_s back as the ring (glv_ring_keep_kernel) behind:
 *       FFT chain                 3 without state and bars; + 1 with GLV_OP_GRAVITY / GLV_OP_AVERAGE (the scan); + 1 with GLV_OP_BARS (bars, bar texels or columns)
 *       GLV_OP_WAVE               3; 4 with GLV_OP_BARS
 * The call is stream-ordered, allocates nothing, synchronises nothing and can be captured into a hipGraph from the first call on.
 * GLV_ERR_INVALID: a NULL batch, d_out or d_work; new_frames outside [1, n]; updates == 0; more than 2^32 rows (updates * streams * 2) or frames (n + updates *
 * new_frames) in one call; d_new not aligned like a frame; the f32 entry with d_new == NULL; d_work not 256-byte aligned.  GLV_ERR_STATE: a batch without the
 * ring of that kind (the query: without any ring), a single-row batch.  (A batch with bufscale cannot occur: glv_batch_set_bufscale refuses ring batches.)  A
 * refused or failed call leaves ring, position, head and state as the caller saw them. */
uint64_t glv_batch_ring_track_work_bytes(const glv_batch* b, uint32_t new_frames, uint32_t updates, unsigned ops);   /* 0: refused, glv_last_error says why */
int glv_batch_ring_track_s16(glv_batch* b, const int16_t* d_new, uint32_t new_frames, uint32_t updates,
                             void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_ring_track_f32(glv_batch* b, const float* d_new, uint32_t new_frames, uint32_t updates,
                             void* d_out, void* d_work, unsigned ops, void* hip_stream);

/* Ring batches in track mode PER STREAM: own update counts and rates.  Added within ABI 7: detect them by the symbol.  A live service is not in lockstep: one
 * listener has four updates pending, the next one, a paused one none, and a live GLava applies gravity at the rate it measures (1.0, then 59.0, then 60.0).
 * These entries are glv_batch_ring_track_s16 / _f32 with a count of updates and a row of rates for every stream, as glv_batch_track_each_* is the table call
 * with them.
 *   updates   the longest row: it sizes d_new, d_out and the workspace.
 *   d_counts  uint32 [streams] in device memory, 4-byte aligned, or NULL: stream s takes c_s = min(d_counts[s], updates) updates; NULL: everybody takes all.
 *   d_ur      float [streams][updates] in device memory, 4-byte aligned, or NULL: update t of stream s applies gravity with ur = d_ur[s * updates + t], as
 *             glv_batch_track_each_* does; NULL: the batch's own ur.  The batch's ur stays.  Both tables are read when the kernels run.
 *   d_new     [streams][updates * new_frames][2]: the pitch is set by `updates`; of stream s only the first c_s * new_frames frames are read, what lies behind
 *             may be anything.  int16, 4-byte aligned (NULL: zero fill), or float, 8-byte aligned (NULL is refused).
 *   d_out     [updates][streams * 2][row], the layout of glv_batch_track_each_*: rows of updates t >= c_s are what that call writes behind a count, the result
 *             of a zero row.
 *   d_work    glv_batch_ring_track_each_work_bytes(b, new_frames, updates, ops) bytes, 256-byte aligned; one query sizes both entries.
 * Contract.  Let R_s be stream s's ring read oldest frame first (n frames) followed by its first c_s * new_frames new frames.  Update t < c_s transforms frames
 * [(t + 1) * new_frames, (t + 1) * new_frames + n) of R_s, and after the call the stream's ring, read oldest first, is the last n frames of R_s (where the
 * library puts the ring's write position is its own business: one position serves every stream).  Every stream is, bit for bit in output rows, gravity and
 * average state and ring, what c_s sequential glv_batch_ring_update_* calls make of a one-stream ring batch holding that stream's state, with
 * glv_batch_set_params(ur = d_ur[s][t]) before update t where a rate table is given.  A stream with c_s = 0 keeps its state and its ring (read oldest first) bit
 * for bit.  head advances by `updates`, as in every per-stream call.  With d_counts == NULL and d_ur == NULL the call is bit for bit glv_batch_ring_track_*; it
 * is also bit for bit glv_batch_track_each_* on the staged recordings (R_s padded with zeros) with the rows starts[s][t] = (t + 1) * new_frames, and takes every
 * FFT form that entry selects on the batch (windows, live, columns; with and without GLV_OP_BARS / GLV_OP_R16; gl_storage 0, 1 and 3; channels 1 and 2).
 * Workspace, in order, each region a multiple of 256 bytes: the staged R_s, streams * pitch frames with pitch = n + updates * new_frames rounded up to 4 frames
 * (at the frame size of the widest ring the batch has); the table of starts, streams * updates * 4 bytes; then what glv_batch_track_at_work_bytes(b, updates,
 * ops) answers.
 * Launches (glv_batch_last_launches): the per-stream table call's for the form, plus 2 (glv_ring_stage_each_kernel in front, glv_ring_keep_each_kernel behind):
 * 3 without state and bars; + 1 with GLV_OP_GRAVITY / GLV_OP_AVERAGE (the scan); + 1 with GLV_OP_BARS.  The transform runs for updates behind a count too.
 * The call is stream-ordered, allocates nothing, synchronises nothing and can be captured into a hipGraph from the first call on; rewriting d_counts, d_ur or
 * d_new re-aims a captured graph.
 * GLV_ERR_INVALID: GLV_OP_WAVE (no state for a count or a rate to act on: glv_batch_ring_track_s16 / _f32 take the wave form); what glv_batch_ring_track_*
 * refuses, in its words; d_ur or d_counts off 4 bytes; d_ur without GLV_OP_GRAVITY; d_counts on a chain without GLV_OP_GRAVITY and GLV_OP_AVERAGE -- the last
 * three in glv_batch_track_each_*'s words.  GLV_ERR_STATE: as glv_batch_ring_track_*.  A refused or failed call leaves ring, position, head, gravity form and
 * state as the caller saw them, and a refused call launches nothing. */
uint64_t glv_batch_ring_track_each_work_bytes(const glv_batch* b, uint32_t new_frames, uint32_t updates, unsigned ops);   /* 0: refused, glv_last_error says why */
int glv_batch_ring_track_each_s16(glv_batch* b, const int16_t* d_new, uint32_t new_frames, uint32_t updates,
                                  const float* d_ur, const uint32_t* d_counts, void* d_out, void* d_work, unsigned ops, void* hip_stream);
int glv_batch_ring_track_each_f32(glv_batch* b, const float* d_new, uint32_t new_frames, uint32_t updates,
                                  const float* d_ur, const uint32_t* d_counts, void* d_out, void* d_work, unsigned ops, void* hip_stream);

/* Stream slots: reset, save and load CHOSEN streams of a batch.  Added within ABI 7: detect them by the symbol.  In the reference every listener is a GLava of
 * its own that starts from calloc'd buffers and leaves when it likes; these calls give one stream of a batch that lifecycle (a listener that takes over a freed
 * slot: reset it), checkpoints for seeking under the track entries, moves between batches and compaction -- without touching the other streams.
 *
 * Common to the three calls: d_idx is uint32 [count] in device memory and is read when the kernel runs (like the tables of glv_batch_track_at_*); an entry
 * >= streams is skipped where it is read, its blob is then neither read nor written, and no launch touches memory outside the batch or the blobs whatever the
 * table holds.  d_blob is count * d->bytes bytes, 16-byte aligned; blob j belongs to d_idx[j].  Each call is ONE launch (glv_slots_kernel, reported by
 * glv_batch_last_launches), stream-ordered, allocates nothing and copies nothing synchronously: it can be captured into a hipGraph, and a captured reset can
 * be replayed at any time and re-aimed by rewriting d_idx.  Save and load take head and the ring positions when they are enqueued, as a process call does.
 * Duplicates in d_idx are harmless for reset and save; for load they are the caller's error: which blob wins is unspecified.
 *
 * The portable form of one stream (a blob) is the regions below in this order, present regions only (glv_stream_state_desc.regions), each a multiple of 16
 * bytes; elements are floats, or GL_R16 texels (uint16) on a gl_storage 1 batch:
 *   bit 0  gravity rows    [2][n] elements          the stream's rows of the batch's gravity store
 *   bit 1  average ring    [2][F][n] elements       oldest frame first: blob row q of a channel is ring slot (head + q) mod F, head being the slot that
 *                                                   receives the next frame (so blob row F - 1 is the newest, which is gravity's state in form 2)
 *   bit 2  s16 PCM ring    [n][2] int16             oldest frame first: blob frame q is ring frame (ring position + q) mod n
 *   bit 3  f32 PCM ring    [n][2] float             likewise with the f32 ring's position
 * No position of the source batch survives into a blob, and the batch that loads one rotates by its own positions.
 *
 *   glv_batch_stream_state_desc   what a blob of this batch is NOW (gravity_form and kept_bins follow the calls the batch has run).
 *   glv_batch_reset_streams       afterwards the listed streams are streams of a batch glv_batch_reset has just cleared, for every later process, ring and
 *       track call, in output and state, bit for bit; every other stream is untouched.  head, the ring positions, the gravity form and the live flag stay: zero
 *       state reads the same at every rotation and in both forms.  A batch with neither state nor ring: GLV_OK, no launch.
 *   glv_batch_save_streams        gathers the listed streams into d_blob and fills *d (the descriptor a later load checks).
 *   glv_batch_load_streams        scatters blobs into the listed streams: after save(A, i) and load(B, j), stream j of B continues exactly as stream i of A
 *       would have -- given the same input every later call writes the same output and leaves the same state, bit for bit, whatever head / ring positions
 *       the two batches are at, also with A == B (source and destination may overlap in the lists: a save completes before the load is enqueued).  Parameters
 *       (fft_scale, ur, bars, ...) are the caller's business, exactly as state is kept across glv_batch_set_params.  Checked on the host before anything
 *       runs, a refused call leaves the batch as it was: n, avg_frames, elem_bytes and regions must equal the batch's own (GLV_ERR_STATE); a blob of
 *       gravity_form 0 loads anywhere; a batch whose form is still 0 adopts the blob's (all its streams are zero, and zero is the same state in both
 *       forms); otherwise the forms must be equal (a batch keeps one form: see glv_batch_gravity_state); a blob with kept_bins == n loads into any such
 *       batch, a GLV_OP_BARS_ONLY one included (whole rows are a superset of what it keeps); a blob with kept_bins < n loads only into a GLV_OP_BARS_ONLY
 *       batch whose glv_batch_live_bins() are no more than it, which then counts as having run its live class and keeps the smaller of its own kept_bins and the blob's.
 * All three: GLV_ERR_INVALID for a NULL or misaligned pointer (d_idx 4 bytes, d_blob 16) and count == 0; GLV_ERR_STATE for a single-row batch (the glv_state
 * drop-ins') and while the batch's latest gravity output lives in the caller's buffer (GLV_OP_OUTPUT_IS_STATE in force: the library does not own that
 * memory); save and load also for a batch with neither state nor ring.  `setbufscale` plays no part: its staging rows are not state.
 * Blobs are plain device memory: moving one to another device (a stream that changes its glv_multi shard) is the caller's own peer copy. */
typedef struct glv_stream_state_desc {   /* host side; what a blob is, filled by the library */
    uint32_t n, avg_frames;
    uint32_t elem_bytes;      /* 4: float state (gl_storage 0 / 2 / 3), 2: GL_R16 texels (gl_storage 1) */
    uint32_t gravity_form;    /* the batch's form when asked: 0 none yet, 1 the gravity store, 2 the newest ring slot (gravity fused with average) */
    uint32_t regions;         /* bit 0 gravity rows, 1 average ring, 2 s16 PCM ring, 3 f32 PCM ring */
    uint32_t kept_bins;       /* n, or how far a GLV_OP_BARS_ONLY batch that has run its live class has kept its state: the smallest extent of its live calls since creation / glv_batch_reset (a process call: its live bins then; a live track call: its kept bins), not what it samples now */
    uint64_t bytes;           /* per stream */
} glv_stream_state_desc;
int glv_batch_stream_state_desc(const glv_batch* b, glv_stream_state_desc* d);
int glv_batch_reset_streams(glv_batch* b, const uint32_t* d_idx, uint32_t count, void* hip_stream);
int glv_batch_save_streams(glv_batch* b, const uint32_t* d_idx, uint32_t count, void* d_blob, glv_stream_state_desc* d, void* hip_stream);
int glv_batch_load_streams(glv_batch* b, const uint32_t* d_idx, uint32_t count, const void* d_blob, const glv_stream_state_desc* d, void* hip_stream);

/* Elastic batches: update the FIRST `count` streams only, and copy streams from slot to slot.  Added within ABI 7: detect them by the symbol.  A batch created
 * for a capacity then costs what its listeners cost: join = reset slot A, A += 1; leave slot i = copy slot A - 1 into i, A -= 1; every update = process the
 * first A streams; grow = create a larger batch, copy the A streams across, destroy the old one (glava_amd/stream_slots.py DensePool is that bookkeeping).
 *
 * glv_batch_process_first_s16 / _f32 / _f32_stereo, glv_batch_ring_update_first_s16 / _f32: each is the un-suffixed call of a batch that has `count` streams.
 * Input and output have the layouts of that call at streams = count, dense and stream-major (d_pcm [count][n][2], [count][k n][2] under bufscale k; d_out
 * [count][2][n] or what ops imply).  Streams 0 .. count - 1 get the output, bit for bit, and are left in the state of a batch created with `count` streams and fed
 * the same inputs since its creation or reset; nothing at or behind row 2 * count of d_out is written.  Every chain, gl_storage, GLV_OP_BARS, GLV_OP_BARS_ONLY,
 * GLV_OP_WAVE, bufscale, GLV_OP_OUTPUT_IS_STATE and glv_batch_set_grid behave as on the un-suffixed call, the same things are refused in the same words, the
 * launches and glv_batch_last_launches are the same; each call can be captured from the first call on and allocates nothing.  count == streams is exactly the
 * un-suffixed call.  GLV_ERR_INVALID: count == 0 or count > streams; GLV_ERR_STATE: a single-row batch.
 * THE BATCH'S LOCKSTEP POSITIONS ADVANCE AS FOR A FULL CALL -- head, the ring positions, the gravity form and the live flag are kept per batch.  Streams >= count
 * are neither read nor written, so their stored state stops matching the positions: it is undefined from then on.  A stream that enters the prefix later must
 * first be the target of glv_batch_reset_streams, glv_batch_load_streams or glv_batch_copy_streams: all three write whole streams at the batch's current
 * positions (zero state reads the same at every rotation).  The library cannot check this protocol -- which streams a call listed is device memory -- so it is
 * the caller's to keep.
 * Not offered in a prefix form: the track entries (a track call works on recordings, and its batch is made for the job), glv_batch_ring_append_* and
 * glv_batch_ring_planar, the tuners (glv_batch_autotune, glv_batch_tune_placement), glv_multi.
 *
 * glv_batch_copy_streams: for every j < count, stream d_dst_idx[j] of dst afterwards continues exactly as stream d_src_idx[j] of src would have -- the contract
 * of glv_batch_save_streams(src) followed by glv_batch_load_streams(dst), bit for bit in output and state, whatever head and ring positions the two batches are
 * at, without the blob: ONE launch (glv_slot_copy_kernel; glv_batch_last_launches(dst) == 1), stream-ordered, allocates nothing, can be captured.  Both tables are
 * uint32 [count] in device memory, read when the kernel runs (a captured copy is re-aimed by rewriting them); positions are taken when the call is enqueued.
 * A pair with either entry >= its batch's streams is skipped where it is read, and no launch touches memory outside the two batches' state arrays whatever the
 * tables hold.  Every other stream of both batches is untouched; src is only read.
 * dst == src is allowed (compaction): a stream named as a destination must then not be named as a source in the same call, and no destination may appear twice,
 * in either case -- the caller's error: the named destinations then hold unspecified contents, nothing else is touched.  A pair with equal entries leaves its
 * stream as it was.
 * Checked on the host before anything runs, a refused call leaves both batches as they were: glv_batch_load_streams' checks with src's descriptor as it is now
 * (glv_batch_stream_state_desc) in the blob's place -- n, avg_frames, elem_bytes, regions; the gravity form, which dst adopts when its own is still 0; kept_bins,
 * after which dst counts as having run its live class -- and for BOTH batches what all stream-slot calls refuse (NULL or misaligned table, count == 0, a
 * single-row batch, GLV_OP_OUTPUT_IS_STATE in force).  GLV_ERR_INVALID: batches on different devices (between devices a stream travels as a blob and the
 * caller's peer copy).  GLV_ERR_STATE: two batches with neither state nor ring. */
int glv_batch_process_first_s16(glv_batch* b, uint32_t count, const int16_t* d_pcm, float* d_out, unsigned ops, void* hip_stream);
int glv_batch_process_first_f32(glv_batch* b, uint32_t count, const float* d_f32, float* d_out, unsigned ops, void* hip_stream);
int glv_batch_process_first_f32_stereo(glv_batch* b, uint32_t count, const float* d_pcm, float* d_out, unsigned ops, void* hip_stream);
int glv_batch_ring_update_first_s16(glv_batch* b, uint32_t count, const int16_t* d_new, uint32_t new_frames, float* d_out, unsigned ops, void* hip_stream);
int glv_batch_ring_update_first_f32(glv_batch* b, uint32_t count, const float* d_new, uint32_t new_frames, float* d_out, unsigned ops, void* hip_stream);
int glv_batch_copy_streams(glv_batch* dst, const uint32_t* d_dst_idx, glv_batch* src, const uint32_t* d_src_idx, uint32_t count, void* hip_stream);

/* smooth_audio() bar sampling of spectra already in HBM (d_spec float [streams][2][n]) into
 * d_bars float [streams][2][bars]; what GLV_OP_BARS runs after the transform.  Refused on a gl_storage 3 batch (GLV_ERR_STATE): there GLV_OP_BARS samples the
 * upload's texels, and caller's float rows go through a gl_storage 0 batch. */
int glv_batch_bars(glv_batch* b, const float* d_spec, float* d_bars, void* hip_stream);

/* GLV_OP_BARS at texels of the pre-smoothed texture: bar k = texel t[k] of the pre-smoothing pass (bars = n, bar_phase 0.5), which is what the
 * shipped modules sample with setsmoothpass true -- smooth_audio(tex, sz, p) is then one texelFetch(tex, int(round(p * sz)), 0) (util/smooth.glsl:61-63;
 * radial/1.frag:69-71, bars/1.frag:64-90; glava_amd.bar_positions computes the t[k] of both modules).  Contract: with the table set,
 *     bars_out[row][k] == twin_out[row][t[k]]   bit for bit, as GL_R16 texels (GLV_OP_R16) and as floats,
 * where the twin is the same batch created with bars = n and bar_phase = 0.5, in its arithmetic (glv_batch_bars_arithmetic, which reports it):
 * GLV_BARS_I8_EXACT -- texel floor(sum W_j c_j / 2^P + 1/2), float (float) (ldexp((double) sum W_j c_j, -P) / 65535), the integer weights of the twin's
 * row t[k] (oracle glvo_bars_int_at) -- for sample_mode average, GLV_BARS_F32_SEQ for maximum / hybrid.  In one launch where the transform kernel
 * takes the bars (the GL_R16 chain, gl_storage 1, sample_mode average, whenever the unsnapped bars of the configuration fuse), else as a second launch.
 *   texels == NULL or count == 0: off -- the unsnapped bars again, bit for bit.  Synchronous, may allocate (like glv_batch_set_params).
 *   Refused: count != bars or any t[k] >= n (GLV_ERR_INVALID); a batch created without GLV_OP_BARS or with gl_storage 0 (GLV_ERR_STATE: a float chain
 *   has no pre-smoothed texture -- true of 0, the operators alone; gl_storage 3, the same chain followed by the upload, takes the table: the twin's rows are
 *   then the upload's texels of the finished float rows, stateless FFT chains included, in one launch where the GL_R16 chain would fuse the same table); a twin whose arithmetic would be GLV_BARS_F32_MATRIX (GLV_ERR_INVALID, glv_last_error says why).
 *   While a table is set: glv_batch_set_params that changes bars or sets gl_storage 0 (a float chain has no pre-smoothed texture: true of 0, not of 3),
 *   glv_batch_bars, and GLV_OP_BARS calls that are not a GL chain
 *   (GLV_OP_FFT with gravity / average, no GLV_OP_SMOOTH; gl_storage 3: any GLV_OP_FFT chain without GLV_OP_SMOOTH / GLV_OP_RAW) or GLV_OP_WAVE | GLV_OP_BARS (the same contract over the wave texture: the twin is the same
 *   GLV_OP_WAVE | GLV_OP_BARS call with bars = n, bar_phase 0.5; always a second launch) are refused with GLV_ERR_STATE; a change of smooth_factor or of the shape rebuilds the
 *   table's taps.  glv_batch_reset keeps the table, glv_batch_destroy frees it.
 * glv_batch_live_bins: every snapped position lies in [0, 1), which the live bins already cover whenever smooth_factor >= 1 / bars (the unsnapped
 * last bar then reaches smooth_audio()'s last bin); a smaller factor grows them to the snapped taps' reach -- refused on a GLV_OP_BARS_ONLY batch
 * that has already run its live class when that is beyond what it kept (glv_stream_state_desc.kept_bins; glv_batch_reset first).  A table that shrinks the
 * live bins, and clearing one, are accepted. */
int glv_batch_set_bar_texels(glv_batch* b, const uint32_t* texels, uint32_t count);

/* GLV_OP_BARS as the columns of the graph module: the float mean of THREE texels of the pre-smoothed texture per column, which is what graph/1.frag:87-88
 * draws from with setsmoothpass true -- smooth_audio_adj (util/smooth.glsl:67-73) fetches at idx - pixel, idx, idx + pixel and returns (al + am + ar) / 3.0F.
 * texels is [count][3]: left, middle, right (glava_amd.bar_positions.graph_column_texels computes the table of a window width).  Contract: with the table
 * set, a GLV_OP_BARS call on a GL chain writes, for every row and column x,
 *     out[row][x] == fdiv(fadd(fadd(T(l), T(m)), T(r)), 3.0f)   bit for bit, as floats,
 * where T(t) is the float of GL_R16 texel c = the twin's texel t of that row: c / 65535 correctly rounded, what texelFetch returns.  The twin is the same
 * batch with bars = n, bar_phase 0.5, GLV_OP_R16, in the arithmetic glv_batch_bars_arithmetic reports (GLV_BARS_I8_EXACT for sample_mode average,
 * GLV_BARS_F32_SEQ for maximum / hybrid).  Plain IEEE float additions in that order and a true division by 3: no fused multiply-add, no reciprocal.
 * Internally the table is a bar-texel table over the DISTINCT texels (neighbouring columns share them: 401 columns read 801 texels, not 1203) plus an
 * index map.  In one launch where the transform kernel takes the bars (as glv_batch_set_bar_texels) and the distinct texels fit behind its row in LDS as
 * 16-bit values -- (distinct + 1) <= 4 x the configuration's lanes per row, 511 texels at N = 4096 and 1023 at N = 16384 as shipped; else a second launch (glv_columns_kernel) over the
 * chain's rows, which keeps a row's texels in LDS: no texel array in HBM either way.
 *   texels == NULL or count == 0: off -- the batch behaves as before, bit for bit.  Synchronous, may allocate (like glv_batch_set_params).
 *   Refused: count != bars, any entry >= n, more than 32766 distinct texels (GLV_ERR_INVALID); setting this table while bar texels are set, or bar texels
 *   while this one is set (GLV_ERR_STATE: clear the other first); GLV_OP_R16 in a call while columns are set (GLV_ERR_STATE: a mean of three texels is not
 *   a texel).  Every other refusal, the glv_batch_set_params / glv_batch_reset / glv_batch_destroy rules and the glv_batch_live_bins rule are those of
 *   glv_batch_set_bar_texels.  Added within ABI 7 without a version change: detect it by the symbol.
 * Measured (64 K streams, N = 4096, GLV_OP_BARS_ONLY, log_mode 1, one MI355X; profiles/r08/column_texels.txt) against the twin plus a gather-and-average of
 * its texels: a 320-pixel window (321 texels, one launch) 1.61 ms against 2.09 ms; an 800-pixel window (801 texels, second launch) 4.08 ms against 3.23 ms;
 * 1920 pixels (1921 texels) 8.23 ms against 5.95 ms.  So at N = 4096 the call pays where the columns fuse -- windows up to 510 pixels wide -- and from
 * there on a caller is better served by the twin and its own gather; the second launch is kept for the contract (every table works), not for speed. */
int glv_batch_set_column_texels(glv_batch* b, const uint32_t* texels /* [count][3]: left, middle, right */, uint32_t count);

/* Kernel-time accounting for the roofline report: HIP events recorded on the caller's
 * stream around every launch between begin/end; returns accumulated milliseconds and the
 * number of launches of the dominant (FFT) kernel. */
int glv_batch_timing_begin(glv_batch* b);
int glv_batch_timing_end(glv_batch* b, double* kernel_ms, uint64_t* launches);

/* Algorithmic HBM bytes one process call moves for the given ops: what the CHAIN must move -- input, state
 * read and written, output.  Rows that one launch of a multi-launch chain hands to the next (the uint16 `av` rows in front of the
 * pre-smoothing pass, bars that are not computed inside the transform's launch) are traffic of the organisation, not of the problem, and
 * are not counted -- except gl_storage 2, whose pass-by-pass f32 round trip (+16 n) is its definition; gl_storage 3 counts as the float chain of
 * gl_storage 0 (the texel rows between its two launches are not counted).  A chain that ends in gravity is
 * counted with its output copy (28 n) unless GLV_OP_OUTPUT_IS_STATE is in `ops` (20 n; a NULL d_out moves those 20 n too).
 * GLV_OP_WAVE: the input bytes the result depends on plus the output bytes, per stereo frame -- without GLV_OP_BARS the whole window (4 n for s16, 8 n
 * for f32) and 4 n texels or 8 n floats out; with GLV_OP_BARS the frames the bars sample (4 or 8 bytes x the sampled reach: the bins below the last tap of
 * any bar, in whole 64s -- 0.288 n with the shipped shape) and 4 or 8 bytes x bars out.  The texel rows between two launches are not counted. */
uint64_t glv_batch_algorithmic_bytes(const glv_batch* b, unsigned ops, int input_is_s16);

/* GLV_OP_BARS_ONLY batches: the bins of a row the chain keeps alive, [0, glv_batch_live_bins) (what the bars sample, in whole store
 * instructions); 0 for every other batch (all n bins live).  The kernels round it up to their last pass's block. */
uint32_t glv_batch_live_bins(const glv_batch* b);

/* Launch-geometry override for tuning: the workgroups of every persistent frame-kernel launch of this batch (process, ring-update and track
 * calls alike).  grid <= 0: automatic (the wisdom's grid, else one workgroup per group of rows until the chip is full).  Any positive grid is
 * valid: fewer workgroups make more trips each, a grid larger than the work leaves the surplus workgroups idle (they retire at their first
 * check).  The result does not depend on the grid, bit for bit -- output and state, every input kind, kernel class and configuration
 * (tests/test_forced_grid.py runs 1, 2 and 3 workgroups, and more than there is work, against the automatic grid and the oracle). */
int glv_batch_set_grid(glv_batch* b, int grid);
int glv_batch_last_grid(const glv_batch* b);      /* workgroups the last frame-kernel launch of this batch used */
int glv_batch_last_launches(const glv_batch* b);  /* kernels the last process / ring-update call of this batch launched (1 for every
                                                     FFT chain that runs fused; the ring copies of an update are not kernels) */
/* Kernel configurations of the batch's size: the library carries, per transform size, the configuration that won the
 * build-time sweeps (variant 0) and the runners-up that came close (a different radix split / points per lane, rows per
 * workgroup, placement of the window and twiddle tables); for s16 frame / ring input with log_mode 0 or 1 -- other
 * inputs have variant 0 only.  glv_batch_set_variant forces one (-1 = automatic: wisdom, else 0). */
int glv_batch_variants(const glv_batch* b);
int glv_batch_set_variant(glv_batch* b, int variant);
int glv_batch_last_variant(const glv_batch* b);   /* configuration the last frame-kernel launch of this batch used */
int glv_batch_describe_variant(const glv_batch* b, int variant, char* buf, size_t len);

/* Launch wisdom -- the role of glfft's FFTWisdom (glfft/glfft_wisdom.cpp:235-446: candidate work-group shapes and radix
 * splits of a transform are timed on the target and the winner remembered per transform description) for this path.
 * glv_batch_autotune times EVERY kernel configuration built for the batch's size on several workgroup counts each, on the
 * batch's device with the caller's buffers (real updates: a stateful batch is reset afterwards), and records the winning
 * (variant, workgroups) process-wide; every later launch with the same description -- device name + compute-unit count, n,
 * input kind, kernel class of `ops`, log_mode, avg_frames of an averaging chain, log2 of the stream count -- uses it.
 * Save / load carry the table across processes (a text file, one entry per line; entries of other devices are kept but
 * never match); the file named by the environment variable GLV_WISDOM is loaded when the first batch is created. */
int glv_batch_autotune(glv_batch* b, const int16_t* d_pcm, float* d_out, unsigned ops, void* hip_stream, int* best_grid, float* best_ms);
/* Placement wisdom (ABI 6).  A stateful chain (GLV_OP_GRAVITY / GLV_OP_AVERAGE) runs at one of two or three speeds, 7 - 14 % apart, decided by where its
 * state arrays lie in physical memory relative to the caller's OUTPUT buffer (profiles/r06/modes.txt: K batches of one process keep K speeds; one batch
 * changes speed with the output buffer; no allocator choice, TLB or clock effect).  This call times the batch's current placement with the caller's real
 * buffers and then up to `candidates` - 1 fresh allocations of the state arrays (all alive together while it runs: up to `candidates` x the state's size,
 * bounded by the free device memory), keeps the fastest, frees the rest and RESETS the state -- call it once, before the first real update, with the
 * buffers the updates will use.  *first_ms / *best_ms (may be NULL): ms per update of the placement the batch was created with / now has. */
int glv_batch_tune_placement(glv_batch* b, const int16_t* d_pcm, void* d_out, unsigned ops, int candidates, void* hip_stream, float* first_ms, float* best_ms);
int glv_wisdom_save(const char* path);
int glv_wisdom_load(const char* path);
int glv_wisdom_clear(void);
int glv_wisdom_count(void);

/* Self test of the s16 window product.  The reference multiplies a float sample by a double window value and rounds the
 * double product to float (render.c:794).  For s16 input the kernels compute the same bits without fp64: the window value
 * is a float pair (hi, lo) with fma(x, hi, x * lo) == (float) ((double) x * w) for every one of the 65536 sample values x =
 * k / 65535 -- found and checked on the device when the batch is created.  This call re-checks EVERY (sample value, window
 * position) pair of the batch's size against the fp64 product on the device: *mismatches (must be 0) and the number of
 * positions whose low part had to be moved off (float) (w - hi) (*shifted, may be NULL). */
int glv_batch_window_selftest(glv_batch* b, unsigned long long* mismatches, int* shifted);

/* Name of the kernel the last process call launched (for matching rocprofv3 rows). */
const char* glv_batch_kernel_name(const glv_batch* b);

/* Which arithmetic GLV_OP_BARS over TEXEL rows (gl_storage != 0) runs on this batch with its current parameters (ABI 6):
 *   GLV_BARS_NONE          the batch has no bar tables (bars == 0 / GLV_OP_BARS not announced)
 *   GLV_BARS_F32_CHAIN     fewer than 256 bars: smooth_audio()'s float chain per bar (the modules' bars; fused into the transform where it fits)
 *   GLV_BARS_I8_EXACT      256 bars or more, the documented form: exact integer weighted means on the i8 matrix cores (oracle glvo_bars_int_at)
 *   GLV_BARS_F32_MATRIX    256 bars or more where the integer tables could NOT be made -- a bar wider than the largest LDS ring (1600 bins: very
 *                          large smooth_factor, or n = 32768 with smooth_factor slightly above 0.025), 2^P scaling beyond 31 bits, a weight
 *                          >= 2^23 / a tile without steps, or GLV_NO_BARS_I8 in the environment at creation: one f32 fma chain per bar on
 *                          the f32 matrix cores (bit-equal to smooth_audio()'s float order, NOT to glvo_bars_int_at)
 *   GLV_BARS_F32_SEQ       (ABI 7) sample_mode maximum / hybrid: one lane per bar and row, the shader's loop in float as glv_params.sample_mode documents
 *                          (oracle glvo_bars_mode_at), float and texel rows alike
 * With bar texels set (glv_batch_set_bar_texels) it reports the twin's arithmetic: GLV_BARS_I8_EXACT or GLV_BARS_F32_SEQ.
 * Float rows (gl_storage 0) always take the float forms.  gl_storage 3 reports what GLV_OP_BARS runs over the upload's texels of its float rows: the same
 * values as 1 and 2 (GLV_BARS_F32_CHAIN and GLV_BARS_F32_MATRIX then name bars a GLV_OP_BARS call on such a batch refuses).  Callers and parity tests that
 * depend on the exact form check this. */
enum { GLV_BARS_NONE = 0, GLV_BARS_F32_CHAIN = 1, GLV_BARS_F32_MATRIX = 2, GLV_BARS_I8_EXACT = 3, GLV_BARS_F32_SEQ = 4 };
int glv_batch_bars_arithmetic(const glv_batch* b);

/* ------------------------------------------------------------------------------------
 * 3. Several GPUs of one node (BASELINE configs[3]).  No reference counterpart.
 *    Streams are independent: device g of G owns the contiguous shard [g*B/G, (g+1)*B/G) --
 *    its PCM, state and spectra live only there -- and there is no data-path collective.
 *    glv_multi_run_s16 drives every shard from its own host thread on its own HIP stream
 *    (the same timed-region contract as bench.py: warm-up, barrier + synchronize, `steps`
 *    updates, barrier + synchronize) and then performs the ONLY communication of the path:
 *    one ncclAllGather of a 32-byte stats record per rank and one ncclAllReduce(max) of the
 *    elapsed seconds, over RCCL (xGMI inside a node).  librccl is resolved with dlopen by
 *    glv_multi_create; hosts that never call glv_multi_* do not need it, and a host without it still runs
 *    (the 32-byte records are then collected on the host: glv_multi_uses_rccl).
 * ------------------------------------------------------------------------------------ */
typedef struct glv_multi glv_multi;
typedef struct glv_multi_stats {   /* what every rank contributes to the all-gather (32 bytes) */
    uint64_t frames;               /* stereo frames the rank processed in the timed region */
    double   seconds;              /* wall clock of the rank's timed region */
    uint64_t bytes;                /* algorithmic HBM bytes of those frames (glv_batch_algorithmic_bytes) */
    double   kernel_ms;            /* HIP-event time of the rank's launches */
} glv_multi_stats;

/* contiguous balanced partition: the first (total % world) ranks take one extra stream */
void glv_multi_shard_range(uint64_t total_streams, int rank, int world, uint64_t* first, uint64_t* count);
/* devices: `ndev` distinct device ordinals (NULL = 0 .. ndev-1) */
int glv_multi_create(const glv_params* p, uint64_t total_streams, unsigned ops_mask, const int* devices, int ndev, glv_multi** out);
int glv_multi_destroy(glv_multi* m);
int glv_multi_devices(const glv_multi* m);
/* 1: the stats record travels over RCCL; 0: librccl is not installed (or GLV_MULTI_RCCL=0) and the table is assembled on the
 * host -- the data path has no collective either way.  Only in the second mode may `devices` name a device more than once. */
int glv_multi_uses_rccl(const glv_multi* m);
/* shard idx: its device, first global stream, stream count and the glv_batch that owns its state (any may be NULL) */
int glv_multi_shard(const glv_multi* m, int idx, int* device, uint64_t* first_stream, uint32_t* streams, glv_batch** batch);
/* d_pcm[idx] / d_out[idx]: that shard's buffers on its own device (int16 [streams][n][2] / float [streams][2][n], or the
 * layout `ops` implies).  stats: [ndev] records as gathered (identical on every rank), max_seconds: the all-reduced
 * maximum of the ranks' elapsed seconds; either may be NULL. */
int glv_multi_run_s16(glv_multi* m, const int16_t* const* d_pcm, float* const* d_out, unsigned ops, int warmup, int steps,
                      glv_multi_stats* stats, double* max_seconds);

#ifdef __cplusplus
}
#endif
#endif /* GLV_SPECTRUM_H */
