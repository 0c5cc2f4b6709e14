// glv_api.cpp -- the C ABI of include/glv_spectrum.h on top of the gfx950 kernels: the entries that create, configure, reset and destroy a batch,
// the process and ring calls, bars, preludes, timing, diagnostics and the single-stream drop-ins.  The other host units (glv_host.h) carry them.
//
// Host-side responsibilities only: argument validation, constant tables (window, twiddles,
// frame weights -- glv_tables.h), device state (gravity buffers, history rings, PCM rings),
// launch geometry, HIP-event timing.  All arithmetic on samples happens in the kernels;
// there is no CPU compute path here and none is ever substituted.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <new>

#include "glv_host.h"
#include "glv_tables.h"       // the host-side table generators (make_*), kBarSeqMin

namespace glvh __attribute__((visibility("hidden"))) {
thread_local std::string g_err = "";
int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
}  // namespace glvh
namespace {
int validate(const glv_params* p) {
    if (!p) return fail(GLV_ERR_INVALID, "params is NULL");
    const int l = log2_exact(p->n);
    if (l < 8 || l > 15) return fail(GLV_ERR_INVALID, "n=%u: must be a power of two in [256, 32768]", p->n);
    if (p->channels != 1 && p->channels != 2) return fail(GLV_ERR_INVALID, "channels=%u: must be 1 or 2", p->channels);
    if (p->avg_frames < 1 || p->avg_frames > GLV_MAX_AVG_FRAMES)
        return fail(GLV_ERR_INVALID, "avg_frames=%u: must be in [1, %d]", p->avg_frames, GLV_MAX_AVG_FRAMES);
    if (p->avg_window_kind > 1) return fail(GLV_ERR_INVALID, "avg_window_kind=%u: must be 0 or 1", p->avg_window_kind);
    if (p->log_mode > 2) return fail(GLV_ERR_INVALID, "log_mode=%u: must be 0, 1 or 2", p->log_mode);
    if (p->gl_storage > 3)
        return fail(GLV_ERR_INVALID, "gl_storage=%u: must be 0, 1 (GL_R16 state, one launch), 2 (pass by pass, f32 state) or 3 (float state, bars sample the GL_R16 upload)", p->gl_storage);
    if (p->ur != p->ur) return fail(GLV_ERR_INVALID, "ur is NaN");   // 0 is legal: render.c:2387 yields it after an interval without updates
    if (p->round_formula > GLV_ROUND_LINEAR) return fail(GLV_ERR_INVALID, "round_formula=%u: 0 sinusoidal, 1 circular, 2 linear", p->round_formula);
    if (p->sample_mode > GLV_SAMPLE_HYBRID) return fail(GLV_ERR_INVALID, "sample_mode=%u: 0 average, 1 maximum, 2 hybrid", p->sample_mode);
    return GLV_OK;
}

int ensure_device(int device) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(GLV_ERR_NO_DEVICE, "no usable HIP device (%s); this library has no CPU path",
                    e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    if (device < 0 || device >= count) return fail(GLV_ERR_INVALID, "device %d out of range [0, %d)", device, count);
    HIP_TRY(hipSetDevice(device));
    return GLV_OK;
}

bool same_params(const glv_params& a, const glv_params& b) {
    return a.n == b.n && a.channels == b.channels && same_bits(a.fft_scale, b.fft_scale) && same_bits(a.fft_cutoff, b.fft_cutoff)
           && same_bits(a.gravity_step, b.gravity_step) && same_bits(a.ur, b.ur) && a.avg_frames == b.avg_frames && a.avg_window == b.avg_window
           && a.avg_window_kind == b.avg_window_kind && a.log_mode == b.log_mode && a.bars == b.bars && same_bits(a.smooth_factor, b.smooth_factor)
           && same_bits(a.smooth_distance, b.smooth_distance) && same_bits(a.smooth_ratio, b.smooth_ratio) && a.gl_storage == b.gl_storage
           && same_bits(a.bar_phase, b.bar_phase) && same_shape(a, b);
}

int batch_create_rows(const glv_params* p, uint32_t streams, unsigned ops_mask, int device, bool single_row, glv_batch** out) {
    if (!out) return fail(GLV_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (int rc = validate(p)) return rc;
    if (streams == 0) return fail(GLV_ERR_INVALID, "streams must be > 0");
    if (streams > (1u << 30)) return fail(GLV_ERR_INVALID, "streams=%u: at most 2^30 (row indices are 32-bit)", streams);
    if (int rc = ensure_device(device)) return rc;
    wisdom_load_env();
    glv_batch* b = new (std::nothrow) glv_batch();
    if (!b) return fail(GLV_ERR_NOMEM, "out of host memory");
    b->p = *p; b->streams = streams; b->ops_mask = ops_mask; b->device = device;
    b->rows = single_row ? 1u : streams * 2u; b->single_row = single_row;
    b->unfused_bars = std::getenv("GLV_UNFUSED_BARS") != nullptr;
    b->unfused_wave = std::getenv("GLV_UNFUSED_WAVE") != nullptr;
    if (const char* o = std::getenv("GLV_TRACK_WAVE_ORDER")) b->track_wave_by_steps = std::strcmp(o, "steps") == 0;
    if (const char* o = std::getenv("GLV_TRACK_FRAMES_SEGMENT")) b->track_frames_segment = (uint32_t) std::strtoul(o, nullptr, 10);
    b->bar_i8_off = std::getenv("GLV_NO_BARS_I8") != nullptr;
    b->log_nn = log2_exact(p->n) - 1;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) {
        b->num_cus = prop.multiProcessorCount;
        std::snprintf(b->device_name, sizeof(b->device_name), "%s", prop.gcnArchName[0] ? prop.gcnArchName : prop.name);
    }
    int rc = b->tab.create(p->n, device);
    if (rc == GLV_OK) rc = batch_alloc(b);
    // every table and buffer the announced operators need is made here, so that the stream-ordered calls never allocate or copy
    if (rc == GLV_OK) rc = batch_prepare(b);
    if (rc != GLV_OK) { glv_batch_destroy(b); return rc; }
    *out = b;
    return GLV_OK;
}

// ---- the single-stream drop-ins' two steps ----------------------------------------------------------
// Scalar knobs may change between calls, exactly like gl_data fields: what depends on them is regenerated when they do (compared
// field by field: padding bytes of a caller's struct mean nothing).  GLava's measured `ur` changes every frame (render.c:2387):
// that touches nothing but the gravity step -- no table, no launch plan.
int sync_params(glv_batch* b, const glv_params* p) {
    if (same_params(b->p, *p)) return GLV_OK;
    glv_params rest = *p;
    rest.ur = b->p.ur; rest.gravity_step = b->p.gravity_step;
    if (!same_params(b->p, rest)) return glv_batch_set_params(b, p);
    b->p.ur = p->ur; b->p.gravity_step = p->gravity_step;
    update_gravity_step(b);
    return GLV_OK;
}

// One update of the state's row from host memory and back: in_bytes of `in` through the staging, `ops`, out_bytes into `out` -- floats
// through the same staging, or GL_R16 texels (`texels`) through a staging of their own, made by the first call that asks for it.
// Mapped staging: memcpy in, one launch, one synchronisation, memcpy out.  Copy staging (GLV_STAGING=copy), and GLV_OP_SMOOTH under
// either (its row goes to the device buffer `seq`): two asynchronous copies around the launch.
int round_trip(glv_state* s, const void* in, size_t in_bytes, void* out, size_t out_bytes, unsigned ops, bool texels) {
    glv_batch* b = s->b;
    HIP_TRY(hipSetDevice(b->device));
    const bool via_seq = s->mapped && (ops & GLV_OP_SMOOTH);
    if (via_seq && !s->seq) HIP_TRY(s->seq.alloc(b->p.n, false));
    if (texels && !s->d_tex) {
        if (s->mapped) {
            HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&s->h_tex), out_bytes, hipHostMallocMapped));
            HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&s->d_tex), s->h_tex, 0));
        } else {
            HIP_TRY(s->tex_copy.alloc(b->p.n, false));
            s->d_tex = s->tex_copy;
        }
    }
    float* d_in = via_seq ? s->seq.get() : s->d_io;
    float* d_out = texels ? reinterpret_cast<float*>(s->d_tex) : d_in;
    if (s->mapped && !via_seq) {
        std::memcpy(s->h_io, in, in_bytes);
        const int rc = process(b, d_in, glv::IN_F32_PLANAR, d_out, ops, 1, 0, nullptr);
        HIP_TRY(hipStreamSynchronize(nullptr));        // also after a failed launch: nothing may still be reading h_io
        if (rc) return rc;
        std::memcpy(out, texels ? static_cast<const void*>(s->h_tex) : s->h_io, out_bytes);
        return GLV_OK;
    }
    HIP_TRY(hipMemcpyAsync(d_in, in, in_bytes, hipMemcpyHostToDevice, nullptr));
    if (int rc = process(b, d_in, glv::IN_F32_PLANAR, d_out, ops, 1, 0, nullptr)) return rc;
    HIP_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, nullptr));
    HIP_TRY(hipStreamSynchronize(nullptr));
    return GLV_OK;
}
}  // namespace

// =====================================================================================================
extern "C" {
void glv_params_default(glv_params* p) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->n = 4096;                 // shaders/glava/rc.glsl:190
    p->channels = 2;
    p->fft_scale = 10.2F;        // smooth_parameters.glsl:46 / render.c:930
    p->fft_cutoff = 0.3F;        // smooth_parameters.glsl:51 / render.c:931
    p->gravity_step = 4.2F;      // smooth_parameters.glsl:67 / render.c:911
    p->ur = 22050.0F / 256.0F;   // rate / (samplesize/4), rc.glsl:181,203; formula render.c:1674
    p->avg_frames = 5;           // smooth_parameters.glsl:56
    p->avg_window = 1;           // smooth_parameters.glsl:61
    p->avg_window_kind = 0;
    p->log_mode = 1;             // hardware log2: <= 1.8e-7 relative on every float (bar 1e-5); 0 = bit-faithful fp64
    p->bars = 80;                // radial.glsl:9 (NBARS 160, two channels)
    p->smooth_factor = 0.025F;   // smooth_parameters.glsl:72
    p->smooth_distance = 0.01F;  // render.c:917
    p->smooth_ratio = 4.0F;      // render.c:918
    p->gl_storage = 0;
    p->bar_phase = 0.0F;
}

// shared with glv_multi.cpp: record an error string for the calling thread
int glv_set_last_error(int code, const char* msg) { g_err = msg ? msg : ""; return code; }
int glv_abi_version(void) { return GLV_ABI_VERSION; }
const char* glv_last_error(void) { return g_err.c_str(); }
int glv_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count;
}

// ---- batched -----------------------------------------------------------------------------------------
int glv_batch_create(const glv_params* p, uint32_t streams, unsigned ops_mask, int device, glv_batch** out) {
    return batch_create_rows(p, streams, ops_mask, device, false, out);
}

int glv_batch_set_params(glv_batch* b, const glv_params* p) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (int rc = validate(p)) return rc;
    if (p->n != b->p.n || p->avg_frames != b->p.avg_frames)
        return fail(GLV_ERR_STATE, "params (n=%u, F=%u) do not match the batch (n=%u, F=%u): fixed at creation", p->n, p->avg_frames, b->p.n, b->p.avg_frames);
    if ((p->gl_storage == 1) != b->state16)
        return fail(GLV_ERR_STATE, "gl_storage=%u: the state of this batch was created as %s", p->gl_storage, b->state16 ? "GL_R16 texels (gl_storage 1)" : "floats (gl_storage 0 / 2 / 3)");
    if (b->snapped() && (p->bars != b->p.bars || p->gl_storage == 0))
        return fail(GLV_ERR_STATE, "bar texels are set (glv_batch_set_bar_texels): bars (%u -> %u) must keep the table's length and gl_storage must stay non-zero "
                                   "(a float chain has no pre-smoothed texture); clear the table first", b->p.bars, p->bars);
    HIP_TRY(hipSetDevice(b->device));
    // the tables are rewritten in place: every kernel already queued on any stream of the device must have read them first (a
    // blocking copy from pageable memory does not order against a caller's non-blocking stream)
    HIP_TRY(hipDeviceSynchronize());
    const glv_params old = b->p;
    b->p = *p;
    int rc = batch_prepare(b);
    // a GLV_OP_BARS_ONLY batch that has run its live class keeps no state beyond the bins its live calls kept (glv_batch::kept_live): parameters under which
    // the bars sample further (or that take the live class away: log_mode 2) would read state that was never maintained -- refused until the state is reset
    if (rc == GLV_OK && !b->keeps_live(b->live_bins()))
        rc = fail(GLV_ERR_STATE, "this GLV_OP_BARS_ONLY batch has run its live kernel class: the state beyond bin %u was not kept, and these parameters "
                                 "(smooth_factor=%g bars=%u log_mode=%u sample_scale=%g sample_range=%g) sample %s -- glv_batch_reset first, or a new batch", b->kept_live,
                  (double) p->smooth_factor, p->bars, p->log_mode, (double) p->sample_scale, (double) p->sample_range, b->live_bins() == 0 ? "every bin (the full chain)" : "beyond it");
    if (rc != GLV_OK) { const std::string said = g_err; b->p = old; (void) batch_prepare(b); g_err = said; }   // a rejected change leaves the batch as it was
    for (auto& row : b->plan_cache) for (auto& pc : row) pc.gen = 0;        // log_mode is part of the wisdom key
    return rc;
}

int glv_batch_reset(glv_batch* b) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    HIP_TRY(hipSetDevice(b->device));
    const size_t n = b->p.n;
    if (b->d_hist) HIP_TRY(hipMemset(b->d_hist, 0, b->hist_bytes()));
    if (b->d_grav) HIP_TRY(hipMemset(b->d_grav, 0, b->grav_bytes()));
    if (b->d_ring) HIP_TRY(hipMemset(b->d_ring, 0, sizeof(int16_t) * 2 * n * b->streams));
    if (b->d_ring_f32) HIP_TRY(hipMemset(b->d_ring_f32, 0, sizeof(float) * 2 * n * b->streams));
    b->ring_pos = 0; b->ring_pos_f32 = 0; b->rewind_state();
    return GLV_OK;
}

int glv_batch_destroy(glv_batch* b) {
    if (!b) return GLV_OK;
    (void) hipSetDevice(b->device);
    b->tab.destroy();
    state_free(b->d_grav);
    state_free(b->d_hist);
    for (hipEvent_t e : b->ev) (void) hipEventDestroy(e);
    delete b;                    // every table and ring frees itself (DeviceArray)
    return GLV_OK;
}

int glv_batch_process_s16(glv_batch* b, const int16_t* d_pcm, float* d_out, unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!(ops & (GLV_OP_FFT | GLV_OP_WAVE))) return fail(GLV_ERR_INVALID, "s16 input requires GLV_OP_FFT or GLV_OP_WAVE");
    return process_windows(b, d_pcm, glv::IN_S16_STEREO, glv::DEC_S16, d_out, ops, (hipStream_t) hip_stream);
}

int glv_batch_process_f32(glv_batch* b, const float* d_f32, float* d_out, unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    return process_windows(b, d_f32, glv::IN_F32_PLANAR, glv::DEC_F32_PLANAR, d_out, ops, (hipStream_t) hip_stream);
}

int glv_batch_process_f32_stereo(glv_batch* b, const float* d_pcm, float* d_out, unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!(ops & (GLV_OP_FFT | GLV_OP_WAVE))) return fail(GLV_ERR_INVALID, "interleaved input requires GLV_OP_FFT or GLV_OP_WAVE");
    return process_windows(b, d_pcm, glv::IN_F32_STEREO, glv::DEC_F32, d_out, ops, (hipStream_t) hip_stream);
}

// append `new_frames` frames of `fb` bytes each per stream at ring position `pos` (frames) of rings with a pitch of n frames:
// one strided copy, or two when the append wraps (any new_frames <= n: fifo.c:38,81,91 accept any sample_sz)
static int ring_append(char* d_ring, const char* d_new, uint32_t pos, uint32_t new_frames, uint32_t n, size_t fb, uint32_t streams, hipStream_t st) {
    const size_t pitch = (size_t) n * fb, width = (size_t) new_frames * fb;
    const uint32_t first = new_frames <= n - pos ? new_frames : n - pos;       // frames that fit before the wrap
    for (int part = 0; part < 2; ++part) {
        const uint32_t cnt = part == 0 ? first : new_frames - first;
        if (cnt == 0) continue;
        char* dst = d_ring + (size_t) (part == 0 ? pos : 0) * fb;
        const size_t w = (size_t) cnt * fb;
        if (d_new) HIP_TRY(hipMemcpy2DAsync(dst, pitch, d_new + (size_t) (part == 0 ? 0 : first) * fb, width, w, streams, hipMemcpyDeviceToDevice, st));
        else       HIP_TRY(hipMemset2DAsync(dst, pitch, 0, w, streams, st));   // fifo.c:67-79
    }
    return GLV_OK;
}

// the append half of a ring update: copy / zero-fill the new frames at the write position of the ring glv_batch_create
// allocated (GLV_OP_RING_S16 / _F32) and advance it.  *old_pos receives the position before the append.  streams: the rings [0, streams) receive frames
// (the batch's, or the prefix of a glv_batch_ring_update_first_* call).
static int ring_push(glv_batch* b, bool f32, const void* d_new, uint32_t new_frames, hipStream_t st, uint32_t* old_pos, uint32_t streams) {
    const uint32_t n = b->p.n;
    if (int rc = refuse_bufscale(b, f32 ? "the f32 ring entries" : "the s16 ring entries")) return rc;
    if (new_frames == 0 || new_frames > n)
        return fail(GLV_ERR_INVALID, "new_frames=%u: must be in [1, n=%u] (sample_sz/4 of %s)", new_frames, n, f32 ? "pulse_input.c:155-178" : "fifo.c:38,91");
    const size_t fb = f32 ? 8 : 4;
    char* ring = f32 ? reinterpret_cast<char*>(b->d_ring_f32.get()) : reinterpret_cast<char*>(b->d_ring.get());
    uint32_t* pos = f32 ? &b->ring_pos_f32 : &b->ring_pos;
    if (!ring)
        return fail(GLV_ERR_STATE, "the batch was created without GLV_OP_RING_%s in its ops_mask (rings are allocated at creation, ring updates never allocate)", f32 ? "F32" : "S16");
    if (int rc = ring_append(ring, static_cast<const char*>(d_new), *pos, new_frames, n, fb, streams, st)) return rc;
    *old_pos = *pos;
    *pos = (*pos + new_frames) % n;                              // the oldest frame now sits here: the window starts there
    return GLV_OK;
}

int glv_batch_ring_update_s16(glv_batch* b, const int16_t* d_new, uint32_t new_frames, float* d_out, unsigned ops,
                              void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!(ops & (GLV_OP_FFT | GLV_OP_WAVE))) return fail(GLV_ERR_INVALID, "ring mode requires GLV_OP_FFT or GLV_OP_WAVE (glv_batch_ring_append_s16 appends without transforming)");
    hipStream_t st = (hipStream_t) hip_stream;
    HIP_TRY(hipSetDevice(b->device));
    if (int rc = check_ops(b, ops, d_out)) return rc;            // nothing is appended when the call cannot be processed
    uint32_t old_pos = 0;
    if (int rc = ring_push(b, false, d_new, new_frames, st, &old_pos, b->streams)) return rc;
    const int rc = process(b, b->d_ring, glv::IN_S16_RING, d_out, ops, b->streams * 2, b->ring_pos, st);
    if (rc != GLV_OK) b->ring_pos = old_pos;                      // a failed launch leaves the ring where the caller saw it
    return rc;
}

int glv_batch_ring_update_f32(glv_batch* b, const float* d_new, uint32_t new_frames, float* d_out, unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!(ops & (GLV_OP_FFT | GLV_OP_WAVE))) return fail(GLV_ERR_INVALID, "ring mode requires GLV_OP_FFT or GLV_OP_WAVE (glv_batch_ring_append_f32 appends without transforming)");
    if (!d_new) return fail(GLV_ERR_INVALID, "d_new is NULL (the PulseAudio backend has no zero-fill path)");
    hipStream_t st = (hipStream_t) hip_stream;
    HIP_TRY(hipSetDevice(b->device));
    if (int rc = check_ops(b, ops, d_out)) return rc;
    uint32_t old_pos = 0;
    if (int rc = ring_push(b, true, d_new, new_frames, st, &old_pos, b->streams)) return rc;
    const int rc = process(b, b->d_ring_f32, glv::IN_F32_RING, d_out, ops, b->streams * 2, b->ring_pos_f32, st);
    if (rc != GLV_OK) b->ring_pos_f32 = old_pos;
    return rc;
}

// Elastic batches (include/glv_spectrum.h): the process and ring-update calls on streams [0, count) of the batch -- the un-suffixed call with 2 * count channel rows
// and count rings, refused in its words; the batch's positions advance as for a full call.
int glv_batch_process_first_s16(glv_batch* b, uint32_t count, const int16_t* d_pcm, float* d_out, unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (int rc = refuse_prefix(b, "glv_batch_process_first_s16", count)) return rc;
    if (!(ops & (GLV_OP_FFT | GLV_OP_WAVE))) return fail(GLV_ERR_INVALID, "s16 input requires GLV_OP_FFT or GLV_OP_WAVE");
    return process_first(b, count, d_pcm, glv::IN_S16_STEREO, glv::DEC_S16, d_out, ops, (hipStream_t) hip_stream);
}

int glv_batch_process_first_f32(glv_batch* b, uint32_t count, const float* d_f32, float* d_out, unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (int rc = refuse_prefix(b, "glv_batch_process_first_f32", count)) return rc;
    return process_first(b, count, d_f32, glv::IN_F32_PLANAR, glv::DEC_F32_PLANAR, d_out, ops, (hipStream_t) hip_stream);
}

int glv_batch_process_first_f32_stereo(glv_batch* b, uint32_t count, const float* d_pcm, float* d_out, unsigned ops, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (int rc = refuse_prefix(b, "glv_batch_process_first_f32_stereo", count)) return rc;
    if (!(ops & (GLV_OP_FFT | GLV_OP_WAVE))) return fail(GLV_ERR_INVALID, "interleaved input requires GLV_OP_FFT or GLV_OP_WAVE");
    return process_first(b, count, d_pcm, glv::IN_F32_STEREO, glv::DEC_F32, d_out, ops, (hipStream_t) hip_stream);
}

// both ring entries' prefix form: glv_batch_ring_update_s16 / _f32 with `count` in the place of the batch's streams
static int ring_update_first(glv_batch* b, bool f32, uint32_t count, const void* d_new, uint32_t new_frames, float* d_out, unsigned ops, hipStream_t st) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (int rc = refuse_prefix(b, f32 ? "glv_batch_ring_update_first_f32" : "glv_batch_ring_update_first_s16", count)) return rc;
    if (!(ops & (GLV_OP_FFT | GLV_OP_WAVE)))
        return fail(GLV_ERR_INVALID, "ring mode requires GLV_OP_FFT or GLV_OP_WAVE (glv_batch_ring_append_%s appends without transforming)", f32 ? "f32" : "s16");
    if (f32 && !d_new) return fail(GLV_ERR_INVALID, "d_new is NULL (the PulseAudio backend has no zero-fill path)");
    HIP_TRY(hipSetDevice(b->device));
    if (int rc = check_ops(b, ops, d_out)) return rc;            // nothing is appended when the call cannot be processed
    uint32_t old_pos = 0;
    if (int rc = ring_push(b, f32, d_new, new_frames, st, &old_pos, count)) return rc;
    uint32_t* const pos = f32 ? &b->ring_pos_f32 : &b->ring_pos;
    const void* const ring = f32 ? static_cast<const void*>(b->d_ring_f32.get()) : static_cast<const void*>(b->d_ring.get());
    const int rc = process(b, ring, f32 ? glv::IN_F32_RING : glv::IN_S16_RING, d_out, ops, 2 * count, *pos, st);
    if (rc != GLV_OK) *pos = old_pos;                            // a failed launch leaves the ring where the caller saw it
    return rc;
}

int glv_batch_ring_update_first_s16(glv_batch* b, uint32_t count, const int16_t* d_new, uint32_t new_frames, float* d_out, unsigned ops, void* hip_stream) {
    return ring_update_first(b, false, count, d_new, new_frames, d_out, ops, (hipStream_t) hip_stream);
}

int glv_batch_ring_update_first_f32(glv_batch* b, uint32_t count, const float* d_new, uint32_t new_frames, float* d_out, unsigned ops, void* hip_stream) {
    return ring_update_first(b, true, count, d_new, new_frames, d_out, ops, (hipStream_t) hip_stream);
}

int glv_batch_ring_append_s16(glv_batch* b, const int16_t* d_new, uint32_t new_frames, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    HIP_TRY(hipSetDevice(b->device));
    uint32_t old_pos = 0;
    return ring_push(b, false, d_new, new_frames, (hipStream_t) hip_stream, &old_pos, b->streams);
}

int glv_batch_ring_append_f32(glv_batch* b, const float* d_new, uint32_t new_frames, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!d_new) return fail(GLV_ERR_INVALID, "d_new is NULL (the PulseAudio backend has no zero-fill path)");
    HIP_TRY(hipSetDevice(b->device));
    uint32_t old_pos = 0;
    return ring_push(b, true, d_new, new_frames, (hipStream_t) hip_stream, &old_pos, b->streams);
}

int glv_batch_ring_planar(glv_batch* b, int f32_ring, float* d_planar, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!d_planar) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (int rc = refuse_bufscale(b, "glv_batch_ring_planar")) return rc;
    const void* ring = f32_ring ? static_cast<const void*>(b->d_ring_f32.get()) : static_cast<const void*>(b->d_ring.get());
    if (!ring) return fail(GLV_ERR_STATE, "the batch has no %s ring yet (create it with GLV_OP_RING_%s or append to it first)", f32_ring ? "f32" : "s16", f32_ring ? "F32" : "S16");
    HIP_TRY(hipSetDevice(b->device));
    hipError_t e = glv::launch_ring_planar(ring, f32_ring ? 1 : 0, b->p.n, f32_ring ? b->ring_pos_f32 : b->ring_pos, b->p.channels == 1, b->streams,
                                           d_planar, (hipStream_t) hip_stream);
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "ring snapshot launch failed: %s", hipGetErrorString(e));
    return GLV_OK;
}

int glv_batch_gravity_state(glv_batch* b, const float** d_state) {
    if (!b || !d_state) return fail(GLV_ERR_INVALID, "NULL argument");
    if (!b->d_grav) return fail(GLV_ERR_STATE, "the batch was created without GLV_OP_GRAVITY");
    if (b->grav_mode == 2)
        return fail(GLV_ERR_STATE, "gravity runs fused with average on this batch: its state is the newest slot of the history ring "
                                   "(float [rows][F][n], not a [streams][2][n] array); request the chain's output instead");
    if (b->state16) return fail(GLV_ERR_STATE, "gl_storage 1 keeps the gravity store as uint16 texels, not floats: request the chain's output instead");
    if (b->ops_mask & GLV_OP_BARS_ONLY) return fail(GLV_ERR_STATE, "the batch was created with GLV_OP_BARS_ONLY: its gravity state exists only where the bars sample");
    *d_state = b->grav_cur;
    return GLV_OK;
}

int glv_batch_bars(glv_batch* b, const float* d_spec, float* d_bars, void* hip_stream) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!d_spec || !d_bars) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (b->p.bars == 0 || b->p.bars > b->p.n) return fail(GLV_ERR_INVALID, "bars=%u out of range", b->p.bars);
    HIP_TRY(hipSetDevice(b->device));
    if (!b->bar.desc) return fail(GLV_ERR_STATE, "the batch has no bar tables (bars / smooth_factor / bar_phase were unusable when it was created)");
    if (b->snapped()) return fail(GLV_ERR_STATE, "glv_batch_bars takes float spectra, not a GL chain's texels: refused while bar texels or column texels are set (glv_batch_set_bar_texels / glv_batch_set_column_texels)");
    if (upload_storage(b->p)) return fail(GLV_ERR_STATE, "glv_batch_bars takes float spectra: on gl_storage 3 GLV_OP_BARS samples the upload's texels (caller's float rows: a gl_storage 0 batch)");
    const glv::BarRowsTables rt = rows_tables(b->p, b->bar_x, b->bar);
    hipError_t e = glv::launch_bars(d_spec, d_bars, (size_t) b->streams * 2, b->p.n, b->p.bars, b->bar_x.nsteps, b->bar_x.items, b->bar.desc, b->bar.w,
                                    (hipStream_t) hip_stream, false, &rt);
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "bars launch failed: %s", hipGetErrorString(e));
    return GLV_OK;
}

int glv_prelude_bufscale(int device, const float* d_in, float* d_out, size_t rows, uint32_t n_out, uint32_t k, void* hip_stream) {
    if (!d_in || !d_out) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (k == 0 || n_out == 0) return fail(GLV_ERR_INVALID, "bufscale k and n_out must be > 0");
    if (int rc = ensure_device(device)) return rc;
    hipError_t e = glv::launch_bufscale(d_in, d_out, rows * n_out, k, (hipStream_t) hip_stream);
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "bufscale launch failed: %s", hipGetErrorString(e));
    return GLV_OK;
}

int glv_prelude_lerp(int device, const float* d_start, const float* d_end, float* d_out, size_t count, float uratio,
                     int kcounter, void* hip_stream) {
    if (!d_start || !d_end || !d_out) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (int rc = ensure_device(device)) return rc;
    float mod = uratio * (float) kcounter;               // render.c:1804-1805
    if (mod > 1.0F) mod = 1.0F;
    hipError_t e = glv::launch_lerp(d_start, d_end, d_out, count, mod, (hipStream_t) hip_stream);
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "lerp launch failed: %s", hipGetErrorString(e));
    return GLV_OK;
}

int glv_batch_timing_begin(glv_batch* b) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    b->timing = true; b->ev_used = 0; b->launches = 0;
    return GLV_OK;
}

int glv_batch_timing_end(glv_batch* b, double* kernel_ms, uint64_t* launches) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    double total = 0.0;
    for (size_t i = 0; i + 1 < b->ev_used; i += 2) {
        HIP_TRY(hipEventSynchronize(b->ev[i + 1]));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, b->ev[i], b->ev[i + 1]));
        total += ms;
    }
    if (kernel_ms) *kernel_ms = total;
    if (launches) *launches = b->launches;
    b->timing = false;
    return GLV_OK;
}

uint64_t glv_batch_algorithmic_bytes(const glv_batch* b, unsigned ops, int input_is_s16) {
    if (!b) return 0;
    // SURVEY.md 8d, per stereo frame with N real samples per channel, F = avg_frames:
    //   in: 4N (s16 x 2ch) or 8N (f32 x 2ch);  out: 8N (f32), 4N (GLV_OP_R16 texels), 8 * bars (GLV_OP_BARS; 4 * bars as texels)
    //   + gravity (no average): read the state 8N, write it 8N -- and the output besides, unless the output IS the state
    //     (GLV_OP_OUTPUT_IS_STATE, or d_out == NULL: SURVEY 8d row B's 20N) or only bars leave the chip
    //   + average: read (F-1) ring slots 8N each, write the newest slot 8N (doubles as gravity state)
    //   gl_storage 1 (GL_R16 state): every state value is a 16-bit texel -- 4N per slot instead of 8N: with F = 5 and texels out
    //     4N + 16N + 4N + 4N = 28N
    //   gl_storage 2 (pass by pass): the transform's f32 spectra are written and read back by the gravity / average pass (+16N)
    const uint64_t N = b->p.n, F = b->p.avg_frames;
    if (ops & GLV_OP_WAVE) {
        // GLV_OP_WAVE: the input bytes the result depends on + the output bytes.  Without bars every frame of the window (4N / 8N) and 4N texels or 8N
        // floats; with bars the frames below the last tap of any bar, in whole 64s (the reach the bars kernels are handed: 0.288 N as shipped), and the
        // bars.  The texel rows between the two launches of the unfused forms are traffic of the organisation and are not counted.
        const uint64_t in_b = input_is_s16 ? 4 : 8, out_b = (ops & GLV_OP_R16) ? 4 : 8;
        if (!(ops & GLV_OP_BARS)) return (in_b * N + out_b * N) * b->streams;
        uint64_t reach = b->snapped() ? b->snap.bins : b->bar.bins;
        if (reach == 0 || reach > N) reach = N;
        return (in_b * reach + out_b * b->p.bars) * b->streams;
    }
    const bool stateful = (ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE)) != 0;
    //   GLV_OP_BARS_ONLY: state traffic is counted for the live bins L only -- the bins the bars sample, NOT the (larger) share of the row the kernel
    //   class keeps (FrameGeometry::live_points: an implementation granularity, its extra bytes are traffic above the algorithmic figure)
    uint64_t L = N;
    if (b->live_bins() != 0 && stateful && (ops & GLV_OP_BARS)) L = b->live_bins();
    const uint64_t sv = (b->state16 && stateful) ? 4 * L : 8 * L;          // one state slot of both channels
    uint64_t per = input_is_s16 ? 4 * N : 8 * N;
    const bool bars = (ops & GLV_OP_BARS) != 0;
    if (bars) per += (uint64_t) ((ops & GLV_OP_R16) ? 4 : 8) * b->p.bars;
    else if (!((ops & GLV_OP_OUTPUT_IS_STATE) && !(ops & GLV_OP_AVERAGE))) per += (ops & GLV_OP_R16) ? 4 * N : 8 * N;
    if (ops & GLV_OP_AVERAGE) per += sv * (F - 1) + sv;
    else if (ops & GLV_OP_GRAVITY) per += 2 * sv;
    if (b->p.gl_storage == 2 && (ops & GLV_OP_FFT) && stateful) per += 16 * N;
    return per * b->streams;
}

uint32_t glv_batch_live_bins(const glv_batch* b) { return b ? b->live_bins() : 0u; }

const char* glv_batch_kernel_name(const glv_batch* b) { return b ? b->kernel_name : ""; }

int glv_batch_bars_arithmetic(const glv_batch* b) {
    if (!b || b->bar_x.count == 0 || !b->bar.desc) return GLV_BARS_NONE;
    if (b->snapped()) return b->p.sample_mode != GLV_SAMPLE_AVERAGE ? GLV_BARS_F32_SEQ : GLV_BARS_I8_EXACT;   // the twin's (set_bar_texels made sure)
    if (b->p.sample_mode != GLV_SAMPLE_AVERAGE) return GLV_BARS_F32_SEQ;
    if (b->p.bars < glv::kBarSeqMin) return GLV_BARS_F32_CHAIN;
    return b->p.gl_storage != 0 && b->bar_x.i8() ? GLV_BARS_I8_EXACT : GLV_BARS_F32_MATRIX;
}

int glv_batch_last_grid(const glv_batch* b) { return b ? b->last_grid : 0; }
int glv_batch_last_launches(const glv_batch* b) { return b ? b->last_launches : 0; }

// ---- single-stream drop-ins -------------------------------------------------------------------------
int glv_state_create(const glv_params* p, int device, glv_state** out) {
    if (!out) return fail(GLV_ERR_INVALID, "out is NULL");
    *out = nullptr;
    glv_state* s = new (std::nothrow) glv_state();
    if (!s) return fail(GLV_ERR_NOMEM, "out of host memory");
    // (GL_R16 state -- the accel path of handle_audio, glv_gl_texture -- also announces the pre-smoothing pass: one scratch row)
    const unsigned mask = GLV_OP_GRAVITY | GLV_OP_AVERAGE | GLV_OP_SMOOTH | GLV_OP_WAVE | (p && (p->gl_storage == 1 || p->gl_storage == 3) && p->bars >= 1 && p->bars <= p->n ? (unsigned) GLV_OP_BARS : 0u);
    int rc = batch_create_rows(p, 1, mask, device, true, &s->b);
    if (rc == GLV_OK) {
        const char* mode = std::getenv("GLV_STAGING");
        s->mapped = !(mode && std::strcmp(mode, "copy") == 0);
        hipError_t e;
        if (s->mapped) {
            e = hipHostMalloc(reinterpret_cast<void**>(&s->h_io), sizeof(float) * p->n, hipHostMallocMapped);
            if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void**>(&s->d_io), s->h_io, 0);
        } else {
            e = hipMalloc(&s->d_io, sizeof(float) * p->n);
        }
        if (e != hipSuccess) rc = fail(GLV_ERR_HIP, "staging allocation failed: %s", hipGetErrorString(e));
    }
    if (rc != GLV_OK) { glv_state_destroy(s); return rc; }
    *out = s;
    return GLV_OK;
}

int glv_state_reset(glv_state* s) {
    if (!s || !s->b) return fail(GLV_ERR_INVALID, "state is NULL");
    return glv_batch_reset(s->b);      // one row, no rings: the same two memsets; the positions and flags it clears besides are never set on such a batch
}

int glv_state_destroy(glv_state* s) {
    if (!s) return GLV_OK;
    if (s->b) { (void) hipSetDevice(s->b->device); glv_batch_destroy(s->b); }
    if (s->mapped) {
        if (s->h_io) (void) hipHostFree(s->h_io);
        if (s->h_tex) (void) hipHostFree(s->h_tex);
    } else if (s->d_io) (void) hipFree(s->d_io);
    delete s;
    return GLV_OK;
}

static int single(const glv_params* p, glv_state* s, float* buf, unsigned ops) {
    if (!s || !s->b) return fail(GLV_ERR_INVALID, "state is NULL");
    if (!buf) return fail(GLV_ERR_INVALID, "buf is NULL");
    if (int rc = validate(p)) return rc;
    glv_batch* b = s->b;
    if (p->n != b->p.n || p->avg_frames != b->p.avg_frames)
        return fail(GLV_ERR_STATE, "params (n=%u, F=%u) do not match the state (n=%u, F=%u)", p->n, p->avg_frames, b->p.n, b->p.avg_frames);
    if (int rc = sync_params(b, p)) return rc;
    return round_trip(s, buf, sizeof(float) * p->n, buf, sizeof(float) * p->n, ops, false);
}

int glv_fft(const glv_params* p, glv_state* s, float* buf) { return single(p, s, buf, GLV_OP_FFT); }
int glv_gravity(const glv_params* p, glv_state* s, float* buf) { return single(p, s, buf, GLV_OP_GRAVITY); }
int glv_average(const glv_params* p, glv_state* s, float* buf) { return single(p, s, buf, GLV_OP_AVERAGE); }
int glv_wrange(const glv_params* p, glv_state* s, float* buf) { return single(p, s, buf, GLV_OP_WRANGE); }
int glv_smooth(const glv_params* p, glv_state* s, float* buf) { return single(p, s, buf, GLV_OP_SMOOTH); }
int glv_magnitude(const glv_params* p, glv_state* s, float* buf) { return single(p, s, buf, GLV_OP_MAGNITUDE); }
int glv_fft_gravity_average(const glv_params* p, glv_state* s, float* buf) {
    return single(p, s, buf, GLV_OP_FFT | GLV_OP_GRAVITY | GLV_OP_AVERAGE);
}
int glv_texels_r16(const glv_params* p, glv_state* s, const float* buf, uint16_t* texels) {
    if (!s || !s->b) return fail(GLV_ERR_INVALID, "state is NULL");
    if (!buf || !texels) return fail(GLV_ERR_INVALID, "NULL buffer");
    if (int rc = validate(p)) return rc;
    if (p->n != s->b->p.n) return fail(GLV_ERR_STATE, "params n=%u does not match the state (n=%u)", p->n, s->b->p.n);
    // (the conversion reads no knob: the state's parameters stay as they are)
    return round_trip(s, buf, sizeof(float) * p->n, texels, sizeof(uint16_t) * p->n, GLV_OP_R16, true);
}

int glv_gl_texture(const glv_params* p, glv_state* s, const float* buf, int smooth_pass, uint16_t* texels) {
    if (!s || !s->b) return fail(GLV_ERR_INVALID, "state is NULL");
    if (!buf || !texels) return fail(GLV_ERR_INVALID, "NULL buffer");
    if (int rc = validate(p)) return rc;
    glv_batch* b = s->b;
    if (p->n != b->p.n || p->avg_frames != b->p.avg_frames)
        return fail(GLV_ERR_STATE, "params (n=%u, F=%u) do not match the state (n=%u, F=%u)", p->n, p->avg_frames, b->p.n, b->p.avg_frames);
    if (p->gl_storage != 1 || !b->state16) return fail(GLV_ERR_STATE, "glv_gl_texture needs a state created with gl_storage = 1 (the GL passes' GL_R16 storage)");
    if (smooth_pass && (p->bars != p->n || !(b->ops_mask & GLV_OP_BARS)))
        return fail(GLV_ERR_INVALID, "glv_gl_texture with the pre-smoothing pass: bars must equal n (bar_phase 0.5: the pass's texel centres) when the state is created");
    if (int rc = sync_params(b, p)) return rc;
    // render.c:2230: no averaging pass with a single frame; the chain then ends in the gravity store
    const unsigned ops = GLV_OP_FFT | GLV_OP_GRAVITY | (p->avg_frames > 1 ? (unsigned) GLV_OP_AVERAGE : 0u) | (smooth_pass ? (unsigned) GLV_OP_BARS : 0u) | GLV_OP_R16;
    return round_trip(s, buf, sizeof(float) * p->n, texels, sizeof(uint16_t) * p->n, ops, true);
}

int glv_wave_texture(const glv_params* p, glv_state* s, const float* buf, int smooth_pass, uint16_t* texels) {
    if (!s || !s->b) return fail(GLV_ERR_INVALID, "state is NULL");
    if (!buf || !texels) return fail(GLV_ERR_INVALID, "NULL buffer");
    if (int rc = validate(p)) return rc;
    glv_batch* b = s->b;
    if (p->n != b->p.n || p->avg_frames != b->p.avg_frames)
        return fail(GLV_ERR_STATE, "params (n=%u, F=%u) do not match the state (n=%u, F=%u)", p->n, p->avg_frames, b->p.n, b->p.avg_frames);
    if (smooth_pass && (!(p->gl_storage == 1 ? b->state16 : p->gl_storage == 3 && !b->state16) || !(b->ops_mask & GLV_OP_BARS)))
        return fail(GLV_ERR_STATE, "glv_wave_texture with the pre-smoothing pass needs a state created with gl_storage = 1 (or 3) and bars = n (the pass samples GL_R16 texels)");
    if (smooth_pass && p->bars != p->n)
        return fail(GLV_ERR_INVALID, "glv_wave_texture with the pre-smoothing pass: bars must equal n (bar_phase 0.5: the pass's texel centres)");
    if (int rc = sync_params(b, p)) return rc;
    const unsigned ops = GLV_OP_WAVE | (smooth_pass ? (unsigned) GLV_OP_BARS : 0u) | GLV_OP_R16;
    return round_trip(s, buf, sizeof(float) * p->n, texels, sizeof(uint16_t) * p->n, ops, true);
}

int glv_device_malloc(int device, size_t bytes, void** d_ptr) {
    if (!d_ptr) return fail(GLV_ERR_INVALID, "d_ptr is NULL");
    *d_ptr = nullptr;
    if (int rc = ensure_device(device)) return rc;
    if (hipMalloc(d_ptr, bytes ? bytes : 1) != hipSuccess) return fail(GLV_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
    return GLV_OK;
}
int glv_device_free(int device, void* d_ptr) {
    if (!d_ptr) return GLV_OK;
    if (int rc = ensure_device(device)) return rc;
    HIP_TRY(hipFree(d_ptr));
    return GLV_OK;
}
int glv_device_upload(int device, void* d_dst, const void* h_src, size_t bytes, void* hip_stream) {
    if (!d_dst || !h_src) return fail(GLV_ERR_INVALID, "NULL pointer");
    if (int rc = ensure_device(device)) return rc;
    HIP_TRY(hipMemcpyAsync(d_dst, h_src, bytes, hipMemcpyHostToDevice, (hipStream_t) hip_stream));
    return GLV_OK;
}
int glv_device_download(int device, void* h_dst, const void* d_src, size_t bytes, void* hip_stream) {
    if (!h_dst || !d_src) return fail(GLV_ERR_INVALID, "NULL pointer");
    if (int rc = ensure_device(device)) return rc;
    HIP_TRY(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, (hipStream_t) hip_stream));
    return GLV_OK;
}
int glv_device_sync(int device, void* hip_stream) {
    if (int rc = ensure_device(device)) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t) hip_stream));
    return GLV_OK;
}

int glv_unpack_s16(int device, const int16_t* pcm, size_t frames, int channels, float* l, float* r) {
    if (!l || !r) return fail(GLV_ERR_INVALID, "NULL output");
    if (channels != 1 && channels != 2) return fail(GLV_ERR_INVALID, "channels=%d: must be 1 or 2", channels);
    if (frames == 0) return GLV_OK;
    if (int rc = ensure_device(device)) return rc;
    DeviceArray<int16_t> d_pcm;
    DeviceArray<float> d_l, d_r;
    if (pcm) HIP_TRY(d_pcm.upload(pcm, frames * 2));
    else     HIP_TRY(d_pcm.alloc(frames * 2, true));            // fifo.c:67-79
    HIP_TRY(d_l.alloc(frames, false));
    HIP_TRY(d_r.alloc(frames, false));
    HIP_TRY(glv::launch_unpack(d_pcm, frames, channels == 1, d_l, d_r, nullptr));
    HIP_TRY(hipMemcpy(l, d_l, frames * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(r, d_r, frames * 4, hipMemcpyDeviceToHost));
    return GLV_OK;
}
}  // extern "C"
