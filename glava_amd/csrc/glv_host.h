// glv_host.h -- what the host units behind the C ABI share (glv_api.cpp, glv_wisdom.cpp, glv_device_state.cpp, glv_bar_tables.cpp, glv_chain.cpp,
// glv_track.cpp): the error channel, the device-array owner, the batch and what it holds, and the functions that cross a unit boundary.  Internal: all
// of it is hidden from the library's dynamic symbol table (namespace glvh), except the two opaque types of include/glv_spectrum.h.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/glv_spectrum.h"
#include "glv_launch.h"       // FrameGeometry, the launchers' table structs; through it glv_frame.h's FrameArgs / FrameClass (no unit instantiates a kernel)

namespace glvh __attribute__((visibility("hidden"))) {
extern thread_local std::string g_err;      // glv_last_error()'s string (glv_api.cpp)
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(GLV_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

inline int log2_exact(uint32_t v) {
    int l = 0;
    while ((1u << l) < v) ++l;
    return (1u << l) == v ? l : -1;
}

// smooth_audio()'s shape as the tables take it: 0 in a glv_params field is the shipped value (smooth_parameters.glsl:17-42)
inline float shape_scale(const glv_params& p) { return p.sample_scale != 0.0f ? p.sample_scale : 8.0f; }
inline float shape_range(const glv_params& p) { return p.sample_range != 0.0f ? p.sample_range : 0.9f; }
inline float shape_hybrid(const glv_params& p) { return p.sample_hybrid_weight != 0.0f ? p.sample_hybrid_weight : 0.65f; }
inline bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }
inline bool same_shape(const glv_params& a, const glv_params& b) {
    return a.round_formula == b.round_formula && a.sample_mode == b.sample_mode && same_bits(a.sample_hybrid_weight, b.sample_hybrid_weight)
           && same_bits(a.sample_scale, b.sample_scale) && same_bits(a.sample_range, b.sample_range);
}

// glv_params.gl_storage 3: the CPU operators on float state as with 0, and GLV_OP_BARS samples the GL_R16 upload of the finished float rows (GLava with
// `setaccelfft false`: render.c:2149-2155, :2185, :2276-2303).  State, float rows and texels out are gl_storage 0's in every bit.
inline bool upload_storage(const glv_params& p) { return p.gl_storage == 3u; }

constexpr int kOpsClasses = 7, kInKinds = 7;     // wisdom classes (wisdom_class): glv::FrameClass 0..6
constexpr int kMaxVariants = 4;
// glv_batch_track_wave_s16, bars in one launch: a workgroup's rows are consecutive output rows (false) or consecutive steps of one channel row (true).
// profiles/r11/track_wave.txt (N = 4096, hop 256, ms by rows / by steps): 1 stream x 2048 steps 0.066 / 0.048, 8 streams 0.207 / 0.178, 64 streams 1.38 / 1.43,
// 1024 streams x 256 steps 2.47 / 2.65 -- apart by about the round-to-round spread either way (the two-launch point, where the order plays no part, shows the
// same 0.064 / 0.044 between the two batches); by rows is the plain order and wastes no partial block per channel row when steps are few.
constexpr bool kTrackWaveBySteps = false;

// One array in device memory and its only owner: freed when the owner goes, so no table has a free list to be kept in step with.
// upload() / alloc() make the new array completely before the held one is replaced and freed: after a failure the owner holds what
// it held.  Synchronous (hipMalloc, hipMemcpy from pageable memory): creation and the set calls only, never the process path
// (tests/test_stream_order.py forbids these names there).
template <class T> class DeviceArray {
    T* p_ = nullptr;
    hipError_t renew(const T* src, size_t count, bool zeroed) {
        T* q = nullptr;
        hipError_t e = hipMalloc(&q, sizeof(T) * count);
        if (e == hipSuccess && src) e = hipMemcpy(q, src, sizeof(T) * count, hipMemcpyHostToDevice);
        if (e == hipSuccess && zeroed) e = hipMemset(q, 0, sizeof(T) * count);
        if (e != hipSuccess) { if (q) (void) hipFree(q); return e; }
        reset();
        p_ = q;
        return hipSuccess;
    }
public:
    DeviceArray() = default;
    DeviceArray(DeviceArray&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DeviceArray& operator=(DeviceArray&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    ~DeviceArray() { reset(); }
    hipError_t upload(const T* src, size_t count) { return renew(src, count, false); }       // exactly `count` elements, copied from the host
    hipError_t upload(const std::vector<T>& v) { return renew(v.data(), v.size(), false); }
    hipError_t alloc(size_t count, bool zeroed) { return renew(nullptr, count, zeroed); }     // no host data: as hipMalloc left them, or zeros
    void reset() { if (p_) (void) hipFree(p_); p_ = nullptr; }
    T* get() const { return p_; }
    operator T*() const { return p_; }
};

// Device-resident constants of one transform size (glv_device_state.cpp: SharedTables are per (device, n), the tilt factors per batch).
struct SharedTables;
struct Tables {
    SharedTables* shared = nullptr;
    glv::cf* d_tw = nullptr;
    double* d_win = nullptr;
    float* d_win_split = nullptr;      // the same window as float pairs, for s16 samples (glv_core.h WinSplit; made on the device)
    int win_shifted = 0;               // positions whose low part was moved by an ulp or more (diagnostics)
    glv::LogEntry* d_log = nullptr;
    DeviceArray<float> d_tilt;
    float tilt_scale = 0.f, tilt_cutoff = 0.f;
    bool tilt_fold = false;
    uint32_t n_ = 0;
    int set_tilt(float fft_scale, float fft_cutoff, bool fold);
    static int make_shared(SharedTables* t);
    int create(uint32_t n, int device);
    void destroy();
};

// One set of GLV_OP_BARS tables (host generated).  A batch holds two: the bars of glv_params (glv_batch::bar) and, while glv_batch_set_bar_texels /
// glv_batch_set_column_texels has a table set, the bars at texels of the pre-smoothing pass (glv_batch::snap).
struct BarTableSet {
    DeviceArray<glv::BarDesc> desc;          // taps
    DeviceArray<float> w;                    // their weights, + one chunk of zeros for padding items (snapped: the uint32 weights W' as float bits; columns
                                             // under maximum / hybrid: the float weights in tap order)
    // work lists for the fused epilogue (lanes / GL groups per row), one per kernel configuration of the size (their lanes per row differ)
    DeviceArray<glv::BarItem> fitems[kMaxVariants];
    uint32_t fnsteps[kMaxVariants] = {}; bool fusable[kMaxVariants] = {};
    DeviceArray<glv::BarModeBlock> mblocks; DeviceArray<float> mw; uint32_t nmblocks = 0;   // sample_mode maximum / hybrid (glv_tables.h make_bar_mode_blocks)
    uint32_t bins = 0;                       // bins of a row the bars sample (bins_reached; 0: no tap, every bin counts as sampled)
};
// ... and what only the bars of glv_params have
struct BarExtras {
    DeviceArray<glv::BarItem> items; uint32_t nsteps = 0;   // work lists for glv_bars_kernel (32 groups per row)
    // >= 256 bars (glv_tables.h make_bar_mtiles): tiles of 32 bars, their weights in MFMA operand layout, the bars' {weight sum, reciprocal}, and -- when
    // they could be cut -- the rounds of glv_bars_rows_kernel for its LDS ring
    DeviceArray<glv::BarMTile> mtiles; DeviceArray<float> wt, wsum; DeviceArray<glv::BarTile> rounds;
    uint32_t ntiles = 0, nrounds = 0, ring_bins = 0, bins_needed = 0;      // bins_needed: bins of a row the many-bars kernels sample (0: all)
    uint32_t chunk_reach = 0;    // bins of a row the chunked work lists READ: whole chunks, past a bar's last tap with weights of +0 (glv_tables.h bar_chunk_reach)
    // the same pass over TEXEL rows (the GL chains, gl_storage != 0): exact integer arithmetic on the i8 matrix cores (glv_tables.h make_bar_itiles)
    DeviceArray<glv::BarMTile> itiles; DeviceArray<int8_t> wq; DeviceArray<glv::BarIFin> fin; DeviceArray<glv::BarTile> irounds;
    uint32_t intiles = 0, inrounds = 0, iring_bins = 0;
    bool i8_none = false;        // the integer tables could not be made for these parameters (a bar wider than any ring / P > 31): the f32 chain serves
    uint32_t count = 0; float factor = -1.f, phase = 0.f;
    glv_params shape_of{};       // made for: bars, smooth_factor, bar_phase and the shape fields (round_formula ... sample_range)
    glv::BarIRowsTables irows_tables() const { return glv::BarIRowsTables{itiles, intiles, wq, fin, irounds, inrounds, iring_bins}; }
    bool i8() const { return irounds.get() != nullptr && inrounds != 0; }
};
// ... and the bars at texels of the pre-smoothing pass.  glv_batch_set_bar_texels: bar k is texel tex[k] (the twin: bars = n, bar_phase 0.5); empty = off.
// The set follows the snapped taps: average -- snapped desc (weight_sum 1, NaN where the weights sum to 0), W' in tap_w's layout plus a zero chunk, one fused
// work list per kernel configuration; maximum / hybrid -- the snapped desc and glv_bars_mode_kernel's blocks.
// glv_batch_set_column_texels: column x is the mean of texels col_tex[x][0..2] of the same pass.  tex then holds the DISTINCT texels (sorted) and the set
// is made over those; col_map says where a column's three sit among them.  The second launch (glv_columns_kernel) has work lists of its own
// (256 / bar_lanes_of(n) groups).
struct SnapExtras {
    std::vector<uint32_t> tex;
    std::vector<uint32_t> col_tex;           // [bars][3] as the caller gave them; empty = off
    DeviceArray<glv::ColumnMap> col_map;
    DeviceArray<glv::BarItem> col_items; uint32_t col_nsteps = 0;
    glv_params of{};                         // the parameters the set was made for (smooth_factor, the shape, bars)
};

// A start / stop pair of HIP events of a call that times its own launches (glv_batch_autotune, glv_batch_tune_placement): both go with the owner.
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    EventPair() = default; EventPair(const EventPair&) = delete; EventPair& operator=(const EventPair&) = delete;
    ~EventPair() { if (e0) (void) hipEventDestroy(e0); if (e1) (void) hipEventDestroy(e1); }
    hipError_t create() { const hipError_t e = hipEventCreate(&e0); return e != hipSuccess ? e : hipEventCreate(&e1); }
};
}  // namespace glvh
using namespace glvh;

// =====================================================================================================
struct glv_batch {
    glv_params p;
    uint32_t streams = 0;
    unsigned ops_mask = 0;
    int device = 0;
    int log_nn = 0;
    int num_cus = 256;
    Tables tab;
    float* d_grav = nullptr;     // [streams*2][n]      gravity state owned by the batch (gravity without average)
    const float* grav_cur = nullptr;   // where the latest gravity output lives: d_grav, or the caller's output buffer of the previous
                                 // call when the output doubles as the state (render.c:733-734; see GLV_OP_PRIVATE_STATE)
    float* d_hist = nullptr;     // [streams*2][F][n]   ring (average; doubles as gravity state)
    DeviceArray<int16_t> d_ring;     // [streams][n][2]     FIFO ring mode
    int grav_mode = 0;           // which buffer holds gravity's `applied`: 0 not used yet, 1 d_grav (gravity without average
                                 // in the same call), 2 the newest ring slot (gravity + average fused)
    uint32_t head = 0;           // history slot receiving the next frame
    uint32_t ring_pos = 0;       // next write position in the PCM ring, in frames
    int grid_override = 0;
    int variant_override = -1;   // kernel configuration forced by glv_batch_set_variant (-1 = wisdom / default)
    int attr_log_mode = -1;      // log mode whose kernels had their function attributes set (batch_prepare)
    int last_launches = 0;       // kernels the last process call launched
    int last_grid = 0;           // workgroups of the last frame-kernel launch
    int last_variant = 0;        // kernel configuration of the last frame-kernel launch
    char device_name[48] = "unknown";
    // what the wisdom said the last time it was asked, per (input kind, kernel class): valid while `gen` equals the table's
    // generation -- the launch path takes no lock and scans nothing once an answer is cached
    struct PlanCache { uint64_t gen = 0; int variant = 0, grid = 0; bool hit = false; } plan_cache[kInKinds][kOpsClasses];
    uint32_t rows = 0;           // channel rows the state arrays and the scratch rows were sized for (streams * 2; 1 for the single-stream drop-ins)
    bool single_row = false;
    bool unfused_bars = false;   // GLV_UNFUSED_BARS in the environment at creation (diagnostics: bars always as a second launch)
    bool unfused_wave = false;   // GLV_UNFUSED_WAVE likewise: GLV_OP_WAVE | GLV_OP_BARS always as the waveform kernel + the bars kernel
    bool track_wave_by_steps = kTrackWaveBySteps;   // row order of glv_batch_track_wave_s16's one-launch form (GLV_TRACK_WAVE_ORDER=rows|steps at creation: diagnostics)
    uint32_t track_frames_segment = 0;              // frames per segment of glv_batch_track_frames_s16 / _f32's frames kernel (GLV_TRACK_FRAMES_SEGMENT=<frames> at creation: diagnostics; 0: glv::track_frames_segment)
    bool state16 = false;        // gl_storage == 1 at creation: d_grav / d_hist hold uint16 texels (2 bytes per value)
    float grav_g = 0.f; uint32_t grav_sub = 0; bool grav_int = false, grav_known = false;   // the gravity step on texels (glv_tables.h gravity_r16_integer_step)
    DeviceArray<float> d_scratch;    // [streams*2][n] spectra feeding GLV_OP_BARS
    DeviceArray<float> d_ring_f32;   // [streams][n][2] interleaved f32 ring (glv_batch_ring_update_f32)
    uint32_t bufscale = 1;           // `setbufscale k` (glv_batch_set_bufscale): a window of every process and track call is k * n frames, decimated to n (render.c:1765-1790); 1: off
    DeviceArray<float> d_decim;      // [streams*2][n] the decimated rows of a process call, which the chain then reads as IN_F32_PLANAR; held while bufscale > 1
    uint32_t ring_pos_f32 = 0;
    DeviceArray<int> d_smin, d_smax; // transform_smooth window bounds (host generated)
    uint32_t smooth_asz = 0;
    uint32_t smooth_reach = 0;   // floats of a row the walk touches: max smax + 1 (>= asz)
    uint32_t smooth_window = 0;  // largest smax - smin + 1; also covers smax - t and t - smin (the ring kernel's slot reuse)
    float smooth_d = -1.f, smooth_r = -1.f;
    BarTableSet bar; BarExtras bar_x;        // GLV_OP_BARS: the bars of glv_params (ensure_bar_tables)
    BarTableSet snap; SnapExtras snap_x;     // ... and at texels of the pre-smoothing pass (build_snap_tables; snap.bins: never 0 while a table is set)
    bool bar_i8_off = false;     // GLV_NO_BARS_I8 in the environment at creation (diagnostics: the f32 matrix-core kernel on texel rows too)
    // bytes of the two state arrays as created (batch_alloc), cleared (glv_batch_reset) and re-placed (glv_batch_tune_placement)
    size_t grav_bytes() const { return (state16 ? sizeof(uint16_t) : sizeof(float)) * rows * p.n; }          // GL_R16 state: texels
    size_t hist_bytes() const { return grav_bytes() * p.avg_frames; }
    // the bookkeeping of a batch whose state arrays were just cleared -- or can no longer be trusted (a failed placement candidate)
    void rewind_state() { head = 0; grav_mode = 0; grav_cur = d_grav; ran_live = false; kept_live = 0; }
    bool snapped() const { return !snap_x.tex.empty(); }
    bool columns() const { return !snap_x.col_tex.empty(); }
    // GLV_OP_BARS_ONLY: the chain lives below the bins the bars sample (the last bin any bar has a tap on, rounded up to 64) -- when EVERY kernel configuration
    // of the size keeps those bins alive in its live class (a compile-time share of the row, FrameGeometry::live_points; whichever configuration a
    // call runs, the bins the bars sample are maintained) and a live class exists for the chain: the GL_R16 chains have one with the bars in a second
    // launch (7) and one with the bars fused (9); the float chains only the fused one (8).
    // 0: every bin is live (no flag, or one of the conditions fails: the full chain, the same results)
    uint32_t live_bins_now = 0;                     // refreshed with the bar tables and when the batch is prepared (update_live_bins)
    uint32_t live_bins() const { return live_bins_now; }
    bool ran_live = false;                          // a live kernel class has run since creation / the last reset: the state beyond the live bins is stale
    // ... and how far it is not: the smallest extent any live call since then has kept (a process call its live bins, a live track call its kept bins, adopted
    // live streams theirs).  Bins [0, kept_live) of every stream are maintained, nothing beyond is; meaningful while ran_live
    uint32_t kept_live = 0;
    void ran_live_over(uint32_t bins) { kept_live = ran_live && kept_live < bins ? kept_live : bins; ran_live = true; }
    uint32_t kept_bins() const { return ran_live ? kept_live : p.n; }
    // may the bars sample `live` bins from now on (0: every bin)?  Once a live call has run, only what every such call kept
    bool keeps_live(uint32_t live) const { return !ran_live || (live != 0 && live <= kept_live); }
    // the live bins with snapped bars that sample `snap_bins` bins of a row (0: none set)
    uint32_t live_bins_with(uint32_t snap_bins) const {
        // (snapped bars sample positions in [0, 1) -- the unsnapped bars' last taps reach scale_audio(1) n once smooth_factor >= 1 / bars; a smaller
        // factor can leave the last snapped taps beyond them, and the live bins then grow to cover them)
        const uint32_t sampled = snap_bins > bar.bins ? snap_bins : bar.bins;
        if (!(ops_mask & GLV_OP_BARS_ONLY) || sampled == 0 || sampled >= p.n || p.gl_storage > 1u || p.log_mode == 2u) return 0u;
        for (int v = 0; v < glv::frame_variants(log_nn); ++v)
            if ((uint32_t) glv::frame_geometry(log_nn, v).live_points * 2u < sampled) return 0u;
        // (a float chain's live class is the fused one: the production configuration must take the bars; a call that runs a configuration which cannot
        // -- forced, or from the wisdom -- takes the full chain for that call: it maintains every bin, the live calls the sampled ones, the bars see no difference)
        if (p.gl_storage == 0u && (!bar.fusable[0] || unfused_bars)) return 0u;
        return sampled;
    }
    void update_live_bins() { live_bins_now = live_bins_with(snapped() ? snap.bins : 0u); }
    // timing
    bool timing = false;
    std::vector<hipEvent_t> ev;  // start/stop pairs
    size_t ev_used = 0;
    uint64_t launches = 0;
    const char* kernel_name = "glv_frame_kernel";
};

struct glv_state {
    glv_batch* b = nullptr;      // a one-row batch (one channel of one stream)
    // Staging of the host-pointer drop-ins: one pinned, device-mapped host block.  The kernel reads the n input floats
    // straight out of it over PCIe and writes its n results (or n GL_R16 texels) straight back, so a call is one launch
    // and one stream synchronisation -- no hipMemcpy in either direction (2 x 16 KB at the default size: the copies'
    // fixed cost, not their bandwidth, was what a call spent its time on).  GLV_STAGING=copy selects the device
    // buffer + two hipMemcpyAsync of round 1 (kept for A/B in tests/test_gpu_parity.py::test_single_stream_dropin_latency).
    float* h_io = nullptr;       // host view
    float* d_io = nullptr;       // device view of h_io (mapped), or a device buffer when copy staging is selected
    uint16_t* h_tex = nullptr;   // the texel outputs' staging, made by the first call that needs it (round_trip)
    uint16_t* d_tex = nullptr;   // device view of h_tex (mapped), or tex_copy's array
    DeviceArray<uint16_t> tex_copy;
    DeviceArray<float> seq;      // device buffer for GLV_OP_SMOOTH: its kernel walks a row element by element, which must not happen over PCIe
    bool mapped = true;
};

namespace glvh __attribute__((visibility("hidden"))) {
// How one process call runs, decided once before anything is launched (plan_chain) and then carried out (run_chain).
struct ChainPlan {
    enum Route {
        GL_FUSED,       // render.c:2188-2265 (+ :2277-2303 with bars) in ONE launch on uint16 state (gl_fused_chain)
        GL_PASSES,      // the transform, then gravity / average as the post kernel's pass over GL_R16-quantised values (gl_passes_chain)
        FRAME,          // the frame kernel
        POST,           // operators on planar rows (no GLV_OP_FFT)
        COPY,           // smooth / bars only: on a copy of the input rows
        WAVE,           // GLV_OP_WAVE: unpack, wrange, upload (glv_wave_kernel) -- with bars the integer pass straight from the frames, or two launches
    } route = FRAME;
    enum Bars { NO_BARS, BARS_F32, BARS_I8, BARS_I8_FLOATS,                    // the second bars launch: over f32 rows, over texel rows (the
                                                                               // integer matrix-core pass), over texel values as floats c / 65535;
                BARS_SNAP, BARS_SNAP_FLOATS, BARS_SNAP_MODE,                    // bars at texels of the pre-smoothing pass: over texel rows, over
                                                                               // c / 65535, and sample_mode maximum / hybrid (glv_bars_mode_kernel)
                BARS_COLUMNS,                                                   // means of three such texels (glv_columns_kernel; rows c / 65535)
                BARS_COLUMNS_TEXELS,                                            // ... over texel rows (a columns track call's scan results; gl_storage 3)
                BARS_MODE_TEXELS, BARS_SNAP_MODE_TEXELS } bars = NO_BARS;       // BARS_F32 / BARS_SNAP_MODE under maximum / hybrid over texel rows (gl_storage 3:
                                                                               // glv_bars_mode_kernel's texel-row kind)
    int variant = 0, grid = 0;                  // the frame kernel's configuration and workgroups (FFT chains)
    glv::FrameClass cls = glv::FC_PLAIN;        // ... and its class
    unsigned ops = 0;                           // what the first kernel runs (FrameArgs::ops)
    bool fused_bars = false;                    // the bars computed in the frame kernel, from the finished row in LDS
    float* out = nullptr;                       // where the first kernel writes its rows (NULL: the state is the output, or only bars leave)
    float* rows = nullptr;                      // the finished rows: what the smooth pass and the second bars launch work on
    uint32_t out_limit = 0, live_points = 0;    // FrameArgs::out_limit / live_points
    bool wave_fused = false;                    // WAVE: the bars in ONE launch (glv_bars_rows_i8_kernel parks texels made from the s16 frames)
    bool wave_r16 = false;                      // WAVE: the waveform kernel writes texels (else their floats c / 65535)
    uint32_t wave_limit = 0;                    // WAVE: samples of a row the waveform kernel produces (what the bars sample, or n)
    const void* dec_in = nullptr;               // bufscale > 1: the caller's windows of k * n frames, which the first launch of the chain decimates into the batch's
    int dec_kind = 0;                           // staging rows (glv::DecimateKind) -- the chain is then the planar entry's on those rows
    uint32_t dec_streams = 0;                   // ... for the streams of the call: units / 2 (all of the batch, or the prefix of a glv_batch_process_first_* call)
};

// ---- what crosses a unit boundary, in the order glv_wisdom / glv_device_state / glv_bar_tables / glv_chain.cpp (indented: tests/src_scan.py finds a DEFINITION by its return type at the start of a line) ----
    void launch_plan(glv_batch* b, uint32_t units, int in_mode, unsigned ops, int* variant, int* grid);
    void wisdom_load_env();
    void state_free(void* p);
    int batch_alloc(glv_batch* b);
    glv::BarRowsTables rows_tables(const glv_params& p, const BarExtras& x, const BarTableSet& s);
    int ensure_smooth_tables(glv_batch* b); int ensure_bar_tables(glv_batch* b); int ensure_scratch(glv_batch* b); int ensure_snap_tables(glv_batch* b);
    bool snap_current(const glv_batch* b);
    bool bars_fusable(const glv_batch* b, unsigned ops);
    bool bars_need_rows(const glv_batch* b, const BarTableSet& s);
    bool gl_fused_chain(const glv_batch* b, unsigned ops);
    unsigned frame_ops(const glv_batch* b, unsigned ops);
    void fill_common(glv::FrameArgs& a, const glv_params& p, const Tables& t);
    int timed_launch_begin(glv_batch* b, hipStream_t st); int timed_launch_end(glv_batch* b, hipStream_t st);
    void update_gravity_step(glv_batch* b);
    int batch_prepare(glv_batch* b);
    int check_ops(const glv_batch* b, unsigned ops, const float* d_out);
    int plan_wave(const glv_batch* b, int in_mode, unsigned ops, uint32_t rot, float* d_out, ChainPlan& pl, bool whole_groups);
    int launch_bars_pass(glv_batch* b, const ChainPlan& pl, float* d_bars, size_t units, bool r16, hipStream_t st);
    int refuse_gravity_mix(const glv_batch* b, unsigned ops); void commit_gravity_form(glv_batch* b, unsigned ops); int refuse_stale_tilt(const glv_batch* b);
    int process(glv_batch* b, const void* d_in, int in_mode, float* d_out, unsigned ops, uint32_t units, uint32_t rot, hipStream_t st, const void* dec_in = nullptr,
                int dec_kind = 0);
    int process_windows(glv_batch* b, const void* d_in, int in_mode, int dec_kind, float* d_out, unsigned ops, hipStream_t st);
    int process_first(glv_batch* b, uint32_t count, const void* d_in, int in_mode, int dec_kind, float* d_out, unsigned ops, hipStream_t st);
    int refuse_prefix(const glv_batch* b, const char* entry, uint32_t count);
    int refuse_bufscale(const glv_batch* b, const char* entry);
}  // namespace glvh
