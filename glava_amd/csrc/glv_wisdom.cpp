// glv_wisdom.cpp -- the launch wisdom: its table and file format, the (kernel configuration, workgroups) of every frame-kernel launch, and the C
// entries that tune, save, load and override them.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <mutex>

#include "glv_host.h"

namespace {
// ---- launch wisdom ----------------------------------------------------------------------------------------------------
// The role glfft's FFTWisdom plays in the reference tree (glfft/glfft_wisdom.cpp:235-446: time candidate work-group shapes
// and radix splits per transform on the target, remember the winner per transform description).  Two things are open at run
// time here: WHICH kernel configuration of the size runs (glv_inst.hip Tuned<K, V>: points per lane / radix split, rows per
// workgroup, where the window and twiddle tables live) and HOW MANY persistent workgroups a launch uses.  Both depend on the
// size, the operator chain, the stream count and the part.  glv_batch_autotune measures the candidates on the device the
// batch lives on; entries are process-wide, keyed on the device's identity (name, CU count) so that a file tuned on one part
// is not applied on another, can be saved and loaded (GLV_WISDOM=<file> loads one when the first batch is created) and are
// consulted by every launch (through a per-batch cache: no lock on the launch path once an answer is cached).
struct WisdomKey { uint32_t n, in_kind, ops_class, log_mode, streams_log2, avg_frames, cus; char device[48]; };
struct WisdomEntry { WisdomKey k; int variant, grid; float ms; };
std::mutex g_wisdom_mu;
std::vector<WisdomEntry> g_wisdom;
std::atomic<uint64_t> g_wisdom_gen{1};      // bumped by every change of the table: invalidates the per-batch caches
bool g_wisdom_env_loaded = false;

uint32_t log2_round(uint32_t v) { uint32_t l = 0; while ((2u << l) <= v) ++l; return ((v >> l << l) * 3 / 2 <= v && l < 31) ? l + 1 : l; }
bool same_key(const WisdomKey& a, const WisdomKey& b) {
    return a.n == b.n && a.in_kind == b.in_kind && a.ops_class == b.ops_class && a.log_mode == b.log_mode && a.streams_log2 == b.streams_log2
           && a.avg_frames == b.avg_frames && a.cus == b.cus && std::strncmp(a.device, b.device, sizeof(a.device)) == 0;
}
void key_set_device(WisdomKey& k, const char* name, uint32_t cus) {
    std::memset(k.device, 0, sizeof(k.device));
    size_t j = 0;
    for (const char* c = name; *c && j + 1 < sizeof(k.device); ++c) k.device[j++] = (*c == ' ' || *c == '\t' || *c == '\n') ? '_' : *c;
    if (j == 0) std::strcpy(k.device, "unknown");
    k.cus = cus;
}
bool wisdom_lookup(const WisdomKey& k, int* variant, int* grid) {
    std::lock_guard<std::mutex> lock(g_wisdom_mu);
    for (const WisdomEntry& e : g_wisdom) if (same_key(e.k, k)) { *variant = e.variant; *grid = e.grid; return true; }
    return false;
}
void wisdom_store(const WisdomKey& k, int variant, int grid, float ms) {
    std::lock_guard<std::mutex> lock(g_wisdom_mu);
    g_wisdom_gen.fetch_add(1, std::memory_order_release);
    for (WisdomEntry& e : g_wisdom) if (same_key(e.k, k)) { e.variant = variant; e.grid = grid; e.ms = ms; return; }
    g_wisdom.push_back(WisdomEntry{k, variant, grid, ms});
}
// Returns the number of entries loaded, -1 when the file cannot be opened.  Lines that are not entries of the current (v2,
// 11-field) format are counted: *skipped, of which *v1 look like the 7-field format of round 2 (n input_kind ops_class log_mode
// log2(streams) workgroups ms) -- a tuned deployment must not fall back to defaults unnoticed.
int wisdom_load_file(const char* path, int* skipped = nullptr, int* v1 = nullptr) {
    FILE* f = std::fopen(path, "r");
    if (!f) { (void) fail(GLV_ERR_INVALID, "cannot open wisdom file %s", path); return -1; }
    char line[320];
    int n_loaded = 0, n_skipped = 0, n_v1 = 0;
    while (std::fgets(line, sizeof(line), f)) {
        if (line[0] == '#' || line[0] == '\n') continue;
        WisdomKey k; int variant, grid; float ms; char dev[48];
        std::memset(&k, 0, sizeof(k));
        if (std::sscanf(line, "%47s %u %u %u %u %u %u %u %d %d %f", dev, &k.cus, &k.n, &k.in_kind, &k.ops_class, &k.log_mode, &k.streams_log2,
                        &k.avg_frames, &variant, &grid, &ms) == 11 && grid > 0 && variant >= 0) {
            key_set_device(k, dev, k.cus);
            wisdom_store(k, variant, grid, ms); ++n_loaded;
        } else {
            ++n_skipped;
            unsigned a[5]; int g1; float m1; char tail[8];
            if (std::sscanf(line, "%u %u %u %u %u %d %f %7s", &a[0], &a[1], &a[2], &a[3], &a[4], &g1, &m1, tail) == 7) ++n_v1;
        }
    }
    std::fclose(f);
    if (skipped) *skipped = n_skipped;
    if (v1) *v1 = n_v1;
    return n_loaded;
}

// The launch wisdom's class of an FFT chain: its frame kernel's class with the bars fused and every bin live.  The key is chosen before the
// configuration, and whether the bars fuse depends on the configuration (BarTableSet::fusable[variant]): a chain with GLV_OP_BARS is class 2 or 6
// even where its bars run as a second launch.  The values are part of the wisdom file format (0..6).
uint32_t wisdom_class(const glv_batch* b, unsigned ops) {
    const unsigned f = frame_ops(b, ops);
    return (uint32_t) glv::frame_class(gl_fused_chain(b, ops), (f & GLV_OP_BARS) != 0, false, f);
}

WisdomKey wisdom_key(const glv_batch* b, int in_mode, unsigned ops) {
    WisdomKey k;
    std::memset(&k, 0, sizeof(k));
    k.n = b->p.n; k.in_kind = (uint32_t) in_mode; k.ops_class = wisdom_class(b, ops); k.log_mode = b->p.log_mode;
    k.streams_log2 = log2_round(b->streams);
    k.avg_frames = (frame_ops(b, ops) & GLV_OP_AVERAGE) ? b->p.avg_frames : 0;          // F changes what a stateful launch moves
    key_set_device(k, b->device_name, (uint32_t) b->num_cus);
    return k;
}

// workgroups of a launch of configuration `variant` over `units` rows when nothing has been tuned
int default_grid(const glv_batch* b, uint32_t units, int variant) {
    const glv::FrameGeometry g = glv::frame_geometry(b->log_nn, variant);
    const uint32_t wgs = (units + g.rows_per_trip - 1) / g.rows_per_trip;
    // persistent workgroups: up to g.rounds rounds of what fits the chip (N=8192, 8192 streams: 0.194 ms with 256-512
    // workgroups, 0.224 ms with 2048; N<=4096, 65536 streams: eight rounds beat two by 1-4 %, profiles/r04/grid_ab.txt)
    const uint32_t round = (uint32_t) b->num_cus * (uint32_t) g.resident;
    if (wgs <= round) return (int) wgs;
    // more rounds than one even out the tail (the hardware dispatches the next workgroup to whichever CU is free), as long as a
    // workgroup still makes at least eight trips: every workgroup pays a prologue (window / table staging, pipeline fill) --
    // N=4096, 16384 streams: 0.168 ms with 512-1024 workgroups, 0.173 with 2048, 0.183 with 4096
    uint32_t grid = wgs / 8u;
    if (grid < round) grid = round;
    if (grid > (uint32_t) g.rounds * round) grid = (uint32_t) g.rounds * round;
    return (int) grid;
}
}  // namespace
namespace glvh __attribute__((visibility("hidden"))) {
// (kernel configuration, workgroups) of the next frame-kernel launch: explicit overrides, else the wisdom, else the defaults
void launch_plan(glv_batch* b, uint32_t units, int in_mode, unsigned ops, int* variant, int* grid) {
    int v = 0, g = 0;
    const uint32_t cls = wisdom_class(b, ops);
    if (b->variant_override < 0 || b->grid_override <= 0) {
        glv_batch::PlanCache& pc = b->plan_cache[in_mode][cls];
        const uint64_t gen = g_wisdom_gen.load(std::memory_order_acquire);
        if (pc.gen != gen) {
            pc.hit = wisdom_lookup(wisdom_key(b, in_mode, ops), &pc.variant, &pc.grid);
            // the ring mode runs the frame mode's kernel with a rotated read position: what was tuned for frames (the input
            // glv_batch_autotune measures) serves it until an entry of its own exists
            // (... and a track call's windows run it with another address per frame: glv::IN_S16_TRACK)
            if (!pc.hit && (in_mode == glv::IN_S16_RING || in_mode == glv::IN_S16_TRACK)) pc.hit = wisdom_lookup(wisdom_key(b, glv::IN_S16_STEREO, ops), &pc.variant, &pc.grid);
            // (... and those of a float recording, glv::IN_F32_TRACK, the interleaved f32 frames' kernel)
            if (!pc.hit && in_mode == glv::IN_F32_TRACK) pc.hit = wisdom_lookup(wisdom_key(b, glv::IN_F32_STEREO, ops), &pc.variant, &pc.grid);
            pc.gen = gen;
        }
        if (pc.hit) { v = pc.variant; g = pc.grid; }
    }
    if (b->variant_override >= 0) { if (b->variant_override != v) g = 0; v = b->variant_override; }
    if (!glv::frame_variant_ok(b->log_nn, in_mode, (int) b->p.log_mode, v)) { v = 0; g = 0; }     // not built for this input / log mode
    if (b->grid_override > 0) g = b->grid_override;
    else if (g > 0) {
        const int rpt = glv::frame_geometry(b->log_nn, v).rows_per_trip;
        const uint32_t wgs_max = (units + rpt - 1) / rpt;
        if ((uint32_t) g > wgs_max) g = (int) wgs_max;
    } else g = default_grid(b, units, v);
    *variant = v; *grid = g;
}

// GLV_WISDOM=<file>, loaded when the first batch of the process is created
void wisdom_load_env() {
    std::unique_lock<std::mutex> lock(g_wisdom_mu);
    const bool first = !g_wisdom_env_loaded;
    g_wisdom_env_loaded = true;
    lock.unlock();
    if (first) if (const char* w = std::getenv("GLV_WISDOM")) {                                    // a missing file is not an error
        int skipped = 0, v1 = 0;
        const int nl = wisdom_load_file(w, &skipped, &v1);
        if (nl >= 0 && skipped > 0)
            std::fprintf(stderr, "glv: GLV_WISDOM=%s: %d entries loaded, %d line(s) skipped%s\n", w, nl, skipped, v1 ? " (7-field v1 format: re-tune)" : "");
    }
}
}  // namespace glvh

extern "C" {
int glv_wisdom_clear(void) {
    std::lock_guard<std::mutex> lock(g_wisdom_mu);
    g_wisdom.clear();
    g_wisdom_gen.fetch_add(1, std::memory_order_release);
    return GLV_OK;
}
int glv_wisdom_count(void) { std::lock_guard<std::mutex> lock(g_wisdom_mu); return (int) g_wisdom.size(); }
int glv_wisdom_load(const char* path) {
    if (!path) return fail(GLV_ERR_INVALID, "path is NULL");
    int skipped = 0, v1 = 0;
    const int n = wisdom_load_file(path, &skipped, &v1);
    if (n < 0) return GLV_ERR_INVALID;
    if (skipped > 0) {
        // a file that yields nothing is an error; a partly usable one loads, with the count left in glv_last_error()
        const int code = n == 0 ? GLV_ERR_INVALID : GLV_OK;
        (void) fail(code, "wisdom file %s: %d entr%s loaded, %d line(s) skipped%s", path, n, n == 1 ? "y" : "ies", skipped,
                    v1 ? " (some are in the 7-field v1 format of an older library: re-tune with glv_batch_autotune and save again)" : " (not in the 11-field v2 format)");
        return code;
    }
    g_err = "";
    return GLV_OK;
}
int glv_wisdom_save(const char* path) {
    if (!path) return fail(GLV_ERR_INVALID, "path is NULL");
    FILE* f = std::fopen(path, "w");
    if (!f) return fail(GLV_ERR_INVALID, "cannot write wisdom file %s", path);
    std::fprintf(f, "# glv launch wisdom v2: device compute_units n input_kind ops_class log_mode log2(streams) avg_frames variant workgroups ms_per_launch\n");
    std::lock_guard<std::mutex> lock(g_wisdom_mu);
    for (const WisdomEntry& e : g_wisdom)
        std::fprintf(f, "%s %u %u %u %u %u %u %u %d %d %.6f\n", e.k.device, e.k.cus, e.k.n, e.k.in_kind, e.k.ops_class, e.k.log_mode, e.k.streams_log2,
                     e.k.avg_frames, e.variant, e.grid, (double) e.ms);
    std::fclose(f);
    return GLV_OK;
}

// Time every kernel configuration built for this batch's size (glv_inst.hip Tuned<K, V>) on a few workgroup counts each, on
// the batch's device with the caller's buffers, and remember the fastest (variant, workgroups) for this (device, size, input,
// chain, log mode, stream count).  The probe launches are real updates of every stream: stateful chains are reset afterwards.
int glv_batch_autotune(glv_batch* b, const int16_t* d_pcm, float* d_out, unsigned ops, void* hip_stream, int* best_grid, float* best_ms) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!(ops & GLV_OP_FFT)) return fail(GLV_ERR_INVALID, "autotune needs GLV_OP_FFT (it tunes the frame kernel)");
    if (int rc = refuse_bufscale(b, "glv_batch_autotune")) return rc;
    if (int rc = check_ops(b, ops, d_out)) return rc;
    if (!d_pcm) return fail(GLV_ERR_INVALID, "NULL device pointer");
    hipStream_t st = (hipStream_t) hip_stream;
    HIP_TRY(hipSetDevice(b->device));
    const uint32_t units = b->streams * 2;
    struct Cand { int variant, grid; };
    std::vector<Cand> cand;
    for (int v = 0; v < glv::frame_variants(b->log_nn); ++v) {
        if (!glv::frame_variant_ok(b->log_nn, glv::IN_S16_STEREO, (int) b->p.log_mode, v)) continue;
        const glv::FrameGeometry geo = glv::frame_geometry(b->log_nn, v);
        const uint32_t wgs = (units + geo.rows_per_trip - 1) / geo.rows_per_trip;
        const uint32_t round = (uint32_t) b->num_cus * (uint32_t) geo.resident;
        for (uint32_t g : { round / 2, round, round * 3 / 2, round * 2, round * 4 }) {
            const int c = (int) (g < 1 ? 1 : (g > wgs ? wgs : g));
            bool dup = false;
            for (const Cand& x : cand) dup |= x.variant == v && x.grid == c;
            if (!dup) cand.push_back(Cand{v, c});
        }
    }
    EventPair ev; HIP_TRY(ev.create());
    const hipEvent_t e0 = ev.e0, e1 = ev.e1;
    const int saved_grid = b->grid_override, saved_variant = b->variant_override;
    Cand best{0, 0}; float bms = 0.f; int rc = GLV_OK;
    for (int pass = 0; pass < 2 && rc == GLV_OK; ++pass)                 // pass 0 warms the clocks up, pass 1 is measured
        for (const Cand& c : cand) {
            b->grid_override = c.grid; b->variant_override = c.variant;
            const int iters = pass == 0 ? 3 : 8;
            if (hipEventRecord(e0, st) != hipSuccess) { rc = fail(GLV_ERR_HIP, "hipEventRecord failed"); break; }
            for (int i = 0; i < iters && rc == GLV_OK; ++i) rc = process(b, d_pcm, glv::IN_S16_STEREO, d_out, ops, units, 0, st);
            if (rc != GLV_OK) break;
            float ms = 0.f;
            if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) {
                rc = fail(GLV_ERR_HIP, "event timing failed"); break;
            }
            ms /= (float) iters;
            if (pass == 1 && (best.grid == 0 || ms < bms)) { best = c; bms = ms; }
        }
    b->grid_override = saved_grid; b->variant_override = saved_variant;
    if (rc != GLV_OK) return rc;
    if (ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE)) { if (int r2 = glv_batch_reset(b)) return r2; }
    wisdom_store(wisdom_key(b, glv::IN_S16_STEREO, ops), best.variant, best.grid, bms);
    if (best_grid) *best_grid = best.grid;
    if (best_ms) *best_ms = bms;
    return GLV_OK;
}

// tuning hook used by tools/tune.py and bench.py --grid (0 = automatic)
int glv_batch_set_grid(glv_batch* b, int grid) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    b->grid_override = grid;
    return GLV_OK;
}
int glv_batch_set_variant(glv_batch* b, int variant) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (variant >= glv::frame_variants(b->log_nn))
        return fail(GLV_ERR_INVALID, "variant %d: n=%u has %d kernel configuration(s)", variant, b->p.n, glv::frame_variants(b->log_nn));
    b->variant_override = variant < 0 ? -1 : variant;
    return GLV_OK;
}
int glv_batch_variants(const glv_batch* b) { return b ? glv::frame_variants(b->log_nn) : 0; }
int glv_batch_last_variant(const glv_batch* b) { return b ? b->last_variant : 0; }

int glv_batch_describe_variant(const glv_batch* b, int variant, char* buf, size_t len) {
    if (!b || !buf || len == 0) return fail(GLV_ERR_INVALID, "NULL argument");
    if (variant < 0 || variant >= glv::frame_variants(b->log_nn)) return fail(GLV_ERR_INVALID, "variant %d out of range", variant);
    const glv::FrameGeometry g = glv::frame_geometry(b->log_nn, variant);
    std::snprintf(buf, len, "n=%u variant %d: %d points per lane, %d lanes per row, %d row(s) per workgroup, %d workgroup(s) per CU, "
                            "%d KiB LDS, twiddles %s, window %s", b->p.n, variant, 1 << g.log_e, g.lanes, g.slots, g.resident, (g.lds_bytes + 1023) / 1024,
                  g.twreg == 1 ? "in VGPRs" : g.twreg == 0 ? "through L2" : g.twreg == 4 ? (g.nbuf == 0 ? "in LDS (split exchange)" : "in LDS") : "middle passes in LDS, last pass through L2",
                  g.winlds ? "in LDS" : "through L2");
    return GLV_OK;
}
}  // extern "C"
