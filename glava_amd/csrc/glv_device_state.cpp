// glv_device_state.cpp -- what a batch keeps in device memory besides the bar tables: the constant tables of its transform size (shared per device
// and size), the tilt factors, the state arrays (gravity store, history ring) with their allocation policies and their placement tuning, the PCM rings.
#include <cstdlib>
#include <mutex>
#include <new>
#include <utility>

#include "glv_host.h"
#include "glv_tables.h"       // make_twiddles / make_window / make_log_table / make_tilt

namespace glvh __attribute__((visibility("hidden"))) {
// Device-resident constants of one transform size.  The size-only tables -- twiddles, the window in both forms (the float-pair
// form is SEARCHED on the device: n workgroups trying 65 536 sample values per position), the log table -- are made once per
// (device, n) and shared by every batch of that size with a reference count (glv_multi shards, the five configs[4]
// batches and the audio backends used to repeat the search and its synchronisation points); the tilt factors depend on a batch's
// parameters and stay per batch.
struct SharedTables {
    int device = 0; uint32_t n = 0; int refs = 0;
    DeviceArray<glv::cf> d_tw; DeviceArray<double> d_win; DeviceArray<float> d_win_split; DeviceArray<glv::LogEntry> d_log;
    int win_shifted = 0;
};
std::mutex g_tab_mu;
std::vector<SharedTables*> g_tabs;

// (re)generate the tilt factors when fft_scale / fft_cutoff / log mode change (render.c:845)
int Tables::set_tilt(float fft_scale, float fft_cutoff, bool fold) {
    if (d_tilt && fft_scale == tilt_scale && fft_cutoff == tilt_cutoff && fold == tilt_fold) return GLV_OK;
    std::vector<float> t(n_);
    glv::make_tilt(t.data(), n_, fft_scale, fft_cutoff, fold);
    tilt_fold = fold;
    // (rewritten where they are once they exist: the array a captured launch points at stays the one the next call reads)
    if (!d_tilt) HIP_TRY(d_tilt.upload(t));
    else HIP_TRY(hipMemcpy(d_tilt, t.data(), sizeof(float) * n_, hipMemcpyHostToDevice));
    tilt_scale = fft_scale; tilt_cutoff = fft_cutoff;
    return GLV_OK;
}
int Tables::make_shared(SharedTables* t) {
    const uint32_t n = t->n, nn = n / 2;
    std::vector<glv::cf> tw(nn, glv::cf{0.0f, 0.0f});
    std::vector<double> win(n);
    glv::make_twiddles(tw.data(), nn);
    glv::make_window(win.data(), n);
    HIP_TRY(t->d_tw.upload(tw));
    HIP_TRY(t->d_win.upload(win));
    {   // the split window: searched and proven on the device for every s16 sample value (glv_misc.hip launch_window_split)
        int* d_fs = nullptr;
        HIP_TRY(t->d_win_split.alloc(2 * (size_t) n, false));
        HIP_TRY(hipMalloc(&d_fs, 2 * sizeof(int)));
        HIP_TRY(hipMemset(d_fs, 0, 2 * sizeof(int)));
        hipError_t e = glv::launch_window_split(t->d_win, t->d_win_split, n, d_fs, nullptr);
        int fs[2] = {0, 0};
        if (e == hipSuccess) e = hipMemcpy(fs, d_fs, sizeof(fs), hipMemcpyDeviceToHost);
        (void) hipFree(d_fs);
        HIP_TRY(e);
        if (fs[0]) return fail(GLV_ERR_HIP, "window table of n=%u has no exact float-pair form on this host's cos()", n);
        t->win_shifted = fs[1];
    }
    glv::LogEntry lt[glv::kLogTabMaxSize];
    glv::make_log_table(lt);
    HIP_TRY(t->d_log.upload(lt, glv::kLogTabMaxSize));
    return GLV_OK;
}
int Tables::create(uint32_t n, int device) {
    n_ = n;
    std::lock_guard<std::mutex> lock(g_tab_mu);       // held across the creation: a second batch of the size waits instead of searching too
    for (SharedTables* t : g_tabs) if (t->device == device && t->n == n) { shared = t; break; }
    if (!shared) {
        SharedTables* t = new (std::nothrow) SharedTables();
        if (!t) return fail(GLV_ERR_NOMEM, "out of host memory");
        t->device = device; t->n = n;
        if (int rc = make_shared(t)) { delete t; return rc; }
        g_tabs.push_back(t);
        shared = t;
    }
    ++shared->refs;
    d_tw = shared->d_tw; d_win = shared->d_win; d_win_split = shared->d_win_split; d_log = shared->d_log; win_shifted = shared->win_shifted;
    return GLV_OK;
}
void Tables::destroy() {
    d_tilt.reset();
    if (shared) {
        std::lock_guard<std::mutex> lock(g_tab_mu);
        if (--shared->refs == 0) {
            for (size_t i = 0; i < g_tabs.size(); ++i) if (g_tabs[i] == shared) { g_tabs.erase(g_tabs.begin() + (long) i); break; }
            delete shared;
        }
        shared = nullptr;
    }
    d_tw = nullptr; d_win = nullptr; d_win_split = nullptr; d_log = nullptr;
}
}  // namespace glvh
namespace {
// The large state arrays (gravity store, history ring): hipMalloc -- or, for the placement experiments of profiles/r06/modes.txt (the stateful
// chains run at one of two or three speeds per PROCESS), what GLV_STATE_ALLOC asks for (read when a batch is created; diagnostics, not API):
//   vmm:<MiB>   virtual memory management: one address range, physical memory created and mapped in chunks of <MiB> MiB (0: one chunk),
//               rounded up to the device's recommended granularity
//   fine        hipExtMallocWithFlags(hipDeviceMallocFinegrained);   uncached   ... (hipDeviceMallocUncached)
struct StateAlloc {                                                             // one vmm address range and the chunks made for it so far, in address order
    void* ptr = nullptr; size_t size = 0;
    struct Chunk { hipMemGenericAllocationHandle_t handle; size_t size; bool mapped; };
    std::vector<Chunk> chunks;
};
static std::mutex g_state_mu;
static std::vector<StateAlloc> g_state_allocs;                                  // (vmm allocations only: what state_free must unmap)
// gives back whatever of `a` exists, chunk by chunk as it was mapped: state_free, and every error return of state_malloc after the reservation
void vmm_release(const StateAlloc& a) {
    char* at = static_cast<char*>(a.ptr);
    for (const StateAlloc::Chunk& c : a.chunks) {
        if (c.mapped) (void) hipMemUnmap(at, c.size);
        (void) hipMemRelease(c.handle);
        at += c.size;
    }
    (void) hipMemAddressFree(a.ptr, a.size);
}

hipError_t state_malloc(void** out, size_t bytes, int device) {
    const char* pol = std::getenv("GLV_STATE_ALLOC");
    if (!pol || !*pol || !std::strcmp(pol, "malloc")) return hipMalloc(out, bytes);
    if (!std::strcmp(pol, "fine")) return hipExtMallocWithFlags(out, bytes, hipDeviceMallocFinegrained);
    if (!std::strcmp(pol, "uncached")) return hipExtMallocWithFlags(out, bytes, hipDeviceMallocUncached);
    if (!std::strncmp(pol, "vmm:", 4)) {
        hipMemAllocationProp prop = {};
        prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = device;
        size_t gran = 0;
        hipError_t e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
        if (e != hipSuccess) return e;
        size_t chunk = (size_t) std::atol(pol + 4) << 20;
        const size_t total = (bytes + gran - 1) / gran * gran;
        if (chunk == 0 || chunk > total) chunk = total;
        chunk = (chunk + gran - 1) / gran * gran;
        StateAlloc a; a.size = total;
        if ((e = hipMemAddressReserve(&a.ptr, total, gran, nullptr, 0)) != hipSuccess) return e;
        for (size_t off = 0; off < total; off += chunk) {
            const size_t sz = off + chunk <= total ? chunk : total - off;
            hipMemGenericAllocationHandle_t h;
            if ((e = hipMemCreate(&h, sz, &prop, 0)) != hipSuccess) { vmm_release(a); return e; }
            a.chunks.push_back(StateAlloc::Chunk{h, sz, false});
            if ((e = hipMemMap(static_cast<char*>(a.ptr) + off, sz, 0, h, 0)) != hipSuccess) { vmm_release(a); return e; }
            a.chunks.back().mapped = true;
        }
        hipMemAccessDesc acc = {}; acc.location = prop.location; acc.flags = hipMemAccessFlagsProtReadWrite;
        if ((e = hipMemSetAccess(a.ptr, total, &acc, 1)) != hipSuccess) { vmm_release(a); return e; }
        *out = a.ptr;
        std::lock_guard<std::mutex> lk(g_state_mu);
        g_state_allocs.push_back(std::move(a));
        return hipSuccess;
    }
    return hipErrorInvalidValue;
}
}  // namespace
namespace glvh __attribute__((visibility("hidden"))) {
void state_free(void* p) {
    if (!p) return;
    {
        std::lock_guard<std::mutex> lk(g_state_mu);
        for (size_t i = 0; i < g_state_allocs.size(); ++i)
            if (g_state_allocs[i].ptr == p) {
                StateAlloc a = std::move(g_state_allocs[i]);
                g_state_allocs.erase(g_state_allocs.begin() + (long) i);
                vmm_release(a);
                return;
            }
    }
    (void) hipFree(p);
}

int batch_alloc(glv_batch* b) {
    const size_t n = b->p.n;
    b->state16 = b->p.gl_storage == 1;
    if ((b->ops_mask & GLV_OP_AVERAGE)) {
        HIP_TRY(state_malloc(reinterpret_cast<void**>(&b->d_hist), b->hist_bytes(), b->device));
        HIP_TRY(hipMemset(b->d_hist, 0, b->hist_bytes()));
    }
    if ((b->ops_mask & GLV_OP_GRAVITY)) {
        // kept even when the ring also exists: the single-op glv_gravity() drop-in owns its own
        // `applied` buffer exactly like the reference's separate udata slot (render.c:724)
        HIP_TRY(state_malloc(reinterpret_cast<void**>(&b->d_grav), b->grav_bytes(), b->device));
        HIP_TRY(hipMemset(b->d_grav, 0, b->grav_bytes()));
        b->grav_cur = b->d_grav;
    }
    // the device rings of the FIFO / PulseAudio modes, when the creation mask announces them
    if (b->ops_mask & GLV_OP_RING_S16) HIP_TRY(b->d_ring.alloc(2 * n * b->streams, true));          // == the calloc'd rings of glava.c:487-494
    if (b->ops_mask & GLV_OP_RING_F32) HIP_TRY(b->d_ring_f32.alloc(2 * n * b->streams, true));
    return GLV_OK;
}
}  // namespace glvh

namespace {
// ---- stream slots (glv_batch_reset_streams / _save_streams / _load_streams) ----------------------------------------------------------------------
// What a blob of this batch is now: the state arrays it owns, the element they hold, and what the calls it has run made of them.
void stream_desc(const glv_batch* b, glv_stream_state_desc* d) {
    const uint64_t n = b->p.n, elem = b->state16 ? 2u : 4u;
    std::memset(d, 0, sizeof(*d));
    d->n = b->p.n; d->avg_frames = b->p.avg_frames; d->elem_bytes = (uint32_t) elem; d->gravity_form = (uint32_t) b->grav_mode;
    d->regions = (b->d_grav ? 1u : 0u) | (b->d_hist ? 2u : 0u) | (b->d_ring ? 4u : 0u) | (b->d_ring_f32 ? 8u : 0u);
    d->kept_bins = b->kept_bins();      // (n while no live call has run; else what every live call since the last reset has kept)
    d->bytes = (b->d_grav ? 2u * n * elem : 0u) + (b->d_hist ? 2u * n * elem * b->p.avg_frames : 0u) + (b->d_ring ? 4u * n : 0u) + (b->d_ring_f32 ? 8u * n : 0u);
}
// The region table of the launch: the stream's part of each array in the portable order, rotated by the batch's positions as they are now (`rotated`;
// a reset writes zeros, which read the same at every rotation).
void stream_regions(const glv_batch* b, bool rotated, glv::SlotTable& t) {
    const uint32_t n = b->p.n, row = n * (b->state16 ? 2u : 4u), F = b->p.avg_frames;
    uint32_t k = 0, start = 0;
    auto add = [&](void* base, uint32_t stream_bytes, uint32_t chan_bytes, uint32_t unit, uint32_t pos, uint32_t mod) {
        t.r[k++] = glv::SlotRegion{static_cast<char*>(base), start, stream_bytes, chan_bytes, (uint32_t) log2_exact(unit), rotated ? pos % mod : 0u, mod};
        start += stream_bytes;
    };
    if (b->d_grav) add(b->d_grav, 2u * row, row, row, 0u, 1u);
    if (b->d_hist) add(b->d_hist, 2u * row * F, row * F, row, b->head, F);
    if (b->d_ring) add(b->d_ring.get(), 4u * n, 4u * n, 4u, b->ring_pos, n);
    if (b->d_ring_f32) add(b->d_ring_f32.get(), 8u * n, 8u * n, 8u, b->ring_pos_f32, n);
    t.nregions = k; t.bytes = start; t.streams = b->streams;
}
// what all three calls refuse; `blob`: the call moves blobs
int slots_check(const glv_batch* b, const char* entry, const uint32_t* d_idx, uint32_t count, const void* d_blob, bool blob) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!d_idx || (reinterpret_cast<uintptr_t>(d_idx) & 3u)) return fail(GLV_ERR_INVALID, "%s: d_idx is NULL or not 4-byte aligned", entry);
    if (blob && (!d_blob || (reinterpret_cast<uintptr_t>(d_blob) & 15u))) return fail(GLV_ERR_INVALID, "%s: d_blob is NULL or not 16-byte aligned", entry);
    if (count == 0) return fail(GLV_ERR_INVALID, "%s: count must be > 0", entry);
    if (b->single_row) return fail(GLV_ERR_STATE, "%s: a single-row batch (the drop-ins') has no streams to choose among", entry);
    if (b->grav_cur != b->d_grav)
        return fail(GLV_ERR_STATE, "%s: the latest gravity output of this batch lives in the caller's buffer (GLV_OP_OUTPUT_IS_STATE): the library does not own that memory", entry);
    return GLV_OK;
}
int slots_launch(glv_batch* b, int kind, const uint32_t* d_idx, uint32_t count, void* d_blob, hipStream_t st) {
    glv::SlotTable t = {};
    stream_regions(b, kind != glv::SLOT_ZERO, t);
    t.idx = d_idx; t.blob = d_blob; t.count = count;
    HIP_TRY(hipSetDevice(b->device));
    const hipError_t e = glv::launch_slots(kind, t, st);
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "stream slots launch failed: %s", hipGetErrorString(e));
    b->last_launches = 1; b->kernel_name = "glv_slots_kernel";
    return GLV_OK;
}
// Whether streams described by *d -- `what`: the blob of a load, the source batch of a copy -- can become streams of batch b, whose own descriptor is `now`;
// checked on the host before anything runs, refused in the entry's name.  *fit: what the batch adopts once the launch went through (adopt_streams).
struct StreamsFit { unsigned form_ops = 0; bool live = false; uint32_t kept = 0; };
int streams_fit(const glv_batch* b, const char* entry, const char* what, const glv_stream_state_desc* d, const glv_stream_state_desc& now, StreamsFit* fit) {
    if (d->n != now.n || d->avg_frames != now.avg_frames || d->elem_bytes != now.elem_bytes || d->regions != now.regions || d->bytes != now.bytes)
        return fail(GLV_ERR_STATE, "%s: %s (n=%u, F=%u, %u-byte elements, regions 0x%x) is not of this batch's kind (n=%u, F=%u, %u-byte elements, "
                                   "regions 0x%x)", entry, what, d->n, d->avg_frames, d->elem_bytes, d->regions, now.n, now.avg_frames, now.elem_bytes, now.regions);
    if (d->gravity_form > 2u) return fail(GLV_ERR_INVALID, "%s: gravity_form=%u: 0, 1 or 2", entry, d->gravity_form);
    // the form gravity's state is kept in: a batch keeps one (refuse_gravity_mix says why, and its words refuse the streams of the other)
    fit->form_ops = d->gravity_form == 0u ? 0u : d->gravity_form == 2u ? (unsigned) (GLV_OP_GRAVITY | GLV_OP_AVERAGE) : (unsigned) GLV_OP_GRAVITY;
    if (int rc = refuse_gravity_mix(b, fit->form_ops)) return rc;
    fit->live = d->kept_bins != now.n; fit->kept = d->kept_bins;
    if (fit->live && (!(b->ops_mask & GLV_OP_BARS_ONLY) || b->live_bins() == 0 || b->live_bins() > d->kept_bins || d->kept_bins > now.n))
        return fail(GLV_ERR_STATE, "%s: %s keeps bins [0, %u) of n=%u only (a GLV_OP_BARS_ONLY batch that has run its live class): it loads into a "
                                   "GLV_OP_BARS_ONLY batch whose glv_batch_live_bins() are no more than that (this batch: %u)", entry, what, d->kept_bins, now.n,
                    (b->ops_mask & GLV_OP_BARS_ONLY) ? b->live_bins() : 0u);
    return GLV_OK;
}
void adopt_streams(glv_batch* b, const StreamsFit& fit) {
    commit_gravity_form(b, fit.form_ops);    // (form 0: nothing to adopt)
    if (fit.live) b->ran_live_over(fit.kept);      // the batch keeps what all of its streams keep
}
}  // namespace

extern "C" {
int glv_batch_stream_state_desc(const glv_batch* b, glv_stream_state_desc* d) {
    if (!b || !d) return fail(GLV_ERR_INVALID, "glv_batch_stream_state_desc: NULL argument");
    if (b->single_row) return fail(GLV_ERR_STATE, "glv_batch_stream_state_desc: a single-row batch (the drop-ins') has no streams to choose among");
    stream_desc(b, d);
    return GLV_OK;
}

int glv_batch_reset_streams(glv_batch* b, const uint32_t* d_idx, uint32_t count, void* hip_stream) {
    if (int rc = slots_check(b, "glv_batch_reset_streams", d_idx, count, nullptr, false)) return rc;
    b->last_launches = 0;
    if (!b->d_grav && !b->d_hist && !b->d_ring && !b->d_ring_f32) return GLV_OK;      // nothing is kept per stream: every stream is a fresh one already
    return slots_launch(b, glv::SLOT_ZERO, d_idx, count, nullptr, (hipStream_t) hip_stream);
}

int glv_batch_save_streams(glv_batch* b, const uint32_t* d_idx, uint32_t count, void* d_blob, glv_stream_state_desc* d, void* hip_stream) {
    if (int rc = slots_check(b, "glv_batch_save_streams", d_idx, count, d_blob, true)) return rc;
    if (!d) return fail(GLV_ERR_INVALID, "glv_batch_save_streams: d is NULL");
    glv_stream_state_desc now;
    stream_desc(b, &now);
    if (now.regions == 0) return fail(GLV_ERR_STATE, "glv_batch_save_streams: the batch keeps neither state nor a ring (ops_mask 0x%x): a stream has nothing to save", b->ops_mask);
    if (int rc = slots_launch(b, glv::SLOT_GATHER, d_idx, count, d_blob, (hipStream_t) hip_stream)) return rc;
    *d = now;
    return GLV_OK;
}

int glv_batch_load_streams(glv_batch* b, const uint32_t* d_idx, uint32_t count, const void* d_blob, const glv_stream_state_desc* d, void* hip_stream) {
    if (int rc = slots_check(b, "glv_batch_load_streams", d_idx, count, d_blob, true)) return rc;
    if (!d) return fail(GLV_ERR_INVALID, "glv_batch_load_streams: d is NULL");
    glv_stream_state_desc now;
    stream_desc(b, &now);
    if (now.regions == 0) return fail(GLV_ERR_STATE, "glv_batch_load_streams: the batch keeps neither state nor a ring (ops_mask 0x%x): a stream has nothing to load", b->ops_mask);
    StreamsFit fit;
    if (int rc = streams_fit(b, "glv_batch_load_streams", "the blob", d, now, &fit)) return rc;
    if (int rc = slots_launch(b, glv::SLOT_SCATTER, d_idx, count, const_cast<void*>(d_blob), (hipStream_t) hip_stream)) return rc;
    adopt_streams(b, fit);
    return GLV_OK;
}

// Chosen streams from slot to slot, inside a batch or between two (include/glv_spectrum.h): the contract of save(src) + load(dst) in one launch and without the
// blob -- load's checks with the source batch's descriptor as it is now in the blob's place, then one kernel that reads every piece where src's positions put it
// and writes it where dst's do.
int glv_batch_copy_streams(glv_batch* dst, const uint32_t* d_dst_idx, glv_batch* src, const uint32_t* d_src_idx, uint32_t count, void* hip_stream) {
    static const char* const entry = "glv_batch_copy_streams";
    if (int rc = slots_check(dst, entry, d_dst_idx, count, nullptr, false)) return rc;
    if (int rc = slots_check(src, entry, d_src_idx, count, nullptr, false)) return rc;
    if (dst->device != src->device)
        return fail(GLV_ERR_INVALID, "%s: the batches live on devices %d and %d: between devices a stream travels as a blob (glv_batch_save_streams, the caller's peer copy, "
                                     "glv_batch_load_streams)", entry, src->device, dst->device);
    glv_stream_state_desc now, from;
    stream_desc(dst, &now);
    stream_desc(src, &from);
    if (now.regions == 0 && from.regions == 0)
        return fail(GLV_ERR_STATE, "%s: the batches keep neither state nor a ring (ops_mask 0x%x, 0x%x): a stream has nothing to copy", entry, src->ops_mask, dst->ops_mask);
    StreamsFit fit;
    if (int rc = streams_fit(dst, entry, "the source batch", &from, now, &fit)) return rc;
    glv::SlotTable ts = {}, td = {};
    stream_regions(src, true, ts);
    stream_regions(dst, true, td);
    ts.idx = d_src_idx; ts.count = count; td.idx = d_dst_idx; td.count = count;
    HIP_TRY(hipSetDevice(dst->device));
    const hipError_t e = glv::launch_slot_copy(ts, td, (hipStream_t) hip_stream);
    if (e != hipSuccess) return fail(GLV_ERR_HIP, "stream copy launch failed: %s", hipGetErrorString(e));
    dst->last_launches = 1; dst->kernel_name = "glv_slot_copy_kernel";
    adopt_streams(dst, fit);
    return GLV_OK;
}

// `setbufscale k` for a batch (include/glv_spectrum.h): the factor, and the staging rows a process call decimates into -- made here, by this call alone, so that
// the process and track calls stay launches only.  Like glv_batch_set_params it waits for the device first: a queued call may still read the array that goes.
// State, head, tables, bar and column texels are not touched; glv_batch_set_params and glv_batch_reset do not touch k.
int glv_batch_set_bufscale(glv_batch* b, uint32_t k) {
    if (k == 0 || k > GLV_MAX_BUFSCALE) return fail(GLV_ERR_INVALID, "glv_batch_set_bufscale: k=%u: must be in [1, %d] (1: off)", k, GLV_MAX_BUFSCALE);
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if ((uint64_t) k * b->p.n > ((uint64_t) 1 << 21))
        return fail(GLV_ERR_INVALID, "glv_batch_set_bufscale: k=%u at n=%u: a window of k * n frames holds at most 2^21", k, b->p.n);
    if (b->single_row) return fail(GLV_ERR_STATE, "glv_batch_set_bufscale: a single-row batch (the drop-ins') takes rows as they are: glv_prelude_bufscale decimates them");
    if (b->ops_mask & (GLV_OP_RING_S16 | GLV_OP_RING_F32))
        return fail(GLV_ERR_STATE, "glv_batch_set_bufscale: the batch was created with GLV_OP_RING_S16 / GLV_OP_RING_F32, whose rings hold n frames");
    if (k == b->bufscale) return GLV_OK;
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipDeviceSynchronize());
    if (k == 1u) b->d_decim.reset();
    else if (!b->d_decim) HIP_TRY(b->d_decim.alloc((size_t) b->rows * b->p.n, false));      // (on failure the owner holds what it held: nothing, and k stays 1)
    b->bufscale = k;
    return GLV_OK;
}
uint32_t glv_batch_bufscale(const glv_batch* b) { return b ? b->bufscale : 0u; }

// Placement wisdom (round 6; profiles/r06/modes.txt).  A stateful chain runs at one of two or three speeds, 7 - 14 % apart, and which one is a property of
// WHERE ITS STATE ARRAYS LIE in physical memory relative to the caller's output buffer: K batches of one process, created one after the other, each keep
// their own speed against the same buffers, and one batch changes speed with the output buffer it is given -- not with the allocator (hipMalloc, virtual
// memory management in one or many chunks, fine-grained: the same mix), not with the TLB (UTCL1 misses 3e4 of 2.8e8 requests in every mode), not with
// clocks, power or temperature.  So the library does what it does for the launch geometry: it measures.  The current placement is timed with the caller's
// real buffers, then up to `candidates` - 1 fresh allocations of the state arrays (the earlier ones stay allocated meanwhile, so every candidate lies on
// other frames); the fastest is kept, the others are freed, the state is reset.
int glv_batch_tune_placement(glv_batch* b, const int16_t* d_pcm, void* d_out, unsigned ops, int candidates, void* hip_stream, float* first_ms, float* best_ms) {
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    if (!(ops & GLV_OP_FFT) || !(ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE))) return fail(GLV_ERR_INVALID, "glv_batch_tune_placement tunes a stateful chain: ops needs GLV_OP_FFT and GLV_OP_GRAVITY / GLV_OP_AVERAGE");
    if (int rc = refuse_bufscale(b, "glv_batch_tune_placement")) return rc;
    if (int rc = check_ops(b, ops, static_cast<float*>(d_out))) return rc;
    if (!d_pcm || !d_out) return fail(GLV_ERR_INVALID, "NULL device pointer");
    if (candidates < 1) candidates = 1;
    if (candidates > 16) candidates = 16;
    hipStream_t st = (hipStream_t) hip_stream;
    HIP_TRY(hipSetDevice(b->device));
    const uint32_t units = b->streams * 2;
    const size_t hist_bytes = b->d_hist ? b->hist_bytes() : 0, grav_bytes = b->d_grav ? b->grav_bytes() : 0;
    EventPair ev; HIP_TRY(ev.create());
    const hipEvent_t e0 = ev.e0, e1 = ev.e1;
    int rc = GLV_OK;
    auto measure = [&](float* ms) -> int {
        if (int r = glv_batch_reset(b)) return r;
        for (int i = 0; i < 4; ++i) if (int r = process(b, d_pcm, glv::IN_S16_STEREO, static_cast<float*>(d_out), ops, units, 0, st)) return r;
        if (hipEventRecord(e0, st) != hipSuccess) return fail(GLV_ERR_HIP, "hipEventRecord failed");
        const int iters = 10;
        for (int i = 0; i < iters; ++i) if (int r = process(b, d_pcm, glv::IN_S16_STEREO, static_cast<float*>(d_out), ops, units, 0, st)) return r;
        if (hipEventRecord(e1, st) != hipSuccess || hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(ms, e0, e1) != hipSuccess) return fail(GLV_ERR_HIP, "event timing failed");
        *ms /= (float) iters;
        return GLV_OK;
    };
    float cur = 0.f;
    for (int i = 0; i < 24 && rc == GLV_OK; ++i) rc = process(b, d_pcm, glv::IN_S16_STEREO, static_cast<float*>(d_out), ops, units, 0, st);      // clocks up
    if (rc == GLV_OK) rc = measure(&cur);
    const float first = cur;
    std::vector<std::pair<void*, void*>> losers;                                 // (hist, grav) of the placements that lost: freed at the end
    for (int c = 1; c < candidates && rc == GLV_OK; ++c) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b < 2 * (hist_bytes + grav_bytes) + ((size_t) 1 << 30)) break;      // room for this candidate and slack
        void *nh = nullptr, *ng = nullptr;
        if (hist_bytes && state_malloc(&nh, hist_bytes, b->device) != hipSuccess) { (void) hipGetLastError(); break; }
        if (grav_bytes && state_malloc(&ng, grav_bytes, b->device) != hipSuccess) { (void) hipGetLastError(); state_free(nh); break; }
        void *oh = b->d_hist, *og = b->d_grav;
        if (nh) b->d_hist = static_cast<float*>(nh);
        if (ng) b->d_grav = static_cast<float*>(ng);
        float ms = 0.f;
        rc = measure(&ms);
        // (a candidate that lost gives its arrays back: grav_cur must not keep pointing into them -- also where measure() failed and no reset follows)
        if (rc == GLV_OK && ms < cur * 0.985f) { cur = ms; losers.emplace_back(oh, og); }
        else { b->d_hist = static_cast<float*>(oh); b->d_grav = static_cast<float*>(og); losers.emplace_back(nh, ng); b->rewind_state(); }
    }
    (void) hipStreamSynchronize(st);
    for (auto& l : losers) { state_free(l.first); state_free(l.second); }
    if (rc != GLV_OK) return rc;
    if (int r = glv_batch_reset(b)) return r;
    if (first_ms) *first_ms = first;
    if (best_ms) *best_ms = cur;
    return GLV_OK;
}

int glv_batch_window_selftest(glv_batch* b, unsigned long long* mismatches, int* shifted) {
    if (!b || !mismatches) return fail(GLV_ERR_INVALID, "glv_batch_window_selftest: NULL argument");
    HIP_TRY(hipSetDevice(b->device));
    unsigned long long* d_m = nullptr;
    HIP_TRY(hipMalloc(&d_m, sizeof(*d_m)));
    hipError_t e = hipMemset(d_m, 0, sizeof(*d_m));
    if (e == hipSuccess) e = glv::launch_window_split_check(b->tab.d_win, b->tab.d_win_split, b->p.n, d_m, nullptr);
    if (e == hipSuccess) e = hipMemcpy(mismatches, d_m, sizeof(*d_m), hipMemcpyDeviceToHost);
    (void) hipFree(d_m);
    HIP_TRY(e);
    if (shifted) *shifted = b->tab.win_shifted;
    return GLV_OK;
}
}  // extern "C"
