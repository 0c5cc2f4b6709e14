// glv_bar_tables.cpp -- the tables made on the host and uploaded when a batch is created or its parameters are set: GLV_OP_BARS taps, weights and
// work lists, the bars and columns at texels of the pre-smoothing pass, GLV_OP_SMOOTH's window bounds, the internal rows.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "glv_host.h"
#include "glv_tables.h"       // the host-side table generators (make_*), kBarSeqMin

namespace {
glv::BarShape bar_shape(const glv_params& p) { return glv::BarShape{p.round_formula, shape_scale(p), shape_range(p), p.sample_mode == GLV_SAMPLE_AVERAGE}; }

// bins of a row a tap table reaches: the largest first_bin + count, in whole 64s (whole store instructions, the ring fill's 16-byte loads); 0: no taps
uint32_t bins_reached(const std::vector<glv::BarDesc>& desc) {
    uint32_t reach = 0;
    for (const glv::BarDesc& d : desc) reach = d.first_bin + d.count > reach ? d.first_bin + d.count : reach;
    return (reach + 63u) & ~63u;
}

// the integer tables of a pass over texel rows for the smallest LDS ring that takes them (glv_launch.h kRowsI8Rings: the rings the kernel is
// built for); returns that ring, 0 (irounds empty) when none does
uint32_t make_itiles_any_ring(std::vector<glv::BarMTile>& itiles, std::vector<int8_t>& wq, std::vector<glv::BarIFin>& fin, std::vector<glv::BarTile>& irounds,
                              const std::vector<glv::BarDesc>& desc, const std::vector<float>& w, uint32_t n) {
    for (uint32_t bins : glv::kRowsI8Rings) {
        if (!glv::make_bar_itiles(itiles, wq, fin, irounds, desc, w, n, bins, (uint32_t) glv::kRowsWaves)) { irounds.clear(); break; }
        if (!irounds.empty()) return bins;
    }
    irounds.clear();
    return 0;
}

// For each kernel configuration of the size: may it compute the results of `desc` inside the frame kernel, behind the finished row in LDS -- whole
// waves per row, one exchange region, and room(lanes): the results and the dump slot fit the slack behind the row -- and if so its work list (the
// configurations' lanes per row differ), made and uploaded.  zero_off: the chunk of zero weights the padding items point at.
template <class Room>
int upload_fused_items(const glv_batch* b, BarTableSet& s, const std::vector<glv::BarDesc>& desc, uint32_t zero_off, Room room) {
    const uint32_t chunk = glv::bar_chunk_of(b->p.n), gl = (uint32_t) glv::bar_lanes_of(b->p.n);
    const int nv = glv::frame_variants(b->log_nn);
    for (int v = 0; v < nv && v < kMaxVariants; ++v) {
        const glv::FrameGeometry geo = glv::frame_geometry(b->log_nn, v);
        s.fusable[v] = geo.lanes % 64 == 0 && geo.nbuf == 1 && room((uint32_t) geo.lanes);
        if (!s.fusable[v]) continue;
        std::vector<glv::BarItem> fitems;
        s.fnsteps[v] = glv::make_bar_items(fitems, desc, (uint32_t) geo.lanes / gl, zero_off, chunk, (uint32_t) geo.bar_batch);
        HIP_TRY(s.fitems[v].upload(fitems));
    }
    return GLV_OK;
}

// glv_batch_set_column_texels: the most distinct texels the frame kernel's epilogue takes; more go to the second launch (glv_columns_kernel).
// Measured at N = 4096, 64 K streams (profiles/r08/column_texels.txt): 321 texels fused 1.61 ms, the second launch 2.10 ms, the twin plus a gather 2.09 ms --
// and the second launch loses to the twin from there up (801 texels 4.08 against 3.23 ms), so whatever fits behind the row is fused: the bound is the room
// of the widest configuration (4 x 256 lanes), not a crossover.  801 texels fused (N = 16384, 256 lanes) is tested but not timed.
constexpr uint32_t kColumnsFuseMax = 1023;

// The tables of bars at texels `tex` of the pre-smoothing pass (glv_batch_set_bar_texels; glv_tables.h make_bar_snap_weights), made in `s` / `x`:
// every check, then the uploads, and the batch's own tables are not touched -- the caller commits them (commit_snap_tables) or, by returning, does
// not: a refused or failed table leaves the batch as it was.  (The internal rows a second launch needs are the one thing made in the batch, after
// everything else went through; a batch may always hold them.)  Synchronous; creation / set calls only.
// columns (glv_batch_set_column_texels): `tex` are the distinct texels the columns read -- bars = their number, not glv_params.bars.
int build_snap_tables(glv_batch* b, const std::vector<uint32_t>& tex, bool columns, BarTableSet& s, SnapExtras& x) {
    const uint32_t n = b->p.n, bars = (uint32_t) tex.size();
    const bool averaging = b->p.sample_mode == GLV_SAMPLE_AVERAGE;
    const glv::BarShape shape = bar_shape(b->p);
    if (averaging) {
        // the twin's texels must be the exact integer means (GLV_BARS_I8_EXACT): its integer tables have to exist
        if (b->bar_i8_off) return fail(GLV_ERR_INVALID, "bar texels: GLV_NO_BARS_I8 is set, so the pre-smoothing pass runs GLV_BARS_F32_MATRIX, which snapped bars do not reproduce");
        std::vector<glv::BarDesc> td;
        std::vector<float> tw;
        glv::make_bar_taps(td, tw, n, n, b->p.smooth_factor, 0.5f, shape);
        std::vector<glv::BarMTile> itiles;
        std::vector<glv::BarTile> irounds;
        std::vector<int8_t> wq;
        std::vector<glv::BarIFin> fin;
        if (!glv::bar_chunks_in_row(td, n) || make_itiles_any_ring(itiles, wq, fin, irounds, td, tw, n) == 0)
            return fail(GLV_ERR_INVALID, "bar texels: the pre-smoothing pass of these parameters (n=%u smooth_factor=%g) has no integer tables (a bar wider than the largest "
                                         "LDS ring, or more than 2^31 in its weight scale): its arithmetic is GLV_BARS_F32_MATRIX, which snapped bars do not reproduce", n, (double) b->p.smooth_factor);
    }
    std::vector<glv::BarDesc> desc;
    std::vector<float> w;
    glv::make_bar_taps(desc, w, n, bars, b->p.smooth_factor, 0.5f, shape, tex.data());
    if (!glv::bar_chunks_in_row(desc, n)) return fail(GLV_ERR_INVALID, "bar texels: a tap chunk would leave the row (n=%u smooth_factor=%g)", n, (double) b->p.smooth_factor);
    s.bins = bins_reached(desc);
    if (s.bins == 0) s.bins = 64u;
    if (averaging) {
        std::vector<uint32_t> wi;
        if (!glv::make_bar_snap_weights(wi, desc, w)) return fail(GLV_ERR_INVALID, "bar texels: a bar's integer weights do not exist for these parameters");
        const uint32_t zero_off = (uint32_t) wi.size(), chunk = glv::bar_chunk_of(n), gl = (uint32_t) glv::bar_lanes_of(n);
        wi.resize(wi.size() + chunk, 0u);
        HIP_TRY(s.w.upload(reinterpret_cast<const float*>(wi.data()), wi.size()));      // (the uint32 weights W' travel as the bits of float weights)
        // every result is 4 bytes behind the row, as the unsnapped totals: bars + the dump slot in the 2 * lanes floats of slack
        // (columns keep 16-bit texels there: twice as many.  kColumnsFuseMax: beyond it the second launch is the quicker route)
        if (int rc = upload_fused_items(b, s, desc, zero_off, [&](uint32_t lanes) { return columns ? bars + 1 <= 4 * lanes && bars <= kColumnsFuseMax : bars + 1 <= 2 * lanes; })) return rc;
        if (columns) {
            std::vector<glv::BarItem> citems;
            x.col_nsteps = glv::make_bar_items(citems, desc, 256u / gl, zero_off, chunk, (uint32_t) glv::kBarBatch);
            HIP_TRY(x.col_items.upload(citems));
        }
    } else if (columns) {
        if (w.empty()) w.push_back(0.0f);
        HIP_TRY(s.w.upload(w));                                  // glv_columns_kernel MODE 1 / 2: the float weights in tap order
    } else {
        std::vector<glv::BarModeBlock> blocks;
        std::vector<float> mw;
        glv::make_bar_mode_blocks(blocks, mw, desc, w);
        if (mw.empty()) mw.push_back(0.0f);
        HIP_TRY(s.mblocks.upload(blocks));
        HIP_TRY(s.mw.upload(mw));
        s.nmblocks = (uint32_t) blocks.size();
    }
    HIP_TRY(s.desc.upload(desc));
    x.tex = tex; x.of = b->p;
    // a second launch needs the chain's rows
    return bars_need_rows(b, s) ? ensure_scratch(b) : GLV_OK;
}
void commit_snap_tables(glv_batch* b, BarTableSet& s, SnapExtras& x) {
    b->snap = std::move(s); b->snap_x = std::move(x);
    b->update_live_bins();
}
}  // namespace
namespace glvh __attribute__((visibility("hidden"))) {
// what launch_bars takes besides the taps: the many-bars tiles (the bars of glv_params only) and the maximum / hybrid blocks of the set `s`
glv::BarRowsTables rows_tables(const glv_params& p, const BarExtras& x, const BarTableSet& s) {
    glv::BarRowsTables t{x.mtiles, x.ntiles, x.wt, x.wsum, x.rounds, x.nrounds, x.ring_bins};
    t.mode = p.sample_mode; t.hybrid_weight = shape_hybrid(p);
    t.mblocks = s.mblocks; t.nmblocks = s.nmblocks; t.mw = s.mw; t.mode_bins = s.bins < p.n ? s.bins : p.n;
    return t;
}

int ensure_smooth_tables(glv_batch* b) {
    if (b->d_smin && b->smooth_d == b->p.smooth_distance && b->smooth_r == b->p.smooth_ratio) return GLV_OK;
    if (!(b->p.smooth_ratio >= 1.0f)) return fail(GLV_ERR_INVALID, "smooth_ratio must be >= 1");
    const size_t n = b->p.n;
    std::vector<int> lo(n), hi(n);
    const size_t asz = glv::make_smooth_bounds(lo.data(), hi.data(), n, b->p.smooth_distance, b->p.smooth_ratio);
    if (!b->d_smin) {                          // n entries each, of which asz are read; both or neither
        DeviceArray<int> smin, smax;
        HIP_TRY(smin.upload(lo));
        HIP_TRY(smax.upload(hi));
        b->d_smin = std::move(smin); b->d_smax = std::move(smax);
    } else {                                   // (rewritten where they are, as the tilt factors)
        HIP_TRY(hipMemcpy(b->d_smin, lo.data(), sizeof(int) * asz, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(b->d_smax, hi.data(), sizeof(int) * asz, hipMemcpyHostToDevice));
    }
    size_t reach = asz;
    long window = 1;
    for (size_t t = 0; t < asz; ++t) {
        if ((size_t) hi[t] + 1 > reach) reach = (size_t) hi[t] + 1;
        // the span the ring must keep around step t: from the first tap (or t itself) to the last tap (or t itself)
        const long a = lo[t] < (long) t ? lo[t] : (long) t, z = hi[t] > (long) t ? hi[t] : (long) t;
        if (z - a + 1 > window) window = z - a + 1;
    }
    b->smooth_window = (uint32_t) window;
    b->smooth_reach = (uint32_t) (reach < n ? reach : n);
    b->smooth_asz = (uint32_t) asz; b->smooth_d = b->p.smooth_distance; b->smooth_r = b->p.smooth_ratio;
    return GLV_OK;
}

// GLV_OP_BARS tables: taps, weights, the work lists of glv_bars_kernel and one fused work list per kernel configuration of the
// size (their lanes per row differ).  Host generation + synchronous upload: creation / glv_batch_set_params only.
// Built in a local set that replaces the batch's as the last step: a refused or failed call leaves the batch exactly as it was.  For the length of
// the call the old and the new tables exist together (kilobytes to a few megabytes, beside state arrays of the streams' size).
int ensure_bar_tables(glv_batch* b) {
    const bool averaging = b->p.sample_mode == GLV_SAMPLE_AVERAGE;                                       // maximum / hybrid: glv_bars_mode_kernel, no matrix-core / fused form
    const bool want_i8 = b->p.gl_storage != 0 && b->p.bars >= glv::kBarSeqMin && !b->bar_i8_off && averaging;      // chains whose rows are texels
    if (b->bar.desc && b->bar_x.count == b->p.bars && b->bar_x.factor == b->p.smooth_factor && b->bar_x.phase == b->p.bar_phase && same_shape(b->bar_x.shape_of, b->p)
        && (want_i8 == (b->bar_x.itiles.get() != nullptr) || b->bar_x.i8_none)) return GLV_OK;
    if (b->p.bars == 0 || b->p.bars > b->p.n) return fail(GLV_ERR_INVALID, "bars=%u out of range", b->p.bars);
    {   // the shape: scale_audio(1) = -log(1 - SAMPLE_RANGE) / SAMPLE_SCALE is the last position smooth_audio() samples (a share of the row)
        const float sc = shape_scale(b->p), rg = shape_range(b->p), hw = shape_hybrid(b->p);
        if (!(sc > 0.0f && sc <= 1e6f) || !(rg > 0.0f && rg < 1.0f) || !(-logf(1.0f - rg) / sc <= 1.0f))
            return fail(GLV_ERR_INVALID, "sample_scale=%g sample_range=%g: need scale > 0, 0 < range < 1 and -log(1 - range) / scale <= 1 (smooth_audio() would fetch texels beyond the texture)", (double) sc, (double) rg);
        if (!(hw > 0.0f && hw <= 1.0f)) return fail(GLV_ERR_INVALID, "sample_hybrid_weight=%g: must be in (0, 1]", (double) hw);
    }
    if (!(b->p.smooth_factor >= 0.0f && b->p.smooth_factor <= 1.0f))       // also rejects NaN
        return fail(GLV_ERR_INVALID, "smooth_factor=%g: must be in [0, 1] (a bar would have no taps)", (double) b->p.smooth_factor);
    if (!(b->p.bar_phase >= 0.0f && b->p.bar_phase < 1.0f)) return fail(GLV_ERR_INVALID, "bar_phase=%g: must be in [0, 1)", (double) b->p.bar_phase);
    std::vector<glv::BarDesc> desc;
    std::vector<float> w;
    glv::make_bar_taps(desc, w, b->p.n, b->p.bars, b->p.smooth_factor, b->p.bar_phase, bar_shape(b->p));
    if (!glv::bar_chunks_in_row(desc, b->p.n)) return fail(GLV_ERR_INVALID, "bars: a tap chunk would leave the row (n=%u smooth_factor=%g)", b->p.n, (double) b->p.smooth_factor);
    BarTableSet s;
    BarExtras x;
    // work lists: 256 / GL groups per row for glv_bars_kernel; T / GL groups for the frame kernel (GL = bar_lanes_of(n); fused bars:
    // whole waves per row, fewer than 2 * lanes bars).  one chunk of zero weights appended for padding items.
    const uint32_t zero_off = (uint32_t) w.size();
    const uint32_t chunk = glv::bar_chunk_of(b->p.n), gl = (uint32_t) glv::bar_lanes_of(b->p.n);
    w.resize(w.size() + chunk, 0.0f);
    std::vector<glv::BarItem> items;
    x.nsteps = glv::make_bar_items(items, desc, 256 / gl, zero_off, chunk);
    x.chunk_reach = glv::bar_chunk_reach(desc, chunk);
    HIP_TRY(x.items.upload(items));
    // bar totals + the dump slot fit the 2 * lanes floats of slack behind the row in LDS
    // (from 256 bars up a bar is one fma chain, glv_tables.h make_bar_mtiles: the chunked loop of the epilogue does not apply)
    if (int rc = upload_fused_items(b, s, desc, zero_off, [&](uint32_t lanes) { return b->p.bars + 1 <= 2 * lanes && b->p.bars < glv::kBarSeqMin && averaging; })) return rc;
    HIP_TRY(s.desc.upload(desc));
    HIP_TRY(s.w.upload(w));
    x.count = b->p.bars; x.factor = b->p.smooth_factor; x.phase = b->p.bar_phase; x.shape_of = b->p;
    s.bins = bins_reached(desc);
    if (!averaging) {                          // sample_mode maximum / hybrid: one lane per bar and row off block-transposed weights, any number of bars
        std::vector<glv::BarModeBlock> blocks;
        std::vector<float> mw;
        glv::make_bar_mode_blocks(blocks, mw, desc, w);
        if (mw.empty()) mw.push_back(0.0f);
        HIP_TRY(s.mblocks.upload(blocks));
        HIP_TRY(s.mw.upload(mw));
        s.nmblocks = (uint32_t) blocks.size();
        if (s.bins == 0) s.bins = 64u;                                             // (no bar has a tap: every bar is 0, or 0 / 0 in the hybrid)
        x.bins_needed = s.bins;                                                    // what a transform in front of the bars has to store of a row
    } else if (b->p.bars >= glv::kBarSeqMin) {
        // many bars (the pre-smoothing pass): tiles of 32 bars for the chain kernels; rounds for the smallest LDS ring that takes them
        std::vector<glv::BarMTile> mtiles;
        std::vector<glv::BarTile> rounds;
        std::vector<float> wt, wsum;
        for (uint32_t bins : glv::kRowsRings) {
            if (!glv::make_bar_mtiles(mtiles, wt, wsum, rounds, desc, w, b->p.n, bins, (uint32_t) glv::kRowsWaves))
                return fail(GLV_ERR_INVALID, "bars: no tile table (bars=%u)", b->p.bars);
            if (!rounds.empty()) { x.ring_bins = bins; break; }
        }
        if (std::getenv("GLV_NO_BARS_ROWS")) rounds.clear();                        // (diagnostics: the one-lane-per-bar kernel for every row count)
        HIP_TRY(x.mtiles.upload(mtiles));
        HIP_TRY(x.wt.upload(wt));
        HIP_TRY(x.wsum.upload(wsum));
        x.ntiles = (uint32_t) mtiles.size();
        x.bins_needed = bins_reached(desc);
        if (!rounds.empty()) {
            HIP_TRY(x.rounds.upload(rounds));
            x.nrounds = (uint32_t) rounds.size();
            const glv::BarRowsTables rt = rows_tables(b->p, x, s);
            HIP_TRY(glv::prepare_bars_rows(b->p.n, &rt));
        }
        // texel rows: the integer tables, for the smallest ring that takes them
        if (want_i8) {
            std::vector<glv::BarMTile> itiles;
            std::vector<glv::BarTile> irounds;
            std::vector<int8_t> wq;
            std::vector<glv::BarIFin> fin;
            x.iring_bins = make_itiles_any_ring(itiles, wq, fin, irounds, desc, w, b->p.n);
            if (irounds.empty()) x.i8_none = true;
            else {
                HIP_TRY(x.itiles.upload(itiles));
                HIP_TRY(x.wq.upload(wq));
                HIP_TRY(x.fin.upload(fin));
                HIP_TRY(x.irounds.upload(irounds));
                x.intiles = (uint32_t) itiles.size(); x.inrounds = (uint32_t) irounds.size();
                const glv::BarIRowsTables irt = x.irows_tables();
                HIP_TRY(glv::prepare_bars_i8(b->p.n, &irt));
            }
        }
    }
    b->bar = std::move(s); b->bar_x = std::move(x);
    b->update_live_bins();
    return GLV_OK;
}

// the internal rows ([rows][n] floats): whatever of a chain does not stay inside one launch waits there for the next
int ensure_scratch(glv_batch* b) {
    if (!b->d_scratch) HIP_TRY(b->d_scratch.alloc((size_t) b->rows * b->p.n, false));
    return GLV_OK;
}

// the snapped tables follow smooth_factor and the shape (glv_batch_set_params; bar_phase does not enter them)
bool snap_current(const glv_batch* b) {
    return b->snap.desc && b->snap_x.of.bars == b->p.bars && same_bits(b->snap_x.of.smooth_factor, b->p.smooth_factor) && same_shape(b->snap_x.of, b->p);
}
int ensure_snap_tables(glv_batch* b) {
    if (!b->snapped() || snap_current(b)) return GLV_OK;
    BarTableSet s;
    SnapExtras x;
    if (int rc = build_snap_tables(b, b->snap_x.tex, b->columns(), s, x)) return rc;
    x.col_tex = std::move(b->snap_x.col_tex); x.col_map = std::move(b->snap_x.col_map);       // the columns' map follows the texels, not the parameters
    commit_snap_tables(b, s, x);
    return GLV_OK;
}

// Can the bars of a chain -- or of every chain a creation mask announces -- be computed inside the frame kernel, from the finished row in LDS?
// The part that does not depend on the kernel configuration (BarTableSet::fusable[variant]: whole-wave rows, the bars fit the slack behind the row):
// a chain with state and no smoothing pass, whose kernel class takes them -- the float chain's bars as GL_R16 texels leave through
// glv_bars_kernel, the GL_R16 chain stores them itself, the GL passes one by one (gl_storage 2, the audit log) never fuse; GLV_UNFUSED_BARS
// (diagnostics) forces two launches.  process() adds that the chain transforms (GLV_OP_FFT) and is not run pass by pass (GLV_OP_RAW).
// gl_storage 3: snapped tables only (bar texels and columns, kernel classes FC_STATE_SNAP / FC_STATE_COLS: the finished float row in LDS is sampled through
// the upload's quantiser, results as texels or floats); its unsnapped bars are the integer pass or glv_bars_mode_kernel, always a second launch.
bool bars_fusable(const glv_batch* b, unsigned ops) {
    return (ops & (GLV_OP_GRAVITY | GLV_OP_AVERAGE)) && !(ops & GLV_OP_SMOOTH) && !b->unfused_bars
           && (b->p.gl_storage == 0 ? !(ops & GLV_OP_R16) : upload_storage(b->p) ? b->snapped() : b->p.gl_storage == 1 && b->p.log_mode != 2);
}
// Do the bars of table set `s` need the internal rows -- true unless every chain the creation mask announces fuses them in every kernel
// configuration.  One difference from process(): under the audit log (log_mode 2) a float chain fuses its bars and gets the rows all the
// same -- which batches hold them is kept as it was.
bool bars_need_rows(const glv_batch* b, const BarTableSet& s) {
    if (upload_storage(b->p)) return true;            // (its unsnapped bars and its stateless chains always take two launches)
    bool all_fused = bars_fusable(b, b->ops_mask) && b->p.log_mode != 2;
    for (int v = 0; v < glv::frame_variants(b->log_nn) && v < kMaxVariants; ++v) all_fused = all_fused && s.fusable[v];
    return !all_fused;
}
}  // namespace glvh

extern "C" {
// glv_batch_set_bar_texels (width 1) and glv_batch_set_column_texels (width 3: left, middle, right) share everything but the table's shape
static int set_snap_texels(glv_batch* b, const uint32_t* texels, uint32_t count, uint32_t width) {
    const bool cols = width == 3;
    const char* what = cols ? "column texels" : "bar texels";
    if (!b) return fail(GLV_ERR_INVALID, "batch is NULL");
    HIP_TRY(hipSetDevice(b->device));
    // the old tables are freed: every kernel already queued on the device must have read them first (as glv_batch_set_params)
    HIP_TRY(hipDeviceSynchronize());
    if (texels == nullptr || count == 0) {                 // off: the unsnapped tables, untouched meanwhile, serve again
        if (b->snapped() && b->columns() != cols) return GLV_OK;      // (the other kind of table is set: this kind is off already)
        // (the unsnapped bars sample what they sampled: the live bins stay or shrink -- the one check of every change all the same)
        if (!b->keeps_live(b->live_bins_with(0u)))
            return fail(GLV_ERR_STATE, "%s: without the table the bars sample beyond the bins this GLV_OP_BARS_ONLY batch has kept -- glv_batch_reset first", what);
        b->snap = BarTableSet(); b->snap_x = SnapExtras();
        b->update_live_bins();
        return GLV_OK;
    }
    if (b->snapped() && b->columns() != cols)
        return fail(GLV_ERR_STATE, "%s: %s are set on this batch -- the two tables exclude each other, clear the other one first", what, cols ? "bar texels" : "column texels");
    if (!(b->ops_mask & GLV_OP_BARS) || !b->bar.desc)
        return fail(GLV_ERR_STATE, "%s: the batch was created without GLV_OP_BARS (or has no bar tables)", what);
    if (b->p.gl_storage == 0)
        return fail(GLV_ERR_STATE, "%s: gl_storage 0 -- a float chain has no pre-smoothed texture to sample", what);
    if (count != b->p.bars) return fail(GLV_ERR_INVALID, "%s: %u entries for bars=%u", what, count, b->p.bars);
    for (uint32_t k = 0; k < count * width; ++k)
        if (texels[k] >= b->p.n) return fail(GLV_ERR_INVALID, "%s: t[%u] = %u is not a texel of the n=%u pass", what, k, texels[k], b->p.n);
    std::vector<uint32_t> tex(texels, texels + (size_t) count * width);
    std::vector<glv::ColumnMap> map;
    if (cols) {                                            // the distinct texels, sorted, and where each column's three sit among them
        std::sort(tex.begin(), tex.end());
        tex.erase(std::unique(tex.begin(), tex.end()), tex.end());
        // glv_columns_kernel keeps them (and a dump slot) as 16-bit values in the 64 KiB of LDS a launch may ask for without an attribute
        if (tex.size() > 32766u) return fail(GLV_ERR_INVALID, "column texels: %zu distinct texels, at most 32766", tex.size());
        map.resize(count);
        for (uint32_t x = 0; x < count; ++x) {
            auto at = [&](uint32_t t) { return (uint16_t) (std::lower_bound(tex.begin(), tex.end(), t) - tex.begin()); };
            map[x] = glv::ColumnMap{at(texels[3 * x]), at(texels[3 * x + 1]), at(texels[3 * x + 2]), 0};
        }
    }
    // built beside the batch's tables and committed as the last step: whatever refuses or fails before leaves the batch exactly as it was
    BarTableSet set;
    SnapExtras extras;
    if (int rc = build_snap_tables(b, tex, cols, set, extras)) return rc;
    // (as glv_batch_set_params: a GLV_OP_BARS_ONLY batch that ran its live class cannot start sampling beyond the bins it kept)
    if (!b->keeps_live(b->live_bins_with(set.bins)))
        return fail(GLV_ERR_STATE, "%s: these taps reach beyond the bins this GLV_OP_BARS_ONLY batch has kept -- glv_batch_reset first", what);
    if (cols) {
        HIP_TRY(extras.col_map.upload(map));
        extras.col_tex.assign(texels, texels + (size_t) count * 3);
    }
    commit_snap_tables(b, set, extras);
    return GLV_OK;
}
int glv_batch_set_bar_texels(glv_batch* b, const uint32_t* texels, uint32_t count) { return set_snap_texels(b, texels, count, 1); }
int glv_batch_set_column_texels(glv_batch* b, const uint32_t* texels, uint32_t count) { return set_snap_texels(b, texels, count, 3); }
}  // extern "C"
