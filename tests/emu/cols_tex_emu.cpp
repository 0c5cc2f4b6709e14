// cols_tex_emu.cpp -- host walk of the row loop of glv_columns_kernel (glava_amd/csrc/glv_bars.hip) in both of its kinds, built by
// tests/test_track_columns_host.py with g++ -ffp-contract=off: float rows c / 65535 (a process call's second launch) and texel rows (the third launch of
// glv_batch_track_columns_s16 / _f32), for the three sample modes.  The tables are the library's own
// (glv_tables.h), the arithmetic is the shared GLV_HD code of glv_frame.h (bar_item_load, bar_snap_lane_sum, bar_item_texel_sum, bar_snap_texel,
// column_mean) and glv_core.h (unorm16, unorm16_to_float); only the lane loops, the order-free integer group reduction and the de-duplication
// (glv_bar_tables.cpp) are spelled out here.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../glava_amd/csrc/glv_tables.h"

using namespace glv;

namespace {
struct ColumnTables {
    std::vector<uint32_t> tex;
    std::vector<ColumnMap> map;
    std::vector<BarDesc> desc;
    std::vector<float> w;
};
void make_column_tables(ColumnTables& t, uint32_t n, const uint32_t* table, uint32_t cols, float smooth_factor, uint32_t mode) {
    t.tex.assign(table, table + (size_t) cols * 3);
    std::sort(t.tex.begin(), t.tex.end());
    t.tex.erase(std::unique(t.tex.begin(), t.tex.end()), t.tex.end());
    t.map.resize(cols);
    for (uint32_t x = 0; x < cols; ++x) {
        auto at = [&](uint32_t v) { return (uint16_t) (std::lower_bound(t.tex.begin(), t.tex.end(), v) - t.tex.begin()); };
        t.map[x] = ColumnMap{at(table[3 * x]), at(table[3 * x + 1]), at(table[3 * x + 2]), 0};
    }
    BarShape shape;
    shape.inclusive = mode == 0;                                                    // (glv_bar_tables.cpp bar_shape)
    make_bar_taps(t.desc, t.w, n, (uint32_t) t.tex.size(), smooth_factor, 0.5f, shape, t.tex.data());
}
}  // namespace

extern "C" {

// rows: uint16 [nrows][n] GL_R16 texels; table: [cols][3]; out: float [nrows][cols].  texel_rows != 0: the texel-row kind, else the float kind on rows
// c / 65535.  mode: sample_mode 0 / 1 / 2.  Returns 0, -1 when the tables cannot be made, -3 on a work-list result outside the texel array.
int colstex_columns(const uint16_t* rows, size_t nrows, uint32_t n, const uint32_t* table, uint32_t cols, float smooth_factor, uint32_t mode, float hybrid_weight,
                    int texel_rows, float* out) {
    ColumnTables t;
    make_column_tables(t, n, table, cols, smooth_factor, mode);
    const uint32_t ntex = (uint32_t) t.tex.size();
    if (!bar_chunks_in_row(t.desc, n)) return -1;
    const uint32_t chunk = bar_chunk_of(n), gl = (uint32_t) bar_lanes_of(n), G = 256u / gl;
    std::vector<BarItem> items;
    std::vector<float> wf;
    uint32_t nsteps = 0;
    if (mode == 0) {
        std::vector<uint32_t> wi;
        if (!make_bar_snap_weights(wi, t.desc, t.w)) return -1;
        const uint32_t zero_off = (uint32_t) wi.size();
        wi.resize(wi.size() + chunk, 0u);
        nsteps = make_bar_items(items, t.desc, G, zero_off, chunk, (uint32_t) kBarBatch);
        wf.resize(wi.size());
        memcpy(wf.data(), wi.data(), sizeof(uint32_t) * wi.size());                 // the weights travel as float bits, as on the device
    }
    const float h = hybrid_weight, omh = 1.0f - hybrid_weight;
    std::vector<uint16_t> ltex(ntex + 2, 0xdeadu);
    std::vector<float> frow(n);
    for (size_t r = 0; r < nrows; ++r) {
        const uint16_t* trow = rows + r * n;
        for (uint32_t i = 0; i < n; ++i) frow[i] = unorm16_to_float(trow[i]);
        if (mode == 0) {
            for (uint32_t g = 0; g < G; ++g) {
                uint64_t total = 0;
                for (uint32_t s = 0; s < nsteps; ++s) {
                    const BarItem& it = items[(size_t) s * G + g];
                    uint64_t chunk_sum = 0;
                    for (uint32_t sub = 0; sub < gl; ++sub)
                        chunk_sum += texel_rows ? bar_item_texel_sum(trow, wf.data(), it, (int) sub)
                                                : bar_snap_lane_sum(bar_item_load<true>(frow.data(), wf.data(), it, (int) sub));
                    total = it.keep != 0.0f ? total + chunk_sum : chunk_sum;
                    if (it.res > ntex) return -3;
                    ltex[it.res] = (uint16_t) bar_snap_texel(total);
                }
            }
        } else {
            for (uint32_t k = 0; k < ntex; ++k) {
                const BarDesc d = t.desc[k];
                if (d.first_bin + d.count > n) return -3;
                float vmax = 0.0f, avg = 0.0f;
                for (uint32_t j = 0; j < d.count; ++j) {
                    float x = texel_rows ? unorm16_to_float(trow[d.first_bin + j]) : frow[d.first_bin + j];
                    x = x > 0.0f ? (x < 1.0f ? x : 1.0f) : 0.0f;
                    const float v = x * t.w[d.tap_offset + j];
                    vmax = vmax < v ? v : vmax;
                    if (mode == 2) avg = avg + v;
                }
                float v = vmax;
                if (mode == 2) v = (vmax * omh) + ((avg / d.weight_sum) * h);
                ltex[k] = (uint16_t) unorm16(v);
            }
        }
        for (uint32_t x = 0; x < cols; ++x) out[r * cols + x] = column_mean(ltex[t.map[x].l], ltex[t.map[x].m], ltex[t.map[x].r]);
    }
    return 0;
}

}  // extern "C"
