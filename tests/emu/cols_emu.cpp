// cols_emu.cpp -- host walk of the columns of glv_batch_set_column_texels (means of three texels of the pre-smoothing pass), built by
// tests/test_column_texels_host.py with g++ -ffp-contract=off: the fused epilogue's step (glava_amd/csrc/glv_kernel_tmpl.h, kernel classes
// FC_GL16_COLS*: the snapped loop over the distinct texels, kept as 16-bit values behind the row, then one column per lane) and the row loop of the
// second launch (glv_bars.hip glv_columns_kernel, sample_mode average).  The tables are the library's own (glv_tables.h) and the arithmetic is the
// shared GLV_HD code of glv_frame.h (bar_item_load, bar_snap_lane_sum, bar_snap_texel, column_mean); only the lane loops, the order-free integer
// group reduction and the de-duplication (glv_bar_tables.cpp set_snap_texels) are spelled out here.
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../glava_amd/csrc/glv_tables.h"

using namespace glv;

extern "C" {

// rows: uint16 [nrows][n] GL_R16 texels; table: [cols][3] left, middle, right; out: float [nrows][cols].  lanes != 0: the fused epilogue of a kernel
// configuration with that many lanes per row (a multiple of 64) and work-list batch `batch`; lanes == 0: the second launch (256 lanes, kBarBatch).
// Returns 0, -1 when the tables cannot be made, -2 when the distinct texels do not fit behind the row.
int colsemu_columns(const uint16_t* rows, size_t nrows, uint32_t n, const uint32_t* table, uint32_t cols, float smooth_factor, uint32_t lanes,
                    uint32_t batch, float* out) {
    std::vector<uint32_t> tex(table, table + (size_t) cols * 3);
    std::sort(tex.begin(), tex.end());
    tex.erase(std::unique(tex.begin(), tex.end()), tex.end());
    const uint32_t ntex = (uint32_t) tex.size();
    std::vector<ColumnMap> map(cols);
    for (uint32_t x = 0; x < cols; ++x) {
        auto at = [&](uint32_t t) { return (uint16_t) (std::lower_bound(tex.begin(), tex.end(), t) - tex.begin()); };
        map[x] = ColumnMap{at(table[3 * x]), at(table[3 * x + 1]), at(table[3 * x + 2]), 0};
    }
    std::vector<BarDesc> desc;
    std::vector<float> w;
    make_bar_taps(desc, w, n, ntex, smooth_factor, 0.5f, BarShape{}, tex.data());
    if (!bar_chunks_in_row(desc, n)) return -1;
    std::vector<uint32_t> wi;
    if (!make_bar_snap_weights(wi, desc, w)) return -1;
    const uint32_t chunk = bar_chunk_of(n), gl = (uint32_t) bar_lanes_of(n), zero_off = (uint32_t) wi.size();
    wi.resize(wi.size() + chunk, 0u);
    const bool fused = lanes != 0;
    if (fused && ntex + 1 > 4 * lanes) return -2;
    const uint32_t G = (fused ? lanes : 256u) / gl;
    std::vector<BarItem> items;
    const uint32_t nsteps = make_bar_items(items, desc, G, zero_off, chunk, fused ? batch : (uint32_t) kBarBatch);
    const uint32_t slack = fused ? 2 * lanes : 0;                                   // floats behind the row (the fused kernel's exchange region)
    std::vector<float> region(n + slack, 0.0f);
    std::vector<uint16_t> own(ntex + 2, 0xdeadu);                                   // the second launch's LDS array
    std::vector<float> wf(wi.size());
    memcpy(wf.data(), wi.data(), sizeof(uint32_t) * wi.size());                     // the weights travel as float bits, as on the device
    for (size_t r = 0; r < nrows; ++r) {
        for (uint32_t i = 0; i < n; ++i) region[i] = unorm16_to_float(rows[r * n + i]);
        for (uint32_t i = n; i < n + slack; ++i) region[i] = __builtin_nanf("");
        uint16_t* ltex = fused ? reinterpret_cast<uint16_t*>(region.data() + n) : own.data();
        for (uint32_t g = 0; g < G; ++g) {
            uint64_t total = 0;
            for (uint32_t s = 0; s < nsteps; ++s) {
                const BarItem& it = items[(size_t) s * G + g];
                uint64_t chunk_sum = 0;
                for (uint32_t sub = 0; sub < gl; ++sub)
                    chunk_sum += fused ? bar_snap_lane_sum(bar_item_load<false>(region.data(), wf.data(), it, (int) sub))
                                       : bar_snap_lane_sum(bar_item_load<true>(region.data(), wf.data(), it, (int) sub));
                total = it.keep != 0.0f ? total + chunk_sum : chunk_sum;
                if (it.res > ntex) return -3;
                ltex[it.res] = (uint16_t) bar_snap_texel(total);
            }
        }
        for (uint32_t x = 0; x < cols; ++x) out[r * cols + x] = column_mean(ltex[map[x].l], ltex[map[x].m], ltex[map[x].r]);
    }
    return 0;
}

// column_mean alone, on given texels (the contract formula as the kernels evaluate it)
void colsemu_mean(const uint16_t* l, const uint16_t* m, const uint16_t* r, size_t count, float* out) {
    for (size_t i = 0; i < count; ++i) out[i] = column_mean(l[i], m[i], r[i]);
}

}  // extern "C"
