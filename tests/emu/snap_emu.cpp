// snap_emu.cpp -- host walk of the fused epilogue's snapped bars (glava_amd/csrc/glv_kernel_tmpl.h, bar_snap: bars at texels of the
// pre-smoothing pass), built by tests/test_snapped_bars_host.py with g++.  The tables are the library's own (glv_tables.h make_bar_taps with
// texels, make_bar_snap_weights, make_bar_items) and the arithmetic is the shared GLV_HD code of glv_frame.h (bar_item_load, bar_snap_lane_sum,
// bar_snap_texel / bar_snap_float); only the lane loop and the group reduction -- order-free integer sums -- are spelled out here.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../glava_amd/csrc/glv_tables.h"

using namespace glv;

extern "C" {

// rows: uint16 [nrows][n] GL_R16 texels; out: uint16 [nrows][bars] (r16) or float [nrows][bars].  lanes: lanes per row of the kernel
// configuration (a multiple of 64); batch: its work-list batch.  Returns 0, or -1 when the tables cannot be made / the bars do not fit.
int snapemu_bars(const uint16_t* rows, size_t nrows, uint32_t n, const uint32_t* texels, uint32_t bars, float smooth_factor, uint32_t lanes,
                 uint32_t batch, int r16, void* out) {
    std::vector<BarDesc> desc;
    std::vector<float> w;
    make_bar_taps(desc, w, n, bars, smooth_factor, 0.5f, BarShape{}, texels);
    if (!bar_chunks_in_row(desc, n)) return -1;
    std::vector<uint32_t> wi;
    if (!make_bar_snap_weights(wi, desc, w)) return -1;
    const uint32_t chunk = bar_chunk_of(n), gl = (uint32_t) bar_lanes_of(n), zero_off = (uint32_t) wi.size();
    wi.resize(wi.size() + chunk, 0u);
    if (bars + 1 > 2 * lanes) return -1;
    const uint32_t G = lanes / gl;
    std::vector<BarItem> items;
    const uint32_t nsteps = make_bar_items(items, desc, G, zero_off, chunk, batch);
    // the slot's LDS region: the row as floats c / 65535 and the slack behind it
    std::vector<float> region(n + 2 * lanes, 0.0f);
    std::vector<float> wf(wi.size());
    memcpy(wf.data(), wi.data(), sizeof(uint32_t) * wi.size());                   // the weights travel as float bits, as on the device
    for (size_t r = 0; r < nrows; ++r) {
        for (uint32_t i = 0; i < n; ++i) region[i] = unorm16_to_float(rows[r * n + i]);
        for (uint32_t i = n; i < n + 2 * lanes; ++i) region[i] = __builtin_nanf("");   // whatever the slack held: never a tap of weight != 0
        uint32_t* lout = reinterpret_cast<uint32_t*>(region.data() + n);
        for (uint32_t g = 0; g < G; ++g) {
            uint64_t total = 0;
            for (uint32_t s = 0; s < nsteps; ++s) {
                const BarItem& it = items[(size_t) s * G + g];
                uint64_t chunk_sum = 0;
                for (uint32_t sub = 0; sub < gl; ++sub) chunk_sum += bar_snap_lane_sum(bar_item_load<false>(region.data(), wf.data(), it, (int) sub));
                total = it.keep != 0.0f ? total + chunk_sum : chunk_sum;
                lout[it.res] = r16 ? bar_snap_texel(total) : __builtin_bit_cast(uint32_t, bar_snap_float(total));
            }
        }
        for (uint32_t k = 0; k < bars; ++k) {
            if (r16) static_cast<uint16_t*>(out)[r * bars + k] = (uint16_t) lout[k];
            else static_cast<float*>(out)[r * bars + k] = __builtin_bit_cast(float, lout[k]) / desc[k].weight_sum;
        }
    }
    return 0;
}

// every 16-bit texel c survives the row's float c / 65535 and the epilogue's conversion back (pack_unorm16, host form): the number that do not
int snapemu_texel_roundtrip_failures(void) {
    int bad = 0;
    for (uint32_t c = 0; c < 65536u; c += 2) {
        const uint32_t p = pack_unorm16(unorm16_to_float(c), unorm16_to_float(c + 1));
        bad += (p & 0xffffu) != c;
        bad += (p >> 16) != c + 1;
    }
    return bad;
}

}  // extern "C"
