// live_kept_emu.cpp -- the kept-bins rule of glv_batch_track_live_s16 / _f32 on the host tables (glv_tables.h bar_chunk_reach, track_kept_bins) beside the
// work lists the chunked float bars run off.  Built by tests/test_track_live_host.py with g++ -ffp-contract=off; no device.
#include <cstdint>
#include <vector>

#include "../../glava_amd/csrc/glv_frame.h"
#include "../../glava_amd/csrc/glv_tables.h"

using namespace glv;

extern "C" {
// The kept-bins rule on the host tables of `bars` bars of a row of n bins (the shipped shape: sinusoidal, scale 8, range 0.9, averaging): returns K for
// the chunked float bars; *live = the bins the bars sample in whole 64s (what glv_batch_live_bins reports where the chain has a live class), *reach =
// the largest first_bin + chunk over the work-list items of glv_bars_kernel (padding items excluded), measured on the items themselves.
uint32_t live_emu_kept(uint32_t n, uint32_t bars, float smooth_factor, float phase, uint32_t* live, uint32_t* reach) {
    std::vector<BarDesc> desc;
    std::vector<float> w;
    make_bar_taps(desc, w, n, bars, smooth_factor, phase, BarShape{0u, 8.0f, 0.9f, true});
    uint32_t sampled = 0;
    for (const BarDesc& d : desc) sampled = d.first_bin + d.count > sampled ? d.first_bin + d.count : sampled;
    *live = (sampled + 63u) & ~63u;
    const uint32_t zero_off = (uint32_t) w.size(), chunk = bar_chunk_of(n);
    std::vector<BarItem> items;
    make_bar_items(items, desc, 256u / (uint32_t) bar_lanes_of(n), zero_off, chunk);
    *reach = 0;
    for (const BarItem& it : items)
        if (it.w_byte != zero_off * 4u && it.tex_byte / 4u + chunk > *reach) *reach = it.tex_byte / 4u + chunk;
    return track_kept_bins(*live, bar_chunk_reach(desc, chunk));
}

// The bins `bars` bars of a row of n bins sample, in whole 64s, under a shape (sinusoidal, averaging; scale / range as glv_params sample_scale / sample_range
// reach the tables): what glv_batch_live_bins reports where the chain has a live class for that many (tests/test_live_bins_changes_host.py pins the ladder
// tests/test_live_bins_changes.py climbs).
uint32_t live_emu_sampled(uint32_t n, uint32_t bars, float smooth_factor, float phase, float scale, float range) {
    std::vector<BarDesc> desc;
    std::vector<float> w;
    make_bar_taps(desc, w, n, bars, smooth_factor, phase, BarShape{0u, scale, range, true});
    uint32_t sampled = 0;
    for (const BarDesc& d : desc) sampled = d.first_bin + d.count > sampled ? d.first_bin + d.count : sampled;
    return (sampled + 63u) & ~63u;
}
}
