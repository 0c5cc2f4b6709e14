// glv_kernel_tmpl.h -- the gfx950 (CDNA4, wave64) frame kernel template and its launcher.
//
//   glv_frame_kernel   PCM (or planar f32) -> unpack -> window -> nn-point FFT -> abs/log/tilt
//                      -> gravity -> average in ONE launch; spectra never leave registers/LDS
//                      between stages.  Replaces transform_fft/gravity/average
//                      (glava/render.c:720-847) and the unpack loop of glava/fifo.c:94-110.
//
// Execution shape: T = nn/E lanes cooperate on one FFT ("slot"), SLOTS slots per workgroup;
// every lane owns E = 8/16/32 complex points and performs up to log2(E) radix-2 stages on them in registers
// between LDS exchanges (ds_write2_b64 / ds_read2_b64 / ds_read_b128; the pass-0 layout is padded by one
// point per E).  HBM traffic is the algorithmic minimum: PCM in (8 B per lane per load, lanes contiguous),
// spectra out (16 B per lane, lanes contiguous), state in/out.  Workgroups are persistent over a
// grid-stride list of frames so per-lane twiddles and tilt factors can stay in VGPRs.
//
// No MFMA: the path is a bandwidth/LDS/VALU problem, not a dense contraction.
//
// Tuning knobs (template parameters; production picks one set per size in glv_inst.hip,
// tools/tune.py sweeps them through glv_tune.hip):
//   LOG_E   log2 of the points a lane owns (4: E=16, T=nn/16 lanes per row; 3: E=8, T=nn/8; 5: E=32, T=nn/32)
//   SLOTS   FFT slots per workgroup
//   NBUF    1: one LDS exchange region per slot, two barriers per exchange
//           2: ping-pong regions, one barrier per exchange
//           0: SPLIT exchange -- one half-size region per slot, the row crosses it one float component at a time (real
//              parts, then imaginary parts: glv_frame.h exchange_write_half), four barriers per exchange.  Halves the
//              LDS a row in flight needs, which is what lets the sizes whose tables do not fit beside two full
//              regions (N=16384: 65 KiB of twiddles) keep them in LDS (TWREG 4) with two rows per CU
//   TWREG   1 (true): passes >= 1 keep their per-lane twiddles in VGPRs across frames
//           0 (false): gathered from the (L2-resident) table at every pass
//           2: middle passes gather from an LDS copy of their table range (entries E-1 .. L0_last-2: 8 KiB
//              for N=16384 at 32 points per lane), the last pass from the L2-resident table
//           3: middle passes from LDS, the last pass resident in VGPRs
//           4: every pass >= 1 from an LDS copy of the table (nn - E entries: 16 KiB at N=4096) -- no twiddle
//              VGPRs; allows 3 waves/SIMD at N=4096 (6 slots), measured slower than 2 (tools/tune.py)
//   WINLDS  true: window table staged once per workgroup into LDS; false: read through L1/L2
//   OCC     __launch_bounds__ minimum waves per SIMD (caps the VGPR budget: 512 / OCC)
//   TILTREG   0: tilt factors re-read from the table per row; 1: the 2E per-lane factors stay in VGPRs across
//             rows; 2: evaluated in registers with the reference's float operations (no memory, no registers)
//             3: log_mode 1: the folded factor tilt * ln2/3 from a per-lane base term and ONE fused multiply-add + max per value
//                (glv_core.h tilt_lin: <= 4.5e-7 from the reference's own rounded factor, contract 1e-5); other log modes as 2
//   PREFETCH  0: no software pipeline (load, transform, store per row)
//           1: in-place pipeline -- the next frame's (s16, interleaved f32) or row's (planar f32) samples
//              are requested before the current row's passes and unpacked/windowed after its epilogue,
//              straight into the point registers.  (Earlier variants that unpacked into a second point
//              set before the epilogue, per frame or per row, measured slower at every size and are gone;
//              profiles/tune_r01.txt still lists them as pf=1 / pf=2, this one as pf=3.)
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "glv_frame.h"

namespace glv {

// ---- slot-scoped synchronisation --------------------------------------------------------------------
// The slots of a workgroup transform independent rows; nothing but the read-only tables is shared between
// them, so an exchange only has to order the waves of ONE slot:
//   * T <= 64: the slot lives inside one wave and LDS executes a wave's instructions in order -- no
//     hardware barrier at all, only a compiler fence;
//   * one slot per workgroup: s_barrier is already slot-scoped;
//   * otherwise (N=4096: two waves per slot, two slots): a counter in LDS per slot.  Lane 0 of every wave
//     adds 1 (ordered behind the wave's own LDS writes), then the wave polls until all T/64 waves of the
//     slot arrived.  A workgroup-wide s_barrier here would keep the two slots in lockstep -- the same
//     coupling that makes 4 slots per workgroup slower than 2.
template <int T, int SLOTS>
struct SlotSync {
    static constexpr bool WAVE_LOCAL = T <= 64 && (64 % T) == 0;
    static constexpr bool WORKGROUP = !WAVE_LOCAL && SLOTS == 1;
    static constexpr bool COUNTER = !WAVE_LOCAL && !WORKGROUP;
    static constexpr uint32_t WAVES = T / 64 > 0 ? T / 64 : 1;
    uint32_t* counter = nullptr;     // LDS, one per slot (COUNTER mode)
    uint32_t expected = 0;
    __device__ __forceinline__ void sync() {
        if constexpr (WAVE_LOCAL) {
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        } else if constexpr (WORKGROUP) {
            __syncthreads();
        } else {
            expected += WAVES;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            while (__hip_atomic_load(counter, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < expected) __builtin_amdgcn_s_sleep(1);
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        }
    }
};

// UNIT_SHORTCUT: pass 0 evaluates its (1, +0) twiddles as a +- b (s16 input only, glv_core.h SubPass::run)
template <int LOG_NN, int LOG_E, int NBUF, int TWREG, bool UNIT_SHORTCUT = true>
struct Body {
    using FR = Frame<LOG_NN, LOG_E>;
    static constexpr int P = FR::P, NN = FR::NN, N = FR::N, T = FR::T;

    // where the per-lane twiddles of pass Q (>= 1) come from
    static constexpr bool TW_LDS_MODE = (TWREG == 4 && P >= 2) || (TWREG >= 2 && P >= 3);
    static constexpr bool is_mid(int q) { return q >= 1 && q < P - 1; }
    static constexpr bool from_lds(int q) { return TW_LDS_MODE && (is_mid(q) || (TWREG == 4 && q >= 1)); }
    static constexpr bool resident(int q) { return q >= 1 && (TWREG == 1 || (TWREG >= 2 && !TW_LDS_MODE) || (TWREG == 3 && q == P - 1)); }
    // LDS copy: table entries [LDS_BIAS, LDS_BIAS + LDS_ENTRIES) = the stages of passes 1..P-2 (TWREG 2, 3)
    // or of every pass >= 1 (TWREG 4: the whole table but pass 0's E-1 entries)
    static constexpr int LDS_BIAS = tw_offset(FR::E);
    static constexpr int LDS_ENTRIES = !TW_LDS_MODE ? 0 : TWREG == 4 ? NN - FR::E : (1 << FR::PL::log_l0(P - 1)) - FR::E;

    template <int PASS>
    static constexpr int tw_off() {
        if constexpr (PASS == 0) return 0;
        else return tw_off<PASS - 1>() + FR::template PassInfo<PASS - 1>::NTW;
    }
    static constexpr int TW_TOTAL = tw_off<P>();

    template <int PASS>
    static __device__ __forceinline__ cf (&tw_ref(cf* all))[FR::template PassInfo<PASS>::NTW] {
        return *reinterpret_cast<cf(*)[FR::template PassInfo<PASS>::NTW]>(all + tw_off<PASS>());
    }

    // pass-0 twiddles: wave-uniform by construction; readfirstlane pins them into SGPRs
    static __device__ __forceinline__ void gather_uniform_tw0(cf* all, const cf* __restrict__ table) {
        cf (&t0)[FR::template PassInfo<0>::NTW] = tw_ref<0>(all);
        FR::template gather_tw<0>(t0, table, 0);
#pragma unroll
        for (int i = 0; i < FR::template PassInfo<0>::NTW; ++i) {
            t0[i].x = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t0[i].x)));
            t0[i].y = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, t0[i].y)));
        }
    }

    // once per kernel: the passes whose twiddles stay in VGPRs
    template <int PASS>
    static __device__ __forceinline__ void gather_resident(cf* all, const cf* __restrict__ table, int tid) {
        if constexpr (resident(PASS)) FR::template gather_tw<PASS>(tw_ref<PASS>(all), table, tid);
        if constexpr (PASS + 1 < P) gather_resident<PASS + 1>(all, table, tid);
    }
    // per row: the twiddles of a non-resident pass, from the LDS copy or the L2-resident table
    template <int PASS>
    static __device__ __forceinline__ void gather_transient(cf* all, const cf* __restrict__ table, const cf* lds_tw, int tid) {
        if constexpr (from_lds(PASS)) FR::template gather_tw<PASS, LDS_BIAS>(tw_ref<PASS>(all), lds_tw, tid);
        else if constexpr (!resident(PASS)) FR::template gather_tw<PASS>(tw_ref<PASS>(all), table, tid);
    }

    // passes PASS..P-1 on the 16 register-resident points; `xcount` counts exchanges so the
    // ping-pong region alternates consistently across channels and frames.  Scheduling fences
    // pin the phase order  compute | LDS write + next twiddle gather | barrier | LDS read | compute
    // so that the backend cannot pull the table loads of later passes (30 VGPRs each) up front.
    template <int PASS, typename SYNC>
    static __device__ __forceinline__ void run(cf (&v)[FR::E], cf* tw_all, const cf* __restrict__ table,
                                               char* xslot, int tid, unsigned& xcount, const cf* lds_tw, SYNC& sy) {
        // pass 0's twiddles are the same for every lane (k0 = 0); the kernel gathers them once, before
        // the row loop, into scalar registers (gather_uniform_tw0) -- a vector load here would sit in
        // front of every row's first butterfly AND, vmcnt being in-order, behind the PCM prefetch.
        FR::template compute<PASS, UNIT_SHORTCUT>(v, tw_ref<PASS>(tw_all));
        if constexpr (PASS + 1 < P) {
            char* xb = xslot + (NBUF == 2 ? (size_t) (xcount & 1u) * FR::XREGION * sizeof(cf) : 0);
            GLV_SCHED_FENCE();
            if constexpr (NBUF == 0) {
                // split exchange: real parts, then imaginary parts, through the one half-size region
                sy.sync();                                  // previous readers of the region are done
                FR::template exchange_write_half<PASS, 0>(xb, v, tid);
                gather_transient<PASS + 1>(tw_all, table, lds_tw, tid);
                sy.sync();
                FR::template exchange_read_half<PASS + 1, 0>(v, xb, tid);
                GLV_SCHED_FENCE();
                sy.sync();                                  // every real part has been read
                FR::template exchange_write_half<PASS, 1>(xb, v, tid);
                sy.sync();
                FR::template exchange_read_half<PASS + 1, 1>(v, xb, tid);
            } else {
            if constexpr (NBUF == 1) sy.sync();         // previous readers of the region are done
            FR::template exchange_write<PASS>(xb, v, tid);
            // the next pass's per-lane twiddles travel from L2 while the exchange settles
            gather_transient<PASS + 1>(tw_all, table, lds_tw, tid);
            sy.sync();
            FR::template exchange_read<PASS + 1>(v, xb, tid);
            }
            GLV_SCHED_FENCE();
            ++xcount;
            run<PASS + 1>(v, tw_all, table, xslot, tid, xcount, lds_tw, sy);
        }
    }
};

// dynamic LDS of one workgroup: exchange regions | window (WINLDS) | log table | middle-pass twiddles (TWREG >= 2) |
// one 16-byte cell per slot for the slot barrier counter
template <int LOG_NN, int LOG_E, int SLOTS, int NBUF, bool WINLDS, int TWREG = 0>
constexpr size_t frame_lds_bytes() {
    return (size_t) SLOTS * (NBUF == 0 ? sizeof(float) : NBUF * sizeof(cf)) * Frame<LOG_NN, LOG_E>::XREGION + (WINLDS ? (size_t) Frame<LOG_NN, LOG_E>::N * sizeof(double) : 0)
           + ((size_t) sizeof(LogEntry) << log_tab_bits_of(LOG_NN)) + (size_t) Body<LOG_NN, LOG_E, NBUF, TWREG>::LDS_ENTRIES * sizeof(cf) + (size_t) 16 * SLOTS;
}

// wave-uniform value -> SGPR (valid when all lanes of the wave hold the same value)
template <bool UNIFORM>
static __device__ __forceinline__ uint32_t maybe_scalar(uint32_t v) {
    if constexpr (UNIFORM) return (uint32_t) __builtin_amdgcn_readfirstlane((int) v);
    else return v;
}

// a pool call's span of stream s (glv_frame.h TrackSpan): one 16-byte load from global memory (the address travels as an integer: say so, or the load is a flat one)
static __device__ __forceinline__ TrackSpan load_track_span(const TrackSpan* spans, uint32_t s) {
    typedef uint32_t span_u4 __attribute__((ext_vector_type(4)));
    const span_u4 v = *(const __attribute__((address_space(1))) span_u4*) (reinterpret_cast<uintptr_t>(spans) + (uintptr_t) s * sizeof(TrackSpan));
    return TrackSpan{ (uint64_t) v.x | (uint64_t) v.y << 32, v.z, v.w };
}

template <int LOG_NN, int IN_KIND, int LOG_MODE, int SLOTS, int NBUF, int TWREG, bool WINLDS, int OCC, int PREFETCH, int TILTREG,
          int LOG_E, int STATEFUL, int WPRE = 0>
__global__ void __launch_bounds__((Frame<LOG_NN, LOG_E>::T * SLOTS), OCC)
glv_frame_kernel(const FrameArgs a) {
    using FR = Frame<LOG_NN, LOG_E>;
    constexpr int E = FR::E;
    constexpr int T = FR::T, N = FR::N;
    // a per-stream table kind (glv_frame.h in_track_each) is its shared-table sibling in everything but the entry it reads (track_entry below): the pipeline is
    // picked by IN_MODE, the sibling's kind, and every other kind is its own IN_MODE
    // a pool kind (in_track_pool: glv_batch_track_pool_*) likewise, and it reads its entry as the per-stream kinds do; what differs is track_at, through the stream's span
    constexpr int IN_MODE = track_pool_shared_kind(IN_KIND);
    constexpr bool TRACK_POOL = in_track_pool(IN_KIND);
    constexpr bool TRACK_EACH = in_track_each(IN_KIND) || TRACK_POOL;
    constexpr bool RING = IN_MODE == IN_S16_RING;
    constexpr bool TRACK_TABLE = in_track_table(IN_MODE);   // a table call's kinds: the window's start comes from a.trk.starts (track_entry / track_at below)
    constexpr bool TRACK = IN_MODE == IN_S16_TRACK || IN_MODE == IN_S16_TRACK_AT;    // windows where they lie in a recording (a.trk): never a ring, stateless classes only (launch_variant)
    constexpr bool TRACKF = IN_MODE == IN_F32_TRACK || IN_MODE == IN_F32_TRACK_AT;   // the same over interleaved stereo f32 recordings: the f32 stereo pipeline and generic loop, another address per frame
    constexpr bool TRACKP = IN_MODE == IN_F32_PLANAR_TRACK_AT;                       // the same over planar float recordings, a table kind only: the planar pipeline over rows and the generic loop, another address per row
    constexpr bool S16 = IN_MODE == IN_S16_STEREO || RING || TRACK;
    constexpr bool WSPLIT = S16 && win_split_of(LOG_NN, STATEFUL);     // s16 samples: the window product without fp64 (glv_core.h apply_window_split)
    // f32 rows may hold -0.0, Inf and NaN: no unit-twiddle shortcut, non-finite values through the bit-faithful log
    constexpr bool NF = !S16;
    using BD = Body<LOG_NN, LOG_E, NBUF, TWREG, S16>;
    constexpr bool WAVE_SLOT = (T % 64) == 0;      // a wave never straddles two slots
    constexpr size_t XBYTES = (size_t) FR::XREGION * (NBUF == 0 ? sizeof(float) : sizeof(cf));     // NBUF 0: split exchange, half-size region
    constexpr int NREG = NBUF == 0 ? 1 : NBUF;                                                         // regions per slot

    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NTHREADS = T * SLOTS;
    const uint32_t slot = maybe_scalar<WAVE_SLOT>(threadIdx.x / T);
    const int tid = (int) (threadIdx.x % T);
    char* xslot = smem + (size_t) slot * NREG * XBYTES;

    const void* gwin = WSPLIT ? a.win_split : static_cast<const void*>(a.win);     // 16 bytes per complex point either way
    const void* win = gwin;
    if constexpr (WINLDS) {
        char* lwin = smem + (size_t) SLOTS * NREG * XBYTES;
        for (int i = threadIdx.x; i < N / 2; i += NTHREADS) st<d2>(lwin, (uint32_t) i * 16u, ld<d2>(gwin, (uint32_t) i * 16u));
        __syncthreads();
        win = lwin;
    }

    // log_mode 0: the 256- or 512-entry (1/c, log(c)/3) table is gathered per value; LDS serves such random
    // 16-byte reads without touching the vector-memory path the PCM/spectrum streams use.
    const LogEntry* logtab = a.logtab;
    if constexpr (LOG_MODE == 0) {
        char* llog = smem + (size_t) SLOTS * NREG * XBYTES + (WINLDS ? (size_t) N * sizeof(double) : 0);
        constexpr int LB = log_tab_bits_of(LOG_NN);             // entries this size uses: every 2^(9 - LB)-th of the table in HBM
        for (int i = threadIdx.x; i < (1 << LB); i += NTHREADS) st<d2>(llog, (uint32_t) i * 16u, ld<d2>(a.logtab, (uint32_t) (i << (kLogTabMaxBits - LB)) * 16u));
        __syncthreads();
        logtab = reinterpret_cast<const LogEntry*>(llog);
    }

    // TWREG >= 2: the twiddle table range of the middle passes is staged into LDS once per workgroup
    const cf* lds_tw = nullptr;
    if constexpr (BD::TW_LDS_MODE) {
        char* ltw = smem + (size_t) SLOTS * NREG * XBYTES + (WINLDS ? (size_t) N * sizeof(double) : 0) + ((size_t) sizeof(LogEntry) << log_tab_bits_of(LOG_NN));
        for (int i = threadIdx.x; i < BD::LDS_ENTRIES; i += NTHREADS) st<cf>(ltw, (uint32_t) i * 8u, ld<cf>(a.tw, (uint32_t) (BD::LDS_BIAS + i) * 8u));
        __syncthreads();
        lds_tw = reinterpret_cast<const cf*>(ltw);
    }

    // slot-scoped synchronisation state (a counter per slot at the end of the LDS allocation)
    SlotSync<T, SLOTS> sy;
    if constexpr (SlotSync<T, SLOTS>::COUNTER) {
        uint32_t* ctr = reinterpret_cast<uint32_t*>(smem + frame_lds_bytes<LOG_NN, LOG_E, SLOTS, NBUF, WINLDS, TWREG>() - 16 * SLOTS) + 4 * slot;
        if (tid == 0) { ctr[0] = 0; ctr[1] = 0; ctr[2] = 0; }
        __syncthreads();
        sy.counter = ctr;
    }

    cf tw_all[BD::TW_TOTAL];
    BD::gather_uniform_tw0(tw_all, a.tw);
    if constexpr (FR::P > 1) BD::template gather_resident<1>(tw_all, a.tw, tid);
    cf tilt_reg[TILTREG == 1 ? E : 1];
    if constexpr (TILTREG == 1) FR::gather_tilt(tilt_reg, a.tilt, tid);
    if constexpr (TILTREG == 3) {
        // the lane part of every output index of the last pass: out_index(tid, gi, r) - out_index(0, gi, r) (the same for all gi, r)
        const int lane_q = FR::template out_index<FR::P - 1>(tid, 0, 0) - FR::template out_index<FR::P - 1>(0, 0, 0);
        tilt_reg[0].x = tilt_lin_base(tilt_lin(a.inv_n, a.fft_scale, a.one_minus_cutoff), 2 * lane_q);
        tilt_reg[0].y = 0.0f;
    }

    // operator chain, uniform for the launch; the kernel class (STATEFUL, glv_frame.h FrameClass) fixes everything else
    const bool raw_out = (a.ops & OP_RAW) != 0;
    constexpr bool FUSED_BARS = fc_fused_bars(STATEFUL);
    constexpr bool GL16 = fc_gl16(STATEFUL);
    constexpr bool GL16_LIVE = GL16 && fc_live(STATEFUL);
    constexpr bool F32_LIVE = !GL16 && fc_live(STATEFUL);
    constexpr bool HAS_STATE = fc_has_state(STATEFUL);
    constexpr bool TEXELS = fc_texel_out(STATEFUL);
    static_assert(!FUSED_BARS || WAVE_SLOT, "fused bars need whole waves per row");
    static_assert(!GL16 || LOG_MODE != 2, "the GL_R16 chain is built for log modes 0 and 1");
    static_assert(!FUSED_BARS || NBUF == 1, "fused bars park the finished row in exchange region 0: needs the full-size, two-barrier region");
    // FC_GL16_LIVE in the s16 frame pipeline: the row's old state is requested before its transform (glv_frame.h gl16_state_prefetch)
    constexpr bool LIVE_PRE = GL16_LIVE && FR::LIVE_PREFETCH && S16 && PREFETCH == 1;
    typename FR::LivePre live_pre;
    const typename FR::LivePre* live_pre_ptr = nullptr;
    auto finish = [&](const cf (&v)[E], size_t row, int tid) {
        // a.out == nullptr (gravity without average only): the spectra ARE the gravity state
        // (render.c:733-734 stores the same value to both), so the second copy is not written
        float* out_row = FUSED_BARS ? reinterpret_cast<float*>(xslot)
                                               : (HAS_STATE && a.out == nullptr ? nullptr : a.out + row * N);
        if constexpr (GL16) {
            float* o = FUSED_BARS ? reinterpret_cast<float*>(xslot)
                                  : ((a.ops & OP_R16) ? reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(a.out) + row * N) : a.out + row * N);
            FR::template epilogue_gl16<LOG_MODE, TILTREG, NF, FUSED_BARS, GL16_LIVE>(v, o, row, tid, a, logtab, tilt_reg, live_pre_ptr);
        } else if constexpr (TEXELS && HAS_STATE) {
            float* out16 = reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(a.out) + row * N);
            if (raw_out) FR::template epilogue<LOG_MODE, EPI_RAW_STATE, 0, true, NF>(v, out16, row, tid, a, logtab);
            else FR::template epilogue<LOG_MODE, EPI_MAG_STATE, TILTREG, true, NF>(v, out16, row, tid, a, logtab, tilt_reg);
        } else if constexpr (F32_LIVE) {
            FR::template epilogue<LOG_MODE, EPI_MAG_STATE, TILTREG, false, NF, true>(v, out_row, row, tid, a, logtab, tilt_reg);
        } else if constexpr (HAS_STATE) {
            if (raw_out) FR::template epilogue<LOG_MODE, EPI_RAW_STATE, 0, false, NF>(v, out_row, row, tid, a, logtab);
            else FR::template epilogue<LOG_MODE, EPI_MAG_STATE, TILTREG, false, NF>(v, out_row, row, tid, a, logtab, tilt_reg);
        } else if constexpr (TEXELS) {
            float* out16 = reinterpret_cast<float*>(reinterpret_cast<uint16_t*>(a.out) + row * N);
            if (raw_out) FR::template epilogue<LOG_MODE, EPI_RAW, 0, true, NF>(v, out16, row, tid, a, logtab);
            else FR::template epilogue<LOG_MODE, EPI_MAG, TILTREG, true, NF>(v, out16, row, tid, a, logtab, tilt_reg);
        } else {
            if (raw_out) FR::template epilogue<LOG_MODE, EPI_RAW, 0, false, NF>(v, out_row, row, tid, a, logtab);
            else FR::template epilogue<LOG_MODE, EPI_MAG, TILTREG, false, NF>(v, out_row, row, tid, a, logtab, tilt_reg);
        }
    };
    // FUSED_BARS: lane k of a slot stores bar k (and k + T, ... when bars > T): the first one's weight sum stays in a register
    float bar_wsum = 1.0f;
    if constexpr (FUSED_BARS && !fc_cols(STATEFUL)) { if ((uint32_t) tid < a.bars) bar_wsum = a.bar_desc[tid].weight_sum; }
    // the epilogue of one row; every lane of the workgroup calls it (barriers inside when FUSED_BARS)
    auto finish_row = [&](const cf (&v)[E], size_t row, int tid, bool active) {
        if constexpr (FUSED_BARS) {
            sy.sync();                                     // every reader of the row's last exchange is done
            if (active) finish(v, row, tid);               // finished row -> LDS, natural order
            sy.sync();
            // T/GL groups of GL = 2 / 4 / 8 lanes work through the row's bar chunks (glv_frame.h "GLV_OP_BARS
            // arithmetic"; work lists from make_bar_items).  BB = bar_batch_of(LOG_NN) steps at a time: their loads (LDS
            // row + L2-resident weights) are issued together and the next batch's items are fetched
            // while the current one is reduced.  No global store inside the loop (vmcnt is one in-order
            // counter): every step stores its running total to the slack behind the row -- slot `res` is the
            // bar a chunk completes, or the dump slot lres[bars] -- and after a barrier the slot's lanes
            // divide by the weight sums and store the bars coalesced.
            constexpr int GL = bar_lanes_of((uint32_t) N);                    // lanes per group: 2 / 4 / 8
            constexpr uint32_t G = T / GL;
            constexpr int BB = bar_batch_of(LOG_NN);
            float* lrow = reinterpret_cast<float*>(xslot);
            float* lres = lrow + N;                                       // XREGION has NN/E points (2T floats) of slack: bars + 1 <= 2T (glv_api.cpp bar_fusable)
            static_assert(2 * T >= 64, "the chunk reads of bar_item_load stay inside the slot's region");
            constexpr bool snap = fc_snap(STATEFUL);
            // columns (glv_batch_set_column_texels): the snapped loop over the DISTINCT texels the columns read, kept as 16-bit texels -- 2 bytes
            // each in the same slack, (texels + 1) <= 4T -- and after the barrier lane x stores the mean of column x's three (column_mean)
            constexpr bool cols = fc_cols(STATEFUL);
            if (active && snap) {
                // bars at texels of the pre-smoothing pass (glv_frame.h bar_snap_lane_sum): the same work lists, exact 64-bit integer sums, and
                // each step's result is already the bar's -- texel or float bits -- so the slack behind the row takes 4 bytes per bar as above
                const int sub = tid & (GL - 1);
                const uint32_t g = (uint32_t) tid / GL;
                const BarItem* items = a.bar_items + g;
                uint32_t* lout = reinterpret_cast<uint32_t*>(lres);
                const bool r16 = a.bars_r16 != 0;
                BarItem it[BB];
#pragma unroll
                for (int b = 0; b < BB; ++b) it[b] = items[(size_t) b * G];
                uint64_t total = 0;
                for (uint32_t s0 = 0; s0 < a.bar_nsteps; s0 += BB) {
                    BarTaps tp[BB];
                    BarItem nx[BB];
#pragma unroll
                    for (int b = 0; b < BB; ++b) tp[b] = bar_item_load<false>(lrow, a.bar_w, it[b], sub);
#pragma unroll
                    for (int b = 0; b < BB; ++b) nx[b] = items[(size_t) (s0 + BB + b) * G];
                    if constexpr (BB <= kBarBatch) GLV_SCHED_FENCE();
#pragma unroll
                    for (int b = 0; b < BB; ++b) {
                        const uint64_t chunk_sum = group_sum64<GL>(bar_snap_lane_sum(tp[b]));
                        total = it[b].keep != 0.0f ? total + chunk_sum : chunk_sum;
                        if constexpr (cols) { if (sub == 0) reinterpret_cast<uint16_t*>(lres)[it[b].res] = (uint16_t) bar_snap_texel(total); }
                        else if (sub == 0) lout[it[b].res] = r16 ? bar_snap_texel(total) : __builtin_bit_cast(uint32_t, bar_snap_float(total));
                    }
#pragma unroll
                    for (int b = 0; b < BB; ++b) it[b] = nx[b];
                }
            } else if (active) {
                const int sub = tid & (GL - 1);
                const uint32_t g = (uint32_t) tid / GL;
                const BarItem* items = a.bar_items + g;
                BarItem it[BB];
#pragma unroll
                for (int b = 0; b < BB; ++b) it[b] = items[(size_t) b * G];
                float total = 0.0f;
                for (uint32_t s0 = 0; s0 < a.bar_nsteps; s0 += BB) {
                    BarTaps tp[BB];
                    BarItem nx[BB];
                    // (taps read from LDS step by step, only the weights held for the batch, would let ten steps fit the
                    // registers -- and ran 0.746 instead of 0.672 ms at six: ten LDS round trips in a row)
#pragma unroll
                    for (int b = 0; b < BB; ++b) tp[b] = bar_item_load<false>(lrow, a.bar_w, it[b], sub);   // slack: 2T >= 63 floats
#pragma unroll
                    for (int b = 0; b < BB; ++b) nx[b] = items[(size_t) (s0 + BB + b) * G];   // table has one batch of padding
                    // every load of the batch is ISSUED before the first sum: left to itself the backend sinks one step's four LDS reads to
                    // their uses -- four exposed LDS round trips (read, lgkmcnt(0), multiply) per batch of TWO steps (N = 4096 GL chain + 80 bars
                    // 1.645 -> 1.481 ms, N = 1024 1.318 -> 1.277, same box alternating: profiles/r05/uniform_branches.txt).  The six-step batches of
                    // N >= 16384 keep the backend's order: there one sunk step of six costs less than 96 registers of loads held at once
                    // (configs[2] 0.626 -> 0.643 ms with the fence on the same box)
                    if constexpr (BB <= kBarBatch) GLV_SCHED_FENCE();
#pragma unroll
                    for (int b = 0; b < BB; ++b) {
                        total = __builtin_fmaf(total, it[b].keep, group_sum<GL>(bar_item_lane_sum(tp[b])));
                        if (sub == 0) lres[it[b].res] = total;
                    }
#pragma unroll
                    for (int b = 0; b < BB; ++b) it[b] = nx[b];
                }
            }
            sy.sync();
            if constexpr (cols) {
                if (active) {
                    const uint16_t* ltex = reinterpret_cast<const uint16_t*>(lres);
                    float* co = a.bars_out + row * a.bars;
                    for (uint32_t x = (uint32_t) tid; x < a.bars; x += T) {
                        const ColumnMap m = a.col_map[x];
                        co[x] = column_mean(ltex[m.l], ltex[m.m], ltex[m.r]);
                    }
                }
            } else
            if (active) {
                if (a.bars_r16 && snap) {                  // snapped texels: the integer results as they are (the GL_R16 chain's, or FC_STATE_SNAP's)
                    uint16_t* bo = reinterpret_cast<uint16_t*>(a.bars_out) + row * a.bars;
                    const uint32_t* lout = reinterpret_cast<const uint32_t*>(lres);
                    for (uint32_t k = (uint32_t) tid; k < a.bars; k += T) bo[k] = (uint16_t) lout[k];
                } else if (GL16 && a.bars_r16) {           // uniform: the bars as GL_R16 texels (the smooth pass's render target, render.c:2277-2303)
                    uint16_t* bo = reinterpret_cast<uint16_t*>(a.bars_out) + row * a.bars;
                    if ((uint32_t) tid < a.bars) bo[tid] = (uint16_t) unorm16(lres[tid] / bar_wsum);
                    for (uint32_t k = (uint32_t) tid + T; k < a.bars; k += T) bo[k] = (uint16_t) unorm16(lres[k] / a.bar_desc[k].weight_sum);
                } else {
                if ((uint32_t) tid < a.bars) a.bars_out[row * a.bars + (uint32_t) tid] = lres[tid] / bar_wsum;
                // more bars than lanes (N=1024: 64 lanes, 80 bars): a second trip, its weight sums from L2
                for (uint32_t k = (uint32_t) tid + T; k < a.bars; k += T) a.bars_out[row * a.bars + k] = lres[k] / a.bar_desc[k].weight_sum;
                }
            }
            // the next row's first exchange write is preceded by a barrier (NBUF == 1): the bars readers are safe
        } else {
            if (active) finish(v, row, tid);
        }
    };
    // row handled by this slot in the iteration that starts at `base` (idle slots clamp to the last
    // row and still take part in the barriers; they just do not store).  For s16 input row r is
    // channel r&1 of frame r>>1: the two channels of a frame sit in neighbouring slots.
    auto row_of = [&](uint32_t base) -> uint32_t {
        const uint32_t r = base + slot;
        return r < a.units ? r : a.units - 1;
    };

    // IN_S16_TRACK / IN_F32_TRACK: where frame f = s * steps + t of the launch begins and where its channel-0 row goes (glv_frame.h TrackWindows).  One 32-bit
    // division per call, on a value that is wave-uniform wherever `slot` is (WAVE_SLOT); the window's start in 64-bit arithmetic, 4 or 8 bytes per frame.
    // Bounded reads: every caller passes f < units / 2 = streams * steps (frame_of / row_of clamp an idle slot and the look-ahead of a slot's last frame to
    // the LAST frame, as they do for back-to-back frames), so s < streams and t < steps: the address is the start of a window the call names, and
    // load_pcm_at reads that window's n frames and not a byte more.  No launch reads outside the windows [s * pitch + t * hop, + n) of the call.
    // IN_F32_TRACK: the same f, so the same windows; load_f32s_raw (pipelined: dwords at 16 c + 4 ch and 16 c + 8 + 4 ch, c < NN, ch < 2) and
    // load_f32_stereo_window_at (generic loop: bytes [16 c, 16 c + 16), c < NN) both stay inside the window's 8 n bytes.
    // The table kinds (TRACK_TABLE): the window begins min(starts[t], start_max) frames into the stream's recording -- track_window_start clamps whatever
    // the table holds to pitch_frames - n, so the bound above holds with [s * pitch + min(starts[t], pitch - n), + n) for the windows.  The entry is one more
    // load, and a load whose value an ADDRESS depends on must not be issued behind stores (the pipelined loops below: one in-order vmcnt): track_entry(f) is
    // therefore asked for one frame AHEAD of the track_at(f, entry) that uses it, together with the previous frame's PCM loads, and W retires both (where f is
    // wave-uniform, WAVE_SLOT, the compiler may make it a scalar load, which vmcnt does not count: nothing here relies on that).  t < steps: the entry read is one the call names.  The hop kinds: 0, no load,
    // and track_at is what it was (the table is a template constant: their code does not change).
    // The per-stream kinds (TRACK_EACH: glv_batch_track_each_*): the entry of frame f is starts[f % table_len], entry t of row s of uint32 [streams][steps] -- asked
    // for where the shared-table kinds ask for theirs, clamped as theirs is, and for every f an entry of the table the call names.
    // The pool kinds (TRACK_POOL: glv_batch_track_pool_*): every stream reads ONE buffer of a.trk.pitch_frames frames through the 16-byte span of stream s = f / steps
    // (glv_frame.h TrackSpan, track_pool_spans), and the window begins at pool_window_start -- clamped into the span, and whatever the span holds into the pool: the
    // bound above holds with [start, + n) inside the pool.  The span is a second load an address depends on: track_span(f) is asked for exactly where track_entry(f)
    // is, one frame ahead and together with the previous frame's PCM loads, and W retires all three; s < streams, so the record read is one the call names.  Every
    // other kind: an empty value, no load, and track_at is what it was.  The planar pool kind's two rows lie pitch_frames = pool_frames floats apart
    // (track_row_at, as ever) and a stream has no rows of its own to skip.
    struct NoSpan {};
    using TSpan = typename std::conditional<TRACK_POOL, TrackSpan, NoSpan>::type;
    auto track_span = [&](uint32_t f) -> TSpan { if constexpr (TRACK_POOL) return load_track_span(track_pool_spans(a.trk), f / a.trk.steps); else return TSpan(); };
    struct TrackAt { const void* win; size_t row0; };
    auto track_entry = [&](uint32_t f) -> uint32_t { if constexpr (TRACK_EACH) return track_table_entry(a.trk, f); else if constexpr (TRACK_TABLE) return a.trk.starts[f % a.trk.steps]; else return 0u; };
    auto track_at = [&](uint32_t f, uint32_t entry, TSpan span = TSpan()) -> TrackAt {
        const uint32_t s = f / a.trk.steps, t = f - s * a.trk.steps;
        uint64_t start;
        (void) span;
        if constexpr (TRACK_POOL) start = pool_window_start(span.first, span.frames, entry, a.trk.pitch_frames, (uint64_t) N);
        else if constexpr (TRACK_TABLE) start = (uint64_t) s * a.trk.pitch_frames + (entry < a.trk.start_max ? entry : a.trk.start_max);      // (track_window_start with a table)
        else start = (uint64_t) s * a.trk.pitch_frames + (uint64_t) t * a.trk.hop;
        if constexpr (TRACKP && !TRACK_POOL) start += (uint64_t) s * a.trk.pitch_frames;      // planar: a stream is TWO rows of pitch_frames floats, and this is where its channel-0 window begins
        return { static_cast<const char*>(a.in) + start * (TRACKF ? 8u : 4u), a.trk.step_major ? ((size_t) t * a.trk.streams + s) * 2u : (size_t) f * 2u };
    };
    (void) track_at; (void) track_entry; (void) track_span;
    // IN_F32_PLANAR_TRACK_AT: one slot = one channel ROW, as in the planar pipeline.  Row r of the launch is channel r & 1 of frame f = r >> 1, so track_at's rules
    // hold with f < units / 2 (row_of clamps an idle slot and every look-ahead to the last row): the window of channel ch begins pitch_frames floats behind
    // channel 0's, inside row 2 s + ch of the recording -- the clamp to start_max = pitch_frames - n keeps its n floats there, whatever the table holds.
    auto track_row_at = [&](uint32_t row, uint32_t entry, TSpan span = TSpan()) -> TrackAt {
        const TrackAt w = track_at(row >> 1, entry, span);
        return { static_cast<const char*>(w.win) + (uint64_t) (row & 1u) * a.trk.pitch_frames * 4u, w.row0 + (row & 1u) };
    };
    (void) track_row_at;

    unsigned xcount = 0;
    // A workgroup with a single slot takes both channel rows of a frame back to back (SEQ = 2), so
    // the frame's PCM is still fetched from HBM once and re-read from this CU's L1/L2.
    constexpr uint32_t SEQ = SLOTS == 1 ? 2 : 1, RPI = SLOTS * SEQ;      // rows per workgroup iteration
    const uint32_t stride = gridDim.x * RPI;
    const uint32_t nsteps = a.units == 0 ? 0 : ((a.units - 1) / RPI / gridDim.x + 1) * SEQ;   // upper bound, uniform
    auto step_base = [&](uint32_t step) -> uint32_t {            // first row of the workgroup's step-th row group
        return blockIdx.x * RPI + (step / SEQ) * stride + (step % SEQ) * SLOTS;
    };
    const int tid_outer = tid;
    if constexpr (S16 && PREFETCH == 1) {
        // In-place frame pipeline: one slot = one FRAME at a time, its two channel rows back to back, so
        // every frame's PCM is loaded exactly once by exactly one slot.  Per row r = 2*m + ch:
        //   A  ch == 1 only: issue the PCM loads of the slot's next frame into `raw` (both channels of
        //      the current frame were unpacked out of it already)        <- HBM latency starts here
        //   B  all FFT passes of row r                     (registers/LDS only: ~2 us of cover)
        //   W  s_waitcnt vmcnt(0): A's loads are a whole transform old, the previous row's stores older
        //   D  epilogue of row r: log/tilt/state + spectrum stores
        //   C  unpack + window row r+1 from `raw` straight into v (register-only: no vector-memory
        //      wait can land behind D's stores, W retired every load)
        // gfx9-class targets count loads and stores on one in-order counter (vmcnt) and a wait with
        // both kinds pending drains everything -- so a row must never need fresh load data right
        // after its predecessor's stores were issued; hence W before D and nothing but registers in C.
        const uint32_t nframes = a.units / 2;
        const uint32_t fstride = gridDim.x * SLOTS;
        const uint32_t nfs = nframes == 0 ? 0 : (nframes - 1) / fstride + 1;
        auto frame_of = [&](uint32_t m) -> uint32_t {
            const uint32_t f = blockIdx.x * SLOTS + m * fstride + slot;
            return f < nframes ? f : nframes - 1;
        };
        auto frame_ptr = [&](uint32_t f) -> const void* { return static_cast<const char*>(a.in) + (size_t) f * ((size_t) N * 4); };
        cf v[E];
        typename FR::Raw raw;
        size_t trow = 0, trow_next = 0;      // TRACK: channel-0 row of the slot's current frame / of the frame whose samples `raw` holds
        uint32_t tent = 0;                   // TRACK, a table call: the table's entry for the frame the NEXT stage A fetches, asked for by the stage A before it
        TSpan tspan = TSpan();               // ... and, a pool call, the span of that frame's stream, asked for with it
        (void) trow; (void) trow_next; (void) frame_ptr; (void) tent; (void) tspan;
        if (blockIdx.x * SLOTS < nframes) {
            int tid = tid_outer;
            asm volatile("" : "+v"(tid));
            if constexpr (TRACK) {
                const TrackAt w = track_at(frame_of(0), track_entry(frame_of(0)), track_span(frame_of(0))); FR::load_pcm_at(raw, w.win, tid); trow = w.row0;
                if constexpr (TRACK_TABLE) tent = track_entry(frame_of(1));      // (guarded: the mere call cost the hop kinds registers)
                if constexpr (TRACK_POOL) tspan = track_span(frame_of(1));
            } else
            FR::template load_pcm<RING>(raw, frame_ptr(frame_of(0)), tid, a.rot);
            FR::template unpack_window<0, WSPLIT>(v, raw, win, tid, 0u, a.mono != 0);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);
        for (uint32_t r = 0; r < 2 * nfs; ++r) {
            const uint32_t m = r >> 1, ch = r & 1u;
            if (blockIdx.x * SLOTS + m * fstride >= nframes) break;                     // uniform for the workgroup
            int tid = tid_outer;
            asm volatile("" : "+v"(tid));
            const uint32_t fraw = blockIdx.x * SLOTS + m * fstride + slot;
            const bool active = fraw < nframes;
            const uint32_t f = frame_of(m);
            if constexpr (TRACK) {                                                               // A (and the entry of the frame after: W retires both)
                if (ch) { const TrackAt w = track_at(frame_of(m + 1), tent, tspan); FR::load_pcm_at(raw, w.win, tid); trow_next = w.row0; if constexpr (TRACK_TABLE) tent = track_entry(frame_of(m + 2));
                          if constexpr (TRACK_POOL) tspan = track_span(frame_of(m + 2)); }
            } else
            if (ch) FR::template load_pcm<RING>(raw, frame_ptr(frame_of(m + 1)), tid, a.rot);   // A
            if constexpr (LIVE_PRE) { FR::live_prefetch(live_pre, (size_t) f * 2 + ch, tid, a); live_pre_ptr = &live_pre; }   // A': the row's old state (W awaits it)
            GLV_SCHED_FENCE();
            BD::template run<0>(v, tw_all, a.tw, xslot, tid, xcount, lds_tw, sy);                            // B
            GLV_SCHED_FENCE();
            __builtin_amdgcn_s_waitcnt(0x0F70);                                                  // W
            // WPRE: the first window values of row r+1 are requested ahead of D's stores (glv_frame.h window_prefetch)
            typename FR::template WinPre<WPRE> wp;
            if constexpr (WPRE > 0) { FR::template window_prefetch<WPRE>(wp, win, tid); GLV_SCHED_FENCE(); }
            if constexpr (TRACK) { finish_row(v, trow + ch, tid, active); if (ch) trow = trow_next; }   // D
            else
            finish_row(v, (size_t) f * 2 + ch, tid, active);                                     // D
            GLV_SCHED_FENCE();
            FR::template unpack_window<WPRE, WSPLIT>(v, raw, win, tid, ch ^ 1u, a.mono != 0, wp.w);      // C
        }
        return;
    }
    if constexpr (IN_MODE == IN_F32_PLANAR && PREFETCH == 1 && LOG_E <= 4) {
        // planar f32 rows (the lb/rb snapshot): the in-place pipeline over ROWS -- A issue the loads of the
        // slot's next row, B transform, W, D epilogue, C window the fetched samples into the point registers
        auto row_ptr = [&](uint32_t row) -> const void* { return static_cast<const char*>(a.in) + (size_t) row * ((size_t) N * 4); };
        cf v[E];
        typename FR::RawF raw;
        if (step_base(0) < a.units) {
            int tid = tid_outer;
            asm volatile("" : "+v"(tid));
            FR::load_f32_raw(raw, row_ptr(row_of(step_base(0))), tid);
            FR::window_f32_raw(v, raw, win, tid);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);
        for (uint32_t step = 0; step < nsteps; ++step) {
            const uint32_t base = step_base(step);
            if (base >= a.units) break;                          // uniform for the workgroup
            int tid = tid_outer;
            asm volatile("" : "+v"(tid));
            const bool active = base + slot < a.units;
            const uint32_t row = row_of(base);
            const uint32_t nb = step_base(step + 1);
            const bool has_next = step + 1 < nsteps && nb < a.units;
            FR::load_f32_raw(raw, row_ptr(row_of(has_next ? nb : base)), tid);                   // A (unconditional)
            GLV_SCHED_FENCE();
            BD::template run<0>(v, tw_all, a.tw, xslot, tid, xcount, lds_tw, sy);                    // B
            GLV_SCHED_FENCE();
            __builtin_amdgcn_s_waitcnt(0x0F70);                                                  // W
            finish_row(v, (size_t) row, tid, active);                                            // D
            GLV_SCHED_FENCE();
            FR::window_f32_raw(v, raw, win, tid);                                                // C
        }
        return;
    }
    if constexpr (TRACKP && PREFETCH == 1 && LOG_E <= 4) {
        // planar float recordings: the pipeline above with each row's window where the table says.  The entry of a row is asked for one step AHEAD of the address
        // that uses it (stage A of the step before, retired by W), as the interleaved table kinds do per frame: no load an address depends on follows stores.
        auto row_ahead = [&](uint32_t step, uint32_t base) -> uint32_t {      // the row the slot takes `step` steps in, or its current one beyond the last
            const uint32_t nb = step_base(step);
            return row_of(step < nsteps && nb < a.units ? nb : base);
        };
        cf v[E];
        typename FR::RawF raw;
        size_t trow = 0, trow_next = 0;      // where the slot's current row goes / the row whose samples `raw` holds
        uint32_t tent = 0;                   // the table's entry for the row the NEXT stage A fetches
        TSpan tspan = TSpan();               // ... and, a pool call, the span of that row's stream
        (void) tspan;
        if (step_base(0) < a.units) {
            int tid = tid_outer;
            asm volatile("" : "+v"(tid));
            const uint32_t r0 = row_of(step_base(0));
            const TrackAt w = track_row_at(r0, track_entry(r0 >> 1), track_span(r0 >> 1)); FR::load_f32_raw_at(raw, w.win, tid); trow = w.row0;
            tent = track_entry(row_ahead(1, step_base(0)) >> 1);
            if constexpr (TRACK_POOL) tspan = track_span(row_ahead(1, step_base(0)) >> 1);
            FR::window_f32_raw(v, raw, win, tid);
        }
        __builtin_amdgcn_s_waitcnt(0x0F70);
        for (uint32_t step = 0; step < nsteps; ++step) {
            const uint32_t base = step_base(step);
            if (base >= a.units) break;                          // uniform for the workgroup
            int tid = tid_outer;
            asm volatile("" : "+v"(tid));
            const bool active = base + slot < a.units;
            const TrackAt w = track_row_at(row_ahead(step + 1, base), tent, tspan);
            FR::load_f32_raw_at(raw, w.win, tid); trow_next = w.row0;                            // A (unconditional)
            tent = track_entry(row_ahead(step + 2, base) >> 1);                                  // (the entry of the row after: W retires it)
            if constexpr (TRACK_POOL) tspan = track_span(row_ahead(step + 2, base) >> 1);
            GLV_SCHED_FENCE();
            BD::template run<0>(v, tw_all, a.tw, xslot, tid, xcount, lds_tw, sy);                    // B
            GLV_SCHED_FENCE();
            __builtin_amdgcn_s_waitcnt(0x0F70);                                                  // W
            finish_row(v, trow, tid, active); trow = trow_next;                                  // D
            GLV_SCHED_FENCE();
            FR::window_f32_raw(v, raw, win, tid);                                                // C
        }
        return;
    }
    constexpr bool F32S = IN_MODE == IN_F32_STEREO || IN_MODE == IN_F32_RING || TRACKF;
    constexpr bool RINGF = IN_MODE == IN_F32_RING;
    if constexpr (F32S && PREFETCH == 1 && LOG_E <= 4) {
        // interleaved stereo f32 (PulseAudio), stereo only (the rare mono mix takes the generic loop below): one
        // slot = one frame, rows back to back, every row fetches its successor row's channel -- the sibling
        // channel of the same frame, then channel 0 of the slot's next frame
        if (a.mono == 0) {
            const uint32_t nframes = a.units / 2;
            const uint32_t fstride = gridDim.x * SLOTS;
            const uint32_t nfs = nframes == 0 ? 0 : (nframes - 1) / fstride + 1;
            auto frame_of = [&](uint32_t m) -> uint32_t {
                const uint32_t f = blockIdx.x * SLOTS + m * fstride + slot;
                return f < nframes ? f : nframes - 1;
            };
            auto frame_ptr = [&](uint32_t f) -> const void* { return static_cast<const char*>(a.in) + (size_t) f * ((size_t) N * 8); };
            cf v[E];
            typename FR::RawF raw;
            size_t trow = 0, trow_next = 0;      // TRACKF: channel-0 row of the slot's current frame / of the frame whose channel-0 samples `raw` holds or held last
            uint32_t tent = 0, tent_next = 0;    // TRACKF, a table call: the table's entries for the slot's current frame and its next, each asked for a frame ahead
            TSpan tspan = TSpan(), tspan_next = TSpan();      // ... and, a pool call, the spans of those frames' streams
            (void) trow; (void) trow_next; (void) frame_ptr; (void) tent; (void) tent_next; (void) tspan; (void) tspan_next;
            if (blockIdx.x * SLOTS < nframes) {
                int tid = tid_outer;
                asm volatile("" : "+v"(tid));
                if constexpr (TRACKF) {
                    if constexpr (TRACK_TABLE) tent = track_entry(frame_of(0));
                    if constexpr (TRACK_POOL) tspan = track_span(frame_of(0));
                    const TrackAt w = track_at(frame_of(0), tent, tspan); FR::template load_f32s_raw<false>(raw, w.win, tid, 0u); trow = w.row0;
                    if constexpr (TRACK_TABLE) tent_next = track_entry(frame_of(1));
                    if constexpr (TRACK_POOL) tspan_next = track_span(frame_of(1));
                } else
                FR::template load_f32s_raw<RINGF>(raw, frame_ptr(frame_of(0)), tid, 0u, a.rot);
                FR::window_f32_raw(v, raw, win, tid);
            }
            __builtin_amdgcn_s_waitcnt(0x0F70);
            for (uint32_t r = 0; r < 2 * nfs; ++r) {
                const uint32_t m = r >> 1, ch = r & 1u;
                if (blockIdx.x * SLOTS + m * fstride >= nframes) break;                 // uniform for the workgroup
                int tid = tid_outer;
                asm volatile("" : "+v"(tid));
                const bool active = blockIdx.x * SLOTS + m * fstride + slot < nframes;
                const uint32_t f = frame_of(m);
                if constexpr (TRACKF) {                                                              // A (unconditional): ch 0 fetches its own window's other channel
                    const TrackAt w = track_at(frame_of(m + ch), ch ? tent_next : tent, ch ? tspan_next : tspan);
                    FR::template load_f32s_raw<false>(raw, w.win, tid, ch ^ 1u);
                    if (ch) { trow_next = w.row0; if constexpr (TRACK_TABLE) { tent = tent_next; tent_next = track_entry(frame_of(m + 2)); }
                              if constexpr (TRACK_POOL) { tspan = tspan_next; tspan_next = track_span(frame_of(m + 2)); } }      // (the entry of the frame after: W retires it)
                } else
                FR::template load_f32s_raw<RINGF>(raw, frame_ptr(frame_of(m + ch)), tid, ch ^ 1u, a.rot);   // A (unconditional)
                GLV_SCHED_FENCE();
                BD::template run<0>(v, tw_all, a.tw, xslot, tid, xcount, lds_tw, sy);                // B
                GLV_SCHED_FENCE();
                __builtin_amdgcn_s_waitcnt(0x0F70);                                              // W
                if constexpr (TRACKF) { finish_row(v, trow + ch, tid, active); if (ch) trow = trow_next; }   // D
                else
                finish_row(v, (size_t) f * 2 + ch, tid, active);                                 // D
                GLV_SCHED_FENCE();
                FR::window_f32_raw(v, raw, win, tid);                                            // C
            }
            return;
        }
    }
    for (uint32_t step = 0; step < nsteps; ++step) {
        const uint32_t base = step_base(step);
        if (base >= a.units) break;                              // uniform for the workgroup
        // Re-define the lane id opaquely every iteration: window / twiddle table reads are loop
        // invariant, and LLVM would otherwise hoist ~120 VGPRs worth of them out of the frame loop
        // (and then spill them).  TWREG is the explicit, budgeted way to keep twiddles resident.
        int tid = tid_outer;
        asm volatile("" : "+v"(tid));
        const bool active = base + slot < a.units;
        const uint32_t row = row_of(base);
        cf v[E];
        if constexpr (TRACK) {
            // not pipelined (no production configuration): one slot = one channel row of the window its frame names, one division per row
            typename FR::Raw raw;
            const TrackAt w = track_at(row >> 1, track_entry(row >> 1), track_span(row >> 1));
            FR::load_pcm_at(raw, w.win, tid);
            GLV_SCHED_FENCE();
            FR::template unpack_window<0, WSPLIT>(v, raw, win, tid, row & 1u, a.mono != 0);
            BD::template run<0>(v, tw_all, a.tw, xslot, tid, xcount, lds_tw, sy);
            finish_row(v, w.row0 + (row & 1u), tid, active);
            continue;
        } else
        if constexpr (TRACKF) {
            // mono at every size, every chain where the configuration is not pipelined for f32 (LOG_E 5): one slot = one channel row of the window its frame names
            const TrackAt w = track_at(row >> 1, track_entry(row >> 1), track_span(row >> 1));
            FR::load_f32_stereo_window_at(v, w.win, win, tid, row & 1u, a.mono != 0);
            BD::template run<0>(v, tw_all, a.tw, xslot, tid, xcount, lds_tw, sy);
            finish_row(v, w.row0 + (row & 1u), tid, active);
            continue;
        } else
        if constexpr (TRACKP) {
            // every chain where the configuration is not pipelined for f32 (LOG_E 5): one slot = one channel row, read where its frame's entry says
            const TrackAt w = track_row_at(row, track_entry(row >> 1), track_span(row >> 1));
            FR::load_f32_window_at(v, w.win, win, tid);
            BD::template run<0>(v, tw_all, a.tw, xslot, tid, xcount, lds_tw, sy);
            finish_row(v, w.row0, tid, active);
            continue;
        } else
        if constexpr (S16) {
            // not pipelined: one slot = one channel row; the two channels of a frame sit in neighbouring
            // slots (the second reader of the frame's PCM hits L1/L2).  Measured faster than keeping the
            // samples in registers across two sequential rows of one slot.
            typename FR::Raw raw;
            FR::template load_pcm<RING>(raw, static_cast<const char*>(a.in) + (size_t) (row >> 1) * ((size_t) N * 4), tid, a.rot);
            GLV_SCHED_FENCE();
            FR::template unpack_window<0, WSPLIT>(v, raw, win, tid, row & 1u, a.mono != 0);
        } else if constexpr (F32S) {
            FR::template load_f32_stereo_window<RINGF>(v, static_cast<const char*>(a.in) + (size_t) (row >> 1) * ((size_t) N * 8), win, tid,
                                                       row & 1u, a.mono != 0, a.rot);
        } else {
            FR::load_f32_window(v, static_cast<const char*>(a.in) + (size_t) row * ((size_t) N * 4), win, tid);
        }
        BD::template run<0>(v, tw_all, a.tw, xslot, tid, xcount, lds_tw, sy);
        finish_row(v, (size_t) row, tid, active);
    }
}



template <int LOG_NN, int IN_MODE, int LOG_MODE, int SLOTS, int NBUF, int TWREG, bool WINLDS, int OCC, int PREFETCH, int TILTREG,
          int LOG_E = 4, int WPRE = 0, int WPRE_S = 0>
hipError_t launch_variant(FrameClass cls, const FrameArgs& a, int grid, hipStream_t st) {
    using FR = Frame<LOG_NN, LOG_E>;
    constexpr size_t lds = frame_lds_bytes<LOG_NN, LOG_E, SLOTS, NBUF, WINLDS, TWREG>();
    static_assert(lds <= 160 * 1024, "exchange regions + window exceed the 160 KiB LDS of a gfx950 CU");
    // the >64 KiB dynamic-LDS opt-in is a per-device function attribute: remember it per device
    // (one process per GPU is the deployment, but a host that drives several devices must work too)
    // (several host threads may drive several devices through the same instantiation -- glv_multi_*: the flags are
    // atomics; two threads racing on one device at worst both set the attribute, which is idempotent)
    struct AttrDone { std::atomic<bool> dev[64] = {}; };
    auto launch = [&](auto k, AttrDone& done, int threads = FR::T * SLOTS) -> hipError_t {
        if (lds > 64 * 1024) {
            int dev = 0;
            (void) hipGetDevice(&dev);
            if (dev < 0 || dev >= 64 || !done.dev[dev].load(std::memory_order_acquire)) {
                hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds);
                if (e != hipSuccess) return e;
                if (dev >= 0 && dev < 64) done.dev[dev].store(true, std::memory_order_release);
            }
        }
        if (grid <= 0) return hipSuccess;             // attribute only: glv_api.cpp batch_prepare readies the kernels a batch may launch, so
                                                      // that no process call changes a function attribute (a first call can be captured)
        hipLaunchKernelGGL(k, dim3(grid), dim3(threads), lds, st, a);
        return hipGetLastError();
    };
    static AttrDone done[kFrameClasses];   // per instantiation and class
    // the stateful epilogue needs the registers a resident last pass (TWREG 3) would occupy
    constexpr int TW_STATEFUL = TWREG == 3 ? 2 : TWREG;
    // the classes this configuration is not built for: fused bars need whole waves per row and the full-size, two-barrier exchange
    // region (NBUF 1); the GL_R16 chain is built for log modes 0 and 1
    auto launch_class = [&](auto c) -> hipError_t {
        constexpr int C = decltype(c)::value;
        // (IN_S16_TRACK / IN_F32_TRACK: a track call's transform is always stateless -- the other fourteen classes are not instantiated for them)
        if constexpr ((fc_fused_bars(C) && !(FR::T % 64 == 0 && NBUF == 1)) || (fc_gl16(C) && LOG_MODE == 2) || ((IN_MODE == IN_S16_TRACK || IN_MODE == IN_F32_TRACK || in_track_table(IN_MODE)) && fc_has_state(C))) return hipErrorInvalidValue;
        else if constexpr (fc_has_state(C))
            return launch(glv_frame_kernel<LOG_NN, IN_MODE, LOG_MODE, SLOTS, NBUF, TW_STATEFUL, WINLDS, OCC, PREFETCH, TILTREG, LOG_E, C, WPRE_S>, done[C]);
        else return launch(glv_frame_kernel<LOG_NN, IN_MODE, LOG_MODE, SLOTS, NBUF, TWREG, WINLDS, OCC, PREFETCH, TILTREG, LOG_E, C, WPRE>, done[C]);
    };
    switch (cls) {     // (in the order of the kernels in the code object)
        case FC_STATE_COLS:      return launch_class(std::integral_constant<int, FC_STATE_COLS>{});
        case FC_STATE_SNAP:      return launch_class(std::integral_constant<int, FC_STATE_SNAP>{});
        case FC_GL16_LIVE:       return launch_class(std::integral_constant<int, FC_GL16_LIVE>{});
        case FC_GL16_COLS_LIVE:  return launch_class(std::integral_constant<int, FC_GL16_COLS_LIVE>{});
        case FC_GL16_COLS:       return launch_class(std::integral_constant<int, FC_GL16_COLS>{});
        case FC_GL16_SNAP_LIVE:  return launch_class(std::integral_constant<int, FC_GL16_SNAP_LIVE>{});
        case FC_GL16_SNAP:       return launch_class(std::integral_constant<int, FC_GL16_SNAP>{});
        case FC_GL16_BARS_LIVE:  return launch_class(std::integral_constant<int, FC_GL16_BARS_LIVE>{});
        case FC_GL16_BARS:       return launch_class(std::integral_constant<int, FC_GL16_BARS>{});
        case FC_GL16:            return launch_class(std::integral_constant<int, FC_GL16>{});
        case FC_STATE_BARS_LIVE: return launch_class(std::integral_constant<int, FC_STATE_BARS_LIVE>{});
        case FC_STATE_BARS:      return launch_class(std::integral_constant<int, FC_STATE_BARS>{});
        case FC_STATE_R16:       return launch_class(std::integral_constant<int, FC_STATE_R16>{});
        case FC_STATE:           return launch_class(std::integral_constant<int, FC_STATE>{});
        case FC_R16:             return launch_class(std::integral_constant<int, FC_R16>{});
        case FC_PLAIN:           return launch_class(std::integral_constant<int, FC_PLAIN>{});
    }
    return hipErrorInvalidValue;
}

}  // namespace glv
