"""CPU: elastic batches (glv_batch_process_first_* / glv_batch_ring_update_first_* / glv_batch_copy_streams) -- what can be held without a device: the
header's declarations and the exported symbols, the argument checks that come before any device is touched, the DensePool bookkeeping
(glava_amd/stream_slots.py), that the new entries are launches and asynchronous copies only (the method of the other _host files), and the copy launcher's
vetting of its two region tables, compiled into a stand-alone program."""
import os
import subprocess

import pytest

from glava_amd import stream_slots as SL
from src_scan import ROOT, assert_launch_only, function_body, read_csrc, read_host_src, strip_comments

PREFIX_ENTRIES = ["glv_batch_process_first_s16", "glv_batch_process_first_f32", "glv_batch_process_first_f32_stereo", "glv_batch_ring_update_first_s16",
                  "glv_batch_ring_update_first_f32"]
ENTRIES = PREFIX_ENTRIES + ["glv_batch_copy_streams"]


def test_header_declares_and_library_exports_the_six_entries(glvlib):
    """within ABI 7, detected by the symbol (tests/test_abi.py then holds every declared symbol to the library)"""
    header = open(os.path.join(ROOT, "include", "glv_spectrum.h")).read()
    L = glvlib.lib()
    for name in ENTRIES:
        assert "int " + name + "(glv_batch* " in header, name
        assert hasattr(L, name), name
    assert L.glv_abi_version() == 7
    assert len(L.glv_batch_copy_streams.argtypes) == 6 and len(L.glv_batch_process_first_s16.argtypes) == 6 and len(L.glv_batch_ring_update_first_f32.argtypes) == 7
    for method in ("process_first_s16", "process_first_f32", "process_first_f32_stereo", "ring_update_first_s16", "ring_update_first_f32", "copy_streams"):
        assert callable(getattr(glvlib.Batch, method)), method
    # the protocol the library cannot check, and what has no prefix form, are said where a caller reads them
    block = header[header.index("/* Elastic batches"):header.index("int glv_batch_process_first_s16(")]
    for words in ("THE BATCH'S LOCKSTEP POSITIONS ADVANCE AS FOR A FULL CALL", "The library cannot check this protocol", "glv_batch_reset_streams, glv_batch_load_streams or glv_batch_copy_streams",
                  "Not offered in a prefix form", "glv_multi", "glv_slot_copy_kernel"):
        assert words in block, words
    assert "DensePool" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_arguments_are_refused_without_a_device(glvlib):
    L = glvlib.lib()
    assert L.glv_batch_process_first_s16(None, 1, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID
    assert L.glv_batch_process_first_f32(None, 1, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID
    assert L.glv_batch_process_first_f32_stereo(None, 1, None, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID
    assert L.glv_batch_ring_update_first_s16(None, 1, None, 8, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID
    assert L.glv_batch_ring_update_first_f32(None, 1, None, 8, None, glvlib.OP_FFT, None) == glvlib.ERR_INVALID
    assert L.glv_batch_copy_streams(None, None, None, None, 1, None) == glvlib.ERR_INVALID
    assert b"NULL" in L.glv_last_error()


def test_dense_pool_keeps_the_listeners_a_prefix():
    pool = SL.DensePool(3)
    assert (pool.capacity, pool.active) == (3, 0)
    assert [pool.attach() for _ in range(3)] == [0, 1, 2] and pool.active == 3
    with pytest.raises(IndexError):
        pool.attach()
    assert pool.detach(0) == (2, 0) and pool.active == 2                 # the last active slot fills the hole
    assert pool.detach(1) is None and pool.active == 1                   # the last slot itself: nothing moves
    with pytest.raises(IndexError):
        pool.detach(1)
    with pytest.raises(IndexError):
        pool.detach(-1)
    assert pool.attach() == 1                                            # a freed slot is taken again
    pool.grow(5)
    assert (pool.capacity, pool.active) == (5, 2)                        # the slots keep their numbers
    assert [pool.attach() for _ in range(3)] == [2, 3, 4]
    with pytest.raises(ValueError):
        pool.grow(4)
    assert pool.detach(0) == (4, 0) and pool.detach(0) == (3, 0) and pool.detach(0) == (2, 0) and pool.detach(0) == (1, 0) and pool.detach(0) is None
    assert pool.active == 0
    with pytest.raises(ValueError):
        SL.DensePool(0)


def test_the_new_entries_launch_and_nothing_else():
    """nothing is allocated, nothing copied synchronously or awaited: the calls can be captured into a hipGraph from the first call on"""
    src = read_host_src()
    sigs = [rf"\nint {name}\(" for name in ENTRIES] + [r"\nstatic int ring_update_first\(", r"\nint process_first\(", r"\nint refuse_prefix\(", r"\nint streams_fit\(",
                                                       r"\nvoid adopt_streams\(", r"\nstatic int ring_push\(", r"\nstatic int ring_append\(", r"\nint decimate_stage\("]
    assert_launch_only(src, sigs)
    plain = strip_comments(src)
    copy = function_body(plain, r"\nint glv_batch_copy_streams\(")
    assert copy.count("launch_slot_copy(") == 1 and "launch_slots(" not in copy and plain.count("launch_slot_copy(") == 1
    assert copy.count("slots_check(") == 2 and "streams_fit(dst, entry, \"the source batch\"" in copy and copy.index("streams_fit(") < copy.index("launch_slot_copy(")
    # load and copy share one set of checks, and load's are made in its own name
    assert "streams_fit(b, \"glv_batch_load_streams\", \"the blob\"" in function_body(plain, r"\nint glv_batch_load_streams\(")
    # a prefix call passes 2 * count where the full call passes the batch's rows, and its staging stage takes the call's streams
    first = function_body(plain, r"\nint process_first\(")
    assert "process(b, d_in, in_mode, d_out, ops, 2 * count, 0, st)" in first and "process(b, b->d_decim, glv::IN_F32_PLANAR, d_out, ops, 2 * count, 0, st, d_in, dec_kind)" in first
    assert "d.w.streams = pl.dec_streams" in function_body(plain, r"\nint decimate_stage\(")
    ring = function_body(plain, r"\nstatic int ring_update_first\(")
    assert "ring_push(b, f32, d_new, new_frames, st, &old_pos, count)" in ring and "2 * count, *pos, st)" in ring and ring.index("check_ops(") < ring.index("ring_push(")
    for name in PREFIX_ENTRIES[:3]:
        body = function_body(plain, rf"\nint {name}\(")
        assert "refuse_prefix(b," in body and "process_first(b, count," in body, name
    # ... and the kernel unit stays plain loads and stores
    unit = strip_comments(read_csrc("glv_slots.hip"))
    for word in ("atomic", "__shared__", "asm", "__builtin_amdgcn"):
        assert word not in unit, word
    assert_launch_only(read_csrc("glv_slots.hip"), [r"\nhipError_t launch_slot_copy\(", r"\nstatic bool slot_table_ok\("])
    kernel = function_body(unit, r"glv_slot_copy_kernel\(const SlotTable src,")
    assert "ss < src.streams && sd < dst.streams && p < pieces" in kernel and "(uint64_t) ss * rs.stream_bytes" in kernel and "(uint64_t) sd * rd.stream_bytes" in kernel


VET_MAIN = r"""
#include <cstdio>
#include "glv_launch.h"
using namespace glv;
// the tables of a float chain with F = 5 and an s16 ring at n = 256, bases that are never dereferenced: every call below is refused before a launch
static SlotTable table(uintptr_t base, uint32_t head, uint32_t ring_pos) {
    SlotTable t = {};
    t.r[0] = SlotRegion{reinterpret_cast<char*>(base), 0u, 2048u, 1024u, 10u, 0u, 1u};
    t.r[1] = SlotRegion{reinterpret_cast<char*>(base + 0x100000), 2048u, 10240u, 5120u, 10u, head, 5u};
    t.r[2] = SlotRegion{reinterpret_cast<char*>(base + 0x200000), 12288u, 1024u, 1024u, 2u, ring_pos, 256u};
    t.nregions = 3; t.bytes = 13312u; t.streams = 7; t.count = 3;
    t.idx = reinterpret_cast<const uint32_t*>(base + 0x300000);
    return t;
}
static int refused(const SlotTable& s, const SlotTable& d) { return launch_slot_copy(s, d, nullptr) == hipErrorInvalidValue ? 1 : 0; }
int main() {
    const SlotTable s = table(0x10000000, 2, 37), d = table(0x20000000, 4, 101);
    SlotTable x;
    int all = 1, k = 0;
#define CASE(side, edit) x = side; edit; { const int r = (&side == &s) ? refused(x, d) : refused(s, x); std::printf("%d %d\n", k++, r); all &= r; }
    CASE(d, x.r[1].mod = 3; x.r[1].chan_bytes = 3072u; x.r[1].stream_bytes = 6144u; x.r[2].start = 8192u; x.bytes = 9216u)      // another F: regions differ
    CASE(d, x.r[2].log_unit = 3u; x.r[2].mod = 128u)                                                                        // another frame size, same bytes
    CASE(s, x.nregions = 2; x.bytes = 12288u)                                                                               // one side has no ring
    CASE(s, x.r[1].pos = 5u)                                                                                                // pos >= mod, either side
    CASE(d, x.r[2].pos = 256u)
    CASE(d, x.r[0].pos = 1u)
    CASE(s, x.bytes = 13320u)                                                                                               // bytes no multiple of 16
    CASE(d, x.r[2].stream_bytes = 1032u; x.r[2].chan_bytes = 1032u; x.bytes = 13320u)
    CASE(d, x.r[2].mod = 258u; x.r[2].chan_bytes = 1032u; x.r[2].stream_bytes = 1032u; x.bytes = 13320u)
    CASE(s, x.r[2].base += 8)                                                                                               // a misaligned array
    CASE(d, x.idx = nullptr)
    CASE(s, x.idx = nullptr)
    CASE(d, x.count = 0u)
    CASE(s, x.count = 2u)                                                                                                   // the tables list different counts
    CASE(d, x.streams = 0u)
    CASE(d, x.nregions = 5u)
    std::printf("all %d\n", all);
    return all ? 0 : 1;
}
"""


def test_the_copy_launcher_vets_both_tables(tmp_path):
    """launch_slot_copy with malformed tables, as a stand-alone program (glv_slots.hip and a main; no device is needed: every case is refused before a launch):
    regions that differ between the sides, pos >= mod, bytes that are no multiple of 16, and the counts the kernel's bounds rest on"""
    from glava_amd import build as B
    main = tmp_path / "vet_main.hip"
    main.write_text(VET_MAIN)
    csrc = os.path.join(ROOT, "glava_amd", "csrc")
    prog = tmp_path / "vet"
    r = subprocess.run([B._hipcc(), "--offload-arch=" + B.ARCH, "-O1", "-std=c++17", "-I", csrc, str(main), os.path.join(csrc, "glv_slots.hip"), "-o", str(prog)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    out = subprocess.run([str(prog)], capture_output=True, text=True)
    lines = out.stdout.split("\n")
    assert out.returncode == 0 and "all 1" in lines, out.stdout + out.stderr
    assert len([l for l in lines if l.endswith(" 1") and not l.startswith("all")]) == 16
