"""Source scanners shared by the host tests that pin a call path of the host units (glava_amd/csrc: glv_host.h and the .cpp files of HOST_UNITS, read as
one text by read_host_src) to launches and asynchronous device-to-device copies
(tests/test_stream_order.py and the test_track*_host.py files): a plain module, like oracle_lib.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORBIDDEN = ["hipMalloc", "hipFree", "hipMemcpy(", "hipMemset(", "hipMemcpyAsync(", "hipStreamSynchronize", "hipDeviceSynchronize",
             "hipHostMalloc", "hipEventSynchronize", "hipMemcpyToSymbol", "hipMemcpyFromSymbol",
             # glv_host.h's DeviceArray hides hipMalloc / hipMemcpy / hipMemset / hipFree behind these methods
             "upload(", "alloc(", "renew(", "reset("]
# the helpers that DO allocate: reachable from creation / set_params only
ALLOCATING_HELPERS = ["ensure_bar_tables", "ensure_smooth_tables", "batch_prepare", "set_tilt", "batch_alloc", "ensure_scratch", "build_snap_tables", "upload_fused_items"]


HOST_UNITS = ["glv_host.h", "glv_api.cpp", "glv_wisdom.cpp", "glv_device_state.cpp", "glv_bar_tables.cpp", "glv_chain.cpp", "glv_track.cpp"]


def read_csrc(name):
    return open(os.path.join(ROOT, "glava_amd", "csrc", name)).read()


def read_host_src():
    """the host layer behind the C ABI as one text, in a fixed order (a function's definition is found by its signature wherever it lives)"""
    return "\n".join(read_csrc(name) for name in HOST_UNITS)


def function_body(src, signature_re):
    m = re.search(signature_re, src)
    assert m, signature_re
    i = src.index("{", m.end() - 1)
    depth, j = 0, i
    while True:
        if src[j] == "{": depth += 1
        elif src[j] == "}":
            depth -= 1
            if depth == 0: break
        j += 1
    return src[i:j + 1]


def strip_comments(s):
    s = re.sub(r"//[^\n]*", "", s)
    return re.sub(r"/\*.*?\*/", "", s, flags=re.S)


def assert_launch_only(src, signatures, allowed=()):
    """every function of `src` named by a signature regex is free of the forbidden calls and of the allocating helpers (`allowed`: exact statements
    a path may issue all the same, removed before the search)"""
    for sig in signatures:
        body = strip_comments(function_body(src, sig))
        for ok in allowed:
            body = body.replace(ok, "")
        for f in FORBIDDEN:
            assert f not in body, (sig, f)
        for helper in ALLOCATING_HELPERS:
            assert helper + "(" not in body, (sig, helper)


# what every track path runs through besides its own entry, sizing query and plan
STATE_CHECKS = [r"\nint gravity_form\(", r"\nint refuse_gravity_mix\(", r"\nvoid commit_gravity_form\(", r"\nint refuse_stale_tilt\("]
TRACK_COMMON = [r"\nint refuse_track_pointers\(", r"\nuint64_t planned_work_bytes\(", r"\nint launch_bars_pass\(", r"\nint check_ops\(", r"\nvoid launch_plan\(",
                r"\nint timed_launch_begin\(", r"\nint timed_launch_end\("]
# ... and the FFT forms' executor with its stages
TRACK_EXECUTOR = [r"\nint track_args\(", r"\nint track_chain\(", r"\nbool pitch_too_short\(", r"\nint track\(glv_batch\* b,", r"\nint track_residues\(",
                  r"\nint track_windows\(", r"\nint track_scan\("] + STATE_CHECKS + TRACK_COMMON
