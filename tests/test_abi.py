"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports
every entry point include/rdl_hip.h declares (no compute calls: no GPU here)."""
import ctypes as C
import os

import pytest

from rdl_lib import HIP_SO, HogbomParams, Integration, SubminorParams, declared_symbols


def test_header_declares_entry_points():
    syms = declared_symbols()
    for must in ("rdl_session_create", "rdl_find_peak", "rdl_subtract_psf",
                 "rdl_hogbom_run", "rdl_subminor_run", "rdl_fft_create",
                 "rdl_fft_convolve", "rdl_integrate", "rdl_iuwt_decompose",
                 "rdl_comm_allreduce_max"):
        assert must in syms
    assert len(syms) > 40


def test_library_exports_every_declared_symbol():
    if not os.path.exists(HIP_SO):
        pytest.skip("librdl_hip.so not built")
    lib = C.CDLL(HIP_SO)
    missing = [s for s in declared_symbols() if not hasattr(lib, s)]
    assert not missing, missing


def test_library_reports_version_and_errors_without_gpu():
    if not os.path.exists(HIP_SO):
        pytest.skip("librdl_hip.so not built")
    lib = C.CDLL(HIP_SO)
    lib.rdl_version.restype = C.c_char_p
    assert b"gfx950" in lib.rdl_version()
    lib.rdl_last_error.restype = C.c_char_p
    # argument validation happens before any device call
    assert lib.rdl_find_peak(None, None, 0, 0, 0, 0, 0, 0, 0, None, 1, None) != 0
    assert b"NULL" in lib.rdl_last_error()


def test_struct_layouts_match_header():
    # offsets the C compiler uses (checked against sizeof in the library build
    # would need a GPU-free helper; here: natural alignment expectations)
    assert C.sizeof(Integration) == 4 * 6 + 4 * 64 + 4
    assert C.sizeof(HogbomParams) % 8 == 0
    assert C.sizeof(SubminorParams) % 8 == 0


# Entry points no test calls directly, each with the reason. Only runtime
# plumbing without a numerical contract, the multi-rank calls, and passes that
# run inside a tested entry point belong here: anything else gets a test.
NOT_CALLED_DIRECTLY = {
    "rdl_device_count": "runtime query, no numerical contract",
    "rdl_host_alloc": "pinned host allocation, no numerical contract",
    "rdl_host_free": "pinned host allocation, no numerical contract",
    "rdl_session_bind": "makes the device current for a worker thread, no numerical contract",
    "rdl_memcpy_peer": "copy between two GPUs, no numerical contract",
    "rdl_timing_enable": "per-session timing switch, no numerical contract",
    "rdl_timing_get": "per-session timing read-out, no numerical contract",
    "rdl_timing_reset": "per-session timing reset, no numerical contract",
    "rdl_comm_id_size": "needs several ranks: tests/test_distributed.py through the host library",
    "rdl_comm_get_unique_id": "needs several ranks: tests/test_distributed.py through the host library",
    "rdl_comm_init": "needs several ranks: tests/test_distributed.py through the host library",
    "rdl_comm_destroy": "needs several ranks: tests/test_distributed.py through the host library",
    "rdl_comm_allreduce_max": "needs several ranks: tests/test_distributed.py through the host library",
    "rdl_comm_allreduce_sum_u64": "needs several ranks: tests/test_distributed.py through the host library",
    "rdl_comm_allreduce_max_n": "needs several ranks: tests/test_distributed.py through the host library",
    "rdl_comm_broadcast": "needs several ranks: tests/test_distributed.py through the host library",
    "rdl_comm_rank": "needs several ranks: tests/test_distributed.py through the host library",
    "rdl_fft64_inverse": "the inverse transform of rdl_fft64_convolve, which is tested",
}


def test_every_entry_point_is_called_by_a_test_or_listed_with_a_reason():
    import glob
    import re
    tests = os.path.dirname(os.path.abspath(__file__))
    text = "".join(open(f).read() for f in sorted(glob.glob(os.path.join(tests, "*.py"))))
    declared = declared_symbols()
    called = {s for s in declared if re.search(r"\b" + s + r"\s*\(", text)}
    uncovered = [s for s in declared if s not in called and s not in NOT_CALLED_DIRECTLY]
    assert not uncovered, f"no test calls these entry points: {uncovered}"
    stale = sorted(s for s in NOT_CALLED_DIRECTLY if s in called or s not in declared)
    assert not stale, f"listed as not called, but called or no longer declared: {stale}"
    allowed = re.compile(r"rdl_(device_count|host_alloc|host_free|session_bind|session_lane|"
                         r"session_join|memcpy_peer|timing_(enable|get|reset)|comm_\w+|"
                         r"conv_columns_layout|conv_columns_window|fft64_inverse)$")
    assert all(allowed.match(s) and reason for s, reason in NOT_CALLED_DIRECTLY.items())
