"""CPU: the window arithmetic of k_verify_events_table (csrc/kernels/verify_window.h) — which bytes of the blob a wavefront
stages in LDS for its usual claims — against a restatement written here over Python integers: the union of what the lanes
read ([topics_off, topics_off + 33·n_topics) when a topic is claimed, [data_off, data_off + 32) when the data is compared),
its lowest offset rounded down to 16, its highest rounded up to 16 and clamped to blob_len, staged when that is at most the
window.  Compiled for the host alone (tests/native/verify_window_harness.cpp)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "verify_window_harness.cpp")
LIB = os.path.join(HERE, "native", "libverify_window_harness.so")
HDR = os.path.join(HERE, "..", "ipc-filecoin-proofs_amd", "csrc", "kernels", "verify_window.h")

WINDOW = 64 * 104
BIG = 2**40  # a blob that never clamps


@pytest.fixture(scope="module")
def harness():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", LIB, SRC], check=True)
    lib = C.CDLL(LIB)
    lib.verify_window_bytes.restype = C.c_uint32
    lib.verify_window_lane_run.argtypes = [C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_void_p]
    lib.verify_window_wave_run.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_void_p]
    assert lib.verify_window_bytes() == WINDOW
    return lib


# ---- the restatement: lanes are (n_topics, topics_off, data_read, data_off, hot) ----
def lane_ranges(lane):
    nt, toff, dread, doff, hot = lane
    out = []
    if hot and nt >= 1:
        out.append((toff, toff + 33 * nt))
    if hot and dread:
        out.append((doff, doff + 32))
    return out


def want_wave(lanes, blob_len):
    rs = [r for l in lanes for r in lane_ranges(l)]
    if not rs:
        return None
    lo, hi = min(a for a, _ in rs), max(b for _, b in rs)
    start = lo - lo % 16
    end = min(-(-hi // 16) * 16, blob_len)
    return start, (end - start if end - start <= WINDOW else 0)


def got_wave(lib, lanes, blob_len):
    arr = np.array(lanes, dtype=np.uint32).reshape(-1, 5)
    out = np.zeros(3, np.uint64)
    lib.verify_window_wave_run(arr.ctypes.data, len(lanes), blob_len, out.ctypes.data)
    return (int(out[1]), int(out[2])) if out[0] else None


def check(lib, lanes, blob_len):
    for l in lanes:  # the harness is handed in-bounds lanes only, as the kernel's bounds check guarantees
        for _, b in lane_ranges(l):
            assert b <= blob_len
    got, want = got_wave(lib, lanes, blob_len), want_wave(lanes, blob_len)
    assert got == want, (lanes[:4], blob_len, got, want)
    return got


def test_one_lane(harness):
    out = np.zeros(3, np.uint64)
    for nt in (0, 1, 2):
        for dread in (0, 1):
            for toff, doff in ((0, 0), (7, 1000), (1000, 7), (2**32 - 1, 2**32 - 1), (2**32 - 1, 0), (0, 2**32 - 1)):
                harness.verify_window_lane_run(nt, toff, dread, doff, out.ctypes.data)
                rs = lane_ranges((nt, toff, dread, doff, 1))
                assert bool(out[0]) == bool(rs)
                if rs:  # (Python integers: 2**32 - 1 + 66 does not wrap here, and must not there)
                    assert (int(out[1]), int(out[2])) == (min(a for a, _ in rs), max(b for _, b in rs))


@pytest.mark.parametrize("n_lanes", [1, 2, 3, 31, 32, 33, 63, 64])
def test_contiguous_entries(harness, n_lanes):
    """the usual blob: one entry per lane, topics then data, back to back — every topic count, with and without data"""
    rng = np.random.default_rng(n_lanes)
    for prefix in range(0, 17):
        for trial in range(6):
            lanes, off = [], prefix
            for _ in range(n_lanes):
                nt, dread = (int(rng.integers(0, 3)), int(rng.integers(0, 2))) if trial else ((trial + n_lanes) % 3, 1)
                lanes.append((nt, off, dread, off + 33 * nt, 1))
                off += 33 * nt + 32
            for blob_len in (off, off + 1, off + 15, off + 16, BIG):  # the last entry ends the blob, or nearly
                got = check(harness, lanes, blob_len)
                if got:
                    assert got[0] % 16 == 0 and got[0] + got[1] <= blob_len
                    assert 0 < got[1] <= WINDOW  # 64 × 98 bytes and the rounding always fit


def test_lanes_that_contribute_nothing(harness):
    far = (2, 2**31, 1, 2**31 + 66, 0)          # not hot: far away, and ignored
    empty = (0, 2**31, 0, 2**31, 1)             # hot, but reads nothing of the blob
    near = (2, 4096, 1, 4096 + 66, 1)
    assert check(harness, [far] * 64, BIG) is None
    assert check(harness, [empty] * 64, BIG) is None
    assert check(harness, [far, empty], BIG) is None
    for k in range(64):
        lanes = [far if i % 2 else empty for i in range(64)]
        lanes[k] = near
        assert check(harness, lanes, BIG) == (4096, 112)
    # the same lanes, hot: they count, and the wavefront falls back
    assert check(harness, [near, (2, 2**31, 1, 2**31 + 66, 1)], BIG) == (4096, 0)


@pytest.mark.parametrize("a", [0, 16, 4096, 2**32 - 1 - 7000 - (2**32 - 1 - 7000) % 16])
def test_fits_exactly_and_one_byte_over(harness, a):
    lo_lane = (0, 0, 1, a, 1)
    for lo_shift in (0, 1, 15):  # the start rounds down to a
        first = (0, 0, 1, a + lo_shift, 1)
        for end, fits in ((a + WINDOW - 16, True), (a + WINDOW - 1, True), (a + WINDOW, True), (a + WINDOW + 1, False), (a + WINDOW + 16, False)):
            last = (0, 0, 1, end - 32, 1)
            got = check(harness, [first, last], BIG)
            assert (got[1] != 0) == fits, (a, lo_shift, end, got)
            got = check(harness, [last, (1, a + 500, 0, 0, 1), first], end)  # the blob ends with the last entry: the clamp
            assert (got[1] != 0) == fits and got[1] in (0, end - a)
    assert check(harness, [lo_lane], BIG) == (a, 32)


def test_offsets_near_the_top(harness):
    top = 2**32 - 1
    for blob_len in (2**32 + 31, 2**32 + 65, 2**32 + 100):
        lanes = [(0, 0, 1, top, 1)]
        if blob_len >= top + 66:
            lanes.append((2, top, 0, 0, 1))
        lanes.append((1, top - 40, 1, top - 7, 1))
        got = check(harness, lanes, blob_len)
        assert got[0] == (top - 40) - (top - 40) % 16 and got[0] + got[1] <= blob_len and got[1] > 0
    # one lane at the bottom, one at the top: 4 GB apart, no wrap into a small difference
    assert check(harness, [(1, 0, 0, 0, 1), (2, top, 1, top, 1)], 2**32 + 100) == (0, 0)
    assert check(harness, [(2, top, 1, top, 1), (1, 0, 0, 0, 1)], 2**32 + 100) == (0, 0)
    assert check(harness, [(1, top - WINDOW, 0, 0, 1), (0, 0, 1, top, 1)], 2**32 + 100) == ((top - WINDOW) - (top - WINDOW) % 16, 0)


def test_rounding_is_clamped(harness):
    # at 0: an extent that starts inside the first 16 bytes starts the window at 0
    for lo in range(0, 16):
        assert check(harness, [(1, lo, 0, 0, 1)], BIG) == (0, -(-(lo + 33) // 16) * 16)
    # at blob_len: the window never reaches past the blob's last byte
    for tail in range(0, 17):
        blob_len = 1000 + 33 + tail
        got = check(harness, [(1, 1000, 0, 0, 1)], blob_len)
        assert got == (992, min(-(-1033 // 16) * 16, blob_len) - 992)
    # a blob shorter than 16 bytes cannot hold a topic entry; 32 bytes of data in a 32-byte blob
    assert check(harness, [(0, 0, 1, 0, 1)], 32) == (0, 32)
    assert check(harness, [(0, 0, 1, 1, 1)], 33) == (0, 33)
