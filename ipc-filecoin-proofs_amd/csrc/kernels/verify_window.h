// csrc/kernels/verify_window.h — the WINDOW of the blob that a wavefront of k_verify_events_table (verify_table.hip) reads
// coalesced into LDS: the byte extent of what its usual claims read there (verify_table_hot: the topics entries and the 32
// data bytes, each only where its guard is true), rounded out to 16 bytes and clamped to the blob.  When the extent fits the
// wavefront's LDS region the claimed bytes come from there; when it does not the wavefront keeps its per-lane global loads.
//
// Every quantity is 64-bit (or a difference already bounded by the window), so nothing wraps for any uint32 offset and
// any blob_len.  Plain C++ over <cstdint>, so that the arithmetic is tested on a CPU (tests/native/verify_window_harness.cpp,
// tests/test_verify_window.py); the kernel uses the same functions on the device.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IPCFP_WINDOW_FN __host__ __device__ inline
#else
#define IPCFP_WINDOW_FN inline
#endif

namespace ipcfp {

// one wavefront's claims (64 × 104 bytes): the region holds them first and the window afterwards
constexpr uint32_t kVerifyWindowBytes = 64u * 104u;

// What the usual claim reads of the blob: [lo, hi).  false: nothing (no topic claimed and no data to compare) — the lane
// contributes nothing to its wavefront's extent.  `data_read`: the claim's data is matchable (hence 32 bytes long).
IPCFP_WINDOW_FN bool verify_window_lane(uint32_t n_topics, uint32_t topics_off, bool data_read, uint32_t data_off, uint64_t& lo,
                                        uint64_t& hi) {
    lo = ~0ull;
    hi = 0;
    if (n_topics >= 1) {
        lo = topics_off;
        hi = uint64_t(topics_off) + 33ull * n_topics;
    }
    if (data_read) {
        const uint64_t a = data_off, b = a + 32ull;
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
    return hi != 0;
}

// the window starts at the wavefront's lowest offset rounded DOWN to 16 (an offset: never below 0)
IPCFP_WINDOW_FN uint64_t verify_window_start(uint64_t lo_min) { return lo_min & ~15ull; }

// A lane's end relative to the start (hi >= start), saturated one past the window: what the wavefront reduces with a
// 32-bit max.  A saturated value never fits, whatever the true distance was.
IPCFP_WINDOW_FN uint32_t verify_window_rel_end(uint64_t hi, uint64_t start) {
    const uint64_t d = hi - start;
    return d > kVerifyWindowBytes ? kVerifyWindowBytes + 1u : uint32_t(d);
}

// Bytes to stage from `start`: the end rounded UP to 16 and clamped to blob_len (every contributing lane is in bounds, so
// the clamp never cuts a claimed byte).  0: the extent does not fit the window.
IPCFP_WINDOW_FN uint32_t verify_window_len(uint64_t start, uint32_t rel_end_max, uint64_t blob_len) {
    if (rel_end_max == 0 || rel_end_max > kVerifyWindowBytes) return 0;
    uint64_t end = (start + rel_end_max + 15ull) & ~15ull;
    end = end > blob_len ? blob_len : end;
    if (end < start + rel_end_max) return 0;  // (an extent past the blob: the caller's bounds check forbids it)
    const uint64_t len = end - start;
    return len > kVerifyWindowBytes ? 0u : uint32_t(len);
}

}  // namespace ipcfp
