// csrc/host/scan_tipsets_layout.h — the LAYOUT of a chain scan's outputs (ipcfp_scan_events_tipsets, host/scan_events_tipsets.cpp):
// what the per-tipset (status, map size, record count) say about where each tipset's map bytes and records lie in the
// concatenated outputs, and how much of either the caller's capacities let through.
//
// A tipset whose scan is an Err has an empty range in both.  The totals and the offsets are never truncated; only the
// prefixes are.  Plain C++ over <cstdint>, so that the arithmetic is tested on a CPU (tests/native/scan_tipsets_layout_harness.cpp,
// tests/test_scan_tipsets.py); the fill kernels index the map with the receipt offsets computed here.
#pragma once
#include <cstdint>

namespace ipcfp {

constexpr uint32_t kTipsetSound = 1;  // == IPCFP_ST_TRUE

struct TipsetsLayout {
    uint64_t n_receipts = 0, n_matches = 0;        // off[n_tipsets] of either array
    uint64_t map_prefix = 0, match_prefix = 0;     // bytes of the map / records the capacities let through
    int64_t first_failing = -1;                    // the lowest tipset that is not sound
};

enum : int { kLayoutOk = 0, kLayoutTooManyReceipts = 1, kLayoutTooManyMatches = 2 };

// receipt_off / match_off: n_tipsets + 1 entries each.  The limits are those of the enumerator (fewer than 2^31 - 1 leaves, so a
// map of dense trees stays below it; a sparse tree's map may be larger and is bounded by 2^63) and of the 32-bit record offsets.
inline int tipsets_layout(const uint32_t* status, const uint64_t* n_idx, const uint64_t* n_match, uint32_t n_tipsets,
                          uint64_t cap_receipts, uint64_t cap_matches, uint64_t* receipt_off, uint64_t* match_off,
                          TipsetsLayout& out) {
    out = TipsetsLayout{};
    uint64_t r = 0, m = 0;
    for (uint32_t t = 0; t < n_tipsets; ++t) {
        receipt_off[t] = r;
        match_off[t] = m;
        if (status[t] != kTipsetSound) {
            if (out.first_failing < 0) out.first_failing = int64_t(t);
            continue;
        }
        if (n_idx[t] >= (1ull << 63) - r) return kLayoutTooManyReceipts;
        if (n_match[t] >= 0xffffffffull - m) return kLayoutTooManyMatches;
        r += n_idx[t];
        m += n_match[t];
    }
    receipt_off[n_tipsets] = r;
    match_off[n_tipsets] = m;
    out.n_receipts = r;
    out.n_matches = m;
    out.map_prefix = r < cap_receipts ? r : cap_receipts;
    out.match_prefix = m < cap_matches ? m : cap_matches;
    return kLayoutOk;
}

// the part of tipset t's range [off[t], off[t + 1]) inside a prefix: how many of its elements were written
inline uint64_t tipset_written(const uint64_t* off, uint32_t t, uint64_t prefix) {
    const uint64_t lo = off[t] < prefix ? off[t] : prefix, hi = off[t + 1] < prefix ? off[t + 1] : prefix;
    return hi - lo;
}

}  // namespace ipcfp
