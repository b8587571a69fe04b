// tests/native/verify_window_harness.cpp — TEST INFRASTRUCTURE.  The window arithmetic of k_verify_events_table
// (csrc/kernels/verify_window.h: which bytes of the blob a wavefront stages in LDS) behind a C interface, compiled for the
// host alone.  tests/test_verify_window.py holds it to a restatement written in the test.
#include <cstdint>

#include "../../ipc-filecoin-proofs_amd/csrc/kernels/verify_window.h"

using namespace ipcfp;

extern "C" {

uint32_t verify_window_bytes() { return kVerifyWindowBytes; }

// one lane: out = {contributes, lo, hi}
void verify_window_lane_run(uint32_t n_topics, uint32_t topics_off, int data_read, uint32_t data_off, uint64_t* out) {
    uint64_t lo, hi;
    out[0] = verify_window_lane(n_topics, topics_off, data_read != 0, data_off, lo, hi) ? 1 : 0;
    out[1] = lo;
    out[2] = hi;
}

// A wavefront of n_lanes lanes, composed as verify_table_hot composes it (a 32-bit min of the starts, a 32-bit max of the
// saturated relative ends).  lanes: n_lanes × {n_topics, topics_off, data_read, data_off, hot}; a lane that is not hot
// contributes nothing.  out = {any lane contributes, start, len (0: does not fit)}.
void verify_window_wave_run(const uint32_t* lanes, uint32_t n_lanes, uint64_t blob_len, uint64_t* out) {
    uint32_t lo_min = 0xffffffffu, rel_max = 0;
    bool any = false;
    for (uint32_t i = 0; i < n_lanes; ++i) {
        const uint32_t* l = lanes + 5 * i;
        uint64_t lo, hi;
        const bool reads = verify_window_lane(l[4] ? l[0] : 0u, l[1], l[4] && l[2], l[3], lo, hi);
        any = any || reads;
        const uint32_t v = reads ? uint32_t(lo) : 0xffffffffu;
        lo_min = v < lo_min ? v : lo_min;
    }
    const uint64_t start = verify_window_start(lo_min);
    for (uint32_t i = 0; i < n_lanes; ++i) {
        const uint32_t* l = lanes + 5 * i;
        uint64_t lo, hi;
        const bool reads = verify_window_lane(l[4] ? l[0] : 0u, l[1], l[4] && l[2], l[3], lo, hi);
        const uint32_t v = reads ? verify_window_rel_end(hi, start) : 0u;
        rel_max = v > rel_max ? v : rel_max;
    }
    out[0] = any ? 1 : 0;
    out[1] = start;
    out[2] = any ? verify_window_len(start, rel_max, blob_len) : 0u;
}

}  // extern "C"
