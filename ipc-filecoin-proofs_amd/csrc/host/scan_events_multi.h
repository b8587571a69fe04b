// csrc/host/scan_events_multi.h — the scan for a set of specs (host/scan_events_multi.cpp), for the host code that builds on it.
#pragma once
#include <vector>

#include "../common.h"

namespace ipcfp {

struct MultiScanResult {
    uint32_t status = IPCFP_ST_ERR;
    uint32_t phase = 0;  // IPCFP_SCAN_PHASE_* of an Err
    uint64_t n_idx = 0, n_matches = 0;
    DevBuf<uint8_t> has;
    DevBuf<ipcfp_event_match_t> matches;
    DevBuf<uint32_t> match_spec;
    DevBuf<uint64_t> spec_counts;
    // caller-owned HBM outputs (ipcfp_scan_events_multi_device): PASS 2 writes there directly when they are set (the
    // map: and large enough); *_p then point into them
    uint8_t* ext_has = nullptr;
    uint64_t ext_has_cap = 0;
    ipcfp_event_match_t* ext_matches = nullptr;  // capacity = the call's cap_matches, like ext_match_spec
    uint32_t* ext_match_spec = nullptr;
    uint8_t* has_p = nullptr;
    ipcfp_event_match_t* matches_p = nullptr;
    uint32_t* match_spec_p = nullptr;
    uint64_t* spec_counts_p = nullptr;
};

// PASS 1 + prefix sum + PASS 2 on the device for n_specs ≤ IPCFP_MAX_SCAN_SPECS specs (host arrays).  `touched_d` (nullable,
// device) is OR-ed into.  At most cap_matches records are written; out.n_matches is the total.
int scan_events_multi_device(ipcfp_ctx* ctx, ipcfp_witness* w, const CidKey& root, const ipcfp_event_filter_t* filters,
                             const uint8_t* has_actor, const uint64_t* actors, uint32_t n_specs, uint32_t* touched_d,
                             MultiScanResult& out, uint64_t cap_matches);

// the filter set of a call (kernels/filter_set.h), built in `host` and queued for upload with one copy: `host` must outlive
// the copy, i.e. the caller drains the stream before it goes away
struct FsView;
int upload_filter_set(ipcfp_ctx* ctx, const ipcfp_event_filter_t* filters, const uint8_t* has_actor, const uint64_t* actors,
                      uint32_t n_specs, std::vector<uint8_t>& host, DevBuf<uint8_t>& dev, FsView& view);

}  // namespace ipcfp
