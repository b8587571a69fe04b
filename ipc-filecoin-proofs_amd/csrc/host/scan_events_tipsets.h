// csrc/host/scan_events_tipsets.h — the scan of a chain of tipsets for a set of specs (host/scan_events_tipsets.cpp), for the
// host code that builds on it.
#pragma once
#include <vector>

#include "../common.h"
#include "scan_tipsets_layout.h"

namespace ipcfp {

struct TipsetsScanResult {
    std::vector<uint32_t> status;  // n_tipsets × ipcfp_status_t
    std::vector<uint8_t> phase;    // n_tipsets × IPCFP_SCAN_PHASE_* (0: TRUE)
    std::vector<uint64_t> receipt_off, match_off;  // n_tipsets + 1 each
    TipsetsLayout layout;
    DevBuf<uint8_t> has;
    DevBuf<ipcfp_event_match_t> matches;
    DevBuf<uint32_t> match_spec;
    DevBuf<uint64_t> spec_counts;
    // caller-owned HBM outputs (ipcfp_scan_events_tipsets_device): PASS 2 writes the prefix there, nothing behind it
    uint8_t* ext_has = nullptr;
    ipcfp_event_match_t* ext_matches = nullptr;
    uint32_t* ext_match_spec = nullptr;
    uint8_t* has_p = nullptr;  // layout.map_prefix bytes
    ipcfp_event_match_t* matches_p = nullptr;  // layout.match_prefix records, like match_spec_p
    uint32_t* match_spec_p = nullptr;
    uint64_t* spec_counts_p = nullptr;
};

// One enumeration of the n_tipsets receipts trees (one more per failing tree), PASS 1, prefix sum, PASS 2.  `touched_d`
// (nullable, device) is OR-ed into.  The stream is drained when it returns.  `skip_mask` (nullable, n_tipsets bytes): a tipset
// whose byte is set is not looked at — its root is never loaded, its ranges are empty, its status stays IPCFP_ST_ERR with
// phase 0 (the chain generator's tipsets that failed before the scan, host/generate.cpp).
int scan_events_tipsets_device(ipcfp_ctx* ctx, ipcfp_witness* w, const uint8_t* roots40, uint32_t n_tipsets,
                               const ipcfp_event_filter_t* filters, const uint8_t* has_actor, const uint64_t* actors, uint32_t n_specs,
                               uint32_t* touched_d, TipsetsScanResult& out, uint64_t cap_receipts, uint64_t cap_matches,
                               const uint8_t* skip_mask = nullptr);

}  // namespace ipcfp
