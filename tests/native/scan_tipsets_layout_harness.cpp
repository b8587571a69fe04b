// tests/native/scan_tipsets_layout_harness.cpp — TEST INFRASTRUCTURE.  The layout arithmetic of the chain scan
// (csrc/host/scan_tipsets_layout.h: per-tipset status, map size and record count → the two offset arrays and the prefixes the
// capacities let through) as a stand-alone program, compiled for the host alone with ASan and UBSan.
// tests/test_scan_tipsets.py holds it to a restatement written in Python (scan_tipsets_cases.layout).
//
// stdin:  n_tipsets cap_receipts cap_matches, then n_tipsets lines "status n_idx n_match"
// stdout: rc n_receipts n_matches map_prefix match_prefix first_failing
//         receipt_off[0 … n_tipsets]
//         match_off[0 … n_tipsets]
//         per tipset: map bytes written, records written          (rc != 0: the first line alone)
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ipc-filecoin-proofs_amd/csrc/host/scan_tipsets_layout.h"

using namespace ipcfp;

int main() {
    uint32_t n = 0;
    uint64_t cap_r = 0, cap_m = 0;
    if (std::scanf("%" SCNu32 " %" SCNu64 " %" SCNu64, &n, &cap_r, &cap_m) != 3) return 2;
    std::vector<uint32_t> status(n);
    std::vector<uint64_t> n_idx(n), n_match(n);
    for (uint32_t t = 0; t < n; ++t)
        if (std::scanf("%" SCNu32 " %" SCNu64 " %" SCNu64, &status[t], &n_idx[t], &n_match[t]) != 3) return 2;
    // exactly n + 1 entries each: an off-by-one in the header is a heap overflow the sanitizer names
    std::vector<uint64_t> r_off(size_t(n) + 1), m_off(size_t(n) + 1);
    TipsetsLayout lay;
    const int rc = tipsets_layout(status.data(), n_idx.data(), n_match.data(), n, cap_r, cap_m, r_off.data(), m_off.data(), lay);
    std::printf("%d %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRId64 "\n", rc, lay.n_receipts, lay.n_matches, lay.map_prefix,
                lay.match_prefix, lay.first_failing);
    if (rc != kLayoutOk) return 0;
    for (uint32_t t = 0; t <= n; ++t) std::printf("%" PRIu64 "%c", r_off[t], t == n ? '\n' : ' ');
    for (uint32_t t = 0; t <= n; ++t) std::printf("%" PRIu64 "%c", m_off[t], t == n ? '\n' : ' ');
    for (uint32_t t = 0; t < n; ++t)
        std::printf("%" PRIu64 " %" PRIu64 "\n", tipset_written(r_off.data(), t, lay.map_prefix), tipset_written(m_off.data(), t, lay.match_prefix));
    return 0;
}
