// tests/native/gen_tipsets_layout_harness.cpp — TEST INFRASTRUCTURE.  The layout arithmetic of the chain event generator
// (csrc/host/gen_tipsets_layout.h: per-tipset status, match count and blob bytes → the claim offsets and the blob segment
// starts; the root count the arguments alone decide) as a stand-alone program, compiled for the host alone with ASan and UBSan.
// tests/test_event_generate_tipsets.py holds it to a restatement written in Python (event_gen_chain_cases.layout).
//
// stdin:  "L" n_tipsets with_blob, then n_tipsets lines "status n_match blob_bytes"
//      or "A" n_tipsets, then n_tipsets + 1 parent offsets
// stdout: L: rc n_claims blob_len n_sound first_failing / claim_off[0 … n_tipsets] / blob_off[0 … n_tipsets] (with_blob; rc != 0: the
//            first line alone)
//         A: rc n_roots
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../ipc-filecoin-proofs_amd/csrc/host/gen_tipsets_layout.h"

using namespace ipcfp;

int main() {
    char mode = 0;
    uint32_t n = 0;
    if (std::scanf(" %c %" SCNu32, &mode, &n) != 2) return 2;
    if (mode == 'A') {
        std::vector<uint32_t> off(size_t(n) + 1);  // exactly n + 1 entries: reading one more is a heap overflow the sanitizer names
        for (uint32_t t = 0; t <= n; ++t)
            if (std::scanf("%" SCNu32, &off[t]) != 1) return 2;
        uint64_t n_roots = 0;
        const int rc = gen_tipsets_args(off.data(), n, &n_roots);
        std::printf("%d %" PRIu64 "\n", rc, n_roots);
        return 0;
    }
    if (mode != 'L') return 2;
    int with_blob = 0;
    if (std::scanf("%d", &with_blob) != 1) return 2;
    std::vector<uint32_t> status(n);
    std::vector<uint64_t> n_match(n), blob(n);
    for (uint32_t t = 0; t < n; ++t)
        if (std::scanf("%" SCNu32 " %" SCNu64 " %" SCNu64, &status[t], &n_match[t], &blob[t]) != 3) return 2;
    std::vector<uint64_t> c_off(size_t(n) + 1), b_off(size_t(n) + 1);
    GenTipsetsLayout lay;
    const int rc = gen_tipsets_layout(status.data(), n_match.data(), with_blob ? blob.data() : nullptr, n, c_off.data(),
                                      with_blob ? b_off.data() : nullptr, lay);
    std::printf("%d %" PRIu64 " %" PRIu64 " %" PRIu32 " %" PRId64 "\n", rc, lay.n_claims, lay.blob_len, lay.n_sound, lay.first_failing);
    if (rc != kGenLayoutOk) return 0;
    for (uint32_t t = 0; t <= n; ++t) std::printf("%" PRIu64 "%c", c_off[t], t == n ? '\n' : ' ');
    if (with_blob)
        for (uint32_t t = 0; t <= n; ++t) std::printf("%" PRIu64 "%c", b_off[t], t == n ? '\n' : ' ');
    return 0;
}
