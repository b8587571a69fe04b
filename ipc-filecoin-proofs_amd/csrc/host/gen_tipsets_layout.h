// csrc/host/gen_tipsets_layout.h — the LAYOUT of a chain generator's outputs (ipcfp_generate_event_claims_tipsets,
// host/generate.cpp): what the per-tipset (status, match count, blob bytes) say about where each tipset's claims lie in the
// one claim list and where its segment starts in the one tight blob.
//
// A tipset whose status is not IPCFP_ST_TRUE has an empty range in both.  Plain C++ over <cstdint>, so that the arithmetic
// is tested on a CPU (tests/native/gen_tipsets_layout_harness.cpp, tests/test_event_generate_tipsets.py).
#pragma once
#include <cstdint>

namespace ipcfp {

constexpr uint32_t kGenTipsetSound = 1;                // == IPCFP_ST_TRUE
constexpr uint64_t kGenMaxClaims = 0xffffffffull;      // claim offsets and match counts are 32-bit on the device: fewer than this
constexpr uint64_t kGenMaxBlob = 0xf0000000ull;        // topics_off / data_off are 32-bit: a blob below 3.75 GB

struct GenTipsetsLayout {
    uint64_t n_claims = 0, blob_len = 0;  // claim_off[n_tipsets], blob_off[n_tipsets]
    uint32_t n_sound = 0;
    int64_t first_failing = -1;           // the lowest tipset that is not sound
};

enum : int { kGenLayoutOk = 0, kGenLayoutTooManyClaims = 1, kGenLayoutBlobTooLarge = 2 };

// claim_off / blob_off: n_tipsets + 1 entries each.  blob_bytes and blob_off are nullable TOGETHER (the claim ranges alone).
inline int gen_tipsets_layout(const uint32_t* status, const uint64_t* n_match, const uint64_t* blob_bytes, uint32_t n_tipsets,
                              uint64_t* claim_off, uint64_t* blob_off, GenTipsetsLayout& out) {
    out = GenTipsetsLayout{};
    uint64_t c = 0, b = 0;
    for (uint32_t t = 0; t < n_tipsets; ++t) {
        claim_off[t] = c;
        if (blob_off) blob_off[t] = b;
        if (status[t] != kGenTipsetSound) {
            if (out.first_failing < 0) out.first_failing = int64_t(t);
            continue;
        }
        ++out.n_sound;
        if (n_match[t] >= kGenMaxClaims - c) return kGenLayoutTooManyClaims;
        c += n_match[t];
        if (blob_off && blob_bytes) {
            if (blob_bytes[t] >= kGenMaxBlob - b) return kGenLayoutBlobTooLarge;
            b += blob_bytes[t];
        }
    }
    claim_off[n_tipsets] = c;
    if (blob_off) blob_off[n_tipsets] = b;
    out.n_claims = c;
    out.blob_len = b;
    return kGenLayoutOk;
}

// what the arguments alone decide about a chain: Σ 2·n_parents message-tree roots, which the enumerator's error word must order
constexpr uint32_t kGenMaxRoots = 65535;
enum : int { kGenArgsOk = 0, kGenArgsNotAscending = 1, kGenArgsTooManyRoots = 2 };
inline int gen_tipsets_args(const uint32_t* parent_off, uint32_t n_tipsets, uint64_t* n_roots) {
    *n_roots = 0;
    if (parent_off[0] != 0) return kGenArgsNotAscending;
    for (uint32_t t = 0; t < n_tipsets; ++t)
        if (parent_off[t + 1] < parent_off[t]) return kGenArgsNotAscending;
    *n_roots = 2ull * parent_off[n_tipsets];
    return *n_roots > kGenMaxRoots ? kGenArgsTooManyRoots : kGenArgsOk;
}

}  // namespace ipcfp
