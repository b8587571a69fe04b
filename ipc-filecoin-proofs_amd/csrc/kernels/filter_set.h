// csrc/kernels/filter_set.h — a SET of event specs (ipcfp_scan_events_multi), probed once per event.
//
// A spec is a filter (topic0 ‖ topic1, 64 key bytes) plus an optional emitter (`EventProofSpec`, src/proofs/generator.rs:
// 18-22).  The specs are grouped by their key bytes: a GROUP owns the members (spec index, has_actor, actor) that share a
// key, stored in ascending spec index — so the members an event satisfies come out in the order the scan's contract asks
// for.  The groups are found through an open-addressing table (linear probing, a power of two of slots, load ≤ 0.5) over
// a 64-bit fingerprint of the key; a slot whose fingerprint equals the probe's is CONFIRMED by comparing all 64 key bytes,
// which stay in the group record.  Witness bytes are adversarial: a probe visits at most `mask + 1` slots, and a
// fingerprint collision (two keys with one fingerprint, or many keys on one slot chain) costs compares, never an answer.
//
// Build and probe are plain C++ over arrays (FsView), compiled for the device by the scan kernels and for the host by
// host/scan_events_multi.cpp and tests/native/filter_set_harness.cpp (tests/test_scan_multi.py).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IPCFP_FS_FN __host__ __device__ __forceinline__
#else
#define IPCFP_FS_FN inline
#endif

namespace ipcfp {

constexpr uint32_t kFsNone = 0xffffffffu;

struct FsSlot {    // 16 B
    uint64_t fp;     // fingerprint of the group's key
    uint32_t group;  // kFsNone: the slot is empty
    uint32_t pad;
};
struct FsGroup {   // 72 B
    uint64_t key[8];  // topic0 ‖ topic1 as little-endian words
    uint32_t first;   // members [first, first + count)
    uint32_t count;
};
struct FsMember {  // 16 B
    uint64_t actor;
    uint32_t spec;
    uint32_t has_actor;
};
static_assert(sizeof(FsSlot) == 16 && sizeof(FsGroup) == 72 && sizeof(FsMember) == 16, "filter set layouts");

struct FsView {
    const FsSlot* slots;      // mask + 1
    const FsGroup* groups;    // n_groups
    const FsMember* members;  // n_specs, group by group
    uint32_t mask, n_groups, n_specs, pad;
};

// slots for n specs: the power of two ≥ 2 n (≥ 4), so the load never exceeds 0.5 and an empty slot always exists
IPCFP_FS_FN uint32_t fs_slots_for(uint32_t n_specs) {
    uint32_t s = 4;
    while (s < 2u * n_specs) s <<= 1;
    return s;
}

// the fingerprint, one key word at a time (a walker folds the words in as it reads them and keeps none)
IPCFP_FS_FN uint64_t fs_fp_init() { return 0x9e3779b97f4a7c15ull; }
IPCFP_FS_FN uint64_t fs_fp_step(uint64_t h, uint64_t word) {
    h ^= word;
    h *= 0xff51afd7ed558ccdull;
    return h ^ (h >> 32);
}
IPCFP_FS_FN uint64_t fs_fingerprint(const uint64_t key[8]) {
    uint64_t h = fs_fp_init();
#pragma unroll
    for (int k = 0; k < 8; ++k) h = fs_fp_step(h, key[k]);
    return h;
}
IPCFP_FS_FN uint32_t fs_home_slot(uint64_t fp, uint32_t mask) { return uint32_t(fp >> 7) & mask; }

IPCFP_FS_FN bool fs_key_equal(const uint64_t a[8], const uint64_t b[8]) {
    uint64_t diff = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) diff |= a[k] ^ b[k];
    return diff == 0;
}

// The group whose key has fingerprint `fp` and satisfies equal(group key), or kFsNone: `equal` is the full 64-byte compare
// of the caller (over a key in registers, or over bytes it reads again).  *compares (nullable): how many it was asked for.
template <typename Eq>
IPCFP_FS_FN uint32_t fs_probe_with(const FsView& v, uint64_t fp, Eq&& equal, uint32_t* compares = nullptr) {
    uint32_t s = fs_home_slot(fp, v.mask), found = kFsNone, cmp = 0;
    for (uint32_t step = 0; step <= v.mask; ++step) {  // bounded by the table, whatever it holds
        const FsSlot sl = v.slots[s];
        if (sl.group == kFsNone) break;
        if (sl.fp == fp && sl.group < v.n_groups) {
            ++cmp;
            if (equal(v.groups[sl.group].key)) {
                found = sl.group;
                break;
            }
        }
        s = (s + 1u) & v.mask;
    }
    if (compares) *compares = cmp;
    return found;
}
// … for a key held as eight words
IPCFP_FS_FN uint32_t fs_probe(const FsView& v, const uint64_t key[8], uint32_t* compares = nullptr) {
    return fs_probe_with(v, fs_fingerprint(key), [&](const uint64_t* gk) { return fs_key_equal(gk, key); }, compares);
}

// Build the set over caller-owned arrays: keys = n_specs × 64 bytes (ipcfp_event_filter_t[n_specs]); slots: n_slots =
// fs_slots_for(n_specs) entries; groups, members, group_of: n_specs entries each.  Returns the number of groups.
inline uint32_t fs_build(const uint8_t* keys, const uint8_t* has_actor, const uint64_t* actors, uint32_t n_specs, FsSlot* slots,
                         uint32_t n_slots, FsGroup* groups, FsMember* members, uint32_t* group_of) {
    const uint32_t mask = n_slots - 1u;
    for (uint32_t s = 0; s < n_slots; ++s) slots[s] = FsSlot{0, kFsNone, 0};
    uint32_t n_groups = 0;
    for (uint32_t j = 0; j < n_specs; ++j) {
        uint64_t key[8];
        for (int k = 0; k < 8; ++k) {
            uint64_t v = 0;
            for (int b = 0; b < 8; ++b) v |= uint64_t(keys[size_t(j) * 64 + 8 * k + b]) << (8 * b);
            key[k] = v;
        }
        const FsView so_far{slots, groups, members, mask, n_groups, 0, 0};
        uint32_t g = fs_probe(so_far, key);
        if (g == kFsNone) {
            g = n_groups++;
            for (int k = 0; k < 8; ++k) groups[g].key[k] = key[k];
            groups[g].first = groups[g].count = 0;
            const uint64_t fp = fs_fingerprint(key);
            uint32_t s = fs_home_slot(fp, mask);
            while (slots[s].group != kFsNone) s = (s + 1u) & mask;  // (load ≤ 0.5: an empty slot exists)
            slots[s] = FsSlot{fp, g, 0};
        }
        group_of[j] = g;
        ++groups[g].count;
    }
    uint32_t run = 0;
    for (uint32_t g = 0; g < n_groups; ++g) {
        groups[g].first = run;
        run += groups[g].count;
        groups[g].count = 0;
    }
    for (uint32_t j = 0; j < n_specs; ++j) {  // ascending spec index inside every group
        FsGroup& gr = groups[group_of[j]];
        const bool ha = has_actor && has_actor[j];
        members[gr.first + gr.count++] = FsMember{ha ? actors[j] : 0ull, j, ha ? 1u : 0u};
    }
    return n_groups;
}

}  // namespace ipcfp
