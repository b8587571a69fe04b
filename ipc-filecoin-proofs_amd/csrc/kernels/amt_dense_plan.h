// csrc/kernels/amt_dense_plan.h — the PLAN of the dense AMT walk (amt_dense.hip): what the roots' (height, bit width, count)
// say about every level, and with that the size of every buffer the walk's kernels write.
//
// fvm_ipld_amt writes message lists, receipts and events with indices 0..count-1, so the whole shape of the tree follows
// from the root: node p of a level has min(W, remaining) entries with the low bits of its bitmap set, and child q of a level
// hangs off parent q / W at slot q % W.  With the shape known there is nothing to count or prefix-sum.
//
// Plain C++ over <cstdint>, <vector> and the ABI header, so that the arithmetic that sizes the buffers is tested on a CPU
// (tests/native/dense_plan_harness.cpp, tests/test_dense_plan.py); the kernels use the same functions on the device.
#pragma once
#include <cstdint>
#include <vector>

#include "ipcfp.h"

#if defined(__HIPCC__)
#define IPCFP_DENSE_PLAN_FN __host__ __device__ inline
#else
#define IPCFP_DENSE_PLAN_FN inline
#endif

namespace ipcfp {

struct DenseRoot {
    uint32_t height, bit_width;
    uint64_t count;
    uint64_t lo, hi;  // the indices to enumerate: [lo, hi) with lo < hi <= count, or (0, 0) for an empty tree
    uint32_t vkind;   // value type of this tree
    uint32_t out_sel; // where its values go: 0 = keys_out (links as witness keys), 1 = leaves, 2 = leaves of the extra root
    uint64_t out_off; // ... from this element on
};
constexpr uint32_t kMaxDenseRoots = 2 * IPCFP_MAX_PARENTS + 1;  // BLS + secp per parent block, + the receipts AMT
constexpr uint32_t kMaxDenseLevels = 24;
// interior levels of at most this many entries at the top of the walk share ONE single-workgroup launch (k_dense_top)
constexpr uint32_t kDenseTopMax = 1024;
struct DenseRoots {  // travels as a kernel ARGUMENT (1.6 KB): no copy at the head of the walk
    DenseRoot r[kMaxDenseRoots];
    uint32_t n;
};
struct DensePlan {
    bool ok = false;          // every root is a dense candidate: the walk may be launched
    uint32_t n_use = 0;       // roots in the walk (the call's own + the extra one when it joined)
    uint32_t max_height = 0;
    uint64_t n_level[kMaxDenseLevels] = {};  // nodes per level (node height)
    uint64_t n_leaves = 0, n_extra = 0, biggest = 0;
    DenseRoots roots{};
};

// nodes of `level` (node height) the whole tree has
IPCFP_DENSE_PLAN_FN uint64_t dense_total(const DenseRoot& r, uint32_t level) {
    if (r.height < level) return 1;  // rides along until its own level
    const uint64_t shift = uint64_t(r.bit_width) * (level + 1);
    if (shift >= 64) return 1;
    const uint64_t n = (r.count + (1ULL << shift) - 1) >> shift;
    return n ? n : 1;
}
// first node of `level` that holds an index of [lo, hi), and how many such nodes there are
IPCFP_DENSE_PLAN_FN uint64_t dense_first(const DenseRoot& r, uint32_t level) {
    const uint64_t shift = uint64_t(r.bit_width) * (level + 1);
    return (r.height < level || shift >= 64 || r.hi == 0) ? 0 : (r.lo >> shift);
}
IPCFP_DENSE_PLAN_FN uint64_t dense_nodes(const DenseRoot& r, uint32_t level) {
    const uint64_t shift = uint64_t(r.bit_width) * (level + 1);
    if (r.height < level || shift >= 64 || r.hi == 0) return 1;
    return ((r.hi - 1) >> shift) - (r.lo >> shift) + 1;
}

// the receipts tree's leaf kernel (k_dense_receipt_leaves): a group of G lanes per leaf node, its stage in LDS
constexpr uint32_t kReceiptStageBytes = 64;  // LDS per lane: a group stages nodes of up to G · 64 - 16 bytes
constexpr uint32_t kReceiptStageSlack = 6;   // words behind a group's stage: what a fetch near the node's end reads beyond it
IPCFP_DENSE_PLAN_FN uint32_t receipt_leaf_group(uint32_t bit_width) { return bit_width >= 6u ? 64u : (1u << bit_width); }
IPCFP_DENSE_PLAN_FN uint32_t receipt_stage_words(uint32_t G) { return G * (kReceiptStageBytes / 8u) + kReceiptStageSlack; }

inline uint64_t amt_span_host(uint32_t bw, uint64_t height) {
    const uint64_t shift = uint64_t(bw) * height;
    return shift >= 64 ? ~0ULL : (1ULL << shift);
}

// root_info: 2 words per root as k_enum_roots writes them ({height | bw << 32, count}; ~0 = a root that failed to load);
// the optional extra root is entry n_roots.  plan.ok stays false for anything the dense walk does not take.
inline void dense_plan(const std::vector<uint64_t>& root_info, uint32_t n_roots, int vkind, bool want_keys, uint64_t lo, uint64_t hi,
                       uint32_t has_extra, int extra_vkind, uint64_t extra_lo, uint64_t extra_hi, DensePlan& plan) {
    plan = DensePlan{};
    const uint32_t n_all = n_roots + (has_extra ? 1u : 0u);
    if (n_roots == 0 || n_all > kMaxDenseRoots || root_info.size() < 2 * size_t(n_all)) return;
    auto shape = [&](uint32_t i, uint64_t rlo, uint64_t rhi, DenseRoot& d) -> bool {  // false: not a dense candidate
        if (root_info[2 * size_t(i)] == ~0ULL) return false;  // a dead root: let the general walk sort it out
        d.height = uint32_t(root_info[2 * size_t(i)]);
        d.bit_width = uint32_t(root_info[2 * size_t(i)] >> 32);
        d.count = root_info[2 * size_t(i) + 1];
        if (d.count == 0 && d.height > 0) return false;  // empty tree with a tall root
        if (d.count > amt_span_host(d.bit_width, d.height + 1)) return false;
        d.lo = rlo < d.count ? rlo : d.count;
        d.hi = rhi < d.count ? rhi : d.count;
        if (d.count && d.lo >= d.hi) return false;  // nothing of this tree in the range
        if (d.count == 0) d.lo = d.hi = 0;
        return true;
    };
    bool try_dense = true;
    uint64_t n_leaves = 0;
    for (uint32_t i = 0; i < n_roots && try_dense; ++i) {
        try_dense = shape(i, lo, hi, plan.roots.r[i]);
        plan.roots.r[i].vkind = uint32_t(vkind);
        plan.roots.r[i].out_sel = want_keys ? 0u : 1u;
        plan.roots.r[i].out_off = n_leaves;
        n_leaves += plan.roots.r[i].hi - plan.roots.r[i].lo;
    }
    // the extra root joins when it is a dense candidate itself; otherwise the call goes on without it
    uint32_t n_use = n_roots;
    uint64_t n_extra = 0;
    if (has_extra && try_dense && shape(n_roots, extra_lo, extra_hi, plan.roots.r[n_roots])) {
        plan.roots.r[n_roots].vkind = uint32_t(extra_vkind);
        plan.roots.r[n_roots].out_sel = 2u;
        plan.roots.r[n_roots].out_off = 0;
        n_extra = plan.roots.r[n_roots].hi - plan.roots.r[n_roots].lo;
        n_use = n_all;
    }
    if (!try_dense) return;
    uint32_t max_height = 0;  // the tallest of the roots in use
    for (uint32_t i = 0; i < n_use; ++i) max_height = plan.roots.r[i].height > max_height ? plan.roots.r[i].height : max_height;
    if (max_height >= kMaxDenseLevels) return;
    uint64_t biggest = n_use;
    for (uint32_t level = 0; level <= max_height; ++level) {
        uint64_t nl = 0;
        for (uint32_t i = 0; i < n_use; ++i) nl += dense_nodes(plan.roots.r[i], level);
        if (nl >= 0x7fffffffULL) return;
        plan.n_level[level] = nl;
        biggest = nl > biggest ? nl : biggest;
    }
    if (n_leaves >= 0x7fffffffULL || n_extra >= 0x7fffffffULL || plan.n_level[max_height] != n_use) return;
    plan.ok = true;
    plan.n_use = n_use;
    plan.roots.n = n_use;
    plan.max_height = max_height;
    plan.n_leaves = n_leaves;
    plan.n_extra = n_extra;
    plan.biggest = biggest;
}

}  // namespace ipcfp

#undef IPCFP_DENSE_PLAN_FN
