// tests/native/dense_plan_harness.cpp — TEST INFRASTRUCTURE.  The plan of the dense AMT walk
// (csrc/kernels/amt_dense_plan.h: the host arithmetic that sizes every buffer the walk's kernels write) behind a C
// interface, compiled for the host alone.  tests/test_dense_plan.py holds it to a restatement written in the test.
#include <cstdint>
#include <vector>

#include "../../ipc-filecoin-proofs_amd/csrc/kernels/amt_dense_plan.h"

using namespace ipcfp;

extern "C" {

// out: kMaxDenseRoots, kMaxDenseLevels, kDenseTopMax, IPCFP_MAX_PARENTS
void dense_plan_limits(uint32_t* out) {
    out[0] = kMaxDenseRoots;
    out[1] = kMaxDenseLevels;
    out[2] = kDenseTopMax;
    out[3] = IPCFP_MAX_PARENTS;
}

// root_info: n_words words, two per root as k_enum_roots writes them ({height | bw << 32, count}; ~0: a dead root).
// scalars: ok, n_use, max_height, n_leaves, n_extra, biggest, roots.n;  n_level: kMaxDenseLevels words;
// roots: kMaxDenseRoots × {height, bit_width, count, lo, hi, vkind, out_sel, out_off}.  Returns plan.ok.
int dense_plan_run(const uint64_t* root_info, uint32_t n_words, uint32_t n_roots, int vkind, int want_keys, uint64_t lo, uint64_t hi,
                   uint32_t has_extra, int extra_vkind, uint64_t extra_lo, uint64_t extra_hi, uint64_t* scalars, uint64_t* n_level,
                   uint64_t* roots) {
    const std::vector<uint64_t> info(root_info, root_info + n_words);
    DensePlan plan;
    dense_plan(info, n_roots, vkind, want_keys != 0, lo, hi, has_extra, extra_vkind, extra_lo, extra_hi, plan);
    scalars[0] = plan.ok ? 1 : 0;
    scalars[1] = plan.n_use;
    scalars[2] = plan.max_height;
    scalars[3] = plan.n_leaves;
    scalars[4] = plan.n_extra;
    scalars[5] = plan.biggest;
    scalars[6] = plan.roots.n;
    for (uint32_t l = 0; l < kMaxDenseLevels; ++l) n_level[l] = plan.n_level[l];
    for (uint32_t i = 0; i < kMaxDenseRoots; ++i) {
        const DenseRoot& r = plan.roots.r[i];
        uint64_t* o = roots + 8 * size_t(i);
        o[0] = r.height;
        o[1] = r.bit_width;
        o[2] = r.count;
        o[3] = r.lo;
        o[4] = r.hi;
        o[5] = r.vkind;
        o[6] = r.out_sel;
        o[7] = r.out_off;
    }
    return plan.ok ? 1 : 0;
}

// the per-root functions the kernels index their frontiers with: {dense_total, dense_first, dense_nodes} of `level`
void dense_root_level(uint32_t height, uint32_t bit_width, uint64_t count, uint64_t lo, uint64_t hi, uint32_t level, uint64_t* out) {
    const DenseRoot r{height, bit_width, count, lo, hi, 0, 0, 0};
    out[0] = dense_total(r, level);
    out[1] = dense_first(r, level);
    out[2] = dense_nodes(r, level);
}

// the receipts tree's leaf kernel: lanes per leaf node, words of LDS per group
void receipt_leaf_launch(uint32_t bit_width, uint32_t* out) {
    out[0] = receipt_leaf_group(bit_width);
    out[1] = receipt_stage_words(out[0]);
}

}  // extern "C"
