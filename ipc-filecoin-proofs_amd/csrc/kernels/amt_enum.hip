// csrc/kernels/amt_enum.hip — `Amt::for_each`: the roots (k_enum_roots) and the general level-synchronous walk, with their
// launchers (amt_enum.h).  The dense walk is amt_dense.hip; the host side that strings the launches together is
// host/amt_enumerate.cpp.
#include "amt_enum.h"

#include <hip/hip_runtime.h>

#include "../common.h"
#include "amt_dense_dev.h"
#include "launch.h"

namespace ipcfp {

__device__ __forceinline__ void enum_error(unsigned long long* err, uint32_t seq, uint64_t base, uint32_t code) {
    atomicMin(err, (unsigned long long)pack_enum_error(seq, base, code));
}

// one root → its frontier entry and its shape {height | bw << 32, count} (~0: the root did not load)
__device__ __forceinline__ void enum_root_one(const WitnessView& w, const AmtRootSpec& spec, int vkind, EnumNode* __restrict__ slot,
                                              unsigned long long* __restrict__ err, uint64_t& info0, uint64_t& info1,
                                              DenseNode* __restrict__ dense_slot) {
    EnumNode e{kNoBlock, 0, 0, spec.seq, 0, 0, 0};
    DenseNode d{0, 0, kNoBlock, 0, spec.seq, 0};
    info0 = ~0ULL;  // dead
    info1 = 0;
    if (!spec.skip) {
        AmtRootInfo info;
        const uint32_t st = amt_load_dense_root(w, spec.root, int(spec.version), info)
                                ? uint32_t(IPCFP_ST_TRUE)
                                : amt_load(w, spec.root, int(spec.version), spec.kind_p1 ? int(spec.kind_p1) - 1 : vkind, info);
        if (st != IPCFP_ST_TRUE) {
            if (!spec.kind_p1) enum_error(err, spec.seq, 0, st);  // (the extra root: left to its own enumeration)
        } else {
            e.block = info.block;
            e.node_off = info.node_off;
            e.height = uint16_t(info.height);
            e.bit_width = uint8_t(info.bit_width);
            info0 = uint64_t(uint32_t(info.height)) | (uint64_t(info.bit_width) << 32);
            info1 = info.count;
            d.block = info.block;
            d.goff = w.off[info.block] + info.node_off;
            d.rem = w.len[info.block] - info.node_off;
        }
    }
    *slot = e;
    if (dense_slot) *dense_slot = d;
}

// roots → frontier (one entry per root, in root order)
__global__ __launch_bounds__(128) void k_enum_roots(WitnessView w, const AmtRootSpec* __restrict__ roots, uint32_t n,
                                                   int vkind, EnumNode* __restrict__ frontier,
                                                   unsigned long long* __restrict__ err,
                                                   uint64_t* __restrict__ root_info /* n × {height|bw<<32, count} */,
                                                   unsigned long long* __restrict__ mailbox, unsigned long long mailbox_seq,
                                                   DenseNode* __restrict__ dense_frontier) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    uint64_t info0 = ~0ULL, info1 = 0;
    if (t < n) {
        enum_root_one(w, roots[t], vkind, frontier + t, err, info0, info1, dense_frontier ? dense_frontier + t : nullptr);
        root_info[2 * t] = info0;
        root_info[2 * t + 1] = info1;
    }
    // The mailbox (host/verify_fast.cpp): PINNED HOST memory the device writes while the stream keeps going.  The root
    // shapes are all the host needs to size and queue the rest of the walk, so it polls these words instead of draining
    // the stream with a synchronisation: [0] = sequence number (written last), [1 + 2t ..] = the shapes.  Single-block
    // launches only (n ≤ 128 roots: 2 · IPCFP_MAX_PARENTS + 1 fit), so that "every root is through" is a __syncthreads.
    if (mailbox && gridDim.x == 1) {
        if (t < n) {
            __hip_atomic_store(mailbox + 1 + 2 * t, (unsigned long long)info0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(mailbox + 2 + 2 * t, (unsigned long long)info1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
        __threadfence_system();
        __syncthreads();
        if (threadIdx.x == 0) __hip_atomic_store(mailbox, mailbox_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// decode the node of entry e (validating it completely); false ⇒ decode error
__device__ __forceinline__ bool enum_read_node(const WitnessView& w, const EnumNode& e, int vkind, AmtNode& nd) {
    Rd r = open_block(w, e.block);
    r.pos = e.node_off;
    amt_read_node(r, e.bit_width, vkind, ~0u, nd);
    if (e.node_off == 0) r.finish();
    return r.ok();
}

// An index range [lo, hi) restricts an enumeration to the values inside it (a receipt-range shard of one tipset,
// SURVEY.md §8e): a child whose span does not meet the range is not counted, not resolved and not loaded — its
// block belongs to another shard's witness.  Nodes that ARE visited are still validated completely.
struct EnumRange {
    uint64_t lo, hi;
};
__device__ __forceinline__ bool span_meets(uint64_t base, uint64_t span, const EnumRange& rg) {
    const uint64_t end = base + span < base ? ~0ULL : base + span;  // saturating
    return base < rg.hi && end > rg.lo;
}
// slots of node `e` (bitmap in nd) whose child span meets the range
__device__ __forceinline__ uint32_t links_in_range(const AmtNode& nd, const EnumNode& e, const EnumRange& rg) {
    const uint64_t span = amt_span(e.bit_width, e.height);
    uint32_t c = 0;
    for (uint32_t sub = 0; sub < nd.width; ++sub)
        if (nd.bit(sub) && span_meets(e.base + uint64_t(sub) * span, span, rg)) ++c;
    return c;
}

// interior level L ≥ 1: how many entries does each frontier entry contribute to the next level?
__global__ __launch_bounds__(256) void k_enum_count(WitnessView w, const EnumNode* __restrict__ frontier, uint32_t n,
                                                    uint32_t level, int vkind, uint32_t* __restrict__ counts,
                                                    unsigned long long* __restrict__ err, EnumRange rg) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const EnumNode e = frontier[t];
    uint32_t c = 0;
    if (e.block != kNoBlock) {
        if (e.leaf_ready || e.height < level) {
            c = 1;  // rides along
        } else {
            AmtNode nd;
            if (!enum_read_node(w, e, vkind, nd)) enum_error(err, e.seq, e.base, IPCFP_ST_ERR_DECODE);
            else c = nd.nlinks ? links_in_range(nd, e, rg) : 1;  // a Leaf above height 0 is carried down as-is
        }
    }
    counts[t] = c;
}

// One lane per OUTPUT entry (child): lane j finds its parent with a binary search over the exclusive
// offsets, steps over the links before its own (the node was validated by k_enum_count) and resolves
// one link.  A node's 8-32 children are thus resolved by as many lanes side by side instead of one lane
// chasing 8-32 hash probes in sequence.
__global__ __launch_bounds__(256) void k_enum_expand(WitnessView w, const EnumNode* __restrict__ frontier, uint32_t n,
                                                     uint32_t level, const uint32_t* __restrict__ offsets,
                                                     uint32_t total, EnumNode* __restrict__ next,
                                                     unsigned long long* __restrict__ err, EnumRange rg) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    // parent = last t with offsets[t] <= j  (entries that contribute nothing share their successor's offset)
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offsets[mid] <= j) lo = mid;
        else hi = mid;
    }
    EnumNode e = frontier[lo];
    const uint32_t k = j - offsets[lo];
    if (e.leaf_ready || e.height < level) {  // rides along (k == 0)
        next[j] = e;
        return;
    }
    Rd r = open_block(w, e.block);
    r.pos = e.node_off;
    r.expect_array(3);
    uint32_t bo, bl;
    r.read_bytes(bo, bl);
    const uint64_t nl = r.read_array();
    if (nl == 0) {  // a Leaf above height 0: carried down as-is
        e.leaf_ready = 1;
        next[j] = e;
        return;
    }
    // the k-th set bit whose child meets the range names the slot; step over the links before ours
    const uint64_t span = amt_span(e.bit_width, e.height);
    uint32_t sub = 0, seen = 0, before = 0;
    for (;; ++sub) {
        if ((r.at(bo + (sub >> 3)) >> (sub & 7)) & 1u) {
            if (span_meets(e.base + uint64_t(sub) * span, span, rg)) {
                if (seen == k) break;
                ++seen;
            }
            ++before;
        }
    }
    for (uint32_t q = 0; q < before; ++q) {
        uint32_t m;
        uint64_t a;
        r.head(m, a);  // tag 42
        r.head(m, a);  // byte-string header
        r.pos += uint32_t(a);
    }
    CidKey key;
    r.read_link_key(key);
    EnumNode c{kNoBlock, 0, e.base + uint64_t(sub) * span, e.seq, uint16_t(e.height - 1), e.bit_width, 0};
    const uint32_t b = witness_find(w, key);
    if (b == kNoBlock) enum_error(err, e.seq, c.base, IPCFP_ST_ERR_MISSING_BLOCK);
    else c.block = b;
    next[j] = c;
}

// leaf level: number of values per entry
__global__ __launch_bounds__(256) void k_enum_count_leaf(WitnessView w, const EnumNode* __restrict__ frontier,
                                                         uint32_t n, int vkind, uint32_t* __restrict__ counts,
                                                         unsigned long long* __restrict__ err, EnumRange rg) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const EnumNode e = frontier[t];
    uint32_t c = 0;
    if (e.block != kNoBlock) {
        AmtNode nd;
        if (!enum_read_node(w, e, vkind, nd)) enum_error(err, e.seq, e.base, IPCFP_ST_ERR_DECODE);
        else if (nd.nlinks) enum_error(err, e.seq, e.base, IPCFP_ST_ERR_DECODE);  // link node at height 0
        else
            for (uint32_t sub = 0; sub < nd.width; ++sub)
                if (nd.bit(sub) && e.base + sub >= rg.lo && e.base + sub < rg.hi) ++c;
    }
    counts[t] = c;
}

__global__ __launch_bounds__(256) void k_enum_emit(WitnessView w, const EnumNode* __restrict__ frontier, uint32_t n,
                                                   int vkind, const uint32_t* __restrict__ counts,
                                                   const uint32_t* __restrict__ offsets,
                                                   LeafRef* __restrict__ leaves, EnumRange rg) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    if (counts[t] == 0) return;
    const EnumNode e = frontier[t];
    const uint32_t o = offsets[t];
    Rd r = open_block(w, e.block);
    r.pos = e.node_off;
    r.expect_array(3);
    uint32_t bo, bl;
    r.read_bytes(bo, bl);
    (void)r.read_array();  // no links in a leaf
    const uint64_t nv = r.read_array();
    uint32_t sub = 0, k = 0;
    for (uint64_t j = 0; j < nv; ++j) {
        while (!((r.at(bo + (sub >> 3)) >> (sub & 7)) & 1u)) ++sub;
        const uint32_t start = r.pos;
        check_value(r, vkind);
        if (e.base + sub >= rg.lo && e.base + sub < rg.hi) leaves[o + k++] = LeafRef{e.block, start, r.pos - start, e.seq, e.base + sub};
        ++sub;
    }
}

// does leaf i hold index first + i for every i?  (the cache's density flag of an enumeration by the general walk)
__global__ __launch_bounds__(256) void k_check_dense(const LeafRef* __restrict__ leaves, uint32_t n, uint64_t first,
                                                     uint32_t* __restrict__ flag) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool bad = i < n && leaves[i].index != first + uint64_t(i);
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// ---- launchers (amt_enum.h) ----

int launch_enum_roots(ipcfp_ctx* ctx, const WitnessView& view, const AmtRootSpec* roots_d, uint32_t n_all, int vkind,
                      EnumNode* frontier_d, unsigned long long* err_d, uint64_t* root_info_d, unsigned long long* mailbox,
                      unsigned long long mailbox_seq, DenseNode* dense_frontier_d) {
    if (n_all == 0 || (mailbox && n_all > 128)) return set_error(ctx, IPCFP_E_INVALID, "launch_enum_roots: %u roots", n_all);
    // with a mailbox: ONE workgroup (the kernel's "every root is through" is a __syncthreads)
    const dim3 grid(mailbox ? 1u : div_up(n_all, 64)), block(mailbox && n_all > 64 ? 128 : 64);
    hipLaunchKernelGGL(k_enum_roots, grid, block, 0, ctx->stream, view, roots_d, n_all, vkind, frontier_d, err_d, root_info_d, mailbox,
                       mailbox_seq, dense_frontier_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_enum_count(ipcfp_ctx* ctx, const WitnessView& view, const EnumNode* frontier_d, uint32_t n, uint32_t level, int vkind,
                      uint32_t* counts_d, unsigned long long* err_d, uint64_t lo, uint64_t hi) {
    const EnumRange rg{lo, hi};
    if (level >= 1)
        hipLaunchKernelGGL(k_enum_count, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, view, frontier_d, n, level, vkind, counts_d,
                           err_d, rg);
    else
        hipLaunchKernelGGL(k_enum_count_leaf, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, view, frontier_d, n, vkind, counts_d,
                           err_d, rg);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_enum_expand(ipcfp_ctx* ctx, const WitnessView& view, const EnumNode* frontier_d, uint32_t n, uint32_t level,
                       const uint32_t* offsets_d, uint32_t total, EnumNode* next_d, unsigned long long* err_d, uint64_t lo, uint64_t hi) {
    hipLaunchKernelGGL(k_enum_expand, dim3(div_up(total, 256)), dim3(256), 0, ctx->stream, view, frontier_d, n, level, offsets_d, total,
                       next_d, err_d, EnumRange{lo, hi});
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_enum_emit(ipcfp_ctx* ctx, const WitnessView& view, const EnumNode* frontier_d, uint32_t n, int vkind,
                     const uint32_t* counts_d, const uint32_t* offsets_d, LeafRef* leaves_d, uint64_t lo, uint64_t hi) {
    hipLaunchKernelGGL(k_enum_emit, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, view, frontier_d, n, vkind, counts_d, offsets_d,
                       leaves_d, EnumRange{lo, hi});
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_check_dense(ipcfp_ctx* ctx, const LeafRef* leaves_d, uint32_t n, uint64_t first, uint32_t* flag_d) {
    hipLaunchKernelGGL(k_check_dense, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, leaves_d, n, first, flag_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
