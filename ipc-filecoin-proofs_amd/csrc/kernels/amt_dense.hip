// csrc/kernels/amt_dense.hip — the DENSE walk of `Amt::for_each`: the kernels and their launcher (plan: amt_dense_plan.h).
//
// With the shape of every tree known from its root there is nothing to count or prefix-sum: ONE kernel per level (the
// children's lanes validate the parent between them, every lane resolves its own link) and ONE leaf kernel that validates
// and emits.  Anything that is not exactly that shape — a sparse node, a lying count, a missing block, a decode error —
// raises `anomaly` and the caller redoes the walk with the general level-synchronous route (amt_enum.hip), which also knows
// how to order errors.
//
// Every lane's work is a short chain of DEPENDENT memory latencies — the levels are a few thousand lanes at most — so
// what these kernels are made for is the number of hops, not bytes or instructions:
//   * a frontier entry (DenseNode) carries the arena offset and length of its node, so a child's lane starts reading its
//     parent without asking the off / len tables first;
//   * the node header is compared with its computed canonical spelling and the lane's own link sits at `header + 43·k`
//     (amt_dense_dev.h) — header and link are fetched side by side, one latency;
//   * after the hash slot, the candidate block's CID, offset and length are fetched side by side as well.
// Three hops per level (node bytes → hash slot → block facts) instead of six.  Anything that is not spelled
// canonically — a non-minimal length, a bit width above 6, a link that is not the standard 43 bytes — is an anomaly.
#include <hip/hip_runtime.h>

#include "../common.h"
#include "amt_dense_dev.h"
#include "amt_enum.h"
#include "event_table.h"

namespace ipcfp {

// which root does frontier entry j of `level` belong to (dense trees side by side), and where do its entries start?
struct DenseWhere {
    DenseRoot dr;
    uint32_t upper_off, here_off;
};
__device__ __forceinline__ DenseWhere dense_where(const DenseRoot* roots, uint32_t j, uint32_t level_here) {
    DenseWhere o;
    uint32_t r = 0;
    o.upper_off = o.here_off = 0;
    o.dr = roots[0];
    uint64_t n_here = dense_nodes(o.dr, level_here);
    while (j >= o.here_off + n_here) {
        o.here_off += uint32_t(n_here);
        o.upper_off += uint32_t(dense_nodes(o.dr, level_here + 1));
        o.dr = roots[++r];
        n_here = dense_nodes(o.dr, level_here);
    }
    return o;
}

// A node of links — an interior node, or a leaf whose values are links — is validated BY ITS LINKS' LANES, each lane a
// share: every lane the header (W-bit map, the low m bits set), lane k link k (at header + 43·k → `mine`: right iff links
// 0..k-1 are standard 43-byte links, which lanes 0..k-1 say of theirs), lane m-1 what follows the last link — in an
// interior node an empty values array, in a leaf nothing; and, when the node is a `whole` block, the end of the block.
// A node on the edge of the range has links without a lane: the first / last lane it does have stands in for them
// (edge_first / edge_last).  Together: everything CollapsedNode::expand checks.  → does this lane's share hold?
__device__ __forceinline__ bool dense_link_share(const uint8_t* node, uint32_t rem, uint32_t whole, uint32_t W, uint32_t m, uint32_t k,
                                                 bool edge_first, bool edge_last, bool leaf, uint32_t& mine) {
    uint64_t h0, h1;
    const uint32_t hdr = dense_header(W, m, leaf, h0, h1);
    mine = hdr + 43u * k;
    bool ok = hdr != 0 && mine + 43u <= rem && header_matches(node, hdr, h0, h1) && std_link_at(node + mine);
    if (ok && edge_first)
        for (uint32_t i = 0; i < k && ok; ++i) ok = std_link_at(node + hdr + 43u * i);
    if (ok && edge_last)
        for (uint32_t i = k + 1; i < m && ok; ++i) ok = hdr + 43u * (i + 1u) <= rem && std_link_at(node + hdr + 43u * i);
    if (ok && (k == m - 1 || edge_last)) {
        const uint32_t tail = hdr + 43u * m;
        if (leaf) ok = !whole || tail == rem;  // nothing after the last value
        else ok = tail + 1u <= rem && node[tail] == 0x80u && (!whole || tail + 1u == rem);  // the values array: empty
    }
    return ok;
}

// frontier entering `level` (≥ 1) → frontier entering level-1; one lane per child
__device__ __forceinline__ void dense_level_one(const WitnessView& w, const DenseNode* __restrict__ cur, const DenseRoot* roots,
                                                uint32_t level, uint32_t j, DenseNode* __restrict__ next,
                                                uint32_t* __restrict__ anomaly) {
    const DenseWhere wh = dense_where(roots, j, level - 1);
    const DenseRoot& dr = wh.dr;
    if (dr.height < level) {  // rides along
        next[j] = cur[wh.upper_off];
        return;
    }
    const uint64_t q = dense_first(dr, level - 1) + (j - wh.here_off);  // absolute node number on the child level
    const uint32_t W = 1u << dr.bit_width;
    const uint64_t p = q >> dr.bit_width;
    const uint32_t k = uint32_t(q) & (W - 1u);
    const DenseNode e = cur[wh.upper_off + uint32_t(p - dense_first(dr, level))];
    DenseNode c{0, e.base + uint64_t(k) * amt_span(dr.bit_width, level), kNoBlock, 0, e.seq, 1};
    if (e.block == kNoBlock) {
        next[j] = c;
        return;
    }
    const uint64_t remaining = dense_total(dr, level - 1) - p * W;
    const uint32_t m = remaining < W ? uint32_t(remaining) : W;  // links this parent must hold
    // a parent on the edge of the range has children without a lane: the first / last lane it does have stands in
    const uint64_t n_here = dense_nodes(dr, level - 1);
    const bool edge_first = j == wh.here_off && k > 0;
    const bool edge_last = j + 1 == wh.here_off + n_here && k + 1 < m;
    const uint8_t* node = w.arena + e.goff;
    uint32_t mine;
    if (!dense_link_share(node, e.rem, e.whole, W, m, k, edge_first, edge_last, /*leaf=*/false, mine)) {
        atomicOr(anomaly, 1u);
        next[j] = c;
        return;
    }
    const CidKey key = std_link_key(node + mine);
    // Blockstore::get: hash slot, then the candidate's CID, offset and length side by side
    uint32_t s = cid_hash(key) & w.mask;
    for (;;) {
        const uint32_t b = w.slots[s];
        if (b == kNoBlock) {
            atomicOr(anomaly, 1u);  // a missing block: the general route names it
            break;
        }
        const CidKey have = load_cid_slot(w.cids, b);
        const uint64_t off = w.off[b];
        const uint32_t len = w.len[b];
        if (cid_equal(have, key)) {
            if (w.touched) atomicOr(&w.touched[b >> 5], 1u << (b & 31));
            c.block = b;
            c.goff = off;
            c.rem = len;
            break;
        }
        s = (s + 1) & w.mask;
    }
    next[j] = c;
}

// `set_err` (non-null on the walk's first interior launch): the receipt records' error word, set to kNoEnumError here — ahead
// of k_dense_receipt_leaves by stream order, without a fill of its own on the leaves' stream
__global__ __launch_bounds__(256) void k_dense_level(WitnessView w, const DenseNode* __restrict__ cur, const DenseRoots roots_arg,
                                                     uint32_t level, uint32_t n_next, DenseNode* __restrict__ next,
                                                     uint32_t* __restrict__ anomaly, unsigned long long* __restrict__ set_err) {
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (set_err && j == 0) *set_err = kNoEnumError;
    if (j < n_next) dense_level_one(w, cur, roots_arg.r, level, j, next, anomaly);
}

// The NARROW interior levels at the top of the trees (a few hundred entries: 14, 71 and 495 for the 1M-receipt tipset) in ONE
// launch of ONE workgroup, a __syncthreads between levels — the frontier of a level is written and read back by this
// workgroup alone, so workgroup-scope ordering is all it needs; no grid barrier (the persistent all-levels form lost to its
// barriers: launch_dense_walk).  What a level of so few entries costs beside K1 and the event parse is not its three
// dependent loads but getting a workgroup ONTO the chip (k_enum_roots: one wavefront, 29 loads, 40-55 µs in the step): here
// that is paid once for the levels together.  `n[i]`: entries of the frontier entering level_hi - 1 - i.
struct DenseTopCounts {
    uint32_t n[8];
};
__global__ __launch_bounds__(256) void k_dense_top(WitnessView w, const DenseNode* frontier, const DenseRoots roots_arg, uint32_t level_hi,
                                                   uint32_t n_levels, DenseTopCounts counts, DenseNode* a, DenseNode* b,
                                                   uint32_t* __restrict__ anomaly, unsigned long long* __restrict__ set_err) {
    if (set_err && threadIdx.x == 0) *set_err = kNoEnumError;  // (as k_dense_level)
    const DenseNode* src = frontier;
    for (uint32_t i = 0; i < n_levels; ++i) {
        const uint32_t n_next = counts.n[i];
        for (uint32_t j = threadIdx.x; j < n_next; j += blockDim.x) dense_level_one(w, src, roots_arg.r, level_hi - i, j, a, anomaly);
        __syncthreads();  // (the level's entries are in place for every wavefront of the workgroup)
        src = a;
        DenseNode* t = a;
        a = b;
        b = t;
    }
}

// leaf level of the trees whose values are LINKS taken as witness keys (Amtv0<Cid>: the message lists) — one lane per
// VALUE.  The leaf is validated by its values' lanes exactly as an interior node by its children's (dense_link_share).
__global__ __launch_bounds__(256) void k_dense_link_leaves(WitnessView w, const DenseNode* __restrict__ cur, const DenseRoots roots_arg,
                                                           uint32_t n_key_roots, uint64_t n_values, uint32_t* __restrict__ anomaly,
                                                           CidKey* __restrict__ keys_main, DenseClear clear) {
    const uint64_t v = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    // (a passenger: the execution order's hash table and first-occurrence flags, which the kernels right behind this one
    // fill, are cleared by this grid instead of by two fill kernels of their own in front of them)
    {
        const uint64_t stride = uint64_t(gridDim.x) * blockDim.x;
        for (uint64_t j = v; j < clear.n_slots; j += stride) clear.slots[j] = ~0ull;
        for (uint64_t j = v; j < clear.n_words; j += stride) clear.words[j] = 0u;
    }
    if (v >= n_values) return;
    // which root (the key trees come first among the roots), which value
    const DenseRoot* roots = roots_arg.r;
    uint32_t r = 0, node_off0 = 0;
    uint64_t voff = 0;
    DenseRoot dr = roots[0];
    while (r + 1 < n_key_roots && v >= voff + (dr.hi - dr.lo)) {
        voff += dr.hi - dr.lo;
        node_off0 += uint32_t(dense_nodes(dr, 0));
        dr = roots[++r];
    }
    const uint64_t idx = dr.lo + (v - voff);
    const uint32_t W = 1u << dr.bit_width;
    const uint64_t pnode = idx >> dr.bit_width;
    const uint32_t k = uint32_t(idx) & (W - 1u);
    const DenseNode e = cur[node_off0 + uint32_t(pnode - dense_first(dr, 0))];
    if (e.block == kNoBlock) return;  // reported where the link failed to resolve
    const uint64_t remaining = dr.count - pnode * W;
    const uint32_t m = remaining < W ? uint32_t(remaining) : W;
    const bool edge_first = idx == dr.lo && k > 0;
    const bool edge_last = idx + 1 == dr.hi && k + 1 < m;
    const uint8_t* node = w.arena + e.goff;
    uint32_t mine;
    if (!dense_link_share(node, e.rem, e.whole, W, m, k, edge_first, edge_last, /*leaf=*/true, mine)) {
        atomicOr(anomaly, 1u);
        return;
    }
    keys_main[dr.out_off + (idx - dr.lo)] = std_link_key(node + mine);
}

// leaf level of every other tree: one lane per leaf node validates it in one pass and writes its values' locations
__global__ __launch_bounds__(256) void k_dense_leaves(WitnessView w, const DenseNode* __restrict__ cur, const DenseRoots roots_arg,
                                                      uint32_t n_nodes, uint32_t first_node, LeafRef* __restrict__ leaves_main,
                                                      uint32_t* __restrict__ anomaly, LeafRef* __restrict__ leaves_extra) {
    const uint32_t t = first_node + blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_nodes) return;
    const DenseWhere wh = dense_where(roots_arg.r, t, 0);
    const DenseRoot& dr = wh.dr;
    if (dr.out_sel == 0 && dr.count != 0) return;  // (a key tree with values: k_dense_link_leaves validates its leaves)
    const uint64_t leaf_off = dr.out_off;
    const int vkind = int(dr.vkind);
    LeafRef* const leaves = dr.out_sel == 1 ? leaves_main : (dr.out_sel == 2 ? leaves_extra : nullptr);
    const uint64_t p = dense_first(dr, 0) + (t - wh.here_off);  // absolute leaf-node number
    const DenseNode e = cur[t];
    const uint32_t W = 1u << dr.bit_width;
    const uint64_t remaining = dr.count - p * W;
    const uint32_t m = remaining < W ? uint32_t(remaining) : W;
    // Whatever happens to this node, every LeafRef it is responsible for is WRITTEN (kNoBlock when there is no value): the
    // kernels queued behind — before the host has seen the anomaly flag — read them (host/verify_fast.cpp).
    auto blank = [&]() {
        if (!leaves) return;
        for (uint32_t i = 0; i < m; ++i) {
            const uint64_t idx = p * W + i;
            if (idx >= dr.lo && idx < dr.hi) leaves[leaf_off + (idx - dr.lo)] = LeafRef{kNoBlock, 0, 0, e.seq, idx};
        }
    };
    if (e.block == kNoBlock) {  // reported where the link failed to resolve
        blank();
        return;
    }
    const uint32_t node_off = uint32_t(e.goff - w.off[e.block]);  // (LeafRefs are relative to the block)
    Rd rd;
    rd.init(w.arena + e.goff, e.rem);
    rd.expect_array(3);
    uint32_t bo, bl;
    rd.read_bytes(bo, bl);
    bool ok = rd.ok() && bl == (W + 7) / 8;
    if (ok) {  // bitmap = the low m bits (bits at or above the width do not count when W < 8)
        for (uint32_t i = 0; i < bl; ++i) {
            const uint32_t lo = i * 8u;
            uint32_t want = m >= lo + 8 ? 0xffu : (m > lo ? (1u << (m - lo)) - 1u : 0u);
            uint32_t have = rd.at(bo + i);
            if (W < 8) have &= (1u << W) - 1u;
            ok = ok && have == want;
        }
    }
    ok = ok && rd.read_array() == 0;  // a leaf holds no links
    const uint64_t nv = rd.read_array();
    ok = ok && rd.ok() && nv == m;
    // every value of the node is type-checked (serde decodes the whole node); the ones inside [lo, hi) are emitted
    for (uint32_t i = 0; ok && i < m; ++i) {
        const uint32_t start = rd.pos;
        const uint64_t idx = p * W + i;
        check_value(rd, vkind);
        ok = rd.ok();
        if (ok && leaves && idx >= dr.lo && idx < dr.hi)
            leaves[leaf_off + (idx - dr.lo)] = LeafRef{e.block, node_off + start, rd.pos - start, e.seq, e.base + i};
    }
    if (ok && e.whole) {
        rd.finish();
        ok = rd.ok();
    }
    if (!ok) {
        atomicOr(anomaly, 1u);
        blank();
    }
}

// The receipt value at `s` of a node — `84 | exit code | return data | gas used | null or the standard 43-byte link` —
// settled from its heads: where it ends, or 0 when it is not spelled so (the caller then takes the reader).  What it
// accepts is exactly what check_receipt accepts for those bytes, ending at the same place: an exit code of at most four
// argument bytes (so a u32), a return-data length of at most four, the gas of any width, the events root null or the
// standard link (read_link's fast form, `root` = true: the link ends the value).  Every byte it looks at lies in front of
// the end it returns, and that end is ≤ rem — so bytes behind `rem` can only make it refuse.  `f8(i)`: the 8 bytes at node
// byte i, little-endian; it is asked for at most 24 bytes behind a position < rem.  Two dependent fetches: the value's start,
// then the bytes behind the return data.
template <class F8>
__device__ __forceinline__ uint32_t receipt_value_fast(const F8& f8, uint32_t s, uint32_t rem, bool& root) {
    root = false;
    if (s >= rem) return 0;
    const uint64_t a0 = f8(s), a1 = f8(s + 8u);
    auto ab = [&](uint32_t i) { return uint32_t((i < 8u ? a0 >> (8u * i) : a1 >> (8u * (i - 8u))) & 0xffull); };
    auto extra = [](uint32_t info) { return info < 24u ? 0u : (info == 24u ? 1u : (info == 25u ? 2u : (info == 26u ? 4u : (info == 27u ? 8u : 99u)))); };
    if (ab(0) != 0x84u) return 0;
    uint32_t b = ab(1);
    uint32_t x = extra(b & 31u);
    if ((b >> 5) != 0u || x > 4u) return 0;  // exit code: an unsigned integer of at most 4 argument bytes
    const uint32_t p = 2u + x;
    b = ab(p);  // the return data: a byte string
    x = extra(b & 31u);
    if ((b >> 5) != 2u || x > 4u) return 0;
    uint64_t len = b & 31u;
    if (x == 1u) len = ab(p + 1u);
    else if (x == 2u) len = (ab(p + 1u) << 8) | ab(p + 2u);
    else if (x == 4u) len = (uint64_t(ab(p + 1u)) << 24) | (ab(p + 2u) << 16) | (ab(p + 3u) << 8) | ab(p + 4u);
    const uint64_t g = uint64_t(s) + p + 1u + x + len;  // gas used
    if (g >= rem) return 0;
    const uint64_t c0 = f8(uint32_t(g)), c1 = f8(uint32_t(g) + 8u), c2 = f8(uint32_t(g) + 16u);
    auto cw = [&](uint32_t i) {  // the 8 bytes at byte i of the window c0 c1 c2 (zeros behind it)
        const uint32_t sh = 8u * (i & 7u);
        const uint64_t lo = i < 8u ? c0 : (i < 16u ? c1 : c2), hi = i < 8u ? c1 : (i < 16u ? c2 : 0ull);
        return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
    };
    b = uint32_t(c0 & 0xffu);
    x = extra(b & 31u);
    if ((b >> 5) != 0u || x > 8u) return 0;
    const uint32_t q = 1u + x;
    const uint64_t t0 = cw(q);
    uint64_t end;
    if ((t0 & 0xffu) == 0xf6u) {
        end = g + q + 1u;  // no events root
    } else {
        if (t0 != 0xa071010027582ad8ull || (cw(q + 8u) & 0xffffffull) != 0x2002e4ull) return 0;
        end = g + q + 43u;
        root = true;
    }
    return end <= rem ? uint32_t(end) : 0u;
}

// Leaf level of the RECEIPTS tree on the verify call's table route (host/verify_fast.cpp): a GROUP of G = min(W, 64) lanes
// per leaf node, lane k for value k — where k_dense_leaves takes one lane per leaf node (its values decoded one after the
// other) and k_receipt_events then reads every receipt a second time.  The group
//   * stages the node in LDS (up to kReceiptStageBytes per value, less 16): one 16-byte load per lane and step, the group's
//     loads side by side over the node;
//   * compares the canonical leaf header (the low m bitmap bits, no links, m values) and finds every value's start in ONE
//     pass over the stage — each lane makes the same pass, so the starts need no sharing: receipt_value_fast validates a
//     value from its heads, the reader on global memory takes what it refuses (check_value(VK_RECEIPT)), so every value of
//     the node is type-checked, those in front of or behind the range included, and behind the last one the end of the block;
//   * then resolves, every lane at once, the events root of its value to the block's record (k_block_events) and writes
//     the LeafRef, the ReceiptRec and, when the table carries a filter, the match count — what k_receipt_events wrote.
// A node larger than its stage is walked the same way on global memory.  Anything else raises `anomaly`; every slot is
// written whatever happens (kNoBlock / RK_WALK): the kernels queued behind read them before the host has seen the flag.
// (the receipts root travels alone: DenseRoots indexed at run time would sit in scratch)
__global__ __launch_bounds__(256) void k_dense_receipt_leaves(WitnessView w, const DenseNode* __restrict__ cur, const DenseRoot dr,
                                                              uint32_t node_off0, uint32_t n_nodes, uint32_t* __restrict__ anomaly,
                                                              LeafRef* __restrict__ leaves, DenseReceiptOut out) {
    extern __shared__ uint64_t receipt_stage[];
    const uint32_t W = 1u << dr.bit_width, G = receipt_leaf_group(dr.bit_width);  // (G divides the workgroup: groups sit in one wavefront)
    const uint32_t gid = (blockIdx.x * blockDim.x + threadIdx.x) / G, j = threadIdx.x & (G - 1u);
    if (gid >= n_nodes) return;  // (whole groups)
    uint64_t* const st = receipt_stage + (threadIdx.x / G) * receipt_stage_words(G);
    const uint64_t pnode = dense_first(dr, 0) + gid;
    const DenseNode e = cur[node_off0 + gid];
    const uint64_t remaining = dr.count - pnode * W;
    const uint32_t m = remaining < W ? uint32_t(remaining) : W;
    uint64_t h0, h1;
    const uint32_t hdr = dense_header(W, m, true, h0, h1);  // (0 for W > 64: no lane has a value of its own then)
    const bool live = e.block != kNoBlock;                  // (else: reported where the link failed to resolve)
    bool ok = live && hdr != 0 && hdr < e.rem;
    const uint8_t* node = w.arena + e.goff;
    const uint32_t sh = uint32_t(e.goff & 15u);
    const bool staged = ok && e.rem <= G * kReceiptStageBytes - 16u;  // (the same for the whole group)
    if (staged) {  // chunks [0, n_ch) of the 16-byte-aligned lines under the node (blocks sit on 128-byte lines)
        const ulonglong2* src = reinterpret_cast<const ulonglong2*>(node - sh);
        const uint32_t n_ch = (sh + e.rem + 15u) / 16u;  // ≤ G · kReceiptStageBytes / 16
        ulonglong2 v[kReceiptStageBytes / 16u];
#pragma unroll
        for (uint32_t i = 0; i < kReceiptStageBytes / 16u; ++i)
            if (j + G * i < n_ch) v[i] = src[j + G * i];
#pragma unroll
        for (uint32_t i = 0; i < kReceiptStageBytes / 16u; ++i)
            if (j + G * i < n_ch) {
                st[2u * (j + G * i)] = v[i].x;
                st[2u * (j + G * i) + 1u] = v[i].y;
            }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    const auto f8_stage = [&](uint32_t i) __attribute__((always_inline)) {
        const uint32_t q = sh + i, r = 8u * (q & 7u);
        const uint64_t lo = st[q >> 3], hi = st[(q >> 3) + 1u];
        return r ? (lo >> r) | (hi << (64u - r)) : lo;
    };
    const auto f8_global = [&](uint32_t i) __attribute__((always_inline)) { return load_u64_any(node + i); };
    // the pass over the node: header, every value, the end; this lane keeps where its own value k = j lies
    uint32_t start = 0, stop = 0;
    bool mine_fast = false, mine_root = false;
    const auto pass = [&](const auto& f8) __attribute__((always_inline)) {
        const uint64_t g0 = f8(0u), g1 = f8(8u);
        const uint64_t m0 = hdr >= 8 ? ~0ull : ((1ull << (8u * hdr)) - 1ull);
        const uint64_t m1 = hdr <= 8 ? 0ull : (hdr >= 16 ? ~0ull : ((1ull << (8u * (hdr - 8u))) - 1ull));
        ok = ((g0 ^ h0) & m0) == 0 && ((g1 ^ h1) & m1) == 0;  // header_matches
        Rd rd;
        rd.init(node, e.rem);
        uint32_t pos = hdr;
        for (uint32_t i = 0; ok && i < m; ++i) {
            bool root;
            uint32_t end = receipt_value_fast(f8, pos, e.rem, root);
            const bool fast = end != 0u;
            if (!fast) {  // a spelling the heads do not settle: the reader decides
                rd.pos = pos;
                check_value(rd, VK_RECEIPT);
                ok = rd.ok();
                end = rd.pos;
            }
            if (i == j) {
                start = pos;
                stop = end;
                mine_fast = fast;
                mine_root = root;
            }
            pos = end;
        }
        if (ok && e.whole) ok = pos == e.rem;  // nothing after the last value
    };
    if (staged) pass(f8_stage);
    else if (ok) pass(f8_global);
    if (live && !ok) atomicOr(anomaly, 1u);
    // this lane's value: the events root, from the stage when the heads settled the value, else from the reader
    CidKey ev_root;
    bool has_root = false;
    if (ok && j < m) {
        if (mine_fast) {
            has_root = mine_root;
            if (has_root) {  // std_link_key of the link that ends the value
#pragma unroll
                for (int q = 0; q < 5; ++q) ev_root.w[q] = staged ? f8_stage(stop - 38u + 8u * q) : f8_global(stop - 38u + 8u * q);
                ev_root.w[4] &= (1ull << 48) - 1ull;
            }
        } else {
            Rd rd;
            rd.init(node, e.rem);
            rd.pos = start;
            rd.expect_array(4);
            if (rd.read_uint() > 0xffffffffULL) rd.fail();  // exit_code: u32
            uint32_t o, l;
            rd.read_bytes(o, l);
            (void)rd.read_uint();
            if (rd.at_null()) {
                rd.read_null();
            } else {  // (a CID longer than a witness key: the general walk folds it — no Blake2b in this kernel)
                uint32_t co, cl;
                rd.read_link(co, cl);
                if (cl > 40u) rd.fail();
                has_root = rd.ok();
                if (has_root) ev_root = rd.key_at(co, cl);
            }
            ok = rd.ok() && rd.pos == stop;  // (the pass's reader took this value already: it ends where the pass said)
            if (!ok) atomicOr(anomaly, 1u);
        }
    }
    // every slot of the range this lane answers for (one, value j, unless W > 64: then the node is an anomaly)
    for (uint32_t k = j; k < m; k += G) {
        const uint64_t idx = pnode * W + k;
        if (idx < dr.lo || idx >= dr.hi) continue;
        const uint32_t t = uint32_t(idx - dr.lo);
        LeafRef lr{kNoBlock, 0, 0, e.seq, idx};
        ReceiptRec rr{RK_WALK, 0, 0, kNoBlock, 0};
        uint32_t c = 0;
        if (ok && k == j) {
            lr = LeafRef{e.block, uint32_t(e.goff - w.off[e.block]) + start, stop - start, e.seq, e.base + k};
            rr.kind = RK_NO_EVENTS;
            if (has_root) {
                const uint32_t b = witness_find(w, ev_root);
                rr.block = b;
                if (b == kNoBlock) {
                    rr.kind = IPCFP_ST_ERR_MISSING_BLOCK;
                    atomicMin(out.err, (unsigned long long)pack_enum_error(1, t, rr.kind));
                } else {
                    const BlockRec br = out.brecs[b];
                    if ((br.kind_matches & 0xffu) == RK_TABLE) {
                        rr.kind = RK_TABLE;
                        rr.first = br.first;
                        rr.bitmap = br.bitmap;
                        c = br.kind_matches >> 8;
                    } else {
                        rr.kind = RK_WALK;
                        c = kWalkPending;
                    }
                }
            }
        }
        leaves[dr.out_off + t] = lr;
        out.rrecs[t] = rr;
        if (out.counts) out.counts[t] = c;
    }
}

// The launches of the dense walk: the interior levels, then the leaf kernels.  `frontier`: the roots' entries
// (k_enum_roots); a / b: two frontier buffers of plan.biggest entries.  The root shapes travel as a kernel argument.
int launch_dense_walk(ipcfp_ctx* ctx, const WitnessView& view, const DenseNode* frontier, const DensePlan& plan,
                      DenseNode* a, DenseNode* b, LeafRef* leaves_main, CidKey* keys_main, LeafRef* leaves_extra, uint32_t* anomaly_d,
                      hipStream_t leaves_stream, hipEvent_t fork_event, const DenseClear* clear, const DenseReceiptOut* receipts) {
    const DenseNode* src = frontier;
    // (All interior levels as ONE persistent launch — a workgroup per CU, a grid barrier per level — was built and is
    // slower: 382 µs against 238 µs for the six launches.  What stretches a level beside K1 and the event parse is the
    // latency of its three dependent loads under their memory traffic, not the dispatch; a barrier adds an L2
    // write-back and an L1 invalidate per level on top.  profiles/r03_experiments.md)
    uint32_t level_from = plan.max_height;
    unsigned long long* set_err = receipts ? receipts->err : nullptr;  // (taken by the first interior launch)
    {   // the narrow levels at the top (at most kDenseTopMax entries each): one launch (k_dense_top)
        DenseTopCounts counts{};
        uint32_t n_top = 0;
        while (n_top < 8 && level_from - n_top >= 1 && plan.n_level[level_from - n_top - 1] <= kDenseTopMax) {
            counts.n[n_top] = uint32_t(plan.n_level[level_from - n_top - 1]);
            ++n_top;
        }
        if (n_top >= 2) {  // (one level alone is k_dense_level's)
            hipLaunchKernelGGL(k_dense_top, dim3(1), dim3(256), 0, ctx->stream, view, src, plan.roots, level_from, n_top, counts, a, b, anomaly_d,
                               set_err);
            set_err = nullptr;
            // the last level written: a for an odd number of levels, b for an even one — and the next writes the other
            if (n_top & 1u) {
                src = a;
                DenseNode* t = a;
                a = b;
                b = t;
            } else {
                src = b;
            }
            level_from -= n_top;
        }
    }
    for (uint32_t level = level_from; level >= 1; --level) {
        const uint32_t nn = uint32_t(plan.n_level[level - 1]);
        hipLaunchKernelGGL(k_dense_level, dim3(div_up(nn, 256)), dim3(256), 0, ctx->stream, view, src, plan.roots, level, nn, a, anomaly_d,
                           set_err);
        set_err = nullptr;
        src = a;
        DenseNode* t = a;
        a = b;
        b = t;  // `src` now lives in b; the next level writes a
    }
    // the key trees (links taken as witness keys) come first among the roots: one lane per value; every other tree: one
    // lane per leaf node
    uint32_t n_key_roots = 0;
    uint64_t n_key_values = 0;
    while (n_key_roots < plan.n_use && plan.roots.r[n_key_roots].out_sel == 0) {
        n_key_values += plan.roots.r[n_key_roots].hi - plan.roots.r[n_key_roots].lo;
        ++n_key_roots;
    }
    for (uint32_t i = n_key_roots; i < plan.n_use; ++i)
        if (plan.roots.r[i].out_sel == 0) return set_error(ctx, IPCFP_E_INVALID, "dense walk: the key trees must come first");
    // The two leaf kernels read the same frontier and write different outputs.  A caller whose consumers sit on two
    // streams (host/verify_fast.cpp: the message keys feed the execution-order kernels on the main stream, the receipt
    // leaves feed k_receipt_events on the aux stream) forks here: k_dense_leaves goes to `leaves_stream`, ordered behind
    // the last interior level by `fork_event`, and runs beside k_dense_link_leaves instead of after it.
    if (set_err) IPCFP_HIP(ctx, hipMemsetAsync(set_err, 0xff, sizeof *set_err, ctx->stream));  // (no interior level: the roots are leaves)
    hipStream_t ls = ctx->stream;
    if (leaves_stream && leaves_stream != ctx->stream && fork_event) {
        IPCFP_HIP(ctx, hipEventRecord(fork_event, ctx->stream));
        IPCFP_HIP(ctx, hipStreamWaitEvent(leaves_stream, fork_event, 0));
        ls = leaves_stream;
    }
    // (every leaf node gets a lane here: those of key trees that have values leave at once, an EMPTY key tree's root is
    // validated here — no value lane looks at it)
    const uint32_t n_nodes = uint32_t(plan.n_level[0]);
    if (receipts) {  // the receipts tree (the extra root, the last one) by its values; the nodes in front of it by nodes when
                     // one of them is not a key tree with values (an empty message list's root)
        const uint32_t ri = plan.n_use - 1;
        const DenseRoot& rr = plan.roots.r[ri];
        if (ri < n_key_roots || rr.out_sel != 2 || rr.vkind != VK_RECEIPT || !leaves_extra)
            return set_error(ctx, IPCFP_E_INVALID, "dense walk: the receipt records want a receipts tree as the extra root");
        const uint32_t r_nodes = uint32_t(dense_nodes(rr, 0)), before = n_nodes - r_nodes;
        bool node_lanes = ri > n_key_roots;
        for (uint32_t i = 0; i < n_key_roots; ++i) node_lanes = node_lanes || plan.roots.r[i].count == 0;
        if (node_lanes)
            hipLaunchKernelGGL(k_dense_leaves, dim3(div_up(before, 256)), dim3(256), 0, ls, view, src, plan.roots, before, 0u,
                               leaves_main, anomaly_d, nullptr);
        if (rr.hi > rr.lo) {  // a group of lanes per leaf node, its stage in LDS
            const uint32_t G = receipt_leaf_group(rr.bit_width);
            hipLaunchKernelGGL(k_dense_receipt_leaves, dim3(div_up(uint64_t(r_nodes) * G, 256)), dim3(256),
                               (256u / G) * receipt_stage_words(G) * sizeof(uint64_t), ls, view, src, rr, before, r_nodes, anomaly_d,
                               leaves_extra, *receipts);
        } else  // (an empty receipts tree: its root node is validated the node way; there is no record to write)
            hipLaunchKernelGGL(k_dense_leaves, dim3(div_up(r_nodes, 256)), dim3(256), 0, ls, view, src, plan.roots, n_nodes, before,
                               leaves_main, anomaly_d, leaves_extra);
    } else {
        hipLaunchKernelGGL(k_dense_leaves, dim3(div_up(n_nodes, 256)), dim3(256), 0, ls, view, src, plan.roots, n_nodes, 0u,
                           leaves_main, anomaly_d, leaves_extra);
    }
    if (clear && !n_key_values) {  // (no lane to take the passenger)
        if (clear->n_slots) IPCFP_HIP(ctx, hipMemsetAsync(clear->slots, 0xff, clear->n_slots * 8, ctx->stream));
        if (clear->n_words) IPCFP_HIP(ctx, hipMemsetAsync(clear->words, 0, clear->n_words * 4, ctx->stream));
    }
    if (n_key_values)
        hipLaunchKernelGGL(k_dense_link_leaves, dim3(div_up(n_key_values, 256)), dim3(256), 0, ctx->stream, view, src, plan.roots,
                           n_key_roots, n_key_values, anomaly_d, keys_main, clear ? *clear : DenseClear{nullptr, 0, nullptr, 0});
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
