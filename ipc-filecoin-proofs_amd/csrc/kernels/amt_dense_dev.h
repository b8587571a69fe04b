// csrc/kernels/amt_dense_dev.h — the canonical spelling of a DENSE AMT node on the device: what the dense walk
// (amt_dense.hip) and the root loader of k_enum_roots (amt_enum.hip) both compare node bytes with.
//
// The node header is not parsed to find out where things are: with the shape known (m entries, the low m bitmap bits) the
// canonical spelling of the header is COMPUTED, the 16 bytes at the node's start are compared with it, and link k sits at
// `header + 43·k` — header and link are fetched side by side, one latency.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "walk_dev.h"

namespace ipcfp {

__device__ __forceinline__ uint64_t load_u64_any(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);  // one unaligned 8-byte load (gfx950 runs in unaligned-access mode)
    return v;
}

// The canonical header of an AMT node whose bitmap is the low m bits of a W-bit map: `83 | 4x bitmap | 8m (links) …` for a
// link node, `83 | 4x bitmap | 80 | 8m (values) …` for a leaf.  → its length (0: this route does not spell such a node)
// and its bytes as two little-endian words.
__device__ __forceinline__ uint32_t dense_header(uint32_t W, uint32_t m, bool leaf, uint64_t& h0, uint64_t& h1) {
    const uint32_t bl = (W + 7u) / 8u;
    h0 = h1 = 0;
    if (bl > 8u || m > 64u || m == 0u) return 0;
    uint32_t n = 0;
    auto put = [&](uint32_t byte) {  // (no byte array: a dynamically indexed one would live in scratch)
        if (n < 8u) h0 |= uint64_t(byte & 0xffu) << (8u * n);
        else h1 |= uint64_t(byte & 0xffu) << (8u * (n - 8u));
        ++n;
    };
    put(0x83);
    put(0x40u | bl);
    for (uint32_t i = 0; i < bl; ++i) {
        const uint32_t lo = i * 8u;
        put(m >= lo + 8u ? 0xffu : (m > lo ? (1u << (m - lo)) - 1u : 0u));
    }
    if (leaf) put(0x80);  // a leaf holds no links
    if (m < 24u) put(0x80u | m);
    else {
        put(0x98);
        put(m);
    }
    return n;
}
__device__ __forceinline__ bool header_matches(const uint8_t* node, uint32_t hdr, uint64_t h0, uint64_t h1) {
    const uint64_t g0 = load_u64_any(node), g1 = load_u64_any(node + 8);
    const uint64_t m0 = hdr >= 8 ? ~0ull : ((1ull << (8u * hdr)) - 1ull);
    const uint64_t m1 = hdr <= 8 ? 0ull : (hdr >= 16 ? ~0ull : ((1ull << (8u * (hdr - 8u))) - 1ull));
    return ((g0 ^ h0) & m0) == 0 && ((g1 ^ h1) & m1) == 0;
}
// the standard 43-byte link at p:   d8 2a | 58 27 | 00 | 01 71 a0 e4 02 20 | digest[32]
__device__ __forceinline__ bool std_link_at(const uint8_t* p) {
    return load_u64_any(p) == 0xa071010027582ad8ull && (load_u64_any(p + 8) & 0xffffffull) == 0x2002e4ull;
}
__device__ __forceinline__ CidKey std_link_key(const uint8_t* p) {
    CidKey k;
#pragma unroll
    for (int j = 0; j < 5; ++j) k.w[j] = load_u64_any(p + 5 + 8 * j);
    k.w[4] &= (1ull << 48) - 1ull;  // 38 = 4·8 + 6 bytes
    return k;
}

// Amt::load of a root whose node is the canonical dense LINK node: TRUE with `info` filled, or "not this shape" — the
// item-by-item amt_load then decides (and is the only one to report an error).
// The root block of a big list — `83 | height | count | node` (Amtv0) or `84 | bit width | height | count | node` (Amt) with
// the node a canonical dense LINK node: `83 | 4x bitmap = low m bits | 8m / 98 m | m standard 43-byte links | 80` and nothing
// behind it — settled from a dozen loads that do not depend on each other.  Exactly what amt_load accepts for these bytes
// (array heads, minimal uints, bitmap of the width's length whose popcount is the link count, well-formed links, no values,
// nothing after the node, height ≤ 64 / bit width); any other spelling or shape returns false and amt_load takes the block.
// Item by item the ten message-list roots and the receipts root of a tipset were 3.7 k instructions of ONE wavefront at
// 30-50 cycles each beside the side streams: 79 µs on the verify call's critical path (profiles/r04_final_timeline.txt).
__device__ __forceinline__ bool amt_load_dense_root(const WitnessView& w, const CidKey& root, int version, AmtRootInfo& info) {
    const uint32_t b = witness_find(w, root);
    if (b == kNoBlock) return false;
    const uint8_t* p = w.arena + w.off[b];
    const uint32_t len = w.len[b];
    if (len < 8u) return false;
    const uint64_t g0 = load_u64_any(p), g1 = load_u64_any(p + 8);  // (blocks sit on 128-byte lines with tail slack)
    auto byte_at = [&](uint32_t i) { return uint32_t((i < 8u ? g0 >> (8u * i) : g1 >> (8u * (i - 8u))) & 0xffull); };
    uint32_t pos = 1, bw = 3;
    if (version == 0) {
        if (byte_at(0) != 0x83u) return false;
    } else {
        if (byte_at(0) != 0x84u) return false;
        bw = byte_at(1);
        if (bw < 1u || bw > 6u) return false;  // (an immediate uint; the dense walk spells headers up to width 6)
        pos = 2;
    }
    const uint32_t height = byte_at(pos);
    if (height < 1u || height > 23u || height > 64u / bw) return false;  // immediate uint; a link node at the root
    ++pos;
    // count: a minimal unsigned integer
    const uint32_t cb = byte_at(pos);
    uint64_t count;
    uint32_t cl;
    if (cb < 0x18u) {
        count = cb;
        cl = 1;
    } else if (cb == 0x18u) {
        count = byte_at(pos + 1);
        cl = 2;
        if (count < 24u) return false;
    } else if (cb == 0x19u) {
        count = (uint64_t(byte_at(pos + 1)) << 8) | byte_at(pos + 2);
        cl = 3;
        if (count < 256u) return false;
    } else if (cb == 0x1au) {
        count = (uint64_t(byte_at(pos + 1)) << 24) | (uint64_t(byte_at(pos + 2)) << 16) | (uint64_t(byte_at(pos + 3)) << 8) | byte_at(pos + 4);
        cl = 5;
        if (count < 65536u) return false;
    } else {
        return false;  // (≥ 2^32 entries, or not an unsigned integer: the long way)
    }
    pos += cl;
    if (pos > 8u) return false;  // (cannot happen: 2 + 1 + 5)
    const uint32_t W = 1u << bw;
    const uint64_t span = amt_span(bw, height);  // indices under one link of the root
    if (count == 0 || span == ~0ULL) return false;
    const uint64_t m64 = (count + span - 1) / span;
    if (m64 > W) return false;  // (more entries than the height holds: not a dense tree)
    const uint32_t m = uint32_t(m64);
    uint64_t h0, h1;
    const uint32_t hdr = dense_header(W, m, false, h0, h1);
    const uint8_t* node = p + pos;
    const uint32_t end = pos + hdr + 43u * m + 1u;  // … links, then the empty values array
    if (hdr == 0 || end != len || !header_matches(node, hdr, h0, h1)) return false;
    bool ok = node[hdr + 43u * m] == 0x80u;
    for (uint32_t i = 0; i < m; ++i) ok = ok && std_link_at(node + hdr + 43u * i);
    if (!ok) return false;
    info.block = b;
    info.node_off = pos;
    info.bit_width = bw;
    info.height = height;
    info.count = count;
    return true;
}

}  // namespace ipcfp
