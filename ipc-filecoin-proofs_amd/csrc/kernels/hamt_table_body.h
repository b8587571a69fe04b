// csrc/kernels/hamt_table_body.h — one block parsed as a HAMT node by ONE lane (hamt_table.h): the only item-by-item
// parse of the node grammar.  Its callers — the per-call node table (hamt_table_lane.hip) and the level-by-level walk's
// one-lane parse (hamt_levels.hip k_hamt_lv_parse) — differ in how a bucket entry is checked, which they pass in; the
// including unit configures the reader (IPCFP_LINE_STAGE).  The 32-lane outline (hamt_levels.hip) is the other producer
// of records and is held to this parse (tests/test_hamt_outline.py).
#pragma once
#include "cbor_dev.h"
#include "hamt_table.h"

namespace ipcfp {

// What a parse knows of its node, and the record that says so.
struct HamtNodeFacts {
    uint32_t status;     // 1: tabulated
    uint32_t kinds_ok;   // (0 when not tabulated)
    uint32_t std_links;
    uint32_t np;
    uint64_t bitfield;
};
__device__ __forceinline__ void hamt_rec_store(HamtNodeRec* __restrict__ out, const HamtNodeFacts& f) {
    out->status = uint8_t(f.status);
    out->kinds_ok = uint8_t(f.kinds_ok);
    out->np = uint8_t(f.np);
    out->pad = 0;
    out->std_links = f.std_links;
    out->bitfield = f.bitfield;
}

// One bucket value at r.pos: which typed decodes does it pass, where does it end?  The typed checks run on the reader
// itself (a failed attempt rewinds).  false: not even a well-formed item.
__device__ __forceinline__ bool value_kinds(Rd& r, uint32_t want, uint32_t& ok_kinds) {
    const uint32_t vstart = r.pos;
    ok_kinds = 0;
    if (want & HK_ACTOR_STATE) {
        check_actor_state(r);
        if (r.ok()) {
            ok_kinds = HK_ACTOR_STATE | HK_ANY;  // (an ActorState is no Vec<u8>: array(5) of a link …)
            return true;
        }
        r.err = 0;
        r.pos = vstart;
    }
    if (want & HK_VEC_U8) {
        check_vec_u8(r);
        if (r.ok()) {
            ok_kinds = HK_VEC_U8 | HK_ANY;
            return true;
        }
        r.err = 0;
        r.pos = vstart;
    }
    r.skip();
    ok_kinds = HK_ANY;
    return r.ok();
}

// The node table's kinds_ok before any bucket entry has narrowed it: the typed kinds asked for, and "any".
__device__ __forceinline__ uint32_t hamt_table_kinds_all(uint32_t kinds) { return (kinds & (HK_ACTOR_STATE | HK_VEC_U8)) | HK_ANY; }
// The node table's bucket-entry step: one `[key bytes, value]` at r.pos, kinds_ok narrowed to the typed checks (of `kinds`)
// the value passes; anything that is no such entry fails the reader.
struct HamtTableEntry {
    uint32_t kinds;
    __device__ __forceinline__ void operator()(Rd& r, uint32_t& kinds_ok) const {
        // A storage entry as every encoder writes it — `82 58 20 <32-byte slot>` and a Vec<u8> of one- and two-byte
        // elements — from two fetches and one more per four elements.  Item by item it is four heads and an element
        // loop, ≈ 2.7 k instructions, and one lane does that for the ≈ 8 entries of its node: 0.6 ms of configs[4]'s
        // call for k_hamt_node_table_lane (profiles/r06_experiments.md).  Anything else takes that way as before.
        if (kinds & HK_VEC_U8) {
            const uint32_t e0 = r.pos;
            if (e0 + 36u <= r.n && (r.peek64(e0) & 0xffffffull) == 0x205882ull) {
                const uint32_t end = vec_u8_end(r, e0 + 35u);
                if (end) {
                    r.pos = end;
                    kinds_ok &= HK_VEC_U8 | HK_ANY;
                    return;
                }
            }
        }
        r.expect_array(2);
        uint32_t ko, kl;
        r.read_bytes(ko, kl);
        if (!r.ok()) return;
        uint32_t vk;
        if (!value_kinds(r, kinds, vk)) {
            if (r.ok()) r.fail();
            return;
        }
        kinds_ok &= vk;
    }
};

// `[bitfield bytes(≤ 8), [≤ 32 pointers]]` at r, every pointer a well-formed link or a bucket of `[key bytes, value]` pairs
// → the record's fields, the pointers' offsets straight into out->ptr_off.  `entry(r, kinds_ok)` checks the bucket entry at
// r.pos and leaves r behind it or failed; kinds_ok starts as `kinds_all` and is what a tabulated node reports.
// A lane with nothing to parse is handed a reader of length 0: it fails at the first item head, before any store to
// ptr_off, so `out` is never touched for it and the caller only has to hold back hamt_rec_store.
template <class Entry>
__device__ __forceinline__ HamtNodeFacts hamt_node_parse(Rd& r, HamtNodeRec* __restrict__ out, uint32_t kinds_all, const Entry& entry) {
    HamtNodeFacts f{0, 0, 0, 0, 0};
    uint32_t kinds_ok = kinds_all;
    do {
        r.expect_array(2);
        uint32_t bo, bl;
        r.read_bytes(bo, bl);
        if (!r.ok() || bl > 8) break;
        for (uint32_t k = 0; k < bl; ++k) f.bitfield |= uint64_t(r.at(bo + bl - 1 - k)) << (8u * k);  // big-endian, last byte = bits 0..7
        const uint64_t np = r.read_array();
        if (!r.ok() || np > kHamtTablePointers) break;
        f.np = uint32_t(np);
        bool fits = true;
        for (uint32_t p = 0; p < f.np && r.ok(); ++p) {
            r.ensure_span(104);  // (a window-staged reader: the link, or the bucket's head and first entry, in one refill for all lanes)
            const uint32_t at = r.pos;
            fits = fits && at <= 0xffffu;
            out->ptr_off[p] = uint16_t(at);
            const uint32_t b0 = r.peek();
            if ((b0 >> 5) == 6) {
                uint32_t o, l;
                r.read_link(o, l);
                // the standard form: d8 2a | 58 27 | 00 | 01 71 a0 e4 02 20 | digest[32]
                if (r.ok() && l == 38 && o == at + 5 && r.peek64(at) == 0xa071010027582ad8ull &&
                    (r.peek64(at + 8) & 0xffffffull) == 0x2002e4ull)
                    f.std_links |= 1u << p;
            } else if ((b0 >> 5) == 4) {
                uint64_t nkv;
                if (b0 < 0x98u) {  // (the head of a short array is its one byte)
                    nkv = b0 - 0x80u;
                    r.pos += 1u;
                } else {
                    nkv = r.read_array();
                }
                for (uint64_t k = 0; k < nkv && r.ok(); ++k) {
                    if (k) r.ensure_span(104);
                    entry(r, kinds_ok);
                }
            } else {
                r.fail();
            }
        }
        r.finish();
        if (r.ok() && fits) {
            f.status = 1;
            f.kinds_ok = kinds_ok;
        }
    } while (false);
    return f;
}

}  // namespace ipcfp
