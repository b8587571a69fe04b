// csrc/kernels/tipset_prologue_body.h — the ONE text of the tipset prologue: what `verify_single_proof` derives from
// (parent_tipset_cids, child_block_cid) before it looks at a proof.  The header facts (verify_header_consistency,
// src/proofs/events/verifier.rs:147-181) and, per parent block, its header, its TxMeta, the TxMeta's re-hash and the two
// message-AMT roots (reconstruct_execution_order / collect_exec_list, src/proofs/events/utils.rs:16-30,48-94), with the
// first-error order of that traversal:
//   error sequence numbers: parent header b → b;  TxMeta of block b → P + 3b;  its BLS AMT → P + 3b + 1;  its secp AMT
//   → P + 3b + 2 — so every parent header counts before the first TxMeta.
// One single-wavefront workgroup per slot: the wavefront opens the block, the lead lane parses it.  Written against `Rd`
// and the CBOR / header helpers only (no walk primitives, like tipset_ctx.h), so each including unit instantiates it with
// its own reader (cbor_dev.h IPCFP_RD_LDS): the LDS prologue (tipset_prepare.hip) and the general form
// (tipset_prepare_general.hip).  What differs between them is passed in:
//   the opener  opener(w, block) → bool, called by EVERY lane of the wavefront: the block is open and opener.reader() —
//               the lead lane's — reads it; or false: it does not fit this unit's stage.  The body then leaves the slot
//               through opener.overflow(c, slot), with nothing of the slot reported or stored;
//   the keys    flags / n_parents / child / parent(i) of the tipset key (TipsetKeysInline, TipsetKeysCtx below);
//   TxMetaMode  what becomes of the TxMeta's re-hash.
#pragma once
#include "amt_types.h"
#include "cbor_dev.h"
#include "claims_dev.h"
#include "header_dev.h"
#include "tipset_ctx.h"
#include "txmeta_dev.h"

namespace ipcfp {

// put_cbor(&(bls_root, secp_root), Blake2b256) must give the CID the header named (utils.rs:65-72) …
enum TxMetaMode : int {
    kTxMetaCheck = 0,  // … checked here, on the lead lane (reconstruct_execution_order: the verify path always checks)
    kTxMetaDefer = 1,  // … left to k_txmeta_rehash (tipset_prepare_general.hip): txmeta_block[b] = block + 1 (tipset_ctx.h); inline keys only
    kTxMetaNone = 2,   // … never compared: the generator's build_execution_order (utils.rs:44)
};

// the tipset key as the inputs' head: a kernel argument, or the context's own head in device memory
struct TipsetKeysInline {
    const TipsetInputs& in;
    __device__ __forceinline__ uint32_t flags() const { return in.flags; }
    __device__ __forceinline__ uint32_t n_parents() const { return in.n_parents; }
    __device__ __forceinline__ const CidKey& child() const { return in.child; }
    __device__ __forceinline__ const CidKey& parent(uint32_t i) const { return in.parents[i]; }
};
// … and of a context that may hold a wide key (tipset_parent)
struct TipsetKeysCtx {
    const TipsetCtxDev& c;
    __device__ __forceinline__ uint32_t flags() const { return c.flags; }
    __device__ __forceinline__ uint32_t n_parents() const { return c.n_parents; }
    __device__ __forceinline__ const CidKey& child() const { return c.child; }
    __device__ __forceinline__ CidKey parent(uint32_t i) const { return tipset_parent(c, i); }
};

// TxMeta = (Cid, Cid)  (utils.rs:61): the two links' CID bytes; false: not that
__device__ __forceinline__ bool txmeta_links(Rd& r, uint32_t& o0, uint32_t& l0, uint32_t& o1, uint32_t& l1) {
    r.expect_array(2);
    r.read_link(o0, l0);
    r.read_link(o1, l1);
    r.finish();
    return r.ok();
}

// slots 0 / 1: the child header (with `child_hdr.parents != parent_cids`) / the first parent header.
// `receipts_spec` (nullable, child part): where to leave the receipts AMT as an enumeration root, so that the enumerator
// takes it along with the message AMTs without the host having seen the header (amt_enum.h EnumExtra).
template <class Keys, class Opener>
__device__ __forceinline__ void prologue_headers(const WitnessView& w, const Keys& keys, TipsetCtxDev& c, bool child_part,
                                                 Opener& opener, AmtRootSpec* receipts_spec) {
    const bool lead = threadIdx.x == 0;
    const bool parsed = (keys.flags() & (TC_PARENTS_PARSED | TC_CHILD_PARSED)) == (TC_PARENTS_PARSED | TC_CHILD_PARSED);
    uint32_t status = IPCFP_ST_ERR_BAD_CLAIM, match = 0;
    long long height = 0;
    const bool wanted = parsed && (child_part || keys.n_parents() > 0);
    if (wanted) {
        // child header (verifier.rs:155-158) / parent_cids[0] (:171-174)
        const uint32_t hb = witness_find(w, child_part ? keys.child() : keys.parent(0));  // uniform across the wavefront
        if (hb == kNoBlock) {
            status = IPCFP_ST_ERR_MISSING_BLOCK;
        } else {
            if (!opener(w, hb)) return opener.overflow(c, child_part ? 0u : 1u);
            if (lead) {
                Rd r = opener.reader();
                HeaderLite h;
                status = decode_header(r, h);
                if (status == IPCFP_ST_TRUE) {
                    height = h.height;
                    if (child_part) {
                        c.receipts_root = h.parent_message_receipts;
                        // `child_hdr.parents != parent_cids` (:161): same count, same CIDs in order
                        bool same = h.n_parents == keys.n_parents();
                        if (same) {
                            Rd q = r;
                            q.err = 0;
                            q.pos = h.parents_off;
                            for (uint32_t i = 0; i < keys.n_parents() && same; ++i) {
                                CidKey k;
                                q.read_link_key(k);
                                same = q.ok() && cid_equal(k, keys.parent(i));
                            }
                        }
                        match = same ? 1u : 0u;
                    }
                }
            }
        }
    }
    if (!lead) return;
    if (child_part) {
        c.child_status = status;
        c.parents_match = match;
        c.child_height = height;
        if (receipts_spec) {  // the receipts AMT as an enumeration root
            AmtRootSpec rs{};
            rs.version = 0;  // Amtv0<Receipt>
            rs.kind_p1 = uint32_t(VK_RECEIPT) + 1u;
            rs.skip = status == IPCFP_ST_TRUE ? 0u : 1u;
            if (!rs.skip) rs.root = c.receipts_root;
            *receipts_spec = rs;
        }
    } else {
        c.parent0_status = status;
        c.parent0_height = height;
    }
}

// slot 2 + b: parent block b → its header, its TxMeta, its two message-AMT roots.  Wave-uniform: every lane reaches every
// barrier, only the lead lane parses and reports.  `err` must hold kNoEnumError or earlier errors on entry.
// A block that does not fit: NOTHING was reported or stored for this slot (header fit, TxMeta did not: the same).
template <class Keys, class Opener>
__device__ __forceinline__ void prologue_roots(const WitnessView& w, const Keys& keys, TipsetCtxDev& c,
                                               AmtRootSpec* __restrict__ roots, unsigned long long* __restrict__ err, uint32_t b,
                                               Opener& opener, TxMetaMode mode) {
    __shared__ CidKey s_tx;
    __shared__ uint32_t s_have_tx;
    const uint32_t P = keys.n_parents();
    if (b >= P) return;
    const bool lead = threadIdx.x == 0;
    auto fail = [&](uint32_t seq, uint32_t code) { atomicMin(err, (unsigned long long)pack_enum_error(seq, 0, code)); };
    // reconstruct_execution_order (utils.rs:20-27): the parent header
    if (lead) s_have_tx = 0;
    const uint32_t hb = witness_find(w, keys.parent(b));
    if (hb == kNoBlock) {
        if (lead) fail(b, IPCFP_ST_ERR_MISSING_BLOCK);
    } else {
        if (!opener(w, hb)) return opener.overflow(c, 2u + b);
        if (lead) {
            Rd hr = opener.reader();
            HeaderLite h;
            const uint32_t st = decode_header(hr, h);
            if (st == IPCFP_ST_TRUE) {
                s_tx = h.messages;
                s_have_tx = 1;
            } else {
                fail(b, st);
            }
        }
    }
    __syncthreads();  // s_tx / s_have_tx; and the header's stage is free again
    // collect_exec_list (utils.rs:56-91)
    const uint32_t seq = P + 3 * b;
    AmtRootSpec bls{}, secp{};
    bls.version = secp.version = 0;
    bls.seq = seq + 1;
    secp.seq = seq + 2;
    bls.skip = secp.skip = 1;
    if (s_have_tx) {
        const CidKey tx = s_tx;
        const uint32_t tb = witness_find(w, tx);  // :58-60
        if (tb == kNoBlock) {
            if (lead) fail(seq, IPCFP_ST_ERR_MISSING_BLOCK);
        } else {
            if (!opener(w, tb)) return opener.overflow(c, 2u + b);
            if (lead) {
                Rd r = opener.reader();
                uint32_t o0, l0, o1, l1;
                if (!txmeta_links(r, o0, l0, o1, l1)) {
                    fail(seq, IPCFP_ST_ERR_DECODE);
                } else if (mode != kTxMetaCheck) {
                    // The re-hash — re-encode, one Blake2b compression on ONE lane, ≈ 3 k instructions — gates nothing: it
                    // only ever adds an error.  Deferred, a launch of its own on the aux stream does it (k_txmeta_rehash),
                    // joined at the end of the call; a mismatch reaches the same error word with the same sequence number.
                    if (mode == kTxMetaDefer) c.txmeta_block[b] = tb + 1u;
                    bls.root = r.key_any(o0, l0);
                    secp.root = r.key_any(o1, l1);
                    bls.skip = secp.skip = 0;
                } else {
                    // put_cbor(&(bls_root, secp_root), Blake2b256): canonical re-encoding, hashed (:65-72)
                    CidKey re;
                    txmeta_rehash(r, o0, l0, o1, l1, re);
                    if (!cid_equal(re, tx)) {
                        fail(seq, IPCFP_ST_ERR_TXMETA_MISMATCH);
                    } else {
                        bls.root = r.key_any(o0, l0);
                        secp.root = r.key_any(o1, l1);
                        bls.skip = secp.skip = 0;
                    }
                }
            }
        }
    }
    if (lead) {
        roots[2 * b] = bls;
        roots[2 * b + 1] = secp;
    }
}

}  // namespace ipcfp
