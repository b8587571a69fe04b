// csrc/kernels/amt_enum.h — level-synchronous `Amt::for_each` over the HBM-resident witness.
//
// The reference walks the big AMTs sequentially and depth-first
// (`bls_amt.for_each`, `secp_amt.for_each` src/proofs/events/utils.rs:76-90; the receipts list that
// drives `find_matching_events`, src/proofs/events/generator.rs:199-239).  Here every node of a level
// is decoded by its own lane, children are placed with a prefix sum so ascending-index order is
// preserved, and each node is decoded exactly once per pass.  Several AMTs (e.g. the BLS and secp
// trees of every parent block) are enumerated TOGETHER: roots lower than the tallest tree ride along
// as pass-through entries until their level comes up, so the output is the concatenation of the
// for_each sequences in root order.
//
// Errors: `for_each` aborts at the first failing node in depth-first order.  Every failure here is
// recorded as (sequence number, base index of the failing node, status code) packed into one u64
// and combined with atomicMin — the minimum IS the first failure in depth-first order, because a
// failing node has no descendants and every node with a smaller base index is visited earlier.
//
// Where what lives:
//   amt_dense_plan.h         the dense walk's plan (host arithmetic that sizes every buffer; compiles without HIP)
//   amt_dense_dev.h          the canonical spelling of a dense node, for the two units below
//   amt_dense.hip            the dense walk: its kernels and launch_dense_walk
//   amt_enum.hip             k_enum_roots, the general walk's kernels, k_check_dense, and their launchers
//   host/amt_enumerate.cpp   amt_enumerate and the witness's enumeration cache: host code over the launchers
#pragma once
#include <cstdint>
#include <vector>

#include "../common.h"
#include "amt_dense_plan.h"
#include "amt_types.h"
#include "walk_dev.h"

struct ipcfp_ctx;
struct ipcfp_witness;

namespace ipcfp {

// Host-side driver state: device buffers reused across levels.
struct AmtEnumResult {
    DevBuf<LeafRef> leaves;
    uint64_t n_leaves = 0;
    uint64_t error = kNoEnumError;  // packed first error (after the final sync)
    bool dense = false;             // every AMT held exactly the indices 0..count-1 (the dense walk succeeded)
    bool keys_written = false;      // the values (links) went to the caller's key buffer instead of `leaves`
};

// An enumeration may be restricted to the indices [lo, hi) (a receipt-range shard of one tipset):
// subtrees that hold no index of the range are neither resolved nor loaded — their blocks live in another
// shard's witness — while every node that is visited is validated completely.  Meant for ONE root.

// One more AMT riding along with a call (dense walk only): its spec is roots_d[n_roots], written by the caller
// or by a kernel queued before; its values have their own type and index range and go to a result of their own.
// `done` stays false when the dense walk did not take it (not dense, failed to load, anomaly): the caller then
// enumerates it by itself.  This is how the verify path walks the receipts AMT in the same launches as the
// message AMTs of the execution order instead of in a second chain of per-level launches.
struct EnumExtra {
    int vkind = 0;
    uint64_t lo = 0, hi = ~0ULL;
    AmtEnumResult* out = nullptr;
    bool done = false;
};

// ---- the dense walk (amt_dense.hip; plan: amt_dense_plan.h) ----
// what k_dense_link_leaves clears on the side (launch_dense_walk `clear`; only when the plan has key values)
struct DenseClear {
    unsigned long long* slots;  // n_slots × ~0
    uint64_t n_slots;
    uint32_t* words;            // n_words × 0
    uint64_t n_words;
};
// the extra root is a receipts tree and its leaves also write the receipts' event records (launch_dense_walk `receipts`):
// what k_receipt_events writes, from k_dense_receipt_leaves — one lane per receipt, the receipt read once
struct BlockRec;
struct ReceiptRec;
struct DenseReceiptOut {
    const BlockRec* brecs;     // k_block_events' records, ordered before the leaves on their stream
    ReceiptRec* rrecs;         // one per receipt of [lo, hi)
    uint32_t* counts;          // nullable: matches of the table's filter (kWalkPending where the table does not cover)
    unsigned long long* err;   // the missing events blocks' error word (set to kNoEnumError by the walk's first interior launch)
};
int launch_dense_walk(ipcfp_ctx* ctx, const WitnessView& view, const DenseNode* frontier, const DensePlan& plan,
                      DenseNode* a, DenseNode* b, LeafRef* leaves_main, CidKey* keys_main, LeafRef* leaves_extra, uint32_t* anomaly_d,
                      hipStream_t leaves_stream = nullptr,  // non-null (with fork_event): k_dense_leaves runs there, beside
                      hipEvent_t fork_event = nullptr,      // k_dense_link_leaves on the main stream
                      const DenseClear* clear = nullptr,
                      // non-null: the extra root's leaves take k_dense_receipt_leaves (a receipts tree), on the leaves' stream
                      const DenseReceiptOut* receipts = nullptr);

// ---- amt_enum.hip: every launcher enqueues on ctx->stream and returns without synchronising ----
// The roots → their frontier entries (general and dense form) and their shapes root_info_d[2t] = {height | bw << 32, count}
// (~0: the root did not load).  `mailbox` (pinned host, nullable): the shapes also go there, for a caller that queues the
// walk itself without draining the stream (host/verify_fast.cpp).  The launch shape follows from it:
//   mailbox == nullptr   div_up(n_all, 64) workgroups of 64 lanes, any number of roots (amt_enumerate);
//   mailbox != nullptr   ONE workgroup of 64 lanes, or of 128 when n_all > 64 — the kernel publishes the sequence number
//                        behind a __syncthreads, so every root must sit in that workgroup: at most 128 roots, else an error.
int launch_enum_roots(ipcfp_ctx* ctx, const WitnessView& view, const AmtRootSpec* roots_d, uint32_t n_all, int vkind,
                      EnumNode* frontier_d, unsigned long long* err_d, uint64_t* root_info_d, unsigned long long* mailbox,
                      unsigned long long mailbox_seq, DenseNode* dense_frontier_d);
// one level of the general walk.  counts_d[t]: entries frontier entry t gives the next level (level ≥ 1), or its values
// inside [lo, hi) (level 0) — then launch_scan_u32, and launch_enum_expand / launch_enum_emit place them
int launch_enum_count(ipcfp_ctx* ctx, const WitnessView& view, const EnumNode* frontier_d, uint32_t n, uint32_t level, int vkind,
                      uint32_t* counts_d, unsigned long long* err_d, uint64_t lo, uint64_t hi);
int launch_enum_expand(ipcfp_ctx* ctx, const WitnessView& view, const EnumNode* frontier_d, uint32_t n, uint32_t level,
                       const uint32_t* offsets_d, uint32_t total, EnumNode* next_d, unsigned long long* err_d, uint64_t lo, uint64_t hi);
int launch_enum_emit(ipcfp_ctx* ctx, const WitnessView& view, const EnumNode* frontier_d, uint32_t n, int vkind,
                     const uint32_t* counts_d, const uint32_t* offsets_d, LeafRef* leaves_d, uint64_t lo, uint64_t hi);
// *flag_d |= 1 unless leaves_d[i].index == first + i for every i
int launch_check_dense(ipcfp_ctx* ctx, const LeafRef* leaves_d, uint32_t n, uint64_t first, uint32_t* flag_d);

// ---- host/amt_enumerate.cpp ----
// Enumerate `n_roots` AMTs (device array `roots_d`) whose values have type `vkind`.
// `err_d` is a device u64 initialised by the caller (kNoEnumError or earlier-stage errors); the
// enumerator atomicMin's into it.  Three steps: the roots (one synchronisation: their shapes); the dense walk when the
// plan allows it (one more: anomaly flag + error word); otherwise — or after an anomaly — the general walk, level by
// level (one per level, and one for the error word).
int amt_enumerate(ipcfp_ctx* ctx, const WitnessView& view, const AmtRootSpec* roots_d, uint32_t n_roots, int vkind,
                  unsigned long long* err_d, AmtEnumResult& out, uint64_t lo = 0, uint64_t hi = ~0ULL,
                  DevBuf<CidKey>* keys_out = nullptr,  // VK_CID on the dense walk: the links as witness keys, no LeafRefs
                  EnumExtra* extra = nullptr);

// hand a finished enumeration of one AMT to the witness's cache (what amt_enumerate_cached would have produced)
int enum_cache_put(ipcfp_ctx* ctx, ipcfp_witness* w, const CidKey& root, int version, int vkind, uint64_t lo, uint64_t hi,
                   AmtEnumResult& en);

// Enumerate one AMT of the witness, or return the cached enumeration (owned by the witness; valid
// until ipcfp_witness_rebuild_index).
int amt_enumerate_cached(ipcfp_ctx* ctx, ipcfp_witness* w, const CidKey& root, int version, int vkind,
                         const EnumCached** out, uint64_t lo = 0, uint64_t hi = ~0ULL);

}  // namespace ipcfp
