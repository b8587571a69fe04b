// csrc/kernels/verify_events.hip — batch `verify_event_proof`: tipset-context preparation,
// execution-order reconstruction, and one proof per lane.
//
// Replaces src/proofs/events/verifier.rs:51-290 and src/proofs/events/utils.rs:16-30,48-94.
// Check order and every Ok(false)/Err outcome follow SURVEY.md A.10; the status byte names the
// reference line that decided.
#define IPCFP_LINE_STAGE 1  // k_verify_events parses whole blocks front to back: see cbor_dev.h
#include <hip/hip_runtime.h>

#include "../common.h"
#include "blake2b_dev.h"
#include "claims_dev.h"
#include "event_log_dev.h"
#include "walk_dev.h"
#include "amt_enum.h"
#include "event_table.h"
#include "tipset_ctx.h"
#include "types_dev.h"
#include "launch.h"
#include "scan_dev.h"
#include "verify_dev.h"

namespace ipcfp {

// stage 2: leaf values (tag-42 links, already validated) → message CID keys
__global__ __launch_bounds__(256) void k_exec_keys(WitnessView w, const LeafRef* __restrict__ leaves, uint32_t n,
                                                   CidKey* __restrict__ keys) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const LeafRef l = leaves[t];
    Rd r;
    r.init(w.arena + w.off[l.block] + l.off, l.len);
    CidKey k;
    r.read_link_key(k);
    keys[t] = k;
}

// stage 3: `seen.insert(c)` — the table keeps, per distinct CID, the SMALLEST raw position.
// A slot is one u64: fingerprint (low half of the key's 64-bit hash) in the high word, raw position in the low
// word.  A probe compares fingerprints first and reads the 40-byte key behind a slot only when they agree — at load
// 0.5 half of all inserts pass an occupied slot, and each of those used to be a random 40-byte read.

__global__ __launch_bounds__(256) void k_exec_insert(const CidKey* __restrict__ keys, uint32_t n,
                                                     unsigned long long* __restrict__ slots, uint32_t mask) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const CidKey key = keys[i];
    const uint64_t h = cid_hash64(key);
    const unsigned long long mine = ((unsigned long long)uint32_t(h) << 32) | i;
    uint32_t s = uint32_t(h >> 32) & mask;
    for (;;) {
        unsigned long long cur = slots[s];
        if (cur == kEmptySlot64) {
            cur = atomicCAS(&slots[s], kEmptySlot64, mine);
            if (cur == kEmptySlot64) return;
        }
        if (uint32_t(cur >> 32) == uint32_t(h) && cid_equal(keys[uint32_t(cur)], key)) {
            atomicMin(&slots[s], mine);  // same fingerprint: the minimum is the smaller position
            return;
        }
        s = (s + 1) & mask;
    }
}

// stages 3+4 in ONE probe per position (host/verify_fast.cpp): `first` (zeroed by the caller) is kept right while the
// table fills.  A position that takes an empty slot counts itself; one that lowers a slot's minimum counts itself and
// un-counts the position it displaced.  Additions commute, so whatever order the wavefronts run in, the holder of each
// slot's final minimum ends at 1 and every other position of that CID at 0 — the second random probe of every position
// (k_exec_first: another 128-byte line apiece) becomes a streaming read of the flags.
// (as in k_index_insert, the probe is the compare-and-swap itself)
__global__ __launch_bounds__(256) void k_exec_insert_flags(const CidKey* __restrict__ keys, uint32_t n,
                                                           unsigned long long* __restrict__ slots, uint32_t mask,
                                                           uint32_t* __restrict__ first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const CidKey key = keys[i];
    const uint64_t h = cid_hash64(key);
    const unsigned long long mine = ((unsigned long long)uint32_t(h) << 32) | i;
    uint32_t s = uint32_t(h >> 32) & mask;
    for (;;) {
        const unsigned long long cur = atomicCAS(&slots[s], kEmptySlot64, mine);
        if (cur == kEmptySlot64) {
            atomicAdd(&first[i], 1u);
            return;
        }
        if (uint32_t(cur >> 32) == uint32_t(h) && cid_equal(keys[uint32_t(cur)], key)) {
            const unsigned long long old = atomicMin(&slots[s], mine);  // (only positions of THIS CID ever lower this slot)
            if (old > mine) {
                atomicAdd(&first[i], 1u);
                atomicAdd(&first[uint32_t(old)], 0xffffffffu);
            }
            return;
        }
        s = (s + 1) & mask;
    }
}

// stage 4: first[i] = 1 iff position i is the first occurrence of its CID (`if seen.insert(*c) { out.push(*c) }`)
__global__ __launch_bounds__(256) void k_exec_first(const CidKey* __restrict__ keys, uint32_t n,
                                                    const unsigned long long* __restrict__ slots, uint32_t mask,
                                                    uint32_t* __restrict__ first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const CidKey key = keys[i];
    const uint64_t h = cid_hash64(key);
    uint32_t s = uint32_t(h >> 32) & mask;
    uint32_t f = 0;
    for (;;) {
        const unsigned long long cur = slots[s];
        if (cur == kEmptySlot64) break;  // cannot happen after stage 3; kept as a stop
        if (uint32_t(cur >> 32) == uint32_t(h)) {
            if (uint32_t(cur) == i) {  // the slot is this position's own: no key to read
                f = 1;
                break;
            }
            if (cid_equal(keys[uint32_t(cur)], key)) break;  // an earlier position holds the same CID
        }
        s = (s + 1) & mask;
    }
    first[i] = f;
}

// The tail of a tipset context ON THE DEVICE (host/verify_fast.cpp; k_exec_scan_finish below): what
// host/verify_events.cpp::verify_packed does between its second synchronisation and the verify kernel — decide whether the
// execution order is reachable, point the context at the tables, copy exec_len — without the host having seen the header
// facts.  Same rules, same order.
__device__ __forceinline__ void ctx_finish_fields(TipsetCtxDev* __restrict__ c, const CtxFinish& a, uint64_t total) {
    c->exec_status = IPCFP_ST_ERR_BAD_CLAIM;
    c->exec_slots = nullptr;
    c->exec_inv = nullptr;
    c->receipt_leaves = nullptr;
    c->n_receipt_leaves = 0;
    c->receipt_first = 0;
    c->receipt_recs = nullptr;
    c->event_recs = nullptr;
    // the execution order is only reached when steps 1-2 can pass for some proof of this context
    const bool reachable = (c->flags & TC_PARENTS_PARSED) && (c->flags & TC_CHILD_PARSED) && c->child_status == IPCFP_ST_TRUE &&
                           c->parents_match && c->n_parents > 0 && c->parent0_status == IPCFP_ST_TRUE;
    if (!reachable) return;
    const unsigned long long e = *a.err;
    const uint32_t status = e == kNoEnumError ? uint32_t(IPCFP_ST_TRUE) : enum_error_code(e);
    c->exec_status = status;
    c->exec_mask = a.mask;
    c->exec_slots = a.slots;
    c->exec_keys = a.keys;
    c->exec_pos = a.pos;
    c->exec_inv = status == IPCFP_ST_TRUE ? a.inv : nullptr;
    c->exec_len = status == IPCFP_ST_TRUE ? total : 0;
    // the receipts AMT rode along with the message AMTs: a table lookup per claim
    c->receipt_leaves = a.receipt_leaves;
    c->n_receipt_leaves = a.n_receipt_leaves;
    c->receipt_first = a.n_receipt_leaves ? a.receipt_first : 0;
    c->receipt_recs = a.receipt_recs;
    c->event_recs = a.event_recs;
}

// Stages 5-6 in ONE launch (host/verify_fast.cpp): the exclusive prefix sum of the first-occurrence flags as a single pass
// with DECOUPLED LOOK-BACK (the pattern of k_scan_tail_fused: a ticket per workgroup, relaxed agent-scope atomics on state
// words that carry the values themselves, no fence), positions and the inverse permutation, and — from the last tile in
// ticket order, which holds the total — the context's tail.  (Was: the flags' tile sums, a one-workgroup scan of them and
// an apply pass — three launches in a row on the way to the verify kernel.)
//   ctl[0]: the ticket (low word); ctl[1 + tile] = flag << 32 | value, flag 1: the tile's aggregate, 2: the inclusive prefix
//   up to it.  ALL ZERO on entry: the words ride behind the flags and are cleared with them (k_dense_link_leaves).
constexpr uint32_t kExecTile = 1024;

__global__ __launch_bounds__(256) void k_exec_scan_finish(const uint32_t* __restrict__ first, uint32_t n, uint32_t* __restrict__ pos,
                                                          uint64_t* __restrict__ total_out, unsigned long long* __restrict__ ctl,
                                                          TipsetCtxDev* __restrict__ c, CtxFinish a) {
    __shared__ uint64_t smem[17];
    __shared__ uint32_t s_tile;
    __shared__ uint64_t s_prefix;
    const uint32_t n_tiles = (n + kExecTile - 1) / kExecTile;
    unsigned long long* const state = ctl + 1;
    if (threadIdx.x == 0) s_tile = atomicAdd(reinterpret_cast<unsigned int*>(ctl), 1u);
    __syncthreads();
    const uint32_t tile = s_tile;
    const uint32_t base = tile * kExecTile + threadIdx.x * 4u;
    uint32_t f[4];
    uint64_t sum = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        f[k] = base + k < n ? first[base + k] : 0u;
        sum += f[k];
    }
    uint64_t tile_total;
    const uint64_t ex = block_exclusive_scan(sum, smem, &tile_total);
    if (threadIdx.x < 64) {  // publish, look back (wave 0)
        const uint32_t lane = threadIdx.x;
        if (lane == 0)
            __hip_atomic_store(state + tile, ((tile == 0 ? 2ull : 1ull) << 32) | (tile_total & 0xffffffffull), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        uint64_t prefix = 0;
        int32_t hi = int32_t(tile) - 1;  // the nearest predecessor not yet accounted for
        while (hi >= 0) {
            const int32_t j = hi - int32_t(lane);
            unsigned long long v = 0;
            bool ready = true;
            if (j >= 0) {
                v = __hip_atomic_load(state + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ready = ((v >> 32) & 3ull) != 0ull;
            }
            const uint64_t not_ready = __ballot(!ready);
            const uint32_t usable = not_ready ? uint32_t(__builtin_ctzll(not_ready)) : 64u;  // lanes 0 .. usable-1
            const uint64_t is_prefix = __ballot(ready && j >= 0 && ((v >> 32) & 3ull) == 2ull);
            const uint64_t in_use = usable >= 64u ? ~0ull : ((1ull << usable) - 1ull);
            const uint64_t pfx_in = is_prefix & in_use;
            const uint32_t stop = pfx_in ? uint32_t(__builtin_ctzll(pfx_in)) : 64u;  // first inclusive prefix met
            const uint32_t take = stop < 64u ? stop + 1u : usable;                   // lanes 0 .. take-1 contribute
            uint64_t mine = (lane < take && j >= 0) ? (v & 0xffffffffull) : 0ull;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
            prefix += mine;
            if (stop < 64u) break;
            hi -= int32_t(take);
            if (take == 0) __builtin_amdgcn_s_sleep(1);
        }
        if (lane == 0) {
            if (tile != 0)
                __hip_atomic_store(state + tile, (2ull << 32) | ((prefix + tile_total) & 0xffffffffull), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
            s_prefix = prefix;
        }
    }
    __syncthreads();
    uint64_t o = s_prefix + ex;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t i = base + k;
        if (i >= n) break;
        pos[i] = uint32_t(o);
        if (f[k]) a.inv[uint32_t(o)] = i;
        o += f[k];
    }
    if (tile == n_tiles - 1 && threadIdx.x == 0) {  // (what later launches read of these is ordered by the end of this one)
        const uint64_t total = s_prefix + tile_total;
        *total_out = total;
        ctx_finish_fields(c, a, total);
    }
}

// the distinct CIDs in execution order (ipcfp_exec_order)
__global__ __launch_bounds__(256) void k_exec_compact(const CidKey* __restrict__ keys, uint32_t n,
                                                      const uint32_t* __restrict__ first,
                                                      const uint32_t* __restrict__ pos, CidKey* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (first[i]) out[pos[i]] = keys[i];
}

// ---------------------------------------------------------------------------
// one proof per lane (the checks every route shares live in verify_dev.h)
// ---------------------------------------------------------------------------
// `where` (nullable) receives the location of the StampedEvent the claim names once the proof has reached it
// (block = 0xffffffff otherwise): a host `check_event` closure runs over those bytes (events/verifier.rs:247-251).
__device__ __forceinline__ uint32_t verify_event_one(const WitnessView& w, const EventClaimPacked& c,
                                                     const TipsetCtxDev& tc, const uint8_t* __restrict__ blob,
                                                     const ipcfp_trust_policy_t& trust, const ipcfp_event_filter_t& filter,
                                                     bool has_filter, ValueLoc* where) {
    // Steps 1-3: trust anchors, header consistency, execution order (verify_dev.h)
    const uint32_t pre = verify_event_prefix(c, tc, trust);
    if (pre != IPCFP_ST_TRUE) return pre;
    // Step 4: verify_receipt_and_event (:207-254)
    uint32_t st;
    ValueLoc rloc;
    if (tc.receipt_leaves && c.exec_index >= tc.receipt_first && c.exec_index - tc.receipt_first < tc.n_receipt_leaves) {
        // the receipts AMT was enumerated (and thereby fully validated) for this context: load + get
        // of a present index cannot fail and yields exactly this leaf                                        // :220-224
        const uint64_t slot = c.exec_index - tc.receipt_first;
        if (tc.receipt_recs) {
            // ... and its events were tabulated (event_table.h): normally k_verify_events_table has settled the claim
            bool settled;
            const uint32_t ts = verify_event_from_table(w, c, tc, blob, filter, has_filter, where, settled);
            if (settled) return ts;
        }
        const LeafRef l = tc.receipt_leaves[slot];
        if (l.block == kNoBlock) return IPCFP_ST_ERR;  // (a leaf the enumeration could not produce: the host redoes the call)
        rloc = ValueLoc{l.block, l.off, l.len};
    } else {
        AmtRootInfo receipts;
        st = amt_load(w, tc.receipts_root, 0, VK_RECEIPT, receipts);                                          // :220
        if (st != IPCFP_ST_TRUE) return st;
        st = amt_get(w, receipts, VK_RECEIPT, c.exec_index, rloc);                                            // :224
        if (st == IPCFP_ST_NOT_FOUND) return IPCFP_ST_FALSE_NO_RECEIPT;
        if (st != IPCFP_ST_TRUE) return st;
    }
    Rd rr;
    rr.init(w.arena + w.off[rloc.block] + rloc.off, rloc.len);
    uint32_t o, l;
    rr.expect_array(4);
    (void)rr.read_uint();
    rr.read_bytes(o, l);
    (void)rr.read_uint();
    if (rr.at_null()) return IPCFP_ST_FALSE_NO_EVENTS_ROOT;                                                   // :229
    CidKey events_root;
    rr.read_link_key(events_root);
    ValueLoc eloc;
    st = amt_load_get(w, events_root, 3, VK_STAMPED_EVENT, c.event_index, eloc);                              // :234-237
    if (st == IPCFP_ST_NOT_FOUND) return IPCFP_ST_FALSE_NO_EVENT;
    if (st != IPCFP_ST_TRUE) return st;
    if (where) *where = eloc;
    // verify_event_data_matches (:257-290)
    Rd er;
    er.init(w.arena + w.off[eloc.block] + eloc.off, eloc.len);
    uint64_t emitter;
    EvmLogLoc log;
    decode_event_log(er, emitter, log);
    if (emitter != c.emitter) return IPCFP_ST_FALSE_EMITTER;                                                  // :262
    if (!log.is_log) return IPCFP_ST_FALSE_NOT_EVM_LOG;                                                       // :267
    if (log.n_topics != c.n_topics) return IPCFP_ST_FALSE_TOPIC_COUNT;                                        // :272
    for (uint32_t i = 0; i < log.n_topics; ++i) {                                                             // :276-281
        const uint8_t* claimed = blob + c.topics_off + 33u * i;
        if (!claimed[0]) return IPCFP_ST_FALSE_TOPIC;  // the claimed string is not "0x" + 64 hex digits
        if (!er.equal32(log.topic_at(i), claimed + 1)) return IPCFP_ST_FALSE_TOPIC;
    }
    if (!(c.flags & EC_DATA_MATCHABLE) || c.data_len != log.data.len) return IPCFP_ST_FALSE_DATA;             // :284-287
    if (!er.equal_bytes(log.data.off, blob + c.data_off, c.data_len)) return IPCFP_ST_FALSE_DATA;
    if (has_filter && !log_matches(er, log, filter)) return IPCFP_ST_FALSE_FILTER;                             // :247-251
    return IPCFP_ST_TRUE;
}

__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_verify_events(WitnessView w, const EventClaimPacked* __restrict__ claims,
                                                       uint32_t n, const TipsetCtxDev* __restrict__ ctxs, uint32_t n_ctxs,
                                                       const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                       ipcfp_trust_policy_t trust,
                                                       ipcfp_event_filter_t filter, int has_filter,
                                                       uint8_t* __restrict__ status, ValueLoc* __restrict__ where,
                                                       int pending_only) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    if (pending_only && status[t] != kStPending) return;  // settled from the event table (verify_table.hip)
    const EventClaimPacked& c = claims[t];
    ValueLoc loc{kNoBlock, 0, 0};
    uint32_t st = IPCFP_ST_ERR_BAD_CLAIM;
    if (claim_in_bounds(c, n_ctxs, blob_len))
        st = verify_event_one(w, c, ctxs[c.context], blob, trust, filter, has_filter != 0, where ? &loc : nullptr);
    status[t] = uint8_t(st);
    if (where) where[t] = loc;
}

// exec_len of a context = the total of the first-occurrence scan, copied on the device so the host
// never waits for it
// ... and the inverse of exec_pos: inv[execution index] = raw position of the message's first occurrence.  A claim
// names (exec_index, message): `exec_keys[inv[exec_index]] == message` settles `position(message) == exec_index`
// with two reads that run along with the claims instead of a hash probe (three reads somewhere in 60 MB).
__global__ __launch_bounds__(256) void k_exec_finish(TipsetCtxDev* __restrict__ c, const uint64_t* __restrict__ total,
                                                     const uint32_t* __restrict__ first, const uint32_t* __restrict__ pos,
                                                     uint32_t n, uint32_t* __restrict__ inv) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) c->exec_len = *total;
    if (i < n && first[i]) inv[pos[i]] = i;
}

// ctl_d: exec_scan_ctl_words(a.raw_len) words, zero when this is queued
int launch_exec_scan_finish(ipcfp_ctx* ctx, TipsetCtxDev* ctx_d, const CtxFinish& a, uint32_t* pos_d, uint64_t* total_d,
                            unsigned long long* ctl_d) {
    const uint32_t n = a.raw_len;
    if (n == 0) return set_error(ctx, IPCFP_E_INVALID, "exec scan: no messages");
    hipLaunchKernelGGL(k_exec_scan_finish, dim3(div_up(n, kExecTile)), dim3(256), 0, ctx->stream, a.first, n, pos_d, total_d, ctl_d,
                       ctx_d, a);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}
size_t exec_scan_ctl_words(uint32_t n) { return 1u + size_t(div_up(n, kExecTile)); }

// ------------------------------ launchers -----------------------------------
int launch_exec_finish(ipcfp_ctx* ctx, TipsetCtxDev* ctx_d, const uint64_t* total_d, const uint32_t* first_d,
                       const uint32_t* pos_d, uint32_t n, uint32_t* inv_d) {
    hipLaunchKernelGGL(k_exec_finish, dim3(n ? div_up(n, 256) : 1), dim3(256), 0, ctx->stream, ctx_d, total_d, first_d, pos_d,
                       n, inv_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_exec_dedup(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* leaves_d, uint32_t n, CidKey* keys_d,
                      unsigned long long* slots_d, uint32_t mask, uint32_t* first_d) {
    if (n == 0) return IPCFP_OK;
    const dim3 g(div_up(n, 256)), b(256);
    if (leaves_d) hipLaunchKernelGGL(k_exec_keys, g, b, 0, ctx->stream, w, leaves_d, n, keys_d);  // else: keys came with the enumeration
    hipLaunchKernelGGL(k_exec_insert, g, b, 0, ctx->stream, keys_d, n, slots_d, mask);
    hipLaunchKernelGGL(k_exec_first, g, b, 0, ctx->stream, keys_d, n, slots_d, mask, first_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

// first_d must be zero (hipMemsetAsync on the same stream) when this is queued
int launch_exec_insert_flags(ipcfp_ctx* ctx, const CidKey* keys_d, uint32_t n, unsigned long long* slots_d, uint32_t mask,
                             uint32_t* first_d) {
    if (n == 0) return IPCFP_OK;
    hipLaunchKernelGGL(k_exec_insert_flags, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, keys_d, n, slots_d, mask, first_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_exec_compact(ipcfp_ctx* ctx, const CidKey* keys_d, uint32_t n, const uint32_t* first_d,
                        const uint32_t* pos_d, CidKey* out_d) {
    if (n == 0) return IPCFP_OK;
    hipLaunchKernelGGL(k_exec_compact, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, keys_d, n, first_d, pos_d,
                       out_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_verify_events(ipcfp_ctx* ctx, const WitnessView& w, const EventClaimPacked* claims_d, uint32_t n,
                         const TipsetCtxDev* ctxs_d, uint32_t n_ctxs, const uint8_t* blob_d, uint64_t blob_len,
                         const ipcfp_trust_policy_t& trust, const ipcfp_event_filter_t* filter, uint8_t* status_d,
                         void* where_d, bool tabulated) {
    if (n == 0) return IPCFP_OK;
    ipcfp_event_filter_t f{};
    if (filter) f = *filter;
    {
        ProfileScope prof(ctx, IPCFP_K_EVENT_VERIFY);
        // claims whose receipt's events are tabulated are settled by a kernel that parses nothing; the general
        // walker then only serves what that one left pending
        if (tabulated) {
            int rc = launch_verify_events_table(ctx, w, claims_d, n, ctxs_d, n_ctxs, blob_d, blob_len, trust, f, filter ? 1 : 0,
                                                status_d, where_d);
            if (rc) return rc;
        }
        hipLaunchKernelGGL(k_verify_events, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w, claims_d, n, ctxs_d,
                           n_ctxs, blob_d, blob_len, trust, f, filter ? 1 : 0, status_d, static_cast<ValueLoc*>(where_d),
                           tabulated ? 1 : 0);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
