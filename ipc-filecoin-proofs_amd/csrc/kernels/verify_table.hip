// csrc/kernels/verify_table.hip — `verify_single_proof` (src/proofs/events/verifier.rs:92-290) for the claims whose
// receipt was enumerated and whose events are tabulated (event_table.h): steps 1-3 are table lookups (execution-order
// hash table), step 4 compares the claim with bytes at addresses the records name.  No block is parsed here, so the
// kernel needs no CBOR reader; a claim the table does not cover is marked kStPending and taken by the general walker
// (k_verify_events) right behind.
//
// The usual claim (verify_table_hot) is four batches of loads, each issued whole before any of it is waited for, and
// then a ladder of selects over registers.  Every other claim keeps the ladder of early returns (verify_table_one) —
// DESIGN.md §31.  What a wavefront reads of contiguous memory — its claims, and the window of the blob its usual claims
// name — it reads coalesced through an LDS region of its own.
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../common.h"
#include "launch.h"
#include "verify_dev.h"
#include "verify_window.h"

namespace ipcfp {

typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ u64x2_t ld16(const uint8_t* __restrict__ p) {
    u64x2_t v;
    __builtin_memcpy(&v, p, 16);  // (any alignment: gfx950 runs in unaligned-access mode)
    return v;
}
__device__ __forceinline__ bool differ32(const u64x2_t a[2], const u64x2_t b[2]) {
    return (((a[0].x ^ b[0].x) | (a[0].y ^ b[0].y)) | ((a[1].x ^ b[1].x) | (a[1].y ^ b[1].y))) != 0;
}

// The claimed bytes of the usual shape — at most two topics, 32 bytes of data — are fetched from the blob right after the
// claim itself, beside the record loads, instead of piece by piece between the (random, slow) reads of the event: a line
// of the blob fetched once per wavefront instead of once per piece (every access costs a whole 128-byte line:
// profiles/r03_fetch_calib.txt), and the chain of dependent loads of a claim is four long instead of eight.
struct ClaimedBytes {
    u64x2_t topic[2][2];
    uint32_t flag[2];  // the matchable byte in front of each topic
    u64x2_t data[2];
};

__device__ __forceinline__ void load_claimed(const EventClaimPacked& c, const uint8_t* __restrict__ blob, ClaimedBytes& p) {
    p = ClaimedBytes{};
    if (c.n_topics >= 1 && c.n_topics <= 2) {
        const uint8_t* q = blob + c.topics_off;
        p.flag[0] = q[0];
        p.topic[0][0] = ld16(q + 1);
        p.topic[0][1] = ld16(q + 17);
        if (c.n_topics == 2) {
            p.flag[1] = q[33];
            p.topic[1][0] = ld16(q + 34);
            p.topic[1][1] = ld16(q + 50);
        }
    }
    if ((c.flags & EC_DATA_MATCHABLE) && c.data_len == 32) {
        p.data[0] = ld16(blob + c.data_off);
        p.data[1] = ld16(blob + c.data_off + 16);
    }
}

// verify_event_record (verify_dev.h) with the claimed bytes in registers and the event's bytes fetched in one batch; the
// verdicts are taken in the reference's order (events/verifier.rs:257-290, then :247-251).  Other shapes: the general form.
__device__ __forceinline__ uint32_t verify_event_record_batched(const WitnessView& w, const EventClaimPacked& c, const EventRec& e,
                                                                const ClaimedBytes& p, const uint8_t* __restrict__ blob,
                                                                const ipcfp_event_filter_t& filter, bool has_filter) {
    if (e.emitter != c.emitter) return IPCFP_ST_FALSE_EMITTER;                                                // :262
    if (!(e.base_flags & kEvIsLog)) return IPCFP_ST_FALSE_NOT_EVM_LOG;                                        // :267
    const uint32_t nt = uint32_t(e.base_flags >> kEvTopicShift) & 0xffu;
    if (nt != c.n_topics) return IPCFP_ST_FALSE_TOPIC_COUNT;                                                  // :272
    if (nt > 2) return verify_event_record(w, c, e, blob, filter, has_filter);
    const uint8_t* item = w.arena + (e.base_flags & kEvBaseMask);
    const bool case_a = (e.base_flags & kEvCaseA) != 0;
    const uint32_t rel0 = e.topic_rel[0], rel1 = case_a ? uint32_t(e.topic_rel[0]) + 32u : uint32_t(e.topic_rel[1]);
    const bool data_shape = (c.flags & EC_DATA_MATCHABLE) && c.data_len == e.data_len;
    const bool data_batched = data_shape && c.data_len == 32;
    u64x2_t t0[2] = {}, t1[2] = {}, d[2] = {};
    if (nt >= 1) {
        t0[0] = ld16(item + rel0);
        t0[1] = ld16(item + rel0 + 16);
    }
    if (nt == 2) {
        t1[0] = ld16(item + rel1);
        t1[1] = ld16(item + rel1 + 16);
    }
    if (data_batched) {
        d[0] = ld16(item + e.data_rel);
        d[1] = ld16(item + e.data_rel + 16);
    }
    if (nt >= 1 && (!p.flag[0] || differ32(p.topic[0], t0))) return IPCFP_ST_FALSE_TOPIC;                     // :276-281
    if (nt == 2 && (!p.flag[1] || differ32(p.topic[1], t1))) return IPCFP_ST_FALSE_TOPIC;
    if (!data_shape) return IPCFP_ST_FALSE_DATA;                                                              // :284-287
    if (data_batched ? differ32(p.data, d) : !bytes_equal_global(item + e.data_rel, blob + c.data_off, c.data_len))
        return IPCFP_ST_FALSE_DATA;
    if (has_filter) {                                                                                         // :247-251
        if (nt < 2) return IPCFP_ST_FALSE_FILTER;
        u64x2_t f0[2], f1[2];
        __builtin_memcpy(f0, filter.topic0, 32);
        __builtin_memcpy(f1, filter.topic1, 32);
        if (differ32(t0, f0) || differ32(t1, f1)) return IPCFP_ST_FALSE_FILTER;
    }
    return IPCFP_ST_TRUE;
}

__device__ __forceinline__ uint32_t verify_table_one(const WitnessView& w, const EventClaimPacked& c, const TipsetCtxDev& tc,
                                                     const uint8_t* __restrict__ blob, const ipcfp_trust_policy_t& trust,
                                                     const ipcfp_event_filter_t& filter, bool has_filter, ValueLoc* where) {
    // everything that depends on the claim alone is in flight before the first verdict is taken
    ClaimedBytes p;
    load_claimed(c, blob, p);
    const bool tabulated = tc.receipt_leaves && tc.receipt_recs && c.exec_index >= tc.receipt_first &&
                           c.exec_index - tc.receipt_first < tc.n_receipt_leaves;
    ReceiptRec rr{RK_WALK, 0, 0, kNoBlock, 0};
    if (tabulated) rr = tc.receipt_recs[c.exec_index - tc.receipt_first];
    const uint32_t st = verify_event_prefix(c, tc, trust);
    if (st != IPCFP_ST_TRUE) return st;
    // verify_event_from_table (verify_dev.h), same rules in the same order
    if (!tabulated || rr.kind == RK_WALK) return kStPending;
    if (rr.kind == RK_NO_EVENTS) return IPCFP_ST_FALSE_NO_EVENTS_ROOT;                                        // :229
    if (rr.kind >= 64) return rr.kind;                                                                        // :234 Err
    if (c.event_index == ~0ULL) return IPCFP_ST_ERR;                                                          // > MAX_INDEX
    if (c.event_index >= 64 || !((rr.bitmap >> c.event_index) & 1ull)) return IPCFP_ST_FALSE_NO_EVENT;        // :237
    const EventRec e = tc.event_recs[rr.first + __popcll(rr.bitmap & ((1ull << c.event_index) - 1ull))];
    if (where) *where = ValueLoc{rr.block, uint32_t((e.base_flags & kEvBaseMask) - w.off[rr.block]), e.ev_len};
    return verify_event_record_batched(w, c, e, p, blob, filter, has_filter);
}

// ---- the usual claim: four load batches, then the verdicts -----------------------------------------------------------
// A claim is "usual" when its wavefront names one context, it claims at most two topics, and its data is 32 bytes or can
// never match: then everything the reference's ladder looks at sits behind a chain of loads FOUR deep,
//   A  the claim
//   B  the claimed bytes in the blob, receipt_recs[exec_index - receipt_first], exec_inv[exec_index], the context's facts
//   C  event_recs[first + popcount], exec_keys[inv], (w.off[block] when locations are wanted)
//   D  the event's topics and data
// and the ladder itself needs no load at all.  Written rung by rung with early returns (verify_table_one) hipcc puts a
// branch and a full wait around nearly every load — seven vector-memory waits and some twenty scalar ones on an honest
// claim.  Here every batch is issued whole, the rungs are selects, and the first failing rung's status stands.
//
// A load whose guard is false reads `safe` (the wavefront's first claim: 104 readable bytes, one line for all 64 lanes)
// instead of branching: never an out-of-bounds index, never a null table.  Every address the ladder of early returns would not
// have formed is guarded off, so this path dereferences a subset of what verify_table_one does.
// (Global address space by name: a table pointer read out of a context is generic to the compiler, and a select between
// it and `safe` would make every one of these a flat load.)
typedef const __attribute__((address_space(1))) uint8_t* gbytes_t;
__device__ __forceinline__ gbytes_t guarded(bool ok, const void* p, const void* safe) {
    return ok ? (gbytes_t)p : (gbytes_t)safe;
}
__device__ __forceinline__ u64x2_t ld16(gbytes_t p) {
    u64x2_t v;
    __builtin_memcpy(&v, p, 16);
    return v;
}
// The end of a batch: the values are waited for HERE, by every lane.  Without it hipcc sinks a load whose result only
// some lanes use into a branch of those lanes and waits for it there, alone — one more link in the chain.
__device__ __forceinline__ void batch_end(uint64_t a, uint64_t b = 0, uint64_t c = 0, uint64_t d = 0, uint64_t e = 0) {
    asm volatile("" ::"v"(a), "v"(b), "v"(c), "v"(d), "v"(e));
}

static_assert(offsetof(ReceiptRec, first) == 4 && offsetof(ReceiptRec, bitmap) == 8 && offsetof(ReceiptRec, block) == 16,
              "verify_table_hot reads a ReceiptRec as three words");
static_assert(offsetof(EventRec, topic_rel) == 16 && offsetof(EventRec, data_rel) == 24 && offsetof(EventRec, ev_len) == 26 &&
                  offsetof(EventRec, data_len) == 28,
              "verify_table_hot reads an EventRec as four words");

__device__ __forceinline__ bool hot_shape(const EventClaimPacked& c) {
    return c.n_topics <= 2 && (!(c.flags & EC_DATA_MATCHABLE) || c.data_len == 32);
}

// ---- a wavefront's LDS region ------------------------------------------------------------------------------------------
// The claims of a wavefront are contiguous (64 × 104 bytes), and so, nearly always, are the blob entries they name.  Read
// lane by lane, one load instruction touches some fifty 128-byte lines; read as ONE byte range, 16 bytes a lane, it touches
// eight, each once.  So every wavefront copies its claims into an LDS region of its own and every lane takes its claim
// from there; the region then takes the WINDOW of the blob (verify_window.h) and the usual claims take their claimed
// bytes from it.  A region belongs to one wavefront: a wavefront's LDS instructions execute in order, so a fence and the
// wavefront barrier between the writes and the reads are all the ordering there is — nothing waits for another wavefront.
constexpr uint32_t kStageStride = kVerifyWindowBytes + 16u;  // (+16: the ninth word of a 32-byte piece that ends the window)
constexpr uint32_t kStageLoads = (kVerifyWindowBytes + 1023u) / 1024u;

// `bytes` <= kVerifyWindowBytes from src (any alignment) to the region: whole 16-byte pieces, all loads in flight before
// the first write, then the odd bytes one lane apiece.  Reads [src, src + bytes) and nothing else.
__device__ __forceinline__ void stage_copy(uint8_t* __restrict__ region, const uint8_t* __restrict__ src, uint32_t bytes, uint32_t lane) {
    const uint32_t whole = bytes & ~15u;
    u64x2_t v[kStageLoads];
#pragma unroll
    for (uint32_t k = 0; k < kStageLoads; ++k) {
        const uint32_t o = (k * 64u + lane) * 16u;
        v[k] = u64x2_t{0, 0};
        if (o < whole) v[k] = ld16(src + o);
    }
    // (every access to a region is a memcpy: bytes to the compiler, which then keeps reads and writes of it in order)
#pragma unroll
    for (uint32_t k = 0; k < kStageLoads; ++k) {
        const uint32_t o = (k * 64u + lane) * 16u;
        if (o < whole) __builtin_memcpy(__builtin_assume_aligned(region + o, 16), &v[k], 16);  // ds_write_b128
    }
    if (whole + lane < bytes) region[whole + lane] = src[whole + lane];
}
__device__ __forceinline__ void stage_publish() {  // the region's writes before its reads, within the wavefront
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// 32 bytes at byte j of the region: nine aligned words and a byte shift (a 64- or 128-bit LDS read off its natural
// alignment is replayed, some 64 cycles each; a 32-bit one is not)
__device__ __forceinline__ void region_ld32(const uint8_t* region, uint32_t j, u64x2_t out[2]) {
    const uint8_t* p = static_cast<const uint8_t*>(__builtin_assume_aligned(region + (j & ~3u), 4));
    const uint32_t s = j & 3u;
    uint32_t x[9], a[8];
#pragma unroll
    for (int i = 0; i < 9; ++i) __builtin_memcpy(&x[i], p + 4 * i, 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = __builtin_amdgcn_alignbyte(x[i + 1], x[i], s);
    out[0] = u64x2_t{a[0] | uint64_t(a[1]) << 32, a[2] | uint64_t(a[3]) << 32};
    out[1] = u64x2_t{a[4] | uint64_t(a[5]) << 32, a[6] | uint64_t(a[7]) << 32};
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, uint32_t(__shfl_xor(v, m, 64)));
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, uint32_t(__shfl_xor(v, m, 64)));
    return v;
}

// Called by EVERY lane of a wavefront whose in-bounds claims name one context; `hot`: this lane holds a usual claim (in
// bounds, hot_shape).  The other lanes only help to carry the window: each of their loads is guarded off, their result
// is to be ignored.  `region`: the wavefront's LDS region, free (the claims are in registers).
// `cold` = true: not decided here (the execution-order compare failed, so the hash table has to be asked; or a record
// kind the table does not define) — the caller runs verify_table_one, and `loc` is to be ignored.
__device__ __forceinline__ uint32_t verify_table_hot(const WitnessView& w, const EventClaimPacked& c, bool hot, const TipsetCtxDev& tc,
                                                     const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                     const ipcfp_trust_policy_t& trust, const ipcfp_event_filter_t& filter,
                                                     bool has_filter, bool want_where, const void* safe, uint8_t* region,
                                                     uint32_t lane, ValueLoc& loc, bool& cold) {
    // ---- batch B: what the claim and the context's pointers address
    const EventCtxFacts f = event_ctx_facts(tc);
    Verdict v;
    event_prefix_rungs(v, c, f, trust);  // (registers only: the claim and the facts)
    const bool pre_ok = hot && !v.settled;
    // (the two records that batch C hangs on go first: vmcnt counts in order, so they are waited for without the blob)
    const bool tabulated = hot && f.has_receipt_table && c.exec_index >= f.receipt_first && c.exec_index - f.receipt_first < f.n_receipt_leaves;
    uint64_t rw[3];  // the ReceiptRec as words
    __builtin_memcpy(rw, guarded(tabulated, f.receipt_recs + (c.exec_index - f.receipt_first), safe), 24);
    const bool inv_ok = pre_ok && f.exec_inv && f.exec_keys && c.exec_index < f.exec_len;
    uint32_t inv;
    __builtin_memcpy(&inv, guarded(inv_ok, f.exec_inv + c.exec_index, safe), 4);
    const bool matchable = (c.flags & EC_DATA_MATCHABLE) != 0;  // hot_shape: then data_len == 32
    const bool rd0 = hot && c.n_topics >= 1, rd1 = hot && c.n_topics == 2, rdd = hot && matchable;
    // the window: the extent of what the wavefront's usual claims read of the blob (claim_in_bounds has passed for each)
    uint64_t lo, hi;
    const bool reads = verify_window_lane(hot ? c.n_topics : 0u, c.topics_off, rdd, c.data_off, lo, hi);
    const uint64_t start = verify_window_start(wave_min(reads ? uint32_t(lo) : 0xffffffffu));  // (lo is an offset: 32 bits)
    const uint32_t win_len = __builtin_amdgcn_readfirstlane(
        __any(reads) ? verify_window_len(start, wave_max(reads ? verify_window_rel_end(hi, start) : 0u), blob_len) : 0u);
    ClaimedBytes p;
    if (win_len) {  // (uniform) coalesced into the region, each lane's pieces out of it
        stage_copy(region, blob + start, win_len, lane);
        stage_publish();
        const uint32_t j0 = rd0 ? uint32_t(c.topics_off - start) : 0u, j1 = rd1 ? j0 + 33u : 0u;
        const uint32_t jd = rdd ? uint32_t(c.data_off - start) : 0u;
        p.flag[0] = region[j0];
        region_ld32(region, j0 + (rd0 ? 1u : 0u), p.topic[0]);
        p.flag[1] = region[j1];
        region_ld32(region, j1 + (rd1 ? 1u : 0u), p.topic[1]);
        region_ld32(region, jd, p.data);
    } else {  // entries too far apart for the window (or nothing to read): lane by lane from the blob
        const gbytes_t q0 = guarded(rd0, blob + c.topics_off, safe);
        const gbytes_t q1 = guarded(rd1, blob + c.topics_off + 33, safe);
        const gbytes_t qd = guarded(rdd, blob + c.data_off, safe);
        p.flag[0] = q0[0];
        p.topic[0][0] = ld16(q0 + 1);
        p.topic[0][1] = ld16(q0 + 17);
        p.flag[1] = q1[0];
        p.topic[1][0] = ld16(q1 + 1);
        p.topic[1][1] = ld16(q1 + 17);
        p.data[0] = ld16(qd);
        p.data[1] = ld16(qd + 16);
    }
    batch_end(rw[0], rw[1], rw[2], inv);
    const uint32_t rr_kind = uint32_t(rw[0]), rr_first = uint32_t(rw[0] >> 32), rr_block = uint32_t(rw[2]);
    const uint64_t rr_bitmap = rw[1];

    // ---- batch C: what the receipt record and the inverse order address
    CidKey key;
    __builtin_memcpy(&key, guarded(inv_ok, f.exec_keys + inv, safe), 40);
    const uint32_t bit = uint32_t(c.event_index) & 63u;
    const bool present = c.event_index < 64 && ((rr_bitmap >> bit) & 1ull);
    const bool have_event = pre_ok && tabulated && rr_kind == RK_TABLE && f.event_recs && present;
    const uint32_t slot = rr_first + uint32_t(__popcll(rr_bitmap & ((1ull << bit) - 1ull)));
    uint64_t ew[4];  // the EventRec as words: no field is ever indexed dynamically
    __builtin_memcpy(ew, guarded(have_event, f.event_recs + slot, safe), 32);
    uint64_t block_off = 0;
    if (want_where) __builtin_memcpy(&block_off, guarded(have_event, w.off + rr_block, safe), 8);  // (uniform)
    batch_end(key.w[0], key.w[1], key.w[2], key.w[3], key.w[4]);
    batch_end(ew[0], ew[1], ew[2], ew[3], block_off);

    // steps 1-3 end: `exec_order.iter().position(|c| c == msg)` == exec_index (verify_event_prefix)
    const bool exec_ok = inv_ok && cid_equal(key, c.message);
    // verify_event_from_table (verify_dev.h), same rules in the same order
    v.rung(!tabulated || rr_kind == RK_WALK, kStPending);
    v.rung(rr_kind == RK_NO_EVENTS, IPCFP_ST_FALSE_NO_EVENTS_ROOT);                                           // :229
    v.rung(rr_kind >= 64, rr_kind);                                                                           // :234 Err
    v.rung(c.event_index == ~0ULL, IPCFP_ST_ERR);                                                             // > MAX_INDEX
    v.rung(!present, IPCFP_ST_FALSE_NO_EVENT);                                                                // :237
    const bool reached = !v.settled;  // the proof has reached its event
    cold = pre_ok && (!exec_ok || (reached && !have_event));

    // verify_event_record_batched, same rules in the same order
    const uint64_t base_flags = ew[0], e_emitter = ew[1];
    const uint32_t rel0 = uint32_t(ew[2]) & 0xffffu, rel1_b = uint32_t(ew[2] >> 16) & 0xffffu;
    const uint32_t data_rel = uint32_t(ew[3]) & 0xffffu, ev_len = uint32_t(ew[3] >> 16) & 0xffffu, e_data_len = uint32_t(ew[3] >> 32);
    v.rung(e_emitter != c.emitter, IPCFP_ST_FALSE_EMITTER);                                                   // :262
    v.rung(!(base_flags & kEvIsLog), IPCFP_ST_FALSE_NOT_EVM_LOG);                                             // :267
    const uint32_t nt = uint32_t(base_flags >> kEvTopicShift) & 0xffu;
    v.rung(nt != c.n_topics, IPCFP_ST_FALSE_TOPIC_COUNT);                                                     // :272

    // ---- batch D: the event's bytes (only where the ladder of early returns reads them too)
    const bool bytes_wanted = have_event && exec_ok && !v.settled;  // hence nt == c.n_topics <= 2
    const uint8_t* item = w.arena + (base_flags & kEvBaseMask);
    const uint32_t rel1 = (base_flags & kEvCaseA) ? rel0 + 32u : rel1_b;
    const bool data_shape = matchable && c.data_len == e_data_len;
    const gbytes_t a0 = guarded(bytes_wanted && nt >= 1, item + rel0, safe);
    const gbytes_t a1 = guarded(bytes_wanted && nt == 2, item + rel1, safe);
    const gbytes_t ad = guarded(bytes_wanted && data_shape, item + data_rel, safe);
    const u64x2_t t0[2] = {ld16(a0), ld16(a0 + 16)}, t1[2] = {ld16(a1), ld16(a1 + 16)}, d[2] = {ld16(ad), ld16(ad + 16)};

    v.rung(nt >= 1 && (!p.flag[0] || differ32(p.topic[0], t0)), IPCFP_ST_FALSE_TOPIC);                        // :276-281
    v.rung(nt == 2 && (!p.flag[1] || differ32(p.topic[1], t1)), IPCFP_ST_FALSE_TOPIC);
    v.rung(!data_shape, IPCFP_ST_FALSE_DATA);                                                                 // :284-287
    v.rung(differ32(p.data, d), IPCFP_ST_FALSE_DATA);
    u64x2_t f0[2], f1[2];
    __builtin_memcpy(f0, filter.topic0, 32);
    __builtin_memcpy(f1, filter.topic1, 32);
    v.rung(has_filter && nt < 2, IPCFP_ST_FALSE_FILTER);                                                      // :247-251
    v.rung(has_filter && (differ32(t0, f0) || differ32(t1, f1)), IPCFP_ST_FALSE_FILTER);

    const bool located = reached && have_event;
    loc.block = located ? rr_block : kNoBlock;
    loc.off = located ? uint32_t((base_flags & kEvBaseMask) - block_off) : 0u;
    loc.len = located ? ev_len : 0u;
    return v.st;
}

__global__ __launch_bounds__(256) void k_verify_events_table(WitnessView w, const EventClaimPacked* __restrict__ claims, uint32_t n,
                                                             const TipsetCtxDev* __restrict__ ctxs, uint32_t n_ctxs,
                                                             const uint8_t* __restrict__ blob, uint64_t blob_len,
                                                             ipcfp_trust_policy_t trust, ipcfp_event_filter_t filter,
                                                             int has_filter, uint8_t* __restrict__ status,
                                                             ValueLoc* __restrict__ where) {
    __shared__ __attribute__((aligned(16))) uint8_t regions[4][kStageStride];
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, first = t - lane;
    if (first >= n) return;  // (a whole wavefront past the batch: nothing below waits for another wavefront)
    const bool live = t < n;
    // the wavefront's claims, [claims + first, claims + first + min(64, n - first)), as one byte range through its region
    uint8_t* const region = regions[threadIdx.x >> 6];
    stage_copy(region, reinterpret_cast<const uint8_t*>(claims + first), min(64u, n - first) * uint32_t(sizeof(EventClaimPacked)), lane);
    stage_publish();
    EventClaimPacked c{};
    // (104·lane is 8-aligned: 64-bit reads, none off its natural alignment)
    if (live) __builtin_memcpy(&c, __builtin_assume_aligned(region + lane * sizeof(EventClaimPacked), 8), sizeof c);
    stage_publish();  // (the region is written again below: every lane's claim is out of it first)
    ValueLoc loc{kNoBlock, 0, 0};
    uint32_t st = IPCFP_ST_ERR_BAD_CLAIM;
    const bool inb = live && claim_in_bounds(c, n_ctxs, blob_len);
    // The proofs of a wavefront nearly always name ONE tipset pair: its context (≈700 bytes of header facts and
    // table pointers) is then read through the scalar unit once per wavefront instead of by 64 lanes apiece.
    const uint32_t ctx0 = __builtin_amdgcn_readfirstlane(inb ? c.context : 0xffffffffu);
    bool cold = inb;  // lanes that take the ladder of early returns
    if (ctx0 != 0xffffffffu && __all(!inb || c.context == ctx0)) {
        const bool hot = inb && hot_shape(c);
        if (__any(hot)) {  // every lane goes in (the window is carried by all 64); only the hot ones come out with a verdict
            ValueLoc hot_loc;
            bool again;
            // (`safe`: one address for the wavefront — its first claim — so that a guarded-off load touches one line)
            const uint32_t hot_st = verify_table_hot(w, c, hot, ctxs[ctx0], blob, blob_len, trust, filter, has_filter != 0,
                                                     where != nullptr, claims + first, region, lane, hot_loc, again);
            const bool keep = !hot || again;
            st = keep ? st : hot_st;
            loc.block = keep ? loc.block : hot_loc.block;
            loc.off = keep ? loc.off : hot_loc.off;
            loc.len = keep ? loc.len : hot_loc.len;
            cold = hot ? again : cold;
        }
    }
    // Everything else — a claim that needs the hash-table probe, more than two topics, data of another length, contexts
    // that differ within the wavefront — takes the ladder of early returns (verify_table_one), each lane with its own context.
    // (They read their claim AGAIN, through a pointer the compiler cannot tell from another: kept in registers for them,
    // the claim's 26 words would be live across the whole hot path and cost it a wavefront of occupancy.)
    if (__any(cold)) {
        if (cold) {
            const EventClaimPacked* mine = claims + t;
            asm volatile("" : "+v"(mine));
            const EventClaimPacked cc = *mine;
            ValueLoc cold_loc{kNoBlock, 0, 0};
            st = verify_table_one(w, cc, ctxs[cc.context], blob, trust, filter, has_filter != 0, &cold_loc);
            loc = cold_loc;
        }
    }
    if (!live) return;
    status[t] = uint8_t(st);
    if (where) where[t] = loc;
}

int launch_verify_events_table(ipcfp_ctx* ctx, const WitnessView& w, const EventClaimPacked* claims_d, uint32_t n,
                               const TipsetCtxDev* ctxs_d, uint32_t n_ctxs, const uint8_t* blob_d, uint64_t blob_len,
                               const ipcfp_trust_policy_t& trust, const ipcfp_event_filter_t& filter, int has_filter,
                               uint8_t* status_d, void* where_d) {
    if (n == 0) return IPCFP_OK;
    hipLaunchKernelGGL(k_verify_events_table, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w, claims_d, n, ctxs_d, n_ctxs,
                       blob_d, blob_len, trust, filter, has_filter, status_d, static_cast<ValueLoc*>(where_d));
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
