// csrc/kernels/storage_claims_gen_body.h — the ONE text of the storage generator's dependent chain, for a single child and
// for a chain of children (storage_claims_gen.hip, whose header comment has the steps and the recorder's rules).
//
// Each body is a kernel template over an INDEX POLICY and is instantiated twice; everything in which the two forms differ
// is a member of the policy, nothing else is:
//
//                      SgenOne — one child                          SgenChain — ONE spec list at each of T children
//   run_at / spec_at   lane i is run i / spec i of tipset 0         i = t·R0 + r / t·n_specs + s, split by a division
//   view               the kernel's recording view as passed —      a copy whose `touched` is row t of the recorder: a lane
//                      `touched` stays wave-uniform                 records for its own tipset only
//   kSlotColumn        false: the slot is read at i, none written   true: read at s, written (replicated) at i
//   run_actor          actor_id[runs[i].first_claim]                actor_id[runs0[r].first_claim], refused when the record
//                                                                   points outside the list
//   spec_run           run_of[i]                                    t·R0 + run_of0[s], refused when the list has no such run
//   run_stretch        [first_claim, the next run's or n)           the same of runs0, clipped to the list
//   child / epoch      the call's                                   children[t] / epochs[t]
//
// The one-child policy's refusals are constant `true`: its instantiations hold no guard the single call did not have.
//
// The templates are the kernels themselves, not device functions behind forwarding kernels, and the spec kernels load the slot
// with two raw_ld128 written in place: at (256, 7) the register allocation of k_sgen_specs_table<SgenChain> tips over on either
// — same VGPRs and occupancy, three times the scratch traffic.
#pragma once
#include "../common.h"
#include "claims_dev.h"
#include "hamt_table.h"
#include "storage_dev.h"
#include "storage_runs.h"
#include "storage_value_dev.h"

namespace ipcfp {

// StorageRun (storage_runs.h) holds the derived facts; its `chain_status` word carries the chain's verdict for the claim
// kernels: IPCFP_ST_TRUE when contract_state is known, else the ERR_* generate_storage_proof returns for every spec of the run.
__device__ __forceinline__ uint32_t chain_verdict(const StorageRun& r) {
    if (r.hdr_status != IPCFP_ST_TRUE) return r.hdr_status;
    if (r.sr_status != IPCFP_ST_TRUE) return r.sr_status;
    if (r.actor_status != IPCFP_ST_TRUE) return r.actor_status;
    return r.evm_status;
}

__device__ __forceinline__ void zero_key(CidKey& k) {
#pragma unroll
    for (int j = 0; j < 5; ++j) k.w[j] = 0;
}

struct alignas(16) Out16 {
    uint64_t lo, hi;
};
static_assert(alignof(Out16) == 16 && sizeof(Out16) == 16, "one 16-byte store");

// RecordingBlockStore::get of a block somebody else has already looked up.  A run's specs mark the same few words: the bit is
// tested with a plain load first (the words only grow, so a stale read costs one redundant atomic, never a lost mark).
__device__ __forceinline__ void mark_block(const WitnessView& w, uint32_t b) {
    uint32_t* word = w.touched + (b >> 5);
    const uint32_t bit = 1u << (b & 31u);
    if (!(__builtin_nontemporal_load(word) & bit)) atomicOr(word, bit);
}
// 32 bytes of column `col` at entry t as two 16-byte vector stores (the columns lie on a 16-byte boundary)
__device__ __forceinline__ void store_32(uint8_t* __restrict__ col, uint32_t t, const uint64_t v[4]) {
    Out16* o = reinterpret_cast<Out16*>(col + 32ull * t);
    o[0] = Out16{v[0], v[1]};
    o[1] = Out16{v[2], v[3]};
}

// ---- the two index policies ----
struct SgenAt {
    uint32_t t, k;  // tipset; run r or spec s of the spec list
};

// Who fills what (storage_claims_gen.hip): n_runs — every launcher; n — launch_sgen_specs and _run_records (0 elsewhere: the
// run kernels but the record kernel read no `n`); child_key, child_epoch — launch_sgen_run_records alone, zero elsewhere.  A
// kernel loads only the members it reads: the others cost bytes of its argument block, no instruction.
struct SgenOne {
    uint32_t n_runs, n;  // n: the specs
    CidKey child_key;
    long long child_epoch;
    static constexpr bool kSlotColumn = false;
    __device__ __forceinline__ uint32_t runs() const { return n_runs; }
    __device__ __forceinline__ uint32_t specs() const { return n; }
    __device__ __forceinline__ uint32_t list_specs() const { return n; }
    __device__ __forceinline__ SgenAt run_at(uint32_t i) const { return SgenAt{0u, i}; }
    __device__ __forceinline__ SgenAt spec_at(uint32_t i) const { return SgenAt{0u, i}; }
    __device__ __forceinline__ WitnessView view(const WitnessView& w, uint32_t) const { return w; }
    __device__ __forceinline__ bool run_actor(const StorageRun* __restrict__ runs, const uint64_t* __restrict__ actor_id, uint32_t i,
                                              SgenAt, uint64_t& actor) const {
        actor = actor_id[runs[i].first_claim];
        return true;
    }
    __device__ __forceinline__ bool spec_run(const uint32_t* __restrict__ run_of, SgenAt at, uint32_t& ri) const {
        ri = run_of[at.k];
        return true;
    }
    __device__ __forceinline__ bool run_stretch(const StorageRun* __restrict__ runs, uint32_t i, SgenAt, uint32_t& first,
                                                uint32_t& last) const {
        first = runs[i].first_claim;
        last = i + 1 < n_runs ? runs[i + 1].first_claim : n;
        return true;
    }
    __device__ __forceinline__ const CidKey& child(uint32_t) const { return child_key; }
    __device__ __forceinline__ long long epoch(uint32_t) const { return child_epoch; }
};

// runs0 / run_of0: the runs of the n_specs-entry list (n_runs0 of them); `words`: one row of the recorder.
// Who fills what (storage_claims_gen_tipsets.inc; the rest stays null): the four counts — every launcher (`words` = 0 by
// launch_sgent_run_records, which records nothing); runs0 — launch_sgent_runs, _run_actors, _run_records, NOT launch_sgent_specs:
// the spec kernels reach a run through run_of0 and must not call run_actor or run_stretch; children — launch_sgent_runs
// (k_sgent_heads) and _run_records; epochs — _run_records alone.
struct SgenChain {
    uint32_t n_tipsets, n_runs0, n_specs, words;
    const StorageRun* __restrict__ runs0;
    const CidKey* __restrict__ children;
    const long long* __restrict__ epochs;
    static constexpr bool kSlotColumn = true;
    // 32-bit products: the host refuses a chain with n_tipsets · n_specs ≥ 2³² − 1 (host/generate.cpp,
    // sgen_tipsets_refuse), and n_runs0 ≤ n_specs
    __device__ __forceinline__ uint32_t runs() const { return n_tipsets * n_runs0; }
    __device__ __forceinline__ uint32_t specs() const { return n_tipsets * n_specs; }
    __device__ __forceinline__ uint32_t list_specs() const { return n_specs; }
    __device__ __forceinline__ SgenAt run_at(uint32_t i) const {
        const uint32_t t = i / n_runs0;
        return SgenAt{t, i - t * n_runs0};
    }
    __device__ __forceinline__ SgenAt spec_at(uint32_t i) const {
        const uint32_t t = i / n_specs;
        return SgenAt{t, i - t * n_specs};
    }
    __device__ __forceinline__ WitnessView view(const WitnessView& w, uint32_t t) const {
        WitnessView v = w;
        v.touched = w.touched + size_t(t) * words;
        return v;
    }
    // the actor of run r of the spec list, or false when its record does not point into the list
    __device__ __forceinline__ bool run_actor(const StorageRun* __restrict__, const uint64_t* __restrict__ actor_id, uint32_t, SgenAt at,
                                              uint64_t& actor) const {
        const uint32_t first = runs0[at.k].first_claim;
        if (first >= n_specs) return false;
        actor = actor_id[first];
        return true;
    }
    __device__ __forceinline__ bool spec_run(const uint32_t* __restrict__ run_of0, SgenAt at, uint32_t& ri) const {
        const uint32_t r0 = run_of0[at.k];
        if (r0 >= n_runs0) return false;  // (no launcher leaves a spec without its run)
        ri = at.t * n_runs0 + r0;
        return true;
    }
    // [first, next run's first or the end), clipped to the list; false: nothing of the list is left at `first`
    __device__ __forceinline__ bool run_stretch(const StorageRun* __restrict__, uint32_t, SgenAt at, uint32_t& first,
                                                uint32_t& last) const {
        first = runs0[at.k].first_claim, last = at.k + 1 < n_runs0 ? runs0[at.k + 1].first_claim : n_specs;
        if (last > n_specs) last = n_specs;
        if (first > last) first = last;
        return first < n_specs;
    }
    __device__ __forceinline__ const CidKey& child(uint32_t t) const { return children[t]; }
    __device__ __forceinline__ long long epoch(uint32_t t) const { return epochs[t]; }
};

// Steps 1 and 3a: extract_and_verify_parent_state (storage/generator.rs:72-103) and the StateRoot behind the DERIVED state
// root (common/decode.rs:23-26): child header → parent_state_root → StateRoot.actors.  The single call decodes it once per
// run (one block, the same for all of them), the chain once per tipset.
__device__ __forceinline__ void chain_head(const WitnessView& w, const CidKey& child, CidKey& parent_state_root, CidKey& actors,
                                           uint32_t& hdr_status, uint32_t& sr_status) {
    zero_key(parent_state_root), zero_key(actors);
    sr_status = IPCFP_ST_ERR;
    HeaderLite hdr;
    uint32_t hb;
    hdr_status = load_header(w, child, hdr, hb);
    if (hdr_status != IPCFP_ST_TRUE) return;
    parent_state_root = hdr.parent_state_root;
    const uint32_t b = witness_find(w, hdr.parent_state_root);
    if (b == kNoBlock) {
        sr_status = IPCFP_ST_ERR_MISSING_BLOCK;
        return;
    }
    Rd r = open_block(w, b);
    CidKey info;
    r.expect_array(3);
    if (r.read_uint() > 5) r.fail();
    r.read_link_key(actors);
    r.read_link_key(info);
    r.finish();
    sr_status = r.ok() ? uint32_t(IPCFP_ST_TRUE) : uint32_t(IPCFP_ST_ERR_DECODE);
}

// the ActorState behind a found key (common/decode.rs:37, ActorState [code, state, …])
__device__ __forceinline__ uint32_t actor_state_of(const WitnessView& w, const ValueLoc& loc, CidKey& actor_state) {
    Rd v;
    v.init(w.arena + w.off[loc.block] + loc.off, loc.len);
    CidKey code;
    v.expect_array(5);
    v.read_link_key(code);
    v.read_link_key(actor_state);
    return v.ok() ? uint32_t(IPCFP_ST_TRUE) : uint32_t(IPCFP_ST_ERR_DECODE);
}

// Step 3b over the node table (hamt_table.h); a block the table does not cover leaves the run `undecided`
template <class P>
__global__ __launch_bounds__(256) void k_sgen_run_actors_table(P p, WitnessView w, const HamtNodeRec* __restrict__ table,
                                                               const uint64_t* __restrict__ actor_id, StorageRun* __restrict__ runs,
                                                               uint32_t undecided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.runs()) return;
    if (runs[i].actor_status != undecided) return;
    const SgenAt at = p.run_at(i);
    const WitnessView v = p.view(w, at.t);
    uint64_t actor;
    if (!p.run_actor(runs, actor_id, i, at, actor)) return;  // (the lane kernel settles it)
    uint8_t key[12];
    const uint32_t kl = id_address_bytes(actor, key);  // common/decode.rs:34
    ValueLoc loc;
    uint32_t st = table_hamt_get(v, table, runs[i].actors, 5, HK_ACTOR_STATE, key, kl, loc);  // decode.rs:29-37
    if (st == kTablePunt) return;
    CidKey actor_state;
    zero_key(actor_state);
    if (st == IPCFP_ST_NOT_FOUND) st = IPCFP_ST_ERR_ACTOR_NOT_FOUND;  // decode.rs:39
    if (st == IPCFP_ST_TRUE) st = actor_state_of(v, loc, actor_state);
    runs[i].actor_status = st;
    runs[i].actor_state = actor_state;
}

// … and by the walker: the runs the table left undecided, or every run of a batch that has no table
template <class P>
__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgen_run_actors_lane(P p, WitnessView w, const uint64_t* __restrict__ actor_id,
                                                                                StorageRun* __restrict__ runs, uint32_t undecided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.runs()) return;
    if (runs[i].actor_status != undecided) return;
    const SgenAt at = p.run_at(i);
    const WitnessView v = p.view(w, at.t);
    CidKey actor_state;
    zero_key(actor_state);
    uint32_t st = IPCFP_ST_ERR;
    uint64_t actor;
    if (p.run_actor(runs, actor_id, i, at, actor)) {
        uint8_t key[12];
        const uint32_t kl = id_address_bytes(actor, key);
        ValueLoc loc;
        st = hamt_get(v, runs[i].actors, 5, VK_ACTOR_STATE, key, kl, loc);
        if (st == IPCFP_ST_NOT_FOUND) st = IPCFP_ST_ERR_ACTOR_NOT_FOUND;
        if (st == IPCFP_ST_TRUE) st = actor_state_of(v, loc, actor_state);
    }
    runs[i].actor_status = st;
    runs[i].actor_state = actor_state;
}

// Step 3c: parse_evm_state behind the derived actor-state CID (:121-133), then which layout the derived contract_state
// decodes as (storage/decode.rs:46-96) — the first thing every spec of the run would find out for itself.
template <class P>
__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgen_run_state(P p, WitnessView w, StorageRun* __restrict__ runs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.runs()) return;
    const WitnessView v = p.view(w, p.run_at(i).t);
    StorageRun run = runs[i];
    if (run.hdr_status == IPCFP_ST_TRUE && run.sr_status == IPCFP_ST_TRUE && run.actor_status == IPCFP_ST_TRUE) {
        const uint32_t eb = witness_find(v, run.actor_state);
        run.evm_status = eb == kNoBlock ? uint32_t(IPCFP_ST_ERR_MISSING_BLOCK) : parse_evm_state(v, eb, run.contract_state);
        if (run.evm_status == IPCFP_ST_TRUE) run.root_kind = sniff_storage_root(v, run.contract_state, run.hamt_root, run.hamt_bw);
    }
    run.chain_status = chain_verdict(run);
    runs[i] = run;
}

// The first step of every storage get of a run, taken once (verify_storage.hip k_storage_run_children), 32 lanes per run:
// the root's block and the blocks behind its standard links; kNoBlock where the table has no record of the root, the pointer
// is no standard link or the block is missing (the spec's own lane then looks it up, recording).  The probes stay on a
// NON-recording view; only the root is marked here, in the run's own view.  The lane index is 64 bits wide, as the
// launchers' grid size is: 32 lanes per run pass 2^32 at 2^27 runs.
template <class P>
__global__ __launch_bounds__(256) void k_sgen_run_children(P p, WitnessView w, const HamtNodeRec* __restrict__ table,
                                                           const StorageRun* __restrict__ runs, uint32_t* __restrict__ root_block,
                                                           uint32_t* __restrict__ root_child) {
    const uint64_t lane = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t i64 = lane >> 5;
    const uint32_t q = uint32_t(lane) & 31u;
    if (i64 >= p.runs()) return;
    const uint32_t i = uint32_t(i64);
    WitnessView quiet = w;
    quiet.touched = nullptr;
    uint32_t rb = kNoBlock, child = kNoBlock;
    if (runs[i].chain_status == IPCFP_ST_TRUE && runs[i].root_kind == 3) {
        rb = witness_find(quiet, runs[i].hamt_root);  // (the 32 lanes of a run: the same probe, broadcast)
        if (rb != kNoBlock) {
            if (q == 0) mark_block(p.view(w, p.run_at(i).t), rb);
            const HamtNodeRec* rec = table + rb;
            const uint32_t head = *reinterpret_cast<const uint32_t*>(rec);
            if ((head & 0xffu) != 1u) {
                rb = kNoBlock;  // not tabulated: nothing is known about its pointers
            } else if (q < ((head >> 16) & 0xffu) && ((rec->std_links >> q) & 1u)) {
                const uint8_t* g = w.arena + w.off[rb] + rec->ptr_off[q];
                CidKey link;
#pragma unroll
                for (int j = 0; j < 5; ++j) __builtin_memcpy(&link.w[j], g + 5 + 8 * j, 8);
                link.w[4] &= (1ull << 48) - 1ull;
                child = witness_find(quiet, link);
            }
        }
    }
    root_child[size_t(i) * 32u + q] = child;
    if (q == 0) root_block[i] = rb;
}

// The block table_hamt_get steps into from a resolved root WITHOUT looking it up — its conditions for taking the root_children
// shortcut, in its order (walk_dev.h) — or kNoBlock when it takes the long way (and records for itself) or stops at the root.
__device__ __forceinline__ uint32_t root_step_child(const HamtNodeRec* __restrict__ table, uint32_t rb, uint32_t bit_width,
                                                    const uint64_t kw[4], const uint32_t* __restrict__ root_children) {
    if (rb == kNoBlock || bit_width < 1 || bit_width > 8) return kNoBlock;
    const uint4 rh = *reinterpret_cast<const uint4*>(table + rb);
    if ((rh.x & 0xffu) != 1u || !((rh.x >> 8) & HK_VEC_U8)) return kNoBlock;
    uint32_t h[8];
    sha256::hash32_words(kw, h);
    const uint32_t idx = sha256::take_bits(h, 0, bit_width);
    const uint64_t bf = uint64_t(rh.z) | (uint64_t(rh.w) << 32);
    if (idx >= 64u || !((bf >> idx) & 1ull)) return kNoBlock;
    const uint32_t rank = uint32_t(__popcll(bf & ((1ull << idx) - 1ull)));
    if (rank >= ((rh.x >> 16) & 0xffu) || !((rh.y >> rank) & 1u)) return kNoBlock;
    return root_children[rank];
}

// Step 4 over the node table, one spec per lane, in the shape of k_verify_storage_table<ColumnClaimSrc>: the slot is two
// 16-byte loads from the contiguous spec column, the get takes the key words in registers, the value is decoded out of the
// lane's LDS slot (storage_value_dev.h) and leaves as two 16-byte stores — a wavefront writes 2 KB of values contiguously.
// A spec it cannot settle (an inline small-map layout, a block the table does not cover) is left kStPending.
// `stepped` is a result of witness_find — below w.n or kNoBlock — so its bound changes no answer.
template <class P>
__global__ __launch_bounds__(256, 7) void k_sgen_specs_table(P p, WitnessView w, const HamtNodeRec* __restrict__ table,
                                                             const uint8_t* __restrict__ slot, const uint32_t* __restrict__ run_of,
                                                             const StorageRun* __restrict__ runs, const uint32_t* __restrict__ root_block,
                                                             const uint32_t* __restrict__ root_child, uint8_t* __restrict__ slot_out,
                                                             uint8_t* __restrict__ value, uint8_t* __restrict__ cflags,
                                                             uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.specs()) return;
    __shared__ ValueStage vstage;
    const SgenAt at = p.spec_at(i);
    const uint8_t* slot_p = slot + 32ull * at.k;
    uint64_t kw[4];
    if constexpr (P::kSlotColumn) {
        const Raw16 a = raw_ld128(slot_p), b = raw_ld128(slot_p + 16);
        kw[0] = a.lo, kw[1] = a.hi, kw[2] = b.lo, kw[3] = b.hi;
        store_32(slot_out, i, kw);
    }
    uint64_t padded[4] = {0, 0, 0, 0};
    uint32_t st = kStPending;
    uint32_t ri;
    if (!p.spec_run(run_of, at, ri)) {
        store_32(value, i, padded);
        cflags[i] = 0;
        status[i] = uint8_t(IPCFP_ST_ERR);
        return;
    }
    const StorageRun& run = runs[ri];
    const WitnessView v = p.view(w, at.t);
    do {
        const uint32_t chain = run.chain_status;
        if (chain != IPCFP_ST_TRUE) { st = chain; break; }
        if (run.root_kind == 4) { st = IPCFP_ST_ERR_MISSING_BLOCK; break; }  // decode.rs:41-43
        if (run.root_kind != 3) break;  // an inline small map (A1-A3): the one-lane kernel searches it
        if constexpr (!P::kSlotColumn) {
            const Raw16 a = raw_ld128(slot_p), b = raw_ld128(slot_p + 16);
            kw[0] = a.lo, kw[1] = a.hi, kw[2] = b.lo, kw[3] = b.hi;
        }
        ValueLoc loc;
        const uint32_t rb = root_block[ri];
        const uint32_t* kids = root_child + size_t(ri) * 32u;
        const uint32_t stepped = root_step_child(table, rb, run.hamt_bw, kw, kids);
        if (stepped != kNoBlock && stepped < w.n) mark_block(v, stepped);  // (the root: k_sgen_run_children)
        const uint32_t hs = table_hamt_get(v, table, run.hamt_root, run.hamt_bw, HK_VEC_U8, slot_p, 32, loc, rb, kids, kw);
        if (hs == kTablePunt) break;
        if (hs == IPCFP_ST_NOT_FOUND) { st = IPCFP_ST_TRUE; break; }  // unwrap_or_default(): a missing key means zero
        if (hs != IPCFP_ST_TRUE) { st = hs; break; }
        const uint8_t* vp = w.arena + w.off[loc.block] + loc.off;
        uint32_t L[8];
        {
            Raw16 tw[kValueStageWords / 2];
#pragma unroll
            for (uint32_t j = 0; j < kValueStageWords / 2; ++j) tw[j] = raw_ld128(vp + 16u * j);  // (≤ 80 bytes past a block: the arena's slack)
#pragma unroll
            for (uint32_t j = 0; j < kValueStageWords / 2; ++j) {
                vstage.w[2 * j][threadIdx.x] = tw[j].lo;
                vstage.w[2 * j + 1][threadIdx.x] = tw[j].hi;
            }
            vstage.w[kValueStageWords][threadIdx.x] = 0;
        }
        if (left_pad_32_staged(vstage, threadIdx.x, loc.len, L) || left_pad_32_raw(vp, loc.len, L)) {
#pragma unroll
            for (int k = 0; k < 4; ++k)  // byte i of the value: limb (31 - i) / 4, big-endian inside it
                padded[k] = uint64_t(__builtin_bswap32(L[7 - 2 * k])) | uint64_t(__builtin_bswap32(L[6 - 2 * k])) << 32;
        } else {
            Rd rd;
            rd.init(vp, loc.len);
            left_pad_32_words(rd, padded);
        }
        st = IPCFP_ST_TRUE;
    } while (false);
    status[i] = uint8_t(st);
    if (st == kStPending) return;
    store_32(value, i, padded);  // (zero unless the get found the slot)
    cflags[i] = st == IPCFP_ST_TRUE ? uint8_t(IPCFP_SCOL_FLAG_MASK) : uint8_t(0);
}

// read_storage_slot + left_pad_32 by the one-lane reader (storage_dev.h).  pending_only: what the table kernel left pending
// (it has written the slot column); else every spec, and the slot column with it.
template <class P>
__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgen_specs_lane(P p, WitnessView w, const uint8_t* __restrict__ slot,
                                                                           const uint32_t* __restrict__ run_of,
                                                                           const StorageRun* __restrict__ runs, uint8_t* __restrict__ slot_out,
                                                                           uint8_t* __restrict__ value, uint8_t* __restrict__ cflags,
                                                                           uint8_t* __restrict__ status, int pending_only) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.specs()) return;
    if (pending_only && status[i] != kStPending) return;
    const SgenAt at = p.spec_at(i);
    const uint8_t* slot_p = slot + 32ull * at.k;
    if constexpr (P::kSlotColumn) {
        if (!pending_only) {
            const Raw16 a = raw_ld128(slot_p), b = raw_ld128(slot_p + 16);
            const uint64_t kw[4] = {a.lo, a.hi, b.lo, b.hi};
            store_32(slot_out, i, kw);
        }
    }
    uint8_t padded[32];
    for (int k = 0; k < 32; ++k) padded[k] = 0;
    uint32_t st = IPCFP_ST_ERR;
    uint32_t ri;
    if (p.spec_run(run_of, at, ri)) {
        const StorageRun& run = runs[ri];
        st = run.chain_status;
        if (st == IPCFP_ST_TRUE) st = read_storage_slot_padded(p.view(w, at.t), run.contract_state, slot_p, padded);
    }
    uint64_t out[4] = {0, 0, 0, 0};
    if (st == IPCFP_ST_TRUE) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint64_t x = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) x |= uint64_t(padded[8 * k + j]) << (8 * j);
            out[k] = x;
        }
    }
    store_32(value, i, out);
    cflags[i] = st == IPCFP_ST_TRUE ? uint8_t(IPCFP_SCOL_FLAG_MASK) : uint8_t(0);
    status[i] = uint8_t(st);
}

// create_proof_claim's shared fields (storage/generator.rs:158-178), one record per run.  A chain that failed before
// contract_state was known leaves flags = 0 and the three derived CID slots zero: the record is well formed and the column
// verifier answers ERR_BAD_CLAIM for its claims.
template <class P>
__global__ __launch_bounds__(256) void k_sgen_run_records(P p, const StorageRun* __restrict__ runs, const uint64_t* __restrict__ actor_id,
                                                          StorageRunRec* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.runs()) return;
    const SgenAt at = p.run_at(i);
    const StorageRun& run = runs[i];
    const bool ok = run.chain_status == IPCFP_ST_TRUE;
    uint32_t first, last;  // the run's stretch of the spec list
    const bool any = p.run_stretch(runs, i, at, first, last);
    StorageRunRec rec;
    rec.child_epoch = p.epoch(at.t);
    rec.actor_id = any ? actor_id[first] : 0;
    rec.child = p.child(at.t);
    zero_key(rec.state_root), zero_key(rec.actor_state), zero_key(rec.storage_root);
    if (ok) {
        rec.state_root = run.parent_state_root;
        rec.actor_state = run.actor_state;
        rec.storage_root = run.contract_state;
    }
    rec.first_claim = at.t * p.list_specs() + first;
    rec.n_claims = last - first;
    rec.flags = ok ? uint32_t(IPCFP_SRUN_FLAG_MASK) : 0u;
    rec.reserved = 0;
    out[i] = rec;
}

}  // namespace ipcfp
