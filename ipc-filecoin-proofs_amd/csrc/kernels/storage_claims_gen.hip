// csrc/kernels/storage_claims_gen.hip — `generate_storage_proof` finished as column claims in HBM, computed over runs.
//
// Replaces generate_storage_proof steps 1-4 and create_proof_claim (src/proofs/storage/generator.rs:72-178) for a batch of
// (actor_id, slot) specs of ONE child block, in the order generate_proof_bundle walks them (src/proofs/generator.rs:42-56).
// kernels/generate.hip gives every spec a lane that decodes the header, the StateRoot, the actors-HAMT path and the EVM
// state for itself; a batch asks them of one contract hundreds of times in a row.  Here a RUN is a maximal stretch of
// consecutive specs with equal actor_id — one call has one child and one epoch, so everything else a run record holds
// (include/ipcfp.h IPCFP_SRUN_*) is a function of the actor — and the chain is walked once per run:
//
//   k_sgen_run_flags      one lane per spec: does a run start here          (then launch_scan_u32, launch_storage_run_heads)
//   k_sgen_run_chain      one lane per run: child header → parent_state_root → StateRoot.actors            (steps 1, 3a)
//   k_sgen_run_actors_*   the actor get over the node table; the lane walker takes what the table punts on      (step 3b)
//   k_sgen_run_state      EVM state behind the DERIVED actor-state CID, layout sniff of the DERIVED contract_state (step 3c)
//   k_sgen_run_children   32 lanes per run: the storage HAMT root's block and the blocks behind its links, resolved once
//   k_sgen_specs_table    one lane per spec: table_hamt_get of its slot, left_pad_32, value / cflags / status      (step 4)
//   k_sgen_specs_lane     the one-lane read_storage_slot for what that leaves pending (inline maps, punts) — or everything
//   k_sgen_run_records    the 192-byte run records (create_proof_claim's shared fields)
//
// The verifier's run kernels (verify_storage.hip) read CLAIMED CIDs, so their three run-level steps are independent; the
// generator's are dependent, hence the kernels of its own.  The device functions are the verifier's.
//
// The recorder.  Every kernel here that fetches a block gets the RECORDING view (WitnessView::touched), and every fetch but
// two goes through witness_find.  Run-level blocks (child header, StateRoot, the actors path, the EVM state, the storage root's
// block, the root node of the storage HAMT) are marked once per run, by the run kernels: the three RecordingBlockStores of every
// spec of the run would see exactly those.  The two exceptions are the first step of a spec's get, taken once per run as the
// verifier takes it: k_sgen_run_children probes ALL of a root's up-to-32 links, so it probes on a NON-recording view, and
// table_hamt_get, given the resolved root and children, looks neither up.  The root is marked by the children kernel (every
// spec of a run whose chain holds fetches it, whatever becomes of its get); the ONE child a spec steps into is marked by the
// spec kernel, which repeats table_hamt_get's conditions for taking the shortcut (root_step_child) — `get` is one fetch per
// visited node, and a node no spec visits stays unmarked.  A punt leaves the marks of the path up to the block the table does
// not cover; the walker that takes over marks the same path again and goes on.
#include <hip/hip_runtime.h>

#include "../common.h"
#include "claims_dev.h"
#include "hamt_table.h"
#include "launch.h"
#include "storage_dev.h"
#include "storage_runs.h"
#include "storage_value_dev.h"

namespace ipcfp {

namespace {

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
// value + 32 t as two 16-byte vector stores (the column lies on a 16-byte boundary)
__device__ __forceinline__ void store_value(uint8_t* __restrict__ value, uint32_t t, const uint64_t v[4]) {
    Out16* o = reinterpret_cast<Out16*>(value + 32ull * t);
    o[0] = Out16{v[0], v[1]};
    o[1] = Out16{v[2], v[3]};
}

}  // namespace

__global__ __launch_bounds__(256) void k_sgen_run_flags(const uint64_t* __restrict__ actor_id, uint32_t n, uint32_t* __restrict__ flag) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    flag[t] = (t == 0 || actor_id[t] != actor_id[t - 1]) ? 1u : 0u;
}

// Steps 1 and 3a: extract_and_verify_parent_state (:72-103) and the StateRoot behind the DERIVED state root
// (common/decode.rs:23-26).  Every run decodes the child header for itself: it is one block, the same for all of them.
__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgen_run_chain(WitnessView w, CidKey child, StorageRun* __restrict__ runs,
                                                                          uint32_t n_runs, uint32_t undecided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_runs) return;
    StorageRun run;
    run.first_claim = runs[i].first_claim;
    zero_key(run.parent_state_root), zero_key(run.actors), zero_key(run.actor_state), zero_key(run.contract_state), zero_key(run.hamt_root);
    run.sr_status = run.actor_status = run.evm_status = IPCFP_ST_ERR;
    run.root_kind = 4;
    run.hamt_bw = 5;
    HeaderLite hdr;
    uint32_t hb;
    run.hdr_status = load_header(w, child, hdr, hb);
    if (run.hdr_status == IPCFP_ST_TRUE) {
        run.parent_state_root = hdr.parent_state_root;
        const uint32_t b = witness_find(w, hdr.parent_state_root);
        if (b == kNoBlock) {
            run.sr_status = IPCFP_ST_ERR_MISSING_BLOCK;
        } else {
            Rd r = open_block(w, b);
            CidKey info;
            r.expect_array(3);
            if (r.read_uint() > 5) r.fail();
            r.read_link_key(run.actors);
            r.read_link_key(info);
            r.finish();
            run.sr_status = r.ok() ? uint32_t(IPCFP_ST_TRUE) : uint32_t(IPCFP_ST_ERR_DECODE);
        }
        if (run.sr_status == IPCFP_ST_TRUE) run.actor_status = undecided;
    }
    run.chain_status = chain_verdict(run);
    runs[i] = run;
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
__global__ __launch_bounds__(256) void k_sgen_run_actors_table(WitnessView w, const HamtNodeRec* __restrict__ table,
                                                               const uint64_t* __restrict__ actor_id, StorageRun* __restrict__ runs,
                                                               uint32_t n_runs, uint32_t undecided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_runs) return;
    if (runs[i].actor_status != undecided) return;
    uint8_t key[12];
    const uint32_t kl = id_address_bytes(actor_id[runs[i].first_claim], key);  // common/decode.rs:34
    ValueLoc loc;
    uint32_t st = table_hamt_get(w, table, runs[i].actors, 5, HK_ACTOR_STATE, key, kl, loc);  // decode.rs:29-37
    if (st == kTablePunt) return;
    CidKey actor_state;
    zero_key(actor_state);
    if (st == IPCFP_ST_NOT_FOUND) st = IPCFP_ST_ERR_ACTOR_NOT_FOUND;  // decode.rs:39
    if (st == IPCFP_ST_TRUE) st = actor_state_of(w, loc, actor_state);
    runs[i].actor_status = st;
    runs[i].actor_state = actor_state;
}

// … and by the walker: the runs the table left undecided, or every run of a batch that has no table
__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgen_run_actors_lane(WitnessView w, const uint64_t* __restrict__ actor_id,
                                                                                StorageRun* __restrict__ runs, uint32_t n_runs,
                                                                                uint32_t undecided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_runs) return;
    if (runs[i].actor_status != undecided) return;
    uint8_t key[12];
    const uint32_t kl = id_address_bytes(actor_id[runs[i].first_claim], key);
    ValueLoc loc;
    uint32_t st = hamt_get(w, runs[i].actors, 5, VK_ACTOR_STATE, key, kl, loc);
    CidKey actor_state;
    zero_key(actor_state);
    if (st == IPCFP_ST_NOT_FOUND) st = IPCFP_ST_ERR_ACTOR_NOT_FOUND;
    if (st == IPCFP_ST_TRUE) st = actor_state_of(w, loc, actor_state);
    runs[i].actor_status = st;
    runs[i].actor_state = actor_state;
}

// Step 3c: parse_evm_state behind the derived actor-state CID (:121-133), then which layout the derived contract_state
// decodes as (storage/decode.rs:46-96) — the first thing every spec of the run would find out for itself.
__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgen_run_state(WitnessView w, StorageRun* __restrict__ runs, uint32_t n_runs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_runs) return;
    StorageRun run = runs[i];
    if (run.hdr_status == IPCFP_ST_TRUE && run.sr_status == IPCFP_ST_TRUE && run.actor_status == IPCFP_ST_TRUE) {
        const uint32_t eb = witness_find(w, run.actor_state);
        run.evm_status = eb == kNoBlock ? uint32_t(IPCFP_ST_ERR_MISSING_BLOCK) : parse_evm_state(w, eb, run.contract_state);
        if (run.evm_status == IPCFP_ST_TRUE) run.root_kind = sniff_storage_root(w, run.contract_state, run.hamt_root, run.hamt_bw);
    }
    run.chain_status = chain_verdict(run);
    runs[i] = run;
}

// The first step of every storage get of a run, taken once (verify_storage.hip k_storage_run_children): the root's block and the
// blocks behind its standard links; kNoBlock where the table has no record of the root, the pointer is no standard link or the
// block is missing (the spec's own lane then looks it up, recording).  Only the root is marked here.
__global__ __launch_bounds__(256) void k_sgen_run_children(WitnessView w, const HamtNodeRec* __restrict__ table,
                                                           const StorageRun* __restrict__ runs, uint32_t n_runs,
                                                           uint32_t* __restrict__ root_block, uint32_t* __restrict__ root_child) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t >> 5, p = t & 31u;
    if (i >= n_runs) return;
    WitnessView quiet = w;
    quiet.touched = nullptr;
    uint32_t rb = kNoBlock, child = kNoBlock;
    if (runs[i].chain_status == IPCFP_ST_TRUE && runs[i].root_kind == 3) {
        rb = witness_find(quiet, runs[i].hamt_root);  // (the 32 lanes of a run: the same probe, broadcast)
        if (rb != kNoBlock) {
            if (p == 0) mark_block(w, rb);
            const HamtNodeRec* rec = table + rb;
            const uint32_t head = *reinterpret_cast<const uint32_t*>(rec);
            if ((head & 0xffu) != 1u) {
                rb = kNoBlock;  // not tabulated: nothing is known about its pointers
            } else if (p < ((head >> 16) & 0xffu) && ((rec->std_links >> p) & 1u)) {
                const uint8_t* g = w.arena + w.off[rb] + rec->ptr_off[p];
                CidKey link;
#pragma unroll
                for (int j = 0; j < 5; ++j) __builtin_memcpy(&link.w[j], g + 5 + 8 * j, 8);
                link.w[4] &= (1ull << 48) - 1ull;
                child = witness_find(quiet, link);
            }
        }
    }
    root_child[size_t(i) * 32u + p] = child;
    if (p == 0) root_block[i] = rb;
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
__global__ __launch_bounds__(256, 7) void k_sgen_specs_table(WitnessView w, const HamtNodeRec* __restrict__ table,
                                                             const uint8_t* __restrict__ slot, uint32_t n,
                                                             const uint32_t* __restrict__ run_of, const StorageRun* __restrict__ runs,
                                                             const uint32_t* __restrict__ root_block,
                                                             const uint32_t* __restrict__ root_child, uint8_t* __restrict__ value,
                                                             uint8_t* __restrict__ cflags, uint8_t* __restrict__ status) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    __shared__ ValueStage vstage;
    const uint32_t ri = run_of[t];
    const StorageRun& run = runs[ri];
    uint64_t padded[4] = {0, 0, 0, 0};
    uint32_t st = kStPending;
    do {
        const uint32_t chain = run.chain_status;
        if (chain != IPCFP_ST_TRUE) { st = chain; break; }
        if (run.root_kind == 4) { st = IPCFP_ST_ERR_MISSING_BLOCK; break; }  // decode.rs:41-43
        if (run.root_kind != 3) break;  // an inline small map (A1-A3): the one-lane kernel searches it
        const uint8_t* slot_p = slot + 32ull * t;
        uint64_t kw[4];
        {
            const Raw16 a = raw_ld128(slot_p), b = raw_ld128(slot_p + 16);
            kw[0] = a.lo, kw[1] = a.hi, kw[2] = b.lo, kw[3] = b.hi;
        }
        ValueLoc loc;
        const uint32_t rb = root_block[ri];
        const uint32_t* kids = root_child + size_t(ri) * 32u;
        const uint32_t stepped = root_step_child(table, rb, run.hamt_bw, kw, kids);
        if (stepped != kNoBlock) mark_block(w, stepped);  // (the root: k_sgen_run_children)
        const uint32_t hs = table_hamt_get(w, table, run.hamt_root, run.hamt_bw, HK_VEC_U8, slot_p, 32, loc, rb, kids, kw);
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
            Rd v;
            v.init(vp, loc.len);
            left_pad_32_words(v, padded);
        }
        st = IPCFP_ST_TRUE;
    } while (false);
    status[t] = uint8_t(st);
    if (st == kStPending) return;
    store_value(value, t, padded);  // (zero unless the get found the slot)
    cflags[t] = st == IPCFP_ST_TRUE ? uint8_t(IPCFP_SCOL_FLAG_MASK) : uint8_t(0);
}

// read_storage_slot + left_pad_32 by the one-lane reader (storage_dev.h): what the table kernel left pending, or every spec
__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgen_specs_lane(WitnessView w, const uint8_t* __restrict__ slot, uint32_t n,
                                                                           const uint32_t* __restrict__ run_of,
                                                                           const StorageRun* __restrict__ runs, uint8_t* __restrict__ value,
                                                                           uint8_t* __restrict__ cflags, uint8_t* __restrict__ status,
                                                                           int pending_only) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    if (pending_only && status[t] != kStPending) return;
    const StorageRun& run = runs[run_of[t]];
    uint8_t padded[32];
    for (int i = 0; i < 32; ++i) padded[i] = 0;
    uint32_t st = run.chain_status;
    if (st == IPCFP_ST_TRUE) st = read_storage_slot_padded(w, run.contract_state, slot + 32ull * t, padded);
    uint64_t v[4] = {0, 0, 0, 0};
    if (st == IPCFP_ST_TRUE) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint64_t x = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) x |= uint64_t(padded[8 * k + j]) << (8 * j);
            v[k] = x;
        }
    }
    store_value(value, t, v);
    cflags[t] = st == IPCFP_ST_TRUE ? uint8_t(IPCFP_SCOL_FLAG_MASK) : uint8_t(0);
    status[t] = uint8_t(st);
}

// create_proof_claim's shared fields (storage/generator.rs:158-178), one record per run.  A chain that failed before
// contract_state was known leaves flags = 0 and the three derived CID slots zero: the record is well formed and the column
// verifier answers ERR_BAD_CLAIM for its claims.
__global__ __launch_bounds__(256) void k_sgen_run_records(const StorageRun* __restrict__ runs, uint32_t n_runs, uint32_t n, CidKey child,
                                                          long long child_epoch, const uint64_t* __restrict__ actor_id,
                                                          StorageRunRec* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_runs) return;
    const StorageRun& run = runs[i];
    const bool ok = run.chain_status == IPCFP_ST_TRUE;
    StorageRunRec rec;
    rec.child_epoch = child_epoch;
    rec.actor_id = actor_id[run.first_claim];
    rec.child = child;
    zero_key(rec.state_root), zero_key(rec.actor_state), zero_key(rec.storage_root);
    if (ok) {
        rec.state_root = run.parent_state_root;
        rec.actor_state = run.actor_state;
        rec.storage_root = run.contract_state;
    }
    rec.first_claim = run.first_claim;
    rec.n_claims = (i + 1 < n_runs ? runs[i + 1].first_claim : n) - run.first_claim;
    rec.flags = ok ? uint32_t(IPCFP_SRUN_FLAG_MASK) : 0u;
    rec.reserved = 0;
    out[i] = rec;
}

// ---- launchers (the context's stream; `w` is the recording view where the kernel fetches blocks) ----
int launch_sgen_run_flags(ipcfp_ctx* ctx, const uint64_t* actor_id_d, uint32_t n, uint32_t* flag_d) {
    if (n == 0) return IPCFP_OK;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
    hipLaunchKernelGGL(k_sgen_run_flags, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, actor_id_d, n, flag_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgen_run_chain(ipcfp_ctx* ctx, const WitnessView& w, const CidKey& child, void* runs_d, uint32_t n_runs, uint32_t undecided) {
    if (n_runs == 0) return IPCFP_OK;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
    hipLaunchKernelGGL(k_sgen_run_chain, dim3(div_up(n_runs, 256)), dim3(256), 0, ctx->stream, w, child, static_cast<StorageRun*>(runs_d),
                       n_runs, undecided);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgen_run_actors(ipcfp_ctx* ctx, const WitnessView& w, const void* table_d, const uint64_t* actor_id_d, void* runs_d,
                           uint32_t n_runs, uint32_t undecided) {
    if (n_runs == 0) return IPCFP_OK;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
    const dim3 g(div_up(n_runs, 256)), blk(256);
    if (table_d)
        hipLaunchKernelGGL(k_sgen_run_actors_table, g, blk, 0, ctx->stream, w, static_cast<const HamtNodeRec*>(table_d), actor_id_d,
                           static_cast<StorageRun*>(runs_d), n_runs, undecided);
    hipLaunchKernelGGL(k_sgen_run_actors_lane, g, blk, 0, ctx->stream, w, actor_id_d, static_cast<StorageRun*>(runs_d), n_runs, undecided);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgen_run_state(ipcfp_ctx* ctx, const WitnessView& w, void* runs_d, uint32_t n_runs) {
    if (n_runs == 0) return IPCFP_OK;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
    hipLaunchKernelGGL(k_sgen_run_state, dim3(div_up(n_runs, 256)), dim3(256), 0, ctx->stream, w, static_cast<StorageRun*>(runs_d), n_runs);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgen_specs(ipcfp_ctx* ctx, const WitnessView& w, const void* table_d, const uint8_t* slot_d, uint32_t n, const uint32_t* run_of_d,
                      const void* runs_d, uint32_t n_runs, uint32_t* root_children_d, uint8_t* value_d, uint8_t* cflags_d,
                      uint8_t* status_d) {
    if (n == 0) return IPCFP_OK;
    if (table_d && !root_children_d) return set_error(ctx, IPCFP_E_INVALID, "the tabled route needs its per-run words");
    ProfileScope prof(ctx, IPCFP_K_SGEN_SPECS);
    const dim3 g(div_up(n, 256)), blk(256);
    if (table_d) {
        uint32_t* root_block = root_children_d;
        uint32_t* root_child = root_children_d + n_runs;
        hipLaunchKernelGGL(k_sgen_run_children, dim3(div_up(uint64_t(n_runs) * 32u, 256)), blk, 0, ctx->stream, w,
                           static_cast<const HamtNodeRec*>(table_d), static_cast<const StorageRun*>(runs_d), n_runs, root_block, root_child);
        hipLaunchKernelGGL(k_sgen_specs_table, g, blk, 0, ctx->stream, w, static_cast<const HamtNodeRec*>(table_d), slot_d, n, run_of_d,
                           static_cast<const StorageRun*>(runs_d), root_block, root_child, value_d, cflags_d, status_d);
    }
    hipLaunchKernelGGL(k_sgen_specs_lane, g, blk, 0, ctx->stream, w, slot_d, n, run_of_d, static_cast<const StorageRun*>(runs_d), value_d,
                       cflags_d, status_d, table_d ? 1 : 0);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgen_run_records(ipcfp_ctx* ctx, const void* runs_d, uint32_t n_runs, uint32_t n, const CidKey& child, long long child_epoch,
                            const uint64_t* actor_id_d, void* out_d) {
    if (n_runs == 0) return IPCFP_OK;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RECORDS);
    hipLaunchKernelGGL(k_sgen_run_records, dim3(div_up(n_runs, 256)), dim3(256), 0, ctx->stream, static_cast<const StorageRun*>(runs_d), n_runs,
                       n, child, child_epoch, actor_id_d, static_cast<StorageRunRec*>(out_d));
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp

#include "storage_claims_gen_tipsets.inc"  // the same for a chain of child headers, on the helpers above
