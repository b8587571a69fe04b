// csrc/kernels/storage_runs.h — what consecutive storage claims share.
//
// `verify_storage_proof` (src/proofs/storage/verifier.rs:24-63) derives, for every proof anew, facts that depend only on
// (child_block_cid, parent_state_root, actor_id, actor_state_cid, storage_root): the child header's parent_state_root
// (:95-111), the actor's state CID behind the state root (:114-127, common/decode.rs:17-42), the EVM state's
// contract_state (:130-145, common/decode.rs:79-97) and which of the six layouts the storage root decodes as
// (storage/decode.rs:46-96).  A bundle asks them of one contract hundreds of times in a row (src/proofs/verifier.rs:19-28
// walks the proofs in order).  Here a RUN = a maximal stretch of consecutive claims that agree on those five fields; the
// facts are computed once per run (exact key comparison, pure functions of the witness) and every claim is then judged
// in the reference's order of checks from its run's record plus its own flags, slot and value.
#pragma once
#include <cstddef>
#include <cstdint>

#include "claims_dev.h"
#include "witness_dev.h"

namespace ipcfp {

struct StorageRun {
    uint32_t first_claim;        // index of the run's first claim
    uint32_t hdr_status;         // TRUE or the ERR_* of get(child) + HeaderLite decode
    CidKey parent_state_root;
    uint32_t sr_status;          // StateRoot block: TRUE / ERR_MISSING_BLOCK / ERR_DECODE
    uint32_t actor_status;       // Hamt get + ActorState decode: TRUE / ERR_ACTOR_NOT_FOUND / ERR_* / kCoopPunt (undecided)
    CidKey actors;               // StateRoot.actors
    CidKey actor_state;          // ActorState.state of the run's actor
    uint32_t evm_status;         // get(actor_state_cid) + parse_evm_state: TRUE / ERR_MISSING_BLOCK / ERR_DECODE
    uint32_t root_kind;          // 0 = inline A1, 1 = A2, 2 = A3, 3 = HAMT (hamt_root, hamt_bw: B1 / B2 / C), 4 = root block missing
    CidKey contract_state;       // EvmState.contract_state
    CidKey hamt_root;
    uint32_t hamt_bw;
    uint32_t chain_status;       // the GENERATOR's word (storage_claims_gen.hip): TRUE when contract_state is known, else the ERR_* of
                                 // the chain; the verifier's run kernels neither write nor read it
};

// ---- where the claims come from ---------------------------------------------------------------------------------------
// The kernels that derive a run's facts, and the claim kernels, are templates over a CLAIM SOURCE: the plain 248-byte
// records (claims_dev.h StorageClaimPacked) or the run-compressed column form (include/ipcfp.h "storage claims in
// run-compressed, column form").  A source answers two questions:
//   run_key(i, first)   the record that holds run i's child, state_root, actor_state, storage_root and actor_id — the
//                       run's first claim, or its record of the run table
//   claim(t, run_of)    claim t as the one-lane kernel reads it (verify_storage_one): the record itself, or a view of
//                       the run record + the columns
// One body per kernel: the two routes cannot drift.
struct StorageRunRec {  // one record of the run table (IPCFP_SRUN_*)
    long long child_epoch;
    uint64_t actor_id;
    CidKey child, state_root, actor_state, storage_root;
    uint32_t first_claim, n_claims, flags, reserved;
};
static_assert(sizeof(StorageRunRec) == IPCFP_SRUN_BYTES && offsetof(StorageRunRec, child_epoch) == IPCFP_SRUN_OFF_CHILD_EPOCH &&
                  offsetof(StorageRunRec, actor_id) == IPCFP_SRUN_OFF_ACTOR_ID && offsetof(StorageRunRec, child) == IPCFP_SRUN_OFF_CHILD &&
                  offsetof(StorageRunRec, state_root) == IPCFP_SRUN_OFF_STATE_ROOT &&
                  offsetof(StorageRunRec, actor_state) == IPCFP_SRUN_OFF_ACTOR_STATE &&
                  offsetof(StorageRunRec, storage_root) == IPCFP_SRUN_OFF_STORAGE_ROOT &&
                  offsetof(StorageRunRec, first_claim) == IPCFP_SRUN_OFF_FIRST_CLAIM && offsetof(StorageRunRec, n_claims) == IPCFP_SRUN_OFF_N_CLAIMS &&
                  offsetof(StorageRunRec, flags) == IPCFP_SRUN_OFF_FLAGS && offsetof(StorageRunRec, reserved) == IPCFP_SRUN_OFF_RESERVED,
              "run record layout");
static_assert(IPCFP_SRUN_FLAG_MASK == (SC_CHILD_PARSED | SC_STATE_ROOT_CANON | SC_ACTOR_STATE_CANON | SC_STORAGE_ROOT_CANON) &&
                  IPCFP_SCOL_FLAG_MASK == (SC_SLOT_PARSED | SC_VALUE_MATCHABLE),
              "flag split");

// The per-run word the claim kernel reads beside its run's record (run_match): bits 0-2 the three claimed-vs-derived
// CID comparisons, made once per run by k_storage_run_children (8 = nobody has compared: no launcher leaves a run at
// that any more; k_verify_storage_table still reads it, its body being kept as it was).  The column route adds what a
// claim would otherwise fetch from the run table: its CID flag bits, the trust policy's answer for the run's epoch,
// and whether the record carries bits nobody knows.
enum : uint32_t {
    RM_STATE_ROOT = 1u, RM_ACTOR_STATE = 2u, RM_STORAGE_ROOT = 4u, RM_NOT_COMPARED = 8u,
    RM_FLAGS_SHIFT = 4,  // bits 4-7: the run's IPCFP_SRUN_FLAG_MASK bits
    RM_TRUSTED = 1u << 8, RM_BAD_RECORD = 1u << 9,
};

struct PlainClaimSrc {
    static constexpr bool kColumns = false;
    const StorageClaimPacked* claims;
    __device__ __forceinline__ const StorageClaimPacked& run_key(uint32_t, uint32_t first_claim) const { return claims[first_claim]; }
    __device__ __forceinline__ const StorageClaimPacked& claim(uint32_t t, const uint32_t*) const { return claims[t]; }
};

struct ColumnClaimView {  // the members verify_storage_one names
    const long long& child_epoch;
    const uint64_t& actor_id;
    const CidKey &child, &state_root, &actor_state, &storage_root;
    const uint8_t *slot, *value;
    uint32_t flags;
};

struct ColumnClaimSrc {
    static constexpr bool kColumns = true;
    const StorageRunRec* runs;
    const uint8_t *slot, *value, *cflags;
    __device__ __forceinline__ const StorageRunRec& run_key(uint32_t i, uint32_t) const { return runs[i]; }
    // (a record or a byte with unknown bits: no CHILD_PARSED, so verify_storage_one's first check answers ERR_BAD_CLAIM)
    __device__ __forceinline__ ColumnClaimView claim(uint32_t t, const uint32_t* run_of) const {
        const StorageRunRec& r = runs[run_of[t]];
        const uint32_t cf = cflags[t];
        const bool known = !(r.flags & ~IPCFP_SRUN_FLAG_MASK) && r.reserved == 0 && !(cf & ~IPCFP_SCOL_FLAG_MASK);
        return ColumnClaimView{r.child_epoch, r.actor_id, r.child, r.state_root, r.actor_state, r.storage_root,
                               slot + 32ull * t, value + 32ull * t, known ? (r.flags | cf) : 0u};
    }
};

}  // namespace ipcfp
