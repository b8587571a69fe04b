// csrc/kernels/storage_claims_gen.hip — `generate_storage_proof` finished as column claims in HBM, computed over runs.
//
// Replaces generate_storage_proof steps 1-4 and create_proof_claim (src/proofs/storage/generator.rs:72-178) for a batch of
// (actor_id, slot) specs of ONE child block, in the order generate_proof_bundle walks them (src/proofs/generator.rs:42-56) —
// and for ONE list of n_specs specs posed at each of T children (ipcfp_generate_storage_claims_tipsets*), answered as T
// single calls laid end to end.
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
// The seven kernels from k_sgen_run_actors_table on are templates over an index policy and have ONE text each
// (storage_claims_gen_body.h): <SgenOne> is the single call's, <SgenChain> that of a chain of child headers, whose own
// kernels (k_sgent_heads, k_sgent_run_init, the cut) and launchers are in storage_claims_gen_tipsets.inc, included at the end.
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

#include "launch.h"
#include "storage_claims_gen_body.h"

namespace ipcfp {

__global__ __launch_bounds__(256) void k_sgen_run_flags(const uint64_t* __restrict__ actor_id, uint32_t n, uint32_t* __restrict__ flag) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    flag[t] = (t == 0 || actor_id[t] != actor_id[t - 1]) ? 1u : 0u;
}

// Steps 1 and 3a of the single call: every run decodes the child header for itself
__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgen_run_chain(WitnessView w, CidKey child, StorageRun* __restrict__ runs,
                                                                          uint32_t n_runs, uint32_t undecided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_runs) return;
    StorageRun run;
    run.first_claim = runs[i].first_claim;
    zero_key(run.actor_state), zero_key(run.contract_state), zero_key(run.hamt_root);
    run.actor_status = run.evm_status = IPCFP_ST_ERR;
    run.root_kind = 4;
    run.hamt_bw = 5;
    chain_head(w, child, run.parent_state_root, run.actors, run.hdr_status, run.sr_status);
    if (run.hdr_status == IPCFP_ST_TRUE && run.sr_status == IPCFP_ST_TRUE) run.actor_status = undecided;
    run.chain_status = chain_verdict(run);
    runs[i] = run;
}

// ---- launchers (the context's stream; `w` is the recording view where the kernel fetches blocks — of a chain, the view whose
// `touched` is row 0 of the recorder).  The run, spec and record launches are the same for both policies. ----
namespace {

template <class P>
void sgen_run_actors(ipcfp_ctx* ctx, const P& p, uint64_t n_runs, const WitnessView& w, const void* table_d, const uint64_t* actor_id_d,
                     void* runs_d, uint32_t undecided) {
    const dim3 g(div_up(n_runs, 256)), blk(256);
    if (table_d)
        hipLaunchKernelGGL(k_sgen_run_actors_table<P>, g, blk, 0, ctx->stream, p, w, static_cast<const HamtNodeRec*>(table_d), actor_id_d,
                           static_cast<StorageRun*>(runs_d), undecided);
    hipLaunchKernelGGL(k_sgen_run_actors_lane<P>, g, blk, 0, ctx->stream, p, w, actor_id_d, static_cast<StorageRun*>(runs_d), undecided);
}

template <class P>
void sgen_specs(ipcfp_ctx* ctx, const P& p, uint64_t n_runs, uint64_t n, const WitnessView& w, const void* table_d, const uint8_t* slot_d,
                const uint32_t* run_of_d, const void* runs_d, uint32_t* root_children_d, uint8_t* slot_out_d, uint8_t* value_d,
                uint8_t* cflags_d, uint8_t* status_d) {
    const dim3 g(div_up(n, 256)), blk(256);
    if (table_d) {
        uint32_t* root_block = root_children_d;
        uint32_t* root_child = root_children_d + n_runs;
        hipLaunchKernelGGL(k_sgen_run_children<P>, dim3(div_up(n_runs * 32u, 256)), blk, 0, ctx->stream, p, w,
                           static_cast<const HamtNodeRec*>(table_d), static_cast<const StorageRun*>(runs_d), root_block, root_child);
        hipLaunchKernelGGL(k_sgen_specs_table<P>, g, blk, 0, ctx->stream, p, w, static_cast<const HamtNodeRec*>(table_d), slot_d, run_of_d,
                           static_cast<const StorageRun*>(runs_d), root_block, root_child, slot_out_d, value_d, cflags_d, status_d);
    }
    hipLaunchKernelGGL(k_sgen_specs_lane<P>, g, blk, 0, ctx->stream, p, w, slot_d, run_of_d, static_cast<const StorageRun*>(runs_d), slot_out_d,
                       value_d, cflags_d, status_d, table_d ? 1 : 0);
}

SgenOne one_child(uint32_t n_runs, uint32_t n) {
    SgenOne p{};
    p.n_runs = n_runs, p.n = n;
    return p;
}

}  // namespace

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
    sgen_run_actors(ctx, one_child(n_runs, 0), n_runs, w, table_d, actor_id_d, runs_d, undecided);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgen_run_state(ipcfp_ctx* ctx, const WitnessView& w, void* runs_d, uint32_t n_runs) {
    if (n_runs == 0) return IPCFP_OK;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
    hipLaunchKernelGGL(k_sgen_run_state<SgenOne>, dim3(div_up(n_runs, 256)), dim3(256), 0, ctx->stream, one_child(n_runs, 0), w,
                       static_cast<StorageRun*>(runs_d));
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgen_specs(ipcfp_ctx* ctx, const WitnessView& w, const void* table_d, const uint8_t* slot_d, uint32_t n, const uint32_t* run_of_d,
                      const void* runs_d, uint32_t n_runs, uint32_t* root_children_d, uint8_t* value_d, uint8_t* cflags_d,
                      uint8_t* status_d) {
    if (n == 0) return IPCFP_OK;
    if (table_d && !root_children_d) return set_error(ctx, IPCFP_E_INVALID, "the tabled route needs its per-run words");
    ProfileScope prof(ctx, IPCFP_K_SGEN_SPECS);
    sgen_specs(ctx, one_child(n_runs, n), n_runs, n, w, table_d, slot_d, run_of_d, runs_d, root_children_d, nullptr, value_d, cflags_d,
               status_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgen_run_records(ipcfp_ctx* ctx, const void* runs_d, uint32_t n_runs, uint32_t n, const CidKey& child, long long child_epoch,
                            const uint64_t* actor_id_d, void* out_d) {
    if (n_runs == 0) return IPCFP_OK;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RECORDS);
    SgenOne p = one_child(n_runs, n);
    p.child_key = child, p.child_epoch = child_epoch;
    hipLaunchKernelGGL(k_sgen_run_records<SgenOne>, dim3(div_up(n_runs, 256)), dim3(256), 0, ctx->stream, p,
                       static_cast<const StorageRun*>(runs_d), actor_id_d, static_cast<StorageRunRec*>(out_d));
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp

#include "storage_claims_gen_tipsets.inc"  // what only a chain of child headers has, and its launchers
