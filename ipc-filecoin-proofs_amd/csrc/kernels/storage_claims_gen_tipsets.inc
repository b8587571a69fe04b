// csrc/kernels/storage_claims_gen_tipsets.inc — the storage generator for a CHAIN of child headers
// (ipcfp_generate_storage_claims_tipsets*, host/generate.cpp): ONE list of n_specs (actor_id, slot) specs posed at each of T
// children, answered as T single calls laid end to end.
//
// Included at the end of storage_claims_gen.hip.  The dependent chain and the spec kernels are the single call's kernel
// templates instantiated over SgenChain (storage_claims_gen_body.h: the index (tipset, run) or (tipset, spec) and the
// recorder's row chosen per lane), launched through that file's sgen_run_actors / sgen_specs; here is what only a chain has.
//
// The runs are those of the spec list (R0 of them, discovered once by the single call's kernels): the chain has T·R0 runs,
// run (t, r) = t·R0 + r, and claim (t, s) = t·n_specs + s.  A run never crosses a tipset.
//
//   k_sgent_heads            one lane per tipset: child header → parent_state_root → StateRoot.actors, into a 96-byte record
//   k_sgent_run_init         one lane per (t, r): the run's StorageRun from its tipset's record — no header is decoded twice
//
// The recorder is T bitmap rows of `words` = ceil(blocks / 32) words: a lane of tipset t works on a copy of the WitnessView
// whose `touched` points at row t (SgenChain::view), so that what it fetches is recorded for its own tipset only.  The cut:
//
//   k_sgent_union            one lane per word: the OR of the T rows — what the host's materialize orders, once
//   k_sgent_cut_masks        one lane per (t, 32 positions of the ordered union): which of them row t holds, and how many
//   k_sgent_cut_fill         behind launch_scan_u32: tipset t's ids in the union's order, and the CSR offsets
//
// Every index read from a device record (a run's first claim, a spec's run, a union position's block id) is compared with
// its bound before it indexes anything; t comes from the lane index and is below T by the grid's bound.

namespace ipcfp {

struct SgenTipsetHead {  // what every run of a tipset shares
    CidKey parent_state_root, actors;
    uint32_t hdr_status, sr_status, pad[2];
};
static_assert(sizeof(SgenTipsetHead) == 96, "one tipset record");

__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgent_heads(WitnessView w, SgenChain c, SgenTipsetHead* __restrict__ heads) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= c.n_tipsets) return;
    SgenTipsetHead h;
    h.pad[0] = h.pad[1] = 0;
    chain_head(c.view(w, t), c.children[t], h.parent_state_root, h.actors, h.hdr_status, h.sr_status);
    heads[t] = h;
}

__global__ __launch_bounds__(256) void k_sgent_run_init(const SgenTipsetHead* __restrict__ heads, SgenChain c, StorageRun* __restrict__ runs,
                                                        uint32_t undecided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_tipsets * c.n_runs0) return;
    const uint32_t t = i / c.n_runs0, r = i - t * c.n_runs0;
    const SgenTipsetHead h = heads[t];
    StorageRun run;
    run.first_claim = t * c.n_specs + c.runs0[r].first_claim;
    run.hdr_status = h.hdr_status;
    run.parent_state_root = h.parent_state_root;
    run.sr_status = h.sr_status;
    run.actors = h.actors;
    zero_key(run.actor_state), zero_key(run.contract_state), zero_key(run.hamt_root);
    run.actor_status = run.evm_status = IPCFP_ST_ERR;
    run.root_kind = 4;
    run.hamt_bw = 5;
    if (run.hdr_status == IPCFP_ST_TRUE && run.sr_status == IPCFP_ST_TRUE) run.actor_status = undecided;
    run.chain_status = chain_verdict(run);
    runs[i] = run;
}

// ---- the cut -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sgent_union(const uint32_t* __restrict__ rows, uint32_t n_tipsets, uint32_t words,
                                                     uint32_t* __restrict__ out) {
    const uint32_t wd = blockIdx.x * blockDim.x + threadIdx.x;
    if (wd >= words) return;
    uint32_t m = 0;
    for (uint32_t t = 0; t < n_tipsets; ++t) m |= rows[size_t(t) * words + wd];
    out[wd] = m;
}

// chunk j of tipset t: positions [32 j, 32 j + 32) of the ordered union (n_union ids, per_tipset = ceil(n_union / 32) chunks)
__global__ __launch_bounds__(256) void k_sgent_cut_masks(const uint32_t* __restrict__ rows, uint32_t n_tipsets, uint32_t words,
                                                         uint32_t n_blocks, const uint32_t* __restrict__ union_ids, uint32_t n_union,
                                                         uint32_t per_tipset, uint32_t* __restrict__ mask, uint32_t* __restrict__ count) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tipsets * per_tipset) return;
    const uint32_t t = i / per_tipset, j = i - t * per_tipset;
    const uint32_t* row = rows + size_t(t) * words;
    uint32_t m = 0;
    for (uint32_t k = 0; k < 32; ++k) {
        const uint32_t p = 32u * j + k;
        if (p >= n_union) break;
        const uint32_t b = union_ids[p];
        if (b < n_blocks && ((row[b >> 5] >> (b & 31u)) & 1u)) m |= 1u << k;
    }
    mask[i] = m;
    count[i] = __popc(m);
}

__global__ __launch_bounds__(256) void k_sgent_cut_fill(const uint32_t* __restrict__ mask, const uint32_t* __restrict__ offset,
                                                        const uint64_t* __restrict__ total, uint32_t n_tipsets, uint32_t per_tipset,
                                                        const uint32_t* __restrict__ union_ids, uint32_t n_union, uint64_t cap,
                                                        uint32_t* __restrict__ ids_out, uint64_t* __restrict__ tipset_off /* n_tipsets + 1 */) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) tipset_off[n_tipsets] = *total;
    if (i >= n_tipsets * per_tipset) return;
    const uint32_t t = i / per_tipset, j = i - t * per_tipset;
    uint64_t o = offset[i];
    if (j == 0) tipset_off[t] = o;
    uint32_t m = mask[i];
    while (m) {
        const uint32_t k = __ffs(m) - 1u;
        m &= m - 1u;
        const uint32_t p = 32u * j + k;
        if (p < n_union && o < cap) ids_out[o] = union_ids[p];
        ++o;
    }
}

// ---- launchers (the context's stream; `w`: the view whose `touched` is row 0 of the recorder) ----
namespace {

SgenChain chain_of(uint32_t n_tipsets, uint32_t n_runs0, uint32_t n_specs, uint32_t words, const void* runs0_d) {
    SgenChain c{};
    c.n_tipsets = n_tipsets, c.n_runs0 = n_runs0, c.n_specs = n_specs, c.words = words;
    c.runs0 = static_cast<const StorageRun*>(runs0_d);
    return c;
}

}  // namespace

int launch_sgent_runs(ipcfp_ctx* ctx, const WitnessView& w, uint32_t words, const CidKey* children_d, uint32_t n_tipsets,
                      const void* runs0_d, uint32_t n_runs0, uint32_t n_specs, void* heads_d, void* runs_d, uint32_t undecided) {
    SgenChain c = chain_of(n_tipsets, n_runs0, n_specs, words, runs0_d);
    c.children = children_d;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
    hipLaunchKernelGGL(k_sgent_heads, dim3(div_up(n_tipsets, 256)), dim3(256), 0, ctx->stream, w, c, static_cast<SgenTipsetHead*>(heads_d));
    hipLaunchKernelGGL(k_sgent_run_init, dim3(div_up(uint64_t(n_tipsets) * n_runs0, 256)), dim3(256), 0, ctx->stream,
                       static_cast<const SgenTipsetHead*>(heads_d), c, static_cast<StorageRun*>(runs_d), undecided);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

// (the EVM state and the layout sniff ride along)
int launch_sgent_run_actors(ipcfp_ctx* ctx, const WitnessView& w, uint32_t words, const void* table_d, const uint64_t* actor_id_d,
                            const void* runs0_d, uint32_t n_runs0, uint32_t n_specs, uint32_t n_tipsets, void* runs_d, uint32_t undecided) {
    const SgenChain c = chain_of(n_tipsets, n_runs0, n_specs, words, runs0_d);
    const uint64_t n_runs = uint64_t(n_tipsets) * n_runs0;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
    sgen_run_actors(ctx, c, n_runs, w, table_d, actor_id_d, runs_d, undecided);
    hipLaunchKernelGGL(k_sgen_run_state<SgenChain>, dim3(div_up(n_runs, 256)), dim3(256), 0, ctx->stream, c, w, static_cast<StorageRun*>(runs_d));
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgent_specs(ipcfp_ctx* ctx, const WitnessView& w, uint32_t words, const void* table_d, const uint8_t* slot_d,
                       const uint32_t* run_of0_d, uint32_t n_specs, uint32_t n_runs0, uint32_t n_tipsets, const void* runs_d,
                       uint32_t* root_children_d, uint8_t* slot_out_d, uint8_t* value_d, uint8_t* cflags_d, uint8_t* status_d) {
    if (table_d && !root_children_d) return set_error(ctx, IPCFP_E_INVALID, "the tabled route needs its per-run words");
    ProfileScope prof(ctx, IPCFP_K_SGEN_SPECS);
    sgen_specs(ctx, chain_of(n_tipsets, n_runs0, n_specs, words, nullptr), uint64_t(n_tipsets) * n_runs0, uint64_t(n_tipsets) * n_specs, w,
               table_d, slot_d, run_of0_d, runs_d, root_children_d, slot_out_d, value_d, cflags_d, status_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgent_run_records(ipcfp_ctx* ctx, const void* runs_d, const void* runs0_d, uint32_t n_runs0, uint32_t n_specs, uint32_t n_tipsets,
                             const CidKey* children_d, const long long* epochs_d, const uint64_t* actor_id_d, void* out_d) {
    SgenChain c = chain_of(n_tipsets, n_runs0, n_specs, 0, runs0_d);
    c.children = children_d, c.epochs = epochs_d;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RECORDS);
    hipLaunchKernelGGL(k_sgen_run_records<SgenChain>, dim3(div_up(uint64_t(n_tipsets) * n_runs0, 256)), dim3(256), 0, ctx->stream, c,
                       static_cast<const StorageRun*>(runs_d), actor_id_d, static_cast<StorageRunRec*>(out_d));
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgent_union(ipcfp_ctx* ctx, const uint32_t* rows_d, uint32_t n_tipsets, uint32_t words, uint32_t* out_d) {
    if (words == 0) return IPCFP_OK;
    ProfileScope prof(ctx, IPCFP_K_SGEN_RECORDS);
    hipLaunchKernelGGL(k_sgent_union, dim3(div_up(words, 256)), dim3(256), 0, ctx->stream, rows_d, n_tipsets, words, out_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgent_cut_count(ipcfp_ctx* ctx, const uint32_t* rows_d, uint32_t n_tipsets, uint32_t words, uint32_t n_blocks,
                           const uint32_t* union_ids_d, uint32_t n_union, uint32_t* mask_d, uint32_t* count_d, uint32_t* offset_d,
                           uint64_t* total_d, uint64_t* scratch_d) {
    const uint32_t per_tipset = div_up(n_union, 32);
    const uint32_t n = n_tipsets * per_tipset;
    if (n == 0) return set_error(ctx, IPCFP_E_INVALID, "the cut of an empty union is the host's");
    ProfileScope prof(ctx, IPCFP_K_SGEN_RECORDS);
    hipLaunchKernelGGL(k_sgent_cut_masks, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, rows_d, n_tipsets, words, n_blocks, union_ids_d,
                       n_union, per_tipset, mask_d, count_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return launch_scan_u32(ctx, count_d, n, offset_d, total_d, scratch_d);
}

int launch_sgent_cut_fill(ipcfp_ctx* ctx, const uint32_t* mask_d, const uint32_t* offset_d, const uint64_t* total_d, uint32_t n_tipsets,
                          const uint32_t* union_ids_d, uint32_t n_union, uint64_t cap, uint32_t* ids_out_d, uint64_t* tipset_off_d) {
    const uint32_t per_tipset = div_up(n_union, 32);
    const uint32_t n = n_tipsets * per_tipset;
    if (n == 0) return set_error(ctx, IPCFP_E_INVALID, "the cut of an empty union is the host's");
    ProfileScope prof(ctx, IPCFP_K_SGEN_RECORDS);
    hipLaunchKernelGGL(k_sgent_cut_fill, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, mask_d, offset_d, total_d, n_tipsets, per_tipset,
                       union_ids_d, n_union, cap, ids_out_d, tipset_off_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
