// csrc/kernels/event_gen_tipsets.inc — `generate_event_proof` (src/proofs/events/generator.rs:75-178) for a CHAIN of tipset
// pairs in one pass (ipcfp_generate_event_claims_tipsets, host/generate.cpp): what the single call does pair by pair with
// everything it keeps once kept per tipset.
//
// Included at the end of tipset_prepare_general.hip, whose device code (StagedOpener, and through tipset_prologue_body.h
// prologue_headers / prologue_roots) the chain prologue calls as it is.  The kernels above keep their text.
//
//   k_gent_prologue     one single-wavefront workgroup per (tipset, slot): slots 0 / 1 the child and first parent header,
//                       slot 2 + b parent block b → TxMeta → its two message-AMT roots (kTxMetaNone: build_execution_order,
//                       utils.rs:32-46).  Stage-1 errors go to the tipset's OWN error word with the single call's sequence
//                       numbers; the roots' `seq` is rewritten to the root's number in the whole chain, which is what the
//                       enumerator's one error word orders
//   k_gent_facts        per tipset: what the host needs of the context (status, receipts root, heights, stage-1 word); the
//                       roots of a tipset whose child header failed are marked `skip`
//   k_gent_skip_roots   roots [lo, hi) → skip (the tipset the enumerator's error word named)
//   k_gent_keys         leaf → message CID key and its tipset (seq → tipset table)
//   k_gent_insert_flags k_exec_insert_flags over the concatenated raw sequence with the key (tipset, CID): ONE table for
//                       the chain, the tipset mixed into the hash and compared before the CID
//   k_gent_exec_ranges  exec_off[t] = the flags' exclusive scan at tipset t's first raw position (exec_off[T] = the total)
//   k_gent_gather       message CID of match k of tipset t = list[exec_off[t] + exec_index]; an index outside the tipset's
//                       execution order raises oor[t] ("Missing message at index", generator.rs:158-160)
//   k_gent_mark_base    k_mark_cids with one missing flag per tipset
//   k_gent_patch_claims claim k of tipset t: tipset index and the tipset's two epochs (plain stores into the records the
//                       unchanged fill kernel wrote)
// All hand-offs are kernel boundaries on the context's stream.

namespace ipcfp {

// one tipset of the chain as the prologue sees it (host-built)
struct GentTipset {
    uint32_t slot_first;  // its first workgroup of k_gent_prologue (2 + n_parents of them)
    uint32_t root_first;  // its first root in the chain's root list (2 * n_parents of them)
    uint32_t n_parents;
    uint32_t dead;        // 1: skipped altogether (a pass that records only the sound tipsets)
};

// what the host reads back per tipset
struct GentFacts {
    CidKey receipts_root;
    long long child_height, parent0_height;
    unsigned long long err;  // stage 1 of the execution order: packed first error with the SINGLE call's sequence numbers
    uint32_t child_status, pad;
};

// the largest t with off[t] <= k, for off[0] == 0 ascending (empty ranges allowed): the range [off[t], off[t + 1]) holds k
template <class Off>
__device__ __forceinline__ uint32_t gent_range_of(const Off* __restrict__ off, uint32_t n_ranges, uint64_t k) {
    uint32_t lo = 0, hi = n_ranges;  // invariant: off[lo] <= k < off[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (uint64_t(off[mid]) <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(64) void k_gent_prologue(WitnessView w, TipsetCtxDev* __restrict__ ctxs, const GentTipset* __restrict__ tips,
                                                      uint32_t n_tipsets, uint32_t n_slots, AmtRootSpec* __restrict__ roots,
                                                      unsigned long long* __restrict__ err) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kHeaderLds];
    if (blockIdx.x >= n_slots) return;
    uint32_t lo = 0, hi = n_tipsets;  // tips[lo].slot_first <= blockIdx.x < tips[hi].slot_first (uniform across the wavefront)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (tips[mid].slot_first <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    const GentTipset tp = tips[lo];
    const uint32_t slot = blockIdx.x - tp.slot_first;
    if (slot >= 2u + tp.n_parents) return;
    AmtRootSpec* const my = roots + tp.root_first;
    const bool lead = threadIdx.x == 0;
    if (tp.dead) {
        if (slot >= 2u && lead) {
            AmtRootSpec s{};
            s.skip = 1;
            s.seq = tp.root_first + 2u * (slot - 2u);
            my[2u * (slot - 2u)] = s;
            s.seq += 1u;
            my[2u * (slot - 2u) + 1u] = s;
        }
        return;
    }
    TipsetCtxDev& c = ctxs[lo];
    const TipsetKeysCtx keys{c};
    StagedOpener opener{lds, Rd{}};
    if (slot < 2u) {
        prologue_headers(w, keys, c, slot == 0u, opener, nullptr);
        return;
    }
    const uint32_t b = slot - 2u;
    prologue_roots(w, keys, c, my, err + lo, b, opener, kTxMetaNone);
    if (lead) {  // (the lead lane wrote both specs: the chain's root numbers over the tipset's own)
        my[2u * b].seq = tp.root_first + 2u * b;
        my[2u * b + 1u].seq = tp.root_first + 2u * b + 1u;
    }
}

__global__ __launch_bounds__(256) void k_gent_facts(const TipsetCtxDev* __restrict__ ctxs, const GentTipset* __restrict__ tips,
                                                    uint32_t n_tipsets, const unsigned long long* __restrict__ err,
                                                    AmtRootSpec* __restrict__ roots, GentFacts* __restrict__ facts) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tipsets) return;
    const GentTipset tp = tips[t];
    GentFacts f{};
    f.err = kNoEnumError;
    f.child_status = IPCFP_ST_ERR;
    if (!tp.dead) {
        const TipsetCtxDev& c = ctxs[t];
        f.child_status = c.child_status;
        f.child_height = c.child_height;
        f.parent0_height = c.parent0_height;
        f.err = err[t];
        if (c.child_status == IPCFP_ST_TRUE) {
            f.receipts_root = c.receipts_root;
        } else {  // generator.rs:89-95 fails first: nothing of this tipset is walked
            for (uint32_t r = 0; r < 2u * tp.n_parents; ++r) roots[tp.root_first + r].skip = 1u;
        }
    }
    facts[t] = f;
}

__global__ __launch_bounds__(256) void k_gent_skip_roots(AmtRootSpec* __restrict__ roots, uint32_t lo, uint32_t hi) {
    const uint32_t r = lo + blockIdx.x * blockDim.x + threadIdx.x;
    if (r < hi) roots[r].skip = 1u;
}

__global__ __launch_bounds__(256) void k_gent_keys(WitnessView w, const LeafRef* __restrict__ leaves, uint32_t n,
                                                   const uint32_t* __restrict__ seq_tipset, uint32_t n_roots, CidKey* __restrict__ keys,
                                                   uint32_t* __restrict__ tip) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const LeafRef l = leaves[i];
    Rd r;
    r.init(w.arena + w.off[l.block] + l.off, l.len);
    CidKey k;
    r.read_link_key(k);
    keys[i] = k;
    tip[i] = seq_tipset[l.seq < n_roots ? l.seq : n_roots - 1u];  // (seq comes from the specs the prologue wrote)
}

constexpr unsigned long long kGentEmptySlot = ~0ULL;  // (== kEmptySlot64, verify_dev.h)

// the 64-bit mix of (tipset, CID): high half selects the slot, low half is the fingerprint
__device__ __forceinline__ uint64_t gent_hash64(const CidKey& k, uint32_t tipset) {
    uint64_t x = cid_hash64(k) ^ ((uint64_t(tipset) + 1ull) * 0xD6E8FEB86659FD93ULL);
    x ^= x >> 32;
    return x * 0x9E3779B97F4A7C15ULL;
}

// `first` zeroed by the caller; slots 0xff.  A slot is {fingerprint, GLOBAL raw position}; see k_exec_insert_flags for why the
// one-probe flags end right whatever order the wavefronts run in.
__global__ __launch_bounds__(256) void k_gent_insert_flags(const CidKey* __restrict__ keys, const uint32_t* __restrict__ tip, uint32_t n,
                                                           unsigned long long* __restrict__ slots, uint32_t mask,
                                                           uint32_t* __restrict__ first) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const CidKey key = keys[i];
    const uint32_t my_tip = tip[i];
    const uint64_t h = gent_hash64(key, my_tip);
    const unsigned long long mine = ((unsigned long long)uint32_t(h) << 32) | i;
    uint32_t s = uint32_t(h >> 32) & mask;
    for (;;) {
        const unsigned long long cur = atomicCAS(&slots[s], kGentEmptySlot, mine);
        if (cur == kGentEmptySlot) {
            atomicAdd(&first[i], 1u);
            return;
        }
        const uint32_t at = uint32_t(cur);
        if (uint32_t(cur >> 32) == uint32_t(h) && at < n && tip[at] == my_tip && cid_equal(keys[at], key)) {
            const unsigned long long old = atomicMin(&slots[s], mine);  // (only positions of THIS (tipset, CID) lower this slot)
            if (old > mine) {
                atomicAdd(&first[i], 1u);
                atomicAdd(&first[uint32_t(old)], 0xffffffffu);
            }
            return;
        }
        s = (s + 1) & mask;
    }
}

// first_by_root: n_roots + 1 entries (launch_tipset_bounds over the roots' numbers); n == 0: every offset is 0
__global__ __launch_bounds__(256) void k_gent_exec_ranges(const GentTipset* __restrict__ tips, uint32_t n_tipsets,
                                                          const uint32_t* __restrict__ first_by_root, const uint32_t* __restrict__ pos,
                                                          const uint64_t* __restrict__ total, uint32_t n, uint32_t* __restrict__ exec_off) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t > n_tipsets) return;
    if (n == 0) {
        exec_off[t] = 0;
        return;
    }
    const uint32_t all = uint32_t(*total);
    if (t == n_tipsets) {
        exec_off[t] = all;
        return;
    }
    const uint32_t r = first_by_root[tips[t].root_first];
    exec_off[t] = r < n ? pos[r] : all;
}

__global__ __launch_bounds__(256) void k_gent_gather(const ipcfp_event_match_t* __restrict__ matches, uint32_t n,
                                                     const uint64_t* __restrict__ match_off, uint32_t n_tipsets,
                                                     const uint32_t* __restrict__ exec_off, const CidKey* __restrict__ list,
                                                     CidKey* __restrict__ msg, uint32_t* __restrict__ oor) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t t = gent_range_of(match_off, n_tipsets, k);
    const uint64_t e = matches[k].exec_index;
    const uint32_t lo = exec_off[t], len = exec_off[t + 1] - lo;
    CidKey out{};
    if (e >= len) atomicOr(&oor[t], 1u);
    else out = list[lo + uint32_t(e)];
    msg[k] = out;
}

__global__ __launch_bounds__(64) void k_gent_mark_base(WitnessView w, const CidKey* __restrict__ keys, const uint32_t* __restrict__ key_tip,
                                                       uint32_t n, uint32_t* __restrict__ missing) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (witness_find(w, keys[i]) == kNoBlock) atomicOr(&missing[key_tip[i]], 1u);
}

__global__ __launch_bounds__(256) void k_gent_patch_claims(EventClaimPacked* __restrict__ claims, uint32_t n,
                                                           const uint64_t* __restrict__ claim_off, uint32_t n_tipsets,
                                                           const long long* __restrict__ parent_epoch,
                                                           const long long* __restrict__ child_epoch) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint32_t t = gent_range_of(claim_off, n_tipsets, k);
    claims[k].parent_epoch = parent_epoch[t];
    claims[k].child_epoch = child_epoch[t];
    if (claims[k].context != 0xffffffffu) claims[k].context = t;  // (a match that cannot be lowered keeps the fill's mark)
}

static_assert(sizeof(GentTipset) == 16 && sizeof(GentFacts) == 72, "host/generate.cpp mirrors these records");

int launch_gent_prologue(ipcfp_ctx* ctx, const WitnessView& w, void* ctxs_d, const void* tips_d, uint32_t n_tipsets, uint32_t n_slots,
                         AmtRootSpec* roots_d, unsigned long long* err_d, void* facts_d) {
    {
        ProfileScope prof(ctx, IPCFP_K_GEN_TIPSETS);
        hipLaunchKernelGGL(k_gent_prologue, dim3(n_slots), dim3(64), 0, ctx->stream, w, static_cast<TipsetCtxDev*>(ctxs_d),
                           static_cast<const GentTipset*>(tips_d), n_tipsets, n_slots, roots_d, err_d);
        hipLaunchKernelGGL(k_gent_facts, dim3(div_up(n_tipsets, 256)), dim3(256), 0, ctx->stream, static_cast<const TipsetCtxDev*>(ctxs_d),
                           static_cast<const GentTipset*>(tips_d), n_tipsets, err_d, roots_d, static_cast<GentFacts*>(facts_d));
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_gent_skip_roots(ipcfp_ctx* ctx, AmtRootSpec* roots_d, uint32_t lo, uint32_t hi) {
    if (hi <= lo) return IPCFP_OK;
    {
        ProfileScope prof(ctx, IPCFP_K_GEN_TIPSETS);
        hipLaunchKernelGGL(k_gent_skip_roots, dim3(div_up(hi - lo, 256)), dim3(256), 0, ctx->stream, roots_d, lo, hi);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_gent_exec_order(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* leaves_d, uint32_t n, const uint32_t* seq_tipset_d,
                           uint32_t n_roots, CidKey* keys_d, uint32_t* tip_d, unsigned long long* slots_d, uint32_t mask,
                           uint32_t* first_d) {
    if (n == 0) return IPCFP_OK;
    {
        ProfileScope prof(ctx, IPCFP_K_GEN_TIPSETS);
        hipLaunchKernelGGL(k_gent_keys, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w, leaves_d, n, seq_tipset_d, n_roots, keys_d,
                           tip_d);
        hipLaunchKernelGGL(k_gent_insert_flags, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, keys_d, tip_d, n, slots_d, mask,
                           first_d);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_gent_exec_ranges(ipcfp_ctx* ctx, const void* tips_d, uint32_t n_tipsets, const uint32_t* first_by_root_d, const uint32_t* pos_d,
                            const uint64_t* total_d, uint32_t n, uint32_t* exec_off_d) {
    {
        ProfileScope prof(ctx, IPCFP_K_GEN_TIPSETS);
        hipLaunchKernelGGL(k_gent_exec_ranges, dim3(div_up(n_tipsets + 1u, 256)), dim3(256), 0, ctx->stream,
                           static_cast<const GentTipset*>(tips_d), n_tipsets, first_by_root_d, pos_d, total_d, n, exec_off_d);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_gent_gather(ipcfp_ctx* ctx, const void* matches_d, uint32_t n, const uint64_t* match_off_d, uint32_t n_tipsets,
                       const uint32_t* exec_off_d, const CidKey* list_d, CidKey* msg_d, uint32_t* oor_d) {
    if (n == 0) return IPCFP_OK;
    {
        ProfileScope prof(ctx, IPCFP_K_GEN_TIPSETS);
        hipLaunchKernelGGL(k_gent_gather, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream,
                           static_cast<const ipcfp_event_match_t*>(matches_d), n, match_off_d, n_tipsets, exec_off_d, list_d, msg_d, oor_d);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_gent_mark_base(ipcfp_ctx* ctx, const WitnessView& w, const CidKey* keys_d, const uint32_t* key_tip_d, uint32_t n,
                          uint32_t* missing_d) {
    if (n == 0) return IPCFP_OK;
    {
        ProfileScope prof(ctx, IPCFP_K_GEN_TIPSETS);
        hipLaunchKernelGGL(k_gent_mark_base, dim3(div_up(n, 64)), dim3(64), 0, ctx->stream, w, keys_d, key_tip_d, n, missing_d);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_gent_patch_claims(ipcfp_ctx* ctx, void* claims_d, uint32_t n, const uint64_t* claim_off_d, uint32_t n_tipsets,
                             const long long* parent_epoch_d, const long long* child_epoch_d) {
    if (n == 0) return IPCFP_OK;
    {
        ProfileScope prof(ctx, IPCFP_K_GEN_TIPSETS);
        hipLaunchKernelGGL(k_gent_patch_claims, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, static_cast<EventClaimPacked*>(claims_d), n,
                           claim_off_d, n_tipsets, parent_epoch_d, child_epoch_d);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
