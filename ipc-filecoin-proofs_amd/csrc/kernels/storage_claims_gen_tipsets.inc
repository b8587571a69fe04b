// csrc/kernels/storage_claims_gen_tipsets.inc — the storage generator for a CHAIN of child headers
// (ipcfp_generate_storage_claims_tipsets*, host/generate.cpp): ONE list of n_specs (actor_id, slot) specs posed at each of T
// children, answered as T single calls laid end to end.
//
// Included at the end of storage_claims_gen.hip, whose device helpers (chain_verdict, zero_key, mark_block, store_value,
// actor_state_of, root_step_child) it uses as they are.  The kernels above keep their text; the bodies below are theirs with
// the index (tipset, run) or (tipset, spec) and the recorder's row chosen per lane.
//
// The runs are those of the spec list (R0 of them, discovered once by the single call's kernels): the chain has T·R0 runs,
// run (t, r) = t·R0 + r, and claim (t, s) = t·n_specs + s.  A run never crosses a tipset.
//
//   k_sgent_heads            one lane per tipset: child header → parent_state_root → StateRoot.actors, into a 96-byte record
//   k_sgent_run_init         one lane per (t, r): the run's StorageRun from its tipset's record — no header is decoded twice
//   k_sgent_run_actors_*     the actor get over the node table, then the lane walker            (k_sgen_run_actors_*)
//   k_sgent_run_state        EVM state and layout sniff                                         (k_sgen_run_state)
//   k_sgent_run_children     32 lanes per (t, r)                                                (k_sgen_run_children)
//   k_sgent_specs_table      one lane per (t, s): slot read at s, value / cflags / status and the slot column written at
//   k_sgent_specs_lane       t·n_specs + s                                                      (k_sgen_specs_*)
//   k_sgent_run_records      the 192-byte records with children[t], epochs[t] and the shifted first_claim
//
// The recorder is T bitmap rows of `words` = ceil(blocks / 32) words: a lane of tipset t works on a copy of the WitnessView
// whose `touched` points at row t, so that what it fetches is recorded for its own tipset only.  The cut:
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

struct SgenChainShape {
    uint32_t n_tipsets, n_runs0, n_specs, words;
};

namespace {

__device__ __forceinline__ WitnessView row_view(const WitnessView& w, uint32_t words, uint32_t t) {
    WitnessView v = w;
    v.touched = w.touched + size_t(t) * words;
    return v;
}

// the actor of run r of the spec list, or false when its record does not point into the list
__device__ __forceinline__ bool run_actor(const StorageRun* __restrict__ runs0, const uint64_t* __restrict__ actor_id, uint32_t r,
                                          uint32_t n_specs, uint64_t& actor) {
    const uint32_t first = runs0[r].first_claim;
    if (first >= n_specs) return false;
    actor = actor_id[first];
    return true;
}

}  // namespace

__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgent_heads(WitnessView w, uint32_t words, const CidKey* __restrict__ children,
                                                                       uint32_t n_tipsets, SgenTipsetHead* __restrict__ heads) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tipsets) return;
    const WitnessView v = row_view(w, words, t);
    SgenTipsetHead h;
    zero_key(h.parent_state_root), zero_key(h.actors);
    h.sr_status = IPCFP_ST_ERR;
    h.pad[0] = h.pad[1] = 0;
    HeaderLite hdr;
    uint32_t hb;
    h.hdr_status = load_header(v, children[t], hdr, hb);
    if (h.hdr_status == IPCFP_ST_TRUE) {
        h.parent_state_root = hdr.parent_state_root;
        const uint32_t b = witness_find(v, hdr.parent_state_root);
        if (b == kNoBlock) {
            h.sr_status = IPCFP_ST_ERR_MISSING_BLOCK;
        } else {
            Rd r = open_block(v, b);
            CidKey info;
            r.expect_array(3);
            if (r.read_uint() > 5) r.fail();
            r.read_link_key(h.actors);
            r.read_link_key(info);
            r.finish();
            h.sr_status = r.ok() ? uint32_t(IPCFP_ST_TRUE) : uint32_t(IPCFP_ST_ERR_DECODE);
        }
    }
    heads[t] = h;
}

__global__ __launch_bounds__(256) void k_sgent_run_init(const SgenTipsetHead* __restrict__ heads, const StorageRun* __restrict__ runs0,
                                                        SgenChainShape c, StorageRun* __restrict__ runs, uint32_t undecided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_tipsets * c.n_runs0) return;
    const uint32_t t = i / c.n_runs0, r = i - t * c.n_runs0;
    const SgenTipsetHead h = heads[t];
    StorageRun run;
    run.first_claim = t * c.n_specs + runs0[r].first_claim;
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

__global__ __launch_bounds__(256) void k_sgent_run_actors_table(WitnessView w, const HamtNodeRec* __restrict__ table,
                                                                const uint64_t* __restrict__ actor_id,
                                                                const StorageRun* __restrict__ runs0, SgenChainShape c,
                                                                StorageRun* __restrict__ runs, uint32_t undecided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_tipsets * c.n_runs0) return;
    if (runs[i].actor_status != undecided) return;
    const uint32_t t = i / c.n_runs0, r = i - t * c.n_runs0;
    const WitnessView v = row_view(w, c.words, t);
    uint64_t actor;
    if (!run_actor(runs0, actor_id, r, c.n_specs, actor)) return;  // (the lane kernel settles it)
    uint8_t key[12];
    const uint32_t kl = id_address_bytes(actor, key);
    ValueLoc loc;
    uint32_t st = table_hamt_get(v, table, runs[i].actors, 5, HK_ACTOR_STATE, key, kl, loc);
    if (st == kTablePunt) return;
    CidKey actor_state;
    zero_key(actor_state);
    if (st == IPCFP_ST_NOT_FOUND) st = IPCFP_ST_ERR_ACTOR_NOT_FOUND;
    if (st == IPCFP_ST_TRUE) st = actor_state_of(v, loc, actor_state);
    runs[i].actor_status = st;
    runs[i].actor_state = actor_state;
}

__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgent_run_actors_lane(WitnessView w, const uint64_t* __restrict__ actor_id,
                                                                                 const StorageRun* __restrict__ runs0, SgenChainShape c,
                                                                                 StorageRun* __restrict__ runs, uint32_t undecided) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_tipsets * c.n_runs0) return;
    if (runs[i].actor_status != undecided) return;
    const uint32_t t = i / c.n_runs0, r = i - t * c.n_runs0;
    const WitnessView v = row_view(w, c.words, t);
    CidKey actor_state;
    zero_key(actor_state);
    uint32_t st = IPCFP_ST_ERR;
    uint64_t actor;
    if (run_actor(runs0, actor_id, r, c.n_specs, actor)) {
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

__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgent_run_state(WitnessView w, SgenChainShape c, StorageRun* __restrict__ runs) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_tipsets * c.n_runs0) return;
    const WitnessView v = row_view(w, c.words, i / c.n_runs0);
    StorageRun run = runs[i];
    if (run.hdr_status == IPCFP_ST_TRUE && run.sr_status == IPCFP_ST_TRUE && run.actor_status == IPCFP_ST_TRUE) {
        const uint32_t eb = witness_find(v, run.actor_state);
        run.evm_status = eb == kNoBlock ? uint32_t(IPCFP_ST_ERR_MISSING_BLOCK) : parse_evm_state(v, eb, run.contract_state);
        if (run.evm_status == IPCFP_ST_TRUE) run.root_kind = sniff_storage_root(v, run.contract_state, run.hamt_root, run.hamt_bw);
    }
    run.chain_status = chain_verdict(run);
    runs[i] = run;
}

// (the probes stay on a non-recording view; only the root is marked, in the run's own row)
__global__ __launch_bounds__(256) void k_sgent_run_children(WitnessView w, const HamtNodeRec* __restrict__ table,
                                                            const StorageRun* __restrict__ runs, SgenChainShape c,
                                                            uint32_t* __restrict__ root_block, uint32_t* __restrict__ root_child) {
    const uint64_t lane = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t i64 = lane >> 5;
    const uint32_t p = uint32_t(lane) & 31u;
    if (i64 >= uint64_t(c.n_tipsets) * c.n_runs0) return;
    const uint32_t i = uint32_t(i64);
    WitnessView quiet = w;
    quiet.touched = nullptr;
    uint32_t rb = kNoBlock, child = kNoBlock;
    if (runs[i].chain_status == IPCFP_ST_TRUE && runs[i].root_kind == 3) {
        rb = witness_find(quiet, runs[i].hamt_root);
        if (rb != kNoBlock) {
            if (p == 0) mark_block(row_view(w, c.words, i / c.n_runs0), rb);
            const HamtNodeRec* rec = table + rb;
            const uint32_t head = *reinterpret_cast<const uint32_t*>(rec);
            if ((head & 0xffu) != 1u) {
                rb = kNoBlock;
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

// the slot of claim (t, s) into the handle's column: two 16-byte stores
__device__ __forceinline__ void store_slot(uint8_t* __restrict__ slot_out, uint32_t i, const uint64_t kw[4]) {
    Out16* o = reinterpret_cast<Out16*>(slot_out + 32ull * i);
    o[0] = Out16{kw[0], kw[1]};
    o[1] = Out16{kw[2], kw[3]};
}

__global__ __launch_bounds__(256, 7) void k_sgent_specs_table(WitnessView w, const HamtNodeRec* __restrict__ table,
                                                              const uint8_t* __restrict__ slot, SgenChainShape c,
                                                              const uint32_t* __restrict__ run_of0, const StorageRun* __restrict__ runs,
                                                              const uint32_t* __restrict__ root_block,
                                                              const uint32_t* __restrict__ root_child, uint8_t* __restrict__ slot_out,
                                                              uint8_t* __restrict__ value, uint8_t* __restrict__ cflags,
                                                              uint8_t* __restrict__ status) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_tipsets * c.n_specs) return;
    __shared__ ValueStage vstage;
    const uint32_t t = i / c.n_specs, s = i - t * c.n_specs;
    const uint8_t* slot_p = slot + 32ull * s;
    uint64_t kw[4];
    {
        const Raw16 a = raw_ld128(slot_p), b = raw_ld128(slot_p + 16);
        kw[0] = a.lo, kw[1] = a.hi, kw[2] = b.lo, kw[3] = b.hi;
    }
    store_slot(slot_out, i, kw);
    uint64_t padded[4] = {0, 0, 0, 0};
    uint32_t st = kStPending;
    const uint32_t r0 = run_of0[s];
    if (r0 >= c.n_runs0) {  // (no launcher leaves a spec without its run)
        store_value(value, i, padded);
        cflags[i] = 0;
        status[i] = uint8_t(IPCFP_ST_ERR);
        return;
    }
    const uint32_t ri = t * c.n_runs0 + r0;
    const StorageRun& run = runs[ri];
    const WitnessView v = row_view(w, c.words, t);
    do {
        const uint32_t chain = run.chain_status;
        if (chain != IPCFP_ST_TRUE) { st = chain; break; }
        if (run.root_kind == 4) { st = IPCFP_ST_ERR_MISSING_BLOCK; break; }
        if (run.root_kind != 3) break;
        ValueLoc loc;
        const uint32_t rb = root_block[ri];
        const uint32_t* kids = root_child + size_t(ri) * 32u;
        const uint32_t stepped = root_step_child(table, rb, run.hamt_bw, kw, kids);
        if (stepped != kNoBlock && stepped < w.n) mark_block(v, stepped);
        const uint32_t hs = table_hamt_get(v, table, run.hamt_root, run.hamt_bw, HK_VEC_U8, slot_p, 32, loc, rb, kids, kw);
        if (hs == kTablePunt) break;
        if (hs == IPCFP_ST_NOT_FOUND) { st = IPCFP_ST_TRUE; break; }
        if (hs != IPCFP_ST_TRUE) { st = hs; break; }
        const uint8_t* vp = w.arena + w.off[loc.block] + loc.off;
        uint32_t L[8];
        {
            Raw16 tw[kValueStageWords / 2];
#pragma unroll
            for (uint32_t j = 0; j < kValueStageWords / 2; ++j) tw[j] = raw_ld128(vp + 16u * j);
#pragma unroll
            for (uint32_t j = 0; j < kValueStageWords / 2; ++j) {
                vstage.w[2 * j][threadIdx.x] = tw[j].lo;
                vstage.w[2 * j + 1][threadIdx.x] = tw[j].hi;
            }
            vstage.w[kValueStageWords][threadIdx.x] = 0;
        }
        if (left_pad_32_staged(vstage, threadIdx.x, loc.len, L) || left_pad_32_raw(vp, loc.len, L)) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
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
    store_value(value, i, padded);
    cflags[i] = st == IPCFP_ST_TRUE ? uint8_t(IPCFP_SCOL_FLAG_MASK) : uint8_t(0);
}

// pending_only: behind the table kernel, which has written the slot column; else every claim, and the slot column with it
__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_sgent_specs_lane(WitnessView w, const uint8_t* __restrict__ slot, SgenChainShape c,
                                                                            const uint32_t* __restrict__ run_of0,
                                                                            const StorageRun* __restrict__ runs, uint8_t* __restrict__ slot_out,
                                                                            uint8_t* __restrict__ value, uint8_t* __restrict__ cflags,
                                                                            uint8_t* __restrict__ status, int pending_only) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_tipsets * c.n_specs) return;
    if (pending_only && status[i] != kStPending) return;
    const uint32_t t = i / c.n_specs, s = i - t * c.n_specs;
    const uint8_t* slot_p = slot + 32ull * s;
    if (!pending_only) {
        const Raw16 a = raw_ld128(slot_p), b = raw_ld128(slot_p + 16);
        const uint64_t kw[4] = {a.lo, a.hi, b.lo, b.hi};
        store_slot(slot_out, i, kw);
    }
    uint8_t padded[32];
    for (int k = 0; k < 32; ++k) padded[k] = 0;
    uint32_t st = IPCFP_ST_ERR;
    const uint32_t r0 = run_of0[s];
    if (r0 < c.n_runs0) {
        const StorageRun& run = runs[t * c.n_runs0 + r0];
        st = run.chain_status;
        if (st == IPCFP_ST_TRUE) st = read_storage_slot_padded(row_view(w, c.words, t), run.contract_state, slot_p, padded);
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
    store_value(value, i, out);
    cflags[i] = st == IPCFP_ST_TRUE ? uint8_t(IPCFP_SCOL_FLAG_MASK) : uint8_t(0);
    status[i] = uint8_t(st);
}

__global__ __launch_bounds__(256) void k_sgent_run_records(const StorageRun* __restrict__ runs, const StorageRun* __restrict__ runs0,
                                                           SgenChainShape c, const CidKey* __restrict__ children,
                                                           const long long* __restrict__ epochs, const uint64_t* __restrict__ actor_id,
                                                           StorageRunRec* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= c.n_tipsets * c.n_runs0) return;
    const uint32_t t = i / c.n_runs0, r = i - t * c.n_runs0;
    const StorageRun& run = runs[i];
    const bool ok = run.chain_status == IPCFP_ST_TRUE;
    // the run's stretch of the spec list: [first, next run's first or the end), clipped to the list
    uint32_t first = runs0[r].first_claim, last = r + 1 < c.n_runs0 ? runs0[r + 1].first_claim : c.n_specs;
    if (last > c.n_specs) last = c.n_specs;
    if (first > last) first = last;
    StorageRunRec rec;
    rec.child_epoch = epochs[t];
    rec.actor_id = first < c.n_specs ? actor_id[first] : 0;
    rec.child = children[t];
    zero_key(rec.state_root), zero_key(rec.actor_state), zero_key(rec.storage_root);
    if (ok) {
        rec.state_root = run.parent_state_root;
        rec.actor_state = run.actor_state;
        rec.storage_root = run.contract_state;
    }
    rec.first_claim = t * c.n_specs + first;
    rec.n_claims = last - first;
    rec.flags = ok ? uint32_t(IPCFP_SRUN_FLAG_MASK) : 0u;
    rec.reserved = 0;
    out[i] = rec;
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
int launch_sgent_runs(ipcfp_ctx* ctx, const WitnessView& w, uint32_t words, const CidKey* children_d, uint32_t n_tipsets,
                      const void* runs0_d, uint32_t n_runs0, uint32_t n_specs, void* heads_d, void* runs_d, uint32_t undecided) {
    const SgenChainShape c = SgenChainShape{n_tipsets, n_runs0, n_specs, words};
    ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
    hipLaunchKernelGGL(k_sgent_heads, dim3(div_up(n_tipsets, 256)), dim3(256), 0, ctx->stream, w, words, children_d, n_tipsets,
                       static_cast<SgenTipsetHead*>(heads_d));
    hipLaunchKernelGGL(k_sgent_run_init, dim3(div_up(uint64_t(n_tipsets) * n_runs0, 256)), dim3(256), 0, ctx->stream,
                       static_cast<const SgenTipsetHead*>(heads_d), static_cast<const StorageRun*>(runs0_d), c, static_cast<StorageRun*>(runs_d),
                       undecided);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgent_run_actors(ipcfp_ctx* ctx, const WitnessView& w, uint32_t words, const void* table_d, const uint64_t* actor_id_d,
                            const void* runs0_d, uint32_t n_runs0, uint32_t n_specs, uint32_t n_tipsets, void* runs_d, uint32_t undecided) {
    const SgenChainShape c = SgenChainShape{n_tipsets, n_runs0, n_specs, words};
    ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
    const dim3 g(div_up(uint64_t(n_tipsets) * n_runs0, 256)), blk(256);
    if (table_d)
        hipLaunchKernelGGL(k_sgent_run_actors_table, g, blk, 0, ctx->stream, w, static_cast<const HamtNodeRec*>(table_d), actor_id_d,
                           static_cast<const StorageRun*>(runs0_d), c, static_cast<StorageRun*>(runs_d), undecided);
    hipLaunchKernelGGL(k_sgent_run_actors_lane, g, blk, 0, ctx->stream, w, actor_id_d, static_cast<const StorageRun*>(runs0_d), c,
                       static_cast<StorageRun*>(runs_d), undecided);
    hipLaunchKernelGGL(k_sgent_run_state, g, blk, 0, ctx->stream, w, c, static_cast<StorageRun*>(runs_d));
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgent_specs(ipcfp_ctx* ctx, const WitnessView& w, uint32_t words, const void* table_d, const uint8_t* slot_d,
                       const uint32_t* run_of0_d, uint32_t n_specs, uint32_t n_runs0, uint32_t n_tipsets, const void* runs_d,
                       uint32_t* root_children_d, uint8_t* slot_out_d, uint8_t* value_d, uint8_t* cflags_d, uint8_t* status_d) {
    if (table_d && !root_children_d) return set_error(ctx, IPCFP_E_INVALID, "the tabled route needs its per-run words");
    const SgenChainShape c = SgenChainShape{n_tipsets, n_runs0, n_specs, words};
    const uint64_t n_runs = uint64_t(n_tipsets) * n_runs0;
    ProfileScope prof(ctx, IPCFP_K_SGEN_SPECS);
    const dim3 g(div_up(uint64_t(n_tipsets) * n_specs, 256)), blk(256);
    if (table_d) {
        uint32_t* root_block = root_children_d;
        uint32_t* root_child = root_children_d + n_runs;
        hipLaunchKernelGGL(k_sgent_run_children, dim3(div_up(n_runs * 32u, 256)), blk, 0, ctx->stream, w,
                           static_cast<const HamtNodeRec*>(table_d), static_cast<const StorageRun*>(runs_d), c, root_block, root_child);
        hipLaunchKernelGGL(k_sgent_specs_table, g, blk, 0, ctx->stream, w, static_cast<const HamtNodeRec*>(table_d), slot_d, c, run_of0_d,
                           static_cast<const StorageRun*>(runs_d), root_block, root_child, slot_out_d, value_d, cflags_d, status_d);
    }
    hipLaunchKernelGGL(k_sgent_specs_lane, g, blk, 0, ctx->stream, w, slot_d, c, run_of0_d, static_cast<const StorageRun*>(runs_d), slot_out_d,
                       value_d, cflags_d, status_d, table_d ? 1 : 0);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_sgent_run_records(ipcfp_ctx* ctx, const void* runs_d, const void* runs0_d, uint32_t n_runs0, uint32_t n_specs, uint32_t n_tipsets,
                             const CidKey* children_d, const long long* epochs_d, const uint64_t* actor_id_d, void* out_d) {
    const SgenChainShape c = SgenChainShape{n_tipsets, n_runs0, n_specs, 0};
    ProfileScope prof(ctx, IPCFP_K_SGEN_RECORDS);
    hipLaunchKernelGGL(k_sgent_run_records, dim3(div_up(uint64_t(n_tipsets) * n_runs0, 256)), dim3(256), 0, ctx->stream,
                       static_cast<const StorageRun*>(runs_d), static_cast<const StorageRun*>(runs0_d), c, children_d, epochs_d, actor_id_d,
                       static_cast<StorageRunRec*>(out_d));
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
