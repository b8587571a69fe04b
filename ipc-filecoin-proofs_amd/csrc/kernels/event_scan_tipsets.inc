// csrc/kernels/event_scan_tipsets.inc — K6 for a CHAIN of tipsets and a set of specs (ipcfp_scan_events_tipsets,
// host/scan_events_tipsets.cpp): the two passes of event_scan_multi.inc over the concatenated receipt leaves of T receipts
// trees, with everything that the single-tipset kernels keep once kept per tipset.
//
// Included at the end of event_scan.hip, behind event_scan_multi.inc whose device helpers (rec_group, log_group,
// group_count, emit_members, the LDS histogram) it uses as they are.  The kernels above keep their text.
//
// The leaves come out of ONE amt_enumerate over T roots with seq = tipset number, in root order: `seq` is non-decreasing
// along the leaf table.  It is written by the enumerator from the root specs the host built, not read from a block; it is
// still compared with n_tipsets before it indexes anything.
//
//   k_tipset_bounds         first[s] = position of the first leaf with seq ≥ s, for s = 0 … T (first[T] = n): a tipset
//                           without a leaf (an empty tree, a tree that failed) gets first[s] == first[s + 1]
//   PASS 1  k_count_tipsets_table / _walk   k_count_multi_* with the error of a receipt in err[seq] and the 32-bit overflow
//                           of a receipt's count in ovf[seq] (T words each: a failing tipset's overflow refuses nothing)
//   k_tipset_mask           counts of every leaf whose tipset has its error word set → 0 (its range of records is empty)
//   k_tipset_shapes         per tipset: last index + 1 (the size of its map) and the record offset at its first leaf
//   PASS 2  k_fill_tipsets_table / _walk    k_fill_multi_* with the map byte at receipt_off[seq] + index, checked against
//                           the tipset's own size, and the recorder's receipts root taken from roots[seq]
// The table kernels hold no walker and use no scratch, as in event_scan_multi.inc.

namespace ipcfp {

// per-tipset tables of one call (device).  receipt_off: n_tipsets + 1 offsets into the concatenated map, a failing tipset's
// range empty (host/scan_tipsets_layout.h wrote them)
struct TipsetsView {
    const AmtRootSpec* roots;           // roots[s].root: the receipts root; roots[s].skip: its enumeration failed
    const unsigned long long* err;      // PASS 1's error word per tipset (kNoEnumError: none)
    const uint64_t* receipt_off;
    uint32_t n_tipsets;
};

__global__ __launch_bounds__(256) void k_tipset_bounds(const LeafRef* __restrict__ leaves, uint32_t n, uint32_t n_tipsets,
                                                       uint32_t* __restrict__ first /* n_tipsets + 1 */) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (n == 0) {  // (launched with one workgroup) no leaf at all: every tipset starts and ends at 0
        for (uint32_t s = t; s <= n_tipsets; s += gridDim.x * blockDim.x) first[s] = 0;
        return;
    }
    if (t >= n) return;
    const uint32_t cur = leaves[t].seq < n_tipsets ? leaves[t].seq : n_tipsets - 1u;
    // the tipsets whose first leaf-or-later is t: those after the previous leaf's, up to this leaf's
    uint32_t s = 0;
    if (t) {
        const uint32_t prev = leaves[t - 1].seq < n_tipsets ? leaves[t - 1].seq : n_tipsets - 1u;
        s = prev + 1u;
    }
    for (; s <= cur; ++s) first[s] = t;
    if (t == n - 1)
        for (s = cur + 1u; s <= n_tipsets; ++s) first[s] = n;
}

__global__ __launch_bounds__(256) void k_count_tipsets_table(WitnessView w, const LeafRef* __restrict__ receipts, uint32_t n, FsView fs,
                                                             const ReceiptRec* __restrict__ rrecs, const EventRec* __restrict__ erecs,
                                                             uint32_t* __restrict__ counts, unsigned long long* __restrict__ err,
                                                             uint32_t n_tipsets) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const ReceiptRec rr = rrecs[t];
    uint32_t c = 0;
    if (rr.kind == RK_TABLE) {
        const uint32_t ne = __popcll(rr.bitmap);
        for (uint32_t j = 0; j < ne; ++j) {
            const EventRec e = erecs[rr.first + j];
            const uint32_t g = rec_group(w.arena, e, fs);
            if (g != kFsNone) c += group_count(fs, g, e.emitter);
        }
    } else if (rr.kind == RK_WALK) {
        c = kWalkPending;
    } else if (rr.kind >= 64) {
        const uint32_t seq = receipts[t].seq;
        if (seq < n_tipsets) atomicMin(err + seq, (unsigned long long)pack_enum_error(1, t, rr.kind));
    }
    counts[t] = c;
}

__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_count_tipsets_walk(WitnessView w, const LeafRef* __restrict__ receipts, uint32_t n,
                                                                              FsView fs, int pending_only, uint32_t* __restrict__ counts,
                                                                              unsigned long long* __restrict__ err, uint32_t n_tipsets,
                                                                              unsigned long long* __restrict__ ovf) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    if (pending_only && counts[t] != kWalkPending) return;
    uint32_t c = 0;
    CidKey ev_root;
    if (receipts[t].block != kNoBlock && receipt_events_root(w, receipts[t], ev_root)) {
        auto visit = [&](uint64_t, uint32_t, Rd& er) {
            uint64_t emitter;
            EvmLogLoc log;
            decode_event_log(er, emitter, log);
            const uint32_t g = log_group(er, log, fs);
            if (g == kFsNone) return;
            const uint32_t gc = group_count(fs, g, emitter);  // (the bound: k_count_multi_walk)
            if (c > kWalkPending - 1u - gc) {
                c = kWalkPending - 1u;
                if (receipts[t].seq < n_tipsets) atomicMax(ovf + receipts[t].seq, 1ull);  // (a flag per tipset, as the errors)
            } else {
                c += gc;
            }
        };
        bool handled;
        uint32_t st = amt3_for_each_leaf_root(w, ev_root, handled, visit);
        if (!handled) {
            c = 0;
            AmtRootInfo info;
            st = amt_load(w, ev_root, 3, VK_STAMPED_EVENT, info);
            if (st == IPCFP_ST_TRUE) st = amt_for_each_lane(w, info, VK_STAMPED_EVENT, visit);
        }
        if (st != IPCFP_ST_TRUE) {
            const uint32_t seq = receipts[t].seq;
            if (seq < n_tipsets) atomicMin(err + seq, (unsigned long long)pack_enum_error(1, t, st));
            c = 0;
        }
    }
    counts[t] = c;
}

__global__ __launch_bounds__(256) void k_tipset_mask(const LeafRef* __restrict__ receipts, uint32_t n, uint32_t* __restrict__ counts,
                                                     const unsigned long long* __restrict__ err, uint32_t n_tipsets) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const uint32_t seq = receipts[t].seq;
    if (seq >= n_tipsets || err[seq] != kNoEnumError) counts[t] = 0;
}

// behind the prefix sum: n_idx[s] = the last leaf's index + 1 (0 without a leaf), match_start[s] = the record offset at the
// tipset's first leaf — the offset of the next leaf there is when it has none, the total behind the last leaf
__global__ __launch_bounds__(256) void k_tipset_shapes(const LeafRef* __restrict__ leaves, uint32_t n, const uint32_t* __restrict__ first,
                                                       const uint32_t* __restrict__ offsets, const uint64_t* __restrict__ total,
                                                       uint32_t n_tipsets, uint64_t* __restrict__ n_idx,
                                                       uint64_t* __restrict__ match_start) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_tipsets) return;
    const uint32_t a = first[s] < n ? first[s] : n, b = first[s + 1] < n ? first[s + 1] : n;
    n_idx[s] = b > a ? leaves[b - 1].index + 1 : 0;
    match_start[s] = a < n ? uint64_t(offsets[a]) : *total;
}

// the map byte of a leaf: inside its tipset's own range, and inside what the caller's capacity lets through
__device__ __forceinline__ void tipset_map_store(const TipsetsView& ts, const MultiOut& out, const LeafRef& leaf, uint32_t c) {
    if (leaf.seq >= ts.n_tipsets) return;
    const uint64_t lo = ts.receipt_off[leaf.seq], hi = ts.receipt_off[leaf.seq + 1];
    if (hi < lo || leaf.index >= hi - lo) return;  // (a failing tipset's range is empty)
    const uint64_t at = lo + leaf.index;
    if (at < out.has_cap) out.has_match[at] = c ? 1 : 0;
}

__global__ __launch_bounds__(256) void k_fill_tipsets_table(WitnessView w, const LeafRef* __restrict__ receipts, uint32_t n, FsView fs,
                                                            const ReceiptRec* __restrict__ rrecs, const EventRec* __restrict__ erecs,
                                                            const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                            MultiOut out, TipsetsView ts) {
    __shared__ uint32_t s_hist[IPCFP_MAX_SCAN_SPECS];
    hist_clear(s_hist);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) {
        const uint32_t c = counts[t];
        const LeafRef leaf = receipts[t];
        tipset_map_store(ts, out, leaf, c);
        const ReceiptRec rr = rrecs[t];
        if (c && rr.kind == RK_TABLE) {  // (the rest is k_fill_tipsets_walk's)
            uint32_t k = 0, ord = 0;
            const uint64_t o = offsets[t];
            const uint64_t block_base = w.off[rr.block];
            for (uint32_t j = 0; j < 64; ++j) {
                if (!((rr.bitmap >> j) & 1ull)) continue;
                const EventRec e = erecs[rr.first + ord++];
                const uint32_t g = rec_group(w.arena, e, fs);
                if (g == kFsNone) continue;
                const EventMatch m{leaf.index, j, e.emitter, ValueLoc{rr.block, uint32_t((e.base_flags & kEvBaseMask) - block_base), e.ev_len}, 0};
                emit_members(fs, g, m, out, o, c, k, s_hist);
            }
        }
    }
    hist_flush(s_hist, fs.n_specs, out.spec_counts);
}

// (launch bounds as k_fill_multi_walk)
__global__ __launch_bounds__(256, 2) void k_fill_tipsets_walk(WitnessView w, const LeafRef* __restrict__ receipts, uint32_t n, FsView fs,
                                                              const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                              MultiOut out, TipsetsView ts, const ReceiptRec* __restrict__ skip_tabulated) {
    __shared__ uint32_t s_hist[IPCFP_MAX_SCAN_SPECS];
    hist_clear(s_hist);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool recording = w.touched != nullptr;
    // every sound tipset's `Amtv0::load(&receipts_root, &rec_receipts)` records its root, matches or not (:195-196)
    if (recording && t < ts.n_tipsets && !ts.roots[t].skip && ts.err[t] == kNoEnumError) {
        AmtRootInfo info;
        (void)amt_load(w, ts.roots[t].root, 0, VK_RECEIPT, info);
    }
    if (t < n) {
        const LeafRef leaf = receipts[t];
        const uint32_t c = counts[t];
        tipset_map_store(ts, out, leaf, c);
        if (c && leaf.seq < ts.n_tipsets && !(skip_tabulated && skip_tabulated[t].kind == RK_TABLE)) {
            if (recording) {  // `r_amt.get(i)` on the recorder (:249): its observable effect is the recorded path
                AmtRootInfo rinfo;
                if (amt_load(w, ts.roots[leaf.seq].root, 0, VK_RECEIPT, rinfo) == IPCFP_ST_TRUE) {
                    ValueLoc rl;
                    (void)amt_get(w, rinfo, VK_RECEIPT, leaf.index, rl);
                }
            }
            CidKey ev_root;
            if (receipt_events_root(w, leaf, ev_root)) {
                uint32_t k = 0;
                const uint64_t o = offsets[t];
                auto visit = [&](uint64_t j, uint32_t b, Rd& er) {
                    const uint32_t start = er.pos;
                    uint64_t emitter;
                    EvmLogLoc log;
                    decode_event_log(er, emitter, log);
                    const uint32_t g = log_group(er, log, fs);
                    if (g == kFsNone) return;
                    const EventMatch m{leaf.index, j, emitter, ValueLoc{b, start, er.pos - start}, 0};
                    emit_members(fs, g, m, out, o, c, k, s_hist);
                };
                // the same blocks in the same order as PASS 1, which found them sound: nothing here can fail
                bool handled;
                (void)amt3_for_each_leaf_root(w, ev_root, handled, visit);
                if (!handled) {
                    AmtRootInfo info;
                    if (amt_load(w, ev_root, 3, VK_STAMPED_EVENT, info) == IPCFP_ST_TRUE)
                        (void)amt_for_each_lane(w, info, VK_STAMPED_EVENT, visit);
                }
            }
        }
    }
    hist_flush(s_hist, fs.n_specs, out.spec_counts);
}

int launch_tipset_bounds(ipcfp_ctx* ctx, const LeafRef* leaves_d, uint32_t n, uint32_t n_tipsets, uint32_t* first_d) {
    {
        ProfileScope prof(ctx, IPCFP_K_SCAN_TIPSETS);
        hipLaunchKernelGGL(k_tipset_bounds, dim3(n ? div_up(n, 256) : 1u), dim3(256), 0, ctx->stream, leaves_d, n, n_tipsets, first_d);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_count_tipsets(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n, const FsView& fs,
                         const EventTableView* table, uint32_t* counts_d, unsigned long long* err_d, uint32_t n_tipsets,
                         unsigned long long* ovf_d) {
    if (n == 0) return IPCFP_OK;
    {
        ProfileScope prof(ctx, IPCFP_K_SCAN_TIPSETS);
        const bool tab = table && table->receipts;
        if (tab)
            hipLaunchKernelGGL(k_count_tipsets_table, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w, receipts_d, n, fs,
                               table->receipts, table->events, counts_d, err_d, n_tipsets);
        hipLaunchKernelGGL(k_count_tipsets_walk, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w, receipts_d, n, fs, tab ? 1 : 0,
                           counts_d, err_d, n_tipsets, ovf_d);
        hipLaunchKernelGGL(k_tipset_mask, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, receipts_d, n, counts_d, err_d, n_tipsets);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_tipset_shapes(ipcfp_ctx* ctx, const LeafRef* leaves_d, uint32_t n, const uint32_t* first_d, const uint32_t* offsets_d,
                         const uint64_t* total_d, uint32_t n_tipsets, uint64_t* n_idx_d, uint64_t* match_start_d) {
    {
        ProfileScope prof(ctx, IPCFP_K_SCAN_TIPSETS);
        hipLaunchKernelGGL(k_tipset_shapes, dim3(div_up(n_tipsets, 256)), dim3(256), 0, ctx->stream, leaves_d, n, first_d, offsets_d,
                           total_d, n_tipsets, n_idx_d, match_start_d);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_fill_tipsets(ipcfp_ctx* ctx, const WitnessView& w, const AmtRootSpec* roots_d, const unsigned long long* err_d,
                        const uint64_t* receipt_off_d, uint32_t n_tipsets, const LeafRef* receipts_d, uint32_t n, const FsView& fs,
                        const uint32_t* counts_d, const uint32_t* offsets_d, void* matches_d, uint32_t* match_spec_d,
                        uint64_t matches_cap, uint8_t* has_match_d, uint64_t has_cap, unsigned long long* spec_counts_d,
                        const EventTableView* table) {
    const MultiOut out{static_cast<EventMatch*>(matches_d), match_spec_d, matches_cap, has_match_d, has_cap, 0, spec_counts_d};
    const TipsetsView ts{roots_d, err_d, receipt_off_d, n_tipsets};
    const uint32_t threads = n > n_tipsets ? n : n_tipsets;  // (a lane per tipset records its root)
    {
        ProfileScope prof(ctx, IPCFP_K_SCAN_TIPSETS);
        // without a recorder the matches of tabulated receipts are read off the records (as launch_fill_multi)
        const bool use_table = table && table->receipts && !w.touched && n;
        if (use_table)
            hipLaunchKernelGGL(k_fill_tipsets_table, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w, receipts_d, n, fs,
                               table->receipts, table->events, counts_d, offsets_d, out, ts);
        hipLaunchKernelGGL(k_fill_tipsets_walk, dim3(div_up(threads, 256)), dim3(256), 0, ctx->stream, w, receipts_d, n, fs, counts_d,
                           offsets_d, out, ts, use_table ? table->receipts : nullptr);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
