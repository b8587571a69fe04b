// csrc/kernels/event_scan_multi.inc — K6 for a SET of specs (ipcfp_scan_events_multi, host/scan_events_multi.cpp): the
// scan's two passes with every event probed ONCE against the filter set (filter_set.h) instead of compared with one filter.
//
// Included at the end of event_scan.hip: the general walkers (amt3_for_each_leaf_root, amt_for_each_lane,
// receipt_events_root) are templates of that translation unit, and the kernels here instantiate them with a visitor that
// probes the set.  The single-filter kernels above keep their text.
//
//   PASS 1  k_count_multi_table   one receipt per lane over the event table: a record that is a log with ≥ 2 topics loads
//                                 its 64 key bytes once, probes, and counts the group's members whose emitter filter
//                                 passes.  Receipts the table does not cover are left kWalkPending.  No walker in this
//                                 kernel: it holds no stack and uses no scratch.
//           k_count_multi_walk    the general walk for those receipts (or for every receipt of a witness without a table)
//   TAIL    k_scan_tail_multi     the table route without a recorder, in ONE launch: the prefix sum by decoupled look-back
//                                 (the body it shares with k_scan_tail_fused), the map, the tabulated receipts' matches, the
//                                 per-spec counts and the results in the mailbox
//   PASS 2  k_fill_multi_table    the has-map (some spec matches), matches + match_spec of tabulated receipts, per-spec counts
//           k_fill_multi_walk     the same through the walkers — untabulated receipts, and EVERY matching receipt when a
//                                 recorder is set (it marks the blocks the reference's RecordingBlockStores see)
// Order: a receipt's matches start at its offset (prefix sum of PASS 1's counts) and are written in event index order, an
// event's in member order, which is ascending spec index (filter_set.h) — the contract of include/ipcfp.h.
// Per-spec counts: a workgroup counts in LDS (one ds_add per match, 4 KB) and adds only its non-zero words to the global
// totals — no global atomic per match.
#include "filter_set.h"

namespace ipcfp {

// the group of a tabulated event, kFsNone when it is no log with two topics or no spec carries its key
__device__ __forceinline__ uint32_t rec_group(const uint8_t* __restrict__ arena, const EventRec& e, const FsView& fs) {
    const uint32_t nt = uint32_t(e.base_flags >> kEvTopicShift) & 0xffu;
    if (!(e.base_flags & kEvIsLog) || nt < 2) return kFsNone;
    const uint8_t* item = arena + (e.base_flags & kEvBaseMask);
    const uint8_t* t0 = item + e.topic_rel[0];
    const uint8_t* t1 = (e.base_flags & kEvCaseA) ? t0 + 32 : item + e.topic_rel[1];
    uint64_t key[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        __builtin_memcpy(&key[k], t0 + 8 * k, 8);
        __builtin_memcpy(&key[4 + k], t1 + 8 * k, 8);
    }
    return fs_probe(fs, key);
}

// … of an event a walker has just decoded
__device__ __forceinline__ uint32_t log_group(Rd& er, const EvmLogLoc& log, const FsView& fs) {
    if (!log.is_log || log.n_topics < 2) return kFsNone;
    // The topics lie inside the item the reader has just decoded.  Their words are loaded straight from the block (not
    // through the reader's window, whose state would stay live across the probe), folded into the fingerprint as they come
    // and loaded again for the (rare) confirming compare.
    const uint8_t* t0 = (const uint8_t*)(er.p + log.topic_at(0));
    const uint8_t* t1 = (const uint8_t*)(er.p + log.topic_at(1));
    uint64_t fp = fs_fp_init();
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        uint64_t v;
        __builtin_memcpy(&v, (k < 4 ? t0 : t1) + 8 * (k & 3), 8);
        fp = fs_fp_step(fp, v);
    }
    return fs_probe_with(fs, fp, [&](const uint64_t* gk) {
        uint64_t diff = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            uint64_t v;
            __builtin_memcpy(&v, (k < 4 ? t0 : t1) + 8 * (k & 3), 8);
            diff |= v ^ gk[k];
        }
        return diff == 0;
    });
}

// members of group g that an event of `emitter` satisfies
__device__ __forceinline__ uint32_t group_count(const FsView& fs, uint32_t g, uint64_t emitter) {
    const uint32_t first = fs.groups[g].first, count = fs.groups[g].count;
    uint32_t c = 0;
    for (uint32_t m = 0; m < count; ++m) {
        const FsMember mem = fs.members[first + m];
        c += (!mem.has_actor || mem.actor == emitter) ? 1u : 0u;
    }
    return c;
}

__global__ __launch_bounds__(256) void k_count_multi_table(WitnessView w, uint32_t n, FsView fs, const ReceiptRec* __restrict__ rrecs,
                                                           const EventRec* __restrict__ erecs, uint32_t* __restrict__ counts,
                                                           unsigned long long* __restrict__ err) {
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
        atomicMin(err, (unsigned long long)pack_enum_error(1, t, rr.kind));
    }
    counts[t] = c;
}

__global__ __launch_bounds__(256, IPCFP_WALK_WAVES) void k_count_multi_walk(WitnessView w, const LeafRef* __restrict__ receipts, uint32_t n,
                                                                            FsView fs, int pending_only, uint32_t* __restrict__ counts,
                                                                            unsigned long long* __restrict__ err,
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
            // a receipt's events are bounded only by the witness's size and every one may count for 1024 specs: the sum
            // stops short of kWalkPending and the call is refused (k_count_multi_table: ≤ 64 records, ≤ 2^16)
            const uint32_t gc = group_count(fs, g, emitter);
            if (c > kWalkPending - 1u - gc) {
                c = kWalkPending - 1u;
                atomicMax(ovf, 1ull);
            } else {
                c += gc;
            }
        };
        bool handled;
        uint32_t st = amt3_for_each_leaf_root(w, ev_root, handled, visit);
        if (!handled) {
            c = 0;  // (the leaf-root attempt calls the visitor only when it handles the root)
            AmtRootInfo info;
            st = amt_load(w, ev_root, 3, VK_STAMPED_EVENT, info);
            if (st == IPCFP_ST_TRUE) st = amt_for_each_lane(w, info, VK_STAMPED_EVENT, visit);
        }
        if (st != IPCFP_ST_TRUE) {
            atomicMin(err, (unsigned long long)pack_enum_error(1, t, st));
            c = 0;
        }
    }
    counts[t] = c;
}

struct MultiOut {
    EventMatch* matches;      // nullable: a sizing call
    uint32_t* match_spec;
    uint64_t cap;
    uint8_t* has_match;
    uint64_t has_cap, has_base;
    unsigned long long* spec_counts;  // n_specs totals
};

// one event's records: the members of group g that pass, from position o + k on (k counts them, cap or no cap)
__device__ __forceinline__ void emit_members(const FsView& fs, uint32_t g, const EventMatch& m, const MultiOut& out, uint64_t o, uint32_t c,
                                             uint32_t& k, uint32_t* s_hist) {
    const uint32_t first = fs.groups[g].first, count = fs.groups[g].count;
    for (uint32_t i = 0; i < count; ++i) {
        const FsMember mem = fs.members[first + i];
        if (mem.has_actor && mem.actor != m.emitter) continue;
        if (out.matches && k < c && o + k < out.cap) {
            out.matches[o + k] = m;
            out.match_spec[o + k] = mem.spec;
        }
        if (mem.spec < IPCFP_MAX_SCAN_SPECS) atomicAdd(&s_hist[mem.spec], 1u);
        ++k;
    }
}

__device__ __forceinline__ void hist_clear(uint32_t* s_hist) {
    for (uint32_t s = threadIdx.x; s < IPCFP_MAX_SCAN_SPECS; s += blockDim.x) s_hist[s] = 0;
    __syncthreads();
}
__device__ __forceinline__ void hist_flush(const uint32_t* s_hist, uint32_t n_specs, unsigned long long* spec_counts) {
    __syncthreads();
    for (uint32_t s = threadIdx.x; s < n_specs && s < IPCFP_MAX_SCAN_SPECS; s += blockDim.x) {
        const uint32_t v = s_hist[s];
        if (v) atomicAdd(spec_counts + s, (unsigned long long)v);
    }
}

__global__ __launch_bounds__(256) void k_fill_multi_table(WitnessView w, const LeafRef* __restrict__ receipts, uint32_t n, FsView fs,
                                                          const ReceiptRec* __restrict__ rrecs, const EventRec* __restrict__ erecs,
                                                          const uint32_t* __restrict__ counts, const uint32_t* __restrict__ offsets,
                                                          MultiOut out) {
    __shared__ uint32_t s_hist[IPCFP_MAX_SCAN_SPECS];
    hist_clear(s_hist);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) {
        const uint32_t c = counts[t];
        const uint64_t index = receipts[t].index;
        if (index >= out.has_base && index - out.has_base < out.has_cap) out.has_match[index - out.has_base] = c ? 1 : 0;
        const ReceiptRec rr = rrecs[t];
        if (c && rr.kind == RK_TABLE) {  // (the rest is k_fill_multi_walk's)
            uint32_t k = 0, ord = 0;
            const uint64_t o = offsets[t];
            const uint64_t block_base = w.off[rr.block];
            for (uint32_t j = 0; j < 64; ++j) {
                if (!((rr.bitmap >> j) & 1ull)) continue;
                const EventRec e = erecs[rr.first + ord++];
                const uint32_t g = rec_group(w.arena, e, fs);
                if (g == kFsNone) continue;
                const EventMatch m{index, j, e.emitter, ValueLoc{rr.block, uint32_t((e.base_flags & kEvBaseMask) - block_base), e.ev_len}, 0};
                emit_members(fs, g, m, out, o, c, k, s_hist);
            }
        }
    }
    hist_flush(s_hist, fs.n_specs, out.spec_counts);
}

// (launch bounds as k_scan_pass2: only the matching receipts do any work, the register allocator gets the whole file)
__global__ __launch_bounds__(256, 2) void k_fill_multi_walk(WitnessView w, CidKey receipts_root, const LeafRef* __restrict__ receipts,
                                                            uint32_t n, FsView fs, const uint32_t* __restrict__ counts,
                                                            const uint32_t* __restrict__ offsets, MultiOut out,
                                                            const ReceiptRec* __restrict__ skip_tabulated) {
    __shared__ uint32_t s_hist[IPCFP_MAX_SCAN_SPECS];
    hist_clear(s_hist);
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    const bool recording = w.touched != nullptr;
    if (t == 0 && recording) {  // `Amtv0::load(&receipts_root, &rec_receipts)` records the root even without matches (:195-196)
        AmtRootInfo info;
        (void)amt_load(w, receipts_root, 0, VK_RECEIPT, info);
    }
    if (t < n) {
        const LeafRef leaf = receipts[t];
        const uint32_t c = counts[t];
        if (leaf.index >= out.has_base && leaf.index - out.has_base < out.has_cap) out.has_match[leaf.index - out.has_base] = c ? 1 : 0;
        if (c && !(skip_tabulated && skip_tabulated[t].kind == RK_TABLE)) {
            if (recording) {  // `r_amt.get(i)` on the recorder (:249): its observable effect is the recorded path
                AmtRootInfo rinfo;
                if (amt_load(w, receipts_root, 0, VK_RECEIPT, rinfo) == IPCFP_ST_TRUE) {
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
                // the same blocks in the same order as PASS 1, which found them sound: nothing here can fail (:259-:262)
                bool handled;
                (void)amt3_for_each_leaf_root(w, ev_root, handled, visit);
                if (!handled) {
                    // (the leaf-root attempt calls the visitor only when it handles the root: nothing was emitted)
                    AmtRootInfo info;
                    if (amt_load(w, ev_root, 3, VK_STAMPED_EVENT, info) == IPCFP_ST_TRUE)
                        (void)amt_for_each_lane(w, info, VK_STAMPED_EVENT, visit);
                }
            }
        }
    }
    hist_flush(s_hist, fs.n_specs, out.spec_counts);
}

// The tail of the table route in ONE launch — k_scan_tail_fused for a set: the prefix sum over PASS 1's counts by decoupled
// look-back (scan_tail_lookback, the one text of it), the any-spec map, offsets, matches + match_spec of tabulated
// receipts, the per-spec counts (LDS histogram, flushed once per workgroup) and the call's results in the mailbox:
// (an Err of PASS 1 is in *err_b before the launch: the kernel then writes no map byte, no record and no count)
//   [0] seq  [1] total  [2] *err_a  [3] *err_b  [4] matching receipts left to the general walk  [5] the total left 32 bits
// The look-back's words carry 32 bits of a sum.  The FIRST tile whose inclusive prefix reaches 2^32 − 1 has only exact
// words behind it (every earlier aggregate and prefix is smaller), so it sees the excess exactly and raises *ovf; what
// later tiles compute is then never used (the host returns IPCFP_E_UNSUPPORTED).
__global__ __launch_bounds__(256) void k_scan_tail_multi(WitnessView w, const LeafRef* __restrict__ receipts, uint32_t n,
                                                         uint64_t dense_first, FsView fs, const ReceiptRec* __restrict__ rrecs,
                                                         const EventRec* __restrict__ erecs, const uint32_t* __restrict__ counts,
                                                         uint32_t* __restrict__ offsets, MultiOut out, ScanTailCtl ctl,
                                                         unsigned int* __restrict__ untabulated, unsigned long long* __restrict__ ovf) {
    __shared__ uint64_t smem[17];
    __shared__ uint32_t s_tile;
    __shared__ uint64_t s_prefix;
    __shared__ uint32_t s_hist[IPCFP_MAX_SCAN_SPECS];
    const uint32_t n_tiles = (n + kScanTile - 1) / kScanTile;
    if (threadIdx.x == 0) s_tile = atomicAdd(ctl.ticket, 1u);
    hist_clear(s_hist);  // (and the barrier behind s_tile)
    const uint32_t tile = s_tile;
    const uint32_t base = tile * kScanTile + threadIdx.x * 4u;
    uint32_t c[4];
    uint64_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        c[k] = base + k < n ? counts[base + k] : 0u;
        s += c[k];
    }
    uint64_t tile_total;
    const uint64_t ex = block_exclusive_scan(s, smem, &tile_total);
    if (threadIdx.x < 64) scan_tail_lookback(ctl, tile, n_tiles, tile_total, &s_prefix);
    __syncthreads();
    if (threadIdx.x == 0 && s_prefix + tile_total >= 0xffffffffull) {
        // (a returning exchange, consumed: performed before this lane's completion count below — see scan_tail_lookback)
        const unsigned long long before = atomicExch(ovf, 1ull);
        asm volatile("" ::"v"(before));
    }
    // PASS 1's verdict is in its error word before this launch starts: nothing is written for a tipset it rejected
    const bool sound = !ctl.err_b || __hip_atomic_load(ctl.err_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ~0ull;
    uint64_t o = s_prefix + ex;
#pragma unroll 1
    for (int k = 0; k < 4; ++k) {
        const uint32_t t = base + k;
        if (t >= n || !sound) break;
        const uint64_t index = dense_first != ~0ull ? dense_first + t : receipts[t].index;
        if (index >= out.has_base && index - out.has_base < out.has_cap) out.has_match[index - out.has_base] = c[k] ? 1 : 0;
        if (c[k]) {
            offsets[t] = uint32_t(o);
            const ReceiptRec rr = rrecs[t];
            if (rr.kind != RK_TABLE) {
                atomicAdd(untabulated, 1u);  // k_fill_multi_walk is queued behind this launch for it (and counts its specs)
            } else {
                uint32_t m = 0, ord = 0;
                const uint64_t block_base = w.off[rr.block];
                for (uint32_t j = 0; j < 64; ++j) {
                    if (!((rr.bitmap >> j) & 1ull)) continue;
                    const EventRec e = erecs[rr.first + ord++];
                    const uint32_t g = rec_group(w.arena, e, fs);
                    if (g == kFsNone) continue;
                    const EventMatch em{index, j, e.emitter, ValueLoc{rr.block, uint32_t((e.base_flags & kEvBaseMask) - block_base), e.ev_len}, 0};
                    emit_members(fs, g, em, out, o, c[k], m, s_hist);
                }
            }
        }
        o += c[k];
    }
    hist_flush(s_hist, fs.n_specs, out.spec_counts);
    // ---- the last workgroup to finish reports (no fence: as k_scan_tail_fused) ----
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int done = atomicAdd(ctl.ticket + 1, 1u);
        if (done == n_tiles - 1) {
            const unsigned long long total = atomicAdd(ctl.total, 0ull);
            const unsigned long long ea = ctl.err_a ? __hip_atomic_load(ctl.err_a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
            const unsigned long long eb = ctl.err_b ? __hip_atomic_load(ctl.err_b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ~0ull;
            const unsigned int walk = atomicExch(untabulated, 0u);
            const unsigned long long over = atomicAdd(ovf, 0ull);
            (void)atomicExch(ctl.ticket, 0u);
            (void)atomicExch(ctl.ticket + 1, 0u);
            __hip_atomic_store(ctl.mailbox + 1, total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(ctl.mailbox + 2, ea, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(ctl.mailbox + 3, eb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(ctl.mailbox + 4, (unsigned long long)walk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(ctl.mailbox + 5, over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(ctl.mailbox, ctl.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

int launch_scan_tail_multi(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n, uint64_t dense_first,
                           const FsView& fs, const EventTableView& table, const uint32_t* counts_d, uint32_t* offsets_d, void* matches_d,
                           uint32_t* match_spec_d, uint64_t matches_cap, uint8_t* has_match_d, uint64_t has_cap, uint64_t has_base,
                           unsigned long long* spec_counts_d, unsigned long long* scratch_d, unsigned long long epoch,
                           const unsigned long long* err_d, unsigned long long* ovf_d, unsigned long long* mailbox_dev,
                           unsigned long long seq) {
    const uint32_t n_tiles = div_up(n, kScanTile);
    ScanTailCtl ctl;  // (the scratch layout of launch_scan_tail_fused)
    ctl.ticket = reinterpret_cast<unsigned int*>(scratch_d);
    ctl.total = scratch_d + 2;
    ctl.state = scratch_d + 3;
    ctl.epoch = epoch & ((1ull << 30) - 1ull);
    ctl.err_a = nullptr;
    ctl.err_b = err_d;
    ctl.mailbox = mailbox_dev;
    ctl.seq = seq;
    const MultiOut out{static_cast<EventMatch*>(matches_d), match_spec_d, matches_cap, has_match_d, has_cap, has_base, spec_counts_d};
    {
        ProfileScope prof(ctx, IPCFP_K_SCAN_MULTI_TAIL);
        hipLaunchKernelGGL(k_scan_tail_multi, dim3(n_tiles), dim3(256), 0, ctx->stream, w, receipts_d, n, dense_first, fs, table.receipts,
                           table.events, counts_d, offsets_d, out, ctl, ctl.ticket + 2, ovf_d);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_count_multi(ipcfp_ctx* ctx, const WitnessView& w, const LeafRef* receipts_d, uint32_t n, const FsView& fs,
                       const EventTableView* table, uint32_t* counts_d, unsigned long long* err_d, unsigned long long* ovf_d) {
    if (n == 0) return IPCFP_OK;
    {
        ProfileScope prof(ctx, IPCFP_K_SCAN_MULTI_COUNT);
        const bool tab = table && table->receipts;
        if (tab)
            hipLaunchKernelGGL(k_count_multi_table, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w, n, fs, table->receipts,
                               table->events, counts_d, err_d);
        hipLaunchKernelGGL(k_count_multi_walk, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w, receipts_d, n, fs, tab ? 1 : 0,
                           counts_d, err_d, ovf_d);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_fill_multi(ipcfp_ctx* ctx, const WitnessView& w, const CidKey& receipts_root, const LeafRef* receipts_d, uint32_t n,
                      const FsView& fs, const uint32_t* counts_d, const uint32_t* offsets_d, void* matches_d, uint32_t* match_spec_d,
                      uint64_t matches_cap, uint8_t* has_match_d, uint64_t has_cap, uint64_t has_base,
                      unsigned long long* spec_counts_d, const EventTableView* table, bool tail_done) {
    const MultiOut out{static_cast<EventMatch*>(matches_d), match_spec_d, matches_cap, has_match_d, has_cap, has_base, spec_counts_d};
    const uint32_t threads = n ? n : 1;
    {
        ProfileScope prof(ctx, IPCFP_K_SCAN_MULTI_FILL);
        // without a recorder the matches of tabulated receipts are read off the records (as launch_scan_pass2)
        const bool use_table = table && table->receipts && !w.touched && n;
        if (use_table && !tail_done)
            hipLaunchKernelGGL(k_fill_multi_table, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w, receipts_d, n, fs,
                               table->receipts, table->events, counts_d, offsets_d, out);
        hipLaunchKernelGGL(k_fill_multi_walk, dim3(div_up(threads, 256)), dim3(256), 0, ctx->stream, w, receipts_root, receipts_d, n,
                           fs, counts_d, offsets_d, out, use_table ? table->receipts : nullptr);
    }
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
