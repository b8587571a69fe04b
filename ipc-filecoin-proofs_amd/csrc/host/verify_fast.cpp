// csrc/host/verify_fast.cpp — `verify_event_proof` for a batch of ONE tipset pair without a mid-call synchronisation.
//
// host/verify_events.cpp::verify_packed waits for the device twice before the verify kernel runs — for the AMT roots'
// shapes (to size the walk) and for the walk's anomaly flag — and each wait drains the stream, wakes the host and
// leaves the GPU idle until the next launch arrives (≈40 + ≈80 µs of a 1.3 ms step).  Here
//   * the root shapes reach the host through the MAILBOX — a page of coherent pinned host memory that k_enum_roots
//     writes while the stream keeps going — so the host sizes and queues everything else without draining anything;
//   * the anomaly flag is read at the END of the call, with the status bytes: every kernel behind the walk is queued
//     before the host knows whether the dense walk held.  They are safe on whatever it left (k_dense_leaves writes every
//     LeafRef it owes, kNoBlock when there is no value; readers skip those), and when the flag is set — a sparse AMT, a
//     lying count, a missing block, a decode error — the call's results are thrown away and verify_packed does the
//     whole batch again its own way (the general level-synchronous walk orders errors as the reference does);
//   * what the host did between the second wait and the verify kernel (is the execution order reachable, where are the
//     tables, exec_len, the inverse permutation) happens on the device (k_exec_scan_finish).
// The call synchronises once.  Same kernels otherwise, same results: tests/test_gpu_events.py, test_gpu_baseline_sizes.py,
// test_gpu_enum_shapes.py (every shape that leaves the dense path) run through this file first.
#include <chrono>
#include <cstring>
#include <memory>
#include <vector>

#include "../common.h"
#include "../kernels/claims_dev.h"
#include "../kernels/amt_enum.h"
#include "../kernels/event_table.h"
#include "../kernels/tipset_ctx.h"
#include "../kernels/types_dev.h"
#include "../kernels/launch.h"
#include "exec_state.h"

using namespace ipcfp;

namespace ipcfp {

// → IPCFP_OK with *done = true: status_d (and where_d) hold the batch's results;
//   IPCFP_OK with *done = false: not this route's case, or the dense walk did not hold — nothing the caller may use;
//   anything else: an ABI error.
static int verify_packed_fast_queue(ipcfp_ctx* ctx, ipcfp_witness* w, std::vector<TipsetCtxDev>& tcs, const EventClaimPacked* claims_d,
                                    uint32_t n, const uint8_t* blob_d, uint64_t blob_len, const ipcfp_trust_policy_t* trust,
                                    const ipcfp_event_filter_t* filter, uint8_t* status_d, void* where_d, bool* done, ScanRide* ride);

int verify_packed_fast(ipcfp_ctx* ctx, ipcfp_witness* w, std::vector<TipsetCtxDev>& tcs, const EventClaimPacked* claims_d,
                       uint32_t n, const uint8_t* blob_d, uint64_t blob_len, const ipcfp_trust_policy_t* trust,
                       const ipcfp_event_filter_t* filter, uint8_t* status_d, void* where_d, bool* done, ScanRide* ride) {
    const int rc = verify_packed_fast_queue(ctx, w, tcs, claims_d, n, blob_d, blob_len, trust, filter, status_d, where_d, done, ride);
    if (rc != IPCFP_OK) {
        // An error return may have left kernels on the main and the aux stream that still use this call's pooled scratch
        // (the leaves, the receipts' event records, the deferred re-hash): the buffers went back to the pool when the
        // function returned, and nothing may be handed out again before those kernels are through.
        (void)upload_task_wait(ctx);
        (void)hipStreamSynchronize(ctx->stream_aux);
        (void)hipStreamSynchronize(ctx->stream);
        if (w->bt_valid) w->bt_joined = true;
    }
    return rc;
}

static int verify_packed_fast_queue(ipcfp_ctx* ctx, ipcfp_witness* w, std::vector<TipsetCtxDev>& tcs, const EventClaimPacked* claims_d,
                                    uint32_t n, const uint8_t* blob_d, uint64_t blob_len, const ipcfp_trust_policy_t* trust,
                                    const ipcfp_event_filter_t* filter, uint8_t* status_d, void* where_d, bool* done, ScanRide* ride) {
    static const ipcfp_trust_policy_t accept_all = {0, 0, 0, 0};
    const bool enabled = ctx->fast_verify != 0;  // (ipcfp_ctx_set_tuning "fast_verify")
    *done = false;
    if (!enabled || !ctx->mailbox || tcs.size() != 1 || !w->use_event_table || ctx->stream_aux == ctx->stream) return IPCFP_OK;
    const TipsetCtxDev& in = tcs[0];
    if (!(in.flags & TC_PARENTS_PARSED) || !(in.flags & TC_CHILD_PARSED) || in.n_parents == 0 || in.n_parents > kMaxParents) return IPCFP_OK;
    for (auto& e : w->enum_cache)  // a scan enumerated the receipts already: verify_packed shares that enumeration
        if (e->vkind == VK_RECEIPT && e->lo == w->receipt_lo && e->hi == w->receipt_hi) return IPCFP_OK;
    const WitnessView view = witness_view(w);
    const uint32_t P = in.n_parents, n_roots = 2 * P, n_all = n_roots + 1;
    // the block-order event parse runs beside everything below (aux stream), counting the last scan's filter
    int rc = ctx->has_scan_hint ? block_table_prefetch(ctx, w, &ctx->scan_hint.filter, int(ctx->scan_hint.has_actor), ctx->scan_hint.actor)
                                : block_table_prefetch(ctx, w, nullptr, 0, 0);
    if (rc) return rc;
    const bool need_general = prologue_needs_general(w->max_block_len);
    // The context on the device: a slice of the control block's ZERO half when there is room (re-initialised at the end of
    // the previous call) — its inputs then travel as a kernel argument of the prologue, which writes them in; no copy
    // kernel at the head of the call (17.7 µs beside the side streams' grids: profiles/r03_last_commit_timeline.txt).
    struct TcsDev {
        DevBuf<TipsetCtxDev> own;
        TipsetCtxDev* p = nullptr;
    } tcs_d;
    TipsetInputs inputs;
    std::memcpy(&inputs, &tcs[0], sizeof inputs);
    tcs_d.p = need_general ? nullptr : static_cast<TipsetCtxDev*>(ctl_take(ctx, sizeof(TipsetCtxDev), false));
    const bool inline_inputs = tcs_d.p != nullptr;
    if (!inline_inputs) {
        IPCFP_HIP(ctx, tcs_d.own.alloc(1));
        tcs_d.p = tcs_d.own.p;
        TipsetCtxDev init = tcs[0];
        for (uint32_t b = 0; b < IPCFP_MAX_PARENTS; ++b) init.txmeta_block[b] = 0;  // (nothing left to re-hash yet)
        IPCFP_HIP(ctx, h2d_small(ctx, tcs_d.p, &init, sizeof(TipsetCtxDev), ctx->stream));
    }
    ExecState ex;
    rc = exec_state_prepare(ctx, ex, P);
    if (rc) return rc;
    PrepareJob job{tcs_d.p, ex.roots.p, ex.err.p};
    DevBuf<EnumNode> frontier;
    DevBuf<DenseNode> dense_frontier;
    DevBuf<uint32_t> small_own;
    DevBuf<uint64_t> info_own;
    // [2] = anomaly flag (the dense walk).  Four words although one is used: every control word taken behind these keeps the
    // offset it has always had in the step's control block.
    uint32_t* small = nullptr;
    uint64_t* info_d = nullptr;
    IPCFP_HIP(ctx, frontier.alloc(n_all));
    IPCFP_HIP(ctx, dense_frontier.alloc(n_all));
    IPCFP_HIP(ctx, ctl_words(ctx, small_own, small, 4, false));
    IPCFP_HIP(ctx, ctl_words(ctx, info_own, info_d, 2 * size_t(n_all), false));
    std::unique_ptr<ProfileScope> prof(new ProfileScope(ctx, IPCFP_K_TIPSET_PROLOGUE));
    // (the TxMeta re-hashes — ≈ 3 k one-lane instructions per parent that gate nothing, they only ever add an error — are
    // left to a launch of their own on the aux stream, joined at the end of the call; not when a block may need the
    // general companion, which hashes inline)
    const bool defer_rehash = !need_general && ctx->rehash_event != nullptr;
    rc = launch_tipset_prepare(ctx, view, &job, nullptr, 1, need_general, defer_rehash, inline_inputs ? &inputs : nullptr);
    if (rc) return rc;
    // ---- the roots; their shapes come back through the mailbox ----
    const unsigned long long seq = ++ctx->mailbox_seq;
    rc = launch_enum_roots(ctx, view, ex.roots.p, n_all, VK_CID, frontier.p, ex.err.p, info_d, ctx->mailbox_dev, seq, dense_frontier.p);
    if (rc) return rc;
    prof.reset();
    {
        const auto deadline = std::chrono::steady_clock::now() + std::chrono::seconds(5);
        uint32_t spins = 0;
        while (__atomic_load_n(ctx->mailbox, __ATOMIC_ACQUIRE) != seq) {
            if ((++spins & 1023u) == 0 && std::chrono::steady_clock::now() > deadline) {
                IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));  // (a failed launch surfaces here)
                if (__atomic_load_n(ctx->mailbox, __ATOMIC_ACQUIRE) != seq)
                    return set_error(ctx, IPCFP_E_HIP, "the AMT roots' shapes never reached the mailbox");
            }
        }
    }
    std::vector<uint64_t> root_info(2 * size_t(n_all));
    for (size_t i = 0; i < root_info.size(); ++i) root_info[i] = __atomic_load_n(ctx->mailbox + 1 + i, __ATOMIC_RELAXED);
    DensePlan plan;
    dense_plan(root_info, n_roots, VK_CID, /*want_keys=*/true, 0, ~0ULL, 1, VK_RECEIPT, w->receipt_lo, w->receipt_hi, plan);
    if (!plan.ok || plan.n_use != n_all || plan.n_leaves == 0 || plan.n_extra == 0) {
        IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));  // (the kernels above still use this call's scratch)
        return IPCFP_OK;
    }
    // ---- everything else, queued in one go ----
    const uint32_t n_msgs = uint32_t(plan.n_leaves), n_rcpt = uint32_t(plan.n_extra);
    DevBuf<DenseNode> a, b;
    DevBuf<LeafRef> rleaves;
    IPCFP_HIP(ctx, a.alloc(plan.biggest));
    IPCFP_HIP(ctx, b.alloc(plan.biggest));
    IPCFP_HIP(ctx, ex.keys.alloc(n_msgs));
    IPCFP_HIP(ctx, rleaves.alloc(n_rcpt));
    // the execution order's hash table and first-occurrence flags: sized now, cleared by the walk's last kernel on the way
    const uint32_t size = exec_table_size(n_msgs);
    ex.mask = size - 1;
    ex.raw_len = n_msgs;
    IPCFP_HIP(ctx, ex.slots.alloc(size));
    // the flags, and behind them (8-byte aligned) the look-back words of k_exec_scan_finish: cleared together
    const size_t first_words = (size_t(n_msgs) + 1) & ~size_t(1), scan_ctl_words = exec_scan_ctl_words(n_msgs);
    IPCFP_HIP(ctx, ex.first.alloc(first_words + 2 * scan_ctl_words));
    IPCFP_HIP(ctx, ex.pos.alloc(n_msgs));
    IPCFP_HIP(ctx, ex.inv.alloc(n_msgs));
    unsigned long long* const scan_ctl = reinterpret_cast<unsigned long long*>(ex.first.p + first_words);
    const DenseClear clear{ex.slots.p, size, ex.first.p, first_words + 2 * scan_ctl_words};
    // the receipts' event records, written by the receipts tree's leaf kernel (k_dense_receipt_leaves) on the aux stream,
    // behind the block-order parse: allocated before the walk is queued; the walk's first interior kernel sets the error word
    std::unique_ptr<EventTableCached> table(new EventTableCached());
    table->lo = w->receipt_lo;
    table->hi = w->receipt_hi;
    table->n = n_rcpt;
    table->events = w->bt_events.p;
    IPCFP_HIP(ctx, table->receipts.alloc(n_rcpt));
    IPCFP_HIP(ctx, table->err_word.alloc(1));
    table->has_counts = w->bt_has_filter;
    if (table->has_counts) {
        table->counts_filter = w->bt_filter;
        IPCFP_HIP(ctx, table->counts.alloc(n_rcpt));
    }
    const DenseReceiptOut recs{w->bt_blocks.p, table->receipts.p, table->has_counts ? table->counts.p : nullptr, table->err_word.p};
    prof.reset(new ProfileScope(ctx, IPCFP_K_AMT_WALK));
    // the receipt leaves (and their records) are consumed on the aux stream, the message keys on the main stream: the two
    // leaf kernels fork accordingly and run side by side
    rc = launch_dense_walk(ctx, view, dense_frontier.p, plan, a.p, b.p, nullptr, ex.keys.p, rleaves.p, small + 2, ctx->stream_aux,
                           ctx->main_event, &clear, &recs);
    if (rc) return rc;
    prof.reset();
    // the receipts the table does not cover: the general walker, aux stream, right behind the leaves
    rc = launch_receipt_walk(ctx, view, rleaves.p, n_rcpt, table->has_counts ? &w->bt_filter.filter : nullptr,
                             int(w->bt_filter.has_actor), w->bt_filter.actor, table->receipts.p,
                             table->has_counts ? table->counts.p : nullptr, table->err_word.p, ctx->stream_aux);
    if (rc) return rc;
    IPCFP_HIP(ctx, hipEventRecord(ctx->aux_event, ctx->stream_aux));
    w->bt_joined = false;
    // ---- a scan riding on this call (ipcfp_verify_and_scan_device): its tail on the aux stream, behind the receipt records
    // and beside the verify kernel — it reads leaves, records and counts, never a claim's status ----
    DevBuf<uint32_t> ride_counts, ride_offsets;
    DevBuf<unsigned long long> ride_err_own;
    unsigned long long ride_seq = 0;
    if (ride && ride->cap_matches <= (1ull << 26) && (!ride->has_d || ride->cap_receipts >= n_rcpt)) {
        struct OnAux {  // everything queued "on the call's stream" below goes to the aux stream
            ipcfp_ctx* c;
            hipStream_t saved;
            ~OnAux() { c->stream = saved; }
        } on_aux{ctx, ctx->stream};
        ctx->stream = ctx->stream_aux;
        const ScanParams want = scan_params_of(ride->filter, ride->has_actor, ride->actor);
        const EventTableView tview = table->view();
        const uint32_t* cnt = nullptr;
        const unsigned long long* table_err = nullptr;
        unsigned long long* err_p = nullptr;
        IPCFP_HIP(ctx, ctl_words(ctx, ride_err_own, err_p, 1, true));
        if (table->has_counts && std::memcmp(&want, &table->counts_filter, sizeof want) == 0) {
            cnt = table->counts.p;  // counted while the table was built (the context's scan hint was this filter)
            table_err = table->err_word.p;
        } else {
            IPCFP_HIP(ctx, ride_counts.alloc(n_rcpt));
            rc = launch_count_from_table(ctx, view, rleaves.p, n_rcpt, ride->filter, ride->has_actor, ride->actor, tview, ride_counts.p, err_p);
            if (rc) return rc;
            cnt = ride_counts.p;
        }
        IPCFP_HIP(ctx, ride_offsets.alloc(n_rcpt));
        unsigned long long* tail_scratch = nullptr;
        rc = scan_tail_scratch(ctx, div_up(n_rcpt, 1024), &tail_scratch);
        if (rc) return rc;
        ride_seq = ++ctx->mailbox_seq;
        rc = launch_scan_tail_fused(ctx, view, rleaves.p, n_rcpt, w->receipt_lo, ride->filter, ride->has_actor, ride->actor, tview, cnt,
                                    ride_offsets.p, ride->cap_matches ? ride->matches_d : nullptr, ride->matches_d ? ride->cap_matches : 0,
                                    ride->has_d, ride->has_d ? n_rcpt : 0, w->receipt_lo, tail_scratch, ++ctx->scan_epoch, table_err,
                                    err_p, ctx->mailbox_dev, ride_seq);
        if (rc) return rc;
        ctx->scan_hint = want;
        ctx->has_scan_hint = true;
    }
    if (defer_rehash) {  // behind the receipts' event records, which the verify kernel waits for — this it does not wait for
        rc = launch_txmeta_rehash(ctx, ctx->stream_aux, view, tcs_d.p, ex.err.p);
        if (rc) return rc;
    }
    // the execution order: first-seen dedupe of the message CIDs, positions, inverse — main stream, beside the above
    prof.reset(new ProfileScope(ctx, IPCFP_K_EXEC_ORDER));
    // (table and flags were cleared by the walk's k_dense_link_leaves: launch_dense_walk `clear`)
    rc = launch_exec_insert_flags(ctx, ex.keys.p, n_msgs, ex.slots.p, ex.mask, ex.first.p);
    if (rc) return rc;
    IPCFP_HIP(ctx, ctl_words(ctx, ex.total_own, ex.total.p, 1, false));
    CtxFinish fin{};
    fin.err = ex.err.p;
    fin.total = ex.total.p;
    fin.first = ex.first.p;
    fin.pos = ex.pos.p;
    fin.inv = ex.inv.p;
    fin.slots = ex.slots.p;
    fin.keys = ex.keys.p;
    fin.mask = ex.mask;
    fin.raw_len = n_msgs;
    fin.receipt_leaves = rleaves.p;
    fin.n_receipt_leaves = n_rcpt;
    fin.receipt_first = w->receipt_lo;
    fin.receipt_recs = table->receipts.p;
    fin.event_recs = table->events;
    rc = launch_exec_scan_finish(ctx, tcs_d.p, fin, ex.pos.p, ex.total.p, scan_ctl);
    if (rc) return rc;
    prof.reset();
    rc = event_table_join(ctx, w);  // (the receipt records: aux_event as recorded behind k_receipt_walk)
    if (rc) return rc;
    if ((rc = claims_ready(ctx))) return rc;  // claims that were crossing PCIe beside all of the above are in HBM
    rc = launch_verify_events(ctx, view, claims_d, n, tcs_d.p, 1, blob_d, blob_len, trust ? *trust : accept_all, filter, status_d,
                              where_d, /*tabulated=*/true);
    if (rc) return rc;
    // the aux stream's tail — the re-hash, the riding scan — joins before the flags are read: its errors and the scan's
    // results are in when the call's one synchronisation returns.  (Recorded only now: the join above took the earlier
    // record, so the verify kernel does not wait for these.)
    if (defer_rehash || ride_seq) {
        hipEvent_t aux_done = defer_rehash ? ctx->rehash_event : ctx->aux_event;
        IPCFP_HIP(ctx, hipEventRecord(aux_done, ctx->stream_aux));
        IPCFP_HIP(ctx, hipStreamWaitEvent(ctx->stream, aux_done, 0));
    }
    // ---- the one synchronisation: did the dense walk hold? ----
    uint32_t bad = 0;
    unsigned long long e = kNoEnumError;
    TipsetCtxDev facts;
    IPCFP_HIP(ctx, ctl_read(ctx, &bad, small + 2, 4));
    IPCFP_HIP(ctx, ctl_read(ctx, &e, ex.err.p, 8));
    IPCFP_HIP(ctx, ctl_read(ctx, &facts, tcs_d.p, sizeof facts));  // (rides on the control block's one read-back when the context lives there)
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream, /*last_of_call=*/true));  // (a fallback below takes fresh words: still fine)
    IPCFP_HIP(ctx, hipGetLastError());
    if (bad || e != kNoEnumError || facts.child_status != IPCFP_ST_TRUE) {
        // (the aux stream may still be writing this call's buffers)
        IPCFP_HIP(ctx, hipStreamSynchronize(ctx->stream_aux));
        w->bt_joined = true;
        return IPCFP_OK;  // *done == false: verify_packed decides, in the reference's order of errors
    }
    tcs[0] = facts;
    // the enumeration of the receipts and their event table now belong to the witness: the scan that follows finds them
    {
        std::unique_ptr<EnumCached> en(new EnumCached());
        std::memcpy(en->root, facts.receipts_root.w, 40);
        en->version = 0;
        en->vkind = VK_RECEIPT;
        en->lo = w->receipt_lo;
        en->hi = w->receipt_hi;
        en->n = n_rcpt;
        en->error = kNoEnumError;
        en->dense = true;
        rleaves.move_to_bytes(en->leaves);
        w->enum_cache.push_back(std::move(en));
        std::memcpy(table->root, facts.receipts_root.w, 40);
        w->table_cache.push_back(std::move(table));
    }
    if (ride_seq) {  // (published before the synchronisation above returned: the main stream joined the tail's stream)
        if (__atomic_load_n(ctx->mailbox, __ATOMIC_ACQUIRE) != ride_seq) return set_error(ctx, IPCFP_E_HIP, "the riding scan's results never reached the mailbox");
        const uint64_t nm = __atomic_load_n(ctx->mailbox + 1, __ATOMIC_RELAXED);
        unsigned long long e1 = __atomic_load_n(ctx->mailbox + 3, __ATOMIC_RELAXED);
        const unsigned long long et = __atomic_load_n(ctx->mailbox + 2, __ATOMIC_RELAXED);
        const uint64_t walk = __atomic_load_n(ctx->mailbox + 4, __ATOMIC_RELAXED);
        if (et < e1) e1 = et;
        if (e1 != kNoEnumError) {
            ride->status = enum_error_code(e1);
            ride->done = true;
        } else if (!walk) {  // (receipts the table does not cover: the caller's ordinary scan walks them)
            ride->status = IPCFP_ST_TRUE;
            ride->n_idx = n_rcpt;
            ride->n_matches = nm;
            ride->done = true;
        }
    }
    *done = true;
    return IPCFP_OK;
}

}  // namespace ipcfp
