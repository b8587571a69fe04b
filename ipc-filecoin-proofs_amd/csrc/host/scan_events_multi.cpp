// csrc/host/scan_events_multi.cpp — `find_matching_events` (src/proofs/events/generator.rs:180-307) for a SET of event
// specs in one pass over the HBM-resident tipset: what `generate_proof_bundle` (src/proofs/generator.rs:58-78) asks for
// spec by spec.  One receipts enumeration, one event table, PASS 1 with every event probed against the filter set
// (kernels/filter_set.h), one prefix sum, PASS 2.
//
// A scan's status does not depend on its filter: PASS 1 reports an undecodable events tree before it looks at a topic, so
// the call has ONE status and ONE phase — those of every single-filter call on the same witness.
// The call touches none of the single-filter calls' state: not ctx->scan_hint, not the table's per-filter counts, not the
// block table's filter (a block table it has to build is built without per-block counts).
#include <cstring>
#include <vector>

#include "../common.h"
#include "../kernels/amt_enum.h"
#include "../kernels/filter_set.h"
#include "../kernels/launch.h"
#include "exec_state.h"
#include "scan_events_multi.h"

using namespace ipcfp;

namespace ipcfp {

// the set, built on the host and uploaded with ONE copy: [slots | groups | members]
int upload_filter_set(ipcfp_ctx* ctx, const ipcfp_event_filter_t* filters, const uint8_t* has_actor, const uint64_t* actors,
                      uint32_t n_specs, std::vector<uint8_t>& host, DevBuf<uint8_t>& dev, FsView& view) {
    const uint32_t n_slots = fs_slots_for(n_specs);
    const size_t slots_b = size_t(n_slots) * sizeof(FsSlot), groups_b = size_t(n_specs) * sizeof(FsGroup),
                 members_b = size_t(n_specs) * sizeof(FsMember);
    host.assign(slots_b + groups_b + members_b, 0);
    std::vector<uint32_t> group_of(n_specs);
    FsSlot* slots = reinterpret_cast<FsSlot*>(host.data());
    FsGroup* groups = reinterpret_cast<FsGroup*>(host.data() + slots_b);
    FsMember* members = reinterpret_cast<FsMember*>(host.data() + slots_b + groups_b);
    const uint32_t n_groups = fs_build(reinterpret_cast<const uint8_t*>(filters), has_actor, actors, n_specs, slots, n_slots, groups,
                                       members, group_of.data());
    IPCFP_HIP(ctx, dev.alloc(host.size()));
    IPCFP_HIP(ctx, hipMemcpyAsync(dev.p, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
    view = FsView{reinterpret_cast<const FsSlot*>(dev.p), reinterpret_cast<const FsGroup*>(dev.p + slots_b),
                  reinterpret_cast<const FsMember*>(dev.p + slots_b + groups_b), n_slots - 1u, n_groups, n_specs, 0};
    return IPCFP_OK;
}

// (the body: every early return leaves copies queued that read or write the caller's frame — see scan_events_multi_device)
static int scan_multi_body(ipcfp_ctx* ctx, ipcfp_witness* w, const CidKey& root, const ipcfp_event_filter_t* filters,
                           const uint8_t* has_actor, const uint64_t* actors, uint32_t n_specs, uint32_t* touched_d,
                           MultiScanResult& out, uint64_t cap_matches, std::vector<uint8_t>& set_host) {
    const WitnessView view = witness_view(w);
    // the block-order event parse starts now (no filter: no per-block counts), beside everything up to the table lookup
    int rc = block_table_prefetch(ctx, w, nullptr, 0, 0);
    if (rc) return rc;
    DevBuf<uint8_t> set_dev;
    FsView fs{};
    rc = upload_filter_set(ctx, filters, has_actor, actors, n_specs, set_host, set_dev, fs);
    if (rc) return rc;
    DevBuf<unsigned long long> err;  // [0] the first failing receipt (kNoEnumError), [1] raised when a count leaves 32 bits
    IPCFP_HIP(ctx, err.alloc(2));
    IPCFP_HIP(ctx, hipMemsetAsync(err.p, 0xff, 8, ctx->stream));
    IPCFP_HIP(ctx, hipMemsetAsync(err.p + 1, 0, 8, ctx->stream));
    unsigned long long* const ovf = err.p + 1;
    const EnumCached* en = nullptr;
    const uint64_t lo = w->receipt_lo, hi = w->receipt_hi;
    rc = amt_enumerate_cached(ctx, w, root, 0, VK_RECEIPT, &en, lo, hi);
    if (rc) return rc;
    if (en->error != kNoEnumError) {
        out.status = enum_error_code(en->error);
        out.phase = IPCFP_SCAN_PHASE_RECEIPTS;
        IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));  // (the set's upload reads set_host)
        return IPCFP_OK;
    }
    const LeafRef* leaves = reinterpret_cast<const LeafRef*>(en->leaves.p);
    const uint32_t n = uint32_t(en->n);
    uint64_t n_idx = 0;  // receipt indices are ascending: the last leaf gives the size of the per-index byte map
    if (n && en->dense) {
        n_idx = n;
    } else if (n) {
        LeafRef last;
        IPCFP_HIP(ctx, d2h_small(ctx, &last, leaves + (n - 1), sizeof last, ctx->stream));
        IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
        n_idx = last.index + 1 - lo;  // the per-index byte map starts at the shard's first index
    }
    DevBuf<uint32_t> counts, offsets;
    IPCFP_HIP(ctx, counts.alloc(n));
    IPCFP_HIP(ctx, offsets.alloc(n));
    EventTableView tview{nullptr, nullptr};
    if (w->use_event_table && n) {
        const EventTableCached* table = nullptr;
        rc = event_table_get(ctx, w, root, en, &table);
        if (rc) return rc;
        tview = table->view();
    }
    // PASS 1
    if (n) {
        rc = launch_count_multi(ctx, view, leaves, n, fs, tview.receipts ? &tview : nullptr, counts.p, err.p, ovf);
        if (rc) return rc;
    }
    // the tail in ONE launch, results through the mailbox: the rule of scan_events_device
    const bool fused = ctx->mailbox && tview.receipts && !touched_d && n && cap_matches <= (1ull << 26);
    // On an Err nothing is written for the caller.  The fused tail is queued before the status is known: it reads PASS 1's
    // error word itself and writes no record and no map byte of an unsound tipset, so it may write into the caller's
    // buffers — but not clear them first (a sparse enumeration's map), and the per-spec counts start from a clear.
    if (out.ext_has && out.ext_has_cap >= n_idx && !(fused && !en->dense)) {
        out.has_p = out.ext_has;
    } else {
        IPCFP_HIP(ctx, out.has.alloc(n_idx));
        out.has_p = out.has.p;
    }
    IPCFP_HIP(ctx, out.spec_counts.alloc(n_specs));
    out.spec_counts_p = out.spec_counts.p;
    IPCFP_HIP(ctx, hipMemsetAsync(out.spec_counts_p, 0, size_t(n_specs) * 8, ctx->stream));
    unsigned long long* const spec_counts = reinterpret_cast<unsigned long long*>(out.spec_counts_p);
    if (fused) {
        unsigned long long* tail_scratch = nullptr;
        rc = scan_tail_scratch(ctx, div_up(n, 1024), &tail_scratch);
        if (rc) return rc;
        if (n_idx && !en->dense) IPCFP_HIP(ctx, hipMemsetAsync(out.has_p, 0, n_idx, ctx->stream));
        if (out.ext_matches && out.ext_match_spec && cap_matches) {
            out.matches_p = out.ext_matches;
            out.match_spec_p = out.ext_match_spec;
        } else {
            IPCFP_HIP(ctx, out.matches.alloc(cap_matches));
            IPCFP_HIP(ctx, out.match_spec.alloc(cap_matches));
            out.matches_p = out.matches.p;
            out.match_spec_p = out.match_spec.p;
        }
        const unsigned long long seq = ++ctx->mailbox_seq;
        rc = launch_scan_tail_multi(ctx, view, leaves, n, en->dense ? lo : ~0ull, fs, tview, counts.p, offsets.p,
                                    cap_matches ? out.matches_p : nullptr, cap_matches ? out.match_spec_p : nullptr, cap_matches,
                                    out.has_p, n_idx, lo, spec_counts, tail_scratch, ++ctx->scan_epoch, err.p, ovf, ctx->mailbox_dev,
                                    seq);
        if (rc) return rc;
        rc = mailbox_wait(ctx, seq, "the multi scan's results");
        if (rc) return rc;
        const uint64_t nm = __atomic_load_n(ctx->mailbox + 1, __ATOMIC_RELAXED);
        const unsigned long long e1 = __atomic_load_n(ctx->mailbox + 3, __ATOMIC_RELAXED);
        const uint64_t walk = __atomic_load_n(ctx->mailbox + 4, __ATOMIC_RELAXED);
        const uint64_t over = __atomic_load_n(ctx->mailbox + 5, __ATOMIC_RELAXED);
        if (e1 != kNoEnumError) {
            out.status = enum_error_code(e1);
            out.phase = IPCFP_SCAN_PHASE_EVENTS;
            return IPCFP_OK;
        }
        if (over || nm >= 0xffffffffull) return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_multi: 2^32 - 1 or more matches over all specs");
        if (walk) {  // matching receipts the table does not cover: the general walk writes their records and counts their specs
            rc = launch_fill_multi(ctx, view, root, leaves, n, fs, counts.p, offsets.p, cap_matches ? out.matches_p : nullptr,
                                   cap_matches ? out.match_spec_p : nullptr, cap_matches, out.has_p, n_idx, lo, spec_counts, &tview, true);
            if (rc) return rc;
        }
        out.n_idx = n_idx;
        out.n_matches = nm;
        out.status = IPCFP_ST_TRUE;
        return IPCFP_OK;  // (the callers queue their copies behind this and synchronise: counts, offsets and the set outlive it)
    }
    // ---- the prefix sum, then PASS 2 (a recorder, no table, no mailbox, or a capacity too big to reserve blindly) ----
    DevBuf<uint64_t> scratch, total;
    IPCFP_HIP(ctx, scratch.alloc(size_t(div_up(n, 1024)) + 2));
    IPCFP_HIP(ctx, total.alloc(1));
    IPCFP_HIP(ctx, hipMemsetAsync(total.p, 0, 8, ctx->stream));
    uint64_t nm = 0;
    unsigned long long e1 = kNoEnumError, over = 0;
    if (n) {
        rc = launch_scan_u32(ctx, counts.p, n, offsets.p, total.p, scratch.p);
        if (rc) return rc;
        IPCFP_HIP(ctx, d2h_small(ctx, &nm, total.p, 8, ctx->stream));
        IPCFP_HIP(ctx, d2h_small(ctx, &e1, err.p, 8, ctx->stream));
        IPCFP_HIP(ctx, d2h_small(ctx, &over, ovf, 8, ctx->stream));
    }
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    if (e1 != kNoEnumError) {
        out.status = enum_error_code(e1);
        out.phase = IPCFP_SCAN_PHASE_EVENTS;
        return IPCFP_OK;
    }
    if (over || nm >= 0xffffffffull) return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_multi: 2^32 - 1 or more matches over all specs");
    if (n_idx) IPCFP_HIP(ctx, hipMemsetAsync(out.has_p, 0, n_idx, ctx->stream));
    const uint64_t cap = cap_matches < nm ? cap_matches : nm;
    if (out.ext_matches && out.ext_match_spec && cap) {
        out.matches_p = out.ext_matches;
        out.match_spec_p = out.ext_match_spec;
    } else {
        IPCFP_HIP(ctx, out.matches.alloc(cap));
        IPCFP_HIP(ctx, out.match_spec.alloc(cap));
        out.matches_p = out.matches.p;
        out.match_spec_p = out.match_spec.p;
    }
    WitnessView rec = view;
    rec.touched = touched_d;
    rc = launch_fill_multi(ctx, rec, root, leaves, n, fs, counts.p, offsets.p, cap ? out.matches_p : nullptr,
                           cap ? out.match_spec_p : nullptr, cap, out.has_p, n_idx, lo, spec_counts, tview.receipts ? &tview : nullptr,
                           false);
    if (rc) return rc;
    out.n_idx = n_idx;
    out.n_matches = nm;
    out.status = IPCFP_ST_TRUE;
    return IPCFP_OK;
}

int scan_events_multi_device(ipcfp_ctx* ctx, ipcfp_witness* w, const CidKey& root, const ipcfp_event_filter_t* filters,
                             const uint8_t* has_actor, const uint64_t* actors, uint32_t n_specs, uint32_t* touched_d,
                             MultiScanResult& out, uint64_t cap_matches) {
    // The set's upload reads `set_host`, and the body's kernels read buffers that go back to the pool when it returns: the
    // stream is drained before either goes away, on every path (an error included).  A caller that reads out.*_p queues
    // its copies on the same stream, behind nothing.
    std::vector<uint8_t> set_host;
    const int rc = scan_multi_body(ctx, w, root, filters, has_actor, actors, n_specs, touched_d, out, cap_matches, set_host);
    const hipError_t e = sync_stream(ctx, ctx->stream);
    if (rc) return rc;
    IPCFP_HIP(ctx, e);
    return IPCFP_OK;
}

}  // namespace ipcfp

static bool multi_args_ok(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* root, const ipcfp_event_filter_t* filters,
                          const uint8_t* has_actor, const uint64_t* actors, uint32_t n_specs, ipcfp_status_t* status_out,
                          uint64_t* n_receipts, uint64_t* n_matches) {
    if (!ctx || !w || w->ctx != ctx || !root || !filters || !status_out || !n_receipts || !n_matches || n_specs == 0) return false;
    if (has_actor && !actors)
        for (uint32_t j = 0; j < n_specs && j < IPCFP_MAX_SCAN_SPECS; ++j)
            if (has_actor[j]) return false;
    return true;
}

extern "C" {

int ipcfp_scan_events_multi(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* receipts_root40,
                            const ipcfp_event_filter_t* filters, const uint8_t* has_actor, const uint64_t* actors,
                            uint32_t n_specs, ipcfp_status_t* status_out, uint8_t* receipt_has_match, uint64_t cap_receipts,
                            uint64_t* n_receipts, ipcfp_event_match_t* matches, uint32_t* match_spec, uint64_t cap_matches,
                            uint64_t* n_matches, uint64_t* spec_counts, uint32_t* touched_bits) {
    if (!multi_args_ok(ctx, w, receipts_root40, filters, has_actor, actors, n_specs, status_out, n_receipts, n_matches))
        return IPCFP_E_INVALID;
    IPCFP_ENTER(ctx);
    if (n_specs > IPCFP_MAX_SCAN_SPECS) return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_multi: %u specs (at most %d)", n_specs, IPCFP_MAX_SCAN_SPECS);
    *n_receipts = *n_matches = 0;
    *status_out = IPCFP_ST_ERR;
    if (!matches || !match_spec) cap_matches = 0;
    const uint32_t words = div_up(w->n, 32);
    DevBuf<uint32_t> touched;
    if (touched_bits) {
        IPCFP_HIP(ctx, touched.alloc(words));
        IPCFP_HIP(ctx, hipMemsetAsync(touched.p, 0, size_t(words) * 4, ctx->stream));
    }
    MultiScanResult res;
    int rc = scan_events_multi_device(ctx, w, key_from_slot(receipts_root40), filters, has_actor, actors, n_specs,
                                      touched_bits ? touched.p : nullptr, res, cap_matches);
    if (rc) return rc;
    *status_out = ipcfp_status_t(res.status);
    w->last_scan_phase = res.status == IPCFP_ST_TRUE ? 0u : res.phase;
    if (res.status != IPCFP_ST_TRUE) return IPCFP_OK;
    *n_receipts = res.n_idx;
    *n_matches = res.n_matches;
    const uint64_t nm = res.n_matches < cap_matches ? res.n_matches : cap_matches;
    if (receipt_has_match && res.n_idx && cap_receipts)
        IPCFP_HIP(ctx, hipMemcpyAsync(receipt_has_match, res.has_p, res.n_idx < cap_receipts ? res.n_idx : cap_receipts,
                                      hipMemcpyDeviceToHost, ctx->stream));
    if (nm) {
        IPCFP_HIP(ctx, hipMemcpyAsync(matches, res.matches_p, nm * sizeof(ipcfp_event_match_t), hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(match_spec, res.match_spec_p, nm * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (spec_counts)
        IPCFP_HIP(ctx, hipMemcpyAsync(spec_counts, res.spec_counts_p, size_t(n_specs) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (touched_bits)
        IPCFP_HIP(ctx, hipMemcpyAsync(touched_bits, touched.p, size_t(words) * 4, hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    ctl_preprime(ctx);
    return IPCFP_OK;
}

int ipcfp_scan_events_multi_device(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* receipts_root40,
                                   const ipcfp_event_filter_t* filters, const uint8_t* has_actor, const uint64_t* actors,
                                   uint32_t n_specs, ipcfp_status_t* status_out, void* receipt_has_match_d,
                                   uint64_t cap_receipts, uint64_t* n_receipts, void* matches_d, void* match_spec_d,
                                   uint64_t cap_matches, uint64_t* n_matches, void* spec_counts_d, void* summary_d) {
    if (!multi_args_ok(ctx, w, receipts_root40, filters, has_actor, actors, n_specs, status_out, n_receipts, n_matches))
        return IPCFP_E_INVALID;
    IPCFP_ENTER(ctx);
    if (n_specs > IPCFP_MAX_SCAN_SPECS) return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_multi: %u specs (at most %d)", n_specs, IPCFP_MAX_SCAN_SPECS);
    *n_receipts = *n_matches = 0;
    *status_out = IPCFP_ST_ERR;
    if (!matches_d || !match_spec_d) cap_matches = 0;
    MultiScanResult res;
    res.ext_has = static_cast<uint8_t*>(receipt_has_match_d);
    res.ext_has_cap = receipt_has_match_d ? cap_receipts : 0;
    res.ext_matches = cap_matches ? static_cast<ipcfp_event_match_t*>(matches_d) : nullptr;
    res.ext_match_spec = cap_matches ? static_cast<uint32_t*>(match_spec_d) : nullptr;
    int rc = scan_events_multi_device(ctx, w, key_from_slot(receipts_root40), filters, has_actor, actors, n_specs, nullptr, res,
                                      cap_matches);
    if (rc) return rc;
    *status_out = ipcfp_status_t(res.status);
    w->last_scan_phase = res.status == IPCFP_ST_TRUE ? 0u : res.phase;
    if (summary_d) {  // {status | phase << 8, n_matches}, as ipcfp_scan_events_device
        const uint64_t sm[2] = {uint64_t(res.status) | (uint64_t(w->last_scan_phase) << 8), res.status == IPCFP_ST_TRUE ? res.n_matches : 0};
        IPCFP_HIP(ctx, h2d_small(ctx, summary_d, sm, sizeof sm, ctx->stream));
    }
    if (res.status == IPCFP_ST_TRUE) {
        *n_receipts = res.n_idx;
        *n_matches = res.n_matches;
        if (spec_counts_d)
            IPCFP_HIP(ctx, hipMemcpyAsync(spec_counts_d, res.spec_counts_p, size_t(n_specs) * 8, hipMemcpyDeviceToDevice, ctx->stream));
        // PASS 2 wrote straight into the caller's buffers when they were large enough; otherwise a (truncating) copy
        if (receipt_has_match_d && res.n_idx && res.has_p != receipt_has_match_d)
            IPCFP_HIP(ctx, hipMemcpyAsync(receipt_has_match_d, res.has_p, res.n_idx < cap_receipts ? res.n_idx : cap_receipts,
                                          hipMemcpyDeviceToDevice, ctx->stream));
    }
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));  // `res` returns its buffers to the pool on exit
    ctl_preprime(ctx);
    return IPCFP_OK;
}

}  // extern "C"
