// csrc/host/scan_events_tipsets.cpp — `find_matching_events` (src/proofs/events/generator.rs:180-307) for a CHAIN of tipsets
// and a set of event specs in one pass over the HBM-resident witness: what a caller that follows an epoch range asks
// ipcfp_scan_events_multi for root by root.  The answer is that of the n_tipsets single calls laid end to end.
//
// One enumeration walks every receipts tree together (kernels/amt_enum.h: seq = tipset number), PASS 1 and PASS 2 run over
// the concatenated leaves (kernels/event_scan_tipsets.inc), and the per-tipset statuses come out of
//   * the enumerator's ONE error word: it names the first failing tree.  That tipset gets its status (phase RECEIPTS), its
//     root spec is marked `skip`, and the roots are enumerated again — a chain with k failing trees takes k + 1 rounds, a
//     sound chain one.  Every round's work is at most that of the single calls it stands for;
//   * PASS 1's error words, one per tipset (phase EVENTS).
// A failing tipset has an empty range in the map and in the records (host/scan_tipsets_layout.h).
// The call touches none of the single calls' state: not the witness's caches of enumerations and event tables, not
// ctx->scan_hint, not the block table's filter (a block table it has to build is built without per-block counts).
#include <cstring>
#include <vector>

#include "../common.h"
#include "../kernels/amt_enum.h"
#include "../kernels/filter_set.h"
#include "../kernels/launch.h"
#include "exec_state.h"
#include "scan_events_multi.h"
#include "scan_events_tipsets.h"

using namespace ipcfp;

namespace ipcfp {

namespace {

// what the body's queued copies read or write on the host: owned by scan_events_tipsets_device, which drains the stream
struct TipsetsHost {
    std::vector<uint8_t> set;
    std::vector<AmtRootSpec> specs;
    std::vector<unsigned long long> words;  // [0, T) PASS 1's error words, [T, 2T) the 32-bit overflow flags
    std::vector<uint64_t> shapes;           // [0, T) n_idx, [T, 2T) the record offset at the first leaf
    uint64_t total = 0;                     // records over all sound tipsets
};

int scan_tipsets_body(ipcfp_ctx* ctx, ipcfp_witness* w, const uint8_t* roots40, uint32_t T, const ipcfp_event_filter_t* filters,
                      const uint8_t* has_actor, const uint64_t* actors, uint32_t n_specs, uint32_t* touched_d, TipsetsScanResult& out,
                      uint64_t cap_receipts, uint64_t cap_matches, TipsetsHost& host, const uint8_t* skip_mask) {
    const WitnessView view = witness_view(w);
    // the block-order event parse starts now (no filter: no per-block counts), beside the enumeration
    int rc = block_table_prefetch(ctx, w, nullptr, 0, 0);
    if (rc) return rc;
    DevBuf<uint8_t> set_dev;
    FsView fs{};
    rc = upload_filter_set(ctx, filters, has_actor, actors, n_specs, host.set, set_dev, fs);
    if (rc) return rc;
    out.status.assign(T, IPCFP_ST_ERR);
    out.phase.assign(T, 0);
    out.receipt_off.assign(size_t(T) + 1, 0);
    out.match_off.assign(size_t(T) + 1, 0);

    // ---- the receipts trees, all together; one more round per failing tree ----
    host.specs.assign(T, AmtRootSpec{});
    for (uint32_t t = 0; t < T; ++t) {
        host.specs[t].root = key_from_slot(roots40 + size_t(t) * IPCFP_CID_SLOT);
        host.specs[t].seq = t;
        if (skip_mask && skip_mask[t]) host.specs[t].skip = 1;  // the caller's: status ERR, phase 0, nothing walked or recorded
    }
    DevBuf<AmtRootSpec> roots;
    DevBuf<unsigned long long> enum_err;
    IPCFP_HIP(ctx, roots.alloc(T));
    IPCFP_HIP(ctx, enum_err.alloc(1));
    IPCFP_HIP(ctx, hipMemcpyAsync(roots.p, host.specs.data(), size_t(T) * sizeof(AmtRootSpec), hipMemcpyHostToDevice, ctx->stream));
    AmtEnumResult en;
    for (uint32_t round = 0;; ++round) {
        IPCFP_HIP(ctx, hipMemsetAsync(enum_err.p, 0xff, 8, ctx->stream));
        rc = amt_enumerate(ctx, view, roots.p, T, VK_RECEIPT, enum_err.p, en);
        if (rc) return rc;
        if (en.error == kNoEnumError) break;
        const uint32_t seq = uint32_t(en.error >> 48);
        if (seq >= T || host.specs[seq].skip || round >= T)
            return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_tipsets: the enumerator names tipset %u twice", seq);
        out.status[seq] = enum_error_code(en.error);
        out.phase[seq] = IPCFP_SCAN_PHASE_RECEIPTS;
        host.specs[seq].skip = 1;
        IPCFP_HIP(ctx, hipMemcpyAsync(roots.p + seq, &host.specs[seq], sizeof(AmtRootSpec), hipMemcpyHostToDevice, ctx->stream));
    }
    const LeafRef* leaves = en.leaves.p;
    const uint32_t n = uint32_t(en.n_leaves);

    // ---- boundaries, the receipt records, PASS 1, the prefix sum, the tipsets' shapes ----
    DevBuf<uint32_t> first, counts, offsets;
    DevBuf<unsigned long long> words;  // the layout of host.words
    DevBuf<uint64_t> shapes, scratch, total, table_err;
    DevBuf<ReceiptRec> rrecs;
    IPCFP_HIP(ctx, first.alloc(size_t(T) + 1));
    IPCFP_HIP(ctx, counts.alloc(n));
    IPCFP_HIP(ctx, offsets.alloc(n));
    IPCFP_HIP(ctx, words.alloc(2 * size_t(T)));
    IPCFP_HIP(ctx, shapes.alloc(2 * size_t(T)));
    IPCFP_HIP(ctx, scratch.alloc(size_t(div_up(n, 1024)) + 2));
    IPCFP_HIP(ctx, total.alloc(1));
    IPCFP_HIP(ctx, hipMemsetAsync(words.p, 0xff, size_t(T) * 8, ctx->stream));
    IPCFP_HIP(ctx, hipMemsetAsync(words.p + T, 0, size_t(T) * 8, ctx->stream));
    IPCFP_HIP(ctx, hipMemsetAsync(total.p, 0, 8, ctx->stream));
    unsigned long long* const err = words.p;
    unsigned long long* const ovf = words.p + T;
    rc = launch_tipset_bounds(ctx, leaves, n, T, first.p);
    if (rc) return rc;
    EventTableView tview{nullptr, nullptr};
    if (w->use_event_table && n) {  // the records of all leaves, local to the call (the per-root tables stay as they are)
        rc = event_table_join(ctx, w);
        if (rc) return rc;
        IPCFP_HIP(ctx, rrecs.alloc(n));
        IPCFP_HIP(ctx, table_err.alloc(1));
        IPCFP_HIP(ctx, hipMemsetAsync(table_err.p, 0xff, 8, ctx->stream));
        rc = launch_receipt_events(ctx, view, leaves, n, nullptr, 0, 0, w->bt_blocks.p, rrecs.p, nullptr,
                                   reinterpret_cast<unsigned long long*>(table_err.p), ctx->stream);
        if (rc) return rc;
        tview = EventTableView{rrecs.p, w->bt_events.p};
    }
    rc = launch_count_tipsets(ctx, view, leaves, n, fs, tview.receipts ? &tview : nullptr, counts.p, err, T, ovf);
    if (rc) return rc;
    if (n) {
        rc = launch_scan_u32(ctx, counts.p, n, offsets.p, total.p, scratch.p);
        if (rc) return rc;
    }
    rc = launch_tipset_shapes(ctx, leaves, n, first.p, offsets.p, total.p, T, shapes.p, shapes.p + T);
    if (rc) return rc;
    host.words.assign(2 * size_t(T), 0);
    host.shapes.assign(2 * size_t(T), 0);
    IPCFP_HIP(ctx, d2h_small(ctx, &host.total, total.p, 8, ctx->stream));
    IPCFP_HIP(ctx, d2h_small(ctx, host.words.data(), words.p, host.words.size() * 8, ctx->stream));
    IPCFP_HIP(ctx, d2h_small(ctx, host.shapes.data(), shapes.p, host.shapes.size() * 8, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));  // the ONE synchronisation between the enumeration and the fills

    // ---- statuses and the layout ----
    const uint64_t nm = host.total;
    std::vector<uint64_t> n_match(T);
    for (uint32_t t = 0; t < T; ++t) {
        const uint64_t next = t + 1 < T ? host.shapes[size_t(T) + t + 1] : nm;
        n_match[t] = next - host.shapes[size_t(T) + t];
        if (host.specs[t].skip) continue;  // (its status is the enumerator's)
        if (host.words[t] != kNoEnumError) {
            out.status[t] = enum_error_code(host.words[t]);
            out.phase[t] = IPCFP_SCAN_PHASE_EVENTS;
            continue;
        }
        if (host.words[size_t(T) + t])
            return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_tipsets: 2^32 - 1 or more matches over all specs (tipset %u)", t);
        out.status[t] = IPCFP_ST_TRUE;
    }
    if (nm >= 0xffffffffull) return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_tipsets: 2^32 - 1 or more matches over all tipsets and specs");
    const int lay = tipsets_layout(out.status.data(), host.shapes.data(), n_match.data(), T, cap_receipts, cap_matches,
                                   out.receipt_off.data(), out.match_off.data(), out.layout);
    if (lay != kLayoutOk)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_tipsets: too many %s over all tipsets", lay == kLayoutTooManyReceipts ? "receipts" : "matches");
    if (out.layout.n_matches != nm) return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_tipsets: the tipsets' record ranges do not add up");

    // ---- PASS 2 ----
    DevBuf<uint64_t> receipt_off;
    IPCFP_HIP(ctx, receipt_off.alloc(size_t(T) + 1));
    IPCFP_HIP(ctx, hipMemcpyAsync(receipt_off.p, out.receipt_off.data(), (size_t(T) + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    const uint64_t map_prefix = out.layout.map_prefix, match_prefix = out.layout.match_prefix;
    if (out.ext_has && map_prefix) {
        out.has_p = out.ext_has;
    } else {
        IPCFP_HIP(ctx, out.has.alloc(map_prefix));
        out.has_p = out.has.p;
    }
    if (map_prefix) IPCFP_HIP(ctx, hipMemsetAsync(out.has_p, 0, map_prefix, ctx->stream));
    if (out.ext_matches && out.ext_match_spec && match_prefix) {
        out.matches_p = out.ext_matches;
        out.match_spec_p = out.ext_match_spec;
    } else {
        IPCFP_HIP(ctx, out.matches.alloc(match_prefix));
        IPCFP_HIP(ctx, out.match_spec.alloc(match_prefix));
        out.matches_p = out.matches.p;
        out.match_spec_p = out.match_spec.p;
    }
    IPCFP_HIP(ctx, out.spec_counts.alloc(n_specs));
    out.spec_counts_p = out.spec_counts.p;
    IPCFP_HIP(ctx, hipMemsetAsync(out.spec_counts_p, 0, size_t(n_specs) * 8, ctx->stream));
    WitnessView rec = view;
    rec.touched = touched_d;
    rc = launch_fill_tipsets(ctx, rec, roots.p, err, receipt_off.p, T, leaves, n, fs, counts.p, offsets.p,
                             match_prefix ? out.matches_p : nullptr, match_prefix ? out.match_spec_p : nullptr, match_prefix,
                             out.has_p, map_prefix, reinterpret_cast<unsigned long long*>(out.spec_counts_p),
                             tview.receipts ? &tview : nullptr);
    if (rc) return rc;
    return IPCFP_OK;  // (the caller drains the stream: the kernels read buffers that go back to the pool with this frame)
}

}  // namespace

int scan_events_tipsets_device(ipcfp_ctx* ctx, ipcfp_witness* w, const uint8_t* roots40, uint32_t n_tipsets,
                               const ipcfp_event_filter_t* filters, const uint8_t* has_actor, const uint64_t* actors, uint32_t n_specs,
                               uint32_t* touched_d, TipsetsScanResult& out, uint64_t cap_receipts, uint64_t cap_matches,
                               const uint8_t* skip_mask) {
    // The body's copies read and write `host`, and its kernels read buffers that go back to the pool when it returns: the
    // stream is drained before either goes away, on every path (an error included), as scan_events_multi_device does.
    TipsetsHost host;
    const int rc = scan_tipsets_body(ctx, w, roots40, n_tipsets, filters, has_actor, actors, n_specs, touched_d, out, cap_receipts,
                                     cap_matches, host, skip_mask);
    const hipError_t e = sync_stream(ctx, ctx->stream);
    if (rc) return rc;
    IPCFP_HIP(ctx, e);
    return IPCFP_OK;
}

}  // namespace ipcfp

static int tipsets_args(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* roots, uint32_t n_tipsets,
                        const ipcfp_event_filter_t* filters, const uint8_t* has_actor, const uint64_t* actors, uint32_t n_specs,
                        ipcfp_status_t* tipset_status, uint64_t* n_receipts, uint64_t* n_matches) {
    if (!ctx || !w || w->ctx != ctx || !roots || !filters || !tipset_status || !n_receipts || !n_matches || n_specs == 0 ||
        n_tipsets == 0)
        return IPCFP_E_INVALID;
    if (has_actor && !actors)
        for (uint32_t j = 0; j < n_specs && j < IPCFP_MAX_SCAN_SPECS; ++j)
            if (has_actor[j]) return IPCFP_E_INVALID;
    if (w->receipt_lo != 0 || w->receipt_hi != ~0ULL) return IPCFP_E_INVALID;  // a shard is a cut of ONE tipset
    return IPCFP_OK;
}

// the per-tipset results → the caller's host arrays, and the witness's phase word
static void tipsets_report(ipcfp_witness_t* w, const TipsetsScanResult& res, uint32_t n_tipsets, ipcfp_status_t* tipset_status,
                           uint8_t* tipset_phase, uint64_t* receipt_off, uint64_t* match_off, uint64_t* n_receipts,
                           uint64_t* n_matches) {
    for (uint32_t t = 0; t < n_tipsets; ++t) {
        tipset_status[t] = ipcfp_status_t(res.status[t]);
        if (tipset_phase) tipset_phase[t] = res.phase[t];
    }
    if (receipt_off) std::memcpy(receipt_off, res.receipt_off.data(), (size_t(n_tipsets) + 1) * 8);
    if (match_off) std::memcpy(match_off, res.match_off.data(), (size_t(n_tipsets) + 1) * 8);
    *n_receipts = res.layout.n_receipts;
    *n_matches = res.layout.n_matches;
    w->last_scan_phase = res.layout.first_failing < 0 ? 0u : res.phase[size_t(res.layout.first_failing)];
}

extern "C" {

int ipcfp_scan_events_tipsets(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* receipts_roots40, uint32_t n_tipsets,
                              const ipcfp_event_filter_t* filters, const uint8_t* has_actor, const uint64_t* actors,
                              uint32_t n_specs, ipcfp_status_t* tipset_status, uint8_t* tipset_phase,
                              uint64_t* tipset_receipt_off, uint64_t* tipset_match_off, uint8_t* receipt_has_match,
                              uint64_t cap_receipts, uint64_t* n_receipts, ipcfp_event_match_t* matches, uint32_t* match_spec,
                              uint64_t cap_matches, uint64_t* n_matches, uint64_t* spec_counts, uint32_t* touched_bits) {
    if (tipsets_args(ctx, w, receipts_roots40, n_tipsets, filters, has_actor, actors, n_specs, tipset_status, n_receipts, n_matches))
        return IPCFP_E_INVALID;
    IPCFP_ENTER(ctx);
    if (n_tipsets > IPCFP_MAX_SCAN_TIPSETS)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_tipsets: %u tipsets (at most %d)", n_tipsets, IPCFP_MAX_SCAN_TIPSETS);
    if (n_specs > IPCFP_MAX_SCAN_SPECS)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_tipsets: %u specs (at most %d)", n_specs, IPCFP_MAX_SCAN_SPECS);
    *n_receipts = *n_matches = 0;
    if (!matches || !match_spec) cap_matches = 0;
    if (!receipt_has_match) cap_receipts = 0;
    const uint32_t words = div_up(w->n, 32);
    DevBuf<uint32_t> touched;
    if (touched_bits) {
        IPCFP_HIP(ctx, touched.alloc(words));
        IPCFP_HIP(ctx, hipMemsetAsync(touched.p, 0, size_t(words) * 4, ctx->stream));
    }
    TipsetsScanResult res;
    int rc = scan_events_tipsets_device(ctx, w, receipts_roots40, n_tipsets, filters, has_actor, actors, n_specs,
                                        touched_bits ? touched.p : nullptr, res, cap_receipts, cap_matches);
    if (rc) return rc;
    tipsets_report(w, res, n_tipsets, tipset_status, tipset_phase, tipset_receipt_off, tipset_match_off, n_receipts, n_matches);
    if (res.layout.map_prefix)
        IPCFP_HIP(ctx, hipMemcpyAsync(receipt_has_match, res.has_p, res.layout.map_prefix, hipMemcpyDeviceToHost, ctx->stream));
    if (res.layout.match_prefix) {
        IPCFP_HIP(ctx, hipMemcpyAsync(matches, res.matches_p, res.layout.match_prefix * sizeof(ipcfp_event_match_t),
                                      hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(match_spec, res.match_spec_p, res.layout.match_prefix * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                      ctx->stream));
    }
    if (spec_counts)
        IPCFP_HIP(ctx, hipMemcpyAsync(spec_counts, res.spec_counts_p, size_t(n_specs) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (touched_bits)
        IPCFP_HIP(ctx, hipMemcpyAsync(touched_bits, touched.p, size_t(words) * 4, hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    ctl_preprime(ctx);
    return IPCFP_OK;
}

int ipcfp_scan_events_tipsets_device(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* receipts_roots40, uint32_t n_tipsets,
                                     const ipcfp_event_filter_t* filters, const uint8_t* has_actor, const uint64_t* actors,
                                     uint32_t n_specs, ipcfp_status_t* tipset_status, uint8_t* tipset_phase,
                                     uint64_t* tipset_receipt_off, uint64_t* tipset_match_off, void* tipset_receipt_off_d,
                                     void* tipset_match_off_d, void* receipt_has_match_d, uint64_t cap_receipts,
                                     uint64_t* n_receipts, void* matches_d, void* match_spec_d, uint64_t cap_matches,
                                     uint64_t* n_matches, void* spec_counts_d) {
    if (tipsets_args(ctx, w, receipts_roots40, n_tipsets, filters, has_actor, actors, n_specs, tipset_status, n_receipts, n_matches))
        return IPCFP_E_INVALID;
    IPCFP_ENTER(ctx);
    if (n_tipsets > IPCFP_MAX_SCAN_TIPSETS)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_tipsets: %u tipsets (at most %d)", n_tipsets, IPCFP_MAX_SCAN_TIPSETS);
    if (n_specs > IPCFP_MAX_SCAN_SPECS)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "scan_events_tipsets: %u specs (at most %d)", n_specs, IPCFP_MAX_SCAN_SPECS);
    *n_receipts = *n_matches = 0;
    if (!matches_d || !match_spec_d) cap_matches = 0;
    if (!receipt_has_match_d) cap_receipts = 0;
    TipsetsScanResult res;
    res.ext_has = static_cast<uint8_t*>(receipt_has_match_d);
    res.ext_matches = cap_matches ? static_cast<ipcfp_event_match_t*>(matches_d) : nullptr;
    res.ext_match_spec = cap_matches ? static_cast<uint32_t*>(match_spec_d) : nullptr;
    int rc = scan_events_tipsets_device(ctx, w, receipts_roots40, n_tipsets, filters, has_actor, actors, n_specs, nullptr, res,
                                        cap_receipts, cap_matches);
    if (rc) return rc;
    tipsets_report(w, res, n_tipsets, tipset_status, tipset_phase, tipset_receipt_off, tipset_match_off, n_receipts, n_matches);
    const size_t off_bytes = (size_t(n_tipsets) + 1) * 8;  // (`res` outlives the copies: the stream is drained below)
    if (tipset_receipt_off_d)
        IPCFP_HIP(ctx, hipMemcpyAsync(tipset_receipt_off_d, res.receipt_off.data(), off_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (tipset_match_off_d)
        IPCFP_HIP(ctx, hipMemcpyAsync(tipset_match_off_d, res.match_off.data(), off_bytes, hipMemcpyHostToDevice, ctx->stream));
    if (spec_counts_d)
        IPCFP_HIP(ctx, hipMemcpyAsync(spec_counts_d, res.spec_counts_p, size_t(n_specs) * 8, hipMemcpyDeviceToDevice, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));  // `res` returns its buffers to the pool on exit
    ctl_preprime(ctx);
    return IPCFP_OK;
}

}  // extern "C"
