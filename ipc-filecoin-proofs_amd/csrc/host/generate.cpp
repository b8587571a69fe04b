// csrc/host/generate.cpp — generator-side entry points: the device does every
// block load, hash and walk of `generate_event_proof` / `generate_storage_proof`; the host only sorts
// the recorded CIDs.
//
//   ipcfp_generate_event_proofs    src/proofs/events/generator.rs:75-178  (+ :180-307 via the scan)
//   ipcfp_generate_storage_proofs  src/proofs/storage/generator.rs:29-69
//   ipcfp_generate_storage_claims  src/proofs/storage/generator.rs:29-178, as column claims in HBM (kernels/storage_claims_gen.hip)
//
// The reference runs against an RPC blockstore and records every block it loads in a
// `RecordingBlockStore`; here the blockstore is the HBM-resident witness (the blocks a
// caller fetched for the tipset) and the recorder is a bitmap over its blocks.  The materialised
// witness is returned as block ids in `Cid: Ord` order (`collect_witness_blocks`,
// src/proofs/common/witness.rs:34-54 iterates a BTreeSet<Cid>).
#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "../common.h"
#include "../kernels/amt_enum.h"
#include "../kernels/claims_dev.h"
#include "../kernels/hamt_table.h"
#include "../kernels/launch.h"
#include "../kernels/storage_runs.h"
#include "exec_state.h"
#include "gen_tipsets_layout.h"
#include "scan_events_multi.h"
#include "scan_events_tipsets.h"
#include "tipset_wide.h"

using namespace ipcfp;

namespace {

struct CidOrd {  // the fields `#[derive(Ord)]` compares: version, codec, multihash {code, size, digest}
    uint64_t version = 0, codec = 0, mh_code = 0, mh_size = 0;
    const uint8_t* digest = nullptr;
    bool ok = false;
};

bool varint(const uint8_t* p, size_t n, size_t& pos, uint64_t& v) {
    v = 0;
    for (int i = 0; i < 9 && pos < n; ++i) {
        const uint8_t b = p[pos++];
        v |= uint64_t(b & 0x7f) << (7 * i);
        if (!(b & 0x80)) return true;
    }
    return false;
}

CidOrd cid_ord(const uint8_t* slot) {
    CidOrd o;
    if (slot[0] == 0x12 && slot[1] == 0x20) {  // CIDv0: bare sha2-256 multihash
        o.version = 0, o.codec = 0x70, o.mh_code = 0x12, o.mh_size = 32, o.digest = slot + 2, o.ok = true;
        return o;
    }
    size_t pos = 0;
    if (!varint(slot, IPCFP_CID_SLOT, pos, o.version) || !varint(slot, IPCFP_CID_SLOT, pos, o.codec) ||
        !varint(slot, IPCFP_CID_SLOT, pos, o.mh_code) || !varint(slot, IPCFP_CID_SLOT, pos, o.mh_size))
        return o;
    if (pos + o.mh_size > IPCFP_CID_SLOT) return o;
    o.digest = slot + pos;
    o.ok = true;
    return o;
}

bool cid_slot_less(const uint8_t* a, const uint8_t* b) {
    const CidOrd x = cid_ord(a), y = cid_ord(b);
    if (!x.ok || !y.ok) return std::memcmp(a, b, IPCFP_CID_SLOT) < 0;
    if (x.version != y.version) return x.version < y.version;
    if (x.codec != y.codec) return x.codec < y.codec;
    if (x.mh_code != y.mh_code) return x.mh_code < y.mh_code;
    if (x.mh_size != y.mh_size) return x.mh_size < y.mh_size;
    return std::memcmp(x.digest, y.digest, x.mh_size) < 0;
}

// recorded bitmap → block ids in `Cid: Ord` order (+ their CIDs)
int materialize(ipcfp_ctx* ctx, ipcfp_witness* w, const uint32_t* touched_d, uint32_t* ids_out, uint8_t* cids_out,
                uint64_t cap, uint64_t* n_out) {
    const uint32_t words = div_up(uint32_t(w->n), 32);
    std::vector<uint32_t> bits(words);
    IPCFP_HIP(ctx, hipMemcpyAsync(bits.data(), touched_d, size_t(words) * 4, hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    std::vector<uint32_t> ids;
    for (uint32_t wd = 0; wd < words; ++wd) {
        uint32_t m = bits[wd];
        while (m) {
            const int b = __builtin_ctz(m);
            m &= m - 1;
            ids.push_back(wd * 32 + uint32_t(b));
        }
    }
    const uint32_t n = uint32_t(ids.size());
    *n_out = n;
    if (n == 0) return IPCFP_OK;
    DevBuf<uint32_t> ids_d;
    DevBuf<CidKey> keys_d;
    IPCFP_HIP(ctx, ids_d.alloc(n));
    IPCFP_HIP(ctx, keys_d.alloc(n));
    IPCFP_HIP(ctx, hipMemcpyAsync(ids_d.p, ids.data(), size_t(n) * 4, hipMemcpyHostToDevice, ctx->stream));
    int rc = launch_gather_block_cids(ctx, w->cids.p, ids_d.p, n, keys_d.p);
    if (rc) return rc;
    std::vector<uint8_t> cids(size_t(n) * IPCFP_CID_SLOT);
    IPCFP_HIP(ctx, hipMemcpyAsync(cids.data(), keys_d.p, cids.size(), hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    std::vector<uint32_t> perm(n);
    for (uint32_t i = 0; i < n; ++i) perm[i] = i;
    // a witness may hold the same CID twice (last one wins in the index): only the indexed copy can be
    // marked, so CIDs are distinct here and the order is total
    std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
        return cid_slot_less(cids.data() + size_t(a) * IPCFP_CID_SLOT, cids.data() + size_t(b) * IPCFP_CID_SLOT);
    });
    const uint64_t take = n < cap ? n : cap;
    for (uint64_t i = 0; i < take; ++i) {
        if (ids_out) ids_out[i] = ids[perm[i]];
        if (cids_out) std::memcpy(cids_out + i * IPCFP_CID_SLOT, cids.data() + size_t(perm[i]) * IPCFP_CID_SLOT, IPCFP_CID_SLOT);
    }
    return IPCFP_OK;
}

struct StorageSpecHost {
    uint64_t actor_id;
    uint8_t slot[32];
};
struct StorageGenHost {
    uint8_t parent_state_root[40], actor_state[40], storage_root[40];
    uint8_t value[32];
    uint32_t status, pad;
};
static_assert(sizeof(StorageGenHost) == sizeof(ipcfp_generated_storage_t), "generated storage record layout");

}  // namespace

namespace {

// What `generate_event_proof` leaves behind on the DEVICE, before anything is copied out: both generator entry points
// run this and differ only in what they do with it.
struct EventGenCore {
    uint32_t status = IPCFP_ST_ERR;
    TipsetCtxDev tc;      // the host copy after the header kernel: heights, receipts root
    WideParents wide;
    DevBuf<uint32_t> touched;  // the recorder's bitmap (+ 2 flag words)
    ScanResult scan;      // scan.matches: the match records
    DevBuf<CidKey> msg;   // message CID of match i
    uint64_t nm = 0;
};

// Steps 1-4 of generate_event_proof (generator.rs:89-135), one text for the single-spec core and the bundle's one pass: the
// recorder (the bitmap + two flag words), the child header → receipts root, then parent headers, TxMeta, the message AMTs
// (recorded) and the execution order with verify_txmeta = false.  One traversal serves record_transaction_amts and
// build_execution_order: both load exactly the same blocks in the same order.
struct EventGenOrder {
    uint32_t status = IPCFP_ST_ERR;  // != TRUE: the Err of these steps (nothing else is then meaningful)
    uint32_t words = 0;              // of the bitmap
    uint32_t* oor_d = nullptr;       // flag: an exec_index is outside the execution order
    uint32_t* missing_d = nullptr;   // flag: a base CID is absent from the store
    DevBuf<TipsetCtxDev> tc_d;
    ExecState ex;
};

int event_gen_order(ipcfp_ctx* ctx, ipcfp_witness* w, const uint8_t* parent_cids40, uint32_t n_parents, const uint8_t* child_cid40,
                    DevBuf<uint32_t>& touched, TipsetCtxDev& tc, WideParents& wide, EventGenOrder& o) {
    o.status = IPCFP_ST_ERR;
    o.words = div_up(uint32_t(w->n), 32);
    IPCFP_HIP(ctx, touched.alloc(o.words + 2));
    IPCFP_HIP(ctx, hipMemsetAsync(touched.p, 0, size_t(o.words + 2) * 4, ctx->stream));
    o.oor_d = touched.p + o.words;
    o.missing_d = touched.p + o.words + 1;
    const WitnessView rec = witness_view(w, touched.p);
    // Step 1 (generator.rs:89-95): child header → receipts root.  The context kernel also loads parent 0.
    if (int rc_t = tipset_inputs_list(ctx, TC_PARENTS_PARSED | TC_CHILD_PARSED, parent_cids40, n_parents, child_cid40, tc, wide)) return rc_t;
    IPCFP_HIP(ctx, o.tc_d.alloc(1));
    IPCFP_HIP(ctx, hipMemcpyAsync(o.tc_d.p, &tc, sizeof tc, hipMemcpyHostToDevice, ctx->stream));
    int rc = launch_ctx_headers(ctx, rec, o.tc_d.p);
    if (rc) return rc;
    IPCFP_HIP(ctx, d2h_small(ctx, &tc, o.tc_d.p, sizeof tc, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    if (tc.child_status != IPCFP_ST_TRUE) {
        o.status = tc.child_status;
        return IPCFP_OK;
    }
    // Steps 2-4 (generator.rs:97-135)
    rc = build_exec_order(ctx, rec, o.tc_d.p, n_parents, o.ex, /*verify_txmeta=*/0);
    if (rc) return rc;
    o.status = o.ex.status;
    return IPCFP_OK;
}

// base witness (generator.rs:97-112): parents, child, receipts root (TxMeta CIDs were marked by the traversal).  Queued;
// base_d is read until the caller's next synchronisation.
int event_gen_mark_base(ipcfp_ctx* ctx, ipcfp_witness* w, DevBuf<uint32_t>& touched, const TipsetCtxDev& tc, const WideParents& wide,
                        uint32_t* missing_d, std::vector<CidKey>& base, DevBuf<CidKey>& base_d) {
    tipset_parent_keys(tc, wide, base);
    base.push_back(tc.child);
    base.push_back(tc.receipts_root);
    IPCFP_HIP(ctx, base_d.alloc(base.size()));
    IPCFP_HIP(ctx, hipMemcpyAsync(base_d.p, base.data(), base.size() * sizeof(CidKey), hipMemcpyHostToDevice, ctx->stream));
    return launch_mark_cids(ctx, witness_view(w, touched.p), base_d.p, uint32_t(base.size()), missing_d);
}

// Steps 1-6 of generate_event_proof and the base witness marks.  IPCFP_OK with core.status != IPCFP_ST_TRUE: the Err the
// reference's `?` surfaces first (nothing else of `core` is then meaningful).
int generate_events_core(ipcfp_ctx* ctx, ipcfp_witness* w, const uint8_t* parent_cids40, uint32_t n_parents, const uint8_t* child_cid40,
                         const ipcfp_event_filter_t* filter, int has_actor, uint64_t actor, EventGenCore& core) {
    core.status = IPCFP_ST_ERR;
    DevBuf<uint32_t>& touched = core.touched;
    TipsetCtxDev& tc = core.tc;
    EventGenOrder order;
    int rc = event_gen_order(ctx, w, parent_cids40, n_parents, child_cid40, touched, tc, core.wide, order);
    if (rc) return rc;
    if (order.status != IPCFP_ST_TRUE) {
        core.status = order.status;
        return IPCFP_OK;
    }
    ExecState& ex = order.ex;
    uint32_t* const oor_d = order.oor_d;
    // Step 5 (generator.rs:137-150): two-pass scan, recording
    ScanResult& scan = core.scan;
    rc = scan_events_device(ctx, w, tc.receipts_root, *filter, has_actor, actor, touched.p, scan);
    if (rc) return rc;
    if (scan.status != IPCFP_ST_TRUE) {
        core.status = scan.status;
        return IPCFP_OK;
    }
    // Step 6 (generator.rs:152-169): message CID of each match = exec_list[exec_index]; the records stay where they are
    const uint64_t nm = scan.n_matches;
    if (nm >= 0xffffffffULL) return set_error(ctx, IPCFP_E_UNSUPPORTED, "too many matches");
    DevBuf<CidKey> exec_list;
    DevBuf<uint64_t> exec_idx;
    if (nm) {
        IPCFP_HIP(ctx, exec_list.alloc(ex.exec_len ? ex.exec_len : 1));
        IPCFP_HIP(ctx, core.msg.alloc(nm));
        rc = launch_exec_compact(ctx, ex.keys.p, uint32_t(ex.raw_len), ex.first.p, ex.pos.p, exec_list.p);
        if (rc) return rc;
        IPCFP_HIP(ctx, exec_idx.alloc(nm));
        rc = launch_match_exec_index(ctx, scan.matches.p, uint32_t(nm), exec_idx.p);
        if (rc) return rc;
        rc = launch_gather_keys(ctx, exec_list.p, ex.exec_len, exec_idx.p, uint32_t(nm), core.msg.p, oor_d);
        if (rc) return rc;
    }
    std::vector<CidKey> base;
    DevBuf<CidKey> base_d;
    rc = event_gen_mark_base(ctx, w, touched, tc, core.wide, order.missing_d, base, base_d);
    if (rc) return rc;
    uint32_t flag[2] = {0, 0};
    IPCFP_HIP(ctx, d2h_small(ctx, flag, oor_d, 8, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));  // (also: exec_list, exec_idx and base_d are no longer read)
    if (flag[0]) {  // "Missing message at index" (generator.rs:158-160) precedes materialisation
        core.status = IPCFP_ST_ERR;
        return IPCFP_OK;
    }
    if (flag[1]) {  // must_get of a base CID fails (witness.rs:45-48)
        core.status = IPCFP_ST_ERR_MISSING_BLOCK;
        return IPCFP_OK;
    }
    core.nm = nm;
    core.status = IPCFP_ST_TRUE;
    return IPCFP_OK;
}

// generate_event_proof for ALL event specs of a bundle in one pass (src/proofs/generator.rs:58-78 runs it spec by spec):
// steps 1-4 — headers, TxMeta, message AMTs, execution order — ONCE, one recorder, one scan per ≤ IPCFP_MAX_SCAN_SPECS
// specs (host/scan_events_multi.cpp), one gather of message CIDs per scan.  What is common to every spec (a header, the
// execution order, the scan's status, a missing base CID) fails spec 0; "Missing message at index" (events/generator.rs:
// 244-246) fails exactly the specs that have a match at a receipt index beyond the execution order.
struct BundleEvents {
    uint32_t common_status = IPCFP_ST_ERR;  // != TRUE: the Err every spec's generate_event_proof surfaces first
    bool missing_base = false;              // must_get of a base CID fails (witness.rs:45-48): after a spec's own Err
    std::vector<uint8_t> spec_oor;          // spec j has a match outside the execution order
    std::vector<ipcfp_event_match_t> matches;  // scan order, chunk by chunk
    std::vector<uint32_t> match_spec;          // global spec index
    std::vector<uint8_t> msg;                  // IPCFP_CID_SLOT bytes per match
    std::vector<uint32_t> block_ids;           // the recorder's blocks, ascending ids
};

int generate_bundle_events(ipcfp_ctx* ctx, ipcfp_witness* w, const uint8_t* parent_cids40, uint32_t n_parents, const uint8_t* child_cid40,
                           const ipcfp_event_filter_t* filters, const uint8_t* has_actor, const uint64_t* actors, uint64_t n_specs,
                           BundleEvents& out) {
    IPCFP_ENTER(ctx);
    out.common_status = IPCFP_ST_ERR;
    out.spec_oor.assign(n_specs, 0);
    DevBuf<uint32_t> touched;
    TipsetCtxDev tc;
    WideParents wide;
    EventGenOrder order;
    int rc = event_gen_order(ctx, w, parent_cids40, n_parents, child_cid40, touched, tc, wide, order);
    if (rc) return rc;
    if (order.status != IPCFP_ST_TRUE) {
        out.common_status = order.status;
        return IPCFP_OK;
    }
    ExecState& ex = order.ex;
    const uint32_t words = order.words;
    DevBuf<CidKey> exec_list;
    bool have_list = false;
    // Steps 5 and 6 per chunk of specs: the scan on the one recorder, then message CID of each match = exec_list[exec_index]
    for (uint64_t first = 0; first < n_specs; first += IPCFP_MAX_SCAN_SPECS) {
        const uint32_t n_chunk = uint32_t(n_specs - first < IPCFP_MAX_SCAN_SPECS ? n_specs - first : IPCFP_MAX_SCAN_SPECS);
        MultiScanResult scan;
        rc = scan_events_multi_device(ctx, w, tc.receipts_root, filters + first, has_actor + first, actors + first, n_chunk, touched.p, scan,
                                      kAllMatches);
        if (rc) return rc;
        if (scan.status != IPCFP_ST_TRUE) {  // (the same for every chunk: a scan's status does not depend on its specs)
            out.common_status = scan.status;
            return IPCFP_OK;
        }
        const uint64_t nm = scan.n_matches;
        if (nm == 0) continue;
        if (out.matches.size() + nm >= 0xffffffffULL) return set_error(ctx, IPCFP_E_UNSUPPORTED, "too many matches");
        DevBuf<CidKey> msg_d;
        DevBuf<uint64_t> exec_idx;
        if (!have_list) {
            IPCFP_HIP(ctx, exec_list.alloc(ex.exec_len ? ex.exec_len : 1));
            rc = launch_exec_compact(ctx, ex.keys.p, uint32_t(ex.raw_len), ex.first.p, ex.pos.p, exec_list.p);
            if (rc) return rc;
            have_list = true;
        }
        IPCFP_HIP(ctx, msg_d.alloc(nm));
        IPCFP_HIP(ctx, hipMemsetAsync(msg_d.p, 0, nm * sizeof(CidKey), ctx->stream));
        IPCFP_HIP(ctx, exec_idx.alloc(nm));
        rc = launch_match_exec_index(ctx, scan.matches_p, uint32_t(nm), exec_idx.p);
        if (rc) return rc;
        rc = launch_gather_keys(ctx, exec_list.p, ex.exec_len, exec_idx.p, uint32_t(nm), msg_d.p, order.oor_d);  // (the flag is the gather's own:
        if (rc) return rc;                                                                                    //  the per-spec verdict is read off the records below)
        const size_t at = out.matches.size();
        out.matches.resize(at + nm);
        out.match_spec.resize(at + nm);
        out.msg.resize((at + nm) * IPCFP_CID_SLOT);
        IPCFP_HIP(ctx, hipMemcpyAsync(out.matches.data() + at, scan.matches_p, nm * sizeof(ipcfp_event_match_t), hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(out.match_spec.data() + at, scan.match_spec_p, nm * 4, hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(out.msg.data() + at * IPCFP_CID_SLOT, msg_d.p, nm * IPCFP_CID_SLOT, hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));  // (the chunk's device buffers go back to the pool)
        for (size_t k = at; k < at + nm; ++k) {
            out.match_spec[k] += uint32_t(first);
            if (out.matches[k].exec_index >= ex.exec_len) out.spec_oor[out.match_spec[k]] = 1;  // "Missing message at index" (:244-246)
        }
    }
    std::vector<CidKey> base;
    DevBuf<CidKey> base_d;
    rc = event_gen_mark_base(ctx, w, touched, tc, wide, order.missing_d, base, base_d);
    if (rc) return rc;
    std::vector<uint32_t> bits(words + 2);
    IPCFP_HIP(ctx, hipMemcpyAsync(bits.data(), touched.p, size_t(words + 2) * 4, hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    out.missing_base = bits[words + 1] != 0;
    for (uint32_t wd = 0; wd < words; ++wd)
        for (uint32_t m = bits[wd]; m; m &= m - 1) out.block_ids.push_back(wd * 32 + uint32_t(__builtin_ctz(m)));
    out.common_status = IPCFP_ST_TRUE;
    return IPCFP_OK;
}

// ipcfp_event_claims_from_matches_device behind its argument checks.  `plan_only`: stop behind the sizes.
struct ClaimGenPlan {
    DevBuf<uint8_t> recs;  // GenRec[n]
    DevBuf<uint64_t> sizes, prefix, scratch, total_d;
    uint64_t total = 0;
};

int claim_gen_plan(ipcfp_ctx* ctx, ipcfp_witness* w, const void* matches_d, uint32_t n, ClaimGenPlan& plan) {
    plan.total = 0;
    if (n == 0) return IPCFP_OK;
    IPCFP_HIP(ctx, plan.recs.alloc(size_t(n) * 32));
    IPCFP_HIP(ctx, plan.sizes.alloc(n));
    IPCFP_HIP(ctx, plan.prefix.alloc(n));
    IPCFP_HIP(ctx, plan.scratch.alloc(size_t(div_up(n, 1024)) + 1));
    IPCFP_HIP(ctx, plan.total_d.alloc(1));
    const int rc = launch_gen_claim_sizes(ctx, witness_view(w), matches_d, n, plan.recs.p, plan.sizes.p, plan.prefix.p, plan.total_d.p,
                                          plan.scratch.p);
    if (rc) return rc;
    IPCFP_HIP(ctx, d2h_small(ctx, &plan.total, plan.total_d.p, 8, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    if (plan.total >= 0xf0000000ULL) return set_error(ctx, IPCFP_E_UNSUPPORTED, "event_claims_from_matches: a claim blob of %llu bytes (limit 3.75 GB)",
                                                     (unsigned long long)plan.total);
    return IPCFP_OK;
}

}  // namespace

// The handle of ipcfp_generate_event_claims: claims and blob in HBM, everything else on the host.
struct ipcfp_generated_events {
    ipcfp_ctx* ctx = nullptr;
    uint64_t n = 0, blob_len = 0;
    DevBuf<ipcfp::EventClaimPacked> claims_d;
    DevBuf<uint8_t> blob_d;
    DevBuf<ipcfp_event_match_t> matches_d;
    DevBuf<CidKey> msg_d;
    // one entry per INPUT tipset (the single call: one); claim.tipset indexes `tipsets`
    std::vector<ipcfp_tipset_ref_t> tipsets;
    std::vector<std::vector<uint8_t>> more_parents;  // per tipset: the slots behind the inline form
    std::vector<ipcfp_status_t> tipset_status;
    std::vector<uint64_t> claim_off;  // n_tipsets + 1
    std::vector<uint32_t> block_ids;
    // host copies, made on first use
    bool have_host = false;
    std::vector<ipcfp_event_claim_t> claims_h;
    std::vector<uint8_t> blob_h;
    std::vector<ipcfp_event_match_t> matches_h;
    std::vector<uint8_t> msg_h;
    ipcfp_unpacked_events_t* unpacked = nullptr;
};

namespace {

// the tipsets the claims name: the keys as they were given (a folded slot stays folded).  parent_off: nullable for ONE tipset
void generated_set_tipsets(ipcfp_generated_events* g, const uint8_t* parent_cids40, const uint32_t* parent_off, uint32_t n_parents_one,
                           const uint8_t* child_cids40, uint32_t n_tipsets) {
    g->tipsets.resize(n_tipsets);
    g->more_parents.assign(n_tipsets, {});
    for (uint32_t t = 0; t < n_tipsets; ++t) {
        ipcfp_tipset_ref_t& ref = g->tipsets[t];
        const uint32_t first = parent_off ? parent_off[t] : 0u;
        const uint32_t n_parents = parent_off ? parent_off[t + 1] - first : n_parents_one;
        const uint8_t* parents = n_parents ? parent_cids40 + size_t(first) * IPCFP_CID_SLOT : nullptr;
        std::memset(&ref, 0, sizeof ref);
        ref.flags = TC_PARENTS_PARSED | TC_CHILD_PARSED;
        ref.n_parents = n_parents;
        std::memcpy(ref.child, child_cids40 + size_t(t) * IPCFP_CID_SLOT, IPCFP_CID_SLOT);
        const uint32_t n_inline = n_parents < uint32_t(IPCFP_MAX_PARENTS) ? n_parents : uint32_t(IPCFP_MAX_PARENTS);
        if (n_inline) std::memcpy(ref.parents, parents, size_t(n_inline) * IPCFP_CID_SLOT);
        if (n_parents > n_inline) {
            g->more_parents[t].assign(parents + size_t(n_inline) * IPCFP_CID_SLOT, parents + size_t(n_parents) * IPCFP_CID_SLOT);
            ref.more_parents = g->more_parents[t].data();
        }
    }
}

int generated_host_copy(ipcfp_generated_events* g) {
    if (g->have_host) return IPCFP_OK;
    ipcfp_ctx* ctx = g->ctx;
    IPCFP_ENTER(ctx);
    g->claims_h.resize(g->n);
    g->blob_h.resize(g->blob_len);
    g->matches_h.resize(g->n);
    g->msg_h.resize(g->n * IPCFP_CID_SLOT);
    if (g->n) {
        IPCFP_HIP(ctx, hipMemcpyAsync(g->claims_h.data(), g->claims_d.p, g->n * sizeof(ipcfp_event_claim_t), hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(g->matches_h.data(), g->matches_d.p, g->n * sizeof(ipcfp_event_match_t), hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(g->msg_h.data(), g->msg_d.p, g->n * IPCFP_CID_SLOT, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (g->blob_len)
        IPCFP_HIP(ctx, hipMemcpyAsync(g->blob_h.data(), g->blob_d.p, g->blob_len, hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    g->have_host = true;
    return IPCFP_OK;
}

// ---- generate_event_proof for a CHAIN of tipset pairs (ipcfp_generate_event_claims_tipsets; kernels/event_gen_tipsets.inc) ----

// host mirrors of the kernels' per-tipset records
struct GentTipsetHost {
    uint32_t slot_first, root_first, n_parents, dead;
};
struct GentFactsHost {
    CidKey receipts_root;
    long long child_height, parent0_height;
    unsigned long long err;
    uint32_t child_status, pad;
};
static_assert(sizeof(GentTipsetHost) == 16 && sizeof(GentFactsHost) == 72, "kernels/event_gen_tipsets.inc GentTipset / GentFacts");

// what the chain's arguments say, built once and read by every pass
struct GentChain {
    uint32_t T = 0, n_roots = 0, n_slots = 0;
    const uint32_t* parent_off = nullptr;
    std::vector<CidKey> parents, children;
    std::vector<uint32_t> seq_tipset;  // root number → tipset
    DevBuf<CidKey> parents_d;
    DevBuf<uint32_t> seq_tipset_d;
};

// what one pass over the chain leaves behind: statuses on the host, matches and their message CIDs on the device
struct GentPass {
    std::vector<uint32_t> status;  // per tipset: the single call's *status_out
    std::vector<GentFactsHost> facts;
    TipsetsScanResult scan;        // scan.matches_p, scan.match_off: the records of the sound tipsets end to end
    DevBuf<CidKey> msg;
    uint64_t nm = 0;
    // host memory the pass's queued copies read or write (alive until the pass's last synchronisation)
    std::vector<TipsetCtxDev> ctxs;
    std::vector<GentTipsetHost> tips;
    std::vector<uint8_t> roots40, skip;
    std::vector<CidKey> base;
    std::vector<uint32_t> base_tip, flags;
};

// One pass: prologue, the message trees, the segmented execution order, the scan, the gather, the base marks — recording
// into `touched_d`.  `dead` (nullable): tipsets that are not looked at at all; their status is taken from `dead_status`.
int gent_pass(ipcfp_ctx* ctx, ipcfp_witness* w, const GentChain& ch, const ipcfp_event_filter_t* filter, int has_actor, uint64_t actor,
              uint32_t* touched_d, const uint8_t* dead, const uint32_t* dead_status, GentPass& ps) {
    const uint32_t T = ch.T;
    const WitnessView rec = witness_view(w, touched_d);
    ps.status.assign(T, IPCFP_ST_TRUE);
    ps.facts.assign(T, GentFactsHost{});
    // ---- the chain prologue: every header, every TxMeta, every message-AMT root; ONE synchronisation ----
    ps.ctxs.assign(T, TipsetCtxDev{});
    ps.tips.resize(T);
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t first = ch.parent_off[t], P = ch.parent_off[t + 1] - first;
        TipsetCtxDev& tc = ps.ctxs[t];
        tc.flags = TC_PARENTS_PARSED | TC_CHILD_PARSED;
        tc.n_parents = P;
        tc.child = ch.children[t];
        for (uint32_t j = 0; j < P && j < uint32_t(IPCFP_MAX_PARENTS); ++j) tc.parents[j] = ch.parents[first + j];
        if (tipset_is_wide(P)) tc.parents_wide = ch.parents_d.p + first;  // (the whole key in HBM: tipset_ctx.h)
        ps.tips[t] = GentTipsetHost{2u * t + first, 2u * first, P, dead && dead[t] ? 1u : 0u};
    }
    DevBuf<TipsetCtxDev> ctxs_d;
    DevBuf<GentTipsetHost> tips_d;
    DevBuf<GentFactsHost> facts_d;
    DevBuf<AmtRootSpec> roots;
    DevBuf<unsigned long long> err_d, enum_err;
    IPCFP_HIP(ctx, ctxs_d.alloc(T));
    IPCFP_HIP(ctx, tips_d.alloc(T));
    IPCFP_HIP(ctx, facts_d.alloc(T));
    IPCFP_HIP(ctx, roots.alloc(size_t(ch.n_roots) + 1));
    IPCFP_HIP(ctx, err_d.alloc(T));
    IPCFP_HIP(ctx, enum_err.alloc(1));
    IPCFP_HIP(ctx, hipMemcpyAsync(ctxs_d.p, ps.ctxs.data(), size_t(T) * sizeof(TipsetCtxDev), hipMemcpyHostToDevice, ctx->stream));
    IPCFP_HIP(ctx, hipMemcpyAsync(tips_d.p, ps.tips.data(), size_t(T) * sizeof(GentTipsetHost), hipMemcpyHostToDevice, ctx->stream));
    IPCFP_HIP(ctx, hipMemsetAsync(err_d.p, 0xff, size_t(T) * 8, ctx->stream));
    int rc = launch_gent_prologue(ctx, rec, ctxs_d.p, tips_d.p, T, ch.n_slots, roots.p, err_d.p, facts_d.p);
    if (rc) return rc;
    IPCFP_HIP(ctx, hipMemcpyAsync(ps.facts.data(), facts_d.p, size_t(T) * sizeof(GentFactsHost), hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    for (uint32_t t = 0; t < T; ++t) {
        if (ps.tips[t].dead) ps.status[t] = dead_status[t];
        else if (ps.facts[t].child_status != IPCFP_ST_TRUE) ps.status[t] = ps.facts[t].child_status;  // generator.rs:89-95
    }
    // ---- the message trees, all together; one more round per failing tipset (as host/scan_events_tipsets.cpp) ----
    AmtEnumResult en;
    if (ch.n_roots) {
        std::vector<uint8_t> named(T, 0);
        for (uint32_t round = 0;; ++round) {
            IPCFP_HIP(ctx, hipMemsetAsync(enum_err.p, 0xff, 8, ctx->stream));
            rc = amt_enumerate(ctx, rec, roots.p, ch.n_roots, VK_CID, enum_err.p, en);
            if (rc) return rc;
            if (en.error == kNoEnumError) break;
            const uint32_t g = uint32_t(en.error >> 48);
            const uint32_t t = g < ch.n_roots ? ch.seq_tipset[g] : T;
            if (t >= T || named[t] || ps.status[t] != IPCFP_ST_TRUE || round >= T)
                return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_event_claims_tipsets: the enumerator names root %u twice", g);
            named[t] = 1;
            // the single call's word: the same failure under the tipset's own sequence number, merged with its stage 1
            const uint32_t local = g - ps.tips[t].root_first;
            const uint64_t seq = uint64_t(ps.tips[t].n_parents) + 3ull * (local / 2u) + 1ull + (local & 1u);
            const uint64_t own = (en.error & 0x0000ffffffffffffull) | ((seq & 0xffffull) << 48);
            ps.status[t] = enum_error_code(own < ps.facts[t].err ? own : ps.facts[t].err);
            rc = launch_gent_skip_roots(ctx, roots.p, ps.tips[t].root_first, ps.tips[t].root_first + 2u * ps.tips[t].n_parents);
            if (rc) return rc;
        }
    }
    for (uint32_t t = 0; t < T; ++t)
        if (ps.status[t] == IPCFP_ST_TRUE && ps.facts[t].err != kNoEnumError) ps.status[t] = enum_error_code(ps.facts[t].err);
    if (en.n_leaves >= 0xffffffffull)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_event_claims_tipsets: 2^32 - 1 or more raw message positions over the chain");
    const uint32_t n = uint32_t(en.n_leaves);
    // ---- the segmented execution order: one table, one prefix sum, the lists end to end ----
    DevBuf<CidKey> keys, list;
    DevBuf<uint32_t> tip, first, pos, first_by_root, exec_off;
    DevBuf<unsigned long long> slots;
    DevBuf<uint64_t> scratch, total;
    IPCFP_HIP(ctx, exec_off.alloc(size_t(T) + 1));
    IPCFP_HIP(ctx, first_by_root.alloc(size_t(ch.n_roots) + 1));
    IPCFP_HIP(ctx, total.alloc(1));
    IPCFP_HIP(ctx, hipMemsetAsync(total.p, 0, 8, ctx->stream));
    IPCFP_HIP(ctx, list.alloc(n ? n : 1));
    if (n) {
        const uint32_t size = exec_table_size(n);
        IPCFP_HIP(ctx, keys.alloc(n));
        IPCFP_HIP(ctx, tip.alloc(n));
        IPCFP_HIP(ctx, first.alloc(n));
        IPCFP_HIP(ctx, pos.alloc(n));
        IPCFP_HIP(ctx, slots.alloc(size));
        IPCFP_HIP(ctx, scratch.alloc(size_t(div_up(n, 1024)) + 2));
        IPCFP_HIP(ctx, hipMemsetAsync(slots.p, 0xff, size_t(size) * 8, ctx->stream));
        IPCFP_HIP(ctx, hipMemsetAsync(first.p, 0, size_t(n) * 4, ctx->stream));
        rc = launch_tipset_bounds(ctx, en.leaves.p, n, ch.n_roots, first_by_root.p);
        if (rc) return rc;
        rc = launch_gent_exec_order(ctx, rec, en.leaves.p, n, ch.seq_tipset_d.p, ch.n_roots, keys.p, tip.p, slots.p, size - 1, first.p);
        if (rc) return rc;
        rc = launch_scan_u32(ctx, first.p, n, pos.p, total.p, scratch.p);
        if (rc) return rc;
        rc = launch_exec_compact(ctx, keys.p, n, first.p, pos.p, list.p);
        if (rc) return rc;
    }
    rc = launch_gent_exec_ranges(ctx, tips_d.p, T, first_by_root.p, pos.p, total.p, n, exec_off.p);
    if (rc) return rc;
    // ---- the scan of the tipsets still sound (generator.rs:137-150), recording ----
    ps.roots40.assign(size_t(T) * IPCFP_CID_SLOT, 0);
    ps.skip.assign(T, 0);
    for (uint32_t t = 0; t < T; ++t) {
        if (ps.status[t] != IPCFP_ST_TRUE) ps.skip[t] = 1;
        else std::memcpy(ps.roots40.data() + size_t(t) * IPCFP_CID_SLOT, ps.facts[t].receipts_root.w, IPCFP_CID_SLOT);
    }
    const uint8_t has_actor8 = has_actor ? 1 : 0;
    rc = scan_events_tipsets_device(ctx, w, ps.roots40.data(), T, filter, &has_actor8, &actor, 1, touched_d, ps.scan, 0, ~0ull, ps.skip.data());
    if (rc) return rc;  // (the stream is drained)
    for (uint32_t t = 0; t < T; ++t)
        if (!ps.skip[t] && ps.scan.status[t] != IPCFP_ST_TRUE) ps.status[t] = ps.scan.status[t];
    if (ps.scan.layout.n_receipts >= 0x7fffffffull)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_event_claims_tipsets: 2^31 - 1 or more receipts over the chain");
    ps.nm = ps.scan.layout.n_matches;  // (< 2^32 - 1: the scan's layout refuses more)
    // ---- message CID of each match (generator.rs:152-169) and the base witness (:97-112) of the tipsets still sound ----
    DevBuf<uint64_t> match_off_d;
    DevBuf<uint32_t> flags_d, base_tip_d;  // flags: [0, T) outside the execution order, [T, 2T) a base CID is absent
    DevBuf<CidKey> base_d;
    IPCFP_HIP(ctx, flags_d.alloc(2 * size_t(T)));
    IPCFP_HIP(ctx, hipMemsetAsync(flags_d.p, 0, 2 * size_t(T) * 4, ctx->stream));
    if (ps.nm) {
        IPCFP_HIP(ctx, match_off_d.alloc(size_t(T) + 1));
        IPCFP_HIP(ctx, hipMemcpyAsync(match_off_d.p, ps.scan.match_off.data(), (size_t(T) + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        IPCFP_HIP(ctx, ps.msg.alloc(ps.nm));
        rc = launch_gent_gather(ctx, ps.scan.matches_p, uint32_t(ps.nm), match_off_d.p, T, exec_off.p, list.p, ps.msg.p, flags_d.p);
        if (rc) return rc;
    }
    ps.base.clear();
    ps.base_tip.clear();
    for (uint32_t t = 0; t < T; ++t) {
        if (ps.status[t] != IPCFP_ST_TRUE) continue;
        for (uint32_t j = ch.parent_off[t]; j < ch.parent_off[t + 1]; ++j) ps.base.push_back(ch.parents[j]);
        ps.base.push_back(ch.children[t]);
        ps.base.push_back(ps.facts[t].receipts_root);
        ps.base_tip.resize(ps.base.size(), t);
    }
    if (!ps.base.empty()) {
        IPCFP_HIP(ctx, base_d.alloc(ps.base.size()));
        IPCFP_HIP(ctx, base_tip_d.alloc(ps.base.size()));
        IPCFP_HIP(ctx, hipMemcpyAsync(base_d.p, ps.base.data(), ps.base.size() * sizeof(CidKey), hipMemcpyHostToDevice, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(base_tip_d.p, ps.base_tip.data(), ps.base_tip.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        rc = launch_gent_mark_base(ctx, rec, base_d.p, base_tip_d.p, uint32_t(ps.base.size()), flags_d.p + T);
        if (rc) return rc;
    }
    ps.flags.assign(2 * size_t(T), 0);
    IPCFP_HIP(ctx, hipMemcpyAsync(ps.flags.data(), flags_d.p, ps.flags.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    for (uint32_t t = 0; t < T; ++t) {
        if (ps.status[t] != IPCFP_ST_TRUE) continue;
        if (ps.flags[t]) ps.status[t] = IPCFP_ST_ERR;  // "Missing message at index" (generator.rs:158-160) precedes materialisation
        else if (ps.flags[size_t(T) + t]) ps.status[t] = IPCFP_ST_ERR_MISSING_BLOCK;  // must_get of a base CID (witness.rs:45-48)
    }
    return IPCFP_OK;
}

// The body behind the argument checks.  Pass 1 looks at every tipset and records optimistically; when a tipset failed, the
// bitmap is cleared and pass 2 runs with every failing tipset skipped, so that the recorder — ONE bitmap — ends up holding
// only what sound tipsets recorded.  A sound chain runs one pass.
int generate_events_tipsets_body(ipcfp_ctx* ctx, ipcfp_witness* w, GentChain& ch, const ipcfp_event_filter_t* filter, int has_actor,
                                 uint64_t actor, ipcfp_generated_events* g) {
    const uint32_t T = ch.T;
    const uint32_t words = div_up(uint32_t(w->n), 32);
    DevBuf<uint32_t> touched;
    IPCFP_HIP(ctx, touched.alloc(words ? words : 1));
    IPCFP_HIP(ctx, hipMemsetAsync(touched.p, 0, size_t(words) * 4, ctx->stream));
    IPCFP_HIP(ctx, ch.parents_d.alloc(ch.parents.size() ? ch.parents.size() : 1));
    IPCFP_HIP(ctx, ch.seq_tipset_d.alloc(ch.seq_tipset.size() ? ch.seq_tipset.size() : 1));
    if (!ch.parents.empty())
        IPCFP_HIP(ctx, hipMemcpyAsync(ch.parents_d.p, ch.parents.data(), ch.parents.size() * sizeof(CidKey), hipMemcpyHostToDevice, ctx->stream));
    if (!ch.seq_tipset.empty())
        IPCFP_HIP(ctx, hipMemcpyAsync(ch.seq_tipset_d.p, ch.seq_tipset.data(), ch.seq_tipset.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    std::unique_ptr<GentPass> ps(new GentPass());
    int rc = gent_pass(ctx, w, ch, filter, has_actor, actor, touched.p, nullptr, nullptr, *ps);
    if (rc) return rc;
    uint32_t failing = 0;
    for (uint32_t t = 0; t < T; ++t) failing += ps->status[t] != IPCFP_ST_TRUE;
    if (failing && failing < T) {
        std::vector<uint8_t> dead(T);
        const std::vector<uint32_t> status1 = ps->status;
        for (uint32_t t = 0; t < T; ++t) dead[t] = status1[t] != IPCFP_ST_TRUE;
        IPCFP_HIP(ctx, hipMemsetAsync(touched.p, 0, size_t(words) * 4, ctx->stream));
        ps.reset(new GentPass());
        rc = gent_pass(ctx, w, ch, filter, has_actor, actor, touched.p, dead.data(), status1.data(), *ps);
        if (rc) return rc;
        for (uint32_t t = 0; t < T; ++t)
            if (ps->status[t] != status1[t])
                return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_event_claims_tipsets: tipset %u answers %u alone and %u beside failing tipsets", t,
                                 ps->status[t], status1[t]);
    } else if (failing) {  // every tipset fails: nothing is claimed, nothing recorded
        IPCFP_HIP(ctx, hipMemsetAsync(touched.p, 0, size_t(words) * 4, ctx->stream));
        ps->nm = 0;
    }
    // ---- the layout, the lowering, the materialised witness ----
    g->tipset_status.resize(T);
    std::vector<uint64_t> n_match(T, 0);
    for (uint32_t t = 0; t < T; ++t) {
        g->tipset_status[t] = ipcfp_status_t(ps->status[t]);
        if (ps->nm) n_match[t] = ps->scan.match_off[t + 1] - ps->scan.match_off[t];
    }
    g->claim_off.assign(size_t(T) + 1, 0);
    GenTipsetsLayout lay;
    if (gen_tipsets_layout(ps->status.data(), n_match.data(), nullptr, T, g->claim_off.data(), nullptr, lay) != kGenLayoutOk)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_event_claims_tipsets: 2^32 - 1 or more matches over the chain");
    if (lay.n_claims != ps->nm) return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_event_claims_tipsets: the tipsets' claim ranges do not add up");
    const uint64_t nm = ps->nm;
    g->n = nm;
    ClaimGenPlan plan;
    rc = claim_gen_plan(ctx, w, ps->scan.matches_p, uint32_t(nm), plan);
    if (rc) return rc;
    g->blob_len = plan.total;
    DevBuf<uint64_t> claim_off_d;
    DevBuf<long long> epochs_d;
    std::vector<long long> epochs(2 * size_t(T));
    if (nm) {
        for (uint32_t t = 0; t < T; ++t) {
            epochs[t] = ps->facts[t].parent0_height;
            epochs[size_t(T) + t] = ps->facts[t].child_height;
        }
        IPCFP_HIP(ctx, g->claims_d.alloc(nm));
        IPCFP_HIP(ctx, g->blob_d.alloc(plan.total + 16));
        IPCFP_HIP(ctx, claim_off_d.alloc(size_t(T) + 1));
        IPCFP_HIP(ctx, epochs_d.alloc(2 * size_t(T)));
        IPCFP_HIP(ctx, hipMemcpyAsync(claim_off_d.p, g->claim_off.data(), (size_t(T) + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(epochs_d.p, epochs.data(), epochs.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        rc = launch_gen_claim_fill(ctx, witness_view(w), ps->scan.matches_p, ps->msg.p, uint32_t(nm), plan.recs.p, plan.prefix.p, plan.total, 0, 0,
                                   0u, g->claims_d.p, g->blob_d.p);
        if (!rc) rc = launch_gent_patch_claims(ctx, g->claims_d.p, uint32_t(nm), claim_off_d.p, T, epochs_d.p, epochs_d.p + T);
        if (rc) {
            (void)sync_stream(ctx, ctx->stream);
            return rc;
        }
    }
    uint64_t nb = 0;
    g->block_ids.resize(w->n ? w->n : 1);
    rc = materialize(ctx, w, touched.p, g->block_ids.data(), nullptr, g->block_ids.size(), &nb);  // ONE per chain; synchronises
    if (rc) {
        (void)sync_stream(ctx, ctx->stream);
        return rc;
    }
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream, true));
    g->block_ids.resize(nb);
    if (nm) {
        if (ps->scan.matches.p == ps->scan.matches_p) {
            g->matches_d.swap(ps->scan.matches);
        } else {
            IPCFP_HIP(ctx, g->matches_d.alloc(nm));
            IPCFP_HIP(ctx, hipMemcpyAsync(g->matches_d.p, ps->scan.matches_p, nm * sizeof(ipcfp_event_match_t), hipMemcpyDeviceToDevice, ctx->stream));
            IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
        }
        g->msg_d.swap(ps->msg);
    }
    return IPCFP_OK;
}

}  // namespace

extern "C" {

int ipcfp_generate_event_proofs(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* parent_cids40, uint32_t n_parents,
                                const uint8_t* child_cid40, const ipcfp_event_filter_t* filter, int has_actor,
                                uint64_t actor, ipcfp_status_t* status_out, ipcfp_event_match_t* matches,
                                uint8_t* message_cids40, uint64_t cap_proofs, uint64_t* n_proofs,
                                uint32_t* witness_block_ids, uint8_t* witness_cids40, uint64_t cap_blocks,
                                uint64_t* n_blocks) {
    if (!ctx || !w || w->ctx != ctx || !child_cid40 || !filter || !status_out || !n_proofs || !n_blocks ||
        (n_parents && !parent_cids40))
        return IPCFP_E_INVALID;
    IPCFP_ENTER(ctx);
    *n_proofs = *n_blocks = 0;
    *status_out = IPCFP_ST_ERR;
    EventGenCore core;
    int rc = generate_events_core(ctx, w, parent_cids40, n_parents, child_cid40, filter, has_actor, actor, core);
    if (rc) return rc;
    if (core.status != IPCFP_ST_TRUE) {
        *status_out = ipcfp_status_t(core.status);
        return IPCFP_OK;
    }
    const uint64_t take = core.nm < cap_proofs ? core.nm : cap_proofs;
    if (take && matches)
        IPCFP_HIP(ctx, hipMemcpyAsync(matches, core.scan.matches.p, take * sizeof(ipcfp_event_match_t), hipMemcpyDeviceToHost, ctx->stream));
    if (take && message_cids40)
        IPCFP_HIP(ctx, hipMemcpyAsync(message_cids40, core.msg.p, take * IPCFP_CID_SLOT, hipMemcpyDeviceToHost, ctx->stream));
    // Step 7 (generator.rs:171-177): materialise in BTreeSet order
    rc = materialize(ctx, w, core.touched.p, witness_block_ids, witness_cids40, cap_blocks, n_blocks);
    if (rc) return rc;
    *n_proofs = core.nm;
    *status_out = IPCFP_ST_TRUE;
    return IPCFP_OK;
}

int ipcfp_event_claims_from_matches_device(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const void* matches_d, uint64_t n,
                                           const void* message_cids40_d, int64_t parent_epoch, int64_t child_epoch,
                                           uint32_t tipset, void* claims_out_d, void* blob_out_d, uint64_t cap_blob,
                                           uint64_t* blob_len_out) {
    if (!ctx || !w || w->ctx != ctx || !blob_len_out) return IPCFP_E_INVALID;
    *blob_len_out = 0;
    IPCFP_ENTER(ctx);
    if (!blob_out_d && cap_blob) return set_error(ctx, IPCFP_E_INVALID, "event_claims_from_matches: no blob buffer but a capacity");
    if (n == 0) return IPCFP_OK;
    if (n >= 0xffffffffULL) return set_error(ctx, IPCFP_E_UNSUPPORTED, "event_claims_from_matches: batch too large");
    const bool sizing = !blob_out_d;
    if (!matches_d || (!sizing && (!message_cids40_d || !claims_out_d)))
        return set_error(ctx, IPCFP_E_INVALID, "event_claims_from_matches: null matches, message CIDs or claim buffer");
    ClaimGenPlan plan;
    int rc = claim_gen_plan(ctx, w, matches_d, uint32_t(n), plan);
    *blob_len_out = plan.total;
    if (rc) return rc;
    if (sizing) return IPCFP_OK;
    if (cap_blob < plan.total)
        return set_error(ctx, IPCFP_E_INVALID, "event_claims_from_matches: the blob is %llu bytes, the buffer holds %llu",
                         (unsigned long long)plan.total, (unsigned long long)cap_blob);
    rc = launch_gen_claim_fill(ctx, witness_view(w), matches_d, static_cast<const CidKey*>(message_cids40_d), uint32_t(n), plan.recs.p,
                               plan.prefix.p, plan.total, parent_epoch, child_epoch, tipset, claims_out_d, static_cast<uint8_t*>(blob_out_d));
    if (rc) return rc;
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream, true));
    return IPCFP_OK;
}

int ipcfp_generate_event_claims(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* parent_cids40, uint32_t n_parents,
                                const uint8_t* child_cid40, const ipcfp_event_filter_t* filter, int has_actor,
                                uint64_t actor, ipcfp_status_t* status_out, ipcfp_generated_events_t** out) {
    if (!ctx || !w || w->ctx != ctx || !child_cid40 || !filter || !status_out || !out || (n_parents && !parent_cids40))
        return IPCFP_E_INVALID;
    *out = nullptr;
    IPCFP_ENTER(ctx);
    *status_out = IPCFP_ST_ERR;
    EventGenCore core;
    int rc = generate_events_core(ctx, w, parent_cids40, n_parents, child_cid40, filter, has_actor, actor, core);
    if (rc) return rc;
    if (core.status != IPCFP_ST_TRUE) {
        *status_out = ipcfp_status_t(core.status);
        return IPCFP_OK;
    }
    std::unique_ptr<ipcfp_generated_events, void (*)(ipcfp_generated_events*)> g(new (std::nothrow) ipcfp_generated_events(),
                                                                                ipcfp_generated_events_destroy);
    if (!g) return set_error(ctx, IPCFP_E_NOMEM, "generate_event_claims: out of memory");
    g->ctx = ctx;
    g->n = core.nm;
    // the one tipset the claims name: the key as it was given (a folded slot stays folded)
    generated_set_tipsets(g.get(), parent_cids40, nullptr, n_parents, child_cid40, 1);
    g->tipset_status.assign(1, IPCFP_ST_TRUE);
    g->claim_off = {0, core.nm};
    // the lowering: sizes, prefix, then a blob of exactly that length
    ClaimGenPlan plan;
    rc = claim_gen_plan(ctx, w, core.scan.matches.p, uint32_t(core.nm), plan);
    if (rc) return rc;
    g->blob_len = plan.total;
    if (core.nm) {
        IPCFP_HIP(ctx, g->claims_d.alloc(core.nm));
        IPCFP_HIP(ctx, g->blob_d.alloc(plan.total + 16));
        rc = launch_gen_claim_fill(ctx, witness_view(w), core.scan.matches.p, core.msg.p, uint32_t(core.nm), plan.recs.p, plan.prefix.p,
                                   plan.total, core.tc.parent0_height, core.tc.child_height, 0u, g->claims_d.p, g->blob_d.p);
        if (rc) {
            (void)sync_stream(ctx, ctx->stream);
            return rc;
        }
    }
    // Step 7 (generator.rs:171-177): materialise in BTreeSet order (synchronises: the fill is done when it returns)
    uint64_t nb = 0;
    g->block_ids.resize(w->n ? w->n : 1);
    rc = materialize(ctx, w, core.touched.p, g->block_ids.data(), nullptr, g->block_ids.size(), &nb);
    if (rc) {
        (void)sync_stream(ctx, ctx->stream);
        return rc;
    }
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream, true));
    g->block_ids.resize(nb);
    g->matches_d.swap(core.scan.matches);
    g->msg_d.swap(core.msg);
    *status_out = IPCFP_ST_TRUE;
    *out = g.release();
    return IPCFP_OK;
}

int ipcfp_generate_event_claims_tipsets(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* parent_cids40, const uint32_t* parent_off,
                                        const uint8_t* child_cids40, uint32_t n_tipsets, const ipcfp_event_filter_t* filter, int has_actor,
                                        uint64_t actor, ipcfp_generated_events_t** out) {
    if (out) *out = nullptr;
    if (!ctx || !w || w->ctx != ctx || !parent_off || !child_cids40 || !filter || !out || n_tipsets == 0) return IPCFP_E_INVALID;
    IPCFP_ENTER(ctx);
    // everything the arguments alone decide, before any device work
    if (n_tipsets > IPCFP_MAX_GEN_TIPSETS)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_event_claims_tipsets: %u tipsets (at most %d)", n_tipsets, IPCFP_MAX_GEN_TIPSETS);
    uint64_t n_roots = 0;
    const int args = gen_tipsets_args(parent_off, n_tipsets, &n_roots);
    if (args == kGenArgsNotAscending) return set_error(ctx, IPCFP_E_INVALID, "generate_event_claims_tipsets: parent_off does not ascend from 0");
    if (parent_off[n_tipsets] && !parent_cids40) return set_error(ctx, IPCFP_E_INVALID, "generate_event_claims_tipsets: parent slots without parent_cids40");
    if (w->receipt_lo != 0 || w->receipt_hi != ~0ULL)  // a shard is a cut of ONE tipset
        return set_error(ctx, IPCFP_E_INVALID, "generate_event_claims_tipsets: the witness has a receipt range set");
    if (args == kGenArgsTooManyRoots)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_event_claims_tipsets: %llu message-tree roots over the chain (the enumerator orders %u)",
                         (unsigned long long)n_roots, kGenMaxRoots);
    for (uint32_t t = 0; t < n_tipsets; ++t)
        if (parent_off[t + 1] - parent_off[t] > IPCFP_MAX_PARENTS_WIDE)
            return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_event_claims_tipsets: tipset %u has a key of %u parent blocks (at most %u)", t,
                             parent_off[t + 1] - parent_off[t], unsigned(IPCFP_MAX_PARENTS_WIDE));
    GentChain ch;
    ch.T = n_tipsets;
    ch.n_roots = uint32_t(n_roots);
    ch.n_slots = 2u * n_tipsets + parent_off[n_tipsets];
    ch.parent_off = parent_off;
    ch.parents.resize(parent_off[n_tipsets]);
    ch.children.resize(n_tipsets);
    ch.seq_tipset.resize(ch.n_roots);
    for (uint32_t j = 0; j < parent_off[n_tipsets]; ++j) ch.parents[j] = key_from_slot(parent_cids40 + size_t(j) * IPCFP_CID_SLOT);
    for (uint32_t t = 0; t < n_tipsets; ++t) {
        ch.children[t] = key_from_slot(child_cids40 + size_t(t) * IPCFP_CID_SLOT);
        for (uint32_t r = 2u * parent_off[t]; r < 2u * parent_off[t + 1]; ++r) ch.seq_tipset[r] = t;
    }
    std::unique_ptr<ipcfp_generated_events, void (*)(ipcfp_generated_events*)> g(new (std::nothrow) ipcfp_generated_events(),
                                                                                ipcfp_generated_events_destroy);
    if (!g) return set_error(ctx, IPCFP_E_NOMEM, "generate_event_claims_tipsets: out of memory");
    g->ctx = ctx;
    generated_set_tipsets(g.get(), parent_cids40, parent_off, 0, child_cids40, n_tipsets);
    const int rc = generate_events_tipsets_body(ctx, w, ch, filter, has_actor, actor, g.get());
    const hipError_t e = sync_stream(ctx, ctx->stream);  // (queued work reads buffers of this frame, on every path)
    if (rc) return rc;
    IPCFP_HIP(ctx, e);
    ctl_preprime(ctx);
    *out = g.release();
    return IPCFP_OK;
}

void ipcfp_generated_events_destroy(ipcfp_generated_events_t* g) {
    if (!g) return;
    if (g->unpacked) ipcfp_unpacked_events_destroy(g->unpacked);
    delete g;
}
uint64_t ipcfp_generated_events_count(const ipcfp_generated_events_t* g) { return g ? g->n : 0; }
const ipcfp_tipset_ref_t* ipcfp_generated_events_tipset(const ipcfp_generated_events_t* g) {
    return g && !g->tipsets.empty() ? g->tipsets.data() : nullptr;
}
uint32_t ipcfp_generated_events_tipset_count(const ipcfp_generated_events_t* g) { return g ? uint32_t(g->tipsets.size()) : 0u; }
const ipcfp_tipset_ref_t* ipcfp_generated_events_tipsets(const ipcfp_generated_events_t* g, uint32_t* n) {
    if (n) *n = g ? uint32_t(g->tipsets.size()) : 0u;
    return g ? g->tipsets.data() : nullptr;
}
const ipcfp_status_t* ipcfp_generated_events_tipset_status(const ipcfp_generated_events_t* g, uint32_t* n) {
    if (n) *n = g ? uint32_t(g->tipset_status.size()) : 0u;
    return g ? g->tipset_status.data() : nullptr;
}
const uint64_t* ipcfp_generated_events_tipset_claim_off(const ipcfp_generated_events_t* g, uint32_t* n) {
    if (n) *n = g ? uint32_t(g->tipsets.size()) : 0u;  // (n_tipsets: the array holds *n + 1 offsets)
    return g ? g->claim_off.data() : nullptr;
}
const void* ipcfp_generated_events_claims_device(const ipcfp_generated_events_t* g) { return g ? g->claims_d.p : nullptr; }
const void* ipcfp_generated_events_blob_device(const ipcfp_generated_events_t* g, uint64_t* blob_len) {
    if (blob_len) *blob_len = g ? g->blob_len : 0;
    return g ? g->blob_d.p : nullptr;
}
int ipcfp_generated_events_copy(ipcfp_generated_events_t* g, ipcfp_event_claim_t* claims_out, uint8_t* blob_out, uint64_t cap_blob) {
    if (!g) return IPCFP_E_INVALID;
    if (blob_out && cap_blob < g->blob_len)
        return set_error(g->ctx, IPCFP_E_INVALID, "generated_events_copy: the blob is %llu bytes, the buffer holds %llu",
                         (unsigned long long)g->blob_len, (unsigned long long)cap_blob);
    if (const int rc = generated_host_copy(g)) return rc;
    if (claims_out && g->n) std::memcpy(claims_out, g->claims_h.data(), g->n * sizeof(ipcfp_event_claim_t));
    if (blob_out && g->blob_len) std::memcpy(blob_out, g->blob_h.data(), g->blob_len);
    return IPCFP_OK;
}
const ipcfp_event_match_t* ipcfp_generated_events_matches(ipcfp_generated_events_t* g, uint64_t* n) {
    if (n) *n = 0;
    if (!g || generated_host_copy(g)) return nullptr;
    if (n) *n = g->n;
    return g->matches_h.data();
}
const uint8_t* ipcfp_generated_events_message_cids(ipcfp_generated_events_t* g, uint64_t* n) {
    if (n) *n = 0;
    if (!g || generated_host_copy(g)) return nullptr;
    if (n) *n = g->n;
    return g->msg_h.data();
}
const uint32_t* ipcfp_generated_events_block_ids(const ipcfp_generated_events_t* g, uint64_t* n) {
    if (n) *n = g ? g->block_ids.size() : 0;
    return g ? g->block_ids.data() : nullptr;
}
int ipcfp_generated_events_proofs(ipcfp_generated_events_t* g, const ipcfp_event_proof_t** proofs, uint64_t* n, uint64_t* bad_index) {
    if (!g || !proofs || !n) return IPCFP_E_INVALID;
    *proofs = nullptr;
    *n = 0;
    if (bad_index) *bad_index = ~0ull;
    if (!g->unpacked) {
        if (const int rc = generated_host_copy(g)) return rc;
        uint64_t bad = ~0ull;
        const int rc = ipcfp_unpack_event_claims(g->tipsets.data(), g->tipsets.size(), g->claims_h.data(), g->n, g->blob_h.data(), g->blob_len, &g->unpacked, &bad);
        if (bad_index) *bad_index = bad;
        if (rc == IPCFP_E_UNSUPPORTED)
            return set_error(g->ctx, rc, "generated_events_proofs: a CID of proof %llu is longer than the %d-byte slot and the claim keeps only its fold",
                             (unsigned long long)bad, int(IPCFP_CID_SLOT));
        if (rc) return set_error(g->ctx, rc, "generated_events_proofs: claim %llu does not unpack", (unsigned long long)bad);
    }
    *proofs = ipcfp_unpacked_events_proofs(g->unpacked, n);
    return IPCFP_OK;
}

int ipcfp_generate_storage_proofs(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* child_cid40,
                                  const uint64_t* actor_ids, const uint8_t* slots32, uint64_t n,
                                  ipcfp_generated_storage_t* out, uint32_t* witness_block_ids, uint8_t* witness_cids40,
                                  uint64_t cap_blocks, uint64_t* n_blocks) {
    if (!ctx || !w || w->ctx != ctx || !child_cid40 || !n_blocks || (n && (!actor_ids || !slots32 || !out)))
        return IPCFP_E_INVALID;
    if (n >= 0xffffffffULL) return set_error(ctx, IPCFP_E_UNSUPPORTED, "batch too large");
    IPCFP_ENTER(ctx);
    *n_blocks = 0;
    if (n == 0) return IPCFP_OK;
    const uint32_t words = div_up(uint32_t(w->n), 32);
    DevBuf<uint32_t> touched;
    IPCFP_HIP(ctx, touched.alloc(words));
    IPCFP_HIP(ctx, hipMemsetAsync(touched.p, 0, size_t(words) * 4, ctx->stream));
    const WitnessView rec = witness_view(w, touched.p);
    std::vector<StorageSpecHost> specs(n);
    for (uint64_t i = 0; i < n; ++i) {
        specs[i].actor_id = actor_ids[i];
        std::memcpy(specs[i].slot, slots32 + i * 32, 32);
    }
    DevBuf<StorageSpecHost> specs_d;
    DevBuf<StorageGenHost> out_d;
    IPCFP_HIP(ctx, specs_d.alloc(n));
    IPCFP_HIP(ctx, out_d.alloc(n));
    IPCFP_HIP(ctx, hipMemcpyAsync(specs_d.p, specs.data(), n * sizeof(StorageSpecHost), hipMemcpyHostToDevice, ctx->stream));
    int rc = launch_generate_storage(ctx, rec, key_from_slot(child_cid40), specs_d.p, uint32_t(n), out_d.p);
    if (rc) return rc;
    IPCFP_HIP(ctx, hipMemcpyAsync(out, out_d.p, n * sizeof(StorageGenHost), hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    // the bundle's witness is the union over the proofs that succeeded; a failing spec aborts
    // generate_proof_bundle (src/proofs/generator.rs:42-49), which the caller sees in out[i].status
    return materialize(ctx, w, touched.p, witness_block_ids, witness_cids40, cap_blocks, n_blocks);
}

int ipcfp_generate_proof_bundle(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* parent_cids40, uint32_t n_parents,
                                const uint8_t* child_cid40, const ipcfp_storage_proof_spec_t* storage_specs,
                                uint64_t n_storage, const ipcfp_event_proof_spec_t* event_specs, uint64_t n_events,
                                ipcfp_generated_storage_t* storage_out, ipcfp_status_t* event_status,
                                ipcfp_event_match_t* matches, uint8_t* message_cids40, uint32_t* match_spec,
                                uint64_t cap_proofs, uint64_t* n_proofs, uint32_t* witness_block_ids,
                                uint8_t* witness_cids40, uint64_t cap_blocks, uint64_t* n_blocks, uint64_t* first_error) {
    if (!ctx || !w || w->ctx != ctx || !child_cid40 || !n_proofs || !n_blocks || !first_error ||
        (n_storage && (!storage_specs || !storage_out)) || (n_events && (!event_specs || !event_status)))
        return IPCFP_E_INVALID;
    *n_proofs = *n_blocks = 0;
    *first_error = ~0ULL;
    std::vector<uint32_t> all_ids;  // the union, de-duplicated below (BTreeSet<(Cid, Vec<u8>)>, generator.rs:34)
    // ---- storage specs (generator.rs:42-56) ----
    if (n_storage) {
        std::vector<uint64_t> actors(n_storage);
        std::vector<uint8_t> slots(n_storage * 32);
        for (uint64_t i = 0; i < n_storage; ++i) {
            actors[i] = storage_specs[i].actor_id;
            std::memcpy(slots.data() + 32 * i, storage_specs[i].slot, 32);
        }
        std::vector<uint32_t> ids(w->n ? w->n : 1);
        uint64_t nb = 0;
        int rc = ipcfp_generate_storage_proofs(ctx, w, child_cid40, actors.data(), slots.data(), n_storage, storage_out,
                                               ids.data(), nullptr, ids.size(), &nb);
        if (rc) return rc;
        for (uint64_t i = 0; i < n_storage; ++i)
            if (storage_out[i].status != IPCFP_ST_TRUE) {
                *first_error = i;
                return IPCFP_OK;  // `generate_storage_proof(..).await?` (generator.rs:48-49)
            }
        all_ids.assign(ids.begin(), ids.begin() + nb);
    }
    // ---- event specs (generator.rs:59-80) ----
    // One pass for all of them: one execution order, one recorder, one scan per IPCFP_MAX_SCAN_SPECS specs
    // (generate_bundle_events).  The reference stops at the first spec whose generate_event_proof fails: the specs are
    // judged in its order afterwards, from what the pass found.
    uint64_t np = 0;
    if (n_events) {
        std::vector<ipcfp_event_filter_t> filters(n_events);
        std::vector<uint8_t> has_actor(n_events);
        std::vector<uint64_t> actors(n_events);
        uint64_t n_ok = 0;  // specs whose filter could be made: a failure there is returned when the reference would reach it
        int rc_filter = IPCFP_OK;
        for (; n_ok < n_events; ++n_ok) {
            const ipcfp_event_proof_spec_t& sp = event_specs[n_ok];
            rc_filter = ipcfp_create_event_filter(ctx, sp.event_signature ? sp.event_signature : "", sp.topic_1 ? sp.topic_1 : "", &filters[n_ok]);
            if (rc_filter) break;
            has_actor[n_ok] = sp.has_actor_id_filter ? 1 : 0;
            actors[n_ok] = sp.actor_id_filter;
        }
        if (n_ok == 0) return rc_filter;
        BundleEvents ev;
        int rc = generate_bundle_events(ctx, w, parent_cids40, n_parents, child_cid40, filters.data(), has_actor.data(), actors.data(), n_ok, ev);
        if (rc) return rc;
        for (uint64_t j = 0; j < n_ok; ++j) {  // `generate_event_proof(..).await?` (generator.rs:65-74), spec by spec
            ipcfp_status_t st = IPCFP_ST_TRUE;
            if (ev.common_status != IPCFP_ST_TRUE) st = ipcfp_status_t(ev.common_status);
            else if (ev.spec_oor[j]) st = IPCFP_ST_ERR;                      // "Missing message at index" precedes materialisation
            else if (ev.missing_base) st = IPCFP_ST_ERR_MISSING_BLOCK;
            event_status[j] = st;
            if (st != IPCFP_ST_TRUE) {
                *first_error = n_storage + j;
                return IPCFP_OK;
            }
        }
        if (rc_filter) return rc_filter;
        // the reference's spec-major proof order: a stable counting partition of the scan's records by spec
        std::vector<uint64_t> start(n_events + 1, 0);
        for (uint32_t s : ev.match_spec) ++start[s + 1];
        for (uint64_t j = 0; j < n_events; ++j) start[j + 1] += start[j];
        for (size_t k = 0; k < ev.matches.size(); ++k) {
            const uint32_t j = ev.match_spec[k];
            const uint64_t at = start[j]++;
            if (at >= cap_proofs) continue;
            if (matches) matches[at] = ev.matches[k];
            if (message_cids40) std::memcpy(message_cids40 + at * IPCFP_CID_SLOT, ev.msg.data() + k * IPCFP_CID_SLOT, IPCFP_CID_SLOT);
            if (match_spec) match_spec[at] = j;
        }
        np = ev.matches.size();
        all_ids.insert(all_ids.end(), ev.block_ids.begin(), ev.block_ids.end());
    }
    *n_proofs = np;
    // ---- the union in `Cid: Ord` order, each block once (generator.rs:84-88) ----
    std::sort(all_ids.begin(), all_ids.end());
    all_ids.erase(std::unique(all_ids.begin(), all_ids.end()), all_ids.end());
    const uint32_t n = uint32_t(all_ids.size());
    *n_blocks = n;
    if (n == 0) return IPCFP_OK;
    IPCFP_ENTER(ctx);
    DevBuf<uint32_t> ids_d;
    DevBuf<CidKey> keys_d;
    IPCFP_HIP(ctx, ids_d.alloc(n));
    IPCFP_HIP(ctx, keys_d.alloc(n));
    IPCFP_HIP(ctx, hipMemcpyAsync(ids_d.p, all_ids.data(), size_t(n) * 4, hipMemcpyHostToDevice, ctx->stream));
    int rc = launch_gather_block_cids(ctx, w->cids.p, ids_d.p, n, keys_d.p);
    if (rc) return rc;
    std::vector<uint8_t> cids(size_t(n) * IPCFP_CID_SLOT);
    IPCFP_HIP(ctx, hipMemcpyAsync(cids.data(), keys_d.p, cids.size(), hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    std::vector<uint32_t> perm(n);
    for (uint32_t i = 0; i < n; ++i) perm[i] = i;
    std::sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) {
        return cid_slot_less(cids.data() + size_t(a) * IPCFP_CID_SLOT, cids.data() + size_t(b) * IPCFP_CID_SLOT);
    });
    for (uint64_t i = 0; i < n && i < cap_blocks; ++i) {
        if (witness_block_ids) witness_block_ids[i] = all_ids[perm[i]];
        if (witness_cids40) std::memcpy(witness_cids40 + i * IPCFP_CID_SLOT, cids.data() + size_t(perm[i]) * IPCFP_CID_SLOT, IPCFP_CID_SLOT);
    }
    return IPCFP_OK;
}

}  // extern "C"

// ---- generate_storage_proof finished as column claims in HBM (include/ipcfp.h; kernels/storage_claims_gen.hip) --------------

// The handle of ipcfp_generate_storage_claims*: run table, columns and status bytes in HBM, everything else on the host.
struct ipcfp_generated_storage_claims {
    ipcfp_ctx* ctx = nullptr;
    uint64_t n = 0;
    uint32_t n_runs = 0;
    DevBuf<uint8_t> runs_d, slot_d, value_d, cflags_d, status_d;
    std::vector<uint32_t> block_ids;
    // host copies, made on first use
    bool have_host = false;
    std::vector<uint8_t> runs_h, slot_h, value_h, cflags_h, status_h;
    uint64_t first_error = ~0ull;
    std::vector<ipcfp_storage_claim_t> rows_h;
    ipcfp_unpacked_storage_t* unpacked = nullptr;
    // a chain (ipcfp_generate_storage_claims_tipsets*): n = n_tipsets · n_specs claims in (tipset, spec) order; block_ids is
    // the union, tipset_ids[tipset_off[t] .. tipset_off[t + 1]) tipset t's own list.  A single-child handle is a chain of
    // one whose list IS block_ids (tipset_off stays empty).
    uint32_t n_tipsets = 1;
    uint64_t n_specs = 0;
    std::vector<uint64_t> tipset_off;
    std::vector<uint32_t> tipset_ids;
    std::vector<uint64_t> tipset_first_error;  // with the host copy
};

namespace {

int sgen_host_copy(ipcfp_generated_storage_claims* g) {
    if (g->have_host) return IPCFP_OK;
    ipcfp_ctx* ctx = g->ctx;
    IPCFP_ENTER(ctx);
    g->runs_h.resize(size_t(g->n_runs) * IPCFP_SRUN_BYTES);
    g->slot_h.resize(g->n * 32);
    g->value_h.resize(g->n * 32);
    g->cflags_h.resize(g->n);
    g->status_h.resize(g->n);
    if (g->n) {
        IPCFP_HIP(ctx, hipMemcpyAsync(g->runs_h.data(), g->runs_d.p, g->runs_h.size(), hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(g->slot_h.data(), g->slot_d.p, g->slot_h.size(), hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(g->value_h.data(), g->value_d.p, g->value_h.size(), hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(g->cflags_h.data(), g->cflags_d.p, g->cflags_h.size(), hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(g->status_h.data(), g->status_d.p, g->status_h.size(), hipMemcpyDeviceToHost, ctx->stream));
        IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    }
    g->first_error = ~0ull;
    for (uint64_t i = 0; i < g->n; ++i)
        if (g->status_h[i] != IPCFP_ST_TRUE) {
            g->first_error = i;
            break;
        }
    g->tipset_first_error.assign(g->n_tipsets, ~0ull);
    for (uint32_t t = 0; t < g->n_tipsets; ++t)
        for (uint64_t i = 0; i < g->n_specs; ++i)
            if (g->status_h[t * g->n_specs + i] != IPCFP_ST_TRUE) {
                g->tipset_first_error[t] = i;
                break;
            }
    g->have_host = true;
    return IPCFP_OK;
}

// The per-call HAMT node table and the runs of a spec list, as the single call and the chain form share them: the table is
// the verifier's, made the way verify_storage_impl makes it (same kernels, same placement: the lane kernel on the aux
// stream, the 32-lane outline of the long blocks on the K1 stream, the main stream discovering the runs and walking their
// chain meanwhile).  The guards are the last members: they drain the side streams before the buffers go back to the pool.
struct SgenPrologue {
    static constexpr uint32_t kTableKinds = HK_ACTOR_STATE | HK_VEC_U8;
    const bool tabled, side, side2;
    DevBuf<HamtNodeRec> table;
    DevBuf<uint32_t> long_list, long_count, flag, pos, run_of;
    DevBuf<uint64_t> scratch, total_d;
    uint64_t n_runs = 0;
    uint32_t n_long = 0;
    hipEvent_t outline_done = nullptr;
    StreamDrainGuard aux_guard, k1_guard;

    SgenPrologue(ipcfp_ctx* ctx, bool use_table)
        : tabled(use_table),
          side(use_table && ctx->stream_aux != ctx->stream && ctx->aux_event && ctx->main_event),
          side2(side && ctx->stream_k1 != ctx->stream && ctx->stream_k1 != ctx->stream_aux),
          aux_guard(ctx->stream_aux),
          k1_guard(ctx->stream_k1) {}

    // the table's lane kernel queued, then run discovery over the n specs: one lane per spec, the prefix sum, and the
    // number of runs with the call's one synchronisation
    int discover(ipcfp_ctx* ctx, ipcfp_witness* wit, const uint64_t* actor_d, uint32_t n) {
        int rc = IPCFP_OK;
        if (tabled) {
            IPCFP_HIP(ctx, table.alloc(wit->n));
            IPCFP_HIP(ctx, long_list.alloc(wit->n));
            IPCFP_HIP(ctx, long_count.alloc(1));
            IPCFP_HIP(ctx, hipMemsetAsync(long_count.p, 0, 4, ctx->stream));
            rc = launch_hamt_list_long(ctx, wit->k1_meta.p, uint32_t(wit->n), long_list.p, long_count.p);
            if (rc) return rc;
            if (side) {
                IPCFP_HIP(ctx, hipEventRecord(ctx->main_event, ctx->stream));
                IPCFP_HIP(ctx, hipStreamWaitEvent(ctx->stream_aux, ctx->main_event, 0));
                aux_guard.armed = true;
                hipStream_t saved = ctx->stream;
                ctx->stream = ctx->stream_aux;  // (the launcher queues on the context's stream)
                rc = launch_hamt_node_table_lane(ctx, wit->arena.p, wit->k1_meta.p, uint32_t(wit->n), kHamtOutlineMinLen, kTableKinds, table.p);
                ctx->stream = saved;
            } else {
                rc = launch_hamt_node_table_lane(ctx, wit->arena.p, wit->k1_meta.p, uint32_t(wit->n), kHamtOutlineMinLen, kTableKinds, table.p);
            }
            if (rc) return rc;
        }
        IPCFP_HIP(ctx, flag.alloc(n));
        IPCFP_HIP(ctx, pos.alloc(n));
        IPCFP_HIP(ctx, run_of.alloc(n));
        IPCFP_HIP(ctx, scratch.alloc(size_t(div_up(n, 1024)) + 2));
        IPCFP_HIP(ctx, total_d.alloc(1));
        rc = launch_sgen_run_flags(ctx, actor_d, n, flag.p);
        if (rc) return rc;
        {
            ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
            rc = launch_scan_u32(ctx, flag.p, n, pos.p, total_d.p, scratch.p);
        }
        if (rc) return rc;
        IPCFP_HIP(ctx, d2h_small(ctx, &n_runs, total_d.p, 8, ctx->stream));
        if (tabled) IPCFP_HIP(ctx, d2h_small(ctx, &n_long, long_count.p, 4, ctx->stream));
        IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
        return IPCFP_OK;
    }

    // the long blocks' records, beside the main stream where the context has the streams for it
    int outline(ipcfp_ctx* ctx, const WitnessView& plain) {
        if (n_long) {
            hipStream_t s = ctx->stream;
            if (side2) {
                s = ctx->stream_k1;
                k1_guard.armed = true;
                IPCFP_HIP(ctx, hipStreamWaitEvent(s, ctx->main_event, 0));
            } else if (ctx->stream_aux != ctx->stream && ctx->aux_event) {
                s = ctx->stream_aux;
                aux_guard.armed = true;
            }
            int rc = launch_hamt_outline_list(ctx, s, plain, table.p, long_list.p, long_count.p, n_long);
            if (!rc) rc = launch_hamt_node_table_rest(ctx, s, plain, long_list.p, long_count.p, n_long, kTableKinds, table.p);
            if (rc) return rc;
            if (s == ctx->stream_k1) {
                if (!ctx->outline_event) IPCFP_HIP(ctx, hipEventCreateWithFlags(&ctx->outline_event, hipEventDisableTiming));
                outline_done = ctx->outline_event;
                IPCFP_HIP(ctx, hipEventRecord(outline_done, s));
            }
        }
        if (aux_guard.armed) IPCFP_HIP(ctx, hipEventRecord(ctx->aux_event, ctx->stream_aux));
        return IPCFP_OK;
    }

    // run_of and every run's first_claim (runs_d: StorageRun[n_runs])
    int heads(ipcfp_ctx* ctx, uint32_t n, void* runs_d) {
        ProfileScope prof(ctx, IPCFP_K_SGEN_RUNS);
        return launch_storage_run_heads(ctx, flag.p, pos.p, n, run_of.p, runs_d);
    }

    // the table is whole behind this: the main stream is ordered behind the side kernels
    int join(ipcfp_ctx* ctx) {
        if (aux_guard.armed) IPCFP_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->aux_event, 0));
        if (outline_done) IPCFP_HIP(ctx, hipStreamWaitEvent(ctx->stream, outline_done, 0));
        aux_guard.armed = k1_guard.armed = false;
        return IPCFP_OK;
    }
};

// The specs are in HBM (actor_d, slot_d); `own_slots` (nullable): a buffer of the call's own that already holds the slot
// column and becomes the handle's, else the column is copied.
int generate_storage_claims_impl(ipcfp_ctx* ctx, ipcfp_witness* wit, const uint8_t* child_cid40, int64_t child_epoch, const uint64_t* actor_d,
                                 const uint8_t* slot_d, uint64_t n64, DevBuf<uint8_t>* own_slots, ipcfp_generated_storage_claims_t** out) {
    std::unique_ptr<ipcfp_generated_storage_claims, void (*)(ipcfp_generated_storage_claims*)> g(
        new (std::nothrow) ipcfp_generated_storage_claims(), ipcfp_generated_storage_claims_destroy);
    if (!g) return set_error(ctx, IPCFP_E_NOMEM, "generate_storage_claims: out of memory");
    g->ctx = ctx;
    g->n = g->n_specs = n64;
    if (n64 == 0) {
        g->tipset_first_error.assign(1, ~0ull);
        g->have_host = true;
        *out = g.release();
        return IPCFP_OK;
    }
    const uint32_t n = uint32_t(n64);
    const CidKey child = key_from_slot(child_cid40);
    const uint32_t words = div_up(uint32_t(wit->n), 32);
    DevBuf<uint32_t> touched;
    IPCFP_HIP(ctx, touched.alloc(words));
    IPCFP_HIP(ctx, hipMemsetAsync(touched.p, 0, size_t(words) * 4, ctx->stream));
    const WitnessView rec = witness_view(wit, touched.p);  // the recorder: every kernel below that fetches a block gets this view
    const WitnessView plain = witness_view(wit);
    // the verifier's rule (host/verify_storage.cpp): the node table pays for itself when the batch is large against the witness
    const int forced = ctx->hamt_table;
    const bool tabled = forced == 1 || (forced != 0 && n64 * 16u >= wit->n);
    if (own_slots) {
        g->slot_d.swap(*own_slots);
    } else {
        IPCFP_HIP(ctx, g->slot_d.alloc(n64 * 32));
        IPCFP_HIP(ctx, hipMemcpyAsync(g->slot_d.p, slot_d, n64 * 32, hipMemcpyDeviceToDevice, ctx->stream));
    }
    IPCFP_HIP(ctx, g->value_d.alloc(n64 * 32));
    IPCFP_HIP(ctx, g->cflags_d.alloc(n64));
    IPCFP_HIP(ctx, g->status_d.alloc(n64));
    constexpr uint32_t kUndecided = 0xfdu;
    DevBuf<StorageRun> runs;
    SgenPrologue pro(ctx, tabled);
    int rc = pro.discover(ctx, wit, actor_d, n);
    if (rc) return rc;
    const uint64_t n_runs = pro.n_runs;
    if (n_runs == 0 || n_runs > n) return set_error(ctx, IPCFP_E_INVALID, "generate_storage_claims: %llu runs of %u specs", (unsigned long long)n_runs, n);
    rc = pro.outline(ctx, plain);
    if (rc) return rc;
    g->n_runs = uint32_t(n_runs);
    IPCFP_HIP(ctx, runs.alloc(n_runs));
    IPCFP_HIP(ctx, g->runs_d.alloc(n_runs * IPCFP_SRUN_BYTES));
    rc = pro.heads(ctx, n, runs.p);
    if (rc) return rc;
    rc = launch_sgen_run_chain(ctx, rec, child, runs.p, uint32_t(n_runs), kUndecided);
    if (rc) return rc;
    rc = pro.join(ctx);
    if (rc) return rc;
    rc = launch_sgen_run_actors(ctx, rec, tabled ? pro.table.p : nullptr, actor_d, runs.p, uint32_t(n_runs), kUndecided);
    if (!rc) rc = launch_sgen_run_state(ctx, rec, runs.p, uint32_t(n_runs));
    DevBuf<uint32_t> root_children;  // block of every run's storage root, then the blocks behind its 32 links
    if (tabled) IPCFP_HIP(ctx, root_children.alloc(size_t(n_runs) * 33u));
    if (!rc)
        rc = launch_sgen_specs(ctx, rec, tabled ? pro.table.p : nullptr, g->slot_d.p, n, pro.run_of.p, runs.p, uint32_t(n_runs), root_children.p,
                               g->value_d.p, g->cflags_d.p, g->status_d.p);
    if (!rc) rc = launch_sgen_run_records(ctx, runs.p, uint32_t(n_runs), n, child, child_epoch, actor_d, g->runs_d.p);
    // the recorded blocks in BTreeSet order (synchronises: the columns are whole when it returns)
    uint64_t nb = 0;
    if (!rc) {
        g->block_ids.resize(wit->n ? wit->n : 1);
        rc = materialize(ctx, wit, touched.p, g->block_ids.data(), nullptr, g->block_ids.size(), &nb);
    }
    if (rc) {
        (void)sync_stream(ctx, ctx->stream);
        return rc;
    }
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream, true));
    g->block_ids.resize(nb);
    *out = g.release();
    return IPCFP_OK;
}

// ---- the same list of specs at every child of a chain (kernels/storage_claims_gen_tipsets.inc) --------------------------
constexpr uint64_t kMaxRecorderWords = 1ull << 28;  // n_tipsets rows of ceil(blocks / 32) words: 1 GiB

// The refusals both forms share, behind the null checks
int sgen_tipsets_refuse(ipcfp_ctx* ctx, const ipcfp_witness* wit, uint32_t n_tipsets, uint64_t n_specs) {
    if (n_tipsets > IPCFP_MAX_GEN_TIPSETS)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_storage_claims_tipsets: %u tipsets (at most %d)", n_tipsets, IPCFP_MAX_GEN_TIPSETS);
    if (n_specs >= 0xffffffffULL || uint64_t(n_tipsets) * n_specs >= 0xffffffffULL)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_storage_claims_tipsets: %u tipsets of %llu specs are too many claims", n_tipsets,
                         (unsigned long long)n_specs);
    if (n_specs && uint64_t(n_tipsets) * div_up(wit->n, 32) > kMaxRecorderWords)
        return set_error(ctx, IPCFP_E_UNSUPPORTED,
                         "generate_storage_claims_tipsets: %u recorder rows over %llu blocks exceed 2^28 words; cut the chain", n_tipsets,
                         (unsigned long long)wit->n);
    return IPCFP_OK;
}

// The specs are in HBM (actor_d, slot_d: the n_specs-entry list); children and epochs are the caller's host arrays.
int generate_storage_claims_tipsets_impl(ipcfp_ctx* ctx, ipcfp_witness* wit, const uint8_t* child_cids40, const int64_t* child_epochs,
                                         uint32_t n_tipsets, const uint64_t* actor_d, const uint8_t* slot_d, uint64_t n_specs64,
                                         ipcfp_generated_storage_claims_t** out) {
    std::unique_ptr<ipcfp_generated_storage_claims, void (*)(ipcfp_generated_storage_claims*)> g(
        new (std::nothrow) ipcfp_generated_storage_claims(), ipcfp_generated_storage_claims_destroy);
    if (!g) return set_error(ctx, IPCFP_E_NOMEM, "generate_storage_claims_tipsets: out of memory");
    const uint64_t n64 = uint64_t(n_tipsets) * n_specs64;
    g->ctx = ctx;
    g->n = n64;
    g->n_specs = n_specs64;
    g->n_tipsets = n_tipsets;
    g->tipset_off.assign(size_t(n_tipsets) + 1, 0);
    if (n64 == 0) {
        g->tipset_first_error.assign(n_tipsets, ~0ull);
        g->have_host = true;
        *out = g.release();
        return IPCFP_OK;
    }
    const uint32_t n_specs = uint32_t(n_specs64);
    const uint32_t words = div_up(wit->n, 32);
    std::vector<CidKey> children(n_tipsets);
    for (uint32_t t = 0; t < n_tipsets; ++t) children[t] = key_from_slot(child_cids40 + size_t(t) * IPCFP_CID_SLOT);
    DevBuf<CidKey> children_d;
    DevBuf<long long> epochs_d;
    DevBuf<uint32_t> rows;  // the recorder: row t is tipset t's
    IPCFP_HIP(ctx, children_d.alloc(n_tipsets));
    IPCFP_HIP(ctx, epochs_d.alloc(n_tipsets));
    IPCFP_HIP(ctx, rows.alloc(size_t(n_tipsets) * words));
    IPCFP_HIP(ctx, hipMemcpyAsync(children_d.p, children.data(), size_t(n_tipsets) * sizeof(CidKey), hipMemcpyHostToDevice, ctx->stream));
    static_assert(sizeof(long long) == sizeof(int64_t), "epochs are copied as they are");
    IPCFP_HIP(ctx, hipMemcpyAsync(epochs_d.p, child_epochs, size_t(n_tipsets) * 8, hipMemcpyHostToDevice, ctx->stream));
    IPCFP_HIP(ctx, hipMemsetAsync(rows.p, 0, size_t(n_tipsets) * words * 4, ctx->stream));
    const WitnessView rec = witness_view(wit, rows.p);  // (every kernel offsets `touched` to its lane's row)
    const WitnessView plain = witness_view(wit);
    // the single call's rule, applied to all the claims of the chain
    const int forced = ctx->hamt_table;
    const bool tabled = forced == 1 || (forced != 0 && n64 * 16u >= wit->n);
    IPCFP_HIP(ctx, g->slot_d.alloc(n64 * 32));
    IPCFP_HIP(ctx, g->value_d.alloc(n64 * 32));
    IPCFP_HIP(ctx, g->cflags_d.alloc(n64));
    IPCFP_HIP(ctx, g->status_d.alloc(n64));
    constexpr uint32_t kUndecided = 0xfdu;
    DevBuf<StorageRun> runs0, runs;
    DevBuf<uint8_t> heads;
    SgenPrologue pro(ctx, tabled);
    int rc = pro.discover(ctx, wit, actor_d, n_specs);  // the runs of the LIST: the same at every child
    if (rc) return rc;
    if (pro.n_runs == 0 || pro.n_runs > n_specs)
        return set_error(ctx, IPCFP_E_INVALID, "generate_storage_claims_tipsets: %llu runs of %u specs", (unsigned long long)pro.n_runs, n_specs);
    const uint32_t n_runs0 = uint32_t(pro.n_runs);
    const uint64_t n_runs = uint64_t(n_tipsets) * n_runs0;
    rc = pro.outline(ctx, plain);
    if (rc) return rc;
    g->n_runs = uint32_t(n_runs);
    IPCFP_HIP(ctx, runs0.alloc(n_runs0));
    IPCFP_HIP(ctx, runs.alloc(n_runs));
    IPCFP_HIP(ctx, heads.alloc(size_t(n_tipsets) * 96));
    IPCFP_HIP(ctx, g->runs_d.alloc(n_runs * IPCFP_SRUN_BYTES));
    rc = pro.heads(ctx, n_specs, runs0.p);
    if (!rc) rc = launch_sgent_runs(ctx, rec, words, children_d.p, n_tipsets, runs0.p, n_runs0, n_specs, heads.p, runs.p, kUndecided);
    if (rc) return rc;
    rc = pro.join(ctx);
    if (rc) return rc;
    const void* table = tabled ? pro.table.p : nullptr;
    rc = launch_sgent_run_actors(ctx, rec, words, table, actor_d, runs0.p, n_runs0, n_specs, n_tipsets, runs.p, kUndecided);
    DevBuf<uint32_t> root_children, uni, union_ids, mask, count, offset, ids_out;
    DevBuf<uint64_t> cut_total, cut_scratch, tipset_off_d;
    if (tabled) IPCFP_HIP(ctx, root_children.alloc(size_t(n_runs) * 33u));
    if (!rc)
        rc = launch_sgent_specs(ctx, rec, words, table, slot_d, pro.run_of.p, n_specs, n_runs0, n_tipsets, runs.p, root_children.p, g->slot_d.p,
                                g->value_d.p, g->cflags_d.p, g->status_d.p);
    if (!rc) rc = launch_sgent_run_records(ctx, runs.p, runs0.p, n_runs0, n_specs, n_tipsets, children_d.p, epochs_d.p, actor_d, g->runs_d.p);
    // the cut: the union row through materialize (its two synchronisations, its host sort), then every tipset's own list in
    // the union's order from the device
    uint64_t nb = 0;
    if (!rc) {
        IPCFP_HIP(ctx, uni.alloc(words));
        rc = launch_sgent_union(ctx, rows.p, n_tipsets, words, uni.p);
    }
    if (!rc) {
        g->block_ids.resize(wit->n ? wit->n : 1);
        rc = materialize(ctx, wit, uni.p, g->block_ids.data(), nullptr, g->block_ids.size(), &nb);
    }
    uint64_t total = 0;
    if (!rc && nb) {
        const uint32_t n_union = uint32_t(nb), chunks = n_tipsets * div_up(n_union, 32);
        IPCFP_HIP(ctx, union_ids.alloc(n_union));
        IPCFP_HIP(ctx, mask.alloc(chunks));
        IPCFP_HIP(ctx, count.alloc(chunks));
        IPCFP_HIP(ctx, offset.alloc(chunks));
        IPCFP_HIP(ctx, cut_total.alloc(1));
        IPCFP_HIP(ctx, cut_scratch.alloc(size_t(div_up(chunks, 1024)) + 2));
        IPCFP_HIP(ctx, tipset_off_d.alloc(size_t(n_tipsets) + 1));
        IPCFP_HIP(ctx, hipMemcpyAsync(union_ids.p, g->block_ids.data(), size_t(n_union) * 4, hipMemcpyHostToDevice, ctx->stream));
        rc = launch_sgent_cut_count(ctx, rows.p, n_tipsets, words, uint32_t(wit->n), union_ids.p, n_union, mask.p, count.p, offset.p, cut_total.p,
                                    cut_scratch.p);
        if (!rc) {
            IPCFP_HIP(ctx, d2h_small(ctx, &total, cut_total.p, 8, ctx->stream));
            IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
            if (total > uint64_t(n_tipsets) * n_union || total >= 0xffffffffULL)
                rc = set_error(ctx, IPCFP_E_UNSUPPORTED, "generate_storage_claims_tipsets: %llu recorded blocks over the chain",
                               (unsigned long long)total);
        }
        if (!rc) {
            IPCFP_HIP(ctx, ids_out.alloc(total ? total : 1));
            rc = launch_sgent_cut_fill(ctx, mask.p, offset.p, cut_total.p, n_tipsets, union_ids.p, n_union, total, ids_out.p, tipset_off_d.p);
        }
        if (!rc) {
            g->tipset_ids.resize(total);
            if (total) IPCFP_HIP(ctx, hipMemcpyAsync(g->tipset_ids.data(), ids_out.p, total * 4, hipMemcpyDeviceToHost, ctx->stream));
            IPCFP_HIP(ctx, hipMemcpyAsync(g->tipset_off.data(), tipset_off_d.p, (size_t(n_tipsets) + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    if (rc) {
        (void)sync_stream(ctx, ctx->stream);
        return rc;
    }
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream, true));  // the CSR's read-back is the call's drain
    g->block_ids.resize(nb);
    // the offsets came from the device: they must tile the list they index
    for (uint32_t t = 0; t < n_tipsets; ++t)
        if (g->tipset_off[t] > g->tipset_off[t + 1] || g->tipset_off[t + 1] > total)
            return set_error(ctx, IPCFP_E_INVALID, "generate_storage_claims_tipsets: the block list of tipset %u does not lie in the chain's", t);
    *out = g.release();
    return IPCFP_OK;
}

}  // namespace

extern "C" {

int ipcfp_generate_storage_claims_tipsets_device(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* child_cids40, const int64_t* child_epochs,
                                                 uint32_t n_tipsets, const void* actor_ids_d, const void* slots32_d, uint64_t n_specs,
                                                 ipcfp_generated_storage_claims_t** out) {
    if (out) *out = nullptr;
    if (!ctx || !w || w->ctx != ctx || !child_cids40 || !child_epochs || !out || n_tipsets == 0 || (n_specs && (!actor_ids_d || !slots32_d)))
        return IPCFP_E_INVALID;
    if (const int rc = sgen_tipsets_refuse(ctx, w, n_tipsets, n_specs)) return rc;
    if ((reinterpret_cast<uintptr_t>(slots32_d) & 15u) || (reinterpret_cast<uintptr_t>(actor_ids_d) & 7u))
        return set_error(ctx, IPCFP_E_INVALID,
                         "generate_storage_claims_tipsets_device: the slot column must lie on a 16-byte boundary, the actor ids on an 8-byte one");
    IPCFP_ENTER(ctx);
    const int rc = generate_storage_claims_tipsets_impl(ctx, w, child_cids40, child_epochs, n_tipsets, static_cast<const uint64_t*>(actor_ids_d),
                                                        static_cast<const uint8_t*>(slots32_d), n_specs, out);
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // (the uploads read the caller's memory)
    return rc;
}

int ipcfp_generate_storage_claims_tipsets(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* child_cids40, const int64_t* child_epochs,
                                          uint32_t n_tipsets, const uint64_t* actor_ids, const uint8_t* slots32, uint64_t n_specs,
                                          ipcfp_generated_storage_claims_t** out) {
    if (out) *out = nullptr;
    if (!ctx || !w || w->ctx != ctx || !child_cids40 || !child_epochs || !out || n_tipsets == 0 || (n_specs && (!actor_ids || !slots32)))
        return IPCFP_E_INVALID;
    if (const int rc = sgen_tipsets_refuse(ctx, w, n_tipsets, n_specs)) return rc;
    IPCFP_ENTER(ctx);
    DevBuf<uint64_t> actor_d;
    DevBuf<uint8_t> slot_d;
    if (n_specs) {
        IPCFP_HIP(ctx, actor_d.alloc(n_specs));
        IPCFP_HIP(ctx, slot_d.alloc(n_specs * 32));
        IPCFP_HIP(ctx, hipMemcpyAsync(actor_d.p, actor_ids, n_specs * 8, hipMemcpyHostToDevice, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(slot_d.p, slots32, n_specs * 32, hipMemcpyHostToDevice, ctx->stream));
    }
    const int rc = generate_storage_claims_tipsets_impl(ctx, w, child_cids40, child_epochs, n_tipsets, actor_d.p, slot_d.p, n_specs, out);
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // (the uploads read the caller's memory)
    return rc;
}

uint32_t ipcfp_generated_storage_claims_tipset_count(const ipcfp_generated_storage_claims_t* g) { return g ? g->n_tipsets : 0; }
uint64_t ipcfp_generated_storage_claims_tipset_first_error(ipcfp_generated_storage_claims_t* g, uint32_t t) {
    if (!g || t >= g->n_tipsets || sgen_host_copy(g)) return ~0ull;
    return g->tipset_first_error[t];
}
const uint32_t* ipcfp_generated_storage_claims_tipset_block_ids(const ipcfp_generated_storage_claims_t* g, uint32_t t, uint64_t* n) {
    if (n) *n = 0;
    if (!g || t >= g->n_tipsets) return nullptr;
    if (g->tipset_off.empty()) {  // a single-child handle: its one list
        if (n) *n = g->block_ids.size();
        return g->block_ids.data();
    }
    if (n) *n = g->tipset_off[t + 1] - g->tipset_off[t];
    return g->tipset_ids.data() + g->tipset_off[t];
}

int ipcfp_generate_storage_claims_device(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* child_cid40, int64_t child_epoch,
                                         const void* actor_ids_d, const void* slots32_d, uint64_t n, ipcfp_generated_storage_claims_t** out) {
    if (!ctx || !w || w->ctx != ctx || !child_cid40 || !out || (n && (!actor_ids_d || !slots32_d))) return IPCFP_E_INVALID;
    *out = nullptr;
    if (n >= 0xffffffffULL) return set_error(ctx, IPCFP_E_UNSUPPORTED, "batch too large");
    if ((reinterpret_cast<uintptr_t>(slots32_d) & 15u) || (reinterpret_cast<uintptr_t>(actor_ids_d) & 7u))
        return set_error(ctx, IPCFP_E_INVALID, "generate_storage_claims_device: the slot column must lie on a 16-byte boundary, the actor ids on an 8-byte one");
    IPCFP_ENTER(ctx);
    return generate_storage_claims_impl(ctx, w, child_cid40, child_epoch, static_cast<const uint64_t*>(actor_ids_d),
                                        static_cast<const uint8_t*>(slots32_d), n, nullptr, out);
}

int ipcfp_generate_storage_claims(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const uint8_t* child_cid40, int64_t child_epoch,
                                  const uint64_t* actor_ids, const uint8_t* slots32, uint64_t n, ipcfp_generated_storage_claims_t** out) {
    if (!ctx || !w || w->ctx != ctx || !child_cid40 || !out || (n && (!actor_ids || !slots32))) return IPCFP_E_INVALID;
    *out = nullptr;
    if (n >= 0xffffffffULL) return set_error(ctx, IPCFP_E_UNSUPPORTED, "batch too large");
    IPCFP_ENTER(ctx);
    DevBuf<uint64_t> actor_d;
    DevBuf<uint8_t> slot_d;
    if (n) {
        IPCFP_HIP(ctx, actor_d.alloc(n));
        IPCFP_HIP(ctx, slot_d.alloc(n * 32));
        IPCFP_HIP(ctx, hipMemcpyAsync(actor_d.p, actor_ids, n * 8, hipMemcpyHostToDevice, ctx->stream));
        IPCFP_HIP(ctx, hipMemcpyAsync(slot_d.p, slots32, n * 32, hipMemcpyHostToDevice, ctx->stream));
    }
    const uint8_t* slots_p = slot_d.p;
    const int rc = generate_storage_claims_impl(ctx, w, child_cid40, child_epoch, actor_d.p, slots_p, n, n ? &slot_d : nullptr, out);
    if (rc) (void)hipStreamSynchronize(ctx->stream);  // (the uploads read the caller's memory)
    return rc;
}

void ipcfp_generated_storage_claims_destroy(ipcfp_generated_storage_claims_t* g) {
    if (!g) return;
    if (g->unpacked) ipcfp_unpacked_storage_destroy(g->unpacked);
    delete g;
}
uint64_t ipcfp_generated_storage_claims_count(const ipcfp_generated_storage_claims_t* g) { return g ? g->n : 0; }
uint32_t ipcfp_generated_storage_claims_run_count(const ipcfp_generated_storage_claims_t* g) { return g ? g->n_runs : 0; }
const void* ipcfp_generated_storage_claims_runs_device(const ipcfp_generated_storage_claims_t* g) { return g ? g->runs_d.p : nullptr; }
const void* ipcfp_generated_storage_claims_slots_device(const ipcfp_generated_storage_claims_t* g) { return g ? g->slot_d.p : nullptr; }
const void* ipcfp_generated_storage_claims_values_device(const ipcfp_generated_storage_claims_t* g) { return g ? g->value_d.p : nullptr; }
const void* ipcfp_generated_storage_claims_cflags_device(const ipcfp_generated_storage_claims_t* g) { return g ? g->cflags_d.p : nullptr; }
const void* ipcfp_generated_storage_claims_status_device(const ipcfp_generated_storage_claims_t* g) { return g ? g->status_d.p : nullptr; }
const uint8_t* ipcfp_generated_storage_claims_status(ipcfp_generated_storage_claims_t* g, uint64_t* n) {
    if (n) *n = 0;
    if (!g || sgen_host_copy(g)) return nullptr;
    if (n) *n = g->n;
    return g->status_h.data();
}
uint64_t ipcfp_generated_storage_claims_first_error(ipcfp_generated_storage_claims_t* g) {
    if (!g || sgen_host_copy(g)) return ~0ull;
    return g->first_error;
}
int ipcfp_generated_storage_claims_copy(ipcfp_generated_storage_claims_t* g, uint8_t* runs_out, uint8_t* slots_out, uint8_t* values_out,
                                        uint8_t* cflags_out) {
    if (!g) return IPCFP_E_INVALID;
    if (const int rc = sgen_host_copy(g)) return rc;
    if (runs_out && !g->runs_h.empty()) std::memcpy(runs_out, g->runs_h.data(), g->runs_h.size());
    if (slots_out && g->n) std::memcpy(slots_out, g->slot_h.data(), g->slot_h.size());
    if (values_out && g->n) std::memcpy(values_out, g->value_h.data(), g->value_h.size());
    if (cflags_out && g->n) std::memcpy(cflags_out, g->cflags_h.data(), g->cflags_h.size());
    return IPCFP_OK;
}
const uint32_t* ipcfp_generated_storage_claims_block_ids(const ipcfp_generated_storage_claims_t* g, uint64_t* n) {
    if (n) *n = g ? g->block_ids.size() : 0;
    return g ? g->block_ids.data() : nullptr;
}
int ipcfp_generated_storage_claims_proofs(ipcfp_generated_storage_claims_t* g, const ipcfp_storage_proof_t** proofs, uint64_t* n,
                                          uint64_t* bad_index) {
    if (!g || !proofs || !n) return IPCFP_E_INVALID;
    *proofs = nullptr;
    *n = 0;
    if (bad_index) *bad_index = ~0ull;
    if (!g->unpacked) {
        if (const int rc = sgen_host_copy(g)) return rc;
        if (g->first_error != ~0ull) {  // `generate_storage_proof(..).await?` (generator.rs:48-49): there is no bundle
            if (bad_index) *bad_index = g->first_error;
            return set_error(g->ctx, IPCFP_E_INVALID, "generated_storage_claims_proofs: spec %llu failed with status %u",
                             (unsigned long long)g->first_error, unsigned(g->status_h[g->first_error]));
        }
        // the host copy expanded to rows (ipcfp_expand_storage_claims' loop over a form this file made itself)
        try {
            g->rows_h.resize(g->n);
        } catch (...) {
            return set_error(g->ctx, IPCFP_E_NOMEM, "generated_storage_claims_proofs: out of memory");
        }
        for (uint32_t r = 0; r < g->n_runs; ++r) {
            const uint8_t* rec = g->runs_h.data() + size_t(r) * IPCFP_SRUN_BYTES;
            uint32_t tail[4];
            std::memcpy(tail, rec + IPCFP_SRUN_OFF_FIRST_CLAIM, sizeof tail);
            if (uint64_t(tail[0]) + tail[1] > g->n) return set_error(g->ctx, IPCFP_E_INVALID, "generated_storage_claims_proofs: run %u does not lie in the batch", r);
            for (uint64_t i = tail[0], e = uint64_t(tail[0]) + tail[1]; i < e; ++i) {
                ipcfp_storage_claim_t& c = g->rows_h[i];
                std::memcpy(&c, rec, IPCFP_SRUN_OFF_FIRST_CLAIM);
                std::memcpy(c.slot, g->slot_h.data() + 32 * i, 32);
                std::memcpy(c.value, g->value_h.data() + 32 * i, 32);
                c.flags = tail[2] | g->cflags_h[i];
                c.reserved = tail[3];
            }
        }
        uint64_t bad = ~0ull;
        const int rc = ipcfp_unpack_storage_claims(g->rows_h.data(), g->n, &g->unpacked, &bad);
        if (bad_index) *bad_index = bad;
        if (rc == IPCFP_E_UNSUPPORTED)
            return set_error(g->ctx, rc, "generated_storage_claims_proofs: a CID of proof %llu is longer than the %d-byte slot and the claim keeps only its fold",
                             (unsigned long long)bad, int(IPCFP_CID_SLOT));
        if (rc) return set_error(g->ctx, rc, "generated_storage_claims_proofs: claim %llu does not unpack", (unsigned long long)bad);
    }
    *proofs = ipcfp_unpacked_storage_proofs(g->unpacked, n);
    return IPCFP_OK;
}

}  // extern "C"
