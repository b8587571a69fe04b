// csrc/host/bundle_write_packed.cpp — the bundle wire format, WRITE direction, from packed claims resident in HBM:
// `serde_json::to_string(&UnifiedProofBundle)` (src/proofs/common/bundle.rs:39-45) of what `generate_proof_bundle` collects
// (src/proofs/generator.rs) where the claims never existed as host strings.  bundle_write.cpp writes the claims head on the
// host out of C strings; here it is written by kernels/claim_text.hip into the SAME device text buffer the block writer
// (kernels/base64_encode.hip) fills behind it, and one copy brings head, blocks and `]}` back.
//
// The text and the refusals are those of the host route, ipcfp_unpack_storage_claims(ipcfp_expand_storage_claims(..)) and
// ipcfp_unpack_event_claims(..) handed to ipcfp_bundle_write_json.
//
// The per-tipset part of an EventProof's text, "parent_tipset_cids":[…],"child_block_cid":"…", is rendered HERE, with
// cidstr.cpp, and uploaded: the tipset table is host memory by the ABI, a chain has a handful of tipsets, and their slots
// would have to cross PCIe either way — as text they cross once and the device renders nothing per tipset.
#include <cstring>
#include <string>
#include <vector>

#include "../common.h"
#include "../kernels/claim_text_dev.h"
#include "../kernels/launch.h"
#include "cidstr.h"

using namespace ipcfp;

namespace {

struct TipsetRec {  // kernels/claim_text.hip TipsetFrag
    uint64_t off;
    uint32_t len;
    uint32_t code;
};
static_assert(sizeof(TipsetRec) == kClaimTextTipsetRec, "tipset fragment record");
constexpr uint32_t kTipsetBad = 7, kTipsetFold = 8;  // claim_text.hip kCtTipsetBad / kCtTipsetFold

// what ipcfp_unpack_event_claims' first pass decides for every tipset, and the text of those that have one
void render_tipsets(const ipcfp_tipset_ref_t* tipsets, uint32_t n_tipsets, std::vector<TipsetRec>& recs, std::string& text) {
    recs.assign(n_tipsets, TipsetRec{0, 0, 0});
    for (uint32_t k = 0; k < n_tipsets; ++k) {
        const ipcfp_tipset_ref_t& tr = tipsets[k];
        TipsetRec& r = recs[k];
        const uint32_t both = IPCFP_TIPSET_PARENTS_PARSED | IPCFP_TIPSET_CHILD_PARSED;
        if ((tr.flags & both) != both || tr.n_parents > uint32_t(IPCFP_MAX_PARENTS_WIDE) ||
            (tr.n_parents > uint32_t(IPCFP_MAX_PARENTS) && !tr.more_parents)) {
            r.code = kTipsetBad;
            continue;
        }
        const size_t start = text.size();
        auto put = [&](const uint8_t* slot) {
            const int len = claimtext::slot_cid_len(slot);
            if (len < 0) r.code = kTipsetFold;
            else if (len == 0) r.code = kTipsetBad;
            else text += '"' + cid_to_string(slot, size_t(len)) + '"';
        };
        text += "\"parent_tipset_cids\":[";
        for (uint32_t j = 0; j < tr.n_parents && !r.code; ++j) {
            if (j) text += ',';
            put(j < uint32_t(IPCFP_MAX_PARENTS) ? tr.parents[j] : tr.more_parents + size_t(j - IPCFP_MAX_PARENTS) * IPCFP_CID_SLOT);
        }
        text += "],\"child_block_cid\":";
        if (!r.code) put(tr.child);
        if (r.code) {
            text.resize(start);
            continue;
        }
        r.off = start;
        r.len = uint32_t(text.size() - start);
    }
}

int refuse(ipcfp_ctx* ctx, int rc, int kind, uint64_t index, int* bad_kind, uint64_t* bad_index, const char* what) {
    if (bad_kind) *bad_kind = kind;
    if (bad_index) *bad_index = index;
    static const char* const names[3] = {"storage claim", "event claim", "block_ids"};
    if (index == ~0ull) return set_error(ctx, rc, "bundle_write_packed_json: %s", what);
    return set_error(ctx, rc, "bundle_write_packed_json: %s[%llu]: %s", names[kind], (unsigned long long)index, what);
}

const char* code_text(uint32_t code) {
    switch (code) {
        case 1: return "the run's flags are not IPCFP_SRUN_FLAG_MASK or its reserved word is not 0";
        case 2: return "the cflags byte is not IPCFP_SCOL_FLAG_MASK";
        case 3: return "a CID slot of the run is not one well-formed CID";
        case 4: return "a CID of the run is longer than the slot and only its fold is kept";
        case 5: return "the tipset index is outside the tipset table";
        case 6: return "IPCFP_CLAIM_MSG_PARSED | IPCFP_CLAIM_DATA_MATCHABLE are not both set";
        case 7: return "the tipset it names has no string form (parsed flags, key length or a malformed CID slot)";
        case 8: return "the tipset it names holds a CID longer than the slot, of which only the fold is kept";
        case 9: return "topics or data leave the blob";
        case 10: return "the message CID slot is not one well-formed CID";
        case 11: return "the message CID is longer than the slot and only its fold is kept";
        default: return "a topic's flag byte is 0";
    }
}

}  // namespace

extern "C" {

int ipcfp_bundle_write_packed_json(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const void* runs_d, uint32_t n_runs, const void* slot_d,
                                   const void* value_d, const void* cflags_d, uint64_t n_storage, const ipcfp_tipset_ref_t* tipsets,
                                   uint32_t n_tipsets, const void* claims_d, uint64_t n_events, const void* blob_d, uint64_t blob_len,
                                   const uint32_t* block_ids, uint64_t n_blocks, char* out, uint64_t cap, uint64_t* len, int* bad_kind,
                                   uint64_t* bad_index) {
    if (bad_kind) *bad_kind = -1;
    if (bad_index) *bad_index = ~0ull;
    if (!ctx || !w || !len || w->ctx != ctx) return IPCFP_E_INVALID;
    *len = 0;
    IPCFP_ENTER(ctx);
    if (!out && cap) return set_error(ctx, IPCFP_E_INVALID, "bundle_write_packed_json: null output with a capacity");
    if (n_storage + n_events >= 0xfffffffcull || n_storage >= 0xfffffffcull || n_events >= 0xfffffffcull)
        return set_error(ctx, IPCFP_E_UNSUPPORTED, "bundle_write_packed_json: 2^32 - 4 claims or more");
    if (n_storage && (!runs_d || !slot_d || !value_d || !cflags_d))
        return set_error(ctx, IPCFP_E_INVALID, "bundle_write_packed_json: null storage column");
    if ((reinterpret_cast<uintptr_t>(runs_d) | reinterpret_cast<uintptr_t>(slot_d) | reinterpret_cast<uintptr_t>(value_d)) & 15u)
        return set_error(ctx, IPCFP_E_INVALID, "bundle_write_packed_json: the run table and the slot / value columns must lie on 16-byte boundaries");
    if ((n_events && !claims_d) || (n_tipsets && !tipsets) || (blob_len && !blob_d))
        return set_error(ctx, IPCFP_E_INVALID, "bundle_write_packed_json: null tipset table, claim array or blob");
    if (reinterpret_cast<uintptr_t>(claims_d) & 7u)
        return set_error(ctx, IPCFP_E_INVALID, "bundle_write_packed_json: claims_d must lie on an 8-byte boundary");
    if (!block_ids && n_blocks != w->n)
        return set_error(ctx, IPCFP_E_INVALID, "bundle_write_packed_json: block_ids is null but n_blocks (%llu) is not the witness's block count (%llu)",
                         (unsigned long long)n_blocks, (unsigned long long)w->n);
    if (n_blocks >= 0xffffffffull) return set_error(ctx, IPCFP_E_UNSUPPORTED, "more than 2^32-2 blocks");
    // every run holds a claim: more runs than claims (or none for some claims) cannot tile [0, n)
    if (n_runs > n_storage || (n_storage && !n_runs))
        return refuse(ctx, IPCFP_E_INVALID, 0, ~0ull, bad_kind, bad_index, "the run table does not tile the storage claims");
    const uint32_t n = uint32_t(n_blocks), ns = uint32_t(n_storage), ne = uint32_t(n_events);
    const uint32_t n_items = ns + ne + 3u;

    // 1. the tipsets' text (host) and its upload
    std::vector<TipsetRec> recs;
    std::string ttext;
    try {
        if (ne) render_tipsets(tipsets, n_tipsets, recs, ttext);
    } catch (...) {
        return set_error(ctx, IPCFP_E_NOMEM, "bundle_write_packed_json: out of memory while rendering the tipsets");
    }
    DevBuf<uint8_t> trecs_d, ttext_d, run_frag_d, run_info_d, text_d;
    DevBuf<uint32_t> run_of_d, ids_d, units_d, unit0_d;
    DevBuf<uint64_t> csize_d, coff_d, cscratch_d, word_d, pos_d, size_d, text_off_d, scratch_d, res_d;
    if (!recs.empty()) {
        IPCFP_HIP(ctx, trecs_d.alloc(recs.size() * sizeof(TipsetRec)));
        if (int rc = upload(ctx, trecs_d.p, recs.data(), recs.size() * sizeof(TipsetRec), ctx->stream)) return rc;
    }
    if (!ttext.empty()) {
        IPCFP_HIP(ctx, ttext_d.alloc(ttext.size()));
        if (int rc = upload(ctx, ttext_d.p, ttext.data(), ttext.size(), ctx->stream)) return rc;
    }

    // 2. runs, per-run fragments, sizes of the head's items and their prefix sums
    ClaimTextIn in{};
    in.cols = StorageColumnsDev{runs_d, n_runs, static_cast<const uint8_t*>(slot_d), static_cast<const uint8_t*>(value_d),
                                static_cast<const uint8_t*>(cflags_d)};
    in.n_storage = ns;
    in.claims_d = claims_d;
    in.n_events = ne;
    in.blob_d = static_cast<const uint8_t*>(blob_d);
    in.blob_len = blob_len;
    in.tipsets_d = trecs_d.p;
    in.tipset_frag_d = ttext_d.p;
    in.n_tipsets = ne ? n_tipsets : 0u;
    // words: [0] first refusal, [1] head length, [2] run table verdict (low 32 bits)
    IPCFP_HIP(ctx, word_d.alloc(3));
    IPCFP_HIP(ctx, hipMemsetAsync(word_d.p, 0xff, 8, ctx->stream));
    IPCFP_HIP(ctx, hipMemsetAsync(word_d.p + 1, 0, 16, ctx->stream));
    if (ns) {
        IPCFP_HIP(ctx, run_of_d.alloc(ns));
        IPCFP_HIP(ctx, run_info_d.alloc(size_t(n_runs) * kClaimTextRunInfo));
        IPCFP_HIP(ctx, run_frag_d.alloc(size_t(n_runs) * kClaimTextRunFragStride));
        IPCFP_HIP(ctx, hipMemsetAsync(run_of_d.p, 0xff, size_t(ns) * 4, ctx->stream));
        if (int rc = launch_storage_column_runs(ctx, in.cols, ns, run_of_d.p, nullptr, reinterpret_cast<uint32_t*>(word_d.p + 2))) {
            (void)sync_stream(ctx, ctx->stream);
            return rc;
        }
        in.run_of_d = run_of_d.p;
        in.run_info_d = run_info_d.p;
        in.run_frag_d = run_frag_d.p;
    }
    IPCFP_HIP(ctx, csize_d.alloc(n_items));
    IPCFP_HIP(ctx, coff_d.alloc(n_items));
    IPCFP_HIP(ctx, cscratch_d.alloc(size_t(div_up(n_items, 1024)) + 1));
    if (int rc = launch_claim_text_sizes(ctx, in, csize_d.p, coff_d.p, word_d.p + 1, cscratch_d.p,
                                         reinterpret_cast<unsigned long long*>(word_d.p))) {
        (void)sync_stream(ctx, ctx->stream);
        return rc;
    }

    // 3. sizes of the block part (bundle_write.cpp steps 2-4), then ONE synchronisation for every size and error word
    uint64_t res[3] = {~0ull, 0, 0};  // first error, text bytes, units
    uint64_t word[3] = {~0ull, 0, 0};
    if (n) {
        if (block_ids) {
            IPCFP_HIP(ctx, ids_d.alloc(n));
            IPCFP_HIP(ctx, hipMemcpyAsync(ids_d.p, block_ids, size_t(n) * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        IPCFP_HIP(ctx, units_d.alloc(n));
        IPCFP_HIP(ctx, unit0_d.alloc(n));
        IPCFP_HIP(ctx, pos_d.alloc(size_t(n) * 2));
        IPCFP_HIP(ctx, size_d.alloc(n));
        IPCFP_HIP(ctx, text_off_d.alloc(n));
        IPCFP_HIP(ctx, scratch_d.alloc(2 * (size_t(div_up(n, 1024)) + 1)));
        IPCFP_HIP(ctx, res_d.alloc(3));
        IPCFP_HIP(ctx, hipMemsetAsync(res_d.p, 0xff, 8, ctx->stream));
        const int rc = launch_bundle_block_sizes(ctx, ids_d.p, n, uint32_t(w->n), w->off.p, w->len.p, w->cids.p, pos_d.p, size_d.p,
                                                 units_d.p, text_off_d.p, unit0_d.p, res_d.p + 1, scratch_d.p,
                                                 reinterpret_cast<unsigned long long*>(res_d.p));
        if (rc) {
            (void)sync_stream(ctx, ctx->stream);
            return rc;
        }
        IPCFP_HIP(ctx, d2h_small(ctx, res, res_d.p, sizeof res, ctx->stream));
    }
    IPCFP_HIP(ctx, d2h_small(ctx, word, word_d.p, sizeof word, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));

    // 4. the refusals in text order: storage, events, blocks
    if (uint32_t(word[2]))
        return refuse(ctx, IPCFP_E_INVALID, 0, ~0ull, bad_kind, bad_index, "the run table does not tile the storage claims");
    if (word[0] != ~0ull) {
        const uint32_t code = uint32_t(word[0] & 15u);
        const int rc = (code == 4 || code == 8 || code == 11) ? IPCFP_E_UNSUPPORTED : IPCFP_E_INVALID;
        return refuse(ctx, rc, int(word[0] >> 36), (word[0] >> 4) & 0xffffffffull, bad_kind, bad_index, code_text(code));
    }
    if (res[0] != ~0ull) {
        const uint32_t code = uint32_t(res[0] & 3u);
        return refuse(ctx, code == 2 ? IPCFP_E_UNSUPPORTED : IPCFP_E_INVALID, 2, res[0] >> 2, bad_kind, bad_index,
                      code == 1   ? "not a block of the witness"
                      : code == 2 ? "the CID of this block is longer than the slot and the witness keeps only its fold"
                                  : "the witness's CID slot is not one well-formed CID");
    }
    if (res[2] >= 0xfffffff0ull) return set_error(ctx, IPCFP_E_UNSUPPORTED, "bundle_write_packed_json: more than 2^32 base64 units (48 GB of blocks)");
    const uint64_t head_len = word[1], blocks_len = res[1];
    if (head_len >= (1ull << 40)) return set_error(ctx, IPCFP_E_UNSUPPORTED, "bundle_write_packed_json: a claims head of 1 TB or more");
    *len = head_len + blocks_len + 2;
    if (!out) return IPCFP_OK;  // the sizing call
    if (cap < *len)
        return set_error(ctx, IPCFP_E_INVALID, "bundle_write_packed_json: the text is %llu bytes, the buffer holds %llu",
                         (unsigned long long)*len, (unsigned long long)cap);

    // 5. the text: head, blocks and the tail in one device buffer
    IPCFP_HIP(ctx, text_d.alloc(*len + 64));
    int rc = launch_claim_text_write(ctx, in, coff_d.p, head_len, text_d.p);
    if (!rc && blocks_len)
        rc = launch_bundle_write_text(ctx, ids_d.p, n, w->arena.p, w->cids.p, pos_d.p, text_off_d.p, unit0_d.p, uint32_t(res[2]),
                                      text_d.p + head_len);
    if (rc) {
        (void)sync_stream(ctx, ctx->stream);
        return rc;
    }
    IPCFP_HIP(ctx, hipMemsetAsync(text_d.p + head_len + blocks_len, ']', 1, ctx->stream));
    IPCFP_HIP(ctx, hipMemsetAsync(text_d.p + head_len + blocks_len + 1, '}', 1, ctx->stream));
    // 6. one blocking copy
    const hipError_t e = hipMemcpyAsync(out, text_d.p, *len, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = sync_stream(ctx, ctx->stream, true);
    IPCFP_HIP(ctx, e);
    IPCFP_HIP(ctx, e2);
    return IPCFP_OK;
}

int ipcfp_bundle_write_generated_json(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, ipcfp_generated_storage_claims_t* gs,
                                      ipcfp_generated_events_t* ge, const uint32_t* block_ids, uint64_t n_blocks, char* out, uint64_t cap,
                                      uint64_t* len, int* bad_kind, uint64_t* bad_index) {
    uint32_t n_tipsets = 0;
    uint64_t blob_len = 0;
    const ipcfp_tipset_ref_t* tipsets = ge ? ipcfp_generated_events_tipsets(ge, &n_tipsets) : nullptr;
    const void* blob_d = ge ? ipcfp_generated_events_blob_device(ge, &blob_len) : nullptr;
    return ipcfp_bundle_write_packed_json(
        ctx, w, gs ? ipcfp_generated_storage_claims_runs_device(gs) : nullptr, gs ? ipcfp_generated_storage_claims_run_count(gs) : 0u,
        gs ? ipcfp_generated_storage_claims_slots_device(gs) : nullptr, gs ? ipcfp_generated_storage_claims_values_device(gs) : nullptr,
        gs ? ipcfp_generated_storage_claims_cflags_device(gs) : nullptr, gs ? ipcfp_generated_storage_claims_count(gs) : 0ull, tipsets,
        n_tipsets, ge ? ipcfp_generated_events_claims_device(ge) : nullptr, ge ? ipcfp_generated_events_count(ge) : 0ull, blob_d, blob_len,
        block_ids, n_blocks, out, cap, len, bad_kind, bad_index);
}

}  // extern "C"
