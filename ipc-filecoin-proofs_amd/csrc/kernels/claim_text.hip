// csrc/kernels/claim_text.hip — packed claims resident in HBM → the claims head of a bundle's JSON text,
//     {"storage_proofs":[ … ],"event_proofs":[ … ],"blocks":[
// as `serde_json::to_string(&UnifiedProofBundle)` writes it (src/proofs/common/bundle.rs:39-45; StorageProof:
// src/proofs/storage/bundle.rs:5-14, EventProof / EventData: src/proofs/events/bundle.rs:5-23), into the text buffer whose
// `blocks` part kernels/base64_encode.hip fills.  Every character is a function of the packed fields (claim_text_dev.h).
//
// The text is a list of ITEMS: the three literals above and one item per claim (its separating comma in front).
//
//   k_claim_run_frags    one lane per storage RUN: the run's flags and four CID slots judged once, and the part of a
//                        StorageProof's text that is the same for every claim of the run rendered once:
//                            {"child_epoch":…,"child_block_cid":"…", … ,"storage_root":"…","slot":"0x
//   (per tipset)         the part of an EventProof's text that is the same for every claim of a tipset,
//                            "parent_tipset_cids":[…],"child_block_cid":"…"
//                        arrives rendered (host/bundle_write_packed.cpp: the tipset table is host memory by the ABI)
//   k_claim_text_sizes   one lane per item: the checks of the host route (host/unpack_claims.cpp, in its order) and the exact
//                        text length; the first refusal by one atomicMin over kind ‖ index ‖ code
//   (launch_scan_u64)    64-bit text offsets
//   k_claim_text_write   one lane per 16 BYTES OF OUTPUT (DESIGN.md §21's form): a wavefront stores 1 KB of contiguous,
//                        aligned text whatever the items are, so no lane's work grows with a claim's data_len — the hex body
//                        of a 64 KB event is 8 K lanes.  A lane finds its item by a wave-uniform binary search over the
//                        offsets and walks forward, as k_base64_encode does.
#include <hip/hip_runtime.h>

#include "../common.h"
#include "claim_text_dev.h"
#include "claims_dev.h"
#include "launch.h"
#include "storage_runs.h"

namespace ipcfp {

namespace ct = claimtext;

static_assert(ct::kSlotBytes == IPCFP_CID_SLOT, "slot size");

// the literals of the two proof objects, in text order (lengths without the NUL)
#define CT_LIT(name, text)                            \
    __device__ const char name[] = text;              \
    constexpr uint32_t name##_n = sizeof(text) - 1u
CT_LIT(kHead0, "{\"storage_proofs\":[");
CT_LIT(kHead1, "],\"event_proofs\":[");
CT_LIT(kHead2, "],\"blocks\":[");
CT_LIT(kSValue, "\",\"value\":\"0x");
CT_LIT(kSEnd, "\"}");
CT_LIT(kEParent, "{\"parent_epoch\":");
CT_LIT(kEChild, ",\"child_epoch\":");
CT_LIT(kEMsg, ",\"message_cid\":\"");
CT_LIT(kEExec, "\",\"exec_index\":");
CT_LIT(kEEvent, ",\"event_index\":");
CT_LIT(kEEmitter, ",\"event_data\":{\"emitter\":");
CT_LIT(kETopics, ",\"topics\":[");
CT_LIT(kEData, "],\"data\":\"0x");
CT_LIT(kEEnd, "\"}}");
#undef CT_LIT

// what a run contributes to each of its claims: 421 bytes at the most (five literals of 15 + 20 + 23 + 13 + 20 + 18 + 12, two
// integers of at most 20 characters, four CID strings of at most 65)
constexpr uint32_t kRunFragStride = kClaimTextRunFragStride;
static_assert(15 + 20 + 20 + 65 + 23 + 65 + 13 + 20 + 20 + 65 + 18 + 65 + 12 <= kRunFragStride, "a run's fragment fits its stride");

// refusal codes (the low 4 bits of the error word): which check of the host route failed
enum : uint32_t {
    kCtRunFlags = 1,    // run flags != IPCFP_SRUN_FLAG_MASK or reserved != 0
    kCtColFlags = 2,    // cflags byte != IPCFP_SCOL_FLAG_MASK
    kCtSlotBad = 3,     // a CID slot of the run is not one well-formed CID
    kCtSlotFold = 4,    // … is a fold                                            (IPCFP_E_UNSUPPORTED)
    kCtTipsetIndex = 5, // claim.tipset >= n_tipsets
    kCtClaimFlags = 6,  // MSG_PARSED | DATA_MATCHABLE not both set
    kCtTipsetBad = 7,   // the named tipset has no text (flags, key length, a malformed slot)
    kCtTipsetFold = 8,  // … a folded slot                                        (IPCFP_E_UNSUPPORTED)
    kCtBlobRange = 9,   // topics or data leave the blob
    kCtMsgBad = 10,     // message_cid slot is not one well-formed CID
    kCtMsgFold = 11,    // … is a fold                                            (IPCFP_E_UNSUPPORTED)
    kCtTopicFlag = 12,  // a topic's flag byte is 0
};

struct RunInfo {
    uint32_t len;   // bytes of the run's fragment
    uint32_t code;  // low 4 bits: 0, or the refusal every claim of the run gets (kCtRunFlags is judged before the slots);
                    // bits 8-13: the flag bits the run lacks and each of its claims must bring in its cflags byte
};
static_assert(sizeof(RunInfo) == kClaimTextRunInfo, "run_info_d");
struct TipsetFrag {  // host-rendered, one per tipset of the caller's table
    uint64_t off;    // into the fragment bytes
    uint32_t len;
    uint32_t code;   // 0, kCtTipsetBad or kCtTipsetFold
};
static_assert(sizeof(TipsetFrag) == kClaimTextTipsetRec, "the host writes these records");

__global__ __launch_bounds__(256) void k_claim_run_frags(const StorageRunRec* __restrict__ tab, uint32_t n_runs,
                                                         uint8_t* __restrict__ frag, RunInfo* __restrict__ info) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_runs) return;
    const StorageRunRec& rec = tab[r];
    const uint8_t* slot[4] = {reinterpret_cast<const uint8_t*>(&rec.child), reinterpret_cast<const uint8_t*>(&rec.state_root),
                              reinterpret_cast<const uint8_t*>(&rec.actor_state), reinterpret_cast<const uint8_t*>(&rec.storage_root)};
    uint32_t code = 0;
    int len[4] = {0, 0, 0, 0};
    // The host route judges the EXPANDED claim: flags = run's | claim's must be all six bits and nothing else.  A run with a
    // bit nobody knows or a reserved word is refused whatever its claims say; the known bits it lacks (`miss`) are its
    // claims' to bring.
    constexpr uint32_t kAll = IPCFP_SRUN_FLAG_MASK | IPCFP_SCOL_FLAG_MASK;
    const uint32_t miss = kAll & ~rec.flags;
    if ((rec.flags & ~kAll) != 0u || rec.reserved != 0u) code = kCtRunFlags;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (code) break;
        len[k] = ct::slot_cid_len(slot[k]);
        if (len[k] < 0) code = kCtSlotFold;
        else if (len[k] == 0) code = kCtSlotBad;
    }
    uint32_t at = 0;
    if (!code) {
        uint8_t* o = frag + size_t(r) * kRunFragStride;
        at += ct::put_lit(o + at, "{\"child_epoch\":");
        at += ct::put_i64(o + at, rec.child_epoch);
        at += ct::put_lit(o + at, ",\"child_block_cid\":\"");
        at += ct::put_cid_str(o + at, slot[0], uint32_t(len[0]));
        at += ct::put_lit(o + at, "\",\"parent_state_root\":\"");
        at += ct::put_cid_str(o + at, slot[1], uint32_t(len[1]));
        at += ct::put_lit(o + at, "\",\"actor_id\":");
        at += ct::put_u64(o + at, rec.actor_id);
        at += ct::put_lit(o + at, ",\"actor_state_cid\":\"");
        at += ct::put_cid_str(o + at, slot[2], uint32_t(len[2]));
        at += ct::put_lit(o + at, "\",\"storage_root\":\"");
        at += ct::put_cid_str(o + at, slot[3], uint32_t(len[3]));
        at += ct::put_lit(o + at, "\",\"slot\":\"0x");
    }
    info[r] = RunInfo{at, code | (miss << 8)};
}

// the items: [0] kHead0, [1, 1 + n_s) storage claims, [1 + n_s] kHead1, then n_e event claims, then kHead2
struct ClaimTextArgs {
    const StorageRunRec* runs;
    const uint32_t* run_of;  // per storage claim; >= n_runs where the run table does not tile (reported elsewhere)
    const RunInfo* run_info;
    const uint8_t* run_frag;
    const uint8_t *slot, *value, *cflags;
    uint32_t n_runs, n_storage;
    const EventClaimPacked* claims;
    const uint8_t* blob;
    uint64_t blob_len;
    const TipsetFrag* tipsets;
    const uint8_t* tipset_frag;
    uint32_t n_tipsets, n_events;
};

// the lengths of an event claim's variable fields
struct EventLayout {
    uint32_t pe, ce, frag, msg, msg_len, exec, event, emitter;
    uint64_t topics, data;
};
__device__ __forceinline__ EventLayout event_layout(const EventClaimPacked& c, const TipsetFrag& t, int msg_len) {
    EventLayout L;
    L.pe = ct::dec_len_i64(c.parent_epoch);
    L.ce = ct::dec_len_i64(c.child_epoch);
    L.frag = t.len;
    L.msg_len = uint32_t(msg_len);
    L.msg = ct::cid_str_len(reinterpret_cast<const uint8_t*>(&c.message), L.msg_len);
    L.exec = ct::dec_len_u64(c.exec_index);
    L.event = ct::dec_len_u64(c.event_index);
    L.emitter = ct::dec_len_u64(c.emitter);
    L.topics = c.n_topics ? 69ull * c.n_topics - 1u : 0ull;  // "0x + 64 digits + " and the commas between
    L.data = 2ull * c.data_len;
    return L;
}
__device__ __forceinline__ uint64_t event_text_len(const EventLayout& L) {
    return uint64_t(kEParent_n + L.pe + kEChild_n + L.ce + 1u + L.frag + kEMsg_n + L.msg + kEExec_n + L.exec + kEEvent_n + L.event +
                    kEEmitter_n + L.emitter + kETopics_n) +
           L.topics + kEData_n + L.data + kEEnd_n;
}

__global__ __launch_bounds__(256) void k_claim_text_sizes(ClaimTextArgs a, uint64_t* __restrict__ size_out,
                                                          unsigned long long* __restrict__ first_bad) {
    const uint64_t n_items = uint64_t(a.n_storage) + a.n_events + 3u;
    const uint64_t it = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if (it >= n_items) return;
    if (it == 0u) {
        size_out[it] = kHead0_n;
        return;
    }
    if (it == uint64_t(a.n_storage) + 1u) {
        size_out[it] = kHead1_n;
        return;
    }
    if (it == n_items - 1u) {
        size_out[it] = kHead2_n;
        return;
    }
    uint32_t code = 0;
    uint64_t size = 0;
    if (it <= a.n_storage) {
        const uint32_t i = uint32_t(it - 1u);
        const uint32_t r = a.run_of[i];
        if (r < a.n_runs) {
            const RunInfo ri = a.run_info[r];
            const uint32_t miss = (ri.code >> 8) & 63u, cf = a.cflags[i];
            if ((ri.code & 15u) == kCtRunFlags) code = kCtRunFlags;
            else if ((cf & ~63u) != 0u || (cf & miss) != miss) code = miss == IPCFP_SCOL_FLAG_MASK ? kCtColFlags : kCtRunFlags;
            else code = ri.code & 15u;
            size = (i ? 1u : 0u) + uint64_t(ri.len) + 64u + kSValue_n + 64u + kSEnd_n;
        }
        if (code) atomicMin(first_bad, ((unsigned long long)i << 4) | code);
    } else {
        const uint32_t i = uint32_t(it - a.n_storage - 2u);
        const EventClaimPacked& c = a.claims[i];
        const uint32_t both = IPCFP_CLAIM_MSG_PARSED | IPCFP_CLAIM_DATA_MATCHABLE;
        int mlen = 0;
        if (c.context >= a.n_tipsets) code = kCtTipsetIndex;
        else if ((c.flags & both) != both) code = kCtClaimFlags;
        else if (a.tipsets[c.context].code) code = a.tipsets[c.context].code;
        else if (uint64_t(c.topics_off) + 33ull * c.n_topics > a.blob_len || uint64_t(c.data_off) + c.data_len > a.blob_len) code = kCtBlobRange;
        else if ((mlen = ct::slot_cid_len(reinterpret_cast<const uint8_t*>(&c.message))) <= 0) code = mlen < 0 ? kCtMsgFold : kCtMsgBad;
        else {
            for (uint32_t k = 0; k < c.n_topics; ++k)
                if (a.blob[size_t(c.topics_off) + 33u * size_t(k)] == 0) code = kCtTopicFlag;
        }
        if (code) atomicMin(first_bad, (1ull << 36) | ((unsigned long long)i << 4) | code);
        else size = (i ? 1u : 0u) + event_text_len(event_layout(c, a.tipsets[c.context], mlen));
    }
    size_out[it] = code ? 0ull : size;
}

// byte k of a storage claim's item
__device__ __forceinline__ uint8_t storage_item_byte(const ClaimTextArgs& a, uint32_t i, uint32_t r, uint32_t frag_len, uint64_t k) {
    if (i) {
        if (k == 0u) return ',';
        --k;
    }
    if (k < frag_len) return a.run_frag[size_t(r) * kRunFragStride + k];
    k -= frag_len;
    if (k < 64u) return ct::hex_char(a.slot + 32ull * i, k);
    k -= 64u;
    if (k < kSValue_n) return uint8_t(kSValue[k]);
    k -= kSValue_n;
    if (k < 64u) return ct::hex_char(a.value + 32ull * i, k);
    k -= 64u;
    return uint8_t(kSEnd[k]);
}

// byte k of an event claim's item
__device__ __forceinline__ uint8_t event_item_byte(const ClaimTextArgs& a, uint32_t i, const EventClaimPacked& c, const TipsetFrag& t,
                                                   const EventLayout& L, uint64_t k) {
    if (i) {
        if (k == 0u) return ',';
        --k;
    }
#define CT_PIECE(lit, n, expr)                    \
    if (k < lit##_n) return uint8_t(lit[k]);      \
    k -= lit##_n;                                 \
    if (k < (n)) return (expr);                   \
    k -= (n)
    CT_PIECE(kEParent, L.pe, ct::dec_char_i64(c.parent_epoch, L.pe, uint32_t(k)));
    CT_PIECE(kEChild, L.ce, ct::dec_char_i64(c.child_epoch, L.ce, uint32_t(k)));
    if (k == 0u) return ',';
    --k;
    if (k < L.frag) return a.tipset_frag[t.off + k];
    k -= L.frag;
    CT_PIECE(kEMsg, L.msg, ct::cid_str_char(reinterpret_cast<const uint8_t*>(&c.message), L.msg_len, uint32_t(k)));
    CT_PIECE(kEExec, L.exec, ct::dec_char_u64(c.exec_index, L.exec, uint32_t(k)));
    CT_PIECE(kEEvent, L.event, ct::dec_char_u64(c.event_index, L.event, uint32_t(k)));
    CT_PIECE(kEEmitter, L.emitter, ct::dec_char_u64(c.emitter, L.emitter, uint32_t(k)));
    if (k < kETopics_n) return uint8_t(kETopics[k]);
    k -= kETopics_n;
    if (k < L.topics) {  // "0x <64> " , "0x <64> " …: 69 characters per topic with its comma
        const uint64_t q = k / 69u;
        const uint32_t j = uint32_t(k - q * 69u);
        if (j == 0u || j == 67u) return '"';
        if (j == 1u) return '0';
        if (j == 2u) return 'x';
        if (j == 68u) return ',';
        return ct::hex_char(a.blob + size_t(c.topics_off) + 33u * size_t(q) + 1u, j - 3u);
    }
    k -= L.topics;
    CT_PIECE(kEData, L.data, ct::hex_char(a.blob + c.data_off, k));
#undef CT_PIECE
    return uint8_t(kEEnd[k]);
}

// Runs only behind a sizing pass that found nothing to refuse: every run_of is a run, every tipset index, blob range and CID
// slot has been checked, so no read leaves its array.  text: on a 16-byte boundary; bytes [0, head_len) are written.
__global__ __launch_bounds__(256) void k_claim_text_write(ClaimTextArgs a, const uint64_t* __restrict__ off, uint64_t head_len,
                                                          uint8_t* __restrict__ text) {
    const uint64_t n_items = uint64_t(a.n_storage) + a.n_events + 3u;
    const uint64_t chunk = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    const uint64_t pos = chunk * 16u;
    const uint64_t chunk0 = chunk & ~63ull;
    const uint64_t pos0 = (uint64_t(__builtin_amdgcn_readfirstlane(uint32_t(chunk0 >> 32))) << 32 |
                           uint64_t(__builtin_amdgcn_readfirstlane(uint32_t(chunk0)))) * 16u;
    if (pos0 >= head_len) return;
    uint64_t lo = 0, hi = n_items;  // the last item that starts at or before the wavefront's first byte (off[0] = 0)
    while (hi - lo > 1u) {
        const uint64_t mid = (lo + hi) >> 1;
        if (off[mid] <= pos0) lo = mid;
        else hi = mid;
    }
    if (pos >= head_len) return;
    const uint32_t n_out = uint32_t(head_len - pos < 16u ? head_len - pos : 16u);
    uint64_t w_lo = 0, w_hi = 0;  // the 16 bytes, shifted in from the top (k_base64_encode's last unit: no indexed registers)
    uint32_t b = 0;
    while (b < n_out) {
        while (lo + 1u < n_items && off[lo + 1u] <= pos + b) ++lo;  // (a claim's item is never empty; this also passes lo's own end)
        const uint64_t item_end = lo + 1u < n_items ? off[lo + 1u] : head_len;
        const uint64_t k0 = pos + b - off[lo];
        const uint32_t cnt = uint32_t(item_end - (pos + b) < uint64_t(n_out - b) ? item_end - (pos + b) : uint64_t(n_out - b));
        auto push = [&](uint8_t ch) {
            w_lo = (w_lo >> 8) | (w_hi << 56);
            w_hi = (w_hi >> 8) | (uint64_t(ch) << 56);
        };
        if (lo == 0u) {
            for (uint32_t j = 0; j < cnt; ++j) push(uint8_t(kHead0[k0 + j]));
        } else if (lo == uint64_t(a.n_storage) + 1u) {
            for (uint32_t j = 0; j < cnt; ++j) push(uint8_t(kHead1[k0 + j]));
        } else if (lo == n_items - 1u) {
            for (uint32_t j = 0; j < cnt; ++j) push(uint8_t(kHead2[k0 + j]));
        } else if (lo <= a.n_storage) {
            const uint32_t i = uint32_t(lo - 1u), r = a.run_of[i];
            const uint32_t frag_len = a.run_info[r].len;
            for (uint32_t j = 0; j < cnt; ++j) push(storage_item_byte(a, i, r, frag_len, k0 + j));
        } else {
            const uint32_t i = uint32_t(lo - a.n_storage - 2u);
            const EventClaimPacked& c = a.claims[i];
            const TipsetFrag t = a.tipsets[c.context];
            const EventLayout L = event_layout(c, t, ct::slot_cid_len(reinterpret_cast<const uint8_t*>(&c.message)));
            for (uint32_t j = 0; j < cnt; ++j) push(event_item_byte(a, i, c, t, L, k0 + j));
        }
        b += cnt;
    }
    if (n_out == 16u) {
        *reinterpret_cast<ulonglong2*>(text + pos) = make_ulonglong2(w_lo, w_hi);
        return;
    }
    // the head's last, partial chunk: the bytes behind it are the block writer's
    for (uint32_t j = n_out; j < 16u; ++j) {
        w_lo = (w_lo >> 8) | (w_hi << 56);
        w_hi >>= 8;
    }
    for (uint32_t j = 0; j < n_out; ++j) {
        text[pos + j] = uint8_t(w_lo);
        w_lo = (w_lo >> 8) | (w_hi << 56);
        w_hi >>= 8;
    }
}

static ClaimTextArgs make_args(const ClaimTextIn& in) {
    ClaimTextArgs a;
    a.runs = static_cast<const StorageRunRec*>(in.cols.runs);
    a.run_of = in.run_of_d;
    a.run_info = static_cast<const RunInfo*>(in.run_info_d);
    a.run_frag = in.run_frag_d;
    a.slot = in.cols.slot;
    a.value = in.cols.value;
    a.cflags = in.cols.cflags;
    a.n_runs = in.cols.n_runs;
    a.n_storage = in.n_storage;
    a.claims = static_cast<const EventClaimPacked*>(in.claims_d);
    a.blob = in.blob_d;
    a.blob_len = in.blob_len;
    a.tipsets = static_cast<const TipsetFrag*>(in.tipsets_d);
    a.tipset_frag = in.tipset_frag_d;
    a.n_tipsets = in.n_tipsets;
    a.n_events = in.n_events;
    return a;
}

int launch_claim_text_sizes(ipcfp_ctx* ctx, const ClaimTextIn& in, uint64_t* size_d, uint64_t* off_d, uint64_t* total_d,
                            uint64_t* scratch_d, unsigned long long* first_bad_d) {
    ProfileScope prof(ctx, IPCFP_K_CLAIM_TEXT);
    if (in.cols.n_runs) {
        hipLaunchKernelGGL(k_claim_run_frags, dim3(div_up(in.cols.n_runs, 256)), dim3(256), 0, ctx->stream,
                           static_cast<const StorageRunRec*>(in.cols.runs), in.cols.n_runs, in.run_frag_d,
                           static_cast<RunInfo*>(in.run_info_d));
        IPCFP_HIP(ctx, hipGetLastError());
    }
    const uint64_t n_items = uint64_t(in.n_storage) + in.n_events + 3u;
    hipLaunchKernelGGL(k_claim_text_sizes, dim3(div_up(n_items, 256)), dim3(256), 0, ctx->stream, make_args(in), size_d, first_bad_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return launch_scan_u64(ctx, size_d, uint32_t(n_items), off_d, total_d, scratch_d);
}

int launch_claim_text_write(ipcfp_ctx* ctx, const ClaimTextIn& in, const uint64_t* off_d, uint64_t head_len, uint8_t* text_d) {
    ProfileScope prof(ctx, IPCFP_K_CLAIM_TEXT);
    const uint64_t chunks = (head_len + 15u) / 16u;
    hipLaunchKernelGGL(k_claim_text_write, dim3(div_up(chunks, 256)), dim3(256), 0, ctx->stream, make_args(in), off_d, head_len, text_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
