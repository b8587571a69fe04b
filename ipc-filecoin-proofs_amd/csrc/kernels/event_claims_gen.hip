// csrc/kernels/event_claims_gen.hip — generated matches → packed EventProof claims (claims_dev.h EventClaimPacked + blob).
//
// The last step of `find_matching_events` (src/proofs/events/generator.rs:262-297): every match becomes an EventProof whose
// `event_data` is `extract_evm_log(&se.event)` (src/proofs/common/evm.rs:13-59).  Matches, message CIDs and the events
// themselves are in HBM when the scan returns, so the proofs are written there too, in the form the verify kernels read:
// byte for byte what host/pack_claims.cpp lower_one makes of the reference's strings.
//
//   k_gen_claim_sizes   one lane per match: the location checked against the witness, decode_event_log over exactly the
//                       item, the claim's blob segment size (33 per topic + the data) and a 32-byte GenRec that says where
//                       the topics and the data lie — the fill decodes nothing
//   (prefix sum)        scan.hip launch_scan_u64 over the sizes
//   k_gen_claim_fill    lane i writes claim record i; lane j assembles bytes [16 j, 16 j + 16) of the blob
//
// Form of the fill: the partition of k_base64_encode.  A lane owns a fixed 16 bytes of the BLOB, a
// wavefront 1 KiB of it; the wavefront finds the claims of its first and last byte by two wave-uniform binary searches
// over the prefix and a lane searches only between them.  The data of one claim runs from 0 to beyond 64 KiB: a lane per
// claim would leave 63 lanes waiting for the longest copy, a lane per 16 blob bytes does the same work whatever the claims'
// sizes are, and every blob byte is written exactly once, by aligned 16-byte stores.
#include <hip/hip_runtime.h>

#include "../common.h"
#include "claims_dev.h"
#include "event_log_dev.h"
#include "launch.h"

namespace ipcfp {

// where one claim's blob bytes come from; offsets count from the start of the match's BLOCK
struct GenRec {
    uint32_t topic_off[4];  // Case B: t1..t4; Case A: topic_off[0] = the concatenation (topic t at + 32 t)
    uint32_t data_off, data_len;
    uint32_t n_topics;
    uint32_t flags;         // kGenOk | kGenCaseA
};
static_assert(sizeof(GenRec) == 32, "GenRec is two 16-byte loads");
constexpr uint32_t kGenOk = 1u, kGenCaseA = 2u;
constexpr uint32_t kGenWindow = 16u;  // blob bytes per lane

__global__ __launch_bounds__(256) void k_gen_claim_sizes(WitnessView w, const ipcfp_event_match_t* __restrict__ matches, uint32_t n,
                                                         GenRec* __restrict__ recs, uint64_t* __restrict__ sizes) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t block = matches[i].event.block, off = matches[i].event.off, len = matches[i].event.len;
    GenRec g{{0u, 0u, 0u, 0u}, 0u, 0u, 0u, 0u};
    uint64_t size = 0;
    // nothing is read before the location is known to lie inside one block (kNoBlock is >= every block count)
    bool inside = block < w.n;
    if (inside) {
        const uint32_t blen = w.len[block];
        inside = len != 0u && off <= blen && len <= blen - off;
    }
    if (inside) {
        Rd r;  // bounded by `len`: every item header, string and fast path checks against r.n before it moves
        r.init(w.arena + w.off[block] + off, len);
        uint64_t emitter;
        EvmLogLoc log;
        decode_event_log(r, emitter, log);
        r.finish();  // exactly ONE StampedEvent: nothing behind it inside [off, off + len)
        if (r.ok() && log.is_log) {
            g.flags = kGenOk | (log.case_a ? kGenCaseA : 0u);
            g.n_topics = log.n_topics;
            g.topic_off[0] = off + log.topic_off[0];
            g.topic_off[1] = off + log.topic_off[1];
            g.topic_off[2] = off + log.topic_off[2];
            g.topic_off[3] = off + log.topic_off[3];
            g.data_off = off + log.data.off;
            g.data_len = log.data.present ? log.data.len : 0u;
            size = 33ull * log.n_topics + g.data_len;
        }
    }
    recs[i] = g;
    sizes[i] = size;
}

// largest c in [lo, hi] with prefix[c] <= b (prefix[lo] <= b is the caller's)
__device__ __forceinline__ uint32_t gen_claim_of(const uint64_t* __restrict__ prefix, uint64_t b, uint32_t lo, uint32_t hi) {
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo + 1u) >> 1);
        if (prefix[mid] <= b) lo = mid;
        else hi = mid - 1u;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_gen_claim_fill(WitnessView w, const ipcfp_event_match_t* __restrict__ matches,
                                                        const CidKey* __restrict__ message, uint32_t n, const GenRec* __restrict__ recs,
                                                        const uint64_t* __restrict__ prefix, uint64_t total, long long parent_epoch,
                                                        long long child_epoch, uint32_t tipset, EventClaimPacked* __restrict__ out,
                                                        uint8_t* __restrict__ blob) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    // ---- the records: lane i, claim i ----
    if (i < n) {
        const GenRec g = recs[i];
        const bool ok = (g.flags & kGenOk) != 0u;
        const uint32_t seg = uint32_t(prefix[i]);  // (total < 2^32: the host refuses a larger blob before this launch)
        EventClaimPacked p;
        p.parent_epoch = parent_epoch;
        p.child_epoch = child_epoch;
        p.exec_index = matches[i].exec_index;
        p.event_index = matches[i].event_index;
        p.emitter = matches[i].emitter;
        p.message = message[i];
        p.context = ok ? tipset : 0xffffffffu;  // cannot be lowered: ERR_BAD_CLAIM when verified, never followed
        p.flags = ok ? (EC_MSG_PARSED | EC_DATA_MATCHABLE) : 0u;
        p.n_topics = ok ? g.n_topics : 0u;
        p.topics_off = ok ? seg : 0u;
        p.data_off = ok ? seg + 33u * g.n_topics : 0u;
        p.data_len = ok ? g.data_len : 0u;
        out[i] = p;
    }
    // ---- the blob: lane i, bytes [16 i, 16 i + 16) ----
    const uint64_t wave_b0 = uint64_t(__builtin_amdgcn_readfirstlane(i & ~63u)) * kGenWindow;
    if (wave_b0 >= total) return;
    const uint64_t wave_last = (wave_b0 + 64ull * kGenWindow <= total ? wave_b0 + 64ull * kGenWindow : total) - 1ull;
    const uint32_t c_lo = gen_claim_of(prefix, wave_b0, 0u, n - 1u);      // wave-uniform: prefix[0] = 0 <= every byte
    const uint32_t c_hi = gen_claim_of(prefix, wave_last, c_lo, n - 1u);  // wave-uniform
    const uint64_t b0 = uint64_t(i) * kGenWindow;
    if (b0 >= total) return;
    const uint32_t want = total - b0 < kGenWindow ? uint32_t(total - b0) : kGenWindow;
    uint32_t c = gen_claim_of(prefix, b0, c_lo, c_hi);
    uint64_t acc_lo = 0, acc_hi = 0;  // the window's bytes, little-endian (two words: no indexed array, no scratch)
    uint32_t k = 0;                   // bytes assembled so far
    while (k < want) {
        // claim c holds byte b0 + k (claims without bytes never do: the search takes the LAST claim that starts at or before it)
        const GenRec g = recs[c];
        const uint32_t q = uint32_t(b0 + k - prefix[c]);  // offset inside the claim's segment
        const uint32_t tbytes = 33u * g.n_topics;
        const uint32_t seg_len = tbytes + g.data_len;
        if (q >= seg_len) break;  // (cannot happen: the prefix is the scan of these very sizes; never follow a run that is not there)
        const uint8_t* base = w.arena + w.off[matches[c].event.block];
        uint32_t src, run;  // a run of source bytes that land back to back, or (run == 0) the one flag byte
        if (q < tbytes) {
            const uint32_t t = q / 33u, r = q - 33u * t;
            // masks, not topic_off[t]: a dynamically indexed member would push the record to scratch (event_log_dev.h topic_at)
            const uint32_t o = (g.topic_off[0] & (t == 0u ? ~0u : 0u)) | (g.topic_off[1] & (t == 1u ? ~0u : 0u)) |
                               (g.topic_off[2] & (t == 2u ? ~0u : 0u)) | (g.topic_off[3] & (t == 3u ? ~0u : 0u));
            const uint32_t topic = (g.flags & kGenCaseA) ? g.topic_off[0] + 32u * t : o;
            src = topic + (r ? r - 1u : 0u);
            run = r ? 33u - r : 0u;
        } else {
            src = g.data_off + (q - tbytes);
            run = seg_len - q;
        }
        if (run == 0u) {  // the flag byte of a topic: "0x" + 64 hex digits, always
            if (k < 8u) acc_lo |= 1ull << (8u * k);
            else acc_hi |= 1ull << (8u * (k - 8u));
            k += 1u;
        } else if (k == 0u && run >= kGenWindow && want == kGenWindow) {
            // the whole window out of one run (the inside of a data string): two unaligned 8-byte loads
            __builtin_memcpy(&acc_lo, base + src, 8);
            __builtin_memcpy(&acc_hi, base + src + 8, 8);
            k = kGenWindow;
        } else {
            const uint32_t take = run < want - k ? run : want - k;
            for (uint32_t j = 0; j < take; ++j, ++k) {
                const uint64_t v = base[src + j];
                if (k < 8u) acc_lo |= v << (8u * k);
                else acc_hi |= v << (8u * (k - 8u));
            }
        }
        if (k < want && b0 + k >= prefix[c] + seg_len) c = gen_claim_of(prefix, b0 + k, c + 1u, c_hi);
    }
    uint8_t* dst = blob + b0;
    if (want == kGenWindow && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0u) {
        *reinterpret_cast<ulonglong2*>(dst) = ulonglong2{acc_lo, acc_hi};
    } else {  // the blob's last window, or a buffer the caller did not align
        for (uint32_t j = 0; j < want; ++j) {
            dst[j] = uint8_t(acc_lo);
            acc_lo = (acc_lo >> 8) | (acc_hi << 56);
            acc_hi >>= 8;
        }
    }
}

int launch_gen_claim_sizes(ipcfp_ctx* ctx, const WitnessView& w, const void* matches_d, uint32_t n, void* recs_d, uint64_t* size_d,
                           uint64_t* off_d, uint64_t* total_d, uint64_t* scratch_d) {
    if (n == 0) {
        IPCFP_HIP(ctx, hipMemsetAsync(total_d, 0, sizeof(uint64_t), ctx->stream));
        return IPCFP_OK;
    }
    {
        ProfileScope prof(ctx, IPCFP_K_CLAIM_SIZES);
        hipLaunchKernelGGL(k_gen_claim_sizes, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, w,
                           static_cast<const ipcfp_event_match_t*>(matches_d), n, static_cast<GenRec*>(recs_d), size_d);
        IPCFP_HIP(ctx, hipGetLastError());
    }
    ProfileScope prof(ctx, IPCFP_K_CLAIM_SCAN);
    return launch_scan_u64(ctx, size_d, n, off_d, total_d, scratch_d);
}

int launch_gen_claim_fill(ipcfp_ctx* ctx, const WitnessView& w, const void* matches_d, const CidKey* message_d, uint32_t n,
                          const void* recs_d, const uint64_t* off_d, uint64_t total, long long parent_epoch, long long child_epoch,
                          uint32_t tipset, void* claims_out_d, uint8_t* blob_out_d) {
    if (n == 0) return IPCFP_OK;
    const uint64_t windows = (total + kGenWindow - 1u) / kGenWindow;  // total < 2^32: fewer than 2^28
    const uint64_t lanes = windows > n ? windows : uint64_t(n);
    ProfileScope prof(ctx, IPCFP_K_CLAIM_FILL);
    hipLaunchKernelGGL(k_gen_claim_fill, dim3(div_up(lanes, 256)), dim3(256), 0, ctx->stream, w,
                       static_cast<const ipcfp_event_match_t*>(matches_d), message_d, n, static_cast<const GenRec*>(recs_d), off_d, total,
                       parent_epoch, child_epoch, tipset, static_cast<EventClaimPacked*>(claims_out_d), blob_out_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
