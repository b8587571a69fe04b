// csrc/kernels/tipset_prepare_general.hip — the tipset prologue (tipset_prologue_body.h) with the general, global-memory
// reader: the one-context form of the generator / shard-plan paths and of wide tipset keys (k_tipset_prepare_one), and
// the companion of the LDS prologue (tipset_prepare.hip) for the slots whose blocks do not fit its stage
// (k_tipset_prepare_flagged); and the prologue's deferred half, the TxMeta re-hashes (k_txmeta_rehash).  A unit of its
// own so that these single-wavefront workgroups carry 8 KB of LDS and not the line-staging area of verify_events.hip:
// beside the block-order event parse a 43 KB workgroup waits for a CU to drain.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../common.h"
#include "blake2b_dev.h"
#include "claims_dev.h"
#include "amt_enum.h"
#include "event_table.h"
#include "tipset_prologue_body.h"
#include "types_dev.h"
#include "launch.h"

namespace ipcfp {

// The opener of this unit (tipset_prologue_body.h): the wavefront stages the block in LDS when it fits (a header decode is
// ~100 CBOR items parsed by ONE lane; from HBM that lane pays a round trip per window chunk), else the reader's window
// runs over HBM.  It always opens.
constexpr uint32_t kHeaderLds = 8192;
struct StagedOpener {
    uint8_t* lds;
    Rd r;
    __device__ __forceinline__ bool operator()(const WitnessView& w, uint32_t b) {
        r = open_block_staged(w, b, lds, kHeaderLds);
        return true;
    }
    __device__ __forceinline__ Rd reader() const { return r; }
    __device__ __forceinline__ void overflow(TipsetCtxDev&, uint32_t) const {}
};

// slot s of job jb: 0 / 1 the header facts (child header with the receipts root as the enumeration's extra spec, first
// parent header), 2 + b parent block b's header → TxMeta → message-AMT roots (for a job that has roots)
__device__ __forceinline__ void prologue_slot(const WitnessView& w, const PrepareJob& jb, uint32_t slot, TxMetaMode mode, uint8_t* lds) {
    const TipsetKeysCtx keys{*jb.ctx};
    StagedOpener opener{lds, Rd{}};
    if (slot < 2) prologue_headers(w, keys, *jb.ctx, slot == 0, opener, jb.roots ? jb.roots + 2u * jb.ctx->n_parents : nullptr);
    else if (jb.roots) prologue_roots(w, keys, *jb.ctx, jb.roots, jb.err, slot - 2u, opener, mode);
}

// The general companion of the LDS prologue: the same jobs and slots, for the slots that kernel left alone because a block
// did not fit its stage (TipsetCtxDev::prologue_general).  Normally every workgroup leaves at once.
__global__ __launch_bounds__(64) void k_tipset_prepare_flagged(WitnessView w, PrepareJobs jobs, uint32_t n_jobs) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kHeaderLds];
    const uint32_t job = blockIdx.x / kPrepareSlots, slot = blockIdx.x % kPrepareSlots;
    if (job >= n_jobs) return;
    const PrepareJob jb = prepare_job(jobs, job);
    if (!((jb.ctx->prologue_general >> slot) & 1ull)) return;
    prologue_slot(w, jb, slot, kTxMetaCheck, lds);
}

// Slots first_slot .. first_slot + gridDim.x - 1 of ONE context, whatever the width of its tipset key (TipsetCtxDev::
// parents_wide); a slot behind the last parent block leaves at once.  `mode`: kTxMetaCheck or kTxMetaNone (the deferred
// re-hash is the LDS launch's: txmeta_block has one word per INLINE parent).
__global__ __launch_bounds__(64) void k_tipset_prepare_one(WitnessView w, PrepareJob jb, uint32_t first_slot, TxMetaMode mode) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kHeaderLds];
    prologue_slot(w, jb, first_slot + blockIdx.x, mode, lds);
}

static int launch_prepare_one(ipcfp_ctx* ctx, const WitnessView& w, const PrepareJob& jb, uint32_t first_slot, uint32_t n_slots,
                              TxMetaMode mode) {
    hipLaunchKernelGGL(k_tipset_prepare_one, dim3(n_slots), dim3(64), 0, ctx->stream, w, jb, first_slot, mode);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

// the whole prologue of a context with a wide key: its own launch (host/tipset_wide.h)
int launch_tipset_prepare_wide(ipcfp_ctx* ctx, const WitnessView& w, const void* job, uint32_t n_parents) {
    return launch_prepare_one(ctx, w, *static_cast<const PrepareJob*>(job), 0, 2u + n_parents, kTxMetaCheck);
}

// the header facts alone (two wavefronts side by side: the two decodes are tens of microseconds of one lane's latency each)
int launch_ctx_headers(ipcfp_ctx* ctx, const WitnessView& w, TipsetCtxDev* ctx_d) {
    return launch_prepare_one(ctx, w, PrepareJob{ctx_d, nullptr, nullptr}, 0, 2, kTxMetaCheck);
}

// stage 1 of the execution order alone: one workgroup per parent block (the grid of the inline form is fixed so that the
// host need not know the count)
int launch_exec_roots(ipcfp_ctx* ctx, const WitnessView& w, const TipsetCtxDev* ctx_d, AmtRootSpec* roots_d,
                      unsigned long long* err_d, int verify_txmeta, uint32_t n_parents) {
    IPCFP_HIP(ctx, hipMemsetAsync(err_d, 0xff, 8, ctx->stream));  // kNoEnumError
    return launch_prepare_one(ctx, w, PrepareJob{const_cast<TipsetCtxDev*>(ctx_d), roots_d, err_d}, 2,
                              n_parents > IPCFP_MAX_PARENTS ? n_parents : IPCFP_MAX_PARENTS,
                              verify_txmeta ? kTxMetaCheck : kTxMetaNone);  // 0: the generator (build_execution_order, utils.rs:44)
}

// The prologue's deferred half — the TxMeta re-hash of parent block b, left behind by the LDS prologue in kTxMetaDefer
// mode (tipset_ctx.h txmeta_block): put_cbor(&(bls_root, secp_root), Blake2b256) must give the CID the header named
// (src/proofs/events/utils.rs:65-72; the verify path always checks).  The block was decoded by the prologue already; its
// CID is the key it was found under.
__device__ __forceinline__ void txmeta_rehash_lane(const WitnessView& w, const TipsetCtxDev& c, uint32_t b, unsigned long long* __restrict__ err) {
    if (b >= c.n_parents || b >= IPCFP_MAX_PARENTS) return;
    if (c.txmeta_block[b] == 0u) return;  // (1 + block id: tipset_ctx.h)
    const uint32_t tb = c.txmeta_block[b] - 1u;
    const uint32_t seq = c.n_parents + 3 * b;
    auto fail = [&](uint32_t code) { atomicMin(err, (unsigned long long)pack_enum_error(seq, 0, code)); };
    Rd r;
    r.init(w.arena + w.off[tb], w.len[tb]);
    uint32_t o[2], l[2];
    if (!txmeta_links(r, o[0], l[0], o[1], l[1]) || l[0] > 64u || l[1] > 64u) {  // (the prologue took this very block: not reachable)
        fail(IPCFP_ST_ERR_DECODE);
        return;
    }
    CidKey re;
    if (w.len[tb] == 87u && o[0] == 6u && l[0] == 38u && o[1] == 49u && l[1] == 38u) {
        // `82 | d8 2a 58 27 00 ‖ 38 | d8 2a 58 27 00 ‖ 38`: the canonical re-encoding IS the block — one compression
        // straight from its bytes (blocks sit on 128-byte lines with tail slack), no byte buffer in scratch
        uint64_t m[16];
        const ulonglong2* q = reinterpret_cast<const ulonglong2*>(w.arena + w.off[tb]);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const ulonglong2 v = k < 6 ? q[k] : ulonglong2{0ull, 0ull};
            m[2 * k] = v.x;
            m[2 * k + 1] = v.y;
        }
        b2b::mask_tail(m, 87u);
        uint64_t h[8];
        b2b::init256(h);
        b2b::compress(h, m, 87ull, true);
        txmeta_cid_of_digest(h, re);
    } else {
        txmeta_rehash(r, o[0], l[0], o[1], l[1], re);
    }
    if (!cid_equal(re, load_cid_slot(w.cids, tb))) fail(IPCFP_ST_ERR_TXMETA_MISMATCH);
}

// one lane per parent block.  Nothing waits for this launch but the end of the call (host/verify_fast.cpp queues it on
// the aux stream behind the receipts' event records): as a second workgroup of k_enum_roots it took 123 µs and held
// the first level of the walk back for as long.
__global__ __launch_bounds__(64) void k_txmeta_rehash(WitnessView w, const TipsetCtxDev* __restrict__ c, unsigned long long* __restrict__ err) {
    txmeta_rehash_lane(w, *c, threadIdx.x, err);
}

int launch_txmeta_rehash(ipcfp_ctx* ctx, hipStream_t stream, const WitnessView& view, const TipsetCtxDev* ctx_d, unsigned long long* err_d) {
    hipLaunchKernelGGL(k_txmeta_rehash, dim3(1), dim3(64), 0, stream, view, ctx_d, err_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

void launch_tipset_prepare_lds(hipStream_t stream, const WitnessView& w, const PrepareJobs& jobs, uint32_t n_jobs, bool defer_rehash,
                               const TipsetInputs* inline_inputs);  // tipset_prepare.hip

// `jobs`: HOST array; `jobs_d`: device copy, needed (and read) only when there are more than kInlineJobs.
// `need_general`: some block of the witness may exceed the LDS stage, so the general companion has to look.
int launch_tipset_prepare(ipcfp_ctx* ctx, const WitnessView& w, const void* jobs, const void* jobs_d, uint32_t n_jobs,
                          bool need_general, bool defer_rehash, const void* inline_inputs) {
    if (defer_rehash && need_general) return set_error(ctx, IPCFP_E_INVALID, "deferred TxMeta re-hash: LDS slots only");
    if (n_jobs == 0) return IPCFP_OK;
    PrepareJobs pj{};
    if (n_jobs <= kInlineJobs) std::memcpy(pj.inline_jobs, jobs, size_t(n_jobs) * sizeof(PrepareJob));
    else pj.more = static_cast<const PrepareJob*>(jobs_d);
    // (`inline_inputs`: the ONE context's TipsetInputs on the host — they ride in the kernel arguments and the context's
    // zeroed device copy is filled in by the launch itself)
    launch_tipset_prepare_lds(ctx->stream, w, pj, n_jobs, defer_rehash, static_cast<const TipsetInputs*>(inline_inputs));
    if (need_general)
        hipLaunchKernelGGL(k_tipset_prepare_flagged, dim3(n_jobs * kPrepareSlots), dim3(64), 0, ctx->stream, w, pj, n_jobs);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp

#include "event_gen_tipsets.inc"
