// csrc/kernels/tipset_prepare.hip — the tipset prologue of the verify path, parsed out of LDS.
//
// What `verify_single_proof` derives from (parent_tipset_cids, child_block_cid) before it looks at a proof: the child
// header and the first parent header (verify_header_consistency, src/proofs/events/verifier.rs:147-181) and, per parent
// block, its header, its TxMeta and the TxMeta's re-hash (reconstruct_execution_order / collect_exec_list,
// src/proofs/events/utils.rs:16-30,48-94).  Each is a parse of ≈100 CBOR items by ONE lane — there is no data
// parallelism inside a header — so the launch is a handful of single-wavefront workgroups whose time is the length
// of one lane's instruction stream, stretched further by whatever shares the CU (K1, the block-order event parse).
// Hence this unit: the wavefront stages the block in LDS and the lane parses it with the LDS reader (cbor_dev.h
// IPCFP_RD_LDS: a byte is a ds_read_u8, a header one aligned ds_read2_b64 — no window to maintain), a third of the
// instructions of the windowed reader the same parse needs on global memory.
//
// The text of the parse is tipset_prologue_body.h, instantiated here with the LDS reader and this unit's opener.  A block
// that does not fit the stage is not parsed here: the slot is flagged in TipsetCtxDev::prologue_general and
// k_tipset_prepare_flagged (tipset_prepare_general.hip), launched right behind, does that slot with the general reader.
#define IPCFP_RD_LDS 1
#include <hip/hip_runtime.h>

#include "../common.h"
#include "blake2b_dev.h"
#include "claims_dev.h"
#include "tipset_prologue_body.h"

namespace ipcfp {

typedef __attribute__((address_space(3))) const uint8_t* lds_bytes_t;

// The opener of this unit (tipset_prologue_body.h): every lane of the wavefront copies block b into the stage, the lead
// lane's reader sits on the copy.  A block that does not fit is not parsed here: the slot is flagged for the general
// companion (TipsetCtxDev::prologue_general).
struct StageOpener {
    rd_chunk_t* stage;
    uint32_t len;
    __device__ __forceinline__ bool operator()(const WitnessView& w, uint32_t b) {
        len = w.len[b];
        if (len + kPrologueStageSlack > kPrologueStageBytes) return false;
        const rd_chunk_t* src = reinterpret_cast<const rd_chunk_t*>(w.arena + w.off[b]);  // line-aligned, padded, + tail slack
        const uint32_t chunks = ((len + 15u) >> 4) + 2u;
        for (uint32_t i = threadIdx.x; i < chunks; i += 64u) stage[i] = src[i];
        __syncthreads();
        return true;
    }
    __device__ __forceinline__ Rd reader() const {
        Rd r;
        r.init((lds_bytes_t)stage, len);
        return r;
    }
    __device__ __forceinline__ void overflow(TipsetCtxDev& c, uint32_t slot) const {
        if (threadIdx.x == 0) atomicOr(&c.prologue_general, 1ull << slot);
    }
};

// INLINE: the one context's inputs are the kernel ARGUMENT `in0` (scalar loads from the kernarg segment); its device copy
// — zeroed memory, not yet written by anyone — gets them from slot 0, for the kernels behind this launch.
// (5 waves per SIMD, i.e. at most 96 VGPRs: what the INLINE instance — the verify step's — was allocated before the
// live-index code left; without the bound the allocator gives the shorter kernel 101 / 103)
template <bool INLINE>
__global__ __launch_bounds__(64, 5) void k_tipset_prepare(WitnessView w, PrepareJobs jobs, uint32_t n_jobs, int defer_rehash,
                                                       TipsetInputs in0) {
    __shared__ rd_chunk_t stage[kPrologueStageChunks];
    const uint32_t job = blockIdx.x / kPrepareSlots, slot = blockIdx.x % kPrepareSlots;
    if (job >= n_jobs) return;
    const PrepareJob jb = prepare_job(jobs, job);
    const TipsetInputs& in = INLINE ? in0 : *reinterpret_cast<const TipsetInputs*>(jb.ctx);
    if (INLINE && slot == 0) {  // 688 bytes, sixteen at a time
        static_assert(sizeof(TipsetInputs) % 8 == 0, "copied as 64-bit words");
        const uint64_t* src = reinterpret_cast<const uint64_t*>(&in0);
        uint64_t* dst = reinterpret_cast<uint64_t*>(jb.ctx);
        for (uint32_t i = threadIdx.x; i < sizeof(TipsetInputs) / 8; i += 64u) dst[i] = src[i];
    }
    // (`in`: the context's inputs — its own head in device memory, or the kernel argument)
    const TipsetKeysInline keys{in};
    StageOpener opener{stage, 0u};
    if (slot < 2) prologue_headers(w, keys, *jb.ctx, slot == 0, opener, jb.roots ? jb.roots + 2u * in.n_parents : nullptr);
    else if (jb.roots) prologue_roots(w, keys, *jb.ctx, jb.roots, jb.err, slot - 2, opener, defer_rehash ? kTxMetaDefer : kTxMetaCheck);
}

void launch_tipset_prepare_lds(hipStream_t stream, const WitnessView& w, const PrepareJobs& jobs, uint32_t n_jobs, bool defer_rehash,
                               const TipsetInputs* inline_inputs) {
    if (inline_inputs && n_jobs == 1)
        hipLaunchKernelGGL(k_tipset_prepare<true>, dim3(kPrepareSlots), dim3(64), 0, stream, w, jobs, n_jobs, defer_rehash ? 1 : 0,
                           *inline_inputs);
    else
        hipLaunchKernelGGL(k_tipset_prepare<false>, dim3(n_jobs * kPrepareSlots), dim3(64), 0, stream, w, jobs, n_jobs,
                           defer_rehash ? 1 : 0, TipsetInputs{});
}

}  // namespace ipcfp
