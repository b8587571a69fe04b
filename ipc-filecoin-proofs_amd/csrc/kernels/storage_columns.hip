// csrc/kernels/storage_columns.hip — StorageProof claims in run-compressed, column form (include/ipcfp.h "storage claims in
// run-compressed, column form"; storage_runs.h StorageRunRec / ColumnClaimSrc): the run table checked and laid out per
// claim, and the expansion to the plain 248-byte records.
//
// The claims of a bundle are the `storage_proofs: Vec<StorageProof>` of src/proofs/common/bundle.rs:36-45 (fields:
// src/proofs/storage/bundle.rs:5-14), verified in order by src/proofs/verifier.rs:19-28.  Whoever built the batch knew
// where one contract's proofs end and the next one's begin; the plain route finds that out again with a pass over 248-byte
// records, a prefix sum and a read-back (verify_storage.hip k_storage_run_flags / k_storage_run_heads).  Here the runs
// ARRIVE: one kernel over the run table checks that they tile [0, n) and writes run_of[t] for their claims.  The kernels
// that judge the claims are the column instantiations of verify_storage.hip's.
#include <hip/hip_runtime.h>

#include "../common.h"
#include "claims_dev.h"
#include "launch.h"
#include "storage_runs.h"

namespace ipcfp {

// 2^lg lanes per run.  The table is untrusted: run i is SOUND when it is not empty, starts at 0 (i = 0), ends where run
// i + 1 starts — or at n, the last one — and ends inside [0, n]; only a sound run's claims are written, so no store leaves
// run_of[0, n) whatever the table says, and the reads are records i and i + 1 < n_runs.  All runs sound ⇒ by induction
// they tile [0, n) in order and every run_of[t] is written exactly once.  Any other ⇒ *bad, and the caller reports
// IPCFP_E_INVALID without looking at run_of.
__global__ __launch_bounds__(256) void k_storage_column_runs(const StorageRunRec* __restrict__ tab, uint32_t n_runs, uint32_t n, uint32_t lg,
                                                             uint32_t* __restrict__ run_of, StorageRun* __restrict__ runs,
                                                             uint32_t* __restrict__ bad) {
    const uint64_t g = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x;
    if ((g >> lg) >= n_runs) return;
    const uint32_t i = uint32_t(g >> lg), l = uint32_t(g) & ((1u << lg) - 1u);
    const uint32_t first = tab[i].first_claim, cnt = tab[i].n_claims;
    const uint64_t end = uint64_t(first) + cnt;
    const uint64_t next = i + 1u < n_runs ? uint64_t(tab[i + 1u].first_claim) : uint64_t(n);
    const bool sound = cnt != 0u && (i != 0u || first == 0u) && end == next && end <= n;
    if (!sound) {
        if (l == 0u) atomicOr(bad, 1u);
        return;
    }
    if (l == 0u && runs) runs[i].first_claim = first;
    for (uint64_t t = uint64_t(first) + l; t < end; t += 1u << lg) run_of[t] = i;
}

// columns → StorageClaimPacked[n].  A plain record is 31 little-endian 8-byte words: 0-21 are words 0-21 of its run's
// record (epoch, actor id, the four CID slots: the same order in both), 22-25 its slot, 26-29 its value, 30 its flags
// (run's | claim's) below the reserved word.  One lane per 16 BYTES OF OUTPUT — two words, each wholly one claim's since
// 248 = 8 · 31 — so a wavefront stores 1 KB of contiguous bytes whatever the record size, and reads the slot and value
// columns contiguously; the run records are re-read by the ≈ 16 lanes of a claim out of the cache.
__device__ __forceinline__ uint64_t expanded_word(const StorageRunRec* __restrict__ tab, const uint64_t* __restrict__ slot,
                                                  const uint64_t* __restrict__ value, const uint8_t* __restrict__ cflags,
                                                  const uint32_t* __restrict__ run_of, uint64_t k) {
    const uint64_t t = k / 31u;
    const uint32_t j = uint32_t(k - t * 31u);
    if (j >= 22u && j < 26u) return slot[4u * t + (j - 22u)];
    if (j >= 26u && j < 30u) return value[4u * t + (j - 26u)];
    const StorageRunRec& r = tab[run_of[t]];
    if (j < 22u) return reinterpret_cast<const uint64_t*>(&r)[j];
    return uint64_t(r.flags | uint32_t(cflags[t])) | uint64_t(r.reserved) << 32;
}

__global__ __launch_bounds__(256) void k_storage_columns_expand(const StorageRunRec* __restrict__ tab, const uint64_t* __restrict__ slot,
                                                                const uint64_t* __restrict__ value, const uint8_t* __restrict__ cflags,
                                                                const uint32_t* __restrict__ run_of, uint64_t n_words,
                                                                uint64_t* __restrict__ out) {
    const uint64_t q = uint64_t(blockIdx.x) * blockDim.x + threadIdx.x, k = 2u * q;
    if (k >= n_words) return;
    const uint64_t a = expanded_word(tab, slot, value, cflags, run_of, k);
    if (k + 1u < n_words) {
        const uint64_t b = expanded_word(tab, slot, value, cflags, run_of, k + 1u);
        *reinterpret_cast<ulonglong2*>(out + k) = make_ulonglong2(a, b);  // (out: on a 16-byte boundary)
    } else {
        out[k] = a;  // an odd number of claims: the last record ends on an 8-byte boundary
    }
}

int launch_storage_column_runs(ipcfp_ctx* ctx, const StorageColumnsDev& cols, uint32_t n, uint32_t* run_of_d, void* runs_d, uint32_t* bad_d) {
    if (cols.n_runs == 0) return IPCFP_OK;
    uint32_t lg = 0;  // lanes per run: the mean run length rounded down to a power of two, a wavefront at the most
    while (lg < 6u && (uint64_t(cols.n_runs) << (lg + 1u)) <= n) ++lg;
    hipLaunchKernelGGL(k_storage_column_runs, dim3(div_up(uint64_t(cols.n_runs) << lg, 256)), dim3(256), 0, ctx->stream,
                       static_cast<const StorageRunRec*>(cols.runs), cols.n_runs, n, lg, run_of_d, static_cast<StorageRun*>(runs_d), bad_d);
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

int launch_expand_storage_columns(ipcfp_ctx* ctx, const StorageColumnsDev& cols, uint32_t n, const uint32_t* run_of_d, void* claims_out_d) {
    if (n == 0) return IPCFP_OK;
    const uint64_t n_words = uint64_t(n) * 31u;
    hipLaunchKernelGGL(k_storage_columns_expand, dim3(div_up((n_words + 1u) / 2u, 256)), dim3(256), 0, ctx->stream,
                       static_cast<const StorageRunRec*>(cols.runs), reinterpret_cast<const uint64_t*>(cols.slot),
                       reinterpret_cast<const uint64_t*>(cols.value), cols.cflags, run_of_d, n_words, static_cast<uint64_t*>(claims_out_d));
    IPCFP_HIP(ctx, hipGetLastError());
    return IPCFP_OK;
}

}  // namespace ipcfp
