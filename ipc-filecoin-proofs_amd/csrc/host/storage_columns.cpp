// csrc/host/storage_columns.cpp — StorageProof claims in run-compressed, column form (include/ipcfp.h "storage claims in
// run-compressed, column form"): the host-side conversion both ways, and the entry points that verify or expand the form
// on the device (kernels/storage_columns.hip, the column instantiations of kernels/verify_storage.hip).
//
// Reference counterpart: the `storage_proofs` of a UnifiedProofBundle (src/proofs/common/bundle.rs:36-45,
// src/proofs/storage/bundle.rs:5-14) handed to `verify_proof_bundle` (src/proofs/verifier.rs:19-28), which walks them in
// order — a contract's proofs stand next to each other and repeat 176 of a packed claim's 248 bytes.
#include <algorithm>
#include <cstring>
#include <new>
#include <thread>
#include <vector>

#include "../common.h"
#include "../kernels/claims_dev.h"
#include "../kernels/launch.h"
#include "../kernels/storage_runs.h"
#include "parallel.h"

using namespace ipcfp;

// One allocation, so that it crosses PCIe as one copy: [run table 192 · n_runs | slot 32 n | value 32 n | cflags n]; every
// section starts on a 16-byte boundary of the buffer (192 and 32 are multiples of 16).
struct ipcfp_storage_columns {
    std::vector<uint8_t> buf;
    uint64_t n = 0;
    uint32_t n_runs = 0;
    size_t off_slot() const { return size_t(n_runs) * IPCFP_SRUN_BYTES; }
    size_t off_value() const { return off_slot() + 32 * size_t(n); }
    size_t off_cflags() const { return off_value() + 32 * size_t(n); }
    size_t bytes() const { return off_cflags() + size_t(n); }
};

namespace {

constexpr size_t kKeyBytes = offsetof(StorageClaimPacked, slot);  // epoch, actor id, the four CID slots: 176 bytes
static_assert(kKeyBytes == IPCFP_SRUN_OFF_FIRST_CLAIM, "a run record starts with the claim's first 176 bytes as they are");

inline bool starts_run(const StorageClaimPacked* c, uint64_t i) {
    return i == 0 || std::memcmp(&c[i], &c[i - 1], kKeyBytes) != 0 || ((c[i].flags ^ c[i - 1].flags) & IPCFP_SRUN_FLAG_MASK);
}

unsigned parts_for(uint64_t n) {
    unsigned hw = std::thread::hardware_concurrency();
    if (hw == 0) hw = 1;
    return unsigned(std::max<uint64_t>(1, std::min<uint64_t>({uint64_t(hw), kMaxParts, n / 4096})));
}

StorageColumnsDev columns_dev(const void* runs_d, uint32_t n_runs, const void* slot_d, const void* value_d, const void* cflags_d) {
    return StorageColumnsDev{runs_d, n_runs, static_cast<const uint8_t*>(slot_d), static_cast<const uint8_t*>(value_d),
                             static_cast<const uint8_t*>(cflags_d)};
}

// what the host can say about the arguments before a kernel sees them (the table's CONTENT is checked where it is)
int check_columns_args(ipcfp_ctx* ctx, const void* runs_d, uint32_t n_runs, const void* slot_d, const void* value_d, const void* cflags_d,
                       uint64_t n) {
    if (n >= 0xffffffffULL) return set_error(ctx, IPCFP_E_UNSUPPORTED, "batch too large");
    if (n && (!runs_d || !slot_d || !value_d || !cflags_d)) return IPCFP_E_INVALID;
    if ((reinterpret_cast<uintptr_t>(runs_d) | reinterpret_cast<uintptr_t>(slot_d) | reinterpret_cast<uintptr_t>(value_d)) & 15u)
        return set_error(ctx, IPCFP_E_INVALID, "the run table and the slot / value columns must lie on 16-byte boundaries");
    // every run holds a claim: more runs than claims (or none for some claims) cannot tile [0, n)
    if (n_runs > n || (n && !n_runs)) return set_error(ctx, IPCFP_E_INVALID, "%u runs cannot tile %llu claims", n_runs, (unsigned long long)n);
    return IPCFP_OK;
}

}  // namespace

extern "C" {

int ipcfp_compact_storage_claims(const ipcfp_storage_claim_t* claims, uint64_t n, ipcfp_storage_columns_t** out) {
    if (!out || (n && !claims)) return IPCFP_E_INVALID;
    *out = nullptr;
    if (n >= 0xffffffffULL) return IPCFP_E_UNSUPPORTED;
    const StorageClaimPacked* c = reinterpret_cast<const StorageClaimPacked*>(claims);
    auto* h = new (std::nothrow) ipcfp_storage_columns();
    if (!h) return IPCFP_E_NOMEM;
    h->n = n;
    const unsigned parts = parts_for(n);
    // pass 1: the runs of every part counted, and what cannot come back byte for byte refused
    uint64_t count[kMaxParts + 1] = {};
    std::atomic<bool> refused{false};
    auto count_part = [&](unsigned t) {
        const uint64_t lo = n * t / parts, hi = n * (t + 1) / parts;
        uint64_t k = 0;
        bool bad = false;
        for (uint64_t i = lo; i < hi; ++i) {
            bad |= c[i].pad != 0 || (c[i].flags & ~(IPCFP_SRUN_FLAG_MASK | IPCFP_SCOL_FLAG_MASK)) != 0;
            k += starts_run(c, i) ? 1 : 0;
        }
        count[t + 1] = k;
        if (bad) refused = true;
    };
    bool ok = run_parts(parts, count_part);
    if (ok && refused) {
        delete h;
        return IPCFP_E_UNSUPPORTED;
    }
    for (unsigned t = 0; t < parts; ++t) count[t + 1] += count[t];
    h->n_runs = uint32_t(count[parts]);
    if (ok) {
        try {
            h->buf.resize(h->bytes());
        } catch (...) {
            ok = false;
        }
    }
    if (!ok) {
        delete h;
        return IPCFP_E_NOMEM;
    }
    // pass 2: every part writes its claims' columns and the records of the runs that START in it; a run's length is known
    // when the next one starts (the part behind, or the end of the batch, closes a part's last run)
    uint8_t* base = h->buf.data();
    uint8_t *slot = base + h->off_slot(), *value = base + h->off_value(), *cflags = base + h->off_cflags();
    auto fill_part = [&](unsigned t) {
        const uint64_t lo = n * t / parts, hi = n * (t + 1) / parts;
        uint64_t r = count[t];  // index of the next run to start
        for (uint64_t i = lo; i < hi; ++i) {
            std::memcpy(slot + 32 * i, c[i].slot, 32);
            std::memcpy(value + 32 * i, c[i].value, 32);
            cflags[i] = uint8_t(c[i].flags & IPCFP_SCOL_FLAG_MASK);
            if (!starts_run(c, i)) continue;
            uint8_t* rec = base + size_t(r) * IPCFP_SRUN_BYTES;
            std::memcpy(rec, &c[i], kKeyBytes);
            uint64_t end = i + 1;  // (runs into the parts behind: they own no record of it)
            while (end < n && !starts_run(c, end)) ++end;
            const uint32_t tail[4] = {uint32_t(i), uint32_t(end - i), c[i].flags & IPCFP_SRUN_FLAG_MASK, 0u};
            std::memcpy(rec + IPCFP_SRUN_OFF_FIRST_CLAIM, tail, sizeof tail);
            ++r;
        }
    };
    if (!run_parts(parts, fill_part)) {
        delete h;
        return IPCFP_E_NOMEM;
    }
    *out = h;
    return IPCFP_OK;
}

void ipcfp_storage_columns_destroy(ipcfp_storage_columns_t* c) { delete c; }
uint64_t ipcfp_storage_columns_count(const ipcfp_storage_columns_t* c) { return c ? c->n : 0; }
const uint8_t* ipcfp_storage_columns_runs(const ipcfp_storage_columns_t* c, uint32_t* n_runs) {
    if (n_runs) *n_runs = c ? c->n_runs : 0;
    return c ? c->buf.data() : nullptr;
}
const uint8_t* ipcfp_storage_columns_slots(const ipcfp_storage_columns_t* c) { return c ? c->buf.data() + c->off_slot() : nullptr; }
const uint8_t* ipcfp_storage_columns_values(const ipcfp_storage_columns_t* c) { return c ? c->buf.data() + c->off_value() : nullptr; }
const uint8_t* ipcfp_storage_columns_cflags(const ipcfp_storage_columns_t* c) { return c ? c->buf.data() + c->off_cflags() : nullptr; }
uint64_t ipcfp_storage_columns_bytes(const ipcfp_storage_columns_t* c) { return c ? c->bytes() : 0; }

int ipcfp_expand_storage_claims(const ipcfp_storage_columns_t* h, ipcfp_storage_claim_t* claims_out) {
    if (!h || (h->n && !claims_out)) return IPCFP_E_INVALID;
    StorageClaimPacked* out = reinterpret_cast<StorageClaimPacked*>(claims_out);
    const uint8_t* base = h->buf.data();
    const uint8_t *slot = base + h->off_slot(), *value = base + h->off_value(), *cflags = base + h->off_cflags();
    const uint64_t n = h->n;
    const uint32_t n_runs = h->n_runs;
    const unsigned parts = unsigned(std::max<uint64_t>(1, std::min<uint64_t>(parts_for(n), n_runs)));
    std::atomic<bool> broken{false};
    auto work = [&](unsigned t) {  // by runs: a part expands the claims of its runs
        const uint64_t lo = uint64_t(n_runs) * t / parts, hi = uint64_t(n_runs) * (t + 1) / parts;
        for (uint64_t r = lo; r < hi; ++r) {
            const uint8_t* rec = base + size_t(r) * IPCFP_SRUN_BYTES;
            uint32_t tail[4];
            std::memcpy(tail, rec + IPCFP_SRUN_OFF_FIRST_CLAIM, sizeof tail);
            if (uint64_t(tail[0]) + tail[1] > n) {  // (a handle is made by ipcfp_compact_storage_claims alone; never trusted with a store)
                broken = true;
                return;
            }
            for (uint64_t i = tail[0], e = uint64_t(tail[0]) + tail[1]; i < e; ++i) {
                std::memcpy(&out[i], rec, kKeyBytes);
                std::memcpy(out[i].slot, slot + 32 * i, 32);
                std::memcpy(out[i].value, value + 32 * i, 32);
                out[i].flags = tail[2] | cflags[i];
                out[i].pad = tail[3];
            }
        }
    };
    if (!run_parts(parts, work)) return IPCFP_E_NOMEM;
    return broken ? IPCFP_E_INVALID : IPCFP_OK;
}

int ipcfp_verify_storage_columns_device(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const void* runs_d, uint32_t n_runs, const void* slot_d,
                                        const void* value_d, const void* cflags_d, uint64_t n, const ipcfp_trust_policy_t* trust,
                                        void* status_d) {
    if (!ctx || !w || w->ctx != ctx || (n && !status_d)) return IPCFP_E_INVALID;
    if (int rc = check_columns_args(ctx, runs_d, n_runs, slot_d, value_d, cflags_d, n)) return rc;
    if (n == 0) return IPCFP_OK;
    IPCFP_ENTER(ctx);
    static const ipcfp_trust_policy_t kAcceptAll = {0, 0, 0, 0};
    int rc = launch_verify_storage_columns(ctx, w, columns_dev(runs_d, n_runs, slot_d, value_d, cflags_d), uint32_t(n),
                                           trust ? *trust : kAcceptAll, static_cast<uint8_t*>(status_d));
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    return IPCFP_OK;
}

int ipcfp_verify_storage_columns(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const ipcfp_storage_columns_t* cols,
                                 const ipcfp_trust_policy_t* trust, ipcfp_status_t* status) {
    if (!ctx || !w || w->ctx != ctx || !cols || (cols->n && !status)) return IPCFP_E_INVALID;
    const uint64_t n = cols->n;
    if (n >= 0xffffffffULL) return set_error(ctx, IPCFP_E_UNSUPPORTED, "batch too large");
    if (n == 0) return IPCFP_OK;
    if (cols->n_runs > n || !cols->n_runs) return set_error(ctx, IPCFP_E_INVALID, "%u runs cannot tile %llu claims", cols->n_runs, (unsigned long long)n);
    IPCFP_ENTER(ctx);
    static const ipcfp_trust_policy_t kAcceptAll = {0, 0, 0, 0};
    DevBuf<uint8_t> cd, sd;
    const size_t bytes = cols->bytes();
    IPCFP_HIP(ctx, cd.alloc(bytes));
    IPCFP_HIP(ctx, sd.alloc(n));
    // The form crosses PCIe on a thread of its own (one copy: the handle is one buffer) while this one queues the node
    // table, which needs only the witness; launch_verify_storage_columns joins the copy in front of the first kernel that
    // reads a run record.
    IPCFP_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (nothing queued earlier may still use the buffers just taken)
    if (bytes >= (size_t(8) << 20)) ctx->upload_task = upload_task_start(ctx, cd.p, cols->buf.data(), bytes, nullptr, nullptr, 0);
    int rc = IPCFP_OK;
    if (!ctx->upload_task) rc = upload(ctx, cd.p, cols->buf.data(), bytes, ctx->stream);
    if (!rc)
        rc = launch_verify_storage_columns(ctx, w, columns_dev(cd.p, cols->n_runs, cd.p + cols->off_slot(), cd.p + cols->off_value(), cd.p + cols->off_cflags()),
                                           uint32_t(n), trust ? *trust : kAcceptAll, sd.p, true);
    const int rc_up = upload_task_wait(ctx);  // (whatever happened: the copy must be over before the buffer goes back to the pool)
    if (rc == IPCFP_OK) rc = rc_up;
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    IPCFP_HIP(ctx, hipMemcpyAsync(status, sd.p, n, hipMemcpyDeviceToHost, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    return IPCFP_OK;
}

int ipcfp_expand_storage_claims_device(ipcfp_ctx_t* ctx, const void* runs_d, uint32_t n_runs, const void* slot_d, const void* value_d,
                                       const void* cflags_d, uint64_t n, void* claims_out_d) {
    if (!ctx || (n && !claims_out_d)) return IPCFP_E_INVALID;
    if (int rc = check_columns_args(ctx, runs_d, n_runs, slot_d, value_d, cflags_d, n)) return rc;
    if (reinterpret_cast<uintptr_t>(claims_out_d) & 15u) return set_error(ctx, IPCFP_E_INVALID, "claims_out_d must lie on a 16-byte boundary");
    if (n == 0) return IPCFP_OK;
    IPCFP_ENTER(ctx);
    const StorageColumnsDev cols = columns_dev(runs_d, n_runs, slot_d, value_d, cflags_d);
    DevBuf<uint32_t> run_of, bad_own;
    uint32_t* bad_d = nullptr;
    uint32_t bad = 0;
    IPCFP_HIP(ctx, run_of.alloc(n));
    IPCFP_HIP(ctx, ctl_words(ctx, bad_own, bad_d, 2, false));
    int rc = launch_storage_column_runs(ctx, cols, uint32_t(n), run_of.p, nullptr, bad_d);
    if (!rc) {
        IPCFP_HIP(ctx, ctl_read(ctx, &bad, bad_d, 4));
        IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));  // (run_of is whole only where the table tiles: its verdict first)
        if (bad) return set_error(ctx, IPCFP_E_INVALID, "the run table does not tile the %llu claims", (unsigned long long)n);
        rc = launch_expand_storage_columns(ctx, cols, uint32_t(n), run_of.p, claims_out_d);
    }
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    return IPCFP_OK;
}

}  // extern "C"
