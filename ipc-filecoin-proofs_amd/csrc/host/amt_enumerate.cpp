// csrc/host/amt_enumerate.cpp — `Amt::for_each` as a sequence of launches (kernels/amt_enum.h), and the witness's cache of
// finished enumerations.  Three steps: the roots; the dense walk when the plan allows it; otherwise the general walk,
// level by level.  Host code over launchers: it sizes the buffers, waits for what it has to see, and decides the route.
#include <cstring>
#include <memory>
#include <vector>

#include "../common.h"
#include "../kernels/amt_enum.h"
#include "../kernels/launch.h"

namespace ipcfp {

namespace {

// the call's roots on the device and on the host (the extra root, when there is one, is entry n_roots)
struct EnumRoots {
    uint32_t n_roots = 0, n_all = 0;
    DevBuf<EnumNode> frontier;         // the general walk's entries
    DevBuf<DenseNode> dense_frontier;  // … and the dense walk's
    std::vector<uint64_t> info;        // n_all × {height | bw << 32, count}; ~0: the root did not load
};

// step 1: load every root; one synchronisation brings their shapes back
int enum_roots(ipcfp_ctx* ctx, const WitnessView& view, const AmtRootSpec* roots_d, int vkind, unsigned long long* err_d, EnumRoots& r) {
    DevBuf<uint64_t> info_own;
    uint64_t* info_d = nullptr;
    IPCFP_HIP(ctx, r.frontier.alloc(r.n_all));
    IPCFP_HIP(ctx, r.dense_frontier.alloc(r.n_all));
    IPCFP_HIP(ctx, ctl_words(ctx, info_own, info_d, 2 * size_t(r.n_all), false));
    int rc = launch_enum_roots(ctx, view, roots_d, r.n_all, vkind, r.frontier.p, err_d, info_d, nullptr, 0ull, r.dense_frontier.p);
    if (rc) return rc;
    r.info.resize(2 * size_t(r.n_all));
    IPCFP_HIP(ctx, ctl_read(ctx, r.info.data(), info_d, r.info.size() * 8));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    return IPCFP_OK;
}

// step 2: the dense walk of a plan that is ok; one synchronisation brings the anomaly flag and the error word back.
// *held = false: an anomaly — the outputs are released again, and the caller walks the call's own roots the general way
// (the anomaly may be the extra root's).
int enum_dense(ipcfp_ctx* ctx, const WitnessView& view, const EnumRoots& r, const DensePlan& plan, bool want_keys,
               unsigned long long* err_d, AmtEnumResult& out, DevBuf<CidKey>* keys_out, EnumExtra* extra, bool* held) {
    const bool with_extra = plan.n_use > r.n_roots;
    DevBuf<DenseNode> a, b;
    DevBuf<uint32_t> anomaly_own;
    uint32_t* anomaly_d = nullptr;
    IPCFP_HIP(ctx, ctl_words(ctx, anomaly_own, anomaly_d, 1, false));
    IPCFP_HIP(ctx, a.alloc(plan.biggest));
    IPCFP_HIP(ctx, b.alloc(plan.biggest));
    if (want_keys) IPCFP_HIP(ctx, keys_out->alloc(plan.n_leaves));
    else IPCFP_HIP(ctx, out.leaves.alloc(plan.n_leaves));
    if (with_extra) IPCFP_HIP(ctx, extra->out->leaves.alloc(plan.n_extra));
    int rc = launch_dense_walk(ctx, view, r.dense_frontier.p, plan, a.p, b.p, want_keys ? nullptr : out.leaves.p,
                               want_keys ? keys_out->p : nullptr, with_extra ? extra->out->leaves.p : nullptr, anomaly_d);
    if (rc) return rc;
    uint32_t bad = 0;
    unsigned long long e = kNoEnumError;  // err_d is untouched by the walk: report what earlier stages left in it
    IPCFP_HIP(ctx, ctl_read(ctx, &bad, anomaly_d, 4));
    IPCFP_HIP(ctx, ctl_read(ctx, &e, err_d, 8));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    IPCFP_HIP(ctx, hipGetLastError());
    *held = !bad;
    if (bad) {
        out.leaves.release();
        if (want_keys) keys_out->release();
        if (with_extra) extra->out->leaves.release();
        return IPCFP_OK;
    }
    out.n_leaves = plan.n_leaves;
    out.error = e;
    out.dense = true;
    out.keys_written = want_keys;
    if (with_extra) {
        extra->out->n_leaves = plan.n_extra;
        extra->out->error = kNoEnumError;
        extra->out->dense = true;
        extra->out->keys_written = false;
        extra->done = true;
    }
    return IPCFP_OK;
}

// step 3: the general walk of the call's own roots — per level count, prefix sum, one synchronisation for the size of the
// next level, expand; the leaf level emits.  A last synchronisation brings the merged error word back.
int enum_general(ipcfp_ctx* ctx, const WitnessView& view, EnumRoots& r, int vkind, unsigned long long* err_d, AmtEnumResult& out,
                 uint64_t lo, uint64_t hi) {
    uint32_t max_height = 0;
    for (uint32_t i = 0; i < r.n_roots; ++i)
        if (r.info[2 * size_t(i)] != ~0ULL) {
            const uint32_t h = uint32_t(r.info[2 * size_t(i)]);
            max_height = h > max_height ? h : max_height;
        }
    DevBuf<EnumNode>& cur = r.frontier;
    DevBuf<EnumNode> nxt;
    DevBuf<uint32_t> counts, offsets;
    DevBuf<uint64_t> scratch, total_d;
    IPCFP_HIP(ctx, total_d.alloc(2));
    uint32_t n = r.n_roots;
    for (uint32_t level = max_height;; --level) {
        IPCFP_HIP(ctx, counts.alloc(n));
        IPCFP_HIP(ctx, offsets.alloc(n));
        IPCFP_HIP(ctx, scratch.alloc(size_t(div_up(n, 1024)) + 2));
        int rc = launch_enum_count(ctx, view, cur.p, n, level, vkind, counts.p, err_d, lo, hi);
        if (rc) return rc;
        rc = launch_scan_u32(ctx, counts.p, n, offsets.p, total_d.p, scratch.p);
        if (rc) return rc;
        uint64_t total = 0;
        IPCFP_HIP(ctx, d2h_small(ctx, &total, total_d.p, 8, ctx->stream));
        IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
        if (total >= 0x7fffffffULL)
            return set_error(ctx, IPCFP_E_UNSUPPORTED, "AMT enumeration expands to %llu entries", (unsigned long long)total);
        if (level >= 1) {
            IPCFP_HIP(ctx, nxt.alloc(total));
            if (total && (rc = launch_enum_expand(ctx, view, cur.p, n, level, offsets.p, uint32_t(total), nxt.p, err_d, lo, hi))) return rc;
            cur.swap(nxt);  // the old frontier returns to the pool; reuse is stream-ordered
            n = uint32_t(total);
            if (n == 0) break;
        } else {
            IPCFP_HIP(ctx, out.leaves.alloc(total));
            out.n_leaves = total;
            if (total && (rc = launch_enum_emit(ctx, view, cur.p, n, vkind, counts.p, offsets.p, out.leaves.p, lo, hi))) return rc;
            break;
        }
    }
    unsigned long long e = kNoEnumError;
    IPCFP_HIP(ctx, d2h_small(ctx, &e, err_d, 8, ctx->stream));
    IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    IPCFP_HIP(ctx, hipGetLastError());
    out.error = e;
    return IPCFP_OK;
}

}  // namespace

int amt_enumerate(ipcfp_ctx* ctx, const WitnessView& view, const AmtRootSpec* roots_d, uint32_t n_roots, int vkind,
                  unsigned long long* err_d, AmtEnumResult& out, uint64_t lo, uint64_t hi, DevBuf<CidKey>* keys_out,
                  EnumExtra* extra) {
    out.keys_written = false;
    if (extra) {
        extra->done = false;
        if (!extra->out || n_roots == 0) extra = nullptr;
    }
    out.n_leaves = 0;
    out.error = kNoEnumError;
    out.leaves.release();
    if (n_roots == 0) return IPCFP_OK;
    out.dense = false;
    ProfileScope prof(ctx, IPCFP_K_EXEC_ORDER);
    EnumRoots r;
    r.n_roots = n_roots;
    r.n_all = n_roots + (extra ? 1u : 0u);  // the extra root's spec is roots_d[n_roots]
    int rc = enum_roots(ctx, view, roots_d, vkind, err_d, r);
    if (rc) return rc;
    const bool want_keys = keys_out && vkind == VK_CID;
    DensePlan plan;
    dense_plan(r.info, n_roots, vkind, want_keys, lo, hi, extra ? 1u : 0u, extra ? extra->vkind : 0, extra ? extra->lo : 0,
               extra ? extra->hi : 0, plan);
    if (plan.ok) {
        bool held = false;
        rc = enum_dense(ctx, view, r, plan, want_keys, err_d, out, keys_out, extra, &held);
        if (rc || held) return rc;
    }
    return enum_general(ctx, view, r, vkind, err_d, out, lo, hi);  // (knows nothing of the extra root)
}

// move an enumeration result into a cache entry (the density check runs only for results of the general walk)
static int enum_cache_fill(ipcfp_ctx* ctx, EnumCached* e, AmtEnumResult& en, uint64_t lo, uint32_t* flag_p) {
    e->n = en.n_leaves;
    e->error = en.error;
    uint32_t not_dense = 0;
    if (en.n_leaves && !en.dense) {
        int rc = launch_check_dense(ctx, en.leaves.p, uint32_t(en.n_leaves), lo, flag_p);
        if (rc) return rc;
        IPCFP_HIP(ctx, ctl_read(ctx, &not_dense, flag_p, 4));
        IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    }
    e->dense = !not_dense;
    en.leaves.move_to_bytes(e->leaves);
    return IPCFP_OK;
}

static std::unique_ptr<EnumCached> enum_cache_entry(const CidKey& root, int version, int vkind, uint64_t lo, uint64_t hi) {
    std::unique_ptr<EnumCached> e(new EnumCached());
    std::memcpy(e->root, root.w, 40);
    e->version = version;
    e->vkind = vkind;
    e->lo = lo;
    e->hi = hi;
    return e;
}

int amt_enumerate_cached(ipcfp_ctx* ctx, ipcfp_witness* w, const CidKey& root, int version, int vkind,
                         const EnumCached** out, uint64_t lo, uint64_t hi) {
    for (auto& e : w->enum_cache)
        if (e->version == version && e->vkind == vkind && e->lo == lo && e->hi == hi &&
            std::memcmp(e->root, root.w, 40) == 0) {
            *out = e.get();
            return IPCFP_OK;
        }
    std::unique_ptr<EnumCached> e = enum_cache_entry(root, version, vkind, lo, hi);
    const WitnessView view = witness_view(w);
    DevBuf<AmtRootSpec> roots;
    DevBuf<unsigned long long> err_own;
    DevBuf<uint32_t> flag_own;
    unsigned long long* err_p = nullptr;  // kNoEnumError
    uint32_t* flag_p = nullptr;
    IPCFP_HIP(ctx, roots.alloc(1));
    IPCFP_HIP(ctx, ctl_words(ctx, err_own, err_p, 1, true));
    IPCFP_HIP(ctx, ctl_words(ctx, flag_own, flag_p, 1, false));
    AmtRootSpec spec{};
    spec.root = root;
    spec.version = uint32_t(version);
    IPCFP_HIP(ctx, h2d_small(ctx, roots.p, &spec, sizeof spec, ctx->stream));
    AmtEnumResult en;
    int rc = amt_enumerate(ctx, view, roots.p, 1, vkind, err_p, en, lo, hi);
    if (rc) return rc;
    rc = enum_cache_fill(ctx, e.get(), en, lo, flag_p);
    if (rc) return rc;
    *out = e.get();
    w->enum_cache.push_back(std::move(e));
    return IPCFP_OK;
}

int enum_cache_put(ipcfp_ctx* ctx, ipcfp_witness* w, const CidKey& root, int version, int vkind, uint64_t lo, uint64_t hi,
                   AmtEnumResult& en) {
    std::unique_ptr<EnumCached> e = enum_cache_entry(root, version, vkind, lo, hi);
    DevBuf<uint32_t> flag_own;
    uint32_t* flag_p = nullptr;
    IPCFP_HIP(ctx, ctl_words(ctx, flag_own, flag_p, 1, false));
    int rc = enum_cache_fill(ctx, e.get(), en, lo, flag_p);
    if (rc) return rc;
    w->enum_cache.push_back(std::move(e));
    return IPCFP_OK;
}

}  // namespace ipcfp
