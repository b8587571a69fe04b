// csrc/host/bundle_write.cpp — the bundle wire format, WRITE direction: what `serde_json::to_string(&UnifiedProofBundle)`
// produces (src/proofs/common/bundle.rs:10-45, events/bundle.rs:5-23, storage/bundle.rs:4-14), compact, fields in
// declaration order.  The split mirrors the parser's (bundle.cpp): the host writes the claim strings — escaping, integers,
// the UTF-8 check a Rust `String` implies — and the device writes every ProofBlock, base64 included
// (kernels/base64_encode.hip), out of the witness that is already resident.
//
// The claims head is written in two passes over contiguous claim ranges (size, then write; host/parallel.h), the shape of
// pack_claims.cpp: a million event proofs are half a gigabyte of text.  IPCFP_HOST_THREADS=k pins the number of ranges.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../common.h"
#include "../kernels/launch.h"
#include "parallel.h"

using namespace ipcfp;

namespace {

// serde_json's ESCAPE table: 0 = copied verbatim, 'u' = \u00XX, anything else = the letter behind the backslash
struct EscapeTable {
    uint8_t t[256];
    constexpr EscapeTable() : t{} {
        for (int i = 0; i < 0x20; ++i) t[i] = 'u';
        t[0x08] = 'b';
        t[0x09] = 't';
        t[0x0a] = 'n';
        t[0x0c] = 'f';
        t[0x0d] = 'r';
        t[uint8_t('"')] = '"';
        t[uint8_t('\\')] = '\\';
    }
};
constexpr EscapeTable kEscape{};

// well-formed UTF-8 as `str::from_utf8` defines it: no overlong forms, no surrogates, nothing above U+10FFFF
bool utf8_ok(const uint8_t* s, size_t n) {
    size_t i = 0;
    while (i < n) {
        const uint8_t c = s[i];
        if (c < 0x80) {
            ++i;
            continue;
        }
        size_t need;
        uint8_t lo = 0x80, hi = 0xbf;
        if (c >= 0xc2 && c <= 0xdf) need = 1;
        else if (c >= 0xe0 && c <= 0xef) {
            need = 2;
            if (c == 0xe0) lo = 0xa0;
            if (c == 0xed) hi = 0x9f;
        } else if (c >= 0xf0 && c <= 0xf4) {
            need = 3;
            if (c == 0xf0) lo = 0x90;
            if (c == 0xf4) hi = 0x8f;
        } else {
            return false;
        }
        if (n - i <= need) return false;
        if (s[i + 1] < lo || s[i + 1] > hi) return false;
        for (size_t k = 2; k <= need; ++k)
            if ((s[i + k] & 0xc0) != 0x80) return false;
        i += need + 1;
    }
    return true;
}

// pass 1: lengths and validity; pass 2: the bytes
struct CountSink {
    static constexpr bool kCheck = true;
    uint64_t n = 0;
    void put(const char*, size_t l) { n += l; }
    void ch(char) { ++n; }
};
struct WriteSink {
    static constexpr bool kCheck = false;
    char* p;
    void put(const char* s, size_t l) {
        std::memcpy(p, s, l);
        p += l;
    }
    void ch(char c) { *p++ = c; }
};
template <class S, size_t N>
inline void lit(S& o, const char (&s)[N]) {
    o.put(s, N - 1);
}

template <class S>
void put_u64(S& o, uint64_t v) {
    char buf[20];
    int at = 20;
    do {
        buf[--at] = char('0' + v % 10);
        v /= 10;
    } while (v);
    o.put(buf + at, size_t(20 - at));
}
template <class S>
void put_i64(S& o, int64_t v) {
    if (v < 0) {
        o.ch('-');
        put_u64(o, uint64_t(0) - uint64_t(v));  // (i64::MIN included)
    } else {
        put_u64(o, uint64_t(v));
    }
}

// a JSON string; false: the pointer is NULL or (pass 1) the bytes are not UTF-8
template <class S>
bool put_string(S& o, const char* s) {
    if (!s) return false;
    const size_t n = std::strlen(s);
    const uint8_t* u = reinterpret_cast<const uint8_t*>(s);
    if (S::kCheck && !utf8_ok(u, n)) return false;
    o.ch('"');
    size_t run = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint8_t e = kEscape.t[u[i]];
        if (!e) continue;
        if (i > run) o.put(s + run, i - run);
        run = i + 1;
        if (e == 'u') {
            const char hex[] = "0123456789abcdef";
            const char esc[6] = {'\\', 'u', '0', '0', hex[u[i] >> 4], hex[u[i] & 15]};
            o.put(esc, 6);
        } else {
            const char esc[2] = {'\\', char(e)};
            o.put(esc, 2);
        }
    }
    if (n > run) o.put(s + run, n - run);
    o.ch('"');
    return true;
}
template <class S>
bool put_string_array(S& o, const char* const* a, uint32_t n) {
    if (n && !a) return false;
    o.ch('[');
    for (uint32_t k = 0; k < n; ++k) {
        if (k) o.ch(',');
        if (!put_string(o, a[k])) return false;
    }
    o.ch(']');
    return true;
}

// nullptr, or the name of the field that cannot be written
template <class S>
const char* put_storage(S& o, const ipcfp_storage_proof_t& p) {
    lit(o, "{\"child_epoch\":");
    put_i64(o, p.child_epoch);
    lit(o, ",\"child_block_cid\":");
    if (!put_string(o, p.child_block_cid)) return "child_block_cid";
    lit(o, ",\"parent_state_root\":");
    if (!put_string(o, p.parent_state_root)) return "parent_state_root";
    lit(o, ",\"actor_id\":");
    put_u64(o, p.actor_id);
    lit(o, ",\"actor_state_cid\":");
    if (!put_string(o, p.actor_state_cid)) return "actor_state_cid";
    lit(o, ",\"storage_root\":");
    if (!put_string(o, p.storage_root)) return "storage_root";
    lit(o, ",\"slot\":");
    if (!put_string(o, p.slot)) return "slot";
    lit(o, ",\"value\":");
    if (!put_string(o, p.value)) return "value";
    o.ch('}');
    return nullptr;
}
template <class S>
const char* put_event(S& o, const ipcfp_event_proof_t& p) {
    lit(o, "{\"parent_epoch\":");
    put_i64(o, p.parent_epoch);
    lit(o, ",\"child_epoch\":");
    put_i64(o, p.child_epoch);
    lit(o, ",\"parent_tipset_cids\":");
    if (!put_string_array(o, p.parent_tipset_cids, p.n_parent_tipset_cids)) return "parent_tipset_cids";
    lit(o, ",\"child_block_cid\":");
    if (!put_string(o, p.child_block_cid)) return "child_block_cid";
    lit(o, ",\"message_cid\":");
    if (!put_string(o, p.message_cid)) return "message_cid";
    lit(o, ",\"exec_index\":");
    put_u64(o, p.exec_index);
    lit(o, ",\"event_index\":");
    put_u64(o, p.event_index);
    lit(o, ",\"event_data\":{\"emitter\":");
    put_u64(o, p.emitter);
    lit(o, ",\"topics\":");
    if (!put_string_array(o, p.topics, p.n_topics)) return "event_data.topics";
    lit(o, ",\"data\":");
    if (!put_string(o, p.data)) return "event_data.data";
    lit(o, "}}");
    return nullptr;
}

constexpr char kHead0[] = "{\"storage_proofs\":[";
constexpr char kHead1[] = "],\"event_proofs\":[";
constexpr char kHead2[] = "],\"blocks\":[";

unsigned claim_threads(uint64_t n) {
    if (const char* e = std::getenv("IPCFP_HOST_THREADS"))
        return std::max(1u, std::min(kMaxParts, unsigned(std::atoi(e))));
    unsigned hw = std::thread::hardware_concurrency();
    if (hw == 0) hw = 1;
    return unsigned(std::max<uint64_t>(1, std::min<uint64_t>({uint64_t(hw), kMaxParts, n / 4096})));
}

// where every range of claims goes: range t of the storage proofs at s_at[t], of the event proofs at e_at[t]
struct ClaimsPlan {
    unsigned parts = 1;
    std::vector<uint64_t> s_at, e_at;
    uint64_t head_len = 0;
};

struct Claims {
    const ipcfp_storage_proof_t* storage;
    uint64_t n_storage;
    const ipcfp_event_proof_t* events;
    uint64_t n_events;
};

int plan_claims(const Claims& c, ClaimsPlan& plan, std::string& err) {
    const unsigned T = plan.parts = claim_threads(c.n_storage + c.n_events);
    struct Part {
        uint64_t s_bytes = 0, e_bytes = 0;
        uint64_t bad = ~0ull;  // index of the first claim of the range that cannot be written
        bool bad_is_event = false;
        const char* field = nullptr;
    };
    std::vector<Part> part(T);
    auto work = [&](unsigned t) {
        Part& r = part[t];
        CountSink o;
        for (uint64_t i = c.n_storage * t / T, hi = c.n_storage * (t + 1) / T; i < hi; ++i) {
            if (i) o.ch(',');
            if (const char* f = put_storage(o, c.storage[i])) {
                r.bad = i, r.field = f;
                return;
            }
        }
        r.s_bytes = o.n;
        o.n = 0;
        for (uint64_t i = c.n_events * t / T, hi = c.n_events * (t + 1) / T; i < hi; ++i) {
            if (i) o.ch(',');
            if (const char* f = put_event(o, c.events[i])) {
                r.bad = i, r.field = f, r.bad_is_event = true;
                return;
            }
        }
        r.e_bytes = o.n;
    };
    if (!run_parts(T, work)) {
        err = "out of memory while sizing the claims";
        return IPCFP_E_NOMEM;
    }
    // the first claim in TEXT order that cannot be written: storage proofs come first
    const Part* first = nullptr;
    for (const Part& r : part)
        if (r.bad != ~0ull && (!first || (first->bad_is_event && !r.bad_is_event))) first = &r;
    if (first) {
        err = std::string(first->bad_is_event ? "event_proofs[" : "storage_proofs[") + std::to_string(first->bad) + "]." +
              first->field + " is NULL or not well-formed UTF-8";
        return IPCFP_E_INVALID;
    }
    plan.s_at.assign(T + 1, 0);
    plan.e_at.assign(T + 1, 0);
    uint64_t at = sizeof kHead0 - 1;
    for (unsigned t = 0; t < T; ++t) {
        plan.s_at[t] = at;
        at += part[t].s_bytes;
    }
    plan.s_at[T] = at;
    at += sizeof kHead1 - 1;
    for (unsigned t = 0; t < T; ++t) {
        plan.e_at[t] = at;
        at += part[t].e_bytes;
    }
    plan.e_at[T] = at;
    plan.head_len = at + sizeof kHead2 - 1;
    return IPCFP_OK;
}

// exactly plan.head_len bytes at out
bool write_claims(const Claims& c, const ClaimsPlan& plan, char* out) {
    const unsigned T = plan.parts;
    std::memcpy(out, kHead0, sizeof kHead0 - 1);
    std::memcpy(out + plan.s_at[T], kHead1, sizeof kHead1 - 1);
    std::memcpy(out + plan.e_at[T], kHead2, sizeof kHead2 - 1);
    auto work = [&](unsigned t) {
        WriteSink o{out + plan.s_at[t]};
        for (uint64_t i = c.n_storage * t / T, hi = c.n_storage * (t + 1) / T; i < hi; ++i) {
            if (i) o.ch(',');
            (void)put_storage(o, c.storage[i]);
        }
        o.p = out + plan.e_at[t];
        for (uint64_t i = c.n_events * t / T, hi = c.n_events * (t + 1) / T; i < hi; ++i) {
            if (i) o.ch(',');
            (void)put_event(o, c.events[i]);
        }
    };
    return run_parts(T, work);
}

}  // namespace

extern "C" {

int ipcfp_bundle_write_claims_json(const ipcfp_storage_proof_t* storage, uint64_t n_storage, const ipcfp_event_proof_t* events,
                                   uint64_t n_events, char* out, uint64_t cap, uint64_t* len) {
    if (!len) return IPCFP_E_INVALID;
    *len = 0;
    if ((n_storage && !storage) || (n_events && !events) || (!out && cap)) return IPCFP_E_INVALID;
    const Claims c{storage, n_storage, events, n_events};
    ClaimsPlan plan;
    std::string err;
    const int rc = plan_claims(c, plan, err);
    if (rc) return rc;
    *len = plan.head_len;
    if (!out) return IPCFP_OK;  // the sizing call
    if (cap < plan.head_len) return IPCFP_E_INVALID;
    return write_claims(c, plan, out) ? IPCFP_OK : IPCFP_E_NOMEM;
}

int ipcfp_bundle_write_json(ipcfp_ctx_t* ctx, ipcfp_witness_t* w, const ipcfp_storage_proof_t* storage, uint64_t n_storage,
                            const ipcfp_event_proof_t* events, uint64_t n_events, const uint32_t* block_ids, uint64_t n_blocks,
                            char* out, uint64_t cap, uint64_t* len) {
    if (!ctx || !w || !len || w->ctx != ctx) return IPCFP_E_INVALID;
    *len = 0;
    IPCFP_ENTER(ctx);
    if ((n_storage && !storage) || (n_events && !events) || (!out && cap))
        return set_error(ctx, IPCFP_E_INVALID, "bundle_write_json: null claim array or null output with a capacity");
    if (!block_ids && n_blocks != w->n)
        return set_error(ctx, IPCFP_E_INVALID, "bundle_write_json: block_ids is null but n_blocks (%llu) is not the witness's block count (%llu)",
                         (unsigned long long)n_blocks, (unsigned long long)w->n);
    if (n_blocks >= 0xffffffffull) return set_error(ctx, IPCFP_E_UNSUPPORTED, "more than 2^32-2 blocks");
    const uint32_t n = uint32_t(n_blocks);

    // 1. the head's size (and whether it can be written at all)
    const Claims c{storage, n_storage, events, n_events};
    ClaimsPlan plan;
    {
        std::string err;
        const int rc = plan_claims(c, plan, err);
        if (rc) return set_error(ctx, rc, "bundle_write_json: %s", err.c_str());
    }

    // 2.-4. sizes of the block part, their prefix sums, ONE synchronisation for the total and the error word
    DevBuf<uint32_t> ids_d, units_d, unit0_d;
    DevBuf<uint64_t> pos_d /* EncPos = 2 u64 */, size_d, text_off_d, scratch_d, res_d;
    DevBuf<uint8_t> text_d;
    uint64_t res[3] = {~0ull, 0, 0};  // first error, text bytes, units
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
        if (rc) return rc;
        IPCFP_HIP(ctx, d2h_small(ctx, res, res_d.p, sizeof res, ctx->stream));
        IPCFP_HIP(ctx, sync_stream(ctx, ctx->stream));
    }
    if (res[0] != ~0ull) {
        const unsigned long long at = res[0] >> 2;
        switch (res[0] & 3u) {
            case 1:
                return set_error(ctx, IPCFP_E_INVALID, "bundle_write_json: block_ids[%llu] is not a block of the witness (%llu blocks)", at,
                                 (unsigned long long)w->n);
            case 2:
                return set_error(ctx, IPCFP_E_UNSUPPORTED,
                                 "bundle_write_json: block_ids[%llu]: the CID of this block is longer than the %d-byte slot and the "
                                 "witness keeps only its fold", at, int(IPCFP_CID_SLOT));
            default:
                return set_error(ctx, IPCFP_E_INVALID, "bundle_write_json: block_ids[%llu]: the witness's CID slot is not one well-formed CID", at);
        }
    }
    if (res[2] >= 0xfffffff0ull) return set_error(ctx, IPCFP_E_UNSUPPORTED, "bundle_write_json: more than 2^32 base64 units (48 GB of blocks)");
    const uint64_t blocks_len = res[1];
    *len = plan.head_len + blocks_len + 2;
    if (!out) return IPCFP_OK;  // the sizing call
    if (cap < *len)
        return set_error(ctx, IPCFP_E_INVALID, "bundle_write_json: the text is %llu bytes, the buffer holds %llu", (unsigned long long)*len,
                         (unsigned long long)cap);

    // 5.-6. the text of the block part, on the device; the head meanwhile on the host
    if (blocks_len) {
        IPCFP_HIP(ctx, text_d.alloc(blocks_len + 64));
        const int rc = launch_bundle_write_text(ctx, ids_d.p, n, w->arena.p, w->cids.p, pos_d.p, text_off_d.p, unit0_d.p, uint32_t(res[2]),
                                                text_d.p);
        if (rc) {
            (void)sync_stream(ctx, ctx->stream);
            return rc;
        }
    }
    const bool head_ok = write_claims(c, plan, out);
    // 7. one blocking copy behind the head
    if (blocks_len) {
        const hipError_t e = hipMemcpyAsync(out + plan.head_len, text_d.p, blocks_len, hipMemcpyDeviceToHost, ctx->stream);
        const hipError_t e2 = sync_stream(ctx, ctx->stream, true);
        IPCFP_HIP(ctx, e);
        IPCFP_HIP(ctx, e2);
    }
    if (!head_ok) return set_error(ctx, IPCFP_E_NOMEM, "bundle_write_json: out of memory while writing the claims");
    // 8. the tail
    out[plan.head_len + blocks_len] = ']';
    out[plan.head_len + blocks_len + 1] = '}';
    return IPCFP_OK;
}

}  // extern "C"
