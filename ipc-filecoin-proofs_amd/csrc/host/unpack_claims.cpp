// csrc/host/unpack_claims.cpp — packed event claims back to the reference's EventProof structs (strings): the inverse of
// host/pack_claims.cpp.
//
// `find_matching_events` returns finished `EventProof`s (src/proofs/events/generator.rs:262-297) whose strings are
// `format!("0x{}", hex::encode(..))` for topics and data (src/proofs/common/evm.rs:41-58) and `Cid::to_string()` for every
// CID.  The engine's generator leaves packed claims in HBM (kernels/event_claims_gen.hip); a caller that wants the wire
// form (ipcfp_bundle_write_json) or the string entry points gets the strings here.  Pure host code (no device, no context),
// in the shape of pack_claims.cpp and bundle_write.cpp: the tipsets' strings in one sequential pass (there are a handful),
// then contiguous claim ranges on run_parts threads — each range is checked and sized, then written at its place in ONE
// character arena.  IPCFP_HOST_THREADS=k pins the number of ranges.
//
// ipcfp_unpack_storage_claims is the same for `StorageProof` (src/proofs/storage/bundle.rs:5-14) as create_proof_claim spells
// it (src/proofs/storage/generator.rs:158-178): four `Cid::to_string()`s, slot and value `format!("0x{}", hex::encode(..))`.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../common.h"
#include "cidstr.h"
#include "parallel.h"

namespace ipcfp {
namespace {

constexpr uint64_t kNoBad = ~0ull;

// the CID a 40-byte slot holds: its length, 0 when the slot is not one well-formed CID + zero padding, -1 when it is a fold
int slot_cid_len(const uint8_t* slot) {
    if (slot[0] == 0xff) return -1;
    size_t len = 34;  // CIDv0: a bare sha2-256 multihash
    if (!(slot[0] == 0x12 && slot[1] == 0x20)) {
        // a binary CID is self-delimiting: version, codec, multihash code, digest size (varints), then the digest
        size_t pos = 0;
        uint64_t field[4] = {0, 0, 0, 0};
        for (int f = 0; f < 4; ++f) {
            bool done = false;
            for (int i = 0; i < 9 && pos < size_t(IPCFP_CID_SLOT) && !done; ++i) {
                const uint8_t b = slot[pos++];
                field[f] |= uint64_t(b & 0x7f) << (7 * i);
                done = !(b & 0x80);
            }
            if (!done) return 0;
        }
        if (field[3] > size_t(IPCFP_CID_SLOT) - pos) return 0;
        len = pos + size_t(field[3]);
    }
    for (size_t i = len; i < size_t(IPCFP_CID_SLOT); ++i)
        if (slot[i]) return 0;
    return cid_binary_ok(slot, len) ? int(len) : 0;
}

struct TipsetStrings {
    int rc = IPCFP_OK;  // what a claim that names this tipset is refused with
    std::vector<std::string> parents;
    std::vector<const char*> parent_ptrs;
    std::string child;
};

void hex0x(const uint8_t* p, size_t n, char* out) {  // "0x" + 2n lowercase digits + NUL
    static const char digits[] = "0123456789abcdef";
    *out++ = '0';
    *out++ = 'x';
    for (size_t i = 0; i < n; ++i) {
        *out++ = digits[p[i] >> 4];
        *out++ = digits[p[i] & 15];
    }
    *out = 0;
}

unsigned claim_threads(uint64_t n) {
    if (const char* e = std::getenv("IPCFP_HOST_THREADS")) return std::max(1u, std::min(kMaxParts, unsigned(std::atoi(e))));
    unsigned hw = std::thread::hardware_concurrency();
    if (hw == 0) hw = 1;
    return unsigned(std::max<uint64_t>(1, std::min<uint64_t>({uint64_t(hw), kMaxParts, n / 4096})));
}

}  // namespace
}  // namespace ipcfp

struct ipcfp_unpacked_events {
    std::vector<ipcfp_event_proof_t> proofs;
    std::vector<ipcfp::TipsetStrings> tipsets;
    std::vector<char> chars;               // message CID, topics and data of every proof, NUL-terminated
    std::vector<const char*> topic_ptrs;   // the proofs' topic arrays, back to back
};

using namespace ipcfp;

extern "C" {

int ipcfp_unpack_event_claims(const ipcfp_tipset_ref_t* tipsets, uint32_t n_tipsets, const ipcfp_event_claim_t* claims, uint64_t n,
                              const uint8_t* blob, uint64_t blob_len, ipcfp_unpacked_events_t** out, uint64_t* bad_index) {
    if (bad_index) *bad_index = kNoBad;
    if (!out) return IPCFP_E_INVALID;
    *out = nullptr;
    if ((n && !claims) || (n_tipsets && !tipsets) || (blob_len && !blob)) return IPCFP_E_INVALID;
    ipcfp_unpacked_events* h = new (std::nothrow) ipcfp_unpacked_events();
    if (!h) return IPCFP_E_NOMEM;
    struct Part {
        uint64_t chars = 0, topics = 0;
        uint64_t bad = kNoBad;
        int rc = IPCFP_OK;
    };
    const unsigned T = claim_threads(n);
    std::vector<Part> part;
    try {
        // ---- pass 1 (sequential): the strings of every tipset; a tipset that has none refuses the claims that name it ----
        h->tipsets.resize(n_tipsets);
        for (uint32_t k = 0; k < n_tipsets; ++k) {
            const ipcfp_tipset_ref_t& tr = tipsets[k];
            TipsetStrings& ts = h->tipsets[k];
            const uint32_t both = IPCFP_TIPSET_PARENTS_PARSED | IPCFP_TIPSET_CHILD_PARSED;
            if ((tr.flags & both) != both || tr.n_parents > uint32_t(IPCFP_MAX_PARENTS_WIDE) ||
                (tr.n_parents > uint32_t(IPCFP_MAX_PARENTS) && !tr.more_parents)) {
                ts.rc = IPCFP_E_INVALID;
                continue;
            }
            auto put = [&](const uint8_t* slot, std::string& s) {
                const int len = slot_cid_len(slot);
                if (len < 0) ts.rc = ts.rc ? ts.rc : IPCFP_E_UNSUPPORTED;
                else if (len == 0) ts.rc = ts.rc ? ts.rc : IPCFP_E_INVALID;
                else s = cid_to_string(slot, size_t(len));
            };
            ts.parents.resize(tr.n_parents);
            for (uint32_t j = 0; j < tr.n_parents && !ts.rc; ++j)
                put(j < uint32_t(IPCFP_MAX_PARENTS) ? tr.parents[j] : tr.more_parents + size_t(j - IPCFP_MAX_PARENTS) * IPCFP_CID_SLOT,
                    ts.parents[j]);
            if (!ts.rc) put(tr.child, ts.child);
            for (const std::string& s : ts.parents) ts.parent_ptrs.push_back(s.c_str());
        }
        // ---- pass 2 (parallel by contiguous ranges): every claim checked and sized ----
        part.resize(T);
        h->proofs.resize(n);
        auto size_work = [&](unsigned t) {
            Part& r = part[t];
            for (uint64_t i = n * t / T, hi = n * (t + 1) / T; i < hi; ++i) {
                const ipcfp_event_claim_t& c = claims[i];
                int rc = IPCFP_OK;
                int mlen = 0;
                const uint32_t both = IPCFP_CLAIM_MSG_PARSED | IPCFP_CLAIM_DATA_MATCHABLE;
                if (c.tipset >= n_tipsets || (c.flags & both) != both) rc = IPCFP_E_INVALID;
                else if (h->tipsets[c.tipset].rc) rc = h->tipsets[c.tipset].rc;
                else if (uint64_t(c.topics_off) + 33ull * c.n_topics > blob_len || uint64_t(c.data_off) + c.data_len > blob_len) rc = IPCFP_E_INVALID;
                else if ((mlen = slot_cid_len(c.message_cid)) <= 0) rc = mlen < 0 ? IPCFP_E_UNSUPPORTED : IPCFP_E_INVALID;
                else
                    for (uint32_t k = 0; k < c.n_topics; ++k)
                        if (blob[size_t(c.topics_off) + 33u * size_t(k)] == 0) rc = IPCFP_E_INVALID;  // the string was not "0x" + 64 hex digits: which one it was is gone
                if (rc) {
                    r.bad = i, r.rc = rc;
                    return;
                }
                // "b" + base32 of mlen bytes (or base58 of a CIDv0: never longer than that), NUL; 67 per topic; the data
                r.chars += 2 + (uint64_t(mlen) * 8 + 4) / 5 + 8;
                r.chars += 67ull * c.n_topics + 3 + 2ull * c.data_len;
                r.topics += c.n_topics ? c.n_topics : 1;
            }
        };
        if (!run_parts(T, size_work)) throw std::bad_alloc();
        for (const Part& r : part)
            if (r.bad != kNoBad) {  // ranges are in claim order: the first range with a refusal holds the lowest claim
                if (bad_index) *bad_index = r.bad;
                const int rc = r.rc;
                delete h;
                return rc;
            }
        // ---- pass 3: one arena, every range writes at its own place ----
        std::vector<uint64_t> c_at(T + 1, 0), t_at(T + 1, 0);
        for (unsigned t = 0; t < T; ++t) {
            c_at[t + 1] = c_at[t] + part[t].chars;
            t_at[t + 1] = t_at[t] + part[t].topics;
        }
        h->chars.resize(c_at[T] + 1);
        h->topic_ptrs.resize(t_at[T] + 1);
        auto write_work = [&](unsigned t) {
            char* o = h->chars.data() + c_at[t];
            const char** tp = h->topic_ptrs.data() + t_at[t];
            for (uint64_t i = n * t / T, hi = n * (t + 1) / T; i < hi; ++i) {
                const ipcfp_event_claim_t& c = claims[i];
                const TipsetStrings& ts = h->tipsets[c.tipset];
                ipcfp_event_proof_t& p = h->proofs[i];
                p.parent_epoch = c.parent_epoch;
                p.child_epoch = c.child_epoch;
                p.parent_tipset_cids = ts.parent_ptrs.data();
                p.n_parent_tipset_cids = uint32_t(ts.parent_ptrs.size());
                p.child_block_cid = ts.child.c_str();
                p.exec_index = c.exec_index;
                p.event_index = c.event_index;
                p.emitter = c.emitter;
                const std::string m = cid_to_string(c.message_cid, size_t(slot_cid_len(c.message_cid)));
                std::memcpy(o, m.c_str(), m.size() + 1);
                p.message_cid = o;
                o += m.size() + 1;
                p.topics = tp;
                p.n_topics = c.n_topics;
                for (uint32_t k = 0; k < c.n_topics; ++k) {
                    hex0x(blob + size_t(c.topics_off) + 33u * size_t(k) + 1, 32, o);
                    tp[k] = o;
                    o += 67;
                }
                tp += c.n_topics ? c.n_topics : 1;
                hex0x(c.data_len ? blob + c.data_off : nullptr, c.data_len, o);
                p.data = o;
                o += 3 + 2ull * c.data_len;
            }
        };
        if (!run_parts(T, write_work)) throw std::bad_alloc();
    } catch (...) {
        delete h;
        return IPCFP_E_NOMEM;
    }
    *out = h;
    return IPCFP_OK;
}

const ipcfp_event_proof_t* ipcfp_unpacked_events_proofs(const ipcfp_unpacked_events_t* u, uint64_t* n) {
    if (n) *n = u ? u->proofs.size() : 0;
    return u ? u->proofs.data() : nullptr;
}

void ipcfp_unpacked_events_destroy(ipcfp_unpacked_events_t* u) { delete u; }

}  // extern "C"

// ---- packed storage claims → StorageProof structs ---------------------------------------------------------------------------

struct ipcfp_unpacked_storage {
    std::vector<ipcfp_storage_proof_t> proofs;
    std::vector<char> chars;  // the six strings of every proof, NUL-terminated
};

extern "C" {

int ipcfp_unpack_storage_claims(const ipcfp_storage_claim_t* claims, uint64_t n, ipcfp_unpacked_storage_t** out, uint64_t* bad_index) {
    if (bad_index) *bad_index = kNoBad;
    if (!out) return IPCFP_E_INVALID;
    *out = nullptr;
    if (n && !claims) return IPCFP_E_INVALID;
    ipcfp_unpacked_storage* h = new (std::nothrow) ipcfp_unpacked_storage();
    if (!h) return IPCFP_E_NOMEM;
    struct Part {
        uint64_t chars = 0;
        uint64_t bad = kNoBad;
        int rc = IPCFP_OK;
    };
    const unsigned T = claim_threads(n);
    constexpr uint32_t kAll = IPCFP_SRUN_FLAG_MASK | IPCFP_SCOL_FLAG_MASK;
    // "b" + base32 of len bytes (or base58 of a CIDv0: never longer than that), NUL
    auto cid_chars = [](int len) { return 2 + (uint64_t(len) * 8 + 4) / 5 + 8; };
    try {
        std::vector<Part> part(T);
        h->proofs.resize(n);
        // ---- pass 1 (parallel by contiguous ranges): every claim checked and sized ----
        auto size_work = [&](unsigned t) {
            Part& r = part[t];
            for (uint64_t i = n * t / T, hi = n * (t + 1) / T; i < hi; ++i) {
                const ipcfp_storage_claim_t& c = claims[i];
                int rc = IPCFP_OK;
                uint64_t chars = 2 * 67;
                if (c.flags != kAll || c.reserved != 0) rc = IPCFP_E_INVALID;  // a bit missing, or bits nobody knows
                const uint8_t* slots[4] = {c.child, c.state_root, c.actor_state, c.storage_root};
                for (int k = 0; k < 4 && !rc; ++k) {
                    const int len = slot_cid_len(slots[k]);
                    if (len < 0) rc = IPCFP_E_UNSUPPORTED;
                    else if (len == 0) rc = IPCFP_E_INVALID;
                    else chars += cid_chars(len);
                }
                if (rc) {
                    r.bad = i, r.rc = rc;
                    return;
                }
                r.chars += chars;
            }
        };
        if (!run_parts(T, size_work)) throw std::bad_alloc();
        for (const Part& r : part)
            if (r.bad != kNoBad) {  // ranges are in claim order: the first range with a refusal holds the lowest claim
                if (bad_index) *bad_index = r.bad;
                const int rc = r.rc;
                delete h;
                return rc;
            }
        // ---- pass 2: one arena, every range writes at its own place ----
        std::vector<uint64_t> c_at(T + 1, 0);
        for (unsigned t = 0; t < T; ++t) c_at[t + 1] = c_at[t] + part[t].chars;
        h->chars.resize(c_at[T] + 1);
        auto write_work = [&](unsigned t) {
            char* o = h->chars.data() + c_at[t];
            auto put_cid = [&](const uint8_t* slot) {
                const std::string s = cid_to_string(slot, size_t(slot_cid_len(slot)));
                std::memcpy(o, s.c_str(), s.size() + 1);
                const char* at = o;
                o += s.size() + 1;
                return at;
            };
            for (uint64_t i = n * t / T, hi = n * (t + 1) / T; i < hi; ++i) {
                const ipcfp_storage_claim_t& c = claims[i];
                ipcfp_storage_proof_t& p = h->proofs[i];
                p.child_epoch = c.child_epoch;
                p.actor_id = c.actor_id;
                p.child_block_cid = put_cid(c.child);
                p.parent_state_root = put_cid(c.state_root);
                p.actor_state_cid = put_cid(c.actor_state);
                p.storage_root = put_cid(c.storage_root);
                hex0x(c.slot, 32, o);
                p.slot = o;
                o += 67;
                hex0x(c.value, 32, o);
                p.value = o;
                o += 67;
            }
        };
        if (!run_parts(T, write_work)) throw std::bad_alloc();
    } catch (...) {
        delete h;
        return IPCFP_E_NOMEM;
    }
    *out = h;
    return IPCFP_OK;
}

const ipcfp_storage_proof_t* ipcfp_unpacked_storage_proofs(const ipcfp_unpacked_storage_t* u, uint64_t* n) {
    if (n) *n = u ? u->proofs.size() : 0;
    return u ? u->proofs.data() : nullptr;
}

void ipcfp_unpacked_storage_destroy(ipcfp_unpacked_storage_t* u) { delete u; }

}  // extern "C"
