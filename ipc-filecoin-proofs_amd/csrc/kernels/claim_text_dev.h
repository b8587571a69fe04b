// csrc/kernels/claim_text_dev.h — the characters of a claim's JSON text as functions of its packed binary fields: what
// `serde_json::to_string` writes for the integers of a StorageProof / EventProof (src/proofs/storage/bundle.rs:5-14,
// src/proofs/events/bundle.rs:5-23), `format!("0x{}", hex::encode(..))` for slot, value, topics and data
// (src/proofs/common/evm.rs:41-58) and `Cid::to_string()` for every CID: "b" + base32-lower without padding for a CIDv1,
// base58btc for a CIDv0.
//
// Two forms of every primitive:
//   *_len / put_*   the length of a field's text, and the text written front to back through a byte pointer (the per-run
//                   fragments of kernels/claim_text.hip, host/bundle_write_packed.cpp's per-tipset fragments);
//   *_char          character k of the text on its own, for a lane that owns 16 bytes of the output and starts in the
//                   middle of a field (k_claim_text_write).
// No table in memory: digits, hex, base32 and base58 characters are arithmetic on the value (kernels/base64_encode.hip
// b64_chars4 is the precedent).
//
// Everything here is plain C++ over byte pointers so that the same code runs on the device and in
// tests/native/claim_text_harness.cpp on the host (tests/test_claim_text_host.py), the idiom of hamt_outline.h.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define IPCFP_CT_FN __host__ __device__ __forceinline__
#else
#define IPCFP_CT_FN inline
#endif

namespace ipcfp {
namespace claimtext {

constexpr uint32_t kSlotBytes = 40;  // IPCFP_CID_SLOT

// ---- decimal ----------------------------------------------------------------------------------------------------------------
IPCFP_CT_FN uint32_t dec_len_u64(uint64_t v) {
    uint32_t n = 1;
    while (v >= 10u) {
        v /= 10u;
        ++n;
    }
    return n;
}
IPCFP_CT_FN uint64_t magnitude(int64_t v) { return v < 0 ? uint64_t(0) - uint64_t(v) : uint64_t(v); }  // (INT64_MIN: 2^63)
IPCFP_CT_FN uint32_t dec_len_i64(int64_t v) { return dec_len_u64(magnitude(v)) + (v < 0 ? 1u : 0u); }
// character k (0: the most significant) of the nd = dec_len_u64(v) digits of v
IPCFP_CT_FN uint8_t dec_char_u64(uint64_t v, uint32_t nd, uint32_t k) {
    for (uint32_t j = nd - 1u - k; j; --j) v /= 10u;
    return uint8_t('0' + uint32_t(v % 10u));
}
IPCFP_CT_FN uint8_t dec_char_i64(int64_t v, uint32_t nd, uint32_t k) {
    if (v >= 0) return dec_char_u64(uint64_t(v), nd, k);
    return k == 0u ? uint8_t('-') : dec_char_u64(magnitude(v), nd - 1u, k - 1u);
}
IPCFP_CT_FN uint32_t put_u64(uint8_t* o, uint64_t v) {
    const uint32_t nd = dec_len_u64(v);
    for (uint32_t k = nd; k--;) {
        o[k] = uint8_t('0' + uint32_t(v % 10u));
        v /= 10u;
    }
    return nd;
}
IPCFP_CT_FN uint32_t put_i64(uint8_t* o, int64_t v) {
    if (v >= 0) return put_u64(o, uint64_t(v));
    o[0] = '-';
    return 1u + put_u64(o + 1, magnitude(v));
}

// ---- "0x" + lowercase hex ---------------------------------------------------------------------------------------------------
IPCFP_CT_FN uint8_t hex_digit(uint32_t nibble) { return uint8_t(nibble + (nibble < 10u ? uint32_t('0') : uint32_t('a') - 10u)); }
// character k of the 2n hex digits of p[0, n)
IPCFP_CT_FN uint8_t hex_char(const uint8_t* p, uint64_t k) {
    const uint32_t b = p[k >> 1];
    return hex_digit(k & 1u ? b & 15u : b >> 4);
}
IPCFP_CT_FN uint32_t put_hex0x(uint8_t* o, const uint8_t* p, uint32_t n) {
    o[0] = '0';
    o[1] = 'x';
    for (uint32_t k = 0; k < 2u * n; ++k) o[2u + k] = hex_char(p, k);
    return 2u + 2u * n;
}

// ---- base32-lower, multibase 'b', no padding: a CIDv1 of 1-40 bytes ------------------------------------------------------------
// RFC 4648 lower-case alphabet: 0-25 'a'-'z', 26-31 '2'-'7'
IPCFP_CT_FN uint8_t b32_digit(uint32_t v) { return uint8_t(v < 26u ? uint32_t('a') + v : uint32_t('2') + (v - 26u)); }
IPCFP_CT_FN uint32_t b32_len(uint32_t len) { return 1u + (8u * len + 4u) / 5u; }  // 'b' + ceil(8 len / 5)
// character k of the b32_len(len) characters; the last group of a 1-4 byte tail is filled up with zero bits
IPCFP_CT_FN uint8_t b32_char(const uint8_t* cid, uint32_t len, uint32_t k) {
    if (k == 0u) return 'b';
    const uint32_t bit = 5u * (k - 1u), i = bit >> 3, sh = bit & 7u;
    const uint32_t w = (uint32_t(cid[i]) << 8) | (i + 1u < len ? uint32_t(cid[i + 1u]) : 0u);  // the 16 bits from byte i on
    return b32_digit((w >> (11u - sh)) & 31u);
}

// ---- base58btc: a CIDv0, 12 20 ‖ sha2-256 digest -----------------------------------------------------------------------------
// The 34 bytes are a 272-bit number v with 0x12·256^33 <= v < 0x13·256^33.  58^45 <= 0x12·256^33 and 0x13·256^33 <= 58^46,
// so v always has exactly 46 base-58 digits — the first is never '1' (a zero), and no leading zero BYTE exists to add one.
constexpr uint32_t kB58Len = 46;
struct Pow58 {
    uint32_t w[9];  // little-endian 32-bit limbs: 288 bits
};
constexpr Pow58 pow58(int e) {
    Pow58 r{{1, 0, 0, 0, 0, 0, 0, 0, 0}};
    for (int i = 0; i < e; ++i) {
        uint64_t carry = 0;
        for (int j = 0; j < 9; ++j) {
            const uint64_t t = uint64_t(r.w[j]) * 58u + carry;
            r.w[j] = uint32_t(t);
            carry = t >> 32;
        }
    }
    return r;
}
// limb 8 holds bits 256-287; 0x12·256^33 = 0x1200 << 256 exactly, 0x13·256^33 = 0x1300 << 256
static_assert(pow58(45).w[8] < 0x1200u, "58^45 <= 0x12·256^33: a CIDv0 has at least 46 base-58 digits");
static_assert(pow58(46).w[8] >= 0x1300u, "0x13·256^33 <= 58^46: a CIDv0 has at most 46 base-58 digits");
// 1-9, A-H, J-N, P-Z, a-k, m-z
IPCFP_CT_FN uint8_t b58_digit(uint32_t v) {
    if (v < 9u) return uint8_t('1' + v);
    if (v < 17u) return uint8_t('A' + (v - 9u));
    if (v < 22u) return uint8_t('J' + (v - 17u));
    if (v < 33u) return uint8_t('P' + (v - 22u));
    if (v < 44u) return uint8_t('a' + (v - 33u));
    return uint8_t('m' + (v - 44u));
}
// the 34 bytes as big-endian limbs, most significant first: limb 0 holds bytes 0-1, limb i bytes 4i-2 … 4i+1
IPCFP_CT_FN void b58_load(const uint8_t* cid, uint32_t limb[9]) {
    limb[0] = (uint32_t(cid[0]) << 8) | cid[1];
    for (int i = 1; i < 9; ++i)
        limb[i] = (uint32_t(cid[4 * i - 2]) << 24) | (uint32_t(cid[4 * i - 1]) << 16) | (uint32_t(cid[4 * i]) << 8) | cid[4 * i + 1];
}
IPCFP_CT_FN uint32_t b58_divide(uint32_t limb[9]) {  // limb /= 58, → the remainder
    uint64_t rem = 0;
    for (int i = 0; i < 9; ++i) {
        const uint64_t cur = (rem << 32) | limb[i];
        limb[i] = uint32_t(cur / 58u);
        rem = cur % 58u;
    }
    return uint32_t(rem);
}
IPCFP_CT_FN uint32_t put_b58_cidv0(uint8_t* o, const uint8_t* cid) {
    uint32_t limb[9];
    b58_load(cid, limb);
    for (uint32_t d = kB58Len; d--;) o[d] = b58_digit(b58_divide(limb));
    return kB58Len;
}
// character k of the 46 on its own: the divisions down to it (a CIDv0 is rare where this runs: Filecoin's CIDs are v1)
IPCFP_CT_FN uint8_t b58_cidv0_char(const uint8_t* cid, uint32_t k) {
    uint32_t limb[9];
    b58_load(cid, limb);
    uint32_t r = 0;
    for (uint32_t d = kB58Len; d-- > k;) r = b58_divide(limb);
    return b58_digit(r);
}

// ---- the CID a 40-byte slot holds -------------------------------------------------------------------------------------------
// `Cid::try_from(bytes)` as host/cidstr.cpp cid_binary_ok states it: CIDv0 = exactly 12 20 ‖ 32 bytes; else version 1, codec,
// multihash code, digest size (minimal varints of at most 9 bytes, size <= 64), then exactly `size` bytes
IPCFP_CT_FN bool uvarint(const uint8_t* p, uint32_t n, uint32_t& pos, uint64_t& v) {
    v = 0;
    for (int shift = 0; shift < 63; shift += 7) {
        if (pos >= n) return false;
        const uint8_t c = p[pos++];
        v |= uint64_t(c & 0x7fu) << shift;
        if (!(c & 0x80u)) return !(c == 0 && shift > 0);
    }
    return false;
}
IPCFP_CT_FN bool cid_binary_ok(const uint8_t* p, uint32_t n) {
    if (n == 34u && p[0] == 0x12 && p[1] == 0x20) return true;
    uint32_t pos = 0;
    uint64_t version, codec, code, size;
    if (!uvarint(p, n, pos, version) || version != 1u) return false;
    if (!uvarint(p, n, pos, codec) || !uvarint(p, n, pos, code)) return false;
    if (!uvarint(p, n, pos, size) || size > 64u) return false;
    return n - pos == size;
}
// The rule of host/unpack_claims.cpp slot_cid_len: the length of the one CID the slot holds in front of zero padding;
// 0: the slot is not that; -1: a fold (0xff …: the CID was longer than the slot and only its hash is left)
IPCFP_CT_FN int slot_cid_len(const uint8_t* slot) {
    if (slot[0] == 0xff) return -1;
    uint32_t len = 34;
    if (!(slot[0] == 0x12 && slot[1] == 0x20)) {
        uint32_t pos = 0;
        uint64_t size = 0;
        for (int f = 0; f < 4; ++f) {
            bool done = false;
            size = 0;
            for (int i = 0; i < 9 && pos < kSlotBytes && !done; ++i) {
                const uint8_t b = slot[pos++];
                size |= uint64_t(b & 0x7fu) << (7 * i);
                done = !(b & 0x80u);
            }
            if (!done) return 0;
        }
        if (size > uint64_t(kSlotBytes - pos)) return 0;
        len = pos + uint32_t(size);
    }
    for (uint32_t i = len; i < kSlotBytes; ++i)
        if (slot[i]) return 0;
    return cid_binary_ok(slot, len) ? int(len) : 0;
}

// ---- `Cid::to_string()` of a slot's CID (len = slot_cid_len(slot) > 0) ---------------------------------------------------------
IPCFP_CT_FN bool cid_is_v0(const uint8_t* cid, uint32_t len) { return len == 34u && cid[0] == 0x12 && cid[1] == 0x20; }
IPCFP_CT_FN uint32_t cid_str_len(const uint8_t* cid, uint32_t len) { return cid_is_v0(cid, len) ? kB58Len : b32_len(len); }
IPCFP_CT_FN uint8_t cid_str_char(const uint8_t* cid, uint32_t len, uint32_t k) {
    return cid_is_v0(cid, len) ? b58_cidv0_char(cid, k) : b32_char(cid, len, k);
}
IPCFP_CT_FN uint32_t put_cid_str(uint8_t* o, const uint8_t* cid, uint32_t len) {
    if (cid_is_v0(cid, len)) return put_b58_cidv0(o, cid);
    const uint32_t n = b32_len(len);
    for (uint32_t k = 0; k < n; ++k) o[k] = b32_char(cid, len, k);
    return n;
}
// a literal without its NUL
template <uint32_t N>
IPCFP_CT_FN uint32_t put_lit(uint8_t* o, const char (&s)[N]) {
    for (uint32_t k = 0; k + 1u < N; ++k) o[k] = uint8_t(s[k]);
    return N - 1u;
}

}  // namespace claimtext
}  // namespace ipcfp
