// csrc/kernels/base64_encode.hip — witness arena → the `blocks` part of a bundle's JSON text.
//
// The mirror of base64.hip: `serialize_base64` (src/proofs/common/bundle.rs:22-28: `B64.encode(data)`, base64 0.21's
// STANDARD engine, '=' padding) for every listed block at once, plus the frame serde_json writes around it:
//     {"cid":[1,113,160,…],"data":"<base64>"}   and a ',' behind every block but the last.
// The text is compact, so the base64 body of a block starts at an ARBITRARY byte of the output.
//
//   k_bundle_block_sizes   one lane per list position: bounds check of the id, CID length and validity from the slot,
//                          the text length of the position's piece, the offset of the base64 body inside it
//   (prefix sums)          64-bit text offsets (scan.hip launch_scan_u64), 16-character unit prefix (launch_scan_u32)
//   k_bundle_write_frames  one lane per position: everything of the piece but the base64 body
//   k_base64_encode        one lane per 12 source bytes → 16 characters
//
// Store form of k_base64_encode: a lane's 16 characters go out as 1-3 head bytes, three ALIGNED dwords
// and 1-3 tail bytes (four aligned dwords when the body happens to sit on a dword boundary).  The bytes one lane's tail
// leaves open in a dword are the head bytes of the next lane, so every byte of the body is written exactly once and
// nothing is read back.
#include <hip/hip_runtime.h>

#include "../common.h"
#include "launch.h"

namespace ipcfp {

// per list position, written by k_bundle_block_sizes
struct EncPos {
    uint64_t src;   // arena offset of the block
    uint32_t len;   // its length in bytes
    uint32_t body;  // offset of the base64 body inside the piece | CID length << 16
};

// error codes of the block part (low two bits of the error word; the position sits above them)
constexpr uint32_t kEncBadId = 1, kEncFolded = 2, kEncBadCid = 3;

__device__ __forceinline__ bool enc_uvarint(const uint8_t* p, uint32_t n, uint32_t& pos, uint64_t& v) {
    // the rule of uvarint_dev (base64.hip): at most 9 bytes, minimal form
    v = 0;
    for (int i = 0; i < 9 && pos < n; ++i) {
        const uint8_t b = p[pos++];
        v |= uint64_t(b & 0x7f) << (7 * i);
        if (!(b & 0x80)) return !(b == 0 && i > 0);
    }
    return false;
}

// The length of the CID a 40-byte slot holds, from its own varints (`Cid::try_from`: CIDv0 = 12 20 + 32 bytes, else
// v1 ‖ codec ‖ multihash code ‖ digest size ‖ digest); 0: not one well-formed CID followed by zero padding.
__device__ __forceinline__ uint32_t slot_cid_len(const uint8_t* s) {
    uint32_t n;
    if (s[0] == 0x12 && s[1] == 0x20) {
        n = 34;
    } else {
        uint32_t pos = 0;
        uint64_t version, codec, code, size;
        if (!enc_uvarint(s, IPCFP_CID_SLOT, pos, version) || version != 1 || !enc_uvarint(s, IPCFP_CID_SLOT, pos, codec) ||
            !enc_uvarint(s, IPCFP_CID_SLOT, pos, code) || !enc_uvarint(s, IPCFP_CID_SLOT, pos, size) || size > 64 ||
            pos + size > IPCFP_CID_SLOT)
            return 0;
        n = pos + uint32_t(size);
    }
    for (uint32_t i = n; i < IPCFP_CID_SLOT; ++i)
        if (s[i]) return 0;
    return n;
}

__global__ __launch_bounds__(256) void k_bundle_block_sizes(const uint32_t* __restrict__ ids, uint32_t n, uint32_t n_witness,
                                                            const uint64_t* __restrict__ off, const uint32_t* __restrict__ len,
                                                            const uint8_t* __restrict__ cids, EncPos* __restrict__ pos_out,
                                                            uint64_t* __restrict__ size_out, uint32_t* __restrict__ units_out,
                                                            unsigned long long* __restrict__ first_bad) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t id = ids ? ids[p] : p;
    uint32_t err = 0, cid_len = 0, digits = 0, blen = 0;
    uint64_t src = 0;
    if (id >= n_witness) {
        err = kEncBadId;
    } else {
        uint8_t s[IPCFP_CID_SLOT];
        const uint64_t* sp = reinterpret_cast<const uint64_t*>(cids + size_t(id) * IPCFP_CID_SLOT);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const uint64_t v = sp[j];
#pragma unroll
            for (int b = 0; b < 8; ++b) s[8 * j + b] = uint8_t(v >> (8 * b));
        }
        if (s[0] == 0xff) err = kEncFolded;
        else if (!(cid_len = slot_cid_len(s))) err = kEncBadCid;
        else {
            for (uint32_t i = 0; i < cid_len; ++i) digits += s[i] >= 100 ? 3u : s[i] >= 10 ? 2u : 1u;
            src = off[id];
            blen = len[id];
        }
    }
    if (err) atomicMin(first_bad, ((unsigned long long)p << 2) | err);
    // {"cid":[  digits and commas  ],"data":"  base64  "}  and the separating comma
    const uint32_t body = 8u + digits + (cid_len ? cid_len - 1u : 0u) + 10u;
    const uint64_t b64 = 4ull * ((uint64_t(blen) + 2u) / 3u);
    pos_out[p] = EncPos{src, blen, body | (cid_len << 16)};
    size_out[p] = err ? 0ull : uint64_t(body) + b64 + 2u + (p + 1u < n ? 1u : 0u);
    units_out[p] = err ? 0u : (blen + 11u) / 12u;
}

__global__ __launch_bounds__(256) void k_bundle_write_frames(const uint32_t* __restrict__ ids, uint32_t n,
                                                             const uint8_t* __restrict__ cids, const EncPos* __restrict__ pos,
                                                             const uint64_t* __restrict__ text_off, uint8_t* __restrict__ text) {
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const uint32_t id = ids ? ids[p] : p;
    const EncPos e = pos[p];
    const uint32_t cid_len = e.body >> 16, body = e.body & 0xffffu;
    uint8_t* o = text + text_off[p];
    const char head[8] = {'{', '"', 'c', 'i', 'd', '"', ':', '['};
    for (int i = 0; i < 8; ++i) o[i] = uint8_t(head[i]);
    uint32_t at = 8;
    const uint8_t* s = cids + size_t(id) * IPCFP_CID_SLOT;
    for (uint32_t i = 0; i < cid_len; ++i) {
        const uint32_t v = s[i];
        if (i) o[at++] = ',';
        if (v >= 100) o[at++] = uint8_t('0' + v / 100u);
        if (v >= 10) o[at++] = uint8_t('0' + (v / 10u) % 10u);
        o[at++] = uint8_t('0' + v % 10u);
    }
    const char mid[10] = {']', ',', '"', 'd', 'a', 't', 'a', '"', ':', '"'};
    for (int i = 0; i < 10; ++i) o[at + i] = uint8_t(mid[i]);
    // (at + 10 == body by construction: both count the same digits)
    uint8_t* t = o + body + 4ull * ((uint64_t(e.len) + 2u) / 3u);
    t[0] = '"';
    t[1] = '}';
    if (p + 1u < n) t[2] = ',';
}

// Three data bytes (little-endian in the low 24 bits of t) → four base64 characters (first character in byte 0).
// The inverse of b64_sextets4 (base64.hip): SWAR on a dword, class by arithmetic.
//   0..25 → 'A'.. (+65)   26..51 → 'a'.. (+71)   52..61 → '0'.. (-4)   62 → '+' (-19)   63 → '/' (-16)
__device__ __forceinline__ uint32_t b64_chars4(uint32_t t) {
    const uint32_t b0 = t & 0xffu, b1 = (t >> 8) & 0xffu, b2 = (t >> 16) & 0xffu;
    const uint32_t s = (b0 >> 2) | ((((b0 & 3u) << 4) | (b1 >> 4)) << 8) | ((((b1 & 15u) << 2) | (b2 >> 6)) << 16) |
                       ((b2 & 63u) << 24);
    const uint32_t H = 0x80808080u, L = 0x01010101u;
    auto ge = [&](uint32_t k) { return ((s + (0x80u - k) * L) & H) >> 7; };  // 0/1 per byte; s < 64 per byte: no carry out
    const uint32_t g26 = ge(26), g52 = ge(52), g62 = ge(62), g63 = ge(63);
    // offset(s) = 65 + 6·[s≥26] − 75·[s≥52] − 15·[s≥62] + 3·[s≥63]; the positive part stays below 256 per byte and is
    // at least 123 wherever the negative part (≤ 90) is not zero, so neither half carries or borrows across bytes
    return (s + 65u * L + 6u * g26 + 3u * g63) - (75u * g52 + 15u * g62);
}

// One lane per 12-byte unit; a wavefront owns 64 CONSECUTIVE units, finds its first position by a wave-uniform binary
// search over the unit prefix and the lanes walk forward from there, as the decoder does.
__global__ __launch_bounds__(256) void k_base64_encode(const uint8_t* __restrict__ arena, const EncPos* __restrict__ pos,
                                                       const uint32_t* __restrict__ unit0, uint32_t n, uint32_t n_units,
                                                       const uint64_t* __restrict__ text_off, uint8_t* __restrict__ text) {
    const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t u_first = __builtin_amdgcn_readfirstlane(u & ~63u);
    if (u_first >= n_units) return;
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (unit0[mid] <= u_first) lo = mid;
        else hi = mid;
    }
    if (u >= n_units) return;
    // positions with zero units (empty blocks) share unit0 with their successor: skip them
    while (lo + 1 < n && unit0[lo + 1] <= u) ++lo;
    const EncPos e = pos[lo];
    const uint32_t k = u - unit0[lo];
    const uint32_t b0 = k * 12u;
    const uint32_t r = min(12u, e.len - b0);  // 1..12 source bytes of this unit
    // every block starts on a 128-byte line and 12·k is a multiple of 4: aligned dword loads; the last unit reads only
    // the dwords its bytes lie in
    const uint32_t* sp = reinterpret_cast<const uint32_t*>(arena + e.src + b0);
    uint32_t w0 = sp[0], w1 = r > 4 ? sp[1] : 0u, w2 = r > 8 ? sp[2] : 0u;
    uint8_t* dst = text + text_off[lo] + (e.body & 0xffffu) + uint64_t(k) * 16u;
    if (r == 12u) {
        const uint32_t c0 = b64_chars4(w0 & 0xffffffu), c1 = b64_chars4((w0 >> 24) | ((w1 & 0xffffu) << 8)),
                       c2 = b64_chars4((w1 >> 16) | ((w2 & 0xffu) << 16)), c3 = b64_chars4(w2 >> 8);
        const uint32_t sh = uint32_t(reinterpret_cast<uintptr_t>(dst) & 3u);
        if (sh == 0) {
            uint32_t* q = reinterpret_cast<uint32_t*>(dst);
            q[0] = c0;
            q[1] = c1;
            q[2] = c2;
            q[3] = c3;
        } else {
            const uint32_t hb = 4u - sh;                     // head bytes in front of the first aligned dword
            const uint32_t up = hb * 8u, down = sh * 8u;
            for (uint32_t i = 0; i < hb; ++i) dst[i] = uint8_t(c0 >> (8u * i));
            uint32_t* q = reinterpret_cast<uint32_t*>(dst + hb);
            q[0] = (c0 >> up) | (c1 << down);
            q[1] = (c1 >> up) | (c2 << down);
            q[2] = (c2 >> up) | (c3 << down);
            uint8_t* t = dst + hb + 12u;
            for (uint32_t i = 0; i < sh; ++i) t[i] = uint8_t(c3 >> (up + 8u * i));
        }
        return;
    }
    // the block's last unit, 1..11 bytes: the bytes behind the block's end are not the block's
    const uint32_t keep = r & 3u ? (1u << (8u * (r & 3u))) - 1u : 0xffffffffu;
    if (r <= 4) w0 &= keep;
    else if (r <= 8) w1 &= keep;
    else w2 &= keep;
    // (two 64-bit words shifted down a character at a time: no indexed register array, no scratch)
    uint64_t clo = uint64_t(b64_chars4(w0 & 0xffffffu)) | (uint64_t(b64_chars4((w0 >> 24) | ((w1 & 0xffffu) << 8))) << 32);
    uint64_t chi = uint64_t(b64_chars4((w1 >> 16) | ((w2 & 0xffu) << 16))) | (uint64_t(b64_chars4(w2 >> 8)) << 32);
    const uint32_t nchar = 4u * ((r + 2u) / 3u);
    const uint32_t pads = (3u - r % 3u) % 3u;
    for (uint32_t i = 0; i < nchar; ++i) {
        dst[i] = i + pads >= nchar ? uint8_t('=') : uint8_t(clo);
        clo = (clo >> 8) | (chi << 56);
        chi >>= 8;
    }
}

// sizes, text offsets, unit prefix: everything the host needs to know before it can allocate the text
int launch_bundle_block_sizes(ipcfp_ctx* ctx, const uint32_t* ids_d, uint32_t n, uint32_t n_witness, const uint64_t* off_d,
                              const uint32_t* len_d, const uint8_t* cids_d, void* pos_d, uint64_t* size_d, uint32_t* units_d,
                              uint64_t* text_off_d, uint32_t* unit0_d, uint64_t* totals_d /* [text bytes, units] */,
                              uint64_t* scratch_d /* 2·(div_up(n,1024)+1) */, unsigned long long* first_bad_d) {
    if (n == 0) {
        IPCFP_HIP(ctx, hipMemsetAsync(totals_d, 0, 2 * sizeof(uint64_t), ctx->stream));
        return IPCFP_OK;
    }
    ProfileScope prof(ctx, IPCFP_K_BASE64);
    hipLaunchKernelGGL(k_bundle_block_sizes, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, ids_d, n, n_witness, off_d, len_d,
                       cids_d, static_cast<EncPos*>(pos_d), size_d, units_d, first_bad_d);
    IPCFP_HIP(ctx, hipGetLastError());
    int rc = launch_scan_u64(ctx, size_d, n, text_off_d, totals_d, scratch_d);
    if (rc) return rc;
    return launch_scan_u32(ctx, units_d, n, unit0_d, totals_d + 1, scratch_d + div_up(n, 1024) + 1);
}

int launch_bundle_write_text(ipcfp_ctx* ctx, const uint32_t* ids_d, uint32_t n, const uint8_t* arena_d, const uint8_t* cids_d,
                             const void* pos_d, const uint64_t* text_off_d, const uint32_t* unit0_d, uint32_t n_units,
                             uint8_t* text_d) {
    if (n == 0) return IPCFP_OK;
    ProfileScope prof(ctx, IPCFP_K_BASE64);
    hipLaunchKernelGGL(k_bundle_write_frames, dim3(div_up(n, 256)), dim3(256), 0, ctx->stream, ids_d, n, cids_d,
                       static_cast<const EncPos*>(pos_d), text_off_d, text_d);
    IPCFP_HIP(ctx, hipGetLastError());
    if (n_units) {
        hipLaunchKernelGGL(k_base64_encode, dim3(div_up(n_units, 256)), dim3(256), 0, ctx->stream, arena_d,
                           static_cast<const EncPos*>(pos_d), unit0_d, n, n_units, text_off_d, text_d);
        IPCFP_HIP(ctx, hipGetLastError());
    }
    return IPCFP_OK;
}

}  // namespace ipcfp
