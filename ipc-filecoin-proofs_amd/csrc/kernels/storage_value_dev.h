// csrc/kernels/storage_value_dev.h — left_pad_32 (src/proofs/common/evm.rs:91-100) of the serde Vec<u8> a storage HAMT holds,
// without a byte array: through the reader into four words, from plain 8-byte reads, and out of the lane's LDS slot.  Shared
// by the claim kernel of the verifier (verify_storage.hip) and the spec kernel of the generator (storage_claims_gen.hip).
#pragma once
#include "storage_dev.h"

namespace ipcfp {

// left_pad_32 (src/proofs/common/evm.rs:91-100) of a serde Vec<u8> (a CBOR array of u8, type-checked by the table) as four
// little-endian words: byte i of the padded value = word i/8, bits 8·(i%8)…
__device__ __forceinline__ void left_pad_32_words(Rd& v, uint64_t out[4]) {
    out[0] = out[1] = out[2] = out[3] = 0;
    const uint64_t n = v.read_array();
    auto put = [&](uint64_t i, uint32_t x) {
        if (n >= 32 && i < n - 32) return;
        const uint32_t j = n >= 32 ? uint32_t(i - (n - 32)) : uint32_t(32 - n + i);
        const uint64_t b = uint64_t(x & 0xffu) << (8u * (j & 7u));
        const uint32_t k = j >> 3;
        out[0] |= k == 0 ? b : 0ull;
        out[1] |= k == 1 ? b : 0ull;
        out[2] |= k == 2 ? b : 0ull;
        out[3] |= k == 3 ? b : 0ull;
    };
    uint64_t i = 0;
    while (i < n && v.ok() && v.pos + 8u <= v.n) {  // eight bytes per fetch (cbor_dev.h vec_u8_step)
        const uint64_t w = v.peek64(v.pos);
        uint32_t used = 0, x;
        while (i < n && vec_u8_step(w, used, x)) put(i++, x);
        v.pos += used;
        if (i < n && used <= 6u) put(i++, uint32_t(v.read_uint()));
    }
    for (; i < n && v.ok(); ++i) put(i, uint32_t(v.read_uint()));
}

// The same from plain 8-byte reads, for the usual spelling (`8n` | `98 nn`, elements of one or two bytes): the padded value is
// what a 32-byte shift register holds after every element has been pushed in at its low end — the last 32 elements, zeros
// above a shorter one — as eight big-endian limbs, L[0] the lowest.  false: another spelling, take the reader.
__device__ __forceinline__ bool left_pad_32_raw(const uint8_t* __restrict__ p, uint32_t avail, uint32_t L[8]) {
#pragma unroll
    for (int m = 0; m < 8; ++m) L[m] = 0;
    const uint32_t hv = p[0];
    uint32_t n, pos;
    if (hv >= 0x80u && hv < 0x98u) {
        n = hv - 0x80u;
        pos = 1u;
    } else if (hv == 0x98u) {
        n = p[1];
        pos = 2u;
    } else {
        return false;
    }
    uint32_t bad = 0;
    uint32_t q = n >> 2;
    for (; q && pos < avail; --q) {  // four elements per 8-byte read: one limb
        const uint64_t w8 = raw_ld64(p + pos);
        uint32_t cur = 0;
        vec_u8_take<4>(uint32_t(w8), uint32_t(w8 >> 32), cur, pos, bad);
#pragma unroll
        for (int m = 7; m > 0; --m) L[m] = L[m - 1];
        L[0] = cur;
    }
    if (q) return false;
    const uint32_t r = n & 3u;
    if (r) {  // the last one to three: the register moves up by as many bytes
        const uint64_t w8 = raw_ld64(p + pos);
        uint32_t cur = 0;
        if (r == 1) vec_u8_take<1>(uint32_t(w8), uint32_t(w8 >> 32), cur, pos, bad);
        else if (r == 2) vec_u8_take<2>(uint32_t(w8), uint32_t(w8 >> 32), cur, pos, bad);
        else vec_u8_take<3>(uint32_t(w8), uint32_t(w8 >> 32), cur, pos, bad);
        const uint32_t down = 32u - 8u * r;
#pragma unroll
        for (int m = 7; m > 0; --m) L[m] = __builtin_amdgcn_alignbit(L[m], L[m - 1], down);  // (L[m] << 8r) | (L[m-1] >> (32 - 8r))
        L[0] = (L[0] << (8u * r)) | cur;
    }
    if (bad || pos > avail) return false;
    return true;
}

// … and out of the lane's LDS slot, where the kernel has put the 72 bytes from the value's first byte on in ONE burst of
// loads: the decode's fetches depend on each other (an element is one or two bytes), and on global memory each was a round
// trip through an L2 that the kernel's own streaming turns over every few microseconds — lines came from memory two and
// three times (FETCH_SIZE 3.2 GB for 1 GB of claims and witness; profiles/r06_experiments.md).  A value longer than the
// stage holds (more than 32 two-byte elements) returns false like any unusual spelling.
constexpr uint32_t kValueStageWords = 10;
struct ValueStage {
    uint64_t w[kValueStageWords + 1][256];  // [word][lane]: a wavefront reading the same word index is conflict-free
};
__device__ __forceinline__ uint64_t stage_ld64(const ValueStage& vs, uint32_t lane, uint32_t at) {
    const uint32_t k = at >> 3, sh = (at & 7u) * 8u;
    const uint64_t lo = vs.w[k][lane], hi = vs.w[k + 1u][lane];
    return (lo >> sh) | ((hi << 1) << (63u - sh));
}
__device__ __forceinline__ bool left_pad_32_staged(const ValueStage& vs, uint32_t lane, uint32_t avail, uint32_t L[8]) {
#pragma unroll
    for (int m = 0; m < 8; ++m) L[m] = 0;
    const uint64_t h8 = vs.w[0][lane];
    const uint32_t hv = uint32_t(h8) & 0xffu;
    uint32_t n, pos;
    if (hv >= 0x80u && hv < 0x98u) {
        n = hv - 0x80u;
        pos = 1u;
    } else if (hv == 0x98u) {
        n = uint32_t(h8 >> 8) & 0xffu;
        pos = 2u;
    } else {
        return false;
    }
    if (n > 32u) return false;  // (≤ 2 + 64 bytes: inside the stage)
    uint32_t bad = 0;
    for (uint32_t q = n >> 2; q; --q) {  // four elements per 8 bytes: one limb
        const uint64_t w8 = stage_ld64(vs, lane, pos);
        uint32_t cur = 0;
        vec_u8_take<4>(uint32_t(w8), uint32_t(w8 >> 32), cur, pos, bad);
#pragma unroll
        for (int m = 7; m > 0; --m) L[m] = L[m - 1];
        L[0] = cur;
    }
    const uint32_t r = n & 3u;
    if (r) {  // the last one to three: the register moves up by as many bytes
        const uint64_t w8 = stage_ld64(vs, lane, pos);
        uint32_t cur = 0;
        if (r == 1) vec_u8_take<1>(uint32_t(w8), uint32_t(w8 >> 32), cur, pos, bad);
        else if (r == 2) vec_u8_take<2>(uint32_t(w8), uint32_t(w8 >> 32), cur, pos, bad);
        else vec_u8_take<3>(uint32_t(w8), uint32_t(w8 >> 32), cur, pos, bad);
        const uint32_t down = 32u - 8u * r;
#pragma unroll
        for (int m = 7; m > 0; --m) L[m] = __builtin_amdgcn_alignbit(L[m], L[m - 1], down);
        L[0] = (L[0] << (8u * r)) | cur;
    }
    return !(bad || pos > avail);
}

}  // namespace ipcfp
