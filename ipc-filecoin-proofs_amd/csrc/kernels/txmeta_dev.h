// csrc/kernels/txmeta_dev.h — the TxMeta re-hash: put_cbor(&(bls_root, secp_root), Blake2b256)
// (src/proofs/events/utils.rs:65-72) on one lane.  Written against `Rd`, so every unit gets it for the reader form it
// was compiled with (cbor_dev.h IPCFP_RD_LDS): the LDS prologue, its general companion, the deferred re-hash.
#pragma once
#include "blake2b_dev.h"
#include "cbor_dev.h"

namespace ipcfp {

// CIDv1, dag-cbor, blake2b-256: 01 71 a0 e4 02 20 ‖ digest, as a witness key
__device__ __forceinline__ void txmeta_cid_of_digest(const uint64_t d[4], CidKey& re) {
    re.w[0] = 0x00002002e4a07101ULL | (d[0] << 48);
    re.w[1] = (d[0] >> 16) | (d[1] << 48);
    re.w[2] = (d[1] >> 16) | (d[2] << 48);
    re.w[3] = (d[2] >> 16) | (d[3] << 48);
    re.w[4] = d[3] >> 16;
}

// The CID of the canonical re-encoding of the two links that `r` read at (o0, l0) and (o1, l1) (lengths <= 64)
__device__ __forceinline__ void txmeta_rehash(Rd& r, uint32_t o0, uint32_t l0, uint32_t o1, uint32_t l1, CidKey& re) {
    uint8_t enc[200];
    uint32_t n = 0;
    enc[n++] = 0x82;
    const uint32_t offs[2] = {o0, o1}, lens[2] = {l0, l1};
    for (int k = 0; k < 2; ++k) {
        enc[n++] = 0xd8;
        enc[n++] = 0x2a;
        const uint32_t bl = lens[k] + 1;
        if (bl < 24) enc[n++] = uint8_t(0x40 | bl);
        else { enc[n++] = 0x58; enc[n++] = uint8_t(bl); }
        enc[n++] = 0x00;
        for (uint32_t i = 0; i < lens[k]; ++i) enc[n++] = uint8_t(r.at(offs[k] + i));
    }
    uint64_t d[4];
    blake2b256_small(enc, n, d);
    txmeta_cid_of_digest(d, re);
}

}  // namespace ipcfp
