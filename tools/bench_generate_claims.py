#!/usr/bin/env python3
"""tools/bench_generate_claims.py — generated matches lowered to packed claims on the device, at tipset scale.

The synthetic tipset with the parameters that give the generator the most matches it offers: ONE event signature and two
subnets (every second event passes the filter), a planted event per receipt drawn, no emitter filter.  Reports the match
count and the blob size, and the median of 5 after 2 warm-ups of
  (a) the three kernels under their profile ids (claim_sizes, claim_scan, claim_fill), one profiled call per sample,
  (b) the whole ipcfp_generate_event_claims call (the handle destroyed outside the clock),
  (c) ipcfp_generate_event_proofs alone: one call with buffers that hold everything,
  (d) the route a C caller has without the lowering once it holds the strings: ipcfp_pack_event_proofs of the same proofs
      + the upload of claims and blob from pageable memory.
The claims of (b) are compared with (d)'s byte for byte.  Prints one JSON line and writes it to --out
(default profiles/generate_claims_bench.json).  `python tools/bench_generate_claims.py --receipts 1000000`"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, SAMPLES = 2, 5


def median_of(fn):
    out = []
    for rep in range(WARMUP + SAMPLES):
        v = fn()
        if rep >= WARMUP:
            out.append(v)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--receipts", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_claims_bench.json"))
    args = ap.parse_args()
    import torch  # (initialises the HIP runtime before the engine does)

    torch.cuda.init()
    import ipc_filecoin_proofs_amd as ipcfp
    from ipc_filecoin_proofs_amd.binding import _p
    from tools.synth import SEED_BASE, Tipset

    tip = Tipset(seed=SEED_BASE + 3, n_receipts=args.receipts, n_parents=5, dup_permille=20, n_planted=args.receipts, n_sigs=1,
                 n_subnets=2, max_events=4, no_events_permille=0, variety=0)
    eng = ipcfp.Engine(0)
    w = eng.witness(tip.data, tip.off, tip.lens, tip.cids)
    lib = eng.lib
    gen_args = (tip.parent_cids, tip.child_cid, tip.topic0, tip.topic1)

    # (b) the whole call
    def whole():
        t0 = time.perf_counter()
        st, g = w.generate_event_claims(*gen_args)  # synchronous: returns after the fill and the materialisation
        dt = time.perf_counter() - t0
        assert st == 1
        g.close()
        return dt

    b_med, b_all = median_of(whole)

    # (a) the kernels, one profiled call per sample (an event pair per launch: not the figure of (b))
    def kernels():
        eng.profile_reset()
        eng.profile_enable(True)
        st, g = w.generate_event_claims(*gen_args)
        eng.profile_enable(False)
        g.close()
        return [eng.profile_read(k)[1] for k in ("claim_sizes", "claim_scan", "claim_fill")]

    ks = [kernels() for _ in range(WARMUP + SAMPLES)][WARMUP:]
    a_med = [statistics.median(s[k] for s in ks) for k in range(3)]

    # (c) the old entry point alone, one call with room for everything
    pc = ipcfp.pack_cids(tip.parent_cids)
    child = ipcfp.cid_slots([tip.child_cid])[0].copy()
    filt = np.frombuffer(bytes(tip.topic0) + bytes(tip.topic1), dtype=np.uint8).copy()
    st, g = w.generate_event_claims(*gen_args)
    n, blob_len, n_ids = g.n, g.blob_len, len(g.block_ids)
    m = np.zeros(n, dtype=ipcfp.MATCH_DTYPE)
    msg = np.zeros((n, 40), dtype=np.uint8)
    ids = np.zeros(w.n, dtype=np.uint32)

    def old():
        s = np.zeros(1, dtype=np.uint8)
        npf, nb = C.c_uint64(), C.c_uint64()
        t0 = time.perf_counter()
        rc = lib.ipcfp_generate_event_proofs(eng.h, w.h, _p(pc), len(tip.parent_cids), _p(child), _p(filt), 0, 0, _p(s), _p(m), _p(msg),
                                             n, C.byref(npf), _p(ids), None, len(ids), C.byref(nb))
        dt = time.perf_counter() - t0
        assert rc == 0 and s[0] == 1 and npf.value == n
        return dt

    c_med, c_all = median_of(old)

    # (d) strings → ipcfp_pack_event_proofs → upload
    proofs, n_p = g.proofs()
    assert n_p == n
    want_cl, want_bl = g.copy()

    def pack_upload():
        h = C.c_void_p()
        t0 = time.perf_counter()
        rc = lib.ipcfp_pack_event_proofs(proofs, n, C.byref(h))
        assert rc == 0
        nc, nbl = C.c_uint64(), C.c_uint64()
        pcl = lib.ipcfp_packed_events_claims(h, C.byref(nc))
        pbl = lib.ipcfp_packed_events_blob(h, C.byref(nbl))
        cl = np.frombuffer((C.c_uint8 * (nc.value * ipcfp.CLAIM_DTYPE.itemsize)).from_address(pcl), dtype=np.uint8)
        bl = np.frombuffer((C.c_uint8 * max(nbl.value, 1)).from_address(pbl), dtype=np.uint8)[: nbl.value]
        t1 = time.perf_counter()
        d_cl = torch.from_numpy(cl).cuda()
        d_bl = torch.from_numpy(bl).cuda()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        same = cl.tobytes() == want_cl.tobytes() and bl.tobytes() == want_bl.tobytes()
        del d_cl, d_bl
        lib.ipcfp_packed_events_destroy(h)
        assert same, "the device lowering and ipcfp_pack_event_proofs disagree"
        return (t2 - t0, t1 - t0, t2 - t1)

    d = [pack_upload() for _ in range(WARMUP + SAMPLES)][WARMUP:]
    d_med = [statistics.median(s[k] for s in d) for k in range(3)]
    g.close()
    w.close()
    eng.close()

    rec = {
        "workload": "%d-receipt tipset, n_sigs=1, n_subnets=2, n_planted=n_receipts, no emitter filter: %d blocks, %d matches, "
                    "claim records %d B, blob %d B, %d witness blocks recorded"
                    % (args.receipts, tip.n_blocks, n, n * ipcfp.CLAIM_DTYPE.itemsize, blob_len, n_ids),
        "matches": n,
        "blob_bytes": blob_len,
        "a_kernel_ms_claim_sizes_median5": a_med[0],
        "a_kernel_ms_claim_scan_median5": a_med[1],
        "a_kernel_ms_claim_fill_median5": a_med[2],
        "a_fill_GBps_written": (blob_len + n * ipcfp.CLAIM_DTYPE.itemsize) / (a_med[2] * 1e-3) / 1e9 if a_med[2] else None,
        "b_seconds_generate_event_claims_median5": b_med,
        "b_seconds_all": b_all,
        "c_seconds_generate_event_proofs_median5": c_med,
        "c_seconds_all": c_all,
        "d_seconds_pack_plus_upload_median5": d_med[0],
        "d_seconds_pack_median5": d_med[1],
        "d_seconds_upload_median5": d_med[2],
        "claims_equal_pack_event_proofs": True,
    }
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
