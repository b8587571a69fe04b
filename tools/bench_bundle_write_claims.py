#!/usr/bin/env python3
"""tools/bench_bundle_write_claims.py — a bundle whose CLAIMS dominate, written from the generator's handle.

The tipset and the all-matching filter of tools/bench_generate_claims.py (≈ 1.57 M event claims in HBM at 1M receipts), no
blocks (block_ids = []): the claims head is the text.  Median of 5 after 2 warm-ups, every sample listed, of
  (a) ipcfp_bundle_write_generated_json end to end into a host buffer (sizing call + writing call),
  (b) the route it replaces on a handle whose first-use caches are cold: ipcfp_generated_events_proofs (host copy, unpack to
      strings) followed by ipcfp_bundle_write_json (sizing call + writing call) — existing code, the BASELINE; a fresh handle
      per sample, generated outside the clock,
  (c) a plain device → host copy of the same number of bytes (pageable destination, as (a) and (b) have),
  (d) the kernels of (a) under the profile id claim_text, one profiled call per sample.
(a)'s text is compared with (b)'s byte for byte.  Prints one JSON line and writes it to --out
(default profiles/bundle_write_claims_bench.json).  `python tools/bench_bundle_write_claims.py --receipts 1000000`"""
import argparse
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--receipts", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundle_write_claims_bench.json"))
    args = ap.parse_args()
    import torch  # (initialises the HIP runtime before the engine does)

    torch.cuda.init()
    import ipc_filecoin_proofs_amd as ipcfp
    from tools.synth import SEED_BASE, Tipset

    tip = Tipset(seed=SEED_BASE + 3, n_receipts=args.receipts, n_parents=5, dup_permille=20, n_planted=args.receipts, n_sigs=1,
                 n_subnets=2, max_events=4, no_events_permille=0, variety=0)
    eng = ipcfp.Engine(0)
    w = eng.witness(tip.data, tip.off, tip.lens, tip.cids)
    gen_args = (tip.parent_cids, tip.child_cid, tip.topic0, tip.topic1)
    no_blocks = np.zeros(0, dtype=np.uint32)

    def handle():
        st, g = w.generate_event_claims(*gen_args)
        assert st == 1
        return g

    g = handle()
    n_claims = g.n

    # (a) the new call
    def new_call():
        t0 = time.perf_counter()
        text = eng.bundle_write_generated_json(w, None, g, block_ids=no_blocks)
        return time.perf_counter() - t0, text

    a, text_a = [], None
    for rep in range(WARMUP + SAMPLES):
        dt, text_a = new_call()
        if rep >= WARMUP:
            a.append(dt)

    # (d) its kernels
    d = []
    for rep in range(WARMUP + SAMPLES):
        eng.profile_reset()
        eng.profile_enable(True)
        eng.bundle_write_generated_json(w, None, g, block_ids=no_blocks)
        eng.profile_enable(False)
        if rep >= WARMUP:
            d.append(eng.profile_read("claim_text")[1])
    g.close()

    # (b) the baseline: strings on the host, a cold handle per sample
    b, b_proofs, text_b = [], [], None
    for rep in range(WARMUP + SAMPLES):
        h = handle()
        t0 = time.perf_counter()
        p, n = h.proofs()
        t1 = time.perf_counter()
        text_b = w.write_bundle_json(None, 0, p, n, block_ids=no_blocks)
        t2 = time.perf_counter()
        h.close()
        if rep >= WARMUP:
            b.append(t2 - t0)
            b_proofs.append(t1 - t0)
    assert text_a == text_b, "the device head and the host head disagree"

    # (c) a plain copy of as many bytes
    src = torch.zeros(len(text_a), dtype=torch.uint8, device="cuda")
    dst = np.empty(len(text_a), dtype=np.uint8)
    c = []
    for rep in range(WARMUP + SAMPLES):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.from_numpy(dst).copy_(src)
        torch.cuda.synchronize()
        if rep >= WARMUP:
            c.append(time.perf_counter() - t0)
    w.close()
    eng.close()

    def spread(v):
        return (max(v) - min(v)) / statistics.median(v)

    rec = {
        "workload": "%d-receipt tipset, n_sigs=1, n_subnets=2, n_planted=n_receipts, no emitter filter: %d event claims, no storage "
                    "claims, no blocks; text %d bytes" % (args.receipts, n_claims, len(text_a)),
        "claims": n_claims,
        "text_bytes": len(text_a),
        "a_seconds_bundle_write_generated_json_median5": statistics.median(a),
        "a_seconds_all": a,
        "a_spread": spread(a),
        "b_seconds_proofs_plus_bundle_write_json_median5": statistics.median(b),
        "b_seconds_all": b,
        "b_spread": spread(b),
        "b_seconds_proofs_median5": statistics.median(b_proofs),
        "c_seconds_plain_d2h_copy_median5": statistics.median(c),
        "c_seconds_all": c,
        "d_kernel_ms_claim_text_median5": statistics.median(d),
        "d_kernel_ms_all": d,
        "text_equal_host_route": True,
    }
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
