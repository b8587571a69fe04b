#!/usr/bin/env python3
"""tools/bench_bundle_write.py — the bundle wire format at tipset scale, WRITE direction.

Builds the synthetic tipset's bundle as tools/bench_bundle.py does (every block + a handful of claims), writes it with
ipcfp_bundle_write_json and reports
  (a) the summed kernel time under the `base64` profile id (sizes, prefix sums, frames, base64),
  (b) the whole call, median of 5 after 2 warm-ups (sizing call and writing call, as the binding makes them, and the
      writing call alone),
  (c) the Python writer tests/bundle_ref.bundle_json on the same input — what the engine's writer replaces,
  (d) the bytes copied back, and the floor of (b): (d) at the box's D2H rate, measured here with one timed blocking copy
      of the same size into the same kind of buffer (fresh pageable memory).
Prints one JSON line and writes it to --out (default profiles/bundle_write_bench.json).
`python tools/bench_bundle_write.py --receipts 1000000`"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--receipts", type=int, default=1_000_000)
    ap.add_argument("--claims", type=int, default=5)
    ap.add_argument("--no-python-writer", action="store_true", help="skip (c) and the byte-for-byte comparison with it")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundle_write_bench.json"))
    args = ap.parse_args()
    import torch  # (initialises the HIP runtime before the engine does)

    torch.cuda.init()
    import bundle_ref
    import claims
    import ipc_filecoin_proofs_amd as ipcfp
    from tools.synth import SEED_BASE, Tipset

    tip = Tipset(seed=SEED_BASE + 3, n_receipts=args.receipts, n_parents=5, dup_permille=20,
                 n_planted=max(1, args.receipts // 1000), max_events=4, no_events_permille=0, variety=0)
    idx = np.arange(min(args.claims, len(tip.claim_exec)))
    ec = claims.EventClaims(tip, indices=idx)
    eng = ipcfp.Engine(0)
    w = eng.witness(tip.data, tip.off, tip.lens, tip.cids)
    lib = eng.lib
    ev_ptr = C.cast(ec.arr, C.c_void_p)

    def sizing():
        n = C.c_uint64()
        eng._check(lib.ipcfp_bundle_write_json(eng.h, w.h, None, 0, ev_ptr, ec.n, None, w.n, None, 0, C.byref(n)), "sizing")
        return int(n.value)

    def writing(out):
        n = C.c_uint64()
        eng._check(lib.ipcfp_bundle_write_json(eng.h, w.h, None, 0, ev_ptr, ec.n, None, w.n, out.ctypes.data_as(C.c_void_p),
                                               out.size, C.byref(n)), "writing")

    both, alone = [], []
    for rep in range(7):
        t0 = time.perf_counter()
        n = sizing()
        out = np.empty(n, dtype=np.uint8)  # fresh pageable memory, as Witness.write_bundle_json allocates it
        t1 = time.perf_counter()
        writing(out)
        t2 = time.perf_counter()
        if rep >= 2:
            both.append(t2 - t0)
            alone.append(t2 - t1)
        if rep < 6:
            del out
    text = out.tobytes()
    del out
    eng.profile_reset()
    eng.profile_enable(True)
    profiled = w.write_bundle_json(None, 0, ec.arr, ec.n)
    eng.profile_enable(False)
    launches, kernel_ms = eng.profile_read("base64")
    assert profiled == text
    del profiled
    head_len = text.index(b'"blocks":[') + 10
    copied = len(text) - head_len - 2

    # the floor: the same number of bytes, HBM → fresh pageable memory, one blocking copy
    src = torch.zeros(copied, dtype=torch.uint8, device="cuda")
    d2h = []
    for _ in range(4):
        dst = torch.empty(copied, dtype=torch.uint8)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dst.copy_(src)
        torch.cuda.synchronize()
        d2h.append(time.perf_counter() - t0)
        del dst
    del src
    floor = statistics.median(d2h[1:])

    rec = {
        "workload": "UnifiedProofBundle JSON of the %d-receipt tipset witness: %d blocks, %.3f GB payload, %.3f GB JSON, %d event claims"
                    % (args.receipts, tip.n_blocks, int(tip.lens.astype(np.int64).sum()) / 1e9, len(text) / 1e9, ec.n),
        "a_kernel_ms_base64_id": kernel_ms,
        "a_profiled_launch_groups": launches,
        "a_text_GBps_of_kernels": copied / (kernel_ms * 1e-3) / 1e9 if kernel_ms else None,
        "b_seconds_sizing_plus_writing_median5": statistics.median(both),
        "b_seconds_writing_call_median5": statistics.median(alone),
        "b_seconds_writing_call_all": alone,
        "d_bytes_copied_back": copied,
        "d2h_seconds_same_bytes_fresh_pageable": floor,
        "d2h_GBps": copied / floor / 1e9,
        "b_writing_call_over_d2h_floor": statistics.median(alone) / floor,
    }
    if not args.no_python_writer:
        blocks = [(tip.cids[i, :38].tobytes(), tip.block(i)) for i in range(tip.n_blocks)]
        events = bundle_ref.event_dicts(tip, indices=idx)
        t0 = time.perf_counter()
        want = bundle_ref.bundle_json([], events, blocks).encode()
        rec["c_python_writer_seconds"] = time.perf_counter() - t0
        rec["text_equals_python_writer"] = want == text
        assert want == text
    w.close()
    eng.close()
    line = json.dumps(rec)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
