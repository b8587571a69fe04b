#!/usr/bin/env python3
"""Plain storage claims against the run-compressed column form (include/ipcfp.h) on BASELINE.json configs[4]:
10 000 contracts x 257 claims, every 1000th value wrong.  One process, one GPU, profiler off, warm-up first; the two
routes ALTERNATE over the repetitions so that drift of the box lands on both.

  T3  claims resident in HBM:   ipcfp_verify_storage_claims_device  vs  ipcfp_verify_storage_columns_device
  T2  claims in pageable host memory, status bytes back:   ipcfp_verify_storage_claims  vs  ipcfp_verify_storage_columns

Every route's verdicts are checked against the expected bytes after its timed region.  Writes ONE JSON (--out) with every
repetition, the medians, the spread between repetitions of the same route, the bytes each form sends and n_runs.
bench.py is the project's yardstick and is not involved beyond lending its tipset builder.

    python tools/bench_storage_columns.py --reps 3 --calls 20 --out profiles/storage_columns_bench.json
    python tools/bench_storage_columns.py --trace-only      # a few calls of each T3 route, for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="repetitions of every route (>= 3)")
    ap.add_argument("--calls", type=int, default=20, help="timed calls per repetition (>= 20)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-only", action="store_true", help="warm-up + 5 calls of each T3 route, nothing written")
    ap.add_argument("--t2-reference-gbs", type=float, default=55.0,
                    help="the rate the headline's T2 window reaches (bench.py --full), for the upload sanity check")
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    import bench
    import ipc_filecoin_proofs_amd as ipcfp

    T = bench._state_tipset()
    n = len(T.sc_actor)
    cl = ipcfp.pack_storage_claims(T.child_cid, T.state_root, T.child_epoch, T.sc_actor, T.sc_actor_state, T.sc_storage_root,
                                   T.sc_slot, T.sc_value)
    wrong = np.arange(500, n, 1000)
    cl["value"][wrong, 31] ^= 1
    want = np.ones(n, dtype=np.uint8)
    want[wrong] = 21
    cols = ipcfp.compact_storage_claims(cl)
    eng = ipcfp.Engine(0)
    w = eng.witness(T.data, T.off, T.lens, T.cids)
    eng.profile_enable(False)

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    d_cl = dev(cl)
    d_runs, d_slot, d_value, d_cflags = dev(cols.runs), dev(cols.slot), dev(cols.value), dev(cols.cflags)
    d_st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    host_st = {}
    torch.cuda.synchronize()

    def t3_plain():
        w.verify_storage_claims_device(d_cl.data_ptr(), n, d_st.data_ptr())

    def t3_columns():
        w.verify_storage_columns_device(d_runs.data_ptr(), cols.n_runs, d_slot.data_ptr(), d_value.data_ptr(), d_cflags.data_ptr(), n,
                                        d_st.data_ptr())

    def t2_plain():
        host_st["t2_plain"] = w.verify_storage_claims(cl)

    def t2_columns():
        host_st["t2_columns"] = w.verify_storage_columns(cols)

    routes = {"t3_plain": t3_plain, "t3_columns": t3_columns, "t2_plain": t2_plain, "t2_columns": t2_columns}

    def check(name):
        got = d_st.cpu().numpy() if name.startswith("t3") else host_st[name]
        if not np.array_equal(got, want):
            raise SystemExit("bench_storage_columns self-check failed: %s verdicts" % name)

    def run(name, calls):
        fn = routes[name]
        if name.startswith("t3"):
            d_st.zero_()
        torch.cuda.synchronize()
        eng.sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()  # (every entry point returns with its stream synchronised)
        dt = time.perf_counter() - t0
        check(name)
        return dt / calls * 1e3

    for name in routes:
        run(name, args.warmup)
    if args.trace_only:
        for name in ("t3_plain", "t3_columns"):
            run(name, 5)
        print("trace run done")
        return
    reps = {name: [] for name in routes}
    for _ in range(max(args.reps, 3)):
        for name in routes:  # alternating: plain, columns, plain, columns
            reps[name].append(run(name, max(args.calls, 20)))
    med = {k: statistics.median(v) for k, v in reps.items()}
    spread = {k: max(v) - min(v) for k, v in reps.items()}
    h2d_plain, h2d_cols = int(cl.nbytes), int(cols.nbytes)
    out = {
        "workload": "BASELINE.json configs[4]: %d storage claims of 10 000 contracts, every 1000th value wrong" % n,
        "n_claims": n, "n_runs": cols.n_runs, "calls_per_repetition": max(args.calls, 20), "warmup_calls": args.warmup,
        "unit": "ms per call", "repetitions_ms": reps, "median_ms": med, "spread_ms": spread,
        "h2d_bytes": {"plain": h2d_plain, "columns": h2d_cols, "ratio": h2d_cols / h2d_plain},
        "t3_columns_minus_plain_ms": med["t3_columns"] - med["t3_plain"],
        "t2_columns_minus_plain_ms": med["t2_columns"] - med["t2_plain"],
        # upload sanity check: the T2 calls minus their T3 counterparts, as a rate over the bytes each form sends
        "t2_upload_estimate_gbs": {"plain": h2d_plain / max(med["t2_plain"] - med["t3_plain"], 1e-9) / 1e6,
                                   "columns": h2d_cols / max(med["t2_columns"] - med["t3_columns"], 1e-9) / 1e6},
        "t2_reference_gbs": args.t2_reference_gbs,
        "t2_reference_source": "the rate of the headline's T2 window in bench.py --full",
        "device": eng.device_info()["name"],
        "verdicts_checked": True,
    }
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    w.close()
    cols.close()
    eng.close()


if __name__ == "__main__":
    main()
