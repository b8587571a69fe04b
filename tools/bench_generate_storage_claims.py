#!/usr/bin/env python3
"""The storage generator finished as column claims in HBM (ipcfp_generate_storage_claims_device) against the record form
(ipcfp_generate_storage_proofs) on BASELINE.json configs[4]'s state: 10 000 contracts x 257 slots, 2.57 M specs.  One
process, one GPU, warm-up first; the routes ALTERNATE over the repetitions so that drift of the box lands on all of them.

  (a) the new kernel groups by profile id (sgen_runs, sgen_specs, sgen_records) on both routes, one profiled call per sample
  (b) the whole ipcfp_generate_storage_claims_device call, tabled (hamt_table = 1) and lane (hamt_table = 0), specs resident
  (c) ipcfp_generate_storage_proofs over the same specs: the record form, one lane per spec — the baseline
  (d) the route a caller has without the new entry point: (c), rows built on the host from the records,
      ipcfp_compact_storage_claims, and the upload of the form

Every route's output is checked after its timed region: the values against the synthetic tipset's table, every status 1, and
(b)'s columns against (d)'s.  Writes ONE JSON (--out) with every repetition, medians and the spread between repetitions.
bench.py is the project's yardstick and is not involved beyond lending its tipset builder.

    python tools/bench_generate_storage_claims.py --out profiles/generate_storage_claims_bench.json
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    import bench
    import ipc_filecoin_proofs_amd as ipcfp

    T = bench._state_tipset()
    n = len(T.sc_actor)
    ids = np.ascontiguousarray(T.sc_actor, dtype=np.uint64)
    slots = np.ascontiguousarray(T.sc_slot, dtype=np.uint8)
    eng = ipcfp.Engine(0)
    w = eng.witness(T.data, T.off, T.lens, T.cids)
    eng.profile_enable(False)
    d_ids = torch.from_numpy(ids.view(np.uint8).reshape(-1).copy()).cuda()
    d_slots = torch.from_numpy(slots.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    kept = {}

    def b_call(table):
        eng.set_tuning("hamt_table", table)
        g = w.generate_storage_claims_device(T.child_cid, T.child_epoch, d_ids.data_ptr(), d_slots.data_ptr(), n)
        eng.set_tuning("hamt_table", -1)
        return g

    def b_tabled():
        kept["g"] = b_call(1)

    def b_lane():
        kept["g"] = b_call(0)

    def c_records():
        kept["rec"] = w.generate_storage_proofs(T.child_cid, ids, slots)

    def d_today():
        rec, _ = w.generate_storage_proofs(T.child_cid, ids, slots)
        rows = ipcfp.pack_storage_claims(T.child_cid, T.state_root, T.child_epoch, ids, rec["actor_state_cid"], rec["storage_root"],
                                         slots, rec["value"])
        rows["state_root"] = rec["parent_state_root"]
        cols = ipcfp.compact_storage_claims(rows)
        buf = np.concatenate([cols.runs.view(np.uint8).reshape(-1), cols.slot.reshape(-1), cols.value.reshape(-1), cols.cflags])
        kept["d_dev"] = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        kept["cols"] = (cols.runs.tobytes(), cols.slot.tobytes(), cols.value.tobytes(), cols.cflags.tobytes(), cols.n_runs)
        cols.close()

    routes = {"b_tabled": b_tabled, "b_lane": b_lane, "c_records": c_records, "d_today": d_today}

    def check(name):
        if name.startswith("b_"):
            g = kept.pop("g")
            runs, slot, value, cflags = g.copy()
            ok = (g.status() == 1).all() and np.array_equal(value, T.sc_value) and g.first_error is None
            if "cols" in kept:
                ok = ok and (runs.tobytes(), slot.tobytes(), value.tobytes(), cflags.tobytes(), g.n_runs) == kept["cols"]
            kept["n_runs"], kept["n_blocks"] = g.n_runs, len(g.block_ids)
            g.close()
        elif name == "c_records":
            rec, ids_out = kept.pop("rec")
            ok = (rec["status"] == 1).all() and np.array_equal(rec["value"], T.sc_value)
            kept["c_blocks"] = len(ids_out)
        else:
            ok = "cols" in kept
        if not ok:
            raise SystemExit("bench_generate_storage_claims self-check failed: %s" % name)

    def run(name):
        torch.cuda.synchronize()
        eng.sync()
        t0 = time.perf_counter()
        routes[name]()  # (every entry point returns with its stream synchronised)
        dt = (time.perf_counter() - t0) * 1e3
        check(name)
        return dt

    order = ("d_today", "b_tabled", "b_lane", "c_records")
    for _ in range(args.warmup):
        for name in order:
            run(name)
    reps = {name: [] for name in order}
    for _ in range(max(args.reps, 3)):
        for name in order:  # alternating
            reps[name].append(run(name))
    if kept["n_blocks"] != kept["c_blocks"]:
        raise SystemExit("bench_generate_storage_claims self-check failed: recorded blocks")

    # (a) the kernel groups on both routes, one profiled call per sample (an event pair brackets each launch group)
    groups = ("sgen_runs", "sgen_specs", "sgen_records")
    a = {route: {k: [] for k in groups} for route in ("tabled", "lane")}
    for _ in range(max(args.reps, 3)):
        for route, table in (("tabled", 1), ("lane", 0)):
            eng.profile_enable(True)
            eng.profile_reset()
            b_call(table).close()
            for k in groups:
                a[route][k].append(eng.profile_read(k)[1])
            eng.profile_enable(False)
    med = {k: statistics.median(v) for k, v in reps.items()}
    spread = {k: max(v) - min(v) for k, v in reps.items()}
    out = {
        "workload": "BASELINE.json configs[4]'s state: %d specs of 10 000 contracts, in bundle order" % n,
        "n_specs": n, "n_runs": kept["n_runs"], "recorded_blocks": kept["n_blocks"], "witness_blocks": int(T.n_blocks),
        "warmup_rounds": args.warmup, "unit": "ms per call", "repetitions_ms": reps, "median_ms": med, "spread_ms": spread,
        "a_kernel_groups_ms": {route: {k: {"median": statistics.median(v), "samples": v} for k, v in g.items()} for route, g in a.items()},
        "b_tabled_over_c": med["b_tabled"] / med["c_records"], "b_lane_over_c": med["b_lane"] / med["c_records"],
        "b_tabled_over_d": med["b_tabled"] / med["d_today"], "b_lane_over_d": med["b_lane"] / med["d_today"],
        "note": "(b) and (c) both end in the host's Cid: Ord sort of the recorded blocks (materialize); it is not separated here",
        "device": eng.device_info()["name"], "outputs_checked": True,
    }
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
    w.close()
    eng.close()


if __name__ == "__main__":
    main()
