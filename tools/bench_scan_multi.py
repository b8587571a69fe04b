#!/usr/bin/env python3
"""tools/bench_scan_multi.py — one scan of the resident tipset for F event specs against F single-filter scans, and the
bundle generator on top of it against the parent commit's build.

The synthetic tipset of --receipts receipts with n_sigs = 16, n_subnets = 64 (1024 (signature, subnet) pairs), witness
resident, event table warm, F ∈ {1, 16, 256, 1024} specs taken from the generator's own names.
  (a) one ipcfp_scan_events_multi_device call against F calls of ipcfp_scan_events_device in the same process, alternating,
      median of 5 after 2 warm-ups: wall time around the synchronised call(s), and HIP-event time of the new kernels under
      their profile ids (scan_multi_count, scan_multi_tail — the table route's one-launch tail, where a call without a
      recorder spends its PASS 2 — and scan_multi_fill) from one profiled call per sample.  The records of the multi
      call are checked against the single calls' first (counts per spec).
  (b) ipcfp_generate_proof_bundle with F event specs, F ∈ {1, 16, 256}: this build and --parent-tree (a built checkout of
      the parent commit) in child processes of their own, alternating, outputs compared byte for byte (a digest) first.
Prints one JSON line and writes it to --out (default profiles/scan_multi_bench.json).  A figure that was not taken is
"not measured".  `python tools/bench_scan_multi.py --parent-tree ab_libs/parent_tree`"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a child of (b) imports the package and the tipset generator of the tree it measures: this one, or a built checkout of the parent)
ROOT = os.environ.get("IPCFP_BENCH_TREE", ROOT)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

WARMUP, SAMPLES = 2, 5
SIGS = ["NewTopDownMessage(bytes32,uint256)", "Transfer(address,address,uint256)", "Approval(address,address,uint256)",
        "Deposit(address,uint256)", "Withdrawal(address,uint256)", "Swap(address,uint256,uint256,uint256,uint256,address)",
        "Sync(uint112,uint112)", "Mint(address,uint256,uint256)", "Burn(address,uint256,uint256,address)",
        "OwnershipTransferred(address,address)", "Upgraded(address)", "Paused(address)", "Unpaused(address)",
        "RoleGranted(bytes32,address,address)", "RoleRevoked(bytes32,address,address)", "Initialized(uint8)"]  # tools/synth/synth.cpp kSigs


def named(f):
    return SIGS[f % 16], f"calib-subnet-{f // 16}"


def setup(receipts):
    import torch  # (initialises the HIP runtime before the engine does)

    torch.cuda.init()
    import ipc_filecoin_proofs_amd as ipcfp
    from tools.synth import SEED_BASE, Tipset

    tip = Tipset(seed=SEED_BASE + 3, n_receipts=receipts, n_sigs=16, n_subnets=64, max_events=4, variety=0)
    eng = ipcfp.Engine(0)
    w = eng.witness(tip.data, tip.off, tip.lens, tip.cids)
    return torch, ipcfp, tip, eng, w


def bundle_child(args):
    """(b) in one process with one library: per F the wall times of ipcfp_generate_proof_bundle and a digest of its outputs"""
    _torch, _ipcfp, tip, eng, w = setup(args.receipts)
    out = {}
    for F in args.F:
        specs = [(*named(f), None) for f in range(F)]
        times, digest = [], None
        for rep in range(1 + args.samples):
            t = time.perf_counter()
            r = w.generate_proof_bundle(tip.parent_cids, tip.child_cid, [], specs)
            dt = time.perf_counter() - t
            if rep:
                times.append(dt * 1e3)
            h = hashlib.sha256()
            for k in ("event_status", "matches", "message_cids", "match_spec", "block_ids"):
                h.update(np.ascontiguousarray(r[k]).tobytes())
            h.update(repr(r["first_error"]).encode())
            assert digest in (None, h.hexdigest())
            digest = h.hexdigest()
        out[str(F)] = {"ms": times, "digest": digest, "n_proofs": int(len(r["matches"])), "n_blocks": int(len(r["block_ids"]))}
    print("BUNDLE " + json.dumps(out), flush=True)


def scan_part(args):
    torch, ipcfp, tip, eng, w = setup(args.receipts)
    res = {}
    n_r = args.receipts
    for F in args.F:
        specs = [(*eng.create_event_filter(*named(f)), None) for f in range(F)]
        cap = 1 << 23
        d_has = torch.zeros(n_r + 64, dtype=torch.uint8, device="cuda")
        d_m = torch.zeros(cap * ipcfp.MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        d_ms = torch.zeros(cap, dtype=torch.int32, device="cuda")
        d_cnt = torch.zeros(F, dtype=torch.int64, device="cuda")

        def multi():
            t = time.perf_counter()
            st, nr, nm = w.scan_events_multi_device(tip.receipts_root, specs, d_has.data_ptr(), n_r, d_m.data_ptr(), d_ms.data_ptr(), cap, d_cnt.data_ptr())
            eng.sync()
            assert st == 1
            return (time.perf_counter() - t) * 1e3, nm

        def singles():
            t = time.perf_counter()
            counts = []
            for t0, t1, _a in specs:
                st, nr, nm = w.scan_events_device(tip.receipts_root, t0, t1, None, d_has.data_ptr(), n_r, d_m.data_ptr(), cap)
                counts.append(nm)
            eng.sync()
            return (time.perf_counter() - t) * 1e3, counts

        tm, ts, kc, kf, kt = [], [], [], [], []
        for rep in range(WARMUP + SAMPLES):
            a, nm = multi()
            b, counts = singles()
            assert d_cnt.cpu().numpy().tolist() == counts and sum(counts) == nm
            eng.profile_enable(True)
            eng.profile_reset()
            multi()
            c, f, tl = (eng.profile_read(k)[1] for k in ("scan_multi_count", "scan_multi_fill", "scan_multi_tail"))
            eng.profile_enable(False)
            if rep >= WARMUP:
                tm.append(a), ts.append(b), kc.append(c), kf.append(f), kt.append(tl)
        res[str(F)] = {"multi_ms": tm, "singles_ms": ts, "count_kernels_ms": kc, "fill_kernels_ms": kf, "tail_kernel_ms": kt, "n_matches": int(nm),
                       "multi_over_singles": statistics.median(tm) / statistics.median(ts)}
    # the cost of F = 1 relative to the single call: the F = 1 row's ratio
    res["F1_over_single_call"] = res["1"]["multi_over_singles"] if "1" in res else "not measured"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--receipts", type=int, default=1_000_000)
    ap.add_argument("--F", type=int, nargs="+", default=None)
    ap.add_argument("--samples", type=int, default=3)
    ap.add_argument("--bundle-child", action="store_true")
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (its own binding and libipcfp.so)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_multi_bench.json"))
    args = ap.parse_args()
    if args.bundle_child:
        args.F = args.F or [1, 16, 256]
        return bundle_child(args)
    args.F = args.F or [1, 16, 256, 1024]
    out = {"receipts": args.receipts, "scan": scan_part(args)}
    if args.parent_tree and os.path.exists(args.parent_tree):
        runs = {"this": [], "parent": []}
        for _round in range(2):
            for tag, tree in (("this", None), ("parent", os.path.abspath(args.parent_tree))):
                env = dict(os.environ)
                if tree:
                    env["IPCFP_BENCH_TREE"] = tree
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--bundle-child", "--receipts", str(args.receipts), "--samples", str(args.samples),
                                    "--F", *[str(f) for f in args.F if f <= 256]], env=env, stdout=subprocess.PIPE, timeout=400, check=True)
                line = [x for x in p.stdout.decode().splitlines() if x.startswith("BUNDLE ")][-1]
                runs[tag].append(json.loads(line[7:]))
        same = all(a[k]["digest"] == b[k]["digest"] for a, b in zip(runs["this"], runs["parent"]) for k in a)
        out["bundle"] = {"outputs_byte_equal": same, "runs": runs}
    else:
        out["bundle"] = "not measured"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
