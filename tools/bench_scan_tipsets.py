#!/usr/bin/env python3
"""tools/bench_scan_tipsets.py — one scan of a CHAIN of tipsets (ipcfp_scan_events_tipsets_device) against the loop of
single-tipset calls it replaces.

T synthetic tipsets of R receipts each (tools/synth, distinct seeds) merged into ONE resident witness, event table warm,
F ∈ {1, 16} specs from the generator's own names.  Default shapes (T, R): (16, 65536), (256, 4096), (4096, 256).
Sides, alternating in one process, median of 5 after 2 warm-ups with the min-max of the five:
  (a) the one call, device form;
  (b) T calls of ipcfp_scan_events_multi_device on FIRST contact: ipcfp_witness_rebuild_index drops the per-root caches
      before each repetition; the block table is rebuilt outside the timed region — for every side — by a chain call over
      one root, which fills no per-root cache;
  (c) the same loop with its per-root caches warm;
  (d) HIP-event time of (a)'s profile groups from one profiled call per sample: exec_order (the enumeration, host waits
      between its launches included), scan_tipsets (the new kernels), event_scan (the receipt records).  The prefix sum
      (launch_scan_u32) belongs to no profile group and is not in (d).
After the timed region the buffers the sides wrote are compared byte for byte.  Also T = 1: (a) against one multi call.
Prints one JSON line and writes it to --out (default profiles/scan_tipsets_bench.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARMUP, SAMPLES = 2, 5
SIGS = ["NewTopDownMessage(bytes32,uint256)", "Transfer(address,address,uint256)", "Approval(address,address,uint256)",
        "Deposit(address,uint256)", "Withdrawal(address,uint256)", "Swap(address,uint256,uint256,uint256,uint256,address)",
        "Sync(uint112,uint112)", "Mint(address,uint256,uint256)", "Burn(address,uint256,uint256,address)",
        "OwnershipTransferred(address,address)", "Upgraded(address)", "Paused(address)", "Unpaused(address)",
        "RoleGranted(bytes32,address,address)", "RoleRevoked(bytes32,address,address)", "Initialized(uint8)"]  # tools/synth/synth.cpp kSigs


def named(f):
    return SIGS[f % 16], f"calib-subnet-{f // 16}"


def merged_chain(T, R):
    """T synthetic tipsets in one set of witness tables → (data, off, lens, cids, [receipts root])"""
    from tools.synth import SEED_BASE, Tipset

    data, off, lens, cids, roots, base = [], [], [], [], [], 0
    for t in range(T):
        tip = Tipset(seed=SEED_BASE + 100 + t, n_receipts=R, n_sigs=16, n_subnets=64, max_events=4, variety=0, parent_epoch=2992953 + t)
        data.append(tip.data)
        off.append(tip.off + np.uint64(base))
        lens.append(tip.lens)
        cids.append(tip.cids)
        roots.append(tip.receipts_root)
        base += len(tip.data)
    assert len(set(roots)) == T
    return np.concatenate(data), np.concatenate(off), np.concatenate(lens), np.concatenate(cids), roots


def spread(xs):
    return {"median": statistics.median(xs), "min": min(xs), "max": max(xs), "all": xs}


def shape(torch, ipcfp, eng, T, R, Fs):
    tables = merged_chain(T, R)
    roots = tables[4]
    out = {}
    with eng.witness(*tables[:4]) as w:
        item = ipcfp.MATCH_DTYPE.itemsize
        for F in Fs:
            specs = [(*eng.create_event_filter(*named(f)), None) for f in range(F)]
            st, _ph, roff, moff, nr, nm = w.scan_events_tipsets_device(roots, specs)  # sizes
            assert set(st.tolist()) == {1}
            roff, moff = roff.astype(np.int64), moff.astype(np.int64)
            bufs = {k: (torch.zeros(nr + 64, dtype=torch.uint8, device="cuda"), torch.zeros((nm + 1) * item, dtype=torch.uint8, device="cuda"),
                        torch.zeros(nm + 1, dtype=torch.int32, device="cuda"), torch.zeros(F, dtype=torch.int64, device="cuda")) for k in "abc"}
            acc = torch.zeros(F, dtype=torch.int64, device="cuda")

            def chain(k="a"):
                h, m, ms, c = bufs[k]
                t0 = time.perf_counter()
                w.scan_events_tipsets_device(roots, specs, h.data_ptr(), nr, m.data_ptr(), ms.data_ptr(), nm, c.data_ptr())
                eng.sync()
                return (time.perf_counter() - t0) * 1e3

            def loop(k):
                h, m, ms, c = bufs[k]
                hp, mp, msp = h.data_ptr(), m.data_ptr(), ms.data_ptr()
                t0 = time.perf_counter()
                for t, root in enumerate(roots):
                    cap = int(moff[t + 1] - moff[t])
                    w.scan_events_multi_device(root, specs, hp + int(roff[t]), int(roff[t + 1] - roff[t]), (mp + int(moff[t]) * item) if cap else 0,
                                               (msp + int(moff[t]) * 4) if cap else 0, cap, 0)
                eng.sync()
                return (time.perf_counter() - t0) * 1e3

            def fresh_block_table():
                w.rebuild_index()
                w.scan_events_tipsets_device(roots[:1], specs)  # (the block table again; no per-root cache is filled)
                eng.sync()

            ta, tb, tc_, groups = [], [], [], {g: [] for g in ("exec_order", "scan_tipsets", "event_scan")}
            for rep in range(WARMUP + SAMPLES):
                fresh_block_table()
                a = chain("a")
                fresh_block_table()
                b = loop("b")          # first contact: every root enumerates and tabulates
                c = loop("c")          # … and again, caches warm
                eng.profile_enable(True)
                eng.profile_reset()
                chain("a")
                g = {k: eng.profile_read(k)[1] for k in groups}
                eng.profile_enable(False)
                if rep >= WARMUP:
                    ta.append(a), tb.append(b), tc_.append(c)
                    for k in groups:
                        groups[k].append(g[k])
            same = all(torch.equal(bufs["a"][i], bufs[k][i]) for k in "bc" for i in range(3))
            one_chain, one_multi = [], []
            for rep in range(WARMUP + SAMPLES):  # T = 1, caches warm: the chain call has no fused tail
                t0 = time.perf_counter()
                w.scan_events_tipsets_device(roots[:1], specs, bufs["a"][0].data_ptr(), int(roff[1]), bufs["a"][1].data_ptr(), bufs["a"][2].data_ptr(), int(moff[1]),
                                             acc.data_ptr())
                eng.sync()
                t1 = time.perf_counter()
                w.scan_events_multi_device(roots[0], specs, bufs["b"][0].data_ptr(), int(roff[1]), bufs["b"][1].data_ptr(), bufs["b"][2].data_ptr(), int(moff[1]),
                                           acc.data_ptr())
                eng.sync()
                t2 = time.perf_counter()
                if rep >= WARMUP:
                    one_chain.append((t1 - t0) * 1e3), one_multi.append((t2 - t1) * 1e3)
            A, B, Cc = spread(ta), spread(tb), spread(tc_)
            out[f"F={F}"] = {"receipts": int(nr), "matches": int(nm), "a_chain_ms": A, "b_loop_first_contact_ms": B, "c_loop_warm_ms": Cc,
                             "a_over_b": A["median"] / B["median"], "a_over_c": A["median"] / Cc["median"],
                             "a_below_b_ranges_apart": A["max"] < B["min"], "d_kernel_groups_ms": {k: spread(v) for k, v in groups.items()},
                             "outputs_byte_equal": bool(same), "T1_chain_ms": spread(one_chain), "T1_multi_ms": spread(one_multi),
                             "T1_chain_over_multi": statistics.median(one_chain) / statistics.median(one_multi)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["16x65536", "256x4096", "4096x256"], help="TxR")
    ap.add_argument("--F", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_tipsets_bench.json"))
    args = ap.parse_args()
    import torch  # (initialises the HIP runtime before the engine does)

    torch.cuda.init()
    import ipc_filecoin_proofs_amd as ipcfp

    res = {"warmup": WARMUP, "samples": SAMPLES, "shapes": {}}
    with ipcfp.Engine(0) as eng:
        for s in args.shapes:
            T, R = (int(x) for x in s.split("x"))
            res["shapes"][s] = shape(torch, ipcfp, eng, T, R, args.F)
            print(s, json.dumps(res["shapes"][s]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
