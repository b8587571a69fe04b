#!/usr/bin/env python3
"""The event generator over a chain (ipcfp_generate_event_claims_tipsets) against the loop of single calls it replaces
(ipcfp_generate_event_claims, once per tipset pair), on ONE witness that holds --distinct synthetic tipset pairs (tools/synth,
one seed each, --receipts receipts, 2 parent blocks, 10 planted events) — small tipsets, so that T = 4096 of them fit HBM and
what is measured is the fixed part of a call.  A chain longer than --distinct cycles through them: the same pair again is
one more tipset with the same answer.

  (a) the one chain call over T pairs
  (b) the loop of T single calls on the same build (its kernels are unchanged)

for T = 1, 16, 256 and 4096, alternating in one process, median of --reps after --warmup rounds with [min, max].  After the
timed region of the last round the outputs are compared byte for byte: statuses, claim offsets, match records, message CIDs,
claims and blob after the rebasing of include/ipcfp.h (claim.tipset, topics_off / data_off by the segment start), and the
union of the single calls' block lists against _block_ids.  Also the HIP-event times of the profile groups of one profiled
call per T.

    python tools/bench_generate_events_tipsets.py --out profiles/generate_events_tipsets_bench.json
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

SIZES = (1, 16, 256, 4096)
GROUPS = ("gen_tipsets", "exec_order", "scan_tipsets", "event_scan", "tipset_prologue", "claim_sizes", "claim_scan", "claim_fill")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--distinct", type=int, default=256)
    ap.add_argument("--receipts", type=int, default=128)
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    torch.cuda.init()
    import ipc_filecoin_proofs_amd as ipcfp
    from tools.synth import SEED_BASE, Tipset

    tips = [Tipset(seed=SEED_BASE + 100 + k, n_receipts=args.receipts, n_parents=2, n_planted=10, max_events=4) for k in range(args.distinct)]
    topic0, topic1 = tips[0].topic0, tips[0].topic1
    assert all(t.topic0 == topic0 and t.topic1 == topic1 for t in tips)
    data = np.concatenate([t.data for t in tips])
    lens = np.concatenate([t.lens for t in tips])
    base = np.concatenate([[0], np.cumsum([len(t.data) for t in tips])[:-1]]).astype(np.uint64)
    off = np.concatenate([t.off + b for t, b in zip(tips, base)])
    cids = np.concatenate([t.cids for t in tips])
    pool = [(list(t.parent_cids), t.child_cid) for t in tips]

    eng = ipcfp.Engine(0)
    w = eng.witness(data, off, lens, cids)
    eng.profile_enable(False)

    def pairs(t):
        return [pool[k % len(pool)] for k in range(t)]

    def chain(ps):
        return w.generate_event_claims_tipsets(ps, topic0, topic1)

    def loop(ps):
        return [w.generate_event_claims(parents, child, topic0, topic1) for parents, child in ps]

    def timed(fn, ps):
        torch.cuda.synchronize()
        eng.sync()
        t0 = time.perf_counter()
        got = fn(ps)  # (every entry point returns with its stream synchronised)
        return (time.perf_counter() - t0) * 1e3, got

    def close_loop(singles):
        for _st, g in singles:
            if g is not None:
                g.close()

    def same(g, singles):
        """the chain's answer against the loop's, byte for byte after the rebasing"""
        claims, blob = g.copy()
        m, c = g.matches()
        start, union = 0, set()
        ok = g.tipset_count == len(singles)
        for t, (st, s) in enumerate(singles):
            a, b = (int(x) for x in g.tipset_claim_off[t:t + 2])
            ok = ok and st == g.tipset_status[t]
            if s is None:
                ok = ok and a == b
                continue
            sc, sb = s.copy()
            sm, smc = s.matches()
            mine = claims[a:b].copy()
            mine["tipset"] = 0
            mine["topics_off"] -= np.uint32(start)
            mine["data_off"] -= np.uint32(start)
            ok = ok and b - a == s.n and mine.tobytes() == sc.tobytes() and blob[start:start + s.blob_len].tobytes() == sb.tobytes()
            ok = ok and m[a:b].tobytes() == sm.tobytes() and c[a:b].tobytes() == smc.tobytes()
            start += s.blob_len
            union |= set(s.block_ids.tolist())
        return bool(ok and start == g.blob_len and set(g.block_ids.tolist()) == union and len(g.block_ids) == len(union))

    def stats(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": v}

    def profiled(fn, ps):
        eng.profile_enable(True)
        eng.profile_reset()
        got = fn(ps)
        out = {k: {"scopes": eng.profile_read(k)[0], "ms": eng.profile_read(k)[1]} for k in GROUPS}
        eng.profile_enable(False)
        close_loop(got) if isinstance(got, list) else got.close()
        return out

    result = {"sizes": {}}
    for t in (int(s) for s in args.sizes.split(",")):
        ps = pairs(t)
        reps = max(3, args.reps if t < 4096 else min(args.reps, 3))
        for _ in range(args.warmup):
            chain(ps).close()
            close_loop(loop(ps))
        a, b = [], []
        for r in range(reps):  # alternating
            dt, g = timed(chain, ps)
            a.append(dt)
            dt, singles = timed(loop, ps)
            b.append(dt)
            if r == reps - 1 and not same(g, singles):
                raise SystemExit("bench_generate_events_tipsets self-check failed: T = %d" % t)
            n_claims, n_union, blob_len, n_sound = g.n, len(g.block_ids), g.blob_len, int((g.tipset_status == 1).sum())
            g.close()
            close_loop(singles)
        sa, sb = stats(a), stats(b)
        result["sizes"][str(t)] = {
            "n_tipsets": t, "n_sound": n_sound, "n_claims": n_claims, "blob_bytes": blob_len, "union_blocks": n_union, "a_chain_ms": sa,
            "b_loop_ms": sb, "a_over_b": sa["median"] / sb["median"], "ranges_overlap": not (sa["max"] < sb["min"] or sb["max"] < sa["min"]),
            "a_profile_groups": profiled(chain, ps), "b_profile_groups": profiled(loop, ps),
        }
        print("T = %d: chain %.3f ms, loop %.3f ms" % (t, sa["median"], sb["median"]), file=sys.stderr, flush=True)
    result.update({
        "workload": "%d distinct synthetic tipset pairs of %d receipts (2 parent blocks, 10 planted events each) in one witness; a longer "
                    "chain cycles through them" % (args.distinct, args.receipts),
        "witness_blocks": int(len(lens)), "witness_bytes": int(len(data)), "warmup_rounds": args.warmup, "repetitions": args.reps,
        "unit": "ms per chain (wall clock, Python call included on both sides); profile groups: scopes and HIP-event ms of one call",
        "device": eng.device_info()["name"], "outputs_checked": True,
    })
    print(json.dumps(result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    w.close()
    eng.close()


if __name__ == "__main__":
    main()
