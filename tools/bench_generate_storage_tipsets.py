#!/usr/bin/env python3
"""The storage generator over a chain (ipcfp_generate_storage_claims_tipsets_device) against the loop of single calls it
replaces (ipcfp_generate_storage_claims_device, once per child), on BASELINE.json configs[4]'s state with T distinct child
headers over it: copies of the tipset's child header with distinct heights, all linking the ONE state root — enough to
measure the fixed part of a call; a chain of differing states is not timed here.

  (a) the one _tipsets_device call over T children
  (b) the loop of T ipcfp_generate_storage_claims_device calls

for T x n_specs = 16 x 16384, 256 x 1024 and 4096 x 64, alternating in one process, median of --reps after --warmup rounds
with [min, max]; the outputs are compared byte for byte after the timed region (columns, run table with first_claim
shifted, status, each tipset's block list, the union).  Also: T = 1 against one single call; the profile groups' HIP-event
times of one profiled call per shape; and the same 262 144 specs as ONE tipset through the chain kernels and through the
single call's — equal work, the recorder's row chosen per lane against the wave-uniform pointer.

    python tools/bench_generate_storage_tipsets.py --out profiles/generate_storage_tipsets_bench.json
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((16, 16384), (256, 1024), (4096, 64))
GROUPS = ("sgen_runs", "sgen_specs", "sgen_records")


def _skip(b, pos):
    """→ the position behind the CBOR item at pos (definite lengths only, as DAG-CBOR has them)"""
    major, info = b[pos] >> 5, b[pos] & 31
    pos += 1
    if info < 24:
        val = info
    else:
        width = {24: 1, 25: 2, 26: 4, 27: 8}[info]
        val = int.from_bytes(b[pos:pos + width], "big")
        pos += width
    if major in (2, 3):
        return pos + val
    if major in (4, 5):
        for _ in range(val * (2 if major == 5 else 1)):
            pos = _skip(b, pos)
        return pos
    if major == 6:
        return _skip(b, pos)
    return pos


def _uint(n):
    for info, width in ((24, 1), (25, 2), (26, 4), (27, 8)):
        if n < 24:
            return bytes([n])
        if n < 1 << (8 * width):
            return bytes([info]) + n.to_bytes(width, "big")
    raise ValueError(n)


def headers_over(header: bytes, heights):
    """Copies of a block header (a 16-item array) whose 8th item, the height, is re-spelled → [(cid, bytes)]"""
    assert header[0] == 0x90
    pos = 1
    for _ in range(7):
        pos = _skip(header, pos)
    end = _skip(header, pos)
    out = []
    for h in heights:
        b = header[:pos] + _uint(h) + header[end:]
        out.append((bytes.fromhex("0171a0e40220") + hashlib.blake2b(b, digest_size=32).digest(), b))
    return out


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

    S = bench._state_tipset()
    t_max = max(t for t, _ in SHAPES)
    hdr = S.block(S.find_block(S.child_cid))
    made = headers_over(hdr, [S.child_epoch + 1 + k for k in range(t_max)])
    extra = np.frombuffer(b"".join(b for _, b in made), dtype=np.uint8)
    lens = np.concatenate([S.lens, np.array([len(b) for _, b in made], dtype=np.uint32)])
    off = np.concatenate([S.off, len(S.data) + np.concatenate([[0], np.cumsum([len(b) for _, b in made])[:-1]]).astype(np.uint64)])
    data = np.concatenate([S.data, extra])
    cids = np.concatenate([S.cids, ipcfp.cid_slots([c for c, _ in made])])
    children = [c for c, _ in made]
    epochs = np.arange(S.child_epoch + 1, S.child_epoch + 1 + t_max, dtype=np.int64)

    eng = ipcfp.Engine(0)
    w = eng.witness(data, off, lens, cids)
    eng.profile_enable(False)
    ids = np.ascontiguousarray(S.sc_actor, dtype=np.uint64)
    slots = np.ascontiguousarray(S.sc_slot, dtype=np.uint8)
    d_ids = torch.from_numpy(ids.view(np.uint8).reshape(-1).copy()).cuda()
    d_slots = torch.from_numpy(slots.reshape(-1).copy()).cuda()
    torch.cuda.synchronize()

    def chain(t, n):
        return w.generate_storage_claims_tipsets_device(children[:t], epochs[:t], d_ids.data_ptr(), d_slots.data_ptr(), n)

    def loop(t, n):
        return [w.generate_storage_claims_device(children[k], int(epochs[k]), d_ids.data_ptr(), d_slots.data_ptr(), n) for k in range(t)]

    def timed(fn, *a):
        torch.cuda.synchronize()
        eng.sync()
        t0 = time.perf_counter()
        got = fn(*a)  # (every entry point returns with its stream synchronised)
        return (time.perf_counter() - t0) * 1e3, got

    def close(x):
        for g in (x if isinstance(x, list) else [x]):
            g.close()

    def same(g, singles, n):
        """the chain's answer against the loop's, byte for byte"""
        runs, slot, value, cflags = g.copy()
        parts = [s.copy() for s in singles]
        for k, p in enumerate(parts):
            p[0]["first_claim"] += k * n
        ok = all(b"".join(p[c].tobytes() for p in parts) == x.tobytes() for c, x in enumerate((runs, slot, value, cflags)))
        ok = ok and g.status().tobytes() == b"".join(s.status().tobytes() for s in singles) and (g.status() == 1).all()
        ok = ok and all(g.tipset_block_ids(k).tolist() == s.block_ids.tolist() for k, s in enumerate(singles))
        ok = ok and sorted(g.block_ids.tolist()) == sorted(set(i for s in singles for i in s.block_ids.tolist()))
        return bool(ok)

    def stats(v):
        return {"median": statistics.median(v), "min": min(v), "max": max(v), "samples": v}

    def profiled(fn, *a):
        eng.profile_enable(True)
        eng.profile_reset()
        close(fn(*a))
        out = {k: eng.profile_read(k)[1] for k in GROUPS}
        eng.profile_enable(False)
        return out

    result = {"shapes": {}}
    reps = max(args.reps, 3)
    for t, n in SHAPES:
        for _ in range(args.warmup):
            close(chain(t, n))
            close(loop(t, n))
        a, b = [], []
        for r in range(reps):  # alternating
            dt, g = timed(chain, t, n)
            a.append(dt)
            dt, singles = timed(loop, t, n)
            b.append(dt)
            if r == reps - 1 and not same(g, singles, n):
                raise SystemExit("bench_generate_storage_tipsets self-check failed: %d x %d" % (t, n))
            n_runs, n_union = g.n_runs, len(g.block_ids)
            close(g)
            close(singles)
        sa, sb = stats(a), stats(b)
        result["shapes"]["%dx%d" % (t, n)] = {
            "n_tipsets": t, "n_specs": n, "n_runs": n_runs, "union_blocks": n_union, "a_chain_ms": sa, "b_loop_ms": sb,
            "a_over_b": sa["median"] / sb["median"], "ranges_overlap": not (sa["max"] < sb["min"] or sb["max"] < sa["min"]),
            "a_kernel_groups_ms": profiled(chain, t, n), "b_kernel_groups_ms": profiled(loop, t, n),
        }
        print("%d x %d: chain %.2f ms, loop %.2f ms" % (t, n, sa["median"], sb["median"]), file=sys.stderr, flush=True)
    # T = 1 against one single call
    n1 = SHAPES[0][1]
    a, b = [], []
    for r in range(args.warmup + reps):
        dt, g = timed(chain, 1, n1)
        da, singles = timed(loop, 1, n1)
        if r >= args.warmup:
            a.append(dt), b.append(da)
        if not same(g, singles, n1):
            raise SystemExit("bench_generate_storage_tipsets self-check failed: T = 1")
        close(g), close(singles)
    result["t1_against_single"] = {"n_specs": n1, "a_chain_ms": stats(a), "b_single_ms": stats(b),
                                   "a_over_b": statistics.median(a) / statistics.median(b)}
    # equal work on both sets of kernels: ONE tipset of 262 144 specs (the recorder's row per lane against the uniform pointer)
    n_all = SHAPES[0][0] * SHAPES[0][1]
    rows = {"chain_kernels": [], "single_kernels": []}
    for _ in range(reps):
        rows["chain_kernels"].append(profiled(chain, 1, n_all))
        rows["single_kernels"].append(profiled(loop, 1, n_all))
    result["one_tipset_%d_specs_kernel_groups_ms" % n_all] = {
        k: {grp: statistics.median(s[grp] for s in v) for grp in GROUPS} for k, v in rows.items()}
    result.update({
        "workload": "BASELINE.json configs[4]'s state under %d child headers of distinct heights, one state root; the first n_specs "
                    "specs of its bundle order at every child" % t_max,
        "witness_blocks": int(len(lens)), "warmup_rounds": args.warmup, "repetitions": reps, "unit": "ms per chain (wall clock); "
        "kernel groups: HIP-event ms summed over the call(s)", "not_timed": "a chain of differing states",
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
