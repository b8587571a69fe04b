"""Shared by tests/test_storage_columns.py (CPU) and tests/test_gpu_storage_columns.py (GPU): random plain storage claims
with repeated keys, a pure-Python restatement of the column form (include/ipcfp.h "storage claims in run-compressed,
column form") written from the header's byte offsets, and the sanitizer build's driver."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_defines():
    """{name: int} of the header's `#define IPCFP_S… <number>u` lines."""
    text = open(os.path.join(ROOT, "include", "ipcfp.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (IPCFP_S[A-Z_]+) (\d+)u", text)}


KEY_FIELDS = ("child_epoch", "actor_id", "child", "state_root", "actor_state", "storage_root")


def random_claims(seed: int, n: int, max_run: int = 300):
    """SCLAIM_DTYPE[n]: runs of random length 1…max_run made by repeating keys, some CIDs unparsed (the all-ones key
    parse_cid_claim writes), all 64 flag values."""
    import ipc_filecoin_proofs_amd as ipcfp

    rng = np.random.default_rng(seed)
    cl = np.zeros(n, dtype=ipcfp.SCLAIM_DTYPE)
    i = 0
    while i < n:
        k = min(int(rng.integers(1, max_run + 1)), n - i)
        key = np.zeros(1, dtype=ipcfp.SCLAIM_DTYPE)
        key["child_epoch"] = rng.integers(-5, 1 << 40)
        key["actor_id"] = rng.integers(0, 1 << 62)
        for f in ("child", "state_root", "actor_state", "storage_root"):
            c = rng.integers(0, 256, 40, dtype=np.uint8)
            c[38:] = 0
            if rng.integers(0, 8) == 0:
                c[:] = 0xFF  # unparsed
            key[f][0] = c
        cid_flags = int(rng.integers(0, 16))
        for f in KEY_FIELDS:
            cl[f][i:i + k] = key[f][0]
        cl["flags"][i:i + k] = cid_flags | (rng.integers(0, 4, k) << 4)
        i += k
    cl["slot"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    cl["value"] = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    # every one of the 64 flag values somewhere (a change of the CID bits starts a run: the counts below know)
    if n >= 64:
        cl["flags"][n - 64:] = np.arange(64)
    return cl


def run_starts(cl) -> np.ndarray:
    """bool[n]: claim i starts a maximal run (numpy restatement: key fields or the four CID flag bits differ)."""
    n = len(cl)
    s = np.zeros(n, dtype=bool)
    if n:
        s[0] = True
    for f in KEY_FIELDS:
        a = cl[f]
        d = a[1:] != a[:-1]
        s[1:] |= d if d.ndim == 1 else d.any(axis=1)
    s[1:] |= ((cl["flags"][1:] ^ cl["flags"][:-1]) & 15) != 0
    return s


def python_expand(runs_bytes: bytes, slot, value, cflags, n: int) -> bytes:
    """The plain 248-byte records from the column form, from the header's offsets alone."""
    d = header_defines()
    rb = d["IPCFP_SRUN_BYTES"]
    out = bytearray(248 * n)
    covered = 0
    for r in range(len(runs_bytes) // rb):
        rec = runs_bytes[r * rb:(r + 1) * rb]
        u32 = lambda o: int.from_bytes(rec[o:o + 4], "little")  # noqa: E731
        first, cnt, flags, res = (u32(d["IPCFP_SRUN_OFF_FIRST_CLAIM"]), u32(d["IPCFP_SRUN_OFF_N_CLAIMS"]),
                                  u32(d["IPCFP_SRUN_OFF_FLAGS"]), u32(d["IPCFP_SRUN_OFF_RESERVED"]))
        assert first == covered and cnt > 0 and res == 0 and flags & ~d["IPCFP_SRUN_FLAG_MASK"] == 0
        head = (rec[d["IPCFP_SRUN_OFF_CHILD_EPOCH"]:][:8] + rec[d["IPCFP_SRUN_OFF_ACTOR_ID"]:][:8] + rec[d["IPCFP_SRUN_OFF_CHILD"]:][:40]
                + rec[d["IPCFP_SRUN_OFF_STATE_ROOT"]:][:40] + rec[d["IPCFP_SRUN_OFF_ACTOR_STATE"]:][:40]
                + rec[d["IPCFP_SRUN_OFF_STORAGE_ROOT"]:][:40])
        for t in range(first, first + cnt):
            assert int(cflags[t]) & ~d["IPCFP_SCOL_FLAG_MASK"] == 0
            out[248 * t:248 * (t + 1)] = (head + bytes(slot[t]) + bytes(value[t]) + (flags | int(cflags[t])).to_bytes(4, "little")
                                          + (0).to_bytes(4, "little"))
        covered += cnt
    assert covered == n
    return bytes(out)


def roundtrip_driver():
    """What the sanitizer build runs: the converter and the host expansion over the round-trip input (threads included)."""
    import ipc_filecoin_proofs_amd as ipcfp

    for seed, n in ((11, 50_000), (12, 1), (13, 4097)):
        cl = random_claims(seed, n)
        with ipcfp.compact_storage_claims(cl) as cols:
            assert cols.n_runs == int(run_starts(cl).sum())
            back = ipcfp.expand_storage_claims(cols)
        assert back.tobytes() == cl.tobytes()
    with ipcfp.compact_storage_claims(np.zeros(0, dtype=ipcfp.SCLAIM_DTYPE)) as cols:
        assert cols.n == 0 and cols.n_runs == 0
    print("storage columns driver ok")


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    roundtrip_driver()
