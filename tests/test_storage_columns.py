"""CPU: storage claims in run-compressed, column form — the host-only converter and expansion
(ipcfp_compact_storage_claims / ipcfp_expand_storage_claims, include/ipcfp.h) against a pure-Python restatement written
from the header's byte offsets, the run counts against numpy, the byte arithmetic of the form, the refusals, and the
same under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import ipc_filecoin_proofs_amd as ipcfp
import storage_columns_cases as cases

ROOT = cases.ROOT


def test_header_offsets_describe_192_bytes():
    d = cases.header_defines()
    assert d["IPCFP_SRUN_BYTES"] == 192 and d["IPCFP_SRUN_BYTES"] % 16 == 0
    offs = [d[k] for k in ("IPCFP_SRUN_OFF_CHILD_EPOCH", "IPCFP_SRUN_OFF_ACTOR_ID", "IPCFP_SRUN_OFF_CHILD", "IPCFP_SRUN_OFF_STATE_ROOT",
                           "IPCFP_SRUN_OFF_ACTOR_STATE", "IPCFP_SRUN_OFF_STORAGE_ROOT", "IPCFP_SRUN_OFF_FIRST_CLAIM",
                           "IPCFP_SRUN_OFF_N_CLAIMS", "IPCFP_SRUN_OFF_FLAGS", "IPCFP_SRUN_OFF_RESERVED")]
    assert offs == [0, 8, 16, 56, 96, 136, 176, 180, 184, 188]
    assert d["IPCFP_SRUN_FLAG_MASK"] == 15 and d["IPCFP_SCOL_FLAG_MASK"] == d["IPCFP_SCLAIM_SLOT_PARSED"] | d["IPCFP_SCLAIM_VALUE_MATCHABLE"]


@pytest.mark.parametrize("seed,n", [(1, 20_000), (2, 1), (3, 300), (4, 70_001)])
def test_round_trip_bytes(seed, n):
    cl = cases.random_claims(seed, n)
    assert n < 64 or set(np.unique(cl["flags"]).tolist()) == set(range(64))
    with ipcfp.compact_storage_claims(cl) as cols:
        assert cols.n == n and cols.n_runs == int(cases.run_starts(cl).sum())
        assert cols.nbytes == 65 * n + 192 * cols.n_runs
        assert (cols.cflags & ~np.uint8(48) == 0).all()
        py = cases.python_expand(cols.runs.tobytes(), cols.slot, cols.value, cols.cflags, n)
        assert py == cl.tobytes()
        # the structured view of the run table reads the same bytes
        assert int(cols.runs["n_claims"].sum()) == n and cols.runs["first_claim"][0] == 0
        assert np.array_equal(cols.runs["first_claim"], np.nonzero(cases.run_starts(cl))[0])
        assert ipcfp.expand_storage_claims(cols).tobytes() == cl.tobytes()


def _base(n=6):
    cl = np.zeros(n, dtype=ipcfp.SCLAIM_DTYPE)
    cl["child_epoch"] = 100
    cl["actor_id"] = 7
    for f in ("child", "state_root", "actor_state", "storage_root"):
        cl[f][:, :38] = np.arange(38, dtype=np.uint8) + len(f)
    cl["flags"] = 63
    cl["slot"][:, 31] = np.arange(n)
    return cl


def test_runs_are_maximal_and_split_on_every_key_part():
    with ipcfp.compact_storage_claims(_base()) as cols:
        assert cols.n_runs == 1 and cols.runs["n_claims"][0] == 6 and cols.runs["flags"][0] == 15
    cl = _base()
    cl["child_epoch"][3:] = 101  # neighbours that differ only in child_epoch
    with ipcfp.compact_storage_claims(cl) as cols:
        assert cols.n_runs == 2 == int(cases.run_starts(cl).sum())
        assert cols.runs["child_epoch"].tolist() == [100, 101] and cols.runs["first_claim"].tolist() == [0, 3]
    for bit in (1, 2, 4, 8):  # … only in one CID flag bit
        cl = _base()
        cl["flags"][2] &= ~np.uint32(bit)
        with ipcfp.compact_storage_claims(cl) as cols:
            assert cols.n_runs == 3 == int(cases.run_starts(cl).sum())
            assert cols.runs["flags"].tolist() == [15, 15 & ~bit, 15]
    for f in ("child", "state_root", "actor_state", "storage_root"):  # … only in byte 39 of one CID slot
        cl = _base()
        cl[f][4:, 39] = 1
        with ipcfp.compact_storage_claims(cl) as cols:
            assert cols.n_runs == 2 == int(cases.run_starts(cl).sum())
            assert ipcfp.expand_storage_claims(cols).tobytes() == cl.tobytes()
    cl = _base()
    cl["flags"][1] = 15 | 16  # the claim's own two bits do not split a run
    cl["flags"][2] = 15
    with ipcfp.compact_storage_claims(cl) as cols:
        assert cols.n_runs == 1 and cols.cflags.tolist() == [48, 16, 0, 48, 48, 48]


def test_state_tipset_one_run_per_contract():
    from tools.synth import Tipset

    C, S = 12, 64
    T = Tipset(n_receipts=8, n_planted=0, n_actors=3000, n_contracts=C, slots_per_contract=S, keep_full_state=0, n_actor_queries=4)
    cl = ipcfp.pack_storage_claims(T.child_cid, T.state_root, T.child_epoch, T.sc_actor, T.sc_actor_state, T.sc_storage_root,
                                   T.sc_slot, T.sc_value)
    n = len(cl)
    assert n == C * (S + 1)
    with ipcfp.compact_storage_claims(cl) as cols:
        assert cols.n_runs == C and (cols.runs["n_claims"] == S + 1).all()
        assert cols.nbytes == 65 * n + 192 * C
        # The bound the feature was specified with: a quarter of 296 bytes per claim ((65 + 192 / 65) / 296 = 0.23 for S >= 64).
        # 296 was a miscount of the plain record — sizeof(ipcfp_storage_claim_t) is 248 — so against the real record the
        # form is 0.27, asserted below; the specified bound is kept as it was written.
        assert cols.nbytes <= 0.25 * 296 * n
        assert ipcfp.SCLAIM_DTYPE.itemsize == 248 and cols.nbytes <= 0.28 * ipcfp.SCLAIM_DTYPE.itemsize * n
        assert ipcfp.expand_storage_claims(cols).tobytes() == cl.tobytes()
    # the arithmetic of the full-size batch (10 000 contracts x 257 claims): the form's bytes, the specified comparison
    # with 296 bytes per claim, and the comparison with the record as it is
    n5, c5 = 2_570_000, 10_000
    assert 65 * n5 + 192 * c5 == 168_970_000 and 296 * n5 == 760_720_000 and 248 * n5 == 637_360_000
    assert abs((65 * n5 + 192 * c5) / (296 * n5) - 0.222) < 0.0005
    assert abs((65 * n5 + 192 * c5) / (248 * n5) - 0.265) < 0.0005


def test_refusals_and_empty():
    cl = _base()
    cl["reserved"][3] = 1
    with pytest.raises(ipcfp.EngineError):
        ipcfp.compact_storage_claims(cl)
    for bit in (64, 1 << 31):
        cl = _base()
        cl["flags"][5] |= bit
        with pytest.raises(ipcfp.EngineError):
            ipcfp.compact_storage_claims(cl)
    with ipcfp.compact_storage_claims(np.zeros(0, dtype=ipcfp.SCLAIM_DTYPE)) as cols:
        assert cols.n == 0 and cols.n_runs == 0 and cols.nbytes == 0
        assert len(ipcfp.expand_storage_claims(cols)) == 0


def test_every_declared_column_entry_point_is_bound():
    lib = ipcfp.load_library()
    for name in ("ipcfp_verify_storage_claims", "ipcfp_verify_storage_columns", "ipcfp_verify_storage_columns_device",
                 "ipcfp_expand_storage_claims_device", "ipcfp_compact_storage_claims", "ipcfp_expand_storage_claims",
                 "ipcfp_storage_columns_bytes"):
        assert getattr(lib, name).argtypes is not None
    for name in ("compact_storage_claims", "expand_storage_claims", "StorageColumns"):
        assert name in ipcfp.__all__
    for m in ("verify_storage_columns", "verify_storage_columns_device", "expand_storage_claims_device", "verify_storage_claims"):
        assert callable(getattr(ipcfp.Witness, m))


def test_converter_under_asan_ubsan():
    """`make asan` (csrc/Makefile: host side instrumented) runs the converter and the host expansion, threads included,
    over the round-trip input without a report."""
    rt = "/opt/rocm/lib/llvm/lib/clang"
    runtimes = []
    if os.path.isdir(rt):
        for v in sorted(os.listdir(rt)):
            c = os.path.join(rt, v, "lib", "linux", "libclang_rt.asan-x86_64.so")
            if os.path.exists(c):
                runtimes.append(c)
    try:
        stdcpp = subprocess.run(["gcc", "-print-file-name=libstdc++.so.6"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.SubprocessError):
        stdcpp = ""
    if not runtimes or not os.path.isabs(stdcpp) or not os.path.exists(stdcpp) or not shutil.which("make"):
        pytest.skip("no clang sanitizer runtime here")
    subprocess.run(["make", "-s", "-j8", "-C", os.path.join(ROOT, "ipc-filecoin-proofs_amd", "csrc"), "asan"], check=True, timeout=1800)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1",
               LD_PRELOAD=f"{runtimes[-1]} {stdcpp}", IPCFP_LIB=os.path.join(ROOT, "ipc-filecoin-proofs_amd", "libipcfp_asan.so"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "storage_columns_cases.py")], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0 and "storage columns driver ok" in p.stdout, tail
    assert "runtime error" not in tail and "AddressSanitizer" not in tail, tail
