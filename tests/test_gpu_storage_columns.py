"""GPU: storage claims in run-compressed, column form (include/ipcfp.h) — device expansion, and the verdicts of
ipcfp_verify_storage_columns_device / ipcfp_verify_storage_columns / ipcfp_verify_storage_claims against the CPU oracle on
the PLAIN claims the columns were made from and against the plain device route, bit-exact.  The form is untrusted input:
malformed run tables are refused (IPCFP_E_INVALID) by bounds checks that never leave the arrays, unknown flag bits make
exactly the claims concerned ERR_BAD_CLAIM."""
import numpy as np
import pytest

import claims
import ipc_filecoin_proofs_amd as ipcfp
import storage_columns_cases as cases
from conftest import fuzz_seed
from tools.synth import SEED_BASE, Tipset

pytestmark = pytest.mark.gpu

TABLE_MODES = (0, 1, -1)  # the `hamt_table` tuning key: one-lane kernel alone, node table forced, default


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def columns_device(w, runs, slot, value, cflags, n, trust=None, n_runs=None):
    """ipcfp_verify_storage_columns_device over numpy copies of the form → status u8[n] (host)."""
    import torch

    d = [_dev(runs), _dev(slot), _dev(value), _dev(cflags)]
    st = torch.full((max(n, 1),), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w.verify_storage_columns_device(d[0].data_ptr(), len(runs) if n_runs is None else n_runs, d[1].data_ptr(), d[2].data_ptr(),
                                    d[3].data_ptr(), n, st.data_ptr(), trust=trust)
    return st.cpu().numpy()[:n]


def plain_device(w, cl, trust=None):
    import torch

    d_cl = _dev(cl)
    st = torch.full((len(cl),), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w.verify_storage_claims_device(d_cl.data_ptr(), len(cl), st.data_ptr(), trust=trust)
    return st.cpu().numpy()


def expand_device(w, runs, slot, value, cflags, n):
    import torch

    d = [_dev(runs), _dev(slot), _dev(value), _dev(cflags)]
    out = torch.full((max(n, 1) * 248,), 0xAA, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    w.expand_storage_claims_device(d[0].data_ptr(), len(runs), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, out.data_ptr())
    return out.cpu().numpy()[: n * 248].tobytes()


def all_routes(engine, w, cl, trust=None):
    """{route: status} of the column form of `cl` over every table mode and both transports, plus the plain routes."""
    out = {}
    with ipcfp.compact_storage_claims(cl) as cols:
        for mode in TABLE_MODES:
            engine.set_tuning("hamt_table", mode)
            try:
                out[("columns_device", mode)] = columns_device(w, cols.runs, cols.slot, cols.value, cols.cflags, cols.n, trust=trust)
                out[("columns_host", mode)] = w.verify_storage_columns(cols, trust=trust)
                out[("plain_device", mode)] = plain_device(w, cl, trust=trust)
                out[("plain_host", mode)] = w.verify_storage_claims(cl, trust=trust)
            finally:
                engine.set_tuning("hamt_table", -1)
    return out


@pytest.fixture(scope="module")
def tip():
    # six storage-root layouts (storage_layout_mix): the inline small maps go to the one-lane kernel (the pending path)
    return Tipset(n_receipts=3000, n_planted=7, variety=1, n_actors=20000, n_contracts=18, slots_per_contract=40,
                  storage_layout_mix=1, n_actor_queries=500, keep_full_state=0)


@pytest.fixture(scope="module")
def both(tip, engine, oracle):
    w = engine.witness(tip.data, tip.off, tip.lens, tip.cids)
    st = oracle.store(tip.data, tip.off, tip.lens, tip.cids)
    yield w, st
    w.close()
    st.close()


def tip_claims(T):
    return ipcfp.pack_storage_claims(T.child_cid, T.state_root, T.child_epoch, T.sc_actor, T.sc_actor_state, T.sc_storage_root,
                                     T.sc_slot, T.sc_value)


def test_device_expansion_is_the_plain_bytes(tip, both):
    w, _ = both
    for cl in (tip_claims(tip), cases.random_claims(fuzz_seed(21), 30_001), cases.random_claims(fuzz_seed(22), 1),
               cases.random_claims(fuzz_seed(23), 2, max_run=1)):
        with ipcfp.compact_storage_claims(cl) as cols:
            assert expand_device(w, cols.runs, cols.slot, cols.value, cols.cflags, cols.n) == cl.tobytes()


def test_all_layouts_status_parity(tip, both, engine):
    w, st = both
    sc = claims.StorageClaims(tip)
    cl = ipcfp.pack_storage_proofs(sc.arr, sc.n)
    assert cl.tobytes() == tip_claims(tip).tobytes()
    want = st.verify_storage_proofs(sc, mode=1)
    assert (want == 1).all() and np.array_equal(want, st.verify_storage_claims_packed(cl))
    for route, got in all_routes(engine, w, cl).items():
        assert np.array_equal(got, want), route


def adversarial(tip, oracle):
    """The 40 claims of tests/test_gpu_walks.py::test_storage_proofs_adversarial, sixteen of them adversarial."""
    n = 40
    sc = claims.StorageClaims(tip, indices=np.arange(n))
    upper = lambda s: s.decode().upper().encode()  # noqa: E731
    sc.set_str(0, "value", "0x" + "00" * 32)
    sc.set_str(1, "value", sc.arr[1].value.decode().upper().replace("0X", "0x"))
    sc.set_str(2, "value", sc.arr[2].value.decode()[:-2])
    sc.set_str(3, "slot", sc.arr[3].slot.decode()[2:])
    sc.set_str(4, "slot", "0x0x" + sc.arr[4].slot.decode()[2:])
    sc.set_str(5, "slot", "0x1234")
    sc.set_str(6, "child_block_cid", "garbage")
    sc.set_str(7, "parent_state_root", upper(sc.arr[7].parent_state_root))
    sc.set_str(8, "actor_state_cid", "f" + tip.sc_actor_state[8][:38].tobytes().hex())
    sc.set_str(9, "storage_root", claims.cid_str(oracle.cid_for_block(b"other")))
    absent = [int(i) for i, pr in zip(tip.query_ids, tip.query_present) if not pr]
    sc.arr[10].actor_id = absent[0]
    sc.arr[11].actor_id = int(tip.sc_actor[11]) + 1
    sc.set_str(12, "child_block_cid", claims.cid_str(oracle.cid_for_block(b"nohdr")))
    sc.set_str(13, "child_block_cid", claims.cid_str(tip.receipts_root))
    sc.arr[14].child_epoch = 5
    sc.set_str(15, "value", "0X" + sc.arr[15].value.decode()[2:])
    return sc


def test_adversarial_status_parity(tip, both, engine, oracle):
    w, st = both
    sc = adversarial(tip, oracle)
    cl = ipcfp.pack_storage_proofs(sc.arr, sc.n)
    want = st.verify_storage_proofs(sc, mode=0)
    for route, got in all_routes(engine, w, cl).items():
        assert np.array_equal(got, want), (route, got.tolist(), want.tolist())
        assert got[5] == 69 and got[6] == 69 and got[10] == 68 and got[12] == 65 and got[13] == 66, route
        assert got[7] == 18 and got[8] == 19 and got[9] == 20 and got[11] == 19, route
        assert got[1] == 1 and got[3] == 1 and got[4] == 1 and got[14] == 1 and got[15] == 1, route
    tp = claims.TrustPolicy(kind=1, ec_chain_empty=0, min_epoch=tip.child_epoch + 1, max_epoch=tip.child_epoch + 9)
    want = st.verify_storage_proofs(sc, trust=tp, mode=0)
    for route, got in all_routes(engine, w, cl, trust=tp).items():
        assert np.array_equal(got, want), (route, got.tolist(), want.tolist())
        assert got[0] == 3 and got[6] == 69 and got[14] == 3, route


def split_runs(runs, rng):
    """Every run of length >= 2 cut in two at a random point (a legal, non-maximal table)."""
    out = []
    for r in runs:
        k = int(r["n_claims"])
        if k < 2:
            out.append(r.copy())
            continue
        cut = int(rng.integers(1, k))
        a, b = r.copy(), r.copy()
        a["n_claims"] = cut
        b["first_claim"] = int(r["first_claim"]) + cut
        b["n_claims"] = k - cut
        out += [a, b]
    return np.array(out, dtype=runs.dtype)


def test_run_shapes(tip, both, engine):
    w, st = both
    rng = np.random.default_rng(fuzz_seed(31))
    cl = tip_claims(tip)
    wrong = np.arange(3, len(cl), 7)
    cl["value"][wrong, 0] ^= 0x10
    want = st.verify_storage_claims_packed(cl)
    assert (want[wrong] == 21).all() and (want != 255).all()
    # every run of length 1: the claims shuffled until no two neighbours share a contract
    perm = rng.permutation(len(cl))
    sh = cl[perm]
    for _ in range(50):
        same = np.nonzero(sh["actor_id"][1:] == sh["actor_id"][:-1])[0]
        if not len(same):
            break
        for i in same:
            j = int(rng.integers(0, len(sh)))
            sh[[i, j]] = sh[[j, i]]
            perm[[i, j]] = perm[[j, i]]
    assert (sh["actor_id"][1:] != sh["actor_id"][:-1]).all()
    for mode in TABLE_MODES:
        engine.set_tuning("hamt_table", mode)
        try:
            with ipcfp.compact_storage_claims(sh) as cols:
                assert cols.n_runs == cols.n
                got = columns_device(w, cols.runs, cols.slot, cols.value, cols.cflags, cols.n)
            assert np.array_equal(got, want[perm]) and np.array_equal(got, plain_device(w, sh)), mode
            # the maximal table with every run split in two
            with ipcfp.compact_storage_claims(cl) as cols:
                runs2 = split_runs(cols.runs, rng)
                assert len(runs2) > cols.n_runs and int(runs2["n_claims"].sum()) == cols.n
                got = columns_device(w, runs2, cols.slot, cols.value, cols.cflags, cols.n)
            assert np.array_equal(got, want), mode
        finally:
            engine.set_tuning("hamt_table", -1)
    # claims that differ only in child_epoch, under a policy that accepts one epoch and not the other
    ep = cl[: 3 * 41].copy()
    other = np.arange(len(ep)) % 5 == 2
    ep["child_epoch"][other] = tip.child_epoch + 100
    tp = claims.TrustPolicy(kind=1, ec_chain_empty=0, min_epoch=tip.child_epoch - 1, max_epoch=tip.child_epoch + 1)
    want_ep = st.verify_storage_claims_packed(ep, trust=tp)
    assert (want_ep[other] == 3).all() and (want_ep[~other] != 3).all()
    for route, got in all_routes(engine, w, ep, trust=tp).items():
        assert np.array_equal(got, want_ep), route


def test_malformed_run_tables_are_refused(tip, both, engine):
    """Bounds checks of untrusted input: every violation of the tiling rule is IPCFP_E_INVALID, with no verdicts."""
    w, _ = both
    cl = tip_claims(tip)
    with ipcfp.compact_storage_claims(cl) as cols:
        runs, slot, value, cflags, n = cols.runs.copy(), cols.slot.copy(), cols.value.copy(), cols.cflags.copy(), cols.n
    assert len(runs) >= 4

    def broken(edit):
        r = runs.copy()
        edit(r)
        return r

    def first_not_zero(r):
        r["first_claim"][0] = 1
        r["n_claims"][0] -= 1

    def empty_run(r):  # run 1 empty, run 0 stretched over its claims: only n_claims == 0 breaks the rule
        r["n_claims"][0] += r["n_claims"][1]
        r["first_claim"][1] += r["n_claims"][1]
        r["n_claims"][1] = 0

    def gap(r):
        r["n_claims"][1] -= 1

    def overlap(r):
        r["n_claims"][1] += 1

    def short_end(r):
        r["n_claims"][-1] -= 1

    def long_end(r):
        r["n_claims"][-1] += 1

    def far_out(r):  # sums that wrap 32 bits, starts far outside the batch
        r["first_claim"][2] = 0xFFFFFFF0
        r["n_claims"][2] = 0x20

    def huge(r):
        r["n_claims"][0] = 0xFFFFFFFF

    for mode in TABLE_MODES:
        engine.set_tuning("hamt_table", mode)
        try:
            for edit in (first_not_zero, empty_run, gap, overlap, short_end, long_end, far_out, huge):
                with pytest.raises(ipcfp.EngineError, match="invalid argument"):
                    columns_device(w, broken(edit), slot, value, cflags, n)
                with pytest.raises(ipcfp.EngineError, match="invalid argument"):
                    expand_device(w, broken(edit), slot, value, cflags, n)
            with pytest.raises(ipcfp.EngineError, match="invalid argument"):
                columns_device(w, runs, slot, value, cflags, n, n_runs=0)
            with pytest.raises(ipcfp.EngineError, match="invalid argument"):  # a table cut short: its last run does not reach n
                columns_device(w, runs[:-1], slot, value, cflags, n)
            # and the sound table still verifies on the same context afterwards
            assert (columns_device(w, runs, slot, value, cflags, n) == 1).all()
        finally:
            engine.set_tuning("hamt_table", -1)


def test_unknown_flag_bits_are_bad_claims(tip, both, engine):
    w, st = both
    cl = tip_claims(tip)
    want = st.verify_storage_claims_packed(cl)
    with ipcfp.compact_storage_claims(cl) as cols:
        runs, slot, value, cflags, n = cols.runs.copy(), cols.slot.copy(), cols.value.copy(), cols.cflags.copy(), cols.n
    runs["flags"][1] |= 16          # a claim's bit in a run's word
    runs["flags"][3] |= 1 << 31
    runs["reserved"][5] = 7
    cflags[[0, n - 1]] |= 1         # a run's bit in a claim's byte
    cflags[100] |= 64
    cflags[101] = 0xFF
    bad = np.zeros(n, dtype=bool)
    for r in (1, 3, 5):
        bad[int(runs["first_claim"][r]): int(runs["first_claim"][r]) + int(runs["n_claims"][r])] = True
    bad[[0, n - 1, 100, 101]] = True
    for mode in TABLE_MODES:
        engine.set_tuning("hamt_table", mode)
        try:
            got = columns_device(w, runs, slot, value, cflags, n)
        finally:
            engine.set_tuning("hamt_table", -1)
        assert (got[bad] == 69).all() and np.array_equal(got[~bad], want[~bad]), mode


@pytest.mark.parametrize("k", [0, 1, 2])
def test_further_corpora(k, engine, oracle):
    seed = fuzz_seed(4100 + k)
    rng = np.random.default_rng(seed)
    T = Tipset(seed=seed, n_receipts=200, n_planted=2, variety=1, n_actors=5000 + 3000 * k, n_contracts=7 + 5 * k,
               slots_per_contract=int(rng.integers(1, 70)), storage_layout_mix=1, n_actor_queries=50, keep_full_state=0)
    cl = tip_claims(T)
    n = len(cl)
    cl["value"][rng.integers(0, n, n // 9), 31] ^= 1
    cl["slot"][rng.integers(0, n, n // 11), 3] ^= 0x40           # a slot nobody wrote: zero, or the claimed value is wrong
    cl["flags"][rng.integers(0, n, n // 13)] &= ~np.uint32(1 << int(rng.integers(0, 6)))
    cl["actor_id"][rng.integers(0, n, 3)] += 1
    cl["storage_root"][rng.integers(0, n, 3), 20] ^= 1
    cl["child_epoch"][rng.integers(0, n, 5)] += 1000
    tp = claims.TrustPolicy(kind=1, ec_chain_empty=0, min_epoch=T.child_epoch, max_epoch=T.child_epoch + 10)
    ost = oracle.store(T.data, T.off, T.lens, T.cids)
    with engine.witness(T.data, T.off, T.lens, T.cids) as w:
        for trust in (None, tp):
            routes = all_routes(engine, w, cl, trust=trust)
            ref = routes[("plain_device", -1)]
            for route, got in routes.items():
                assert np.array_equal(got, ref), (seed, route)
        # the oracle's packed entry point reads claims whose strings are canonical: compare where every flag is set
        full = cl["flags"] == 63
        want = ost.verify_storage_claims_packed(cl[full], trust=tp)
        assert np.array_equal(routes[("columns_device", -1)][full], want), seed
    ost.close()


@pytest.fixture(scope="module")
def state():
    return Tipset(seed=SEED_BASE + 4, n_receipts=8, n_planted=0, n_actors=4_000_000, n_contracts=10_000,
                  slots_per_contract=256, keep_full_state=0, n_actor_queries=int(65536 * 1.01))


def test_full_size_every_storage_proof(state, engine, oracle):
    import torch

    T = state
    cl = tip_claims(T)
    n = len(cl)
    assert n == 2_570_000
    wrong = np.arange(500, n, 1000)
    cl["value"][wrong, 31] ^= 1
    ost = oracle.store(T.data, T.off, T.lens, T.cids, threads=0)
    want = ost.verify_storage_claims_packed(cl, threads=0)
    ost.close()
    assert (want != 255).all() and len(wrong) == 2570
    assert (want[wrong] == 21).all() and (want == 1).sum() == n - len(wrong)
    with ipcfp.compact_storage_claims(cl) as cols, engine.witness(T.data, T.off, T.lens, T.cids) as w:
        assert cols.n_runs == 10_000 and cols.nbytes == 65 * n + 192 * 10_000
        got = columns_device(w, cols.runs, cols.slot, cols.value, cols.cflags, n)
        assert np.array_equal(got, want)
        assert np.array_equal(plain_device(w, cl), want)
        assert np.array_equal(w.verify_storage_columns(cols), want)
        assert np.array_equal(w.verify_storage_claims(cl), want)
        assert expand_device(w, cols.runs, cols.slot, cols.value, cols.cflags, n) == cl.tobytes()
    torch.cuda.empty_cache()
