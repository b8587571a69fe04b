"""GPU: the storage generator finished as column claims resident in HBM (kernels/storage_claims_gen.hip,
ipcfp_generate_storage_claims / _device) — on both routes of the entry point (`hamt_table` 0: one lane per spec, 1: the
per-call node table), and the way from the handle to the column verifier, the string verifier and the wire.

The expected columns are always ipcfp.compact_storage_claims of rows built in numpy from tests/pystorage_gen.py's answer
under the rules of include/ipcfp.h (storage_gen_cases.expected_rows); the status must also be the oracle's; the recorded
blocks must be, id for id, what ipcfp_generate_storage_proofs returns for the same arguments.  The code under test never
supplies its own expectation."""
import numpy as np
import pytest
import torch

import bundle_ref
import claims
import ipc_filecoin_proofs_amd as ipcfp
import pystorage_gen as pg
import storage_chain_cases as sc
import storage_gen_cases as sg
from conftest import fuzz_seed
from test_gpu_limits import make_long_tip
from tools.synth import Tipset

pytestmark = pytest.mark.gpu

T = sg.TREE
ROUTES = (0, 1)


@pytest.fixture()
def routed(engine):
    def use(table):
        engine.set_tuning("hamt_table", table)
    yield use
    engine.set_tuning("hamt_levels", -1)
    engine.set_tuning("hamt_table", -1)
    engine.set_tuning("hamt_coop", -1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def rows_of(g):
    """The handle's host copy expanded to rows in numpy (run record + columns)."""
    runs, slot, value, cflags = g.copy()
    rows = np.zeros(g.n, dtype=ipcfp.SCLAIM_DTYPE)
    covered = np.zeros(g.n, dtype=np.int64)
    for r in runs:
        lo, hi = int(r["first_claim"]), int(r["first_claim"]) + int(r["n_claims"])
        assert hi <= g.n and int(r["reserved"]) == 0 and int(r["n_claims"]) > 0
        covered[lo:hi] += 1
        for f in ("child_epoch", "actor_id", "child", "state_root", "actor_state", "storage_root"):
            rows[f][lo:hi] = r[f]
        rows["flags"][lo:hi] = int(r["flags"]) | cflags[lo:hi]
    assert (covered == 1).all()  # the runs tile [0, n)
    rows["slot"], rows["value"] = slot, value
    return rows


def check(g, want_rows, want_status):
    """status, and the column form byte for byte against compact_storage_claims of the expected rows"""
    assert g.n == len(want_rows)
    assert g.status().tolist() == list(want_status)
    bad = [i for i, s in enumerate(want_status) if s != 1]
    assert g.first_error == (bad[0] if bad else None)
    runs, slot, value, cflags = g.copy()
    with ipcfp.compact_storage_claims(want_rows) as cols:
        assert g.n_runs == cols.n_runs
        assert runs.tobytes() == cols.runs.tobytes()
        assert slot.tobytes() == cols.slot.tobytes() and value.tobytes() == cols.value.tobytes()
        assert cflags.tobytes() == cols.cflags.tobytes()
    assert rows_of(g).tobytes() == np.ascontiguousarray(want_rows).tobytes()
    for p in (g.runs_ptr, g.slot_ptr, g.value_ptr, g.cflags_ptr):
        assert (p % 16 == 0 and p) or g.n == 0


# ---- 1. every posable case of storage_chain_cases.CASES, one witness and one spec each --------------------------------
def test_every_posable_chain_case(engine, oracle, routed):
    skipped, wrong = [], []
    for name, (store, claim, _expect) in sc.CASES.items():
        spec = pg.spec_of(claim)
        if spec is None:
            skipped.append(name)
            continue
        child, aid, slot = spec
        py = pg.generate(store.blocks, child, aid, slot)
        tables = store.tables()
        ost = oracle.store(*tables)
        ost_st = ost.generate_storage_proof(child, aid, slot)[0]
        ost.close()
        ids, slots = np.array([aid], dtype=np.uint64), np.frombuffer(slot, dtype=np.uint8).reshape(1, 32)
        want = sg.expected_rows(ipcfp.SCLAIM_DTYPE, child, sg.EPOCH, ids, slots, [py])
        cids = list(store.blocks)
        with engine.witness(*tables) as w:
            for table in ROUTES:
                routed(table)
                _, old_ids = w.generate_storage_proofs(child, ids, slots)
                with w.generate_storage_claims(child, sg.EPOCH, ids, slots) as g:
                    try:
                        assert py[0] == ost_st
                        check(g, want, [py[0]])
                        assert g.block_ids.tolist() == old_ids.tolist()
                        if py[0] == 1:
                            assert [cids[i] for i in g.block_ids] == py[2]
                    except AssertionError as e:
                        wrong.append((name, table, str(e)[:300]))
    assert not wrong, wrong[:5]
    assert len(skipped) <= 12, skipped


# ---- 2. one hand-built state tree under one child header ---------------------------------------------------------------
def _batches():
    names = list(T.contracts)
    natural = T.runs([(c, len(T.contracts[c][1])) for c in names])
    out = {f"n{n}": natural[:n] for n in (0, 1, 63, 64, 65, 257)}
    out["run_lengths_1_2_64_65_257"] = T.runs([("a1", 1), ("b2", 2), ("many6", 64), ("c", 65), ("many5", 257)])
    out["every_spec_its_own_run"] = [(c, k) for k in range(2) for c in names]
    out["one_run"] = T.runs([("many5", 300)])
    out["same_actor_in_two_runs"] = T.runs([("a2", 2), ("evm_absent", 2), ("a2", 3), ("path_fork", 3), ("root_absent", 2), ("a2", 1)])
    rng = np.random.default_rng(fuzz_seed(7300))
    out["shuffled"] = T.runs([(names[int(rng.integers(len(names)))], int(rng.integers(1, 6))) for _ in range(90)])
    out["successes"] = T.runs([(c, min(len(T.contracts[c][1]), 40)) for c in T.successes()])
    return out


BATCHES = _batches()


@pytest.fixture(scope="module")
def tree(engine, oracle):
    w = engine.witness(*T.store.tables())
    ost = oracle.store(*T.store.tables())
    yield w, ost
    ost.close()
    w.close()


def tree_expect(ost, ids, slots):
    answers = [T.py(a, s.tobytes()) for a, s in zip(ids, slots)]
    for a, s, py in zip(ids, slots, answers):
        assert T.oracle(ost, a, s.tobytes())[0] == py[0]
    return answers, sg.expected_rows(ipcfp.SCLAIM_DTYPE, T.child, sg.EPOCH, ids, slots, answers)


@pytest.mark.parametrize("table", ROUTES)
@pytest.mark.parametrize("name", list(BATCHES))
def test_batches_over_the_tree(tree, routed, name, table):
    w, ost = tree
    ids, slots, lit = T.batch(BATCHES[name])
    answers, want = tree_expect(ost, ids, slots)
    assert [a[0] for a in answers] == lit
    routed(table)
    _, old_ids = w.generate_storage_proofs(T.child, ids, slots)
    with w.generate_storage_claims(T.child, sg.EPOCH, ids, slots) as g:
        check(g, want, lit)
        assert g.block_ids.tolist() == old_ids.tolist()
        if all(s == 1 for s in lit):
            orc = sg.union_ord([T.oracle(ost, a, s.tobytes())[3] for a, s in zip(ids, slots)])
            assert [T.cids[i] for i in g.block_ids] == orc == sg.union_ord([a[2] for a in answers])
    if name == "shuffled":
        assert len(set(lit)) >= 4
    if name == "run_lengths_1_2_64_65_257":
        assert g.n_runs == 5


# ---- 3. a state tree whose nodes go to the 32-lane outline ---------------------------------------------------------------
@pytest.mark.parametrize("table", ROUTES)
def test_state_tree_wide_enough_for_the_outline(engine, oracle, routed, table):
    store, claim, parts = sc.chain(sc.layout("C", sc.PAIRS), sc.S[2], sc.VAL[2], salt=1, n_actors=3000)
    assert max(len(b) for b in store.blocks.values()) >= 2048
    child = parts["child"]
    picks = [(1001, sc.S[2]), (1001, sc.ABSENT), (999_999, sc.S[2]), (2500, sc.S[2]), (2500, sc.S[1]), (1001, sc.S[1])]
    ids = np.array([a for a, _ in picks], dtype=np.uint64)
    slots = np.stack([np.frombuffer(s, dtype=np.uint8) for _, s in picks])
    answers = [pg.generate(store.blocks, child, a, s) for a, s in picks]
    assert [a[0] for a in answers] == [1, 1, 68, 65, 65, 1]
    ost = oracle.store(*store.tables())
    assert [ost.generate_storage_proof(child, a, s)[0] for a, s in picks] == [a[0] for a in answers]
    ost.close()
    want = sg.expected_rows(ipcfp.SCLAIM_DTYPE, child, sg.EPOCH, ids, slots, answers)
    with engine.witness(*store.tables()) as w:
        routed(table)
        _, old_ids = w.generate_storage_proofs(child, ids, slots)
        with w.generate_storage_claims(child, sg.EPOCH, ids, slots) as g:
            check(g, want, [a[0] for a in answers])
            assert g.block_ids.tolist() == old_ids.tolist()


# ---- 4. the device-spec entry point; the handle's pointers into the column verifier ------------------------------------
@pytest.mark.parametrize("table", ROUTES)
def test_device_specs_and_the_column_verifier(engine, oracle, tree, routed, table):
    w, ost = tree
    ids, slots, lit = T.batch(BATCHES["shuffled"])
    answers, want = tree_expect(ost, ids, slots)
    routed(table)
    d_ids, d_slots = dev(ids), dev(slots)
    assert d_slots.data_ptr() % 16 == 0
    with w.generate_storage_claims(T.child, sg.EPOCH, ids, slots) as h, \
            w.generate_storage_claims_device(T.child, sg.EPOCH, d_ids.data_ptr(), d_slots.data_ptr(), len(ids)) as g:
        check(g, want, lit)
        assert g.block_ids.tolist() == h.block_ids.tolist()
        assert [x.tobytes() for x in g.copy()] == [x.tobytes() for x in h.copy()]
        # the handle's own device pointers against the witness pruned to the recorded blocks
        sub = g.block_ids.astype(np.int64)
        data, off, lens, c40 = T.store.tables()
        d_st = torch.zeros(g.n, dtype=torch.uint8, device="cuda")
        d_rows = torch.zeros(g.n * ipcfp.SCLAIM_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        with engine.witness(data, off[sub], lens[sub], c40[sub]) as pw:
            pw.verify_storage_columns_device(g.runs_ptr, g.n_runs, g.slot_ptr, g.value_ptr, g.cflags_ptr, g.n, d_st.data_ptr())
            pw.expand_storage_claims_device(g.runs_ptr, g.n_runs, g.slot_ptr, g.value_ptr, g.cflags_ptr, g.n, d_rows.data_ptr())
        got = d_st.cpu().numpy()
        assert got.tolist() == [1 if s == 1 else 69 for s in lit]
        rows = d_rows.cpu().numpy().view(ipcfp.SCLAIM_DTYPE)
        assert rows.tobytes() == np.ascontiguousarray(want).tobytes()
        # the oracle's string verifier over the expanded rows (it takes rows with every flag set: the status-1 specs)
        ok = np.array([s == 1 for s in lit])
        pst = oracle.store(data, off[sub], lens[sub], c40[sub])
        assert (pst.verify_storage_claims_packed(rows[ok]) == 1).all()
        pst.close()


@pytest.mark.parametrize("table", ROUTES)
def test_every_recorded_block_is_needed(engine, tree, routed, table):
    """the all-success batch: without any one block of the pruned witness at least one proof no longer verifies"""
    w, ost = tree
    ids, slots, lit = T.batch(BATCHES["successes"])
    assert all(s == 1 for s in lit)
    routed(table)
    data, off, lens, c40 = T.store.tables()
    with w.generate_storage_claims(T.child, sg.EPOCH, ids, slots) as g:
        d_st = torch.zeros(g.n, dtype=torch.uint8, device="cuda")
        sub = g.block_ids.astype(np.int64)
        assert 10 < len(sub) < 200
        for drop in range(len(sub)):
            keep = np.delete(sub, drop)
            with engine.witness(data, off[keep], lens[keep], c40[keep]) as pw:
                pw.verify_storage_columns_device(g.runs_ptr, g.n_runs, g.slot_ptr, g.value_ptr, g.cflags_ptr, g.n, d_st.data_ptr())
            assert not (d_st.cpu().numpy() == 1).all(), drop


# ---- 5. strings and the bundle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ROUTES)
def test_strings_and_the_bundle(engine, tree, routed, table):
    w, ost = tree
    ids, slots, lit = T.batch(BATCHES["successes"])
    answers, want = tree_expect(ost, ids, slots)
    routed(table)
    with w.generate_storage_claims(T.child, sg.EPOCH, ids, slots) as g:
        p, n = g.proofs()
        assert n == g.n == len(ids)
        dicts = [dict(child_epoch=sg.EPOCH, child_block_cid=sc.cid_str(T.child), parent_state_root=sc.cid_str(a[1]["parent_state_root"]),
                      actor_id=int(i), actor_state_cid=sc.cid_str(a[1]["actor_state_cid"]), storage_root=sc.cid_str(a[1]["storage_root"]),
                      slot=sc.hex0x(s.tobytes()), value=sc.hex0x(a[1]["value"])) for i, s, a in zip(ids, slots, answers)]
        assert g.proof_rows() == dicts
        text = w.write_bundle_json(p, n, None, 0, block_ids=g.block_ids)
        blocks = [(T.cids[i], T.store.blocks[T.cids[i]]) for i in g.block_ids]
        assert text == bundle_ref.bundle_json(dicts, [], blocks).encode()
        b = engine.bundle(text)
        try:
            ss, es = b.verify()
        finally:
            b.close()
        assert len(ss) == g.n and (ss == 1).all() and len(es) == 0
        assert (w.verify_storage_proofs(p, n) == 1).all()  # the strings through the string verifier, too
    # a handle with a failing spec has no proofs: IPCFP_E_INVALID at first_error
    ids, slots, lit = T.batch(BATCHES["same_actor_in_two_runs"])
    with w.generate_storage_claims(T.child, sg.EPOCH, ids, slots) as g:
        first = [i for i, s in enumerate(lit) if s != 1][0]
        assert g.first_error == first > 0
        with pytest.raises(ipcfp.EngineError) as e:
            g.proofs()
        assert e.value.rc == -1 and e.value.bad_index == first
    with w.generate_storage_claims(T.child, sg.EPOCH, ids[:0], slots[:0]) as g:
        assert g.n == 0 and g.n_runs == 0 and g.first_error is None and g.proofs()[1] == 0 and len(g.block_ids) == 0


@pytest.mark.parametrize("table", ROUTES)
def test_long_cids(engine, routed, table):
    """CIDs longer than the slot: the columns carry the folds, equal the lowering of the long CID strings and verify; the
    string form does not exist."""
    tip, rw = make_long_tip()
    data, off, lens = rw.tables()
    slots40 = ipcfp.cid_slots(rw.cids)
    child_long = rw.renamed[tip.child_cid[:38]]
    scl = claims.StorageClaims(tip)
    for k in range(scl.n):
        scl.set_str(k, "child_block_cid", rw.s(tip.child_cid))
    want = ipcfp.pack_storage_proofs(scl.arr, scl.n)
    routed(table)
    with engine.witness(data, off, lens, slots40) as w:
        assert (w.verify_storage_claims(want) == 1).all()
        _, old_ids = w.generate_storage_proofs(child_long, tip.sc_actor, tip.sc_slot)
        with w.generate_storage_claims(child_long, tip.child_epoch, tip.sc_actor, tip.sc_slot) as g:
            check(g, want, [1] * scl.n)
            assert g.block_ids.tolist() == old_ids.tolist()
            runs = g.copy()[0]
            assert (runs["child"][:, 0] == 0xFF).all() and (slots40[g.block_ids, 0] == 0xFF).sum() >= 2
            d_st = torch.zeros(g.n, dtype=torch.uint8, device="cuda")
            w.verify_storage_columns_device(g.runs_ptr, g.n_runs, g.slot_ptr, g.value_ptr, g.cflags_ptr, g.n, d_st.data_ptr())
            assert (d_st.cpu().numpy() == 1).all()
            with pytest.raises(ipcfp.EngineError) as e:
                g.proofs()
            assert e.value.rc == -5 and e.value.bad_index == 0


# ---- 6. the synthetic tipset's claim table -------------------------------------------------------------------------------
@pytest.mark.parametrize("table", ROUTES)
def test_synthetic_tipset(engine, routed, table):
    tip = Tipset(n_receipts=300, n_parents=2, n_planted=2, variety=1, max_events=4, n_actors=1500, n_contracts=8,
                 slots_per_contract=12, storage_layout_mix=1, n_actor_queries=6)
    scl = claims.StorageClaims(tip)
    want = ipcfp.pack_storage_proofs(scl.arr, scl.n)
    assert scl.n >= 8 * 12
    routed(table)
    with engine.witness(tip.data, tip.off, tip.lens, tip.cids) as w:
        _, old_ids = w.generate_storage_proofs(tip.child_cid, tip.sc_actor, tip.sc_slot)
        with w.generate_storage_claims(tip.child_cid, tip.child_epoch, tip.sc_actor, tip.sc_slot) as g:
            check(g, want, [1] * scl.n)
            assert g.n_runs == 1 + int((tip.sc_actor[1:] != tip.sc_actor[:-1]).sum()) >= 8
            assert np.array_equal(g.copy()[2], tip.sc_value)
            assert g.block_ids.tolist() == old_ids.tolist()
