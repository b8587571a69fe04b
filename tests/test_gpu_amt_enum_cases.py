"""GPU: the AMT enumerator's named cases (tests/amt_enum_cases.py) through every entry point that enumerates —

    scan            scan_events, whole or under the case's receipt range; once more on a witness made under IPCFP_EVENT_TABLE=0
    exec_order      reconstruct_execution_order
    packed_fast     verify_event_claims, fast_verify = 1, on first contact: the table route (host/verify_fast.cpp), whose dense
                    walk ends in k_dense_receipt_leaves — `amt_walk` says whether it was queued
    packed_general  the same claims, fast_verify = 0
    strings         verify_event_proofs
    one_call        verify_and_scan_device (a subset: its buffers are sized by the case's receipts)
    generate        generate_event_proofs, and the shard planner, for the cases that run without a range

— against the case's LITERALS, and where the literal says TRUE against the oracle for what a literal does not hold: the
touched block set (under a range: pyevents' for up to 10 000 receipts, the oracle's where the range is the whole tree; the one
ranged case above that, across the middle of 65 537, goes without), the execution order's bytes, the generator's messages and
witness ids.  Every scan is made twice: the second answer must be the first's and must not have walked.  One witness per case; the cases
of the small trees once more MERGED into one witness, every tree scanned twice (the second answer comes from the witness's
cache of enumerations, which must not answer for another root).  No case is an input the engine may decline: each one has
an answer."""
import os

import numpy as np
import pytest
import torch

import amt_enum_cases as ae
import event_chain_cases as ec
import ipc_filecoin_proofs_amd as ipcfp
import pyamt
import pyevents
from test_amt_enum_cases import claim_mismatch, generate_literal, n_present, order_mismatch, scan_mismatch

pytestmark = pytest.mark.gpu

NAMES = list(ae.CASES)
ONE_CALL = ("sizes", "stage", "shared", "two")


@pytest.fixture()
def routed(engine):
    def use(fast):
        engine.set_tuning("fast_verify", fast)
    yield use
    engine.set_tuning("fast_verify", -1)


def dev(a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.zeros(64, np.uint8)])).cuda()


def triples(m):
    return list(zip(m["exec_index"].tolist(), m["event_index"].tolist(), m["emitter"].tolist()))


def cid_set(cids40, ids):
    return {bytes(cids40[i, :38]) if cids40[i, 36:38].any() else bytes(cids40[i, :36]) for i in ids}


def oracle_cid_set(rows):
    return {bytes(r[:38]) if r[36:38].any() else bytes(r[:36]) for r in rows}


@pytest.mark.parametrize("name", NAMES)
def test_case(engine, oracle, routed, name):
    c, b = ae.CASES[name], ae.build(name)
    tabs = b.store.tables()
    cids40 = tabs[3]
    root, parents, child = b.parts["receipts"], b.parts["parents"], b.parts["child"]
    whole = c.rng is None
    ost = oracle.store(*tabs)
    wrong = []
    try:
        with engine.witness(*tabs) as w:
            if not whole:
                w.set_receipt_range(*c.rng)
            # ---- the scan
            st, has, m, ids = w.scan_events(root, *ae.FILTER)
            wrong += scan_mismatch(c, st, has, triples(m), "scan")
            # … and once more: the answer of the enumeration the first scan left on the witness (amt_enumerate_cached), without
            # another walk — `exec_order` is the profile group of amt_enumerate, whatever tree it walks
            engine.profile_enable(True, only="exec_order")
            try:
                engine.profile_reset()
                again = w.scan_events(root, *ae.FILTER)
                walks = engine.profile_read("exec_order")[0]
            finally:
                engine.profile_enable(False)
            if (again[0], again[1].tobytes(), again[2].tobytes()) != (st, has.tobytes(), m.tobytes()) or walks != 0:
                wrong.append((name, "scan", "the second scan differs, or walked again", walks))
            if st == 1 == c.scan[0]:
                if whole or (c.rng[0] == 0 and c.rng[1] >= c.meta["n"]):
                    want = oracle_cid_set(ost.scan_events(root, *ae.FILTER, cap_receipts=1 << 22, cap_matches=1 << 17, cap_touched=1 << 17)[3])
                elif n_present(c) <= 10_000:
                    want = pyevents.scan(b.store.blocks, root, *ae.FILTER, lo=c.rng[0], hi=c.rng[1])[3]
                else:  # (range_65537_across_the_middle: 21 847 receipts — pyevents would take seconds, the oracle has no range)
                    want = None
                if want is not None and cid_set(cids40, ids) != want:
                    wrong.append((name, "scan", "touched set", len(ids), len(want)))
            # ---- the execution order
            st, cids = w.exec_order(parents)
            wrong += order_mismatch(c, st, cids, "exec_order")
            if st == 1 == c.order[0]:
                ost_, ocids = ost.exec_order(parents, cap=1 << 17)
                if ost_ != 1 or not np.array_equal(cids, ocids):
                    wrong.append((name, "exec_order", "bytes differ from the oracle's"))
            # ---- the verifier: packed on first contact (the table route), packed general, strings
            if b.claims:
                pr = ec.proofs([cl for _t, cl, _s in b.claims])
                ts, cl, blob = ipcfp.pack_event_proofs(pr.arr, pr.n)
                engine.profile_enable(True, only="amt_walk")
                try:
                    for fast, tag in ((1, "packed_fast"), (0, "packed_general")):
                        routed(fast)
                        w.rebuild_index()
                        if not whole:
                            w.set_receipt_range(*c.rng)
                        engine.profile_reset()
                        wrong += claim_mismatch(c, b, w.verify_event_claims(ts, cl, blob, len(blob)), tag)
                        walks = engine.profile_read("amt_walk")[0]
                        if c.walks is not None and walks != (c.walks if fast else 0):
                            wrong.append((name, tag, "amt_walk launches", walks, c.walks if fast else 0))
                finally:
                    engine.profile_enable(False)
                routed(-1)
                w.rebuild_index()
                if not whole:
                    w.set_receipt_range(*c.rng)
                wrong += claim_mismatch(c, b, w.verify_event_proofs(pr.arr, pr.n), "strings")
                if c.family in ONE_CALL and whole:
                    cap = (c.scan[1] if c.scan[0] == 1 else c.meta["n"]) + 16
                    d_cl, d_blob = dev(cl), dev(blob)
                    d_st = torch.full((pr.n + 64,), 77, dtype=torch.uint8, device="cuda")
                    d_has = torch.full((cap,), 9, dtype=torch.uint8, device="cuda")
                    d_m = torch.zeros(cap * ipcfp.MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
                    for tag in ("one_call", "one_call_cached"):
                        if tag == "one_call":
                            w.rebuild_index()
                        d_st.fill_(77)
                        sst, snr, snm = w.verify_and_scan_device(ts, d_cl.data_ptr(), pr.n, d_blob.data_ptr(), len(blob), d_st.data_ptr(), *ae.FILTER, None,
                                                                 d_has.data_ptr(), cap, d_m.data_ptr(), cap)
                        engine.sync()
                        wrong += claim_mismatch(c, b, d_st.cpu().numpy()[: pr.n], tag)
                        mm = d_m.cpu().numpy()[: snm * ipcfp.MATCH_DTYPE.itemsize].view(ipcfp.MATCH_DTYPE) if sst == 1 else None
                        wrong += scan_mismatch(c, sst, d_has.cpu().numpy()[:snr] if sst == 1 else None, triples(mm) if sst == 1 else None, tag)
            # ---- the generator and the shard planner
            if whole and not c.meta.get("shard_witness"):
                w.rebuild_index()
                gst, gm, gmsg, gids = w.generate_event_proofs(parents, child, *ae.FILTER)
                if gst != generate_literal(c):
                    wrong.append((name, "generate", "status", gst, generate_literal(c)))
                elif gst == 1:
                    ogst, otrip, omsg, owit = ost.generate_event_proof(parents, child, *ae.FILTER, cap_proofs=1 << 17, cap_witness=1 << 17)
                    if ogst != 1 or triples(gm) != [tuple(int(x) for x in t) for t in otrip] or not np.array_equal(gmsg, omsg):
                        wrong.append((name, "generate", "proofs differ from the oracle's"))
                    if [bytes(r) for r in cids40[gids]] != [bytes(r) for r in owit]:
                        wrong.append((name, "generate", "witness ids differ from the oracle's", len(gids), len(owit)))
                w.rebuild_index()
                # the planner enumerates the message lists (the execution order is every shard's); of the receipts tree it
                # LOADS the root and cuts [0, the root's `count`) — whatever the tree holds (csrc/host/shard.cpp)
                pst, lo, hi, nr, pids = w.shard_plan_tipset(parents, child, 3, 1)
                try:
                    want_st, want_nr = 1, pyevents.amt_load(b.store.blocks, root, 0, pyevents.check_receipt).count
                except pyevents.Err as e:
                    want_st, want_nr = e.status, 0
                if c.order[0] != 1:
                    want_st = c.order[0]
                if pst != want_st or (pst == 1 and (nr, lo, hi) != (want_nr, want_nr // 3, 2 * want_nr // 3)):
                    wrong.append((name, "shard_plan_tipset", pst, want_st, nr, lo, hi))
        # ---- the scan once more, every receipt and claim walking its blocks (no event table)
        os.environ["IPCFP_EVENT_TABLE"] = "0"
        try:
            with engine.witness(*tabs) as w:
                if not whole:
                    w.set_receipt_range(*c.rng)
                st, has, m, _ = w.scan_events(root, *ae.FILTER, want_touched=False)
                wrong += scan_mismatch(c, st, has, triples(m), "scan without the event table")
        finally:
            os.environ.pop("IPCFP_EVENT_TABLE", None)
    finally:
        ost.close()
    assert not wrong, wrong[:12]


# ---- merged: many trees in one witness; the cache of enumerations -----------------------------------------------------------------
def merged(names):
    store = pyamt.Store()
    built = {}
    for n in names:
        built[n] = ae.build(n)
        for cid, block in built[n].store.blocks.items():
            assert store.blocks.setdefault(cid, block) == block
    return store, built


@pytest.mark.parametrize("size_class", ["up_to_600", "8200", "65537"])
def test_merged_witness_and_the_cache_of_enumerations(engine, size_class):
    """All receipt trees of one size class in ONE witness (a case's nodes among the others', most of them shared between the
    trees): every tree scanned in turn, then every tree once more — the second answer comes from the enumeration the first
    left on the witness, and it is the same; no tree is answered with another's."""
    pick = {"up_to_600": lambda c: c.meta.get("n", 10 ** 9) <= 600 and c.family in ("sizes", "heights", "count", "stage"),
            "8200": lambda c: c.family == "links" and c.meta.get("n") == ae.LN,
            "65537": lambda c: c.meta.get("n") == ae.BIG and c.family in ("sizes", "shared", "two")}[size_class]
    names = [n for n, c in ae.CASES.items() if pick(c) and c.rng is None and not c.drop]
    assert len(names) >= {"up_to_600": 100, "8200": 20, "65537": 5}[size_class], len(names)
    store, built = merged(names)
    roots = {built[n].parts["receipts"] for n in names}
    assert len(roots) > len(names) // 2  # (the cases that differ in their message lists alone share a receipts tree)
    wrong = []
    with engine.witness(*store.tables()) as w:
        first, walked = {}, set()
        engine.profile_enable(True, only="exec_order")
        try:
            for turn in (0, 1):
                for n in names if turn == 0 else reversed(names):
                    c, root = ae.CASES[n], built[n].parts["receipts"]
                    engine.profile_reset()
                    st, has, m, _ = w.scan_events(root, *ae.FILTER, want_touched=False)
                    walks = engine.profile_read("exec_order")[0]  # (amt_enumerate's profile group: one per enumeration made)
                    wrong += scan_mismatch(c, st, has, triples(m), f"merged, turn {turn}")
                    got = (st, has.tobytes(), m.tobytes())
                    if turn == 1 and got != first[n]:
                        wrong.append((n, "the cached enumeration answers differently"))
                    # a root's first scan enumerates it; every later one is answered from the cache
                    if (walks != 0) != (root not in walked):
                        wrong.append((n, f"turn {turn}", "enumerations made", walks, "a first scan" if root not in walked else "a later scan"))
                    walked.add(root)
                    first.setdefault(n, got)
        finally:
            engine.profile_enable(False)
    assert not wrong, wrong[:12]


def test_cached_enumeration_is_keyed_by_the_range(engine):
    """one witness, one root, one range after another and back: an enumeration made under one range never answers for another"""
    name = "size_4097"
    c, b = ae.CASES[name], ae.build(name)
    rngs = [ae.CASES[n].rng for n in NAMES if n.startswith("range_4097_from_")] + [(0, 4097), (ae.RLO, ae.RHI)]
    with engine.witness(*b.store.tables()) as w:
        for lo, hi in rngs + rngs[::-1]:
            w.set_receipt_range(lo, hi)  # (drops the witness's cached enumerations: include/ipcfp.h)
            for again in (0, 1):
                engine.profile_enable(True, only="exec_order")
                try:
                    engine.profile_reset()
                    st, has, m, _ids = w.scan_events(b.parts["receipts"], *ae.FILTER, want_touched=False)
                    walks = engine.profile_read("exec_order")[0]
                finally:
                    engine.profile_enable(False)
                n = max(0, min(hi, 4097) - lo)
                assert st == 1 and has.tolist() == [1] * n and triples(m) == [(i, 0, ae.EMITTER) for i in range(lo, lo + n)], (lo, hi)
                assert (walks == 0) == bool(again), (lo, hi, again, walks)
