"""GPU: ipcfp_scan_events_multi* — one scan of the resident tipset for a SET of event specs — through the C ABI, on every
(tipset, set) of tests/scan_multi_cases.py.

For each: the records split by match_spec equal the J expected single-filter lists exactly, spec_counts their lengths, the
map the OR of the expected maps, touched_bits the union of the expected recorded blocks, the combined order the contract
(scan_multi_cases.merge), the status what each single call gives.  Routes: the event table on and off, first contact and
the cached table, with and without touched_bits, the host and the device form, caps of 0, 1, total - 1 and total, receipt
ranges on `tiles`.  Then the argument errors, a synthetic tipset with all 1024 pairs, a context whose single-filter calls
must not notice the multi calls between them, and ipcfp_generate_proof_bundle over the scan.
Expected values: tests/test_scan_multi.py holds them to pyevents.scan per spec and to the oracle on the CPU."""
import contextlib
import os

import numpy as np
import pytest
import torch

import event_chain_cases as ec
import ipc_filecoin_proofs_amd as ipcfp
import pyevents
import scan_multi_cases as mc

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def witness_of(engine, store, table=True):
    """a witness made with the event table on or off (IPCFP_EVENT_TABLE is read when the witness is made)"""
    old = os.environ.get("IPCFP_EVENT_TABLE")
    os.environ["IPCFP_EVENT_TABLE"] = "1" if table else "0"
    try:
        with engine.witness(*store.tables()) as w:
            yield w
    finally:
        if old is None:
            os.environ.pop("IPCFP_EVENT_TABLE", None)
        else:
            os.environ["IPCFP_EVENT_TABLE"] = old


def rows(m, ms=None):
    t = zip(m["exec_index"].tolist(), m["event_index"].tolist(), m["emitter"].tolist())
    return list(t) if ms is None else [(*r, s) for r, s in zip(t, ms.tolist())]


def id_of(store):
    return {c: i for i, c in enumerate(store.blocks)}


def held(w, store, root, specs, want, tag, touched=True):
    """one host-form call against the expected answer `want` = scan_multi_cases.expected(…)"""
    st, per_want, has_want, rec_want = want
    got = w.scan_events_multi(root, specs, want_touched=touched)
    assert got[0] == st, (tag, got[0], st)
    if st != pyevents.TRUE:
        return None
    _st, has, m, ms, counts, ids, per = got
    assert [rows(p) for p in per] == per_want, tag
    assert counts.tolist() == [len(p) for p in per_want], tag
    assert has.tolist() == has_want, tag
    assert rows(m, ms) == mc.merge(per_want), tag
    if touched:
        ids_of = id_of(store)
        assert set(ids.tolist()) == {ids_of[c] for c in rec_want}, tag
    return m, ms, counts


def device_form(w, root, specs, want, tag, cap=None):
    st, per_want, has_want, _rec = want
    total = sum(len(p) for p in per_want) if st == pyevents.TRUE else 0
    cap = total if cap is None else cap
    n_has = len(has_want) if st == pyevents.TRUE else 64
    d_has = torch.full((n_has + 64,), 9, dtype=torch.uint8, device="cuda")
    d_m = torch.zeros((cap + 1) * ipcfp.MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_ms = torch.full((cap + 1,), 0x7fffffff, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((len(specs) + 1,), -1, dtype=torch.int64, device="cuda")
    d_sum = torch.zeros(2, dtype=torch.int64, device="cuda")
    gs, nr, nm = w.scan_events_multi_device(root, specs, d_has.data_ptr(), n_has, d_m.data_ptr(), d_ms.data_ptr(), cap, d_cnt.data_ptr(),
                                            d_sum.data_ptr())
    w.eng.sync()
    assert gs == st, (tag, gs, st)
    summary = d_sum.cpu().numpy()
    assert int(summary[0]) & 0xff == st, tag
    if st != pyevents.TRUE:
        assert (int(summary[0]) >> 8) == w.last_scan_phase() != 0 and int(summary[1]) == 0, tag
        assert d_has.cpu().numpy().tolist() == [9] * (n_has + 64) and d_cnt.cpu().numpy().tolist() == [-1] * (len(specs) + 1), tag  # nothing written
        return
    assert (nr, nm, int(summary[1])) == (len(has_want), total, total), tag
    assert d_has.cpu().numpy()[:nr].tolist() == has_want and d_has.cpu().numpy()[nr:].tolist() == [9] * 64, tag
    take = min(cap, total)
    m = d_m.cpu().numpy()[: take * ipcfp.MATCH_DTYPE.itemsize].view(ipcfp.MATCH_DTYPE)
    ms = d_ms.cpu().numpy()
    assert rows(m, ms[:take]) == mc.merge(per_want)[:take] and int(ms[cap]) == 0x7fffffff, tag
    cnt = d_cnt.cpu().numpy()
    assert cnt[:-1].tolist() == [len(p) for p in per_want] and int(cnt[-1]) == -1, tag


def caps(w, root, specs, want, tag):
    """caps of 0, 1, total - 1 and total: the truncated prefix and the full counts"""
    _st, per_want, has_want, _rec = want
    full = mc.merge(per_want)
    total = len(full)
    for cap in sorted({0, 1, max(total - 1, 0), total}):
        _s, has, m, ms, counts, _ids, _per = w.scan_events_multi(root, specs, want_touched=False, cap_matches=cap)
        assert rows(m, ms) == full[: min(cap, total)], (tag, cap)
        assert counts.tolist() == [len(p) for p in per_want] and has.tolist() == has_want, (tag, cap)
        device_form(w, root, specs, want, (tag, "device cap", cap), cap=cap)


def every_route(engine, store, root, specs, name, lo=0, hi=None, with_caps=True):
    want = mc.expected(store.blocks, root, specs, lo, hi)
    single_status = pyevents.scan(store.blocks, root, specs[0][0], specs[0][1], specs[0][2], lo, hi)[0]
    assert want[0] == single_status
    for table in (True, False):
        with witness_of(engine, store, table) as whole:
            w = whole if (lo, hi) == (0, None) else whole.subset(np.arange(whole.n), lo, hi)
            try:
                tag = (name, "table" if table else "walk")
                held(w, store, root, specs, want, (*tag, "first contact"))           # builds the enumeration (and the table)
                held(w, store, root, specs, want, (*tag, "cached"))
                held(w, store, root, specs, want, (*tag, "no recorder"), touched=False)
                device_form(w, root, specs, want, (*tag, "device"))
                # the status equals a single call's, and the single call after the multi calls answers as ever
                t0, t1, actor = specs[-1]
                gs, ghas, gm, _ids = w.scan_events(root, t0, t1, actor=actor)
                assert gs == want[0], tag
                if gs == pyevents.TRUE:
                    assert rows(gm) == want[1][-1], tag
                    if with_caps:  # (table: the fused tail clips; walk: k_fill_multi_walk does)
                        caps(w, root, specs, want, tag)
                else:
                    phase = w.last_scan_phase()
                    w.scan_events_multi(root, specs)
                    assert w.last_scan_phase() == phase != 0, tag
            finally:
                if w is not whole:
                    w.close()


SETS = None


def sets_over_edges():
    global SETS
    if SETS is None:
        SETS = mc.spec_sets_over_edges(mc.recorded_slot_of)  # (home slots as recorded: no compiler, no harness here)
    return SETS


EDGE_SETS = ["every_present_pair", "traps", "repeated_three_times", "emitter_filters", "size_1", "size_2", "size_63", "size_64", "size_65", "size_1024",
             "shuffled_0", "shuffled_1", "one_home_slot"]


@pytest.mark.parametrize("name", EDGE_SETS)
def test_edges(engine, name):
    st, parts, _ = mc.edges()
    specs = sets_over_edges()[name]
    assert set(sets_over_edges()) == set(EDGE_SETS)
    every_route(engine, st, parts["receipts"], specs, f"edges/{name}", with_caps=name in ("traps", "emitter_filters", "size_65", "shuffled_0"))


def test_the_two_shuffles_give_one_answer_per_spec(engine):
    st, parts, _ = mc.edges()
    a, b = sets_over_edges()["shuffled_0"], sets_over_edges()["shuffled_1"]
    with witness_of(engine, st) as w:
        ga, gb = w.scan_events_multi(parts["receipts"], a), w.scan_events_multi(parts["receipts"], b)
    by_a = {repr(sp): rows(p) for sp, p in zip(a, ga[6])}
    by_b = {repr(sp): rows(p) for sp, p in zip(b, gb[6])}
    assert by_a == by_b and ga[1].tolist() == gb[1].tolist() and ga[5].tolist() == gb[5].tolist()


@pytest.mark.parametrize("n", mc.TILE_SIZES)
def test_tiles(engine, n):
    st, roots = mc.tiles()
    every_route(engine, st, roots[n], mc.TILE_SPECS, f"tiles/{n}", with_caps=n == 2049)


@pytest.mark.parametrize("lo,hi", mc.TILE_RANGES)
def test_tiles_under_a_receipt_range(engine, lo, hi):
    st, roots = mc.tiles()
    every_route(engine, st, roots[2049], mc.TILE_SPECS, f"tiles/2049[{lo},{hi})", lo, hi)


def test_short_order_scans_clean(engine):
    st, parts = mc.short_order()
    every_route(engine, st, parts["receipts"], [(*mc.SHORT_X, None)] + [(a, b, None) for a, b in mc.SHORT_OTHERS], "short_order")


def test_err_tipsets_have_the_single_calls_status_and_phase(engine):
    seen = set()
    for name, st, parts in mc.err_tipsets():
        specs = [(*ec.FILTER, None), (*mc.pair(0), 7), (*ec.OTHER_FILTER, None)]
        every_route(engine, st, parts["receipts"], specs, f"err/{name}")
        for table in (True, False):
            with witness_of(engine, st, table) as w:
                gs, *_ = w.scan_events(parts["receipts"], *ec.FILTER)
                phase = w.last_scan_phase()
            with witness_of(engine, st, table) as w:
                gm = w.scan_events_multi(parts["receipts"], specs)
                assert (gm[0], w.last_scan_phase()) == (gs, phase) and gs != pyevents.TRUE and phase != 0, (name, table)
                assert gm[1:] == (None,) * 6
            seen.add((gs, phase))
    assert len(seen) >= 2


def launches(engine, call):
    """(launches of the one-launch tail, launch groups of the separate PASS 2) that `call` makes"""
    engine.profile_enable(True)
    try:
        engine.profile_reset()
        call()
        return engine.profile_read("scan_multi_tail")[0], engine.profile_read("scan_multi_fill")[0]
    finally:
        engine.profile_enable(False)


def test_which_route_serves_which_call(engine):
    """the rule of the single-filter scan: the tail in one launch when the table is there, no recorder is asked for and the
    capacity is at most 2^26 — and then the separate PASS 2 only for receipts the table leaves to the walk (`tiles` has
    none); a recorder or a witness without a table takes the prefix sum and the separate PASS 2.  The binding makes TWO
    ABI calls per scan: a sizing call, which never has a recorder, then the call that takes the outputs."""
    tst, roots = mc.tiles()
    est, eparts, _ = mc.edges()
    specs = sets_over_edges()["every_present_pair"]
    with witness_of(engine, tst) as w:
        w.scan_events_multi(roots[2049], mc.TILE_SPECS, want_touched=False)  # (the enumeration and the table)
        assert launches(engine, lambda: w.scan_events_multi(roots[2049], mc.TILE_SPECS, want_touched=False)) == (2, 0)
        assert launches(engine, lambda: w.scan_events_multi(roots[2049], mc.TILE_SPECS, want_touched=False, cap_matches=0)) == (2, 0)
        assert launches(engine, lambda: w.scan_events_multi(roots[2049], mc.TILE_SPECS, want_touched=True)) == (1, 1)
        assert launches(engine, lambda: w.scan_events_multi_device(roots[2049], mc.TILE_SPECS)) == (1, 0)
    with witness_of(engine, est) as w:
        tail, fill = launches(engine, lambda: w.scan_events_multi(eparts["receipts"], specs, want_touched=False))
        assert tail == 2 and fill <= 2
    with witness_of(engine, tst, table=False) as w:
        assert launches(engine, lambda: w.scan_events_multi(roots[2049], mc.TILE_SPECS, want_touched=False)) == (0, 2)


def test_spec_counts_of_0_and_1025(engine):
    st, parts, _ = mc.edges()
    with witness_of(engine, st) as w:
        with pytest.raises(ipcfp.EngineError, match=r"\(-1\)"):
            w.scan_events_multi(parts["receipts"], [])
        with pytest.raises(ipcfp.EngineError, match=r"\(-5\)"):
            w.scan_events_multi(parts["receipts"], mc.padded([], 1024) + [(*mc.pair(0), None)])
        with pytest.raises(ipcfp.EngineError, match=r"\(-1\)"):
            w.scan_events_multi_device(parts["receipts"], [])
        with pytest.raises(ipcfp.EngineError, match=r"\(-5\)"):
            w.scan_events_multi_device(parts["receipts"], mc.padded([], 1024) + [(*mc.pair(0), None)])
        assert ipcfp.MAX_SCAN_SPECS == mc.MAX_SPECS == 1024
        assert w.scan_events_multi(parts["receipts"], mc.padded([(*mc.pair(0), None)], 1024))[4][0] == 4


def test_a_synthetic_tipset_with_all_1024_pairs(engine, oracle):
    from tools.synth import Tipset

    tip = Tipset(n_receipts=3000, n_sigs=16, n_subnets=64, variety=1)
    blocks = {bytes(tip.cids[i, :38]): tip.block(i) for i in range(tip.n_blocks)}
    st0, _n, listing, _ = mc._listing(blocks, tip.receipts_root, 0, None)
    assert st0 == pyevents.TRUE
    pairs = list(dict.fromkeys((t0, t1) for _i, _j, _em, t0, t1 in listing))
    assert 512 < len(pairs) <= 1024
    specs = mc.padded([(a, b, None) for a, b in pairs], 1024)
    want = mc.expected(blocks, tip.receipts_root, specs, want_rec=False)
    # the tipset's own claim table (one claim per receipt that has events) names events of the lists
    for e, j, em, nt, tp in zip(tip.claim_exec.tolist(), tip.claim_event.tolist(), tip.claim_emitter.tolist(), tip.claim_ntopics.tolist(), tip.claim_topics):
        if nt >= 2:
            assert (e, j, em) in want[1][pairs.index((bytes(tp[0]), bytes(tp[1])))]
    with engine.witness(tip.data, tip.off, tip.lens, tip.cids) as w:
        for tag in ("first contact", "cached"):
            gs, has, m, ms, counts, _ids, per = w.scan_events_multi(tip.receipts_root, specs, want_touched=False)
            assert gs == pyevents.TRUE and [rows(p) for p in per] == want[1] and has.tolist() == want[2], tag
            assert rows(m, ms) == mc.merge(want[1]) and int(counts.sum()) == len(listing) == len(m), tag
        device_form(w, tip.receipts_root, specs, want, "synthetic device")
        gm = w.scan_events_multi(tip.receipts_root, specs, want_touched=False)
    ost = oracle.store(tip.data, tip.off, tip.lens, tip.cids)
    for k in np.random.default_rng(5).choice(len(pairs), 32, replace=False).tolist() + [1023]:
        a, b, _ = specs[k]
        os_, _ohas, otrip, _ = ost.scan_events(tip.receipts_root, a, b, cap_receipts=4096, cap_matches=4096, cap_touched=1 << 14)
        assert os_ == 1 and [tuple(int(x) for x in r) for r in otrip] == rows(gm[6][k]), k
    ost.close()


def test_single_filter_neighbours_do_not_notice_the_multi_calls(engine):
    """single scan A → multi → verify_event_proofs under a filter → single scan B → multi → single scan A, against a context
    that never saw a multi call"""
    st, parts, _ = mc.edges()
    root = parts["receipts"]
    A, B = (*mc.pair(0), None), (*ec.FILTER, 1001)
    specs = sets_over_edges()["emitter_filters"] + sets_over_edges()["traps"]
    want = mc.expected(st.blocks, root, specs)
    claims = mc.own_claims()
    filt = mc.pair(0)
    verdicts = [pyevents.verify(st.blocks, c, None, filt) for c in claims]
    assert verdicts[0] == 1 and set(verdicts[1:]) == {17}
    pr = ec.proofs(claims)

    def single(w, sp):
        gs, has, m, ids = w.scan_events(root, sp[0], sp[1], actor=sp[2])
        return gs, has.tobytes(), m.tobytes(), ids.tobytes()

    with ipcfp.Engine(0) as fresh:
        with fresh.witness(*st.tables()) as w:
            plain = [single(w, A), w.verify_event_proofs(pr.arr, pr.n, filt=ec.event_filter(filt)).tolist(), single(w, B), single(w, A)]
    for table in (True, False):
        with witness_of(engine, st, table) as w:
            got = [single(w, A)]
            held(w, st, root, specs, want, ("neighbours", table, 1))
            got.append(w.verify_event_proofs(pr.arr, pr.n, filt=ec.event_filter(filt)).tolist())
            got.append(single(w, B))
            held(w, st, root, specs, want, ("neighbours", table, 2))
            got.append(single(w, A))
        assert got == plain and got[1] == verdicts, table
    for sp, g in ((A, plain[0]), (B, plain[2])):
        ws = pyevents.scan(st.blocks, root, *sp)
        assert g[0] == 1 and np.frombuffer(g[1], np.uint8).tolist() == ws[1] and rows(np.frombuffer(g[2], ipcfp.MATCH_DTYPE)) == ws[2]


# ---- ipcfp_generate_proof_bundle over the scan ---------------------------------------------------------------------------------------
def bundle_expected(blocks, parts, named):
    """J × pyevents.generate in the reference's order → (first_error | None, event_status up to it, proofs spec-major,
    match_spec, witness CIDs in `Cid: Ord` order)"""
    status, proofs, spec_of, union = [], [], [], set()
    for j, (q, actor) in enumerate(named):
        gs, rows_, wit = pyevents.generate(blocks, parts["parents"], parts["child"], *mc.named_pair(q), actor)
        status.append(gs)
        if gs != pyevents.TRUE:
            return j, status, [], [], []
        proofs += rows_
        spec_of += [j] * len(rows_)
        union |= wit
    return None, status, proofs, spec_of, sorted(union)  # (chain CIDs of one type: `Cid: Ord` is byte order)


def bundle_rows(out):
    m = out["matches"]
    return [(int(a), int(b), int(c), bytes(x[:38])) for a, b, c, x in zip(m["exec_index"], m["event_index"], m["emitter"], out["message_cids"])]


@pytest.mark.parametrize("case", range(7))
def test_bundle_in_one_pass(engine, case):
    name, st, parts, named = mc.bundle_cases()[case]
    first_error, status, proofs, spec_of, wit = bundle_expected(st.blocks, parts, named)
    assert (first_error is not None) == name.startswith("short_order/x_f"), name
    specs = [(*mc.named(q), actor) for q, actor in named]
    cids = list(st.blocks)
    for table in (True, False):
        with witness_of(engine, st, table) as w:
            assert engine.create_event_filter(*mc.named(named[0][0])) == mc.named_pair(named[0][0])
            for tag in ("first contact", "cached"):
                out = w.generate_proof_bundle(parts["parents"], parts["child"], [], specs)
                assert out["first_error"] == first_error, (name, table, tag)
                n = len(status)
                assert out["event_status"][:n].tolist() == status and not out["event_status"][n:].any(), (name, table, tag)
                assert bundle_rows(out) == proofs and out["match_spec"].tolist() == spec_of, (name, table, tag)
                assert [cids[i] for i in out["block_ids"]] == wit, (name, table, tag)
            if first_error is None:  # the same outputs from J calls of ipcfp_generate_event_proofs, merged here
                merged, merged_spec, ids = [], [], set()
                for j, (q, actor) in enumerate(named):
                    gs, gm, gmsg, gids = w.generate_event_proofs(parts["parents"], parts["child"], *mc.named_pair(q), actor=actor)
                    assert gs == 1
                    merged += [(int(a), int(b), int(c), bytes(x[:38])) for a, b, c, x in zip(gm["exec_index"], gm["event_index"], gm["emitter"], gmsg)]
                    merged_spec += [j] * len(gm)
                    ids |= set(gids.tolist())
                assert bundle_rows(out) == merged and out["match_spec"].tolist() == merged_spec
                assert sorted(cids[i] for i in ids) == [cids[i] for i in out["block_ids"]]
    if first_error is None and name.startswith("edges"):
        assert len(proofs) >= len({q for q, a in named if a is None and q < mc.N_NAMED})


def test_bundle_on_an_err_tipset_fails_its_first_event_spec(engine):
    for name, st, parts in mc.err_tipsets():
        want = pyevents.generate(st.blocks, parts["parents"], parts["child"], *mc.named_pair(0))[0]
        assert want != pyevents.TRUE
        with witness_of(engine, st) as w:
            out = w.generate_proof_bundle(parts["parents"], parts["child"], [], [(*mc.named(0), None), (*mc.named(1), 7), (*mc.named(0), None)])
        assert out["first_error"] == 0 and out["event_status"].tolist() == [want, 0, 0], name
        assert len(out["matches"]) == 0 and len(out["block_ids"]) == 0, name


def test_bundle_with_storage_specs_on_a_synthetic_tipset(engine, oracle):
    from tools.synth import Tipset

    tip = Tipset(n_receipts=400, n_parents=2, n_planted=6, variety=1, max_events=4, n_actors=1200, n_contracts=4, slots_per_contract=8,
                 storage_layout_mix=1, n_actor_queries=6)
    sig, subnet = "NewTopDownMessage(bytes32,uint256)", "calib-subnet-1"
    especs = [(sig, subnet, tip.filter_actor), (sig, subnet, None), (sig, "no-such-subnet", None), (sig, subnet, None), ("Other(uint256)", subnet, None)]
    sspecs = [(int(tip.sc_actor[k]), tip.sc_slot[k].tobytes()) for k in (0, 3, 7)]
    with engine.witness(tip.data, tip.off, tip.lens, tip.cids) as w:
        filters = [engine.create_event_filter(s, t) for s, t, _a in especs]
        assert filters[0] == (tip.topic0, tip.topic1)
        out = w.generate_proof_bundle(tip.parent_cids, tip.child_cid, sspecs, especs)
        bad = w.generate_proof_bundle(tip.parent_cids, tip.child_cid, sspecs[:1] + [(10 ** 9, bytes(32))], especs)
    assert out["first_error"] is None and (out["storage"]["status"] == 1).all() and out["event_status"].tolist() == [1] * 5
    assert bad["first_error"] == 1 and len(bad["matches"]) == 0 and len(bad["block_ids"]) == 0 and not bad["event_status"].any()
    ost = oracle.store(tip.data, tip.off, tip.lens, tip.cids)
    union, rows_, spec_of = set(), [], []
    for a, slot in sspecs:
        s, _o3, _val, wit = ost.generate_storage_proof(tip.child_cid, a, slot)
        assert s == 1
        union |= {bytes(c) for c in wit}
    for j, ((t0, t1), (_s, _t, actor)) in enumerate(zip(filters, especs)):
        s, trip, msg, wit = ost.generate_event_proof(tip.parent_cids, tip.child_cid, t0, t1, actor=actor)
        assert s == 1
        rows_ += [(int(t[0]), int(t[1]), int(t[2]), bytes(m[:38])) for t, m in zip(trip, msg)]
        spec_of += [j] * len(trip)
        union |= {bytes(c) for c in wit}
    ost.close()
    assert bundle_rows(out) == rows_ and out["match_spec"].tolist() == spec_of and len(rows_) > 10 and spec_of.count(2) == spec_of.count(4) == 0
    assert [bytes(tip.cids[i]) for i in out["block_ids"]] == sorted(union)
