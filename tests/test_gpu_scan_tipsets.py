"""GPU: ipcfp_scan_events_tipsets* — one scan of a CHAIN of tipsets for a set of event specs — through the C ABI, on every
chain of tests/scan_tipsets_cases.py.

For each chain, on a witness made with the event table on and off: the host form with and without touched_bits and the
device form give the per-tipset statuses and phases, the two offset arrays, the concatenated map, records + match_spec,
spec_counts, the recorded blocks and the totals of the case module (tests/test_scan_tipsets.py holds those to the oracle
on the CPU).  A second judge: T calls of scan_events_multi on the same witness, concatenated.  Then the capacities, the
state around the call, the counts of enumerations and launch groups, and the refusals.  Every input here is one a hostile bundle may contain; nothing
tries to provoke a device fault."""
import contextlib
import os

import numpy as np
import pytest
import torch

import ipc_filecoin_proofs_amd as ipcfp
import pyevents
import scan_multi_cases as mc
import scan_tipsets_cases as tc

pytestmark = pytest.mark.gpu

GUARD = 64


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


@pytest.fixture(scope="module", params=[True, False], ids=["table", "walk"])
def wit(engine, request):
    store, _roots = tc.world()
    with witness_of(engine, store, request.param) as w:
        yield w


def roots_of(tipsets):
    _store, roots = tc.world()
    return [roots[t] for t in tipsets]


def ids_want(rec):
    store, _ = tc.world()
    ids_of = {c: i for i, c in enumerate(store.blocks)}
    return {ids_of[c] for c in rec}


def held_host(w, name, touched=True, tag=""):
    tipsets, key = tc.chains()[name]
    e = tc.expected_chain(name)
    g = w.scan_events_tipsets(roots_of(tipsets), tc.SPEC_SETS[key], want_touched=touched)
    tag = (name, tag, "touched" if touched else "no recorder")
    assert g["status"].tolist() == e["status"] and g["phase"].tolist() == e["phase"], tag
    assert g["receipt_off"].tolist() == e["receipt_off"] and g["match_off"].tolist() == e["match_off"], tag
    assert (g["n_receipts"], g["n_matches"]) == (e["receipt_off"][-1], e["match_off"][-1]), tag
    assert g["has_match"].tolist() == e["has"], tag
    assert rows(g["matches"], g["match_spec"]) == e["rows"], tag
    assert g["spec_counts"].tolist() == e["spec_counts"], tag
    assert [m.tolist() for m in g["maps"]] == e["maps"], tag
    assert [rows(m, s) for m, s in zip(g["records"], g["record_specs"])] == e["records"], tag
    assert w.last_scan_phase() == e["last_phase"], tag
    if touched:
        assert set(g["touched"].tolist()) == ids_want(e["rec"]), tag
    return g


def device_form(w, name, cap_r=None, cap_m=None, tag=""):
    tipsets, key = tc.chains()[name]
    specs = tc.SPEC_SETS[key]
    e = tc.expected_chain(name)
    T, total_r, total_m = len(tipsets), e["receipt_off"][-1], e["match_off"][-1]
    cap_r = total_r if cap_r is None else cap_r
    cap_m = total_m if cap_m is None else cap_m
    item = ipcfp.MATCH_DTYPE.itemsize
    d_has = torch.full((cap_r + GUARD,), 9, dtype=torch.uint8, device="cuda")
    d_m = torch.full(((cap_m + 1) * item,), 0xAB, dtype=torch.uint8, device="cuda")
    d_ms = torch.full((cap_m + 1,), 0x7fffffff, dtype=torch.int32, device="cuda")
    d_cnt = torch.full((len(specs) + 1,), -1, dtype=torch.int64, device="cuda")
    d_roff = torch.full((T + 2,), -1, dtype=torch.int64, device="cuda")
    d_moff = torch.full((T + 2,), -1, dtype=torch.int64, device="cuda")
    st, ph, roff, moff, nr, nm = w.scan_events_tipsets_device(roots_of(tipsets), specs, d_has.data_ptr(), cap_r, d_m.data_ptr(), d_ms.data_ptr(), cap_m,
                                                              d_cnt.data_ptr(), d_roff.data_ptr(), d_moff.data_ptr())
    w.eng.sync()
    tag = (name, tag, "device", cap_r, cap_m)
    assert st.tolist() == e["status"] and ph.tolist() == e["phase"], tag
    assert roff.tolist() == e["receipt_off"] and moff.tolist() == e["match_off"] and (nr, nm) == (total_r, total_m), tag
    assert d_roff.cpu().tolist() == e["receipt_off"] + [-1] and d_moff.cpu().tolist() == e["match_off"] + [-1], tag
    assert w.last_scan_phase() == e["last_phase"], tag
    take_r, take_m = min(cap_r, total_r), min(cap_m, total_m)
    has = d_has.cpu().numpy()
    assert has[:take_r].tolist() == e["has"][:take_r] and has[take_r:].tolist() == [9] * (len(has) - take_r), tag  # nothing behind the prefix
    raw = d_m.cpu().numpy()
    m = raw[: take_m * item].view(ipcfp.MATCH_DTYPE)
    ms = d_ms.cpu().numpy()
    assert rows(m, ms[:take_m]) == e["rows"][:take_m], tag
    assert set(raw[take_m * item:].tolist()) == {0xAB} and set(ms[take_m:].tolist()) == {0x7fffffff}, tag
    cnt = d_cnt.cpu().numpy()
    assert cnt[:-1].tolist() == e["spec_counts"] and int(cnt[-1]) == -1, tag


CHAINS = list(tc.chains())


@pytest.mark.parametrize("name", CHAINS)
def test_every_chain_on_every_route(wit, name):
    held_host(wit, name, touched=True)
    held_host(wit, name, touched=False)
    device_form(wit, name)


@pytest.mark.parametrize("name", [n for n in CHAINS if len(tc.chains()[n][0]) <= 66] + ["mixed/257"])
def test_the_single_calls_on_the_same_witness_concatenate_to_the_same_bytes(wit, name):
    tipsets, key = tc.chains()[name]
    specs = tc.SPEC_SETS[key]
    g = wit.scan_events_tipsets(roots_of(tipsets), specs, want_touched=True)
    has, m, ms, ids, status, phase, roff, moff = [], [], [], set(), [], [], [0], [0]
    counts = np.zeros(len(specs), dtype=np.uint64)
    for root in roots_of(tipsets):
        s = wit.scan_events_multi(root, specs, want_touched=True)
        status.append(s[0])
        phase.append(wit.last_scan_phase())
        if s[0] == pyevents.TRUE:
            has.append(s[1].tobytes())
            m.append(s[2].tobytes())
            ms.append(s[3].tobytes())
            counts += s[4]
            ids |= set(s[5].tolist())
        roff.append(roff[-1] + (len(s[1]) if s[0] == pyevents.TRUE else 0))
        moff.append(moff[-1] + (len(s[2]) if s[0] == pyevents.TRUE else 0))
    assert g["status"].tolist() == status and g["phase"].tolist() == phase, name
    assert g["receipt_off"].tolist() == roff and g["match_off"].tolist() == moff, name
    assert g["has_match"].tobytes() == b"".join(has) and g["matches"].tobytes() == b"".join(m) and g["match_spec"].tobytes() == b"".join(ms), name
    assert g["spec_counts"].tolist() == counts.tolist() and set(g["touched"].tolist()) == ids, name
    if len(tipsets) == 1:  # T = 1: ipcfp_scan_events_multi, byte for byte
        s = wit.scan_events_multi(roots_of(tipsets)[0], specs, want_touched=True)
        if s[0] == pyevents.TRUE:
            assert (g["has_match"].tobytes(), g["matches"].tobytes(), g["match_spec"].tobytes(), g["spec_counts"].tobytes(), g["touched"].tobytes()) == \
                (s[1].tobytes(), s[2].tobytes(), s[3].tobytes(), s[4].tobytes(), s[5].tobytes())
        else:
            assert g["n_receipts"] == g["n_matches"] == 0 and not g["spec_counts"].any() and len(g["touched"]) == 0


@pytest.mark.parametrize("name", ["fail/one_of_each_phase", "tile/1023+1025", "mixed/257", "empty/two_in_a_row", "fail/every_tipset"])
def test_capacities_cut_the_concatenated_outputs_to_a_prefix(wit, name):
    tipsets, key = tc.chains()[name]
    e = tc.expected_chain(name)
    roff, moff = e["receipt_off"], e["match_off"]
    total_r, total_m = roff[-1], moff[-1]
    inside_r = next((a + (b - a) // 2 for a, b in zip(roff, roff[1:]) if b - a >= 2), 0)
    inside_m = next((a + (b - a) // 2 for a, b in zip(moff, moff[1:]) if b - a >= 2), 0)
    on_r = next((b for a, b in zip(roff, roff[1:]) if 0 < b < total_r), 0)
    on_m = next((b for a, b in zip(moff, moff[1:]) if 0 < b < total_m), 0)
    caps_r = sorted({0, 1, inside_r, on_r, max(total_r - 1, 0), total_r})
    caps_m = sorted({0, 1, inside_m, on_m, max(total_m - 1, 0), total_m})
    if total_r:
        assert inside_r and on_r and inside_m and on_m, name
    for cap_r, cap_m in [(c, total_m) for c in caps_r] + [(total_r, c) for c in caps_m] + [(caps_r[len(caps_r) // 2], caps_m[len(caps_m) // 2])]:
        device_form(wit, name, cap_r=cap_r, cap_m=cap_m, tag="caps")
        g = wit.scan_events_tipsets(roots_of(tipsets), tc.SPEC_SETS[key], want_touched=False, cap_matches=cap_m, cap_receipts=cap_r)
        assert g["has_match"].tolist() == e["has"][:cap_r] and rows(g["matches"], g["match_spec"]) == e["rows"][:cap_m], (name, cap_r, cap_m)
        assert g["receipt_off"].tolist() == roff and g["match_off"].tolist() == moff and g["spec_counts"].tolist() == e["spec_counts"], (name, cap_r, cap_m)
        assert (g["n_receipts"], g["n_matches"]) == (total_r, total_m), (name, cap_r, cap_m)
        for t, st in enumerate(e["status"]):
            if st != pyevents.TRUE:  # nothing is written for a failing tipset
                assert len(g["maps"][t]) == 0 and len(g["records"][t]) == 0, (name, t)


# ---- the state around the call --------------------------------------------------------------------------------------------------------
def single(w, root, sp):
    got = w.scan_events(root, sp[0], sp[1], actor=sp[2])
    return tuple(x if not hasattr(x, "tobytes") else x.tobytes() for x in got) + (w.last_scan_phase(),)


def multi(w, root, specs):
    s = w.scan_events_multi(root, specs)
    return tuple(x if not hasattr(x, "tobytes") else x.tobytes() for x in s[:6])


@pytest.mark.parametrize("table", [True, False])
def test_single_tipset_calls_do_not_notice_a_chain_call(engine, table):
    store, roots = tc.world()
    name = "fail/one_of_each_phase"
    tipsets, key = tc.chains()[name]
    specs = tc.SPEC_SETS[key]
    sp = specs[1]  # (an emitter filter: what the scan hint and the block table's filter would carry)
    with witness_of(engine, store, table) as w:
        before = [single(w, roots["edges"], sp), multi(w, roots["edges"], specs), single(w, roots[tc.FAIL_EVENTS[0]], sp)]
        held_host(w, name, tag="between single calls")
        after = [single(w, roots["edges"], sp), multi(w, roots["edges"], specs), single(w, roots[tc.FAIL_EVENTS[0]], sp)]
        assert before == after
        # a root never scanned singly still makes its own enumeration on its first single scan, and only on the first
        engine.profile_enable(True, only="exec_order")
        try:
            walks = []
            for _turn in (0, 1):
                engine.profile_reset()
                got = single(w, roots[tc.A], specs[0])
                walks.append(engine.profile_read("exec_order")[0])
            assert walks[0] >= 1 and walks[1] == 0, walks
        finally:
            engine.profile_enable(False)
        want = pyevents.scan(store.blocks, roots[tc.A], *specs[0])
        assert got[0] == 1 and np.frombuffer(got[1], np.uint8).tolist() == want[1] and rows(np.frombuffer(got[2], ipcfp.MATCH_DTYPE)) == want[2]
        # the chain call itself enumerates every time: it neither reads nor fills the per-root cache
        engine.profile_enable(True, only="exec_order")
        try:
            engine.profile_reset()
            device_form(w, "empty/middle", tag="after the single scans")
            assert engine.profile_read("exec_order")[0] >= 1
        finally:
            engine.profile_enable(False)
    with witness_of(engine, store, table) as fresh:  # a witness that never saw a chain call
        assert [single(fresh, roots["edges"], sp), multi(fresh, roots["edges"], specs), single(fresh, roots[tc.FAIL_EVENTS[0]], sp)] == before


def test_a_rebuild_index_between_two_chain_calls_changes_nothing(wit):
    a = held_host(wit, "mixed/257", tag="before the rebuild")
    wit.rebuild_index()
    b = held_host(wit, "mixed/257", tag="after the rebuild")
    for k in ("has_match", "matches", "match_spec", "spec_counts", "touched", "receipt_off", "match_off"):
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- profile scopes ---------------------------------------------------------------------------------------------------------------------
def scopes(engine, w, tipsets, specs):
    """(enumerations made, launch groups of the new kernels, statuses) of one device-form call.  `exec_order` has ONE profile
    scope around a whole amt_enumerate and `scan_tipsets` one per launcher of event_scan_tipsets.inc, so these are counts of
    enumerations and of launch groups, not of kernel launches: that the launches INSIDE an enumeration are per level and not
    per root is how enum_general is written (host/amt_enumerate.cpp), which no profile group observes."""
    engine.profile_enable(True)
    try:
        engine.profile_reset()
        st, *_ = w.scan_events_tipsets_device(roots_of(tipsets), specs)
        return engine.profile_read("exec_order")[0], engine.profile_read("scan_tipsets")[0], st.tolist()
    finally:
        engine.profile_enable(False)


def test_enumerations_and_launch_groups_do_not_depend_on_the_length_of_a_sound_chain(engine, wit):
    flat = ["ae/size_9", "ae/size_63", "ae/size_64", "ae/count_20_receipts_immediate"]  # trees of height 1
    specs = tc.SPECS_8
    e4, s4, st4 = scopes(engine, wit, tc.cycle(flat, 4), specs)
    e64, s64, st64 = scopes(engine, wit, tc.cycle(flat, 64), specs)
    assert set(st4) == set(st64) == {1}
    assert (e4, s4) == (e64, s64) and e4 >= 1 and s4 >= 1, (e4, s4, e64, s64)
    # beyond the dense plan's 65 roots the general walk serves the chain: per level, not per root
    e66, s66, _ = scopes(engine, wit, tc.cycle(flat, 66), specs)
    e512, s512, _ = scopes(engine, wit, tc.cycle(flat, 512), specs)
    assert (e66, s66) == (e512, s512) and s66 == s4, (e66, s66, e512, s512)
    # k failing receipts trees: at most k + 1 enumerations (times the sound chain's own count on the same route: 64 roots with
    # a dead one among them take the general walk's first step, like the chain of 66)
    for k, bad in ((1, [tc.FAIL_RECEIPTS[0]]), (2, list(tc.FAIL_RECEIPTS[:2])), (3, list(tc.FAIL_RECEIPTS))):
        chain = tc.cycle(flat, 64)
        for i, f in enumerate(bad):
            chain[7 + 20 * i] = f
        ek, sk, stk = scopes(engine, wit, chain, specs)
        assert sum(1 for s in stk if s != 1) == k
        assert e64 == e66 == 1 and ek <= (k + 1) * e64 and sk == s64, (k, ek, sk)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_and_refusals(engine, wit):
    _store, roots = tc.world()
    one = [roots[tc.A]]
    specs = tc.SPECS_2
    for call in (wit.scan_events_tipsets, wit.scan_events_tipsets_device):
        with pytest.raises(ipcfp.EngineError, match=r"\(-1\)"):
            call([], specs)
        with pytest.raises(ipcfp.EngineError, match=r"\(-1\)"):
            call(one, [])
        with pytest.raises(ipcfp.EngineError, match=r"\(-5\)"):
            call(one, mc.padded([], 1024) + [(*mc.pair(0), None)])
        with pytest.raises(ipcfp.EngineError, match=r"\(-5\)"):
            call(roots_of(tc.refused_chain()), specs)
    assert ipcfp.MAX_SCAN_TIPSETS == tc.MAX_TIPSETS
    # null mandatory pointers and a has_actor[j] without actors, at the C ABI
    lib, C = engine.lib, __import__("ctypes")
    slots = ipcfp.cid_slots(one).copy()
    filt, has_a, actors = wit._scan_specs([(*mc.pair(0), 7)])
    st, ph = np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    nr, nm = C.c_uint64(), C.c_uint64()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = [engine.h, wit.h, p(slots), 1, p(filt), p(has_a), p(actors), 1, p(st), p(ph), None, None, None, 0, C.byref(nr), None, None, 0, C.byref(nm), None, None]
    assert lib.ipcfp_scan_events_tipsets(*good) == 0 and st[0] == 1
    for k in (2, 4, 6, 8, 14, 18):  # roots, filters, actors (under a set has_actor), tipset_status, n_receipts, n_matches
        bad = list(good)
        bad[k] = None
        assert lib.ipcfp_scan_events_tipsets(*bad) == -1, k
    no_has = list(good)
    no_has[5] = no_has[6] = None  # (no spec filters by emitter: actors may be null)
    assert lib.ipcfp_scan_events_tipsets(*no_has) == 0
    # … and the same on the device form
    good_d = good[:12] + [None, None, None, 0, C.byref(nr), None, None, 0, C.byref(nm), None]
    st[0] = 0
    assert lib.ipcfp_scan_events_tipsets_device(*good_d) == 0 and st[0] == 1
    for k in (2, 4, 6, 8, 16, 20):  # roots, filters, actors (under a set has_actor), tipset_status, n_receipts, n_matches
        bad = list(good_d)
        bad[k] = None
        assert lib.ipcfp_scan_events_tipsets_device(*bad) == -1, k
    no_has = list(good_d)
    no_has[5] = no_has[6] = None
    assert lib.ipcfp_scan_events_tipsets_device(*no_has) == 0


def test_a_witness_with_a_receipt_range_is_refused(engine):
    store, roots = tc.world()
    with witness_of(engine, store) as whole:
        w = whole.subset(np.arange(whole.n), 2, 9)
        try:
            for call in (w.scan_events_tipsets, w.scan_events_tipsets_device):
                with pytest.raises(ipcfp.EngineError, match=r"\(-1\)"):
                    call([roots[tc.A]], tc.SPECS_2)
            assert w.scan_events_multi(roots[tc.A], tc.SPECS_2)[0] == 1  # (the single-tipset call serves the shard)
        finally:
            w.close()
        assert whole.scan_events_tipsets([roots[tc.A]], tc.SPECS_2)["status"].tolist() == [1]
