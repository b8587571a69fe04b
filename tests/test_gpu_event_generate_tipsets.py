"""GPU: ipcfp_generate_event_claims_tipsets — generate_event_proof for a CHAIN of tipset pairs in one pass — through the C ABI,
on every chain of tests/event_gen_chain_cases.py.

For each chain: the per-tipset statuses, the claim offsets, the match records, the message CIDs, the claims and blob (through
_proofs: ipcfp_unpack_event_claims over the handle's tipsets) and the recorded blocks in `Cid: Ord` order against the case
module (tests/test_event_generate_tipsets.py holds that to the oracle on the CPU).  A second judge for chains of up to 64
tipsets: T single calls on the same witness, byte-compared after the rebasing the header names.  Then the round trip through
the verifier on the subset witness, the refusals, the state around the call and the counts of enumerations.  Every input here
is one a hostile bundle may contain; nothing tries to provoke a device fault."""
import ctypes as C

import numpy as np
import pytest
import torch

import event_chain_cases as ec
import event_gen_chain_cases as gc
import ipc_filecoin_proofs_amd as ipcfp
import pyevents

pytestmark = pytest.mark.gpu

CHAINS = list(gc.chains())


@pytest.fixture(scope="module")
def wit(engine):
    store, _pairs = gc.world()
    with engine.witness(*store.tables()) as w:
        yield w


def pairs_of(name):
    _store, pairs = gc.world()
    return [pairs[p] for p in gc.chains()[name]]


def slot(cid):
    return bytes(cid).ljust(ipcfp.binding.CID_SLOT, b"\0")


def rows_of(g):
    m, c = g.matches()
    return [(int(a), int(b), int(e), bytes(s)) for a, b, e, s in zip(m["exec_index"], m["event_index"], m["emitter"], c)]


@pytest.fixture(scope="module")
def heights():
    store, _ = gc.world()
    return lambda cid: pyevents.header(store.blocks[cid]).height


def held(w, name, heights, tag=""):
    """one chain call against expected_chain → the handle (the caller closes it)"""
    store, _ = gc.world()
    e = gc.expected_chain(name)
    pairs = pairs_of(name)
    g = w.generate_event_claims_tipsets(pairs, *gc.FILTER)
    tag = (name, tag)
    assert g.tipset_count == len(pairs) == len(g.tipsets), tag
    assert g.tipset_status.tolist() == e["status"], tag
    assert g.tipset_claim_off.tolist() == e["claim_off"] and g.n == len(e["rows"]), tag
    assert rows_of(g) == [(*r[:3], slot(r[3])) for r in e["rows"]], tag
    cids = list(store.blocks)
    assert [cids[i] for i in g.block_ids.tolist()] == e["needed"], tag
    for t, (parents, child) in enumerate(pairs):  # one ipcfp_tipset_ref_t per INPUT tipset, failing ones included
        ref = g.tipsets[t]
        assert ref["flags"] == 3 and ref["n_parents"] == len(parents) and bytes(ref["child"]) == slot(child), tag
        n_inline = min(len(parents), ipcfp.binding.MAX_PARENTS)
        assert [bytes(p) for p in ref["parents"][:n_inline]] == [slot(p) for p in parents[:n_inline]], tag
        assert bool(ref["more_parents"]) == (len(parents) > ipcfp.binding.MAX_PARENTS), tag
    # claims and blob, spelled by the library over the handle's own tipsets
    proofs = g.proof_rows()
    assert len(proofs) == g.n, tag
    k = 0
    for t, (parents, child) in enumerate(pairs):
        for r in e["per_tipset"][t]:
            p = proofs[k]
            assert (p["exec_index"], p["event_index"], p["emitter"], p["message_cid"]) == (*r[:3], ec.cid_str(r[3])), (tag, k)
            assert p["parent_tipset_cids"] == [ec.cid_str(c) for c in parents] and p["child_block_cid"] == ec.cid_str(child), (tag, k)
            assert (p["parent_epoch"], p["child_epoch"]) == (heights(parents[0]), heights(child)), (tag, k)
            k += 1
    claims, _blob = g.copy()
    for t in range(len(pairs)):
        a, b = e["claim_off"][t], e["claim_off"][t + 1]
        assert set(claims["tipset"][a:b].tolist()) <= {t}, tag
    return g


def rebased(claims, blob, a, b, start, length):
    """claims [a, b) of a chain and their blob segment [start, start + length) as the single call spells them"""
    c = claims[a:b].copy()
    c["tipset"] = 0
    c["topics_off"] -= np.uint32(start)
    c["data_off"] -= np.uint32(start)
    return c.tobytes(), blob[start:start + length].tobytes()


@pytest.mark.parametrize("name", CHAINS)
def test_chain(wit, heights, name):
    with held(wit, name, heights) as g:
        pairs = pairs_of(name)
        if len(pairs) > gc.SINGLE_CALL_LIMIT:
            return
        claims, blob = g.copy()
        m, c = g.matches()
        start = 0
        for t, (parents, child) in enumerate(pairs):  # the second judge: the single call on the same witness
            st, gs = wit.generate_event_claims(parents, child, *gc.FILTER)
            assert st == g.tipset_status[t], (name, t)
            a, b = (int(x) for x in g.tipset_claim_off[t:t + 2])
            if gs is None:
                assert a == b, (name, t)
                continue
            with gs:
                sc, sb = gs.copy()
                sm, smc = gs.matches()
                assert b - a == gs.n, (name, t)
                assert rebased(claims, blob, a, b, start, gs.blob_len) == (sc.tobytes(), sb.tobytes()), (name, t)
                assert m[a:b].tobytes() == sm.tobytes() and c[a:b].tobytes() == smc.tobytes(), (name, t)
                start += gs.blob_len
        assert start == g.blob_len, name


ROUND_TRIP = [n for n in CHAINS if not n.startswith("one/") and n != "fail/every_tipset" and len(gc.chains()[n]) <= gc.SINGLE_CALL_LIMIT]


@pytest.mark.parametrize("name", ROUND_TRIP + ["one/ok/0", "one/parents/33"])
def test_round_trip_through_the_verifier(wit, name):
    """the handle's tipsets, claims and blob on the subset witness of its _block_ids: every claim verifies"""
    with wit.generate_event_claims_tipsets(pairs_of(name), *gc.FILTER) as g:
        sub = wit.subset(g.block_ids)
        try:
            status = torch.full((max(g.n, 1),), 0xEE, dtype=torch.uint8, device="cuda")
            if g.n:
                sub.verify_event_claims_device(g.tipsets, g.claims_ptr, g.n, g.blob_ptr, g.blob_len, status.data_ptr())
                wit.eng.sync()
                assert set(status.cpu().tolist()) == {1}, name
        finally:
            sub.close()


def test_all_places_without_a_match_still_record(wit, heights):
    with held(wit, "nomatch/all", heights) as g:
        assert g.n == 0 and g.blob_len == 0 and len(g.block_ids) > 0
        assert g.copy()[1].size == 0
    with held(wit, "fail/every_tipset", heights) as g:
        assert g.n == 0 and g.blob_len == 0 and len(g.block_ids) == 0


def test_a_handle_of_the_single_call(wit):
    _store, pairs = gc.world()
    parents, child = pairs["ok/0"]
    st, g = wit.generate_event_claims(parents, child, *gc.FILTER)
    with g:
        assert st == 1 and g.tipset_count == 1 and g.tipset_status.tolist() == [1] and g.tipset_claim_off.tolist() == [0, g.n]
        assert len(g.tipsets) == 1 and g.n == 7


def test_an_emitter_filter(wit):
    """has_actor / actor reach the scan: one emitter of ok/0, none of ok/1"""
    _store, pairs = gc.world()
    want = [gc.expected_pair(p, gc._emitter("ok/0", 2)) for p in ("ok/0", "ok/1")]
    with wit.generate_event_claims_tipsets([pairs["ok/0"], pairs["ok/1"]], *gc.FILTER, actor=gc._emitter("ok/0", 2)) as g:
        assert g.tipset_status.tolist() == [1, 1] and g.tipset_claim_off.tolist() == [0, 1, 1]
        assert rows_of(g) == [(*r[:3], slot(r[3])) for w_ in want for r in w_[1]]


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def raw_call(engine, w, parents40, off, children40, T, filt, out, has_actor=0):
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    return engine.lib.ipcfp_generate_event_claims_tipsets(engine.h, None if w is None else w.h, p(parents40), p(off), p(children40), T, p(filt),
                                                          has_actor, 0, None if out is None else C.byref(out))


def test_argument_errors_and_refusals(engine, wit):
    _store, pairs = gc.world()
    parents, child = pairs["ok/1"]
    p40, c40 = ipcfp.cid_slots(parents).copy(), ipcfp.cid_slots([child]).copy()
    off = np.array([0, len(parents)], dtype=np.uint32)
    filt = np.frombuffer(gc.FILTER[0] + gc.FILTER[1], dtype=np.uint8).copy()
    SENTINEL = 0x1234
    def refused(rc_want, text, *a, **kw):
        out = C.c_void_p(SENTINEL)
        assert raw_call(engine, *a, out, **kw) == rc_want, text
        assert out.value is None, text  # *out == NULL after any refusal
        if text:
            assert text in (engine.lib.ipcfp_last_error(engine.h) or b"").decode(), text
    good = C.c_void_p(SENTINEL)
    assert raw_call(engine, wit, p40, off, c40, 1, filt, good) == 0 and good.value not in (None, SENTINEL)
    engine.lib.ipcfp_generated_events_destroy(good)
    # IPCFP_E_INVALID: null mandatory pointers, no tipset, offsets that do not ascend from 0
    refused(-1, "", None, p40, off, c40, 1, filt)
    refused(-1, "", wit, p40, None, c40, 1, filt)
    refused(-1, "", wit, p40, off, None, 1, filt)
    refused(-1, "", wit, p40, off, c40, 1, None)
    refused(-1, "", wit, p40, off, c40, 0, filt)
    assert raw_call(engine, wit, p40, off, c40, 1, filt, None) == -1
    refused(-1, "parent slots without parent_cids40", wit, None, off, c40, 1, filt)
    refused(-1, "does not ascend from 0", wit, p40, np.array([1, 1], dtype=np.uint32), c40, 1, filt)
    refused(-1, "does not ascend from 0", wit, np.tile(p40, (3, 1)), np.array([0, 2, 1], dtype=np.uint32), np.tile(c40, (2, 1)), 2, filt)
    # IPCFP_E_UNSUPPORTED, from the arguments alone: too many tipsets; 2048 tipsets of 16 arbitrary parent slots = 65 536 roots
    T = gc.MAX_TIPSETS + 1
    refused(-5, "tipsets (at most", wit, np.tile(p40, (T, 1)), np.arange(T + 1, dtype=np.uint32), np.tile(c40, (T, 1)), T, filt)
    junk = np.full((2048 * 16, ipcfp.binding.CID_SLOT), 0x5A, dtype=np.uint8)
    refused(-5, "65536 message-tree roots", wit, junk, np.arange(2049, dtype=np.uint32) * 16, np.tile(c40, (2048, 1)), 2048, filt)
    # … one parent slot fewer is taken (and answers: no such parents)
    with wit.generate_event_claims_tipsets([([bytes(junk[0])[:38]] * 15, child)] + [([bytes(junk[0])[:38]] * 16, child)] * 2047, *gc.FILTER) as g:
        assert g.tipset_count == 2048 and set(g.tipset_status.tolist()) == {gc.ERR_MISSING_BLOCK} and g.n == 0 and len(g.block_ids) == 0
    with pytest.raises(ipcfp.EngineError, match=r"\(-1\)"):
        wit.generate_event_claims_tipsets([], *gc.FILTER)


def test_a_witness_with_a_receipt_range_is_refused(engine, wit):
    _store, pairs = gc.world()
    w = wit.subset(np.arange(wit.n), 2, 9)
    try:
        with pytest.raises(ipcfp.EngineError, match=r"\(-1\).*receipt range"):
            w.generate_event_claims_tipsets([pairs["ok/0"]], *gc.FILTER)
    finally:
        w.close()
    with wit.generate_event_claims_tipsets([pairs["ok/0"]], *gc.FILTER) as g:
        assert g.tipset_status.tolist() == [1]


# ---- the state around the call ------------------------------------------------------------------------------------------------------------
def singles(w, store, pairs):
    out = []
    for name in ("ok/0", "fail/events/0", "nine"):
        parents, child = pairs[name]
        st, g = w.generate_event_claims(parents, child, *gc.FILTER)
        if g is None:
            out.append((st,))
        else:
            with g:
                cl, bl = g.copy()
                out.append((st, cl.tobytes(), bl.tobytes(), g.block_ids.tobytes()))
        root = pyevents.header(store.blocks[pairs["ok/0"][1]]).receipts
        sc = w.scan_events(root, *gc.FILTER, actor=gc._emitter("ok/0", 1))
        out.append(tuple(x if not hasattr(x, "tobytes") else x.tobytes() for x in sc) + (w.last_scan_phase(),))
    with w.generate_event_claims_tipsets([pairs["ok/0"]], *gc.FILTER) as g:  # claims to verify, made by the call under test itself
        status = torch.zeros(g.n, dtype=torch.uint8, device="cuda")
        w.verify_event_claims_device(g.tipsets, g.claims_ptr, g.n, g.blob_ptr, g.blob_len, status.data_ptr())
        w.eng.sync()
        out.append(bytes(status.cpu().tolist()))
    return out


def test_single_tipset_calls_do_not_notice_a_chain_call(engine, heights):
    store, pairs = gc.world()
    with engine.witness(*store.tables()) as w:
        before = singles(w, store, pairs)
        held(w, "fail/two_kinds", heights, tag="between single calls").close()
        after = singles(w, store, pairs)
        assert before == after
        held(w, "sound/17", heights, tag="after single calls").close()
        assert singles(w, store, pairs) == before
    with engine.witness(*store.tables()) as fresh:  # a witness that never saw a chain call
        assert singles(fresh, store, pairs)[:-1] == before[:-1]


# ---- profile scopes -------------------------------------------------------------------------------------------------------------------------
def scopes(engine, w, pairs):
    """(enumerations made, launch groups of the new kernels, statuses) of one chain call: `exec_order` has one scope around a
    whole amt_enumerate, `gen_tipsets` one per launcher of event_gen_tipsets.inc"""
    engine.profile_enable(True)
    try:
        engine.profile_reset()
        with w.generate_event_claims_tipsets(pairs, *gc.FILTER) as g:
            return engine.profile_read("exec_order")[0], engine.profile_read("gen_tipsets")[0], g.tipset_status.tolist()
    finally:
        engine.profile_enable(False)


def test_enumerations_do_not_depend_on_the_length_of_a_sound_chain(engine, wit):
    _store, pairs = gc.world()
    same_shape = [pairs[f"ok/{k}"] for k in range(0, 17, 3)]  # two parents of (3, 1) and (2, 1) messages each
    e2, s2, st2 = scopes(engine, wit, gc.cycle(same_shape, 2))
    e64, s64, st64 = scopes(engine, wit, gc.cycle(same_shape, 64))
    assert set(st2) == set(st64) == {1}
    assert e2 == e64 == 2, (e2, e64)  # all message trees, then all receipts trees
    assert s2 == s64 and s2 >= 1, (s2, s64)


@pytest.mark.parametrize("name", [n for n in CHAINS if n.startswith("fail/") and not n.startswith("one/")])
def test_failing_chains_make_at_most_4_plus_f_enumerations(engine, wit, name):
    e, _s, st = scopes(engine, wit, pairs_of(name))
    f = sum(1 for s in st if s != 1)
    assert f >= 1 and e <= 4 + f, (name, e, f)
