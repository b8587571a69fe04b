"""GPU: the event chain's named cases (tests/event_chain_cases.py) through EVERY route of the engine —

    strings         verify_event_proofs
    packed_fast     pack_event_proofs → verify_event_claims, tuning fast_verify = 1
    packed_general  the same, fast_verify = 0 (the index rebuilt between the two)
    device          verify_event_claims_device on uploaded claims
    compact         compact_event_claims → verify_event_claims_compact, for the claims the transport form can carry
    one_call        verify_and_scan_device
    one_call_cached the same call again, on the receipts and the event table the call before left on the witness
    located         verify_event_proofs_located — whose location must hold the claimed StampedEvent whenever the verifier
                    got as far as comparing it

— against the literal status of each case, and for the mutator against tests/pyevents.py.  Every route but one_call_cached
makes FIRST CONTACT with the witness: the index is rebuilt in front of it, which drops the receipts enumeration and the
event table an earlier call filed there, so that with default tuning and one tipset each takes the route without a
mid-call synchronisation (host/verify_fast.cpp) — the riding scan of verify_and_scan_device included — where it applies.  One witness per case with a batch
of one; every receipt case as ONE batch over one_tipset() (the event table's route), in receipt order, shuffled with
repeats, under a filter and under a trust window; two tipsets in one witness; the scan and the generator against pyevents
on every witness.  Measured on an MI355X: no test of this file takes more than 0.5 s."""
import numpy as np
import pytest
import torch

import assumption_cases as ac
import event_chain_cases as ec
import ipc_filecoin_proofs_amd as ipcfp
import pyamt
import pyevents
import pystorage
from conftest import fuzz_seed

pytestmark = pytest.mark.gpu

ROUTES = ("strings", "packed_fast", "packed_general", "device", "compact", "one_call", "one_call_cached", "located")
NAMES = list(ec.CASES)


@pytest.fixture()
def routed(engine):
    def use(fast):
        engine.set_tuning("fast_verify", fast)
    yield use
    engine.set_tuning("fast_verify", -1)


def dev(a):
    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.zeros(64, np.uint8)])).cuda()  # (never an empty allocation)


def compactable(pr):
    """positions of the claims the transport form carries, by the CPU converter, one claim at a time"""
    keep = []
    for i in range(pr.n):
        one = ec.proofs([pr.rows[i]])
        _ts, cl, blob = ipcfp.pack_event_proofs(one.arr, one.n)
        try:
            ipcfp.compact_event_claims(cl, blob, len(blob))
            keep.append(i)
        except ipcfp.EngineError:
            pass
    return keep


def answers(w, use, blocks, claim_list, trust=None, filt=None, out_loc=None):
    """{route: [status]} of one batch over one witness; a claim the compact form refuses is None on that route.
    `out_loc`: a list that receives the located route's locations"""
    pr = ec.proofs(claim_list)
    pr.rows = claim_list
    n = pr.n
    tp, ft = ec.trust_policy(trust), ec.event_filter(filt)
    use(-1)
    out = {"strings": w.verify_event_proofs(pr.arr, n, trust=tp, filt=ft).tolist()}
    ts, cl, blob = ipcfp.pack_event_proofs(pr.arr, n)
    for fast, tag in ((1, "packed_fast"), (0, "packed_general")):
        use(fast)
        w.rebuild_index()
        out[tag] = w.verify_event_claims(ts, cl, blob, len(blob), trust=tp, filt=ft).tolist()
    use(-1)
    w.rebuild_index()
    d_cl, d_blob = dev(cl), dev(blob)
    d_st = torch.full((n + 64,), 77, dtype=torch.uint8, device="cuda")
    w.verify_event_claims_device(ts, d_cl.data_ptr(), n, d_blob.data_ptr(), len(blob), d_st.data_ptr(), trust=tp, filt=ft)
    w.eng.sync()
    out["device"] = d_st.cpu().numpy()[:n].tolist()
    # compact: the whole batch where the converter takes it, else the claims it takes one by one
    keep = list(range(n))
    try:
        groups, cc, cblob, cblob_len = ipcfp.compact_event_claims(cl, blob, len(blob))
        ts_c = ts
    except ipcfp.EngineError:
        keep = compactable(pr)
        if keep:
            sub = ec.proofs([claim_list[i] for i in keep])
            ts_c, cl_c, blob_c = ipcfp.pack_event_proofs(sub.arr, sub.n)
            groups, cc, cblob, cblob_len = ipcfp.compact_event_claims(cl_c, blob_c, len(blob_c))
    out["compact"] = [None] * n
    if keep:
        w.rebuild_index()
        got = w.verify_event_claims_compact(ts_c, groups, cc, cblob, cblob_len, trust=tp, filt=ft).tolist()
        for i, g in zip(keep, got):
            out["compact"][i] = g
    # one call: verify + the scan of tipsets[0]'s child — whose scan answer is pyevents' wherever the first tipset's child
    # header names a receipts root; on first contact (the scan rides on the verify call), then on what that call cached
    try:
        child = pystorage.cid_from_string(claim_list[0]["child_block_cid"])
        [pystorage.cid_from_string(s) for s in claim_list[0]["parent_tipset_cids"]]
        want = pyevents.scan(blocks, pyevents.header(blocks[child]).receipts, ec.FILTER[0], ec.FILTER[1]) if child in blocks else None
    except (ValueError, pystorage.Err):
        want = None
    d_has = torch.zeros(1 << 12, dtype=torch.uint8, device="cuda")
    d_m = torch.zeros((1 << 12) * ipcfp.MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    for tag in ("one_call", "one_call_cached"):
        if tag == "one_call":
            w.rebuild_index()
        d_st.fill_(77)
        d_has.fill_(9)
        d_m.fill_(0)
        sst, snr, snm = w.verify_and_scan_device(ts, d_cl.data_ptr(), n, d_blob.data_ptr(), len(blob), d_st.data_ptr(), ec.FILTER[0], ec.FILTER[1],
                                                 None, d_has.data_ptr(), 1 << 12, d_m.data_ptr(), 1 << 12, trust=tp, filt=ft)
        w.eng.sync()
        out[tag] = d_st.cpu().numpy()[:n].tolist()
        if want is not None:
            assert sst == want[0], (tag, "scan status", sst, want[0])
            if sst == 1:
                m = d_m.cpu().numpy()[: snm * ipcfp.MATCH_DTYPE.itemsize].view(ipcfp.MATCH_DTYPE)
                assert d_has.cpu().numpy()[:snr].tolist() == want[1], tag
                assert [(int(a), int(b), int(c)) for a, b, c in zip(m["exec_index"], m["event_index"], m["emitter"])] == want[2], tag
    w.rebuild_index()
    st, loc = w.verify_event_proofs_located(pr.arr, n, trust=tp, filt=ft)
    out["located"] = st.tolist()
    out["_loc"] = loc
    # the location holds the claimed StampedEvent whenever the verifier compared it (12-17 and TRUE)
    cmp = [i for i in range(n) if st[i] == 1 or 12 <= st[i] <= 17]
    if cmp:
        bad = []
        for i, b in zip(cmp, w.read_values(loc[cmp], stride=int(loc["len"][cmp].max()) + 16)):
            c = claim_list[i]
            try:
                same = b is not None and pyevents.check_stamped_event(pystorage.decode(b)) == pyevents.claimed_event(blocks, c)
            except pystorage.Err as e:
                same = False
                b = f"{e} in {b[:16]!r}…"
            if not same:
                bad.append((c["exec_index"], c["event_index"], c["emitter"], int(st[i]), tuple(int(loc[f][i]) for f in ("block", "off", "len")), b[:40]))
        assert not bad, ("located: (exec_index, event_index, emitter, status, location, bytes)", bad[:8])
    # every route answers every claim with a status verify_event_proof can give: none is skipped, none returns a placeholder
    loc = out.pop("_loc")
    assert set(out) == set(ROUTES), out
    if out_loc is not None:
        out_loc.append(loc)
    assert all(len(v) == n and set(v) <= pyevents.STATUSES | ({None} if r == "compact" else set()) for r, v in out.items()), out
    return out


def wrong_answers(got, names, want):
    return [(name, route, st[i], want[i]) for route, st in got.items() for i, name in enumerate(names) if st[i] is not None and st[i] != want[i]]


def declined(got):
    return sum(1 for g in got["compact"] if g is None)


@pytest.mark.parametrize("group", range(8))
def test_every_case_in_a_witness_of_its_own(engine, routed, group):
    wrong, n_declined, refused = [], 0, 0
    for name in NAMES[group::8]:
        store, claim, expect = ec.CASES[name]
        with engine.witness(*store.tables()) as w:
            got = answers(w, routed, store.blocks, [claim], ec.META[name]["trust"], ec.META[name]["filter"])
        wrong += wrong_answers(got, [name], [expect])
        n_declined += declined(got)
        pr = ec.proofs([claim])
        pr.rows = [claim]
        refused += 1 - len(compactable(pr))
    assert not wrong, wrong
    # no case is skipped on a route except those the compact form's CPU converter refuses
    assert n_declined <= refused < len(NAMES[group::8]) // 2, (n_declined, refused)


def test_event_carried_assumptions(engine, routed):
    wrong = []
    for name in sorted(ac.EVENT_CASES):
        store, claim, expect = ac.EVENT_CASES[name]()
        with engine.witness(*store.tables()) as w:
            wrong += wrong_answers(answers(w, routed, store.blocks, [claim]), [name], [expect])
    assert not wrong, wrong


@pytest.fixture(scope="module")
def one():
    return ec.one_tipset()


# the first-contact routes that, with default tuning (or fast_verify = 1) and one tipset, take host/verify_fast.cpp
FIRST_CONTACT_FAST = ("packed_fast", "device", "compact", "one_call", "located")


def test_one_tipset_in_receipt_order(engine, routed, one):
    """… and the route is the one the module says: IPCFP_K_AMT_WALK brackets the dense walk of host/verify_fast.cpp and
    nothing else, so its launch count says how many calls went down the route without a mid-call synchronisation and
    found the message and receipt AMTs dense — where the verify kernel runs over the event table
    (`launch_verify_events(…, tabulated = true)`).  At least the five first-contact routes must have."""
    store, parts, names, cl, want = one
    engine.profile_enable(True, only="amt_walk")
    engine.profile_reset()
    try:
        with engine.witness(*store.tables()) as w:
            got = answers(w, routed, store.blocks, cl)
        fast_calls = engine.profile_read("amt_walk")[0]
    finally:
        engine.profile_enable(False)
    wrong = wrong_answers(got, names, want)
    assert not wrong, wrong[:20]
    assert declined(got) < len(cl) // 4
    assert fast_calls >= len(FIRST_CONTACT_FAST), fast_calls


def test_event_on_the_last_byte_of_the_arena(engine, routed):
    """The events root is the last block of the arena's schedule (the smallest chunk class, the last id in it) and the event
    its last bytes: the located event ends where the block ends, and behind the block there is only the arena's tail."""
    for name, expect in (("event_ends_on_the_last_byte_of_the_last_block_of_the_arena", 1),
                         ("event_ends_on_the_last_byte_of_the_last_block_of_the_arena_wrong_last_nibble", 15)):
        store, claim, literal = ec.CASES[name]
        assert literal == expect
        data, off, lens, cids = store.tables()
        locs = []
        with engine.witness(data, off, lens, cids) as w:
            got = answers(w, routed, store.blocks, [claim], out_loc=locs)
        assert not wrong_answers(got, [name], [expect])
        loc = locs[0][0]
        last = len(lens) - 1
        assert cids[last, :38].tobytes() == ec.META[name]["parts"]["events_root"]
        assert all(ec.chunks(int(x)) >= ec.chunks(int(lens[last])) for x in lens)
        assert int(loc["block"]) == last and int(loc["off"]) + int(loc["len"]) == int(lens[last]), loc


def test_one_tipset_shuffled_with_repeats(engine, routed, one):
    """run lengths 1-5; more than 256 claims, so a workgroup boundary is crossed"""
    store, parts, names, cl, want = one
    rng = np.random.default_rng(fuzz_seed(8200))
    order = [int(i) for i in rng.permutation(len(cl)) for _ in range(int(rng.integers(1, 6)))]
    assert len(order) > 256
    with engine.witness(*store.tables()) as w:
        got = answers(w, routed, store.blocks, [cl[i] for i in order])
    wrong = wrong_answers(got, [names[i] for i in order], [want[i] for i in order])
    assert not wrong, wrong[:20]


@pytest.mark.parametrize("filt", ["filter_0_1", "filter_0_2"])
def test_one_tipset_under_a_filter(engine, routed, one, filt):
    """the literal of each claim under the filter: event_chain_cases.under_filter of its literal without one"""
    store, parts, names, cl, plain = one
    f = ec.FILTER if filt == "filter_0_1" else ec.OTHER_FILTER
    want = [ec.under_filter(x, c, f) for x, c in zip(plain, cl)]
    assert want.count(17) > 30 and want.count(1) > 10
    with engine.witness(*store.tables()) as w:
        got = answers(w, routed, store.blocks, cl, None, f)
    wrong = wrong_answers(got, names, want)
    assert not wrong, wrong[:20]


def test_one_tipset_under_a_trust_window(engine, routed, one):
    """Every string of these claims parses, so the window decides before any block is read: a claim whose parent epoch is
    moved out of it is 2, one whose child epoch is moved out of it is 3 (verifier.rs:134,139), the rest keep their literal."""
    store, parts, names, cl, plain = one
    rng = np.random.default_rng(fuzz_seed(8201))
    window = ec.TRUST["both_inside"][0]
    claims, want = [], []
    for c, x in zip(cl, plain):
        c = dict(c)
        k = int(rng.integers(6))
        if k == 0:
            c["child_epoch"] += 1
            x = 3
        elif k == 1:
            c["parent_epoch"] -= 1
            x = 2
        claims.append(c)
        want.append(x)
    assert want.count(2) > 30 and want.count(3) > 30 and len(set(want)) >= 10
    with engine.witness(*store.tables()) as w:
        got = answers(w, routed, store.blocks, claims, window)
    wrong = wrong_answers(got, names, want)
    assert not wrong, wrong[:20]


def test_two_tipsets_in_one_witness_interleaved(engine, routed):
    """two tipset pairs in one witness, their claims interleaved: two contexts, the general route by construction"""
    a_store, a_claim, _ = ec.tipset(salt=1)
    b_store, b_claim, b_parts = ec.second_tipset()
    store = pyamt.Store()
    store.blocks = {**a_store.blocks, **b_store.blocks}
    a = [dict(a_claim), {**a_claim, "emitter": 7}, {**a_claim, "exec_index": 3}, {**a_claim, "event_index": 9}, {**a_claim, "message_cid": b_claim["message_cid"]},
         {**a_claim, "child_block_cid": b_claim["child_block_cid"]}, {**a_claim, "data": "0x"}]
    b = [dict(b_claim), {**b_claim, "emitter": 7}, {**b_claim, "parent_epoch": ec.PARENT_EPOCH}, {**b_claim, "topics": b_claim["topics"][:1]},
         {**b_claim, "parent_tipset_cids": a_claim["parent_tipset_cids"]}, {**b_claim, "message_cid": a_claim["message_cid"]}, {**b_claim, "event_index": 1}]
    cl = [c for pair in zip(a, b) for c in pair] * 3
    want = [pyevents.verify(store.blocks, c) for c in cl]
    assert want[:2] == [1, 1] and len(set(want)) >= 8, want
    with engine.witness(*store.tables()) as w:
        got = answers(w, routed, store.blocks, cl)
    wrong = wrong_answers(got, [str(i) for i in range(len(cl))], want)
    assert not wrong, wrong


def scan_witnesses():
    seen = set()
    for n in NAMES:
        if " / " in n and "rc" not in ec.META[n]:
            continue
        key = ec.META[n].get("rc", n)
        if key not in seen:
            seen.add(key)
            yield n, ec.CASES[n][0], ec.META[n]["parts"]
    store, parts, *_ = ec.one_tipset()
    yield "one_tipset", store, parts


# (the second scan of a witness uses another filter than the first: the table's cached match counts cannot be reused)
FILTERS = ((ec.FILTER, None), (ec.OTHER_FILTER, None), (ec.FILTER, 1001), (ec.FILTER, 4000))


@pytest.mark.parametrize("group", range(4))
def test_scan_and_generate_equal_pyevents(engine, group):
    n_ok = n_err = 0
    for name, store, parts in list(scan_witnesses())[group::4]:
        data, off, lens, cids = store.tables()
        with engine.witness(data, off, lens, cids) as w:
            for (t0, t1), actor in FILTERS:
                want = pyevents.scan(store.blocks, parts["receipts"], t0, t1, actor)
                gs, ghas, gm, gids = w.scan_events(parts["receipts"], t0, t1, actor=actor)
                assert gs == want[0], (name, actor, gs, want[0])
                if gs == 1:
                    n_ok += 1
                    assert ghas.tolist() == want[1], (name, actor)
                    assert [(int(a), int(b), int(c)) for a, b, c in zip(gm["exec_index"], gm["event_index"], gm["emitter"])] == want[2], (name, actor)
                    assert {cids[i, :38].tobytes() for i in gids} == want[3], (name, actor)
                else:
                    n_err += 1
                gw = pyevents.generate(store.blocks, parts["parents"], parts["child"], t0, t1, actor)
                gs, gm, gmsg, gids = w.generate_event_proofs(parts["parents"], parts["child"], t0, t1, actor=actor)
                assert gs == gw[0], (name, actor, gs, gw[0])
                if gs == 1:
                    got = [(int(a), int(b), int(c), bytes(m[:38])) for a, b, c, m in zip(gm["exec_index"], gm["event_index"], gm["emitter"], gmsg)]
                    assert got == gw[1], (name, actor)
                    assert {cids[i, :38].tobytes() for i in gids} == gw[2], (name, actor)
    assert n_ok > 80 and n_err > 20


ROUNDS = 150


def test_structured_mutator_engine_equals_pyevents(engine, routed):
    """150 rounds of event_chain_cases.mutated_tipset (tests/test_event_chain.py runs 350 on the CPU), from a seed of its
    own; every route."""
    rng = np.random.default_rng(fuzz_seed(8300))
    wrong = []
    for k in range(ROUNDS):
        blocks, claim, trust, filt = ec.mutated_tipset(rng)
        want = pyevents.verify(blocks, claim, trust, filt)
        with engine.witness(*ec.store_of(blocks).tables()) as w:
            wrong += wrong_answers(answers(w, routed, blocks, [claim], trust, filt), [f"round {k}: {claim}"], [want])
    assert not wrong, wrong[:10]
