"""Tipsets and spec sets for the scan over a SET of event specs (ipcfp_scan_events_multi), buildable on the CPU.

    edges()        one tipset: every receipt case of event_chain_cases.RC that scans clean on its own, then ≈ 40 receipts of
                   this module's own whose events carry ≥ 128 distinct (topic0, topic1) pairs — 3 and 4 topics, Case A,
                   single-topic events, one pair under three emitters, one pair twice in one receipt, a pair and its swap
    tiles()        a receipts tree of 2049 receipts with one small event each (the prefix sum crosses two 1024-tiles), a second
                   event planted at receipts 0, 1023, 1024, 2047 and 2048, and the same tree cut to 1023, 1024 and 1025 receipts
    short_order()  6 executed messages, 8 receipts: spec X matches only at receipt 7 — the generator's per-spec Err
    err_tipsets()  five receipt cases that do NOT scan clean, each alone
    spec sets      spec_sets_over_edges(slot_of): every present pair, traps next to present pairs, repeats, emitter filters,
                   sizes 1 … 1024 padded with pairs nobody emits, shuffles, and pairs whose fingerprints share a home slot
                   (slot_of: the CPU harness of csrc/kernels/filter_set.h, tests/test_scan_multi.py)

A spec is (topic0, topic1, actor or None).  The expected answer of a set is pyevents.scan per spec; `merge` restates the
order contract: the multi list is the J single lists merged by (exec_index, event_index, spec)."""
import functools
import json
import os

import numpy as np

import event_chain_cases as ec
import pyamt
import pyevents
import pymini
from event_spellings import data_bytes, entry, stamped, topic

MAX_SPECS = 1024


# ---- events of this module ---------------------------------------------------------------------------------------------------------
def pair(q):
    """pair q of this module: topics 20 … 219 of event_spellings.topic, none of them one of event_chain_cases.T (1 … 9)"""
    return topic(20 + q), topic(219 - q)


def event(emitter, topics, case_a=False, n_data=12):
    if case_a:
        return stamped(emitter, [entry("topics", b"".join(topics)), entry("data", data_bytes(n_data, emitter & 0xFF))])
    return stamped(emitter, [entry(f"t{k + 1}", t) for k, t in enumerate(topics)] + [entry("d", data_bytes(n_data, emitter & 0xFF))])


N_PAIRS = 130


def named(q):
    """(event signature, subnet id) q: what an EventProofSpec holds (src/proofs/generator.rs:18-22)"""
    return f"ScanMulti{q}(bytes32,uint256)", f"multi-subnet-{q}"


@functools.lru_cache(maxsize=None)
def named_pair(q):
    """the filter create_event_filter makes of named(q): Keccak-256(signature), ascii_to_bytes32(subnet id)"""
    sig, subnet = named(q)
    return pymini.keccak256(sig.encode()), subnet.encode()[:32].ljust(32, b"\0")


N_NAMED = 40
EXTRA = (topic(15), topic(16))  # third and fourth topics
NOBODY = [(topic(230 + k % 20), topic(10 + k // 20)) for k in range(1100)]  # pairs no event carries (topic1 ∈ 10 … 64 + …)


def own_receipts():
    """[events dict or None]: the module's own receipts"""
    out = []
    for r in range(32):  # pairs 0 … 127, four per receipt, in every shape
        evs = {}
        for k in range(4):
            q = 4 * r + k
            a, b = pair(q)
            if k == 0:
                evs[k] = event(7000 + q, [a, b])
            elif k == 1:
                evs[k] = event(7000 + q, [a, b, EXTRA[0]])
            elif k == 2:
                evs[k] = event(7000 + q, [a, b], case_a=True)
            else:
                evs[2 * k] = event(7000 + q, [a, b, EXTRA[0], EXTRA[1]], case_a=(r % 2 == 1))  # (index 6: a gap in the leaf)
        out.append(evs)
    a0, b0 = pair(0)
    a5, b5 = pair(5)
    a9, b9 = pair(9)
    out.append({0: event(8000, [a0]), 1: event(8000, [b0], case_a=True), 2: event(8000, [a0, b0][:1])})  # single-topic: never match
    out.append({0: event(8001, [a0, b0]), 1: event(8002, [a0, b0], case_a=True)})                        # pair 0 under three emitters (7000 above)
    out.append({0: event(8100, [a5, b5]), 1: event(8100, [b5, b5]), 2: event(8101, [a5, b5, EXTRA[1]])})   # pair 5 twice in one receipt
    out.append({0: event(8200, [b9, a9])})                                                                # pair 9 with its topics swapped
    out.append(None)                                                                                      # no events root
    out.append({0: ec.NOT_A_LOG})
    out.append({0: event(8300, list(pair(128))), 3: event(8301, list(pair(129)), case_a=True)})
    out.append({0: event(0, [a0, b0])})                                                                   # emitter 0
    for r in range(N_NAMED // 4):  # pairs a bundle can ask for by name, in the same four shapes
        out.append({k: event(8500 + 4 * r + k, list(named_pair(4 * r + k)) + list(EXTRA[: k % 3]), case_a=(k == 2)) for k in range(4)})
    out.append({0: event(8600, list(named_pair(0))), 1: event(8500, list(named_pair(0))), 5: event(8601, list(named_pair(7)))})
    return out


# ---- the receipt cases of event_chain_cases that scan clean / do not ------------------------------------------------------------------
def _alone(mk):
    return ec.tipset(msgs=[([ec.M("a"), ec.M("b")], [])], at=(0, 0), event=ec.SIB, salt=1,
                     receipts={0: (lambda s: pyamt.receipt(events_root=mk(s))), 1: lambda s: pyamt.receipt()})


@functools.lru_cache(maxsize=None)
def rc_split():
    """(clean, failing): names of the RC cases by whether pyevents.scan accepts the case alone in a tipset"""
    clean, failing = [], []
    for name, mk, _cl in ec.RC:
        st, _claim, parts = _alone(mk)
        (clean if pyevents.scan(st.blocks, parts["receipts"], *ec.FILTER)[0] == pyevents.TRUE else failing).append(name)
    return tuple(clean), tuple(failing)


def _receipt_of(events):
    if events is None:
        return lambda s: pyamt.receipt()
    return lambda s: pyamt.receipt(events_root=ec.events_root(s, events))


@functools.lru_cache(maxsize=None)
def edges():
    """→ (store, parts, n_rc): receipts [0, n_rc) are the clean RC cases, the module's own follow"""
    clean, _ = rc_split()
    by_name = {name: mk for name, mk, _cl in ec.RC}
    makers = [(lambda mk: lambda s: pyamt.receipt(events_root=mk(s)))(by_name[n]) for n in clean]
    makers += [_receipt_of(e) for e in own_receipts()]
    n = len(makers)
    m = [ec.M(f"edges{i}") for i in range(n)]
    msgs = [(m[: n // 3], m[n // 3: n // 2]), (m[n // 2: n - 5] + m[:2], m[n - 5:])]
    st, claim, parts = ec.tipset(msgs=msgs, receipts=dict(enumerate(makers)), at=(0, 0), event=ec.SIB, salt=777)
    parts["claim"] = claim  # the tipset's fields of a claim; the event's fields are the caller's
    return st, parts, len(clean)


def own_claims(k=6):
    """honest claims for event 0 of the module's first k own receipts of edges() (pairs 0, 4, 8, …)"""
    _st, parts, n_rc = edges()
    own = own_receipts()
    return [{**parts["claim"], "exec_index": n_rc + r, "message_cid": ec.cid_str(parts["order"][n_rc + r]), **ec.at_index(0, own[r][0])}
            for r in range(k)]


@functools.lru_cache(maxsize=None)
def err_tipsets():
    """[(name, store, parts)]: five RC cases that do not scan clean, each alone"""
    _, failing = rc_split()
    by_name = {name: mk for name, mk, _cl in ec.RC}
    picked = failing[:: max(1, len(failing) // 5)][:5]
    out = []
    for name in picked:
        st, _claim, parts = _alone(by_name[name])
        out.append((name, st, parts))
    return out


# ---- tiles ----------------------------------------------------------------------------------------------------------------------------
TILE_ALL = (topic(210), topic(211))      # in every receipt
TILE_PLANTED = (topic(212), topic(213))  # at PLANTED only
PLANTED = (0, 1023, 1024, 2047, 2048)
TILE_SIZES = (2049, 1023, 1024, 1025)


@functools.lru_cache(maxsize=None)
def tiles():
    """→ (store, {n_receipts: receipts root}): one store, the same receipts cut to each of TILE_SIZES"""
    st = pyamt.Store()
    plain = ec.events_root(st, {0: event(9000, list(TILE_ALL), n_data=4)})
    both = ec.events_root(st, {0: event(9000, list(TILE_ALL), n_data=4), 1: event(9001, list(TILE_PLANTED), case_a=True, n_data=4)})
    made = {i: pyamt.receipt(gas=i, events_root=both if i in PLANTED else plain) for i in range(max(TILE_SIZES))}
    return st, {n: pyamt.build_amt(st, {i: made[i] for i in range(n)}, version=0) for n in TILE_SIZES}


TILE_SPECS = [(*TILE_ALL, None), (*TILE_PLANTED, None), (*TILE_ALL, 9001), (*TILE_PLANTED, 9001), (*NOBODY[0], None), (*TILE_ALL, None)]
TILE_RANGES = ((1000, 1030), (1024, 2049))


# ---- short_order ----------------------------------------------------------------------------------------------------------------------
SHORT_X_NAME, SHORT_OTHER_NAMES = 100, [101, 102, 103, 101]
SHORT_X = named_pair(SHORT_X_NAME)
SHORT_OTHERS = [named_pair(q) for q in SHORT_OTHER_NAMES]


@functools.lru_cache(maxsize=None)
def short_order():
    """→ (store, parts): 6 executed messages, receipts 0 … 7; X matches only at receipt 7, the others below 6"""
    receipts = {i: _receipt_of({0: event(9100 + i, list(SHORT_OTHERS[i % 3]))}) for i in range(6)}
    receipts[6] = _receipt_of(None)
    receipts[7] = _receipt_of({0: event(9107, list(SHORT_X)), 1: event(9108, [SHORT_X[1], SHORT_X[0]])})
    st, _claim, parts = ec.tipset(receipts=receipts, at=(0, 0), event=ec.SIB, salt=555)
    assert len(parts["order"]) == 6
    return st, parts


def bundle_cases():
    """[(name, store, parts, [(q, actor)])]: the event specs of a bundle BY NAME (named(q)) — J of them on edges(), with
    duplicates and emitter filters among them, and short_order() with X first, fourth of five, and absent"""
    st, parts, _ = edges()
    five = [(0, None), (0, 8600), (7, None), (0, None), (5, 4242)]
    forty = [(q, None) for q in range(34)] + [(0, 8500), (0, None), (7, 8601), (200, None), (3, 1), (39, None)]
    out = [(f"edges/{j}", st, parts, (five if j <= 5 else forty)[:j]) for j in (1, 2, 5, 40)]
    sst, sparts = short_order()
    others = [(q, None) for q in SHORT_OTHER_NAMES]
    x = (SHORT_X_NAME, None)
    out.append(("short_order/x_first", sst, sparts, [x] + others))
    out.append(("short_order/x_fourth", sst, sparts, others[:3] + [x] + others[3:]))
    out.append(("short_order/x_absent", sst, sparts, others))
    return out


# ---- spec sets over edges -------------------------------------------------------------------------------------------------------------
def present_pairs(blocks, receipts_root):
    """every (topic0, topic1) some log of the tipset carries, in first-seen order, with the emitters seen under it"""
    seen = {}
    r_amt = pyevents.amt_load(blocks, receipts_root, 0, pyevents.check_receipt)
    for _i, root in pyevents.amt_for_each(r_amt):
        if root is None:
            continue
        for _j, ev in pyevents.amt_for_each(pyevents.amt_load(blocks, root, 3, pyevents.check_stamped_event)):
            log = pyevents.extract_evm_log(ev[1])
            if log is not None and len(log[0]) >= 2:
                seen.setdefault((bytes(log[0][0]), bytes(log[0][1])), []).append(ev[0])
    return seen


def flip(b, at):
    b = bytearray(b)
    b[at] ^= 0x01
    return bytes(b)


def padded(specs, size):
    assert len(specs) <= size <= MAX_SPECS
    return list(specs) + [(*NOBODY[k], None) for k in range(size - len(specs))]


def colliding(slot_of, n_slots, among, want=2):
    """`want` keys of `among` that share a home slot in a table of n_slots, by asking the harness"""
    slots = slot_of(n_slots, [a + b for a, b in among])
    by = {}
    for key, s in zip(among, slots):
        by.setdefault(s, []).append(key)
        if len(by[s]) >= want:
            return by[s]
    raise AssertionError("no home-slot collision among the candidates")


CHAIN_SLOTS = 64  # the table the `one_home_slot` set of 24 specs gets
HOME_SLOTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_multi_home_slots.json")


def slot_candidates():
    """the keys the collision chains are picked from: (present pairs of edges(), pairs nobody emits)"""
    st, parts, _n_rc = edges()
    return list(present_pairs(st.blocks, parts["receipts"])), NOBODY[:600]


def recorded_slot_of(n_slots, keys):
    """slot_of from the home slots the CPU harness printed for slot_candidates(), recorded in tests/golden (the CPU test
    holds the record to the harness; the GPU test needs no compiler)"""
    with open(HOME_SLOTS) as f:
        rec = json.load(f)
    assert n_slots == rec["n_slots"] == CHAIN_SLOTS
    present, nobody = slot_candidates()
    assert len(rec["present"]) == len(present) and len(rec["nobody"]) == len(nobody)
    slot = {a + b: s for (a, b), s in zip(present + nobody, rec["present"] + rec["nobody"])}
    return [slot[k] for k in keys]


def spec_sets_over_edges(slot_of):
    """→ {name: [spec]} over edges(); slot_of(n_slots, [64-byte key]) → home slots (the CPU harness, or its record)"""
    st, parts, _n_rc = edges()
    pres = present_pairs(st.blocks, parts["receipts"])
    keys = list(pres)
    sets = {"every_present_pair": [(a, b, None) for a, b in keys]}
    a, b = pair(0)
    a2, b2 = pair(6)
    sets["traps"] = [(a, b, None), (a, flip(b, 31), None), (flip(a, 0), b, None), (b, a, None), (a, a, None), (bytes(32), bytes(32), None),
                     (a2, b2, None), (a2, flip(b2, 31), None), (flip(a2, 0), b2, None), (b2, a2, None), (*pair(9), None), (pair(9)[1], pair(9)[0], None)]
    sets["repeated_three_times"] = [(a2, b2, None), (a, b, None), (a2, b2, None), (*ec.FILTER, None), (a2, b2, None)]
    sets["emitter_filters"] = [(a, b, 8001), (a, b, 4242), (a, b, 0), (a, b, None), (a, b, 7000), (a, b, 8002), (*ec.FILTER, 1001), (*ec.FILTER, None)]
    base = [(a, b, None), (a, b, 8001), (*pair(5), None), (*ec.FILTER, None), (*ec.OTHER_FILTER, None)]
    for size in (1, 2, 63, 64, 65, 1024):
        sets[f"size_{size}"] = padded(base[:size], size)
    rng = np.random.default_rng(4711)
    mixed = padded(sets["every_present_pair"][:40] + sets["emitter_filters"] + sets["traps"], 96)
    for k in (0, 1):
        sets[f"shuffled_{k}"] = [mixed[i] for i in rng.permutation(len(mixed))]
    # a true collision chain: present pairs that share a home slot in the table this very set gets (plus absent keys on that
    # slot, which the probe must walk past or stop at)
    size = 24
    n_slots = 4
    while n_slots < 2 * size:
        n_slots <<= 1
    assert n_slots == CHAIN_SLOTS
    chain = colliding(slot_of, n_slots, keys, want=3)
    absent = colliding(slot_of, n_slots, NOBODY[:600], want=3)
    chain_set = [(x, y, None) for x, y in chain] + [(x, y, None) for x, y in absent]
    sets["one_home_slot"] = padded(chain_set, size)
    return sets


# ---- the model --------------------------------------------------------------------------------------------------------------------------
def expected_by_scans(blocks, receipts_root, specs, lo=0, hi=None):
    """pyevents.scan per spec → (status, [per-spec triples], OR of the has-maps, union of the recorded CIDs); equal specs are
    scanned once.  THE definition of the expected answer; `expected` below is the same thing computed faster, and
    tests/test_scan_multi.py holds the two to each other."""
    memo = {}
    per, has_or, rec = [], None, set()
    for sp in specs:
        if sp not in memo:
            memo[sp] = pyevents.scan(blocks, receipts_root, sp[0], sp[1], sp[2], lo, hi)
        st, has, trip, seen = memo[sp]
        if st != pyevents.TRUE:
            return st, None, None, None
        per.append(trip)
        has_or = list(has) if has_or is None else [x | y for x, y in zip(has_or, has)]
        rec |= seen
    return pyevents.TRUE, per, has_or, rec


_LISTINGS = {}


def _listing(blocks, receipts_root, lo, hi):
    """(status, map length, [(exec_index, event_index, emitter, topic0, topic1)] of the logs with ≥ 2 topics) — one walk"""
    key = (id(blocks), receipts_root, lo, hi)
    if key not in _LISTINGS:
        st, has, _trip, _rec = pyevents.scan(blocks, receipts_root, *NOBODY[0], None, lo, hi)  # (the status does not depend on the filter)
        rows = []
        if st == pyevents.TRUE:
            for i, root in pyevents.amt_for_each(pyevents.amt_load(blocks, receipts_root, 0, pyevents.check_receipt), lo, hi):
                if root is None:
                    continue
                for j, ev in pyevents.amt_for_each(pyevents.amt_load(blocks, root, 3, pyevents.check_stamped_event)):
                    log = pyevents.extract_evm_log(ev[1])
                    if log is not None and len(log[0]) >= 2:
                        rows.append((i, j, ev[0], bytes(log[0][0]), bytes(log[0][1])))
        _LISTINGS[key] = (st, len(has) if has is not None else 0, rows, {})
    return _LISTINGS[key]


def expected(blocks, receipts_root, specs, lo=0, hi=None, want_rec=True):
    """expected_by_scans from ONE walk of the tipset: a spec's list is the listed logs that carry its pair (and emitter); the
    blocks a spec records depend only on WHICH receipts match, so pyevents.scan runs once per distinct has-map"""
    st, n_has, rows, rec_of = _listing(blocks, receipts_root, lo, hi)
    if st != pyevents.TRUE:
        return st, None, None, None
    by_pair = {}
    for i, j, em, t0, t1 in rows:
        by_pair.setdefault((t0, t1), []).append((i, j, em))
    per, has_or, rec = [], [0] * n_has, set()
    for t0, t1, actor in specs:
        trip = [r for r in by_pair.get((t0, t1), ()) if actor is None or r[2] == actor]
        per.append(trip)
        has = tuple(sorted({i for i, _j, _em in trip}))
        for i in has:
            has_or[i - lo] = 1
        if want_rec and has not in rec_of:
            rec_of[has] = pyevents.scan(blocks, receipts_root, t0, t1, actor, lo, hi)[3]
        if want_rec:
            rec |= rec_of[has]
    return pyevents.TRUE, per, has_or, (rec if want_rec else None)


def merge(per_spec):
    """the order contract: J single lists → the multi list [(exec_index, event_index, emitter, spec)], ascending
    (exec_index, event_index), one event's records in ascending spec index"""
    rows = [(e, j, s, em) for s, trip in enumerate(per_spec) for e, j, em in trip]
    rows.sort(key=lambda r: (r[0], r[1], r[2]))
    return [(e, j, em, s) for e, j, s, em in rows]
