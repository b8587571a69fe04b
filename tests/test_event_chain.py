"""CPU: the event chain's named cases (tests/event_chain_cases.py) under three judges — the LITERAL status written next to
each case, tests/pyevents.py (an independent Python restatement of verify_event_proof, the execution order and the event
scan) and the C++ oracle through its string entry point (modes 0 and 1) and its packed entry point — the scan and the
generator of the oracle against pyevents on every witness, all receipt cases as ONE batch over one_tipset(), and a
structured mutator on which the oracle must equal pyevents round for round.  Measured: the file takes 10 s, 3 of them
to build the case table and 3 for the one-tipset batch."""
import collections
import re

import numpy as np
import pytest

import assumption_cases as ac
import event_chain_cases as ec
import ipc_filecoin_proofs_amd as ipcfp
import pyevents
import pystorage
from conftest import fuzz_seed

NAMES = list(ec.CASES)


def oracle_answers(oracle, blocks, claim_list, trust=None, filt=None):
    """{entry point: status list} of the oracle over one witness: the string verifier in both of its modes (0: a fresh
    execution order per proof, as the reference builds one; 1: one per tipset) and the packed entry point over
    `pack_event_proofs` of the same strings.  The oracle's packed entry point goes back to strings, so it answers a claim
    only where the packed form can be turned into strings again: `expressible` below says which — written from the
    claim's own strings, never taken from the entry point; a claim it declines is None here, and the callers assert that
    it declined exactly the inexpressible ones.  (The ENGINE's packed routes judge those claims too:
    tests/test_gpu_event_chain.py.)"""
    st = oracle.store(*ec.store_of(blocks).tables())
    pr = ec.proofs(claim_list)
    tp, ft = ec.trust_policy(trust), ec.event_filter(filt)
    out = {"strings_mode_0": st.verify_event_proofs(pr, trust=tp, filt=ft, mode=0).tolist(),
           "strings_mode_1": st.verify_event_proofs(pr, trust=tp, filt=ft, mode=1).tolist()}
    ts, cl, blob = ipcfp.pack_event_proofs(pr.arr, pr.n)
    got = st.verify_event_claims_packed(ts, cl, blob, trust=tp, filt=ft).tolist()
    st.close()
    out["packed"] = [None if g == 255 else g for g in got]
    assert [g is None for g in out["packed"]] == [not expressible(c) for c in claim_list], (out["packed"], claim_list)
    assert all(len(g) == len(claim_list) and set(g) <= pyevents.STATUSES | {None} for g in out.values()), out
    assert None not in out["strings_mode_0"] and None not in out["strings_mode_1"]
    return out


HEX = re.compile("0[xX]([0-9a-fA-F]{2})*")


def expressible(claim) -> bool:
    """every CID string parses, data is "0x" + hex, every topic "0x" + 64 hex digits, and at most 8 topics (the oracle's
    packed entry point keeps 8 strings)"""
    try:
        for s in claim["parent_tipset_cids"] + [claim["child_block_cid"], claim["message_cid"]]:
            pystorage.cid_from_string(s)
    except ValueError:
        return False
    return (len(claim["topics"]) <= 8 and HEX.fullmatch(claim["data"]) is not None
            and all(HEX.fullmatch(t) is not None and len(t) == 66 for t in claim["topics"]))


def test_pyevents_gives_every_literal():
    wrong = []
    for n, (st, cl, ex) in ec.CASES.items():
        got = pyevents.verify(st.blocks, cl, ec.META[n]["trust"], ec.META[n]["filter"])
        if got != ex:
            wrong.append((n, got, ex))
    assert not wrong, wrong


def test_the_table_covers_what_it_must():
    seen = collections.Counter(ex for _, _, ex in ec.CASES.values())
    assert set(seen) == set(range(1, 18)) | {64, 65, 66, 67, 69, 71} == set(pyevents.STATUSES), seen
    assert len(ec.CASES) >= 845 and len(ec.RC) >= 120
    # the header / TxMeta ladder with every header beyond the prologue's 8 KB stage: same literal, and the headers ARE long
    assert len(ec.LONG_HEADER_BASES) >= 42
    for base in ec.LONG_HEADER_BASES:
        st, _claim, expect = ec.CASES[base + ec.LONG_HEADERS]
        parts = ec.META[base + ec.LONG_HEADERS]["parts"]
        assert expect == ec.CASES[base][2], base
        held = [len(st.blocks[c]) for c in [parts["child"]] + parts["parents"] if c in st.blocks]
        assert all(n > 8192 or n < 16 for n in held) and sum(n > 8192 for n in held) >= len(held) - 1, (base, held)
    assert sum(1 for n, (st, _c, ex) in ec.CASES.items() if "trailer_longer_than_the_prologue_stage" in n
               and max(len(st.blocks.get(c, b"")) for c in ec.META[n]["parts"]["txmeta"]) > 8192 and ex in (65, 66)) == 3
    # every spelling of spelling_cases() is a receipt case, the good ones with the four perturbed claims beside the honest one
    for name, _ev, _em, bad in ec.spelling_cases():
        tags = {n.split(" / ")[1] for n in ec.CASES if n.startswith(f"spelling {name} / ") and n.count(" / ") == 1}
        assert ("not_a_log" in tags) if bad else {"honest", "emitter", "data_one_byte_longer"} <= tags, (name, tags)
    # filter and trust variants
    assert sum(1 for n in ec.CASES if " / filter_0_1" in n) >= 30 and sum(1 for n in ec.CASES if " / trust_" in n) >= 40
    assert {ec.CASES[n][2] for n in ec.CASES if " / filter_" in n} >= {1, 17, 12, 11, 65}


@pytest.mark.parametrize("group", range(8))
def test_oracle_gives_every_literal(oracle, group):
    wrong = []
    for name in NAMES[group::8]:
        st, claim, expect = ec.CASES[name]
        got = oracle_answers(oracle, st.blocks, [claim], ec.META[name]["trust"], ec.META[name]["filter"])
        wrong += [(name, entry, g[0], expect) for entry, g in got.items() if g[0] is not None and g[0] != expect]
    assert not wrong, wrong


def test_one_tipset_as_one_batch(oracle):
    store, parts, names, cl, want = ec.one_tipset()
    assert len(cl) > 500 and [pyevents.verify(store.blocks, c) for c in cl] == want
    for entry, g in oracle_answers(oracle, store.blocks, cl).items():
        assert not [(n, x, w) for n, x, w in zip(names, g, want) if x is not None and x != w], entry
    # the rule that gives the literals under a filter (event_chain_cases.under_filter) is what pyevents computes
    for f in (ec.FILTER, ec.OTHER_FILTER):
        assert [ec.under_filter(x, c, f) for x, c in zip(want, cl)] == [pyevents.verify(store.blocks, c, None, f) for c in cl]
    # under a filter and a trust window the expected answers are pyevents'
    for trust, filt in ((ec.TRUST["both_inside"][0], ec.FILTER),):
        want2 = [pyevents.verify(store.blocks, c, trust, filt) for c in cl]
        for entry, g in oracle_answers(oracle, store.blocks, cl, trust, filt).items():
            assert not [(n, x, w) for n, x, w in zip(names, g, want2) if x is not None and x != w], (entry, trust, filt)


def scan_witnesses():
    """(name, blocks, parts) of every witness with a scan answer: the witness-level cases (one per distinct store) and
    one_tipset()"""
    seen = set()
    for n in NAMES:
        if " / " in n and "rc" not in ec.META[n]:
            continue  # (a filter / trust variant shares its witness with the case it varies)
        key = ec.META[n].get("rc", n)
        if key not in seen:
            seen.add(key)
            yield n, ec.CASES[n][0].blocks, ec.META[n]["parts"]
    store, parts, *_ = ec.one_tipset()
    yield "one_tipset", store.blocks, parts


FILTERS = ((ec.FILTER, None), (ec.OTHER_FILTER, None), (ec.FILTER, 1001), (ec.FILTER, 4000))


def triples(trip):
    return [tuple(int(x) for x in row) for row in trip]


def test_oracle_scan_and_generate_equal_pyevents(oracle):
    n_ok = n_err = 0
    for name, blocks, parts in scan_witnesses():
        st = oracle.store(*ec.store_of(blocks).tables())
        for (t0, t1), actor in FILTERS:
            want = pyevents.scan(blocks, parts["receipts"], t0, t1, actor)
            os_, ohas, otrip, otouched = st.scan_events(parts["receipts"], t0, t1, actor=actor, cap_receipts=1 << 10, cap_matches=1 << 12, cap_touched=1 << 12)
            assert os_ == want[0], (name, actor, os_, want[0])
            if os_ == 1:
                n_ok += 1
                assert ohas.tolist() == want[1] and triples(otrip) == want[2], (name, actor)
                assert {bytes(c[:38]) for c in otouched} == want[3], (name, actor)
            else:
                n_err += 1
            gw = pyevents.generate(blocks, parts["parents"], parts["child"], t0, t1, actor)
            gs, gtrip, gmsg, gwit = st.generate_event_proof(parts["parents"], parts["child"], t0, t1, actor=actor, cap_proofs=1 << 12, cap_witness=1 << 12)
            assert gs == gw[0], (name, actor, gs, gw[0])
            if gs == 1:
                assert [(*t, bytes(m[:38])) for t, m in zip(triples(gtrip), gmsg)] == gw[1], (name, actor)
                assert {bytes(c[:38]) for c in gwit} == gw[2], (name, actor)
        st.close()
    assert n_ok > 400 and n_err > 100
    # the one scan answer written down by hand
    st_, cl, _ = ec.CASES["base_true"]
    for (filt, actor), want in ec.META["base_true"]["scan"].items():
        got = pyevents.scan(st_.blocks, ec.META["base_true"]["parts"]["receipts"], filt[0], filt[1], actor)
        assert got[0] == 1 and got[2] == want and got[1] == [1 if any(t[0] == i for t in want) else 0 for i in range(6)]


@pytest.mark.parametrize("name", sorted(ac.EVENT_CASES))
def test_event_carried_assumption(oracle, name):
    st, claim, expect = ac.EVENT_CASES[name]()
    assert pyevents.verify(st.blocks, claim) == expect
    for entry, got in oracle_answers(oracle, st.blocks, [claim]).items():
        assert got[0] == expect, (name, entry, got[0])  # (every string of these claims is canonical: packed answers too)


ROUNDS = 350


def test_structured_mutator_oracle_equals_pyevents(oracle):
    """350 rounds of event_chain_cases.mutated_tipset.  The conditions on the mutator are counted on pyevents' answers alone:
    at least 10 distinct statuses, at least a quarter of the rounds reach verify_receipt_and_event, at most half end in a
    missing block or a decode error."""
    rng = np.random.default_rng(fuzz_seed(8100))
    seen = collections.Counter()
    step4 = 0
    for k in range(ROUNDS):
        blocks, claim, trust, filt = ec.mutated_tipset(rng)
        want = pyevents.verify(blocks, claim, trust, filt)
        seen[want] += 1
        step4 += pyevents.reaches_step_4(blocks, claim, trust)
        for entry, got in oracle_answers(oracle, blocks, [claim], trust, filt).items():
            assert got[0] in (want, None), (k, entry, got[0], want, claim)
    assert len(seen) >= 10, seen
    assert step4 >= ROUNDS // 4, (step4, seen)
    assert seen[65] + seen[66] <= ROUNDS // 2, seen
