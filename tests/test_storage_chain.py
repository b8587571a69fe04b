"""CPU: the storage chain's named cases (tests/storage_chain_cases.py) under three judges — the LITERAL status written
next to each case, tests/pystorage.py (an independent Python restatement of verify_storage_proof) and the C++ oracle —
and a structured mutator on which the oracle must equal pystorage round for round."""
import collections
import re

import numpy as np
import pytest

import assumption_cases as ac
import ipc_filecoin_proofs_amd as ipcfp
import pystorage
import storage_chain_cases as sc
from conftest import fuzz_seed

NAMES = list(sc.CASES)


def oracle_answers(oracle, blocks, claim_list, trust=None):
    """{entry point: status list} of the oracle over one witness: the string verifier in both of its modes (0: a fresh
    store per proof, as the reference loads one; 1: one shared store) and the packed entry point — which can express a
    claim only where every string is canonical (flags == 63); a claim it declines is None here, and WHICH claims it may
    decline is asserted by the callers (storage_chain_cases.PACKED_MAY_DECLINE), never taken on trust.  The ENGINE's row
    and column routes do judge those claims (tests/test_gpu_storage_chain.py): for them these routes are held to the
    literal and to pystorage only, the string ABI to all three judges."""
    st = oracle.store(*sc.store_of(blocks).tables())
    pr = sc.proofs(claim_list)
    tp = sc.trust_policy(trust)
    out = {"strings_mode_0": st.verify_storage_proofs(pr, trust=tp, mode=0).tolist(),
           "strings_mode_1": st.verify_storage_proofs(pr, trust=tp, mode=1).tolist()}
    packed = ipcfp.pack_storage_proofs(pr.arr, pr.n)
    got = st.verify_storage_claims_packed(packed, trust=tp)
    out["packed"] = [int(g) if f == 63 else None for g, f in zip(got, packed["flags"])]
    st.close()
    return out


def test_pystorage_gives_every_literal():
    wrong = [(n, pystorage.verify(st.blocks, cl, sc.META[n]["trust"]), ex) for n, (st, cl, ex) in sc.CASES.items()
             if pystorage.verify(st.blocks, cl, sc.META[n]["trust"]) != ex]
    assert not wrong, wrong


def test_the_table_covers_what_it_must():
    seen = collections.Counter(ex for _, _, ex in sc.CASES.values())
    assert {1, 3, 18, 19, 20, 21, 65, 66, 68, 69} <= set(seen), seen
    have = {(m["layout"], m["slot"]) for n, m in sc.META.items() if sc.CASES[n][2] == 1 and m["layout"]}
    assert have == {(L, k) for L in sc.LAYOUTS for k in ("present", "absent", "zero")}
    # a "zero" case stores zeros (it is not an absent slot), a "present" case claims a non-zero value
    for n, m in sc.META.items():
        if m["slot"] == "zero":
            assert sc.CASES[n][1]["value"] == "0x" + "00" * 32 and sc.CASES[n][1]["slot"] == sc.hex0x(sc.S[1])
        if m["slot"] == "present":
            assert sc.CASES[n][1]["value"] != "0x" + "00" * 32
    assert len(sc.CASES) >= 250
    # no case is skipped on any route: the only answers a route withholds are the packed row's, for exactly the cases named
    # in PACKED_MAY_DECLINE, each of which edits a claim string away from its canonical spelling
    assert sc.PACKED_MAY_DECLINE <= set(sc.CASES) and len(sc.PACKED_MAY_DECLINE) <= 20
    assert all(not canonical(sc.CASES[n][1]) for n in sc.PACKED_MAY_DECLINE)


def canonical(claim):
    """every CID string is its own `to_string()`, slot and value are "0x" and 64 lower-case hex digits"""
    try:
        cids = all(pystorage.cid_to_string(pystorage.cid_from_string(claim[f])) == claim[f]
                   for f in ("child_block_cid", "parent_state_root", "actor_state_cid", "storage_root"))
    except ValueError:
        return False
    return cids and all(re.fullmatch("0x[0-9a-f]{64}", claim[f]) for f in ("slot", "value"))


def declined(answers):
    """the positions at which the packed entry point gave no answer; every string entry point must answer everywhere"""
    assert None not in answers["strings_mode_0"] and None not in answers["strings_mode_1"]
    return {i for i, g in enumerate(answers["packed"]) if g is None}


@pytest.mark.parametrize("group", range(8))
def test_oracle_gives_every_literal(oracle, group):
    wrong = []
    for name in NAMES[group::8]:
        st, claim, expect = sc.CASES[name]
        got = oracle_answers(oracle, st.blocks, [claim], sc.META[name]["trust"])
        if bool(declined(got)) != (name in sc.PACKED_MAY_DECLINE):
            wrong.append((name, "packed", got["packed"][0], "declined" if name in sc.PACKED_MAY_DECLINE else expect))
        wrong += [(name, entry, g[0], expect) for entry, g in got.items() if g[0] is not None and g[0] != expect]
    assert not wrong, wrong


def test_merged_witness_changes_no_answer(oracle):
    """All cases in one witness (the arrangement the GPU test launches as one batch): pystorage still gives every literal
    — the merge keeps apart what it must — and the oracle agrees claim for claim, with and without a trust window."""
    store, names, apart = sc.merged()
    assert len(names) > 0.9 * len(sc.CASES), apart
    plain = [n for n in names if sc.META[n]["trust"] is None]
    cl = [sc.CASES[n][1] for n in plain]
    want = [pystorage.verify(store.blocks, c) for c in cl]
    assert want == [sc.CASES[n][2] for n in plain]
    got = oracle_answers(oracle, store.blocks, cl)
    assert {plain[i] for i in declined(got)} == sc.PACKED_MAY_DECLINE & set(plain)
    for entry, g in got.items():
        assert [x for x in g if x is not None] == [w for x, w in zip(g, want) if x is not None], entry
    cl = [sc.CASES[n][1] for n in names]
    want = [pystorage.verify(store.blocks, c, sc.TRUST_WINDOW) for c in cl]
    assert 3 in want
    got = oracle_answers(oracle, store.blocks, cl, sc.TRUST_WINDOW)
    assert {names[i] for i in declined(got)} == sc.PACKED_MAY_DECLINE & set(names)
    for entry, g in got.items():
        assert [x for x in g if x is not None] == [w for x, w in zip(g, want) if x is not None], entry


@pytest.mark.parametrize("name", sorted(ac.STORAGE_CASES))
def test_storage_carried_assumption(oracle, name):
    st, claim, expect = ac.STORAGE_CASES[name]()
    assert pystorage.verify(st.blocks, claim) == expect
    for entry, got in oracle_answers(oracle, st.blocks, [claim]).items():
        assert got[0] == expect, (name, entry, got[0])  # (every string of these claims is canonical: packed answers too)


ROUNDS = 350


def test_structured_mutator_oracle_equals_pystorage(oracle):
    """350 rounds of storage_chain_cases.mutated_chain — a valid chain of a random layout with one or two FIELDS re-spelled
    (wrong major type, length ± 1, null, non-minimal head, swapped link) or a block dropped, nothing re-hashed.
    Measured on the CPU box: 350 rounds take 0.5 s, tests/test_oracle_py_property.py 0.4 s."""
    rng = np.random.default_rng(fuzz_seed(7100))
    seen = collections.Counter()
    for k in range(ROUNDS):
        blocks, claim, trust = sc.mutated_chain(rng)
        want = pystorage.verify(blocks, claim, trust)
        seen[want] += 1
        for entry, got in oracle_answers(oracle, blocks, [claim], trust).items():
            assert got[0] == want, (k, entry, got[0], want, claim)  # (the mutator edits blocks, never a claim string)
    # on the reference's answers alone: the menu reaches the error paths and every FALSE of the storage verifier
    assert sum(c for s, c in seen.items() if s >= 64) >= ROUNDS // 4, seen
    assert len({s for s in seen if s in (3, 18, 19, 20, 21)}) >= 4, seen
