"""GPU: the storage chain's named cases (tests/storage_chain_cases.py) through EVERY route of the engine — the string ABI,
packed rows and the column form, each of the latter with the one-lane kernel (`hamt_table` = 0) and with the node table
(= 1) — against the literal status of each case and against tests/pystorage.py.  One witness per case with a batch of
one; all cases merged into one witness as one batch, in table order and shuffled with repeats (runs of every kind and
the table's punts side by side in one launch, run lengths 1-5), with and without a trust window; one state tree big
enough for the 32-lane outline; and the structured mutator."""
import numpy as np
import pytest

import assumption_cases as ac
import ipc_filecoin_proofs_amd as ipcfp
import pystorage
import storage_chain_cases as sc
from conftest import fuzz_seed

pytestmark = pytest.mark.gpu

ROUTES = ("strings", "rows_lane", "rows_table", "columns_lane", "columns_table")
STATUSES = {1, 3, 18, 19, 20, 21, 65, 66, 68, 69, 70}  # what verify_storage_proof can answer (include/ipcfp.h)


@pytest.fixture()
def routed(engine):
    def use(table):
        engine.set_tuning("hamt_table", table)
    yield use
    engine.set_tuning("hamt_levels", -1)
    engine.set_tuning("hamt_table", -1)
    engine.set_tuning("hamt_coop", -1)


def answers(w, use, claim_list, trust=None):
    """{route: [status]} of one batch over one witness"""
    pr = sc.proofs(claim_list)
    tp = sc.trust_policy(trust)
    use(-1)
    out = {"strings": w.verify_storage_proofs(pr.arr, pr.n, trust=tp).tolist()}
    rows = ipcfp.pack_storage_proofs(pr.arr, pr.n)
    with ipcfp.compact_storage_claims(rows) as cols:
        for table, tag in ((0, "lane"), (1, "table")):
            use(table)
            out["rows_" + tag] = w.verify_storage_claims(rows, trust=tp).tolist()
            out["columns_" + tag] = w.verify_storage_columns(cols, trust=tp).tolist()
    # every route answers every claim: none is skipped, none returns a placeholder
    assert set(out) == set(ROUTES) and all(len(st) == len(claim_list) and set(st) <= STATUSES for st in out.values()), out
    return out


def wrong_answers(got, names, want):
    return [(name, route, st[i], want[i]) for route, st in got.items() for i, name in enumerate(names) if st[i] != want[i]]


def test_every_case_in_a_witness_of_its_own(engine, routed):
    wrong = []
    for name, (store, claim, expect) in sc.CASES.items():
        with engine.witness(*store.tables()) as w:
            wrong += wrong_answers(answers(w, routed, [claim], sc.META[name]["trust"]), [name], [expect])
    assert not wrong, wrong


def test_storage_carried_assumptions(engine, routed):
    wrong = []
    for name in sorted(ac.STORAGE_CASES):
        store, claim, expect = ac.STORAGE_CASES[name]()
        with engine.witness(*store.tables()) as w:
            wrong += wrong_answers(answers(w, routed, [claim]), [name], [expect])
    assert not wrong, wrong


@pytest.fixture(scope="module")
def merged():
    store, names, apart = sc.merged()
    # kept apart (each needs a CID absent that another case holds; they run in test_every_case_in_a_witness_of_its_own):
    # b1_inner_root_absent, c_root_absent, two_bad_slot_hex_and_storage_root_absent, two_storage_root_absent_and_wrong_value
    assert len(apart) <= 6, apart
    return store, names


def test_all_cases_in_one_witness_in_table_order(engine, routed, merged):
    store, names = merged
    plain = [n for n in names if sc.META[n]["trust"] is None]
    with engine.witness(*store.tables()) as w:
        got = answers(w, routed, [sc.CASES[n][1] for n in plain])
    wrong = wrong_answers(got, plain, [sc.CASES[n][2] for n in plain])
    assert not wrong, wrong


def test_all_cases_in_one_witness_shuffled_with_repeats(engine, routed, merged):
    store, names = merged
    rng = np.random.default_rng(fuzz_seed(7200))
    plain = [n for n in names if sc.META[n]["trust"] is None]
    order = [plain[i] for i in rng.permutation(len(plain)) for _ in range(int(rng.integers(1, 6)))]
    with engine.witness(*store.tables()) as w:
        got = answers(w, routed, [sc.CASES[n][1] for n in order])
    wrong = wrong_answers(got, order, [sc.CASES[n][2] for n in order])
    assert not wrong, wrong[:20]


def test_all_cases_in_one_witness_under_a_trust_window(engine, routed, merged):
    """Policy kind 1 with an epoch window that excludes some cases; the expected answers are pystorage's."""
    store, names = merged
    rng = np.random.default_rng(fuzz_seed(7201))
    claims = []
    for n in names:
        c = dict(sc.CASES[n][1])
        if sc.META[n]["trust"] is None and rng.integers(3) == 0:
            c["child_epoch"] = int(rng.choice([sc.TRUST_WINDOW[1] - 1, sc.TRUST_WINDOW[2] + 1, -5]))
        claims.append(c)
    want = [pystorage.verify(store.blocks, c, sc.TRUST_WINDOW) for c in claims]
    assert want.count(3) > 50 and len(set(want)) >= 10
    with engine.witness(*store.tables()) as w:
        got = answers(w, routed, claims, sc.TRUST_WINDOW)
    wrong = wrong_answers(got, names, want)
    assert not wrong, wrong[:20]


def test_state_tree_wide_enough_for_the_outline(engine, routed):
    """3000 actors: the actors HAMT's lower nodes are buckets of ActorStates, several KB each — at least
    kHamtOutlineMinLen (2048) bytes, so the node table decodes them with the 32-lane outline."""
    C5 = sc.layout("C", sc.PAIRS)
    chains = {
        "valid": (1, sc.chain(C5, sc.S[2], sc.VAL[2], salt=1, n_actors=3000)),
        "wrong_value": (21, sc.chain(C5, sc.S[2], sc.VAL[3], salt=2, n_actors=3000)),
        "actor_not_found": (68, sc.chain(C5, sc.S[2], sc.VAL[2], salt=3, n_actors=3000, edit={"actor_id": 999})),
        "a_malformed_actor_in_the_claimed_actors_node": (66, sc.chain(C5, sc.S[2], sc.VAL[2], salt=4, n_actors=3000, actor=lambda f: sc.array(f[:4]))),
        "other_actor_of_the_tree": (19, sc.chain(C5, sc.S[2], sc.VAL[2], salt=5, n_actors=3000, edit={"actor_id": 2500})),
    }
    wrong = []
    for name, (expect, (store, claim, parts)) in chains.items():
        assert max(len(b) for b in store.blocks.values()) >= 2048
        assert pystorage.verify(store.blocks, claim) == expect
        with engine.witness(*store.tables()) as w:
            wrong += wrong_answers(answers(w, routed, [claim] * 3), [name] * 3, [expect] * 3)
    assert not wrong, wrong


ROUNDS = 150


def test_structured_mutator_engine_equals_pystorage(engine, routed):
    """150 rounds of storage_chain_cases.mutated_chain (tests/test_storage_chain.py runs 350 on the CPU; each round here is
    a witness upload and five launches), from a seed of its own; every route."""
    rng = np.random.default_rng(fuzz_seed(7300))
    wrong = []
    for k in range(ROUNDS):
        blocks, claim, trust = sc.mutated_chain(rng)
        want = pystorage.verify(blocks, claim, trust)
        with engine.witness(*sc.store_of(blocks).tables()) as w:
            wrong += wrong_answers(answers(w, routed, [claim], trust), [f"round {k}: {claim}"], [want])
    assert not wrong, wrong[:10]
