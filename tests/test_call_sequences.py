"""The call sequences of tests/call_sequences.py, without a GPU: their coverage is a CONDITION (asserted here on the
generated sequence, never relaxed: a sequence that misses an adjacency is extended), their expected answers are not
trivial, and the reference that judges the engine in tests/test_gpu_call_sequences.py is itself stateless — the whole
sequence through one long-lived oracle store per witness equals the memoised fresh-store answers, op by op."""
import pytest

import call_sequences as cs
import ipc_filecoin_proofs_amd as ipcfp


@pytest.fixture(scope="module")
def ops():
    return cs.sequence()


@pytest.fixture(scope="module")
def expected(ops):
    """[(op, fresh-store answer, long-lived answer)] of the whole sequence"""
    model = cs.Model()
    held = cs.LongLived(model)
    out = []
    try:
        for op in ops:
            model.lifts(op)
            out.append((op, model.expect(op), held.answer(op)))
            model.apply(op)
    finally:
        held.close()
    assert all(v == -1 for v in model.tuning.values()), model.tuning
    return out


def test_the_sequence_is_a_function_of_the_seed(ops):
    assert cs.sequence() == ops and cs.sequence(cs.fuzz_seed(cs.BASE_SEED) + 1) != ops
    assert eval(repr(ops[:50])) == ops[:50]  # a literal


def test_every_ordered_pair_of_op_kinds_is_adjacent_on_the_same_witness(ops):
    pairs, *_ = cs.adjacencies(ops)
    for wit, kinds in cs.KINDS.items():
        missing = [(a, b) for a in kinds for b in kinds if (wit, a, b) not in pairs]
        assert not missing, (wit, missing[:10])


def test_every_op_kind_follows_another_witness_a_failing_call_and_each_state_change(ops):
    _, after_other, after = cs.adjacencies(ops)
    every = {k for ks in cs.KINDS.values() for k in ks}
    assert every == set(cs.SYNTH_KINDS) and len(every) == 26
    assert every <= after_other, every - after_other
    for s in cs.AFTER + cs.FAILING_KINDS:
        assert every <= {k for p, k in after if p == s}, (s, every - {k for p, k in after if p == s})
    assert not cs.coverage_gaps(ops)
    # and directly: positions i-1, i of the list itself, same witness
    for s in cs.AFTER + cs.FAILING_KINDS:
        seen = {ops[i][0] for i in range(1, len(ops)) if ops[i - 1][0] == s and ops[i - 1][1] == ops[i][1]}
        assert every <= seen, (s, every - seen)


def test_the_first_burst_grows_the_tables_between_two_queued_calls(ops):
    """Burst 0 puts the context's HAMT node tables at stake: BOTH queued calls take a route that uses them under the tuning
    in force, nothing before it has sized them, and the second call's witness needs more than the first call's tables
    hold with their slack (grow() of host/primitives.cpp allocates need + need / 4)."""
    assert ops[0] == ("burst", "A", (0,)) and [op for op in ops if op[0] == "burst" and op[2] == (0,)] == [ops[0]]
    model = cs.Model()
    assert all(v == -1 for v in model.tuning.values())  # the sequence's first op: default tuning, no earlier call
    parts = cs.burst_parts(ops[0])
    assert [(p[0], p[1]) for p in parts] == [("hamt_get", "A"), ("hamt_get", "B")]
    base = cs.witnesses(model.seed)
    keys = [len(base[p[1]].keys[p[2][2]]) for p in parts]
    blocks = [len(base[p[1]].cids) for p in parts]
    assert keys[0] == 1024 < keys[1]
    assert [cs.hamt_route(model.tuning, k, n) for k, n in zip(keys, blocks)] == ["levels", "levels"]
    assert blocks[1] > blocks[0] + blocks[0] // 4
    # later on, tuning words force the table and the level route for small batches too, and the walker alone
    routes = set()
    for op in ops:
        if op[0] == "hamt_get":
            w = model.w[op[1]]
            routes.add(cs.hamt_route(model.tuning, len(w.base.keys[op[2][2]]), len(w.cids), (5, 4, 8)[op[2][1]],
                                     ("actor_state", "any", "vec_u8")[op[2][0]]))
        model.lifts(op)
        model.apply(op)
    assert routes == {"table", "levels", "walker"}
    used = {p[0] for op in ops if op[0] == "burst" for p in cs.burst_parts(op)}
    assert used == {"hamt_get", "verify_event_claims", "scan_events", "verify_and_scan_device", "verify_storage_columns", "generate_storage_claims"}
    assert any(len({p[1] for p in cs.burst_parts(op)}) == 2 for op in ops if op[0] == "burst")


def test_a_receipt_range_stays_on_for_the_ops_that_follow_it(ops):
    """every kind a range stays on for runs at least once under a range that is not the full one"""
    model = cs.Model()
    under = set()
    for op in ops:
        model.lifts(op)
        if op[0] == "burst":  # a burst's parts run under the ranges their witnesses have
            under |= {"burst:" + p[0] for p in cs.burst_parts(op) if model.w[p[1]].range != cs.FULL}
        if any(model.w[w].range != cs.FULL for w in cs.witnesses_of(op)):
            under.add(op[0])
        model.apply(op)
    assert set(cs.RANGED) - {"set_receipt_range"} <= under | {"set_receipt_range"}, set(cs.RANGED) - under
    assert all(op[2] != (0,) for op in ops if op[0] == "set_receipt_range")
    assert {"burst:scan_events", "burst:verify_event_claims", "burst:verify_and_scan_device", "burst:hamt_get"} <= under, under


def test_chunks_are_short(ops):
    parts = cs.chunks(ops)
    assert all(len(c) <= cs.CHUNK for _, c in parts) and sum(len(c) for _, c in parts) == len(ops)
    assert [i for i, _ in parts] == list(range(0, len(ops), cs.CHUNK))


def test_the_expected_answers_are_not_trivial(expected):
    statuses = {k: set() for k in cs.VERIFY_KINDS}
    matches = {}
    codes = {k: set() for k in cs.FAILING_KINDS}
    for op, want, _ in expected:
        kind, wit, args = op
        if kind in cs.VERIFY_KINDS:
            st = want[0] if isinstance(want, tuple) else want
            statuses[kind] |= set(st)
        elif kind == "scan_events" and want[0] == 1:
            matches[(wit, args[0])] = max(matches.get((wit, args[0]), 0), len(want[2]))
        elif kind == "scan_events" and args[3] == 2:
            assert want == (cs.ERR_MISSING,), op
        elif kind in cs.FAILING_KINDS and wit != "C":
            codes[kind].add(want[1] if want[0] in ("rc", "overflow") else None)
        elif kind == "bad_compact_group":
            assert want[cs.bad_group(cs.Model().w[wit])] == cs.ERR_BAD_CLAIM
    assert all(len(s) >= 5 for s in statuses.values()), {k: sorted(s) for k, s in statuses.items()}
    # every witness's own and other filter have matches, in the tipset and in the sequence's own scans; the third has none
    fresh = cs.Model()
    for wit in "ABC":
        for f in (0, 1):
            assert len(fresh.expect(("scan_events", wit, (f, 0, 1, 0)))[2]) > 0 and matches[(wit, f)] > 0, (wit, f, matches)
        assert matches[(wit, 2)] == 0
    assert codes["bad_run_table"] == codes["bad_bundle_block_id"] == {-1} and codes["short_scan_cap"] == {1}, codes
    # the status of the claim that names no group, among answers that are otherwise the verifier's
    bad = [want for op, want, _ in expected if op[0] == "bad_compact_group"]
    assert bad and all(ipcfp.ST.ERR_BAD_CLAIM in w for w in bad) and len(set(bad[0])) >= 4


def test_a_replaced_block_changes_later_answers(expected):
    for wit in "ABC":
        by_key = {}
        replaced = False
        for op, want, _ in expected:
            if op[1] != wit:
                continue
            replaced |= op[0] == "put_replace"
            if op[0] in ("scan_events", "verify_event_claims", "verify_cids", "verify_storage_proofs", "verify_storage_columns", "generate_storage_claims") and replaced:
                if op[0] == "scan_events":  # (whether the touched set was asked for does not make two scans differ)
                    op, want = (op[0], op[1], op[2][:2] + op[2][3:]), want[:3]
                by_key.setdefault((op[0], op[2] if op[0] != "has_get" else ()), set()).add(repr(want))
        assert any(len(v) > 1 for k, v in by_key.items() if k[0] in ("scan_events", "verify_event_claims")), wit
        assert len(by_key[("verify_cids", ())]) > 1, wit
        if wit != "C":  # the storage side reads replaced blocks too: a contract's actor state
            for kind in ("verify_storage_proofs", "verify_storage_columns", "generate_storage_claims"):
                assert any(len(v) > 1 for k, v in by_key.items() if k[0] == kind), (wit, kind)


def test_the_reference_is_stateless(expected):
    """one long-lived store per witness, every op of the sequence in order, against a fresh store per answer"""
    wrong = [(i, op) for i, (op, fresh, held) in enumerate(expected) if fresh != held]
    assert not wrong, wrong[:10]
    assert sum(1 for op, *_ in expected if op[1] != "C" and op[0] in cs.QUERY_KINDS) >= 2 * len(cs.QUERY_KINDS) * len(cs.SYNTH_KINDS)
