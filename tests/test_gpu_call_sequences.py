"""GPU: a resident context is held to call-order independence.  One context of this module's own and three witnesses kept
resident (tests/call_sequences.py: two synthetic tipsets of different block counts, and two hand-built tipset pairs in one
witness) go through the seeded sequence of ABI calls — per witness an Eulerian circuit over its op kinds, every ordered
pair of kinds once, the three circuits interleaved; verifiers in every transport form, scans, walks, generators, the
Blockstore face, index rebuilds, blocks added and REPLACED, receipt ranges set, kept on and lifted, witnesses closed and made anew,
tuning words moved, calls that fail, and bursts of device entry points queued back to back before one synchronisation.
Every answer — status bytes, has-match maps, match triples, touched sets as CID sets, located bytes, generated columns —
must equal the model's, which asks a fresh oracle store (or tests/pyevents.py) and never the engine
(tests/test_call_sequences.py holds the sequence's coverage and the reference's own statelessness).

One test per chunk of the sequence, in order: the state carries from chunk to chunk, and a chunk run alone starts from fresh
witnesses of the model's blocks at its first op — valid either way, because the expectations are stateless.  IPCFP_FUZZ_SEED
moves the two synthetic tipsets and the sequence.  Measured on an MI355X: no chunk takes more than 0.5 s
(the first one's fixtures — the context, the three witnesses — 2 s), the file 8 s."""
import numpy as np
import pytest

import call_sequences as cs
import ipc_filecoin_proofs_amd as ipcfp

pytestmark = pytest.mark.gpu

OPS = cs.sequence()
CHUNKS = cs.chunks(OPS)


@pytest.fixture(scope="module")
def run():
    """the module's own context (a failure then reproduces whatever ran before in the session) and its witnesses"""
    import torch

    torch.cuda.init()
    eng = ipcfp.Engine(0)
    r = cs.Runner(eng, cs.Model())
    yield r
    r.close()
    eng.close()


def stand_at(run, start):
    """the engine and the model at op `start` of the sequence: carried over from the chunk before, or made anew"""
    if run.at != start:
        run.model.reset()
        for op in OPS[:start]:
            run.model.lifts(op)
            run.model.apply(op)
        run.adopt()
    run.at = None  # (stays None when the chunk ends in an exception: the next one starts anew)


def describe(start, i, op, got, want):
    def short(x):
        s = repr(x)
        return s if len(s) < 400 else s[:400] + "…"

    if isinstance(got, tuple) and isinstance(want, tuple) and len(got) == len(want):
        diff = [(k, short(g), short(w)) for k, (g, w) in enumerate(zip(got, want)) if g != w]
    elif isinstance(got, bytes) and isinstance(want, bytes) and len(got) == len(want):
        at = [k for k in range(len(got)) if got[k] != want[k]]
        diff = [("positions", at[:16], "got", [got[k] for k in at[:16]], "want", [want[k] for k in at[:16]])]
    else:
        diff = [(short(got), short(want))]
    return (f"seed {cs.Model().seed}, op {i} (its chunk starts at {start}): {op} differs from the model in {diff}; "
            f"call_sequences.replay({OPS[max(0, i - 7): i + 1]!r}, seed={cs.Model().seed})")


@pytest.mark.parametrize("start", [s for s, _ in CHUNKS])
def test_chunk(run, start):
    stand_at(run, start)
    wrong = []
    for i, op in enumerate(OPS[start: start + cs.CHUNK], start):
        for name in run.model.lifts(op):
            run.w[name].set_receipt_range(*cs.FULL)
        want = run.model.expect(op)
        got = run.run(op)
        run.model.apply(op)
        if got != want:
            wrong.append(describe(start, i, op, got, want))
    run.at = start + len(OPS[start: start + cs.CHUNK])
    assert not wrong, (len(wrong), wrong[:3])


def test_afterwards_a_fresh_witness_on_the_session_engine_and_default_tuning(engine, run):
    """What the sequences leave behind.  The session's context — which the same process shares the device with — answers
    a scan and a verify on a fresh witness.  That every tuning word is back at -1 is a property of the SEQUENCE, stated
    here on its last ops (one set_tuning(key, -1) per key; the ABI has no getter to read the words back from the engine);
    the fixture's teardown sets them once more."""
    assert [op for op in OPS[-len(cs.TUNING):]] == [("set_tuning", "A", (k, 0)) for k in range(len(cs.TUNING))]
    assert all(values[0] == -1 for _, values in cs.TUNING)
    fresh = cs.Model()
    session = cs.Runner(engine, fresh)
    try:
        session.open("A")
        for op in (("scan_events", "A", (0, 1, 1, 0)), ("verify_event_claims", "A", (1, 0))):
            want = fresh.expect(op)
            assert session.run(op) == want, op
            assert len(want[2]) > 0 if op[0] == "scan_events" else len(set(want)) >= 5
    finally:
        session.close()


# ---- regressions: the shortest sequence that showed each defect the sequences found, as a literal ---------------------------------
# (none found so far: DESIGN.md §3, "What stays between calls, and what holds it")
def test_replay_accepts_a_literal(run):
    """`replay` is what a failure message hands over: a literal sequence from fresh witnesses, here on this module's context"""
    ops = [("scan_events", "A", (0, 0, 1, 0)), ("put_replace", "A", (2,)), ("verify_event_claims", "A", (0, 0)),
           ("set_receipt_range", "A", (2,)), ("scan_events", "A", (0, 0, 0, 0)), ("bad_bundle_block_id", "A", ()),
           ("burst", "A", (0,)), ("has_get", "C", (5,))]
    assert cs.replay(ops, engine=run.eng) == []
    run.at = None  # (replay left the context's tuning at -1 and closed its own witnesses; this module's are as they were)
    run.adopt()
    assert np.array_equal(run.w["A"].verify_cids()[0], np.frombuffer(run.model.expect(("verify_cids", "A", ()))[0], dtype=np.uint8))
