"""GPU: ipcfp_bundle_write_packed_json / ipcfp_bundle_write_generated_json — the claims head of a bundle's JSON text written
by kernels/claim_text.hip out of packed claims resident in HBM, ahead of the blocks.  The expected text comes from
tests/bundle_packed_cases.py and tests/bundle_ref.py (Python), never from the engine; where the engine's host route
(_proofs + ipcfp_bundle_write_json) is compared, it is a second judge."""
import numpy as np
import pytest
import torch

from conftest import fuzz_seed

import bundle_packed_cases as cases
import bundle_ref
import event_gen_chain_cases as gc
import ipc_filecoin_proofs_amd as ipcfp
from tools.synth import Tipset

pytestmark = pytest.mark.gpu

CHAIN_PREFIX = bytes.fromhex("0171a0e40220")


def dev(a):
    a = np.ascontiguousarray(a)
    if a.size == 0:
        return None
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def ptr(t):
    return 0 if t is None else t.data_ptr()


class Resident:
    """a case's packed inputs in HBM"""

    def __init__(self, case):
        self.case = case
        self.t = [dev(case.runs), dev(case.slot), dev(case.value), dev(case.cflags), dev(case.claims), dev(case.blob)]

    def write(self, engine, w, block_ids=(), cap=None):
        c, t = self.case, self.t
        ids = None if block_ids is None else np.asarray(block_ids, dtype=np.uint32)
        return engine.bundle_write_packed_json(w, ptr(t[0]), len(c.runs), ptr(t[1]), ptr(t[2]), ptr(t[3]), c.n_storage, c.tipsets,
                                               ptr(t[4]), c.n_events, ptr(t[5]), c.blob_len, block_ids=ids, cap=cap)


@pytest.fixture(scope="module")
def blocks():
    rng = np.random.default_rng(fuzz_seed(0xB70))
    out = []
    for k in range(100):
        d = rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes()
        out.append((CHAIN_PREFIX + rng.integers(0, 256, 32, dtype=np.uint8).tobytes(), d))
    out.append((b"\xff\x2a" + bytes(36), b"folded"))  # a block whose CID the witness keeps only as a fold: [100]
    return out


@pytest.fixture(scope="module")
def wit(engine, blocks):
    data, off, lens, cids = bundle_ref.tables_from_blocks(blocks[:100])
    cids = np.concatenate([cids, np.zeros((1, 40), dtype=np.uint8)])
    cids[100, :38] = np.frombuffer(blocks[100][0], dtype=np.uint8)
    data = np.concatenate([data, np.frombuffer(blocks[100][1], dtype=np.uint8)])
    off = np.concatenate([off, np.array([int(off[-1]) + int(lens[-1])], dtype=np.uint64)])
    lens = np.concatenate([lens, np.array([len(blocks[100][1])], dtype=np.uint32)])
    with engine.witness(data, off, lens, cids) as w:
        yield w


SMALL = cases.Case("sound_after_a_refusal")
cases.add_storage(SMALL, [cases._run("small", 2)])
cases.add_event(SMALL, cases.add_tipset(SMALL, [cases.cid38("sp")], cases.cid38("sc")), data=b"\x07")


def outcome(engine, w, res, **kw):
    try:
        return res.write(engine, w, **kw)
    except ipcfp.EngineError as e:
        return (e.rc, e.bad_kind, e.bad_index)


# ---- 1. the table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.ALL, ids=lambda c: c.name)
def test_every_case_of_the_table(engine, wit, case):
    got = outcome(engine, wit, Resident(case))
    if case.refusal is None:
        assert got == case.head() + b"]}"
    else:
        assert got == case.refusal
        msg = engine.lib.ipcfp_last_error(engine.h).decode()
        assert "bundle_write_packed_json" in msg and (case.refusal[2] is None or "[%d]" % case.refusal[2] in msg), msg
    # the context is whole: a sound call on it
    assert outcome(engine, wit, Resident(SMALL)) == SMALL.head() + b"]}"


def test_the_sound_cases_in_one_call(engine, wit):
    m = cases.merge(cases.SOUND)
    assert m.n_events >= 500 and m.n_storage >= 700  # several workgroups of items, a few hundred KB of text
    assert outcome(engine, wit, Resident(m)) == m.head() + b"]}"


# ---- 2. the buffer contract ----------------------------------------------------------------------------------------------------
def test_buffer_contract(engine, wit):
    m = cases.merge([c for c in cases.SOUND if c.name.startswith(("cids", "place_", "tipsets"))])
    res, want = Resident(m), m.head() + b"]}"
    rc, n, _ = res.write(engine, wit, cap=0)
    assert (rc, n) == (0, len(want))
    rc, n, buf = res.write(engine, wit, cap=len(want) - 1)
    assert rc == -1 and n == len(want) and (buf == 0xA5).all()
    rc, n, buf = res.write(engine, wit, cap=len(want))
    assert (rc, n) == (0, len(want)) and buf.tobytes() == want
    rc, n, buf = res.write(engine, wit, cap=len(want) + 64)
    assert (rc, n) == (0, len(want)) and buf[: len(want)].tobytes() == want and (buf[len(want):] == 0xA5).all()
    # a refusal writes nothing and still says nothing about a length
    bad = Resident(next(c for c in cases.REFUSED if c.name == "two_defects"))
    rc, n, buf = bad.write(engine, wit, cap=1 << 20)
    assert rc == -5 and n == 0 and (buf == 0xA5).all()


# ---- 3. with blocks -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [0, 1, 100])
def test_head_and_blocks(engine, wit, blocks, n_blocks):
    for case in (cases.merge([c for c in cases.SOUND if c.name.startswith("place_")], "places"), cases.Case("no_claims")):
        ids = list(range(n_blocks))[::-1]
        got = Resident(case).write(engine, wit, block_ids=ids)
        assert got == bundle_ref.bundle_json(case.storage_dicts, case.event_dicts, [blocks[i] for i in ids]).encode()
    if n_blocks == 100:  # block_ids == NULL: every block of the witness — the folded one among them
        assert outcome(engine, wit, Resident(SMALL), block_ids=None) == (-5, cases.BLOCKS, 100)


def test_block_refusals_behind_a_sound_head(engine, wit, blocks):
    res = Resident(SMALL)
    assert outcome(engine, wit, res, block_ids=[3, 4, 101, 5]) == (-1, cases.BLOCKS, 2)
    assert outcome(engine, wit, res, block_ids=[3, 100, 101]) == (-5, cases.BLOCKS, 1)
    # events before blocks, storage before events
    bad = Resident(next(c for c in cases.REFUSED if c.name == "claim_flags_1"))
    assert outcome(engine, wit, bad, block_ids=[101]) == (-1, cases.EVENTS, 1)
    assert outcome(engine, wit, res, block_ids=[7]) == SMALL.head() + bundle_ref.block_json(*blocks[7]).encode() + b"]}"


# ---- 4. from the generators ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tip():
    return Tipset(n_receipts=3000, n_parents=3, dup_permille=60, n_planted=7, variety=1, max_events=5, no_events_permille=100,
                  n_actors=3000, n_contracts=8, slots_per_contract=12, storage_layout_mix=1, n_actor_queries=12)


def test_generated_handles_of_the_synthetic_tipset(engine, tip):
    with engine.witness(tip.data, tip.off, tip.lens, tip.cids) as w:
        st, ge = w.generate_event_claims(tip.parent_cids, tip.child_cid, tip.topic0, tip.topic1)
        assert st == 1 and ge.n > 0
        with ge, w.generate_storage_claims(tip.child_cid, tip.child_epoch, tip.sc_actor, tip.sc_slot) as gs:
            assert gs.n > 0 and gs.first_error is None
            ids = np.union1d(gs.block_ids, ge.block_ids).astype(np.uint32)
            got = engine.bundle_write_generated_json(w, gs, ge, block_ids=ids)
            sp, ns = gs.proofs()
            ep, ne = ge.proofs()
            assert got == w.write_bundle_json(sp, ns, ep, ne, block_ids=ids)
            # … and Python's writer over the handles' strings
            blocks = [(tip.cids[i, :38].tobytes(), tip.block(i)) for i in ids]
            assert got == bundle_ref.bundle_json(gs.proof_rows(), ge.proof_rows(), blocks).encode()
            b = engine.bundle(got)
            try:
                ss, es = b.verify()
            finally:
                b.close()
            assert len(ss) == gs.n and len(es) == ge.n and (ss == 1).all() and (es == 1).all()
            # one handle alone; none at all
            assert engine.bundle_write_generated_json(w, None, ge, block_ids=[]) == w.write_bundle_json(None, 0, ep, ne, block_ids=[])
            assert engine.bundle_write_generated_json(w, gs, None, block_ids=[]) == w.write_bundle_json(sp, ns, None, 0, block_ids=[])
            assert engine.bundle_write_generated_json(w, None, None, block_ids=[]) == b'{"storage_proofs":[],"event_proofs":[],"blocks":[]}'
        # a chain of children with a failing one in the middle: refused where _proofs is, at _first_error
        bogus = cases.cid38("no such child")
        with w.generate_storage_claims_tipsets([tip.child_cid, bogus, tip.child_cid], [tip.child_epoch, 5, -6], tip.sc_actor,
                                               tip.sc_slot) as gs:
            n = len(tip.sc_actor)
            assert gs.n == 3 * n and gs.first_error == n
            with pytest.raises(ipcfp.EngineError) as e:
                engine.bundle_write_generated_json(w, gs, None, block_ids=[])
            assert (e.value.rc, e.value.bad_kind, e.value.bad_index) == (-1, cases.STORAGE, n)
            with pytest.raises(ipcfp.EngineError) as e2:
                gs.proofs()
            assert (e2.value.rc, e2.value.bad_index) == (-1, n)
        with w.generate_storage_claims_tipsets([tip.child_cid, tip.child_cid], [tip.child_epoch, -tip.child_epoch], tip.sc_actor,
                                               tip.sc_slot) as gs:
            sp, ns = gs.proofs()
            assert engine.bundle_write_generated_json(w, gs, None, block_ids=gs.block_ids) == \
                w.write_bundle_json(sp, ns, None, 0, block_ids=gs.block_ids)


@pytest.mark.parametrize("name", ["fail/txmeta_absent/middle", "sound/3", "parent_counts"])
def test_generated_event_chain(engine, name):
    store, pairs = gc.world()
    with engine.witness(*store.tables()) as w:
        with w.generate_event_claims_tipsets([pairs[p] for p in gc.chains()[name]], *gc.FILTER) as ge:
            assert ge.n > 0 and ge.tipset_count == len(gc.chains()[name])
            if name.startswith("fail"):
                assert (ge.tipset_status != 1).sum() == 1
            ep, ne = ge.proofs()
            got = engine.bundle_write_generated_json(w, None, ge, block_ids=ge.block_ids)
            assert got == w.write_bundle_json(None, 0, ep, ne, block_ids=ge.block_ids)
            assert bundle_ref.parse_bundle(got)["event_proofs"] == ge.proof_rows()
            b = engine.bundle(got)
            try:
                ss, es = b.verify()
            finally:
                b.close()
            assert len(es) == ge.n and (es == 1).all()


# ---- 5. fuzz -------------------------------------------------------------------------------------------------------------------
def test_fuzz_against_the_python_writer(engine, wit):
    rng = np.random.default_rng(fuzz_seed(0xC1A1))
    pick = lambda xs: xs[int(rng.integers(0, len(xs)))]  # noqa: E731
    for rnd in range(40):
        c = cases.Case("fuzz_%d" % rnd)
        n = int(rng.integers(1, 301))
        n_s = int(rng.integers(0, n + 1))
        runs = []
        left = n_s
        while left:
            k = int(min(left, rng.integers(1, 70)))
            runs.append(cases._run(("fz", rnd, len(runs)), k, epoch=pick(cases.EPOCHS), actor=pick(cases.UINTS),
                                   cids=[pick(cases.SOUND_CIDS) for _ in range(4)]))
            left -= k
        cases.add_storage(c, runs)
        ts = [cases.add_tipset(c, [pick(cases.SOUND_CIDS) for _ in range(pick([1, 2, 5, 33]))], pick(cases.SOUND_CIDS))
              for _ in range(int(rng.integers(1, 4)))]
        for _ in range(n - n_s):
            cases.add_event(c, pick(ts), pe=pick(cases.EPOCHS), ce=pick(cases.EPOCHS), exec_index=pick(cases.UINTS),
                            event_index=pick(cases.UINTS), emitter=pick(cases.UINTS), msg=pick(cases.SOUND_CIDS),
                            topics=cases._topics(rng, pick(cases.TOPIC_COUNTS)),
                            data=rng.integers(0, 256, pick(cases.DATA_LENS[:-2]), dtype=np.uint8).tobytes())
        assert outcome(engine, wit, Resident(c)) == c.head() + b"]}", rnd
