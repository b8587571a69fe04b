"""GPU: the table verifier's ladder (csrc/kernels/verify_table.hip) rung by rung, against the CPU oracle.

k_verify_events_table settles the usual claim — one context per wavefront, at most two claimed topics, 32 bytes of
claimed data or data that can never match — from four load batches and a ladder of selects (verify_table_hot), and every
other claim from the ladder of early returns (verify_table_one).  Both must report the FIRST rung a claim breaks, in the
reference's order (src/proofs/events/verifier.rs:92-290).  Here: one claim per rung, every pair of rungs (the earlier one
must win), batch sizes at the edges of the wavefront and the workgroup, orders that put both kinds of claim into one
wavefront, and a batch over two tipset pairs interleaved claim by claim (contexts differ within every wavefront: every
claim takes verify_table_one) — each with and without a filter, under the trust policies of
test_gpu_events.test_event_proofs_adversarial, with and without event locations, under fast_verify 1 and 0.

Every expected status is the oracle's; where test_gpu_events.py names a literal code for a lie, the same literal is
asserted here.  Locations are held to those of the ladder of early returns: the same claims interleaved with another
pair's.  No claim is ever left out of a comparison (`compare` asserts it)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import claims
from tools.synth import Tipset

pytestmark = pytest.mark.gpu

NO_BLOCK = 0xFFFFFFFF
# statuses of a proof that has reached its event (verifier.rs:257-290, 247-251): these carry a location
REACHED = (1, 12, 13, 14, 15, 16, 17)


def spec_of(T, i):
    """the honest claim of row i of T's claim table, as a dict a lie can be told in"""
    e, nt = int(T.claim_exec[i]), int(T.claim_ntopics[i])
    return dict(parents=[claims.cid_str(c) for c in T.parent_cids], child=claims.cid_str(T.child_cid),
                parent_epoch=T.parent_epoch, child_epoch=T.child_epoch, message=claims.cid40_str(T.exec_order[e]),
                exec_index=e, event_index=int(T.claim_event[i]), emitter=int(T.claim_emitter[i]),
                topics=[claims.hex0x(T.claim_topics[i, t].tobytes()) for t in range(nt)],
                data=claims.hex0x(T.claim_data[i, : int(T.claim_datalen[i])].tobytes()))


class Batch:
    """An array of EventProof structs (tests/claims.py) built from specs; owns the strings behind it."""

    def __init__(self, specs):
        self.specs = specs
        self.n = len(specs)
        self.arr = (claims.EventProof * max(self.n, 1))()
        self._keep = []
        for k, s in enumerate(specs):
            p = self.arr[k]
            parents = [x.encode() for x in s["parents"]]
            parr = (C.c_char_p * max(len(parents), 1))(*parents)
            topics = [x.encode() for x in s["topics"]]
            tarr = (C.c_char_p * max(len(topics), 1))(*topics)
            child, msg, data = s["child"].encode(), s["message"].encode(), s["data"].encode()
            self._keep += [parents, parr, topics, tarr, child, msg, data]
            p.parent_epoch, p.child_epoch = s["parent_epoch"], s["child_epoch"]
            p.parent_tipset_cids, p.n_parent_tipset_cids = parr, len(parents)
            p.child_block_cid, p.message_cid = child, msg
            p.exec_index, p.event_index, p.emitter = s["exec_index"], s["event_index"], s["emitter"]
            p.topics, p.n_topics, p.data = tarr, len(topics), data

    def claimed_shapes(self):
        """(claims of the usual shape, claims with more than two topics, claims whose matchable data is not 32 bytes)"""
        wide = sum(len(s["topics"]) > 2 for s in self.specs)
        odd = sum(s["data"].startswith("0x") and len(s["data"]) != 66 for s in self.specs)
        usual = sum(len(s["topics"]) <= 2 and not (s["data"].startswith("0x") and len(s["data"]) != 66) for s in self.specs)
        return usual, wide, odd


class World:
    pass


@pytest.fixture(scope="module")
def world(engine, oracle):
    """Two small tipsets (the arguments of test_gpu_events.py's fixture at 256 receipts) in ONE witness, the oracle's
    store of the same blocks, and the rows of the first tipset's claim table by shape."""
    a = Tipset(n_receipts=256, n_parents=3, dup_permille=80, n_planted=9, variety=1, max_events=6, no_events_permille=150)
    b = Tipset(n_receipts=256, n_parents=3, dup_permille=80, n_planted=9, variety=1, max_events=6, no_events_permille=150,
               seed=a.params["seed"] + 17, parent_epoch=a.parent_epoch + 40)
    data = np.concatenate([a.data, b.data])
    off = np.concatenate([a.off, b.off + np.uint64(a.data.size)])
    lens = np.concatenate([a.lens, b.lens])
    cids = np.concatenate([a.cids, b.cids])
    W = World()
    W.a, W.b = a, b
    W.w = engine.witness(data, off, lens, cids)
    W.st = oracle.store(data, off, lens, cids)
    W.engine = engine
    W.other_cid = claims.cid_str(oracle.cid_for_block(b"x"))
    W.filt = claims.make_filter(a.topic0, a.topic1)
    W.policies = [None,
                  claims.TrustPolicy(1, 0, a.parent_epoch, a.parent_epoch),       # child epoch outside → untrusted child
                  claims.TrustPolicy(1, 0, a.child_epoch, a.child_epoch + 5),     # parent epoch outside
                  claims.TrustPolicy(1, 1, 0, 10 ** 9),                           # empty EC chain
                  claims.TrustPolicy(1, 0, a.parent_epoch, a.child_epoch)]        # both inside
    honest = Batch([spec_of(a, i) for i in range(len(a.claim_exec))])
    W.honest_want = W.st.verify_event_proofs(honest, mode=1)
    nt, dl = a.claim_ntopics, a.claim_datalen
    ok = W.honest_want == 1
    W.rows_usual = np.nonzero(ok & (nt == 2) & (dl == 32))[0]          # two topics, 32 bytes: the usual shape
    W.rows_one_topic = np.nonzero(ok & (nt == 1))[0]
    W.rows_wide = np.nonzero(ok & (nt > 2))[0]                         # more than two topics
    W.rows_odd_data = np.nonzero(ok & (nt == 2) & (dl != 32))[0]       # Case A logs: 48 bytes
    W.rows_not_log = np.nonzero(W.honest_want == 13)[0]                # the event is no EVM log
    planted = set(a.planted.tolist())
    W.rows_planted = np.array([i for i in W.rows_usual if int(a.claim_exec[i]) in planted], dtype=np.int64)
    have = set(a.claim_exec.tolist())
    W.no_event_receipts = [e for e in range(len(a.exec_order)) if e not in have]
    W.filler = [spec_of(b, i) for i in range(len(b.claim_exec))]
    # how many claims of each shape the tipset yields: each kind of claim the kernel tells apart is there
    W.shape_counts = dict(usual=len(W.rows_usual), one_topic=len(W.rows_one_topic), wide=len(W.rows_wide),
                          odd_data=len(W.rows_odd_data), not_log=len(W.rows_not_log), planted=len(W.rows_planted),
                          no_event_receipts=len(W.no_event_receipts), other_pair=len(W.filler))
    for name, count in W.shape_counts.items():
        assert count > 0, (name, W.shape_counts)
    W.n_rows = len(honest.specs)
    assert W.n_rows >= 130 and len(W.filler) >= 130
    yield W
    W.w.close()
    W.st.close()


# ---- the lies, in the ladder's order -----------------------------------------------------------------------------------
# (name, the literal status test_gpu_events.py's `exp` table names for it or None, batch of the hot path the rung's
#  inputs arrive in, the lie).  A lie that MOVES the claim to another receipt or event is told first (`moves`).
def _flip_last(h):
    return h[:-1] + ("0" if h[-1] != "0" else "1")


def lies(W):
    a = W.a
    e0 = W.no_event_receipts[0]
    r13 = int(W.rows_not_log[0])

    def move_to_receipt_without_events(s):
        s["exec_index"], s["message"] = e0, claims.cid40_str(a.exec_order[e0])

    def move_to_event_that_is_no_log(s):
        e = int(a.claim_exec[r13])
        s["exec_index"], s["message"] = e, claims.cid40_str(a.exec_order[e])
        s["event_index"], s["emitter"] = int(a.claim_event[r13]), int(a.claim_emitter[r13])

    def upd(**kw):
        return lambda s: s.update(kw)

    return [
        ("child epoch", 5, "B", lambda s: s.update(child_epoch=s["child_epoch"] + 1)),
        ("parent epoch", 6, "B", lambda s: s.update(parent_epoch=s["parent_epoch"] - 1)),
        ("message unparsable", 69, "B", upd(message="zzz")),
        # (a string that does not parse names no message of the order either: told on top of it, this lie changes nothing)
        ("message not in the exec order", 7, "C", lambda s: s.update(message=W.other_cid) if s["message"] != "zzz" else None),
        ("message at another index", 8, "C", lambda s: s.update(exec_index=s["exec_index"] + 1)),
        ("no events root", None, "C", move_to_receipt_without_events),
        ("no such event", 11, "C", upd(event_index=999)),
        ("emitter", 12, "C", lambda s: s.update(emitter=s["emitter"] + 1)),
        ("not an EVM log", None, "C", move_to_event_that_is_no_log),
        ("topic count", 14, "C", lambda s: s.update(topics=s["topics"][:1])),
        ("topic 0", 15, "D", lambda s: s.update(topics=["0x" + "11" * 32] + s["topics"][1:])),
        ("topic 1", 15, "D", lambda s: s.update(topics=s["topics"][:1] + ["0x" + "22" * 32] + s["topics"][2:])
         if len(s["topics"]) >= 2 else None),
        ("data length", 16, "D", lambda s: s.update(data=s["data"] + "00")),
        ("data bytes", 16, "D", lambda s: s.update(data=_flip_last(s["data"]))),
        ("data without 0x", 16, "D", lambda s: s.update(data=s["data"][2:])),
    ]


MOVES = ("no events root", "not an EVM log")
LITERAL = {"no events root": 10, "not an EVM log": 13}  # (ipcfp.h; test_gpu_events.py names 13 in its honest test)


def tell(spec, lie_list):
    """the lies told on a copy of the claim: the moves first, then in the ladder's order"""
    s = dict(spec)
    for name, _, _, fn in sorted(lie_list, key=lambda l: l[0] not in MOVES):
        fn(s)
    return s


def settings():
    """(filter?, trust policy index, locations?, fast_verify): every combination of filter, locations and fast_verify
    under AcceptAll, and each of the four policies with and without filter and locations."""
    out = [(f, 0, loc, fast) for f in (False, True) for loc in (False, True) for fast in (1, 0)]
    out += [(f, p, loc, 1) for p in (1, 2, 3, 4) for f in (False, True) for loc in (False, True)]
    return out


def compare(got, want, what):
    left_out = len(want) - len(got)
    assert left_out == 0, what                       # every claim of the batch is compared
    bad = np.nonzero(got != want)[0]
    assert len(bad) == 0, (what, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def run_everywhere(W, batch, what):
    """The batch in every setting against the oracle; with locations, against the same claims interleaved with another
    pair's (two contexts in every wavefront: the ladder of early returns).  Returns the plain run's statuses."""
    n = batch.n
    mixed = Batch([s for pair in zip(batch.specs, itertools.cycle(W.filler)) for s in pair])
    wants, plain = {}, None
    try:
        for use_filter, pol, located, fast in settings():
            filt, trust = (W.filt if use_filter else None), W.policies[pol]
            key = (use_filter, pol)
            if key not in wants:
                wants[key] = (W.st.verify_event_proofs(batch, trust=trust, filt=filt, mode=0),
                              W.st.verify_event_proofs(mixed, trust=trust, filt=filt, mode=0))
            want, want_mixed = wants[key]
            W.engine.set_tuning("fast_verify", fast)
            tag = (what, "filter" if use_filter else "no filter", "policy %d" % pol, "located" if located else "plain", fast)
            if not located:
                got = W.w.verify_event_proofs(batch.arr, n, trust=trust, filt=filt)
                compare(got, want, tag)
                if key == (False, 0) and plain is None:
                    plain = got
                continue
            got, loc = W.w.verify_event_proofs_located(batch.arr, n, trust=trust, filt=filt)
            compare(got, want, tag)
            got_m, loc_m = W.w.verify_event_proofs_located(mixed.arr, mixed.n, trust=trust, filt=filt)
            compare(got_m, want_mixed, tag + ("interleaved",))
            for f in ("block", "off", "len"):
                assert np.array_equal(loc[f], loc_m[f][0::2]), tag + (f,)
            reached = np.isin(got, REACHED)
            assert (loc["block"][reached] != NO_BLOCK).all() and (loc["block"][~reached] == NO_BLOCK).all(), tag
    finally:
        W.engine.set_tuning("fast_verify", -1)
    return plain


def test_one_claim_per_rung(world):
    W = world
    base = [spec_of(W.a, int(i)) for i in W.rows_usual]
    L = lies(W)
    specs = [tell(base[k % len(base)], [lie]) for k, lie in enumerate(L)]
    # the data-length rung inside the usual shape: 32 claimed bytes against an event of 48
    odd = spec_of(W.a, int(W.rows_odd_data[0]))
    specs.append(dict(odd, data=odd["data"][:66]))
    # an event index below 64 that the receipt does not have, and the index past MAX_INDEX (Err)
    specs.append(dict(base[0], event_index=63))
    specs.append(dict(base[1], event_index=2 ** 64 - 1))
    specs += base[: 70 - len(specs)]                      # honest claims around them: more than one wavefront
    batch = Batch(specs)
    got = run_everywhere(W, batch, "rungs")
    for k, (name, literal, _, _) in enumerate(L):
        literal = LITERAL.get(name, literal)
        assert got[k] == literal, (name, got[k], literal)
    assert got[len(L)] == 16 and got[len(L) + 1] == 11 and got[len(L) + 2] == 64
    assert (got[len(L) + 3:] == 1).all()


def test_the_earlier_of_two_broken_rungs_is_reported(world):
    """Every pair of lies (so every adjacent pair of rungs, and every pair whose rungs take their inputs from two
    different load batches): the status is the one of the lie that comes first in the ladder."""
    W = world
    base = [spec_of(W.a, int(i)) for i in np.concatenate([W.rows_planted, W.rows_usual])]
    L = lies(W)
    pairs = [(i, j) for i in range(len(L)) for j in range(i + 1, len(L)) if not (L[i][0] in MOVES and L[j][0] in MOVES)]
    # (the two lies that move the claim elsewhere cannot both be told; they are neither adjacent nor in different batches)
    adjacent = {(i, i + 1) for i in range(len(L) - 1)}
    spanning = {(i, j) for i, j in itertools.combinations(range(len(L)), 2) if L[i][2] != L[j][2]}
    assert adjacent <= set(pairs) and spanning <= set(pairs) and len(spanning) > 0
    batch = Batch([tell(base[k % len(base)], [L[i], L[j]]) for k, (i, j) in enumerate(pairs)])
    got = run_everywhere(W, batch, "pairs")
    for k, (i, j) in enumerate(pairs):
        first = LITERAL.get(L[i][0], L[i][1])
        assert got[k] == first, (L[i][0], L[j][0], got[k], first)


def test_one_context_whose_parents_do_not_match(world):
    """Parents in another order are another tipset key: ONE context for the whole batch (so its wavefronts stay on the
    usual path) whose header facts fail — and every later lie told on top of it changes nothing."""
    W = world
    base = [spec_of(W.a, int(i)) for i in W.rows_usual]
    L = lies(W)
    specs = [tell(base[k % len(base)], [lie]) for k, lie in enumerate(L)] + base[:50]
    for s in specs:
        s["parents"] = s["parents"][::-1]
    got = run_everywhere(W, Batch(specs), "parents mismatch")
    assert (got == 4).all()


@pytest.mark.parametrize("n", [1, 63, 65, 257])
def test_batch_sizes_at_the_edges_of_wavefront_and_workgroup(world, n):
    W = world
    specs = [spec_of(W.a, i % W.n_rows) for i in range(n)]   # the claim table in its own order (216 rows), again from its head
    for k in range(0, n, 7):
        specs[k] = dict(specs[k], emitter=specs[k]["emitter"] + 1)
    specs[n - 1] = dict(specs[n - 1], event_index=999)    # the last lane of the last wavefront
    got = run_everywhere(W, Batch(specs), "size %d" % n)
    assert got[n - 1] == 11 and (n == 1 or got[0] == 12)


def test_both_kinds_of_claim_in_one_wavefront(world):
    """Claimed topic counts 1, 2, 3, 4 alternating, claimed data of 0 / 32 / 33 / 100 bytes alternating: the usual shape
    and the others lane by lane."""
    W = world
    a = W.a
    by_topics = {1: W.rows_one_topic, 2: W.rows_usual, 4: W.rows_wide}
    specs = []
    for k in range(96):
        want_topics = 1 + k % 4
        if want_topics == 3:   # the tipset has no event of three topics: a four-topic event claimed with three
            s = spec_of(a, int(W.rows_wide[(k // 4) % len(W.rows_wide)]))
            s["topics"] = s["topics"][:3]
        else:
            rows = by_topics[want_topics]
            s = spec_of(a, int(rows[(k // 4) % len(rows)]))
        specs.append(s)
    for k in range(96, 192):
        s = spec_of(a, int(W.rows_usual[k % len(W.rows_usual)]))
        nbytes = (0, 32, 33, 100)[k % 4]
        s["data"] = (s["data"] + "ab" * 68)[: 2 + 2 * nbytes]
        specs.append(s)
    specs += [spec_of(a, int(i)) for i in W.rows_odd_data[:8]]   # honest claims of 48 bytes
    batch = Batch(specs)
    usual, wide, odd = batch.claimed_shapes()
    # 96 topic-count claims: 48 with one or two topics, 48 with three or four; 96 data claims: 24 of each length, 72 of
    # them not 32 bytes; and the honest 48-byte ones
    assert wide == 48 and odd >= 72 + 8 and usual > 0 and usual + wide + odd >= batch.n
    got = run_everywhere(W, batch, "mixed shapes")
    assert (got[2:96:4] == 14).all()                      # three topics claimed of four
    assert (got[97:192:4] == 1).all() and (got[96:192:4] == 16).all() and (got[98:192:4] == 16).all()
    assert (got[192:] == 1).all()


def test_two_tipset_pairs_interleaved_claim_by_claim(world):
    """Contexts that differ within every wavefront: every claim takes the ladder of early returns, with its own context."""
    W = world
    L = lies(W)
    mine = [spec_of(W.a, int(i)) for i in W.rows_usual]
    specs = []
    for k in range(130):
        specs.append(tell(mine[k % len(mine)], [L[k % len(L)]]) if k % 3 == 0 else mine[k % len(mine)])
        specs.append(W.filler[k] if k % 5 else dict(W.filler[k], emitter=W.filler[k]["emitter"] + 1))
    got = run_everywhere(W, Batch(specs), "two pairs")
    assert (got == 1).sum() > 100 and len(np.unique(got)) >= 8
