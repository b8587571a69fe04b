"""GPU: the receipts tree's leaf kernel on the verify call's table route stages each leaf node in LDS and finds its values'
starts in one pass per node (k_dense_receipt_leaves: a group of lanes per node).  Held to the oracle — status bytes, the
scan's has-match map and match records — where that pass meets something other than the common case: a receipt range
that starts and ends inside a leaf node, nodes larger than the stage (long return data: the pass runs on global memory),
heads the pass does not settle (non-minimal and 8-byte heads: the reader takes the value) in any slot of a node, and a
leaf whose header is not canonical (a hole in its bitmap: the anomaly, then the general walk)."""
import numpy as np
import pytest

from conftest import fuzz_seed

import ipc_filecoin_proofs_amd as ipcfp
from tools.synth import Tipset

pytestmark = pytest.mark.gpu

N = 6000


def packed(tip):
    ts, cl, blob, blob_len = ipcfp.pack_event_claims(
        tip.parent_cids, tip.child_cid, tip.parent_epoch, tip.child_epoch, tip.claim_exec, tip.claim_event,
        tip.claim_emitter, tip.exec_order[tip.claim_exec.astype(np.int64)], tip.claim_ntopics, tip.claim_topics,
        tip.claim_datalen, tip.claim_data)
    cl["event_index"][5::19] += 1
    cl["emitter"][2::29] += 1
    return ts, cl, blob, blob_len


def oracle_answers(oracle, tip, ts, cl, blob):
    ost = oracle.store(tip.data, tip.off, tip.lens, tip.cids, threads=0)
    want = ost.verify_event_claims_packed(ts, cl, blob, threads=0)
    o_st, o_has, o_trip, _ = ost.scan_events(tip.receipts_root, tip.topic0, tip.topic1, actor=tip.filter_actor,
                                             want_touched=False, threads=0)
    ost.close()
    return want, o_st, o_has, o_trip


def run(engine, tip, ts, cl, blob, blob_len, rng=None):
    """status bytes of the claims (of the range's receipts when `rng`), how often the table route's dense walk was queued,
    and the scan of the same witness: (status, has-match map, match triples)"""
    engine.profile_enable(True)
    engine.profile_reset()
    try:
        with engine.witness(tip.data, tip.off, tip.lens, tip.cids) as w:
            pos = None
            if rng is not None:
                w.set_receipt_range(*rng)
                pos, cl, blob, blob_len = ipcfp.route_event_claims(cl, blob, blob_len, rng[0], rng[1], False)
            st = w.verify_event_claims(ts, cl, blob, blob_len)
            walks = engine.profile_read("amt_walk")[0]
            s_st, s_has, s_m, _ = w.scan_events(tip.receipts_root, tip.topic0, tip.topic1, actor=tip.filter_actor,
                                                want_touched=False)
    finally:
        engine.profile_enable(False)
    trip = np.stack([s_m["exec_index"], s_m["event_index"], s_m["emitter"]], axis=1) if len(s_m) else np.zeros((0, 3))
    return pos, st, walks, (s_st, s_has, trip)


def check(want, o_st, o_has, o_trip, pos, st, scan, rng=None):
    lo, hi = (0, N) if rng is None else rng
    w = want if pos is None else want[pos.astype(np.int64)]
    assert np.array_equal(st, w), (np.nonzero(st != w)[0][:10], st[st != w][:10], w[st != w][:10])
    s_st, s_has, trip = scan
    assert s_st == o_st == 1
    assert np.array_equal(s_has, o_has[lo:hi])
    keep = (o_trip[:, 0] >= lo) & (o_trip[:, 0] < hi) if len(o_trip) else np.zeros(0, dtype=bool)
    assert np.array_equal(np.asarray(trip, dtype=np.int64), np.asarray(o_trip[keep], dtype=np.int64).reshape(-1, 3))


@pytest.mark.parametrize("events_bit_width,seed", [(3, 1), (5, 2), (7, 3)])
@pytest.mark.parametrize("rng", [None, (1003, 4869), (5, 5997)])
def test_unusual_receipts_through_the_node_groups(engine, oracle, events_bit_width, seed, rng):
    """Long return data (nodes beyond the stage) and heads of any width in every slot, over the whole tree and over
    ranges that start and end inside a leaf node (1003 = 8·125 + 3, 4869 = 8·608 + 5)."""
    tip = Tipset(n_receipts=N, n_parents=3, n_planted=20, variety=1, max_events=6, no_events_permille=120,
                 events_bit_width=events_bit_width, receipt_spelling=1, seed=fuzz_seed(1300 + seed))
    assert tip.lens.max() > 65536
    ts, cl, blob, blob_len = packed(tip)
    want, o_st, o_has, o_trip = oracle_answers(oracle, tip, ts, cl, blob)
    assert (want == 1).sum() > len(want) // 2 and len(set(want.tolist())) >= 3
    pos, st, walks, scan = run(engine, tip, ts, cl, blob, blob_len, rng)
    assert walks == 1  # the table route's dense walk, receipt leaves included, was queued
    check(want, o_st, o_has, o_trip, pos, st, scan, rng)


@pytest.mark.parametrize("rng", [None, (9, 5990)])
def test_common_receipts_through_the_node_groups(engine, oracle, rng):
    """The bench's spelling (every node inside the stage, every value settled by its heads), whole and ranged."""
    tip = Tipset(n_receipts=N, n_parents=3, dup_permille=20, n_planted=20, variety=1, max_events=4, seed=fuzz_seed(1310))
    ts, cl, blob, blob_len = packed(tip)
    want, o_st, o_has, o_trip = oracle_answers(oracle, tip, ts, cl, blob)
    pos, st, walks, scan = run(engine, tip, ts, cl, blob, blob_len, rng)
    assert walks == 1
    check(want, o_st, o_has, o_trip, pos, st, scan, rng)


@pytest.mark.parametrize("hole", [8 * 300 + 1, 8 * 301 + 4, 8 * 302 + 8])
def test_leaf_header_not_canonical(engine, oracle, hole):
    """A receipt left out of the tree: its leaf's bitmap has a hole in the first, a middle or the last slot — the header
    is not the canonical one, the kernel raises the anomaly and the call is redone the general way."""
    tip = Tipset(n_receipts=N, n_parents=3, n_planted=20, variety=1, max_events=4, receipt_spelling=1, receipt_hole=hole,
                 seed=fuzz_seed(1320))
    ts, cl, blob, blob_len = packed(tip)
    ost = oracle.store(tip.data, tip.off, tip.lens, tip.cids, threads=0)
    want = ost.verify_event_claims_packed(ts, cl, blob, threads=0)
    ost.close()
    _, st, _, _ = run_verify_only(engine, tip, ts, cl, blob, blob_len)
    assert np.array_equal(st, want), (np.nonzero(st != want)[0][:10], st[st != want][:10], want[st != want][:10])


def run_verify_only(engine, tip, ts, cl, blob, blob_len):
    with engine.witness(tip.data, tip.off, tip.lens, tip.cids) as w:
        return None, w.verify_event_claims(ts, cl, blob, blob_len), None, None
