"""GPU: the verify call's table route reads every receipt once — the receipts tree's leaf kernel finds its value by the heads
of the values in front of it, type-checks it and writes the LeafRef and the receipt's event record in the same lane
(k_dense_receipt_leaves).  Held to the oracle on receipts the synthetic writer spells unusually (tools/synth
`receipt_spelling`: return data of 0 to 70 000 bytes, exit code / length / gas heads of the minimal width or any wider one,
exit codes up to 2^32 - 1, 64-bit gas), on events AMTs the table does not cover (wide nodes: RK_WALK), on a receipts AMT
with a hole (a sparse leaf: the dense walk's anomaly, then the general walk), on an events root naming a block the
witness lacks, with duplicate messages across parents and lying claims, and with a scan riding on the call."""
import numpy as np
import pytest

from conftest import fuzz_seed

import ipc_filecoin_proofs_amd as ipcfp
from tools.synth import Tipset

pytestmark = pytest.mark.gpu


def packed(tip):
    ts, cl, blob, blob_len = ipcfp.pack_event_claims(
        tip.parent_cids, tip.child_cid, tip.parent_epoch, tip.child_epoch, tip.claim_exec, tip.claim_event,
        tip.claim_emitter, tip.exec_order[tip.claim_exec.astype(np.int64)], tip.claim_ntopics, tip.claim_topics,
        tip.claim_datalen, tip.claim_data)
    cl["event_index"][3::17] += 1
    cl["emitter"][7::23] += 1
    cl["exec_index"][11::29] += 1
    return ts, cl, blob, blob_len


def verify_profiled(engine, tip, ts, cl, blob, blob_len, data=None, off=None, lens=None, cids=None):
    """status bytes, and how often the dense walk of the table route was queued (profile group amt_walk: verify_fast.cpp)"""
    engine.profile_enable(True)
    engine.profile_reset()
    try:
        with engine.witness(tip.data if data is None else data, tip.off if off is None else off,
                            tip.lens if lens is None else lens, tip.cids if cids is None else cids) as w:
            st = w.verify_event_claims(ts, cl, blob, blob_len)
        walks = engine.profile_read("amt_walk")[0]
    finally:
        engine.profile_enable(False)
    return st, walks


def ride(engine, w, tip, ts, cl, blob, blob_len):
    import torch

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    n, nr = len(cl), int(tip.params["n_receipts"])
    d_cl, d_blob = dev(cl), dev(blob)
    d_st = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    d_has = torch.full((nr + 16,), 9, dtype=torch.uint8, device="cuda")
    d_m = torch.zeros(8192 * 40, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sst, snr, snm = w.verify_and_scan_device(ts, d_cl.data_ptr(), n, d_blob.data_ptr(), blob_len, d_st.data_ptr(),
                                             tip.topic0, tip.topic1, tip.filter_actor, d_has.data_ptr(), nr + 16, d_m.data_ptr(), 8192)
    engine.sync()
    m = d_m.cpu().numpy()[: snm * 40].view(ipcfp.MATCH_DTYPE) if sst == 1 else None
    trip = None if m is None else np.stack([m["exec_index"], m["event_index"], m["emitter"]], axis=1)
    return d_st.cpu().numpy(), sst, snr, d_has.cpu().numpy()[:snr] if sst == 1 else None, trip


@pytest.mark.parametrize("bit_width,seed", [(5, 1), (5, 2), (7, 3)])
def test_receipt_spellings_match_the_oracle(engine, oracle, bit_width, seed):
    tip = Tipset(n_receipts=6000, n_parents=3, n_planted=20, variety=1, max_events=6, no_events_permille=120,
                 events_bit_width=bit_width, receipt_spelling=1, seed=fuzz_seed(1200 + seed))
    assert tip.lens.max() > 65536  # (a leaf holding a receipt with 65 536 or more bytes of return data)
    ts, cl, blob, blob_len = packed(tip)
    ost = oracle.store(tip.data, tip.off, tip.lens, tip.cids, threads=0)
    want = ost.verify_event_claims_packed(ts, cl, blob, threads=0)
    os_, ohas, otrip, _ = ost.scan_events(tip.receipts_root, tip.topic0, tip.topic1, actor=tip.filter_actor, want_touched=False, threads=0)
    ost.close()
    assert (want == 1).sum() > len(want) // 2 and len(set(want.tolist())) >= 3  # (the spellings are receipts the reference takes)
    st, walks = verify_profiled(engine, tip, ts, cl, blob, blob_len)
    assert walks == 1  # the table route's dense walk, receipt leaves included, was queued
    assert np.array_equal(st, want), (np.nonzero(st != want)[0][:10], st[st != want][:10], want[st != want][:10])
    with engine.witness(tip.data, tip.off, tip.lens, tip.cids) as w:
        got = ride(engine, w, tip, ts, cl, blob, blob_len)
    assert np.array_equal(got[0], want)
    assert got[1] == os_ == 1 and got[2] == len(ohas) and np.array_equal(got[3], ohas)
    assert np.array_equal(got[4], otrip) if len(otrip) else got[4] is None or len(got[4]) == 0


@pytest.mark.parametrize("hole", [1, 2500, 5999])
def test_sparse_receipts_leaf(engine, oracle, hole):
    """A receipt left out of the receipts AMT: its leaf's bitmap has a hole, the dense walk raises its anomaly and the call
    is redone the general way — every status byte as the oracle has it."""
    tip = Tipset(n_receipts=6000, n_parents=3, n_planted=20, variety=1, max_events=4, receipt_hole=hole, seed=fuzz_seed(1220))
    ts, cl, blob, blob_len = packed(tip)
    ost = oracle.store(tip.data, tip.off, tip.lens, tip.cids, threads=0)
    want = ost.verify_event_claims_packed(ts, cl, blob, threads=0)
    ost.close()
    st, _ = verify_profiled(engine, tip, ts, cl, blob, blob_len)
    assert np.array_equal(st, want), (np.nonzero(st != want)[0][:10], st[st != want][:10], want[st != want][:10])


def test_missing_events_block(engine, oracle):
    """An events root that names a block the witness does not hold: the claims on that receipt and the scan say so, as the
    oracle does."""
    tip = Tipset(n_receipts=3000, n_parents=3, n_planted=12, variety=0, max_events=4, no_events_permille=0, seed=fuzz_seed(1210))
    ts, cl, blob, blob_len = packed(tip)
    with engine.witness(tip.data, tip.off, tip.lens, tip.cids) as w:
        _, _, m, _ = w.scan_events(tip.receipts_root, tip.topic0, tip.topic1, actor=None, want_touched=False)
    assert len(m) >= 4
    victim = int(m[len(m) // 2]["block"])  # the events AMT root of a receipt with a matching event
    keep = np.arange(len(tip.lens)) != victim
    off, lens, cids = tip.off[keep], tip.lens[keep], tip.cids[keep]
    ost = oracle.store(tip.data, off, lens, cids, threads=0)
    want = ost.verify_event_claims_packed(ts, cl, blob, threads=0)
    o_scan = ost.scan_events(tip.receipts_root, tip.topic0, tip.topic1, actor=tip.filter_actor, want_touched=False, threads=0)
    ost.close()
    assert (want >= 64).sum() >= 1 and o_scan[0] >= 64
    st, walks = verify_profiled(engine, tip, ts, cl, blob, blob_len, off=off, lens=lens, cids=cids)
    assert walks == 1
    assert np.array_equal(st, want)
    with engine.witness(tip.data, off, lens, cids) as w:
        gs = w.scan_events(tip.receipts_root, tip.topic0, tip.topic1, actor=tip.filter_actor, want_touched=False)
    assert gs[0] == o_scan[0]
