"""GPU: the fallbacks a context takes when a side stream or a pinned page cannot be had never change an outcome.

`ipcfp_ctx_create` may fail to create K1's stream, the aux stream, the mailbox page or the control block, and goes on
without; IPCFP_K1_STREAM=0, IPCFP_AUX_STREAM=0, IPCFP_MAILBOX=0 and IPCFP_CTL_BLOCK=0 force each of those. A fresh
context under each of them (and under all four) runs the CID check, verify_event_proof with honest and lying claims
in both orders with the scan, and a storage batch large enough for the tabled route: every byte must equal the oracle's
and the default context's.

That a forced context really is in its fallback is checked where the ABI shows it: the route without a mid-call
synchronisation (host/verify_fast.cpp, the only code that brackets IPCFP_K_TIPSET_PROLOGUE) needs the mailbox and an aux
stream of its own, so its launch count is zero under IPCFP_MAILBOX=0 and IPCFP_AUX_STREAM=0 and positive otherwise.  K1's
stream and the control block have no such witness through the ABI; every switch name is checked against the getenv
sites of host/context.cpp, so that a renamed switch cannot leave this test running the default route."""
import os

import numpy as np
import pytest

from conftest import fuzz_seed

import claims
import ipc_filecoin_proofs_amd as ipcfp
from test_gpu_event_table import packed, same_scan
from tools.synth import Tipset

pytestmark = pytest.mark.gpu

SWITCHES = ("IPCFP_K1_STREAM", "IPCFP_AUX_STREAM", "IPCFP_MAILBOX", "IPCFP_CTL_BLOCK")


def storage_claims(tip):
    sc = claims.StorageClaims(tip)
    for k in range(3, sc.n, 17):  # lies: a wrong value, a value no padded word can equal, a wrong storage root
        if k % 3 == 0:
            sc.set_str(k, "value", "0x" + "ee" * 32)
        elif k % 3 == 1:
            sc.set_str(k, "value", "0x1234")
        else:
            sc.set_str(k, "storage_root", claims.cid_str(tip.child_cid))
    return sc


def run_all(eng, ev_tip, ev_claims, st_tip, sc, blocks):
    """Everything one context answers, in a fixed order."""
    data, off, lens, cids = blocks
    out = {}
    eng.profile_enable(True, only="tipset_prologue")
    eng.profile_reset()
    with eng.witness(data, off, lens, cids) as w:
        out["cid_planted"] = w.verify_cids()
    ts, cl, blob, blob_len = ev_claims
    for order in ("verify-first", "scan-first"):
        with eng.witness(ev_tip.data, ev_tip.off, ev_tip.lens, ev_tip.cids) as w:
            out["cid_" + order] = w.verify_cids()
            if order == "scan-first":
                scan = w.scan_events(ev_tip.receipts_root, ev_tip.topic0, ev_tip.topic1, actor=ev_tip.filter_actor)
                st = w.verify_event_claims(ts, cl, blob, blob_len)
            else:
                st = w.verify_event_claims(ts, cl, blob, blob_len)
                scan = w.scan_events(ev_tip.receipts_root, ev_tip.topic0, ev_tip.topic1, actor=ev_tip.filter_actor)
            scan_any = w.scan_events(ev_tip.receipts_root, ev_tip.topic0, ev_tip.topic1, actor=None, want_touched=False)
        out["events_" + order] = (st, scan, scan_any)
    with eng.witness(st_tip.data, st_tip.off, st_tip.lens, st_tip.cids) as w:
        out["storage"] = w.verify_storage_proofs(sc.arr, sc.n)
    out["fast_verify_calls"] = eng.profile_read("tipset_prologue")[0]
    eng.profile_enable(False)
    return out


def fresh_engine_results(env, *args):
    before = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)
    try:
        with ipcfp.Engine(0) as eng:  # (the switches are read when the context is created)
            return run_all(eng, *args)
    finally:
        for k, v in before.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_every_forced_fallback_equals_the_oracle_and_the_default_context(engine, oracle):
    context_cpp = open(os.path.join(os.path.dirname(os.path.abspath(ipcfp.__file__)), os.pardir, "ipc-filecoin-proofs_amd",
                                    "csrc", "host", "context.cpp")).read()
    for k in SWITCHES:
        assert 'getenv("%s")' % k in context_cpp, k
    ev_tip = Tipset(n_receipts=6000, n_parents=3, n_planted=25, variety=1, max_events=5, no_events_permille=80,
                    events_bit_width=5, seed=fuzz_seed(905))
    ev_claims = packed(ev_tip)
    st_tip = Tipset(n_receipts=8, n_planted=0, n_actors=3000, n_contracts=12, slots_per_contract=40, storage_layout_mix=1,
                    seed=fuzz_seed(77))
    sc = storage_claims(st_tip)
    assert sc.n * 16 >= len(st_tip.lens), "the storage batch must take the tabled route"
    # 512 random blocks with one planted bad CID
    rng = np.random.default_rng(fuzz_seed(12))
    n = 512
    lens = rng.integers(1, 1500, n).astype(np.uint32)
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = rng.integers(0, 256, int(lens.sum()), dtype=np.uint8)
    cids = np.zeros((n, 40), dtype=np.uint8)
    cids[:, :6] = np.frombuffer(bytes.fromhex("0171a0e40220"), dtype=np.uint8)
    cids[:, 6:38] = oracle.hash_batch("blake2b256", data, off, lens)
    cids[77, 20] ^= 0x04
    blocks = (data, off, lens, cids)

    # the oracle
    ts, cl, blob, _ = ev_claims
    ost = oracle.store(ev_tip.data, ev_tip.off, ev_tip.lens, ev_tip.cids, threads=0)
    want_ev = ost.verify_event_claims_packed(ts, cl, blob, threads=0)
    o_scan = ost.scan_events(ev_tip.receipts_root, ev_tip.topic0, ev_tip.topic1, actor=ev_tip.filter_actor, threads=0)
    o_any = ost.scan_events(ev_tip.receipts_root, ev_tip.topic0, ev_tip.topic1, actor=None, want_touched=False, threads=0)
    ost.close()
    ost = oracle.store(st_tip.data, st_tip.off, st_tip.lens, st_tip.cids, threads=0)
    want_st = ost.verify_storage_proofs(sc, mode=0)
    ost.close()
    assert (want_ev != 255).all() and len(set(want_ev.tolist())) >= 5
    assert (want_st == 1).sum() > sc.n // 2 and len(set(want_st.tolist())) >= 3
    want_cid = np.ones(n, dtype=np.uint8)
    want_cid[77] = 0

    def check_oracle(got, what):
        st, nbad = got["cid_planted"]
        assert np.array_equal(st, want_cid) and nbad == 1, what
        for order in ("verify-first", "scan-first"):
            st, nbad = got["cid_" + order]
            assert nbad == 0 and (st == 1).all(), (what, order)
            st, scan, scan_any = got["events_" + order]
            assert np.array_equal(st, want_ev), (what, order, np.nonzero(st != want_ev)[0][:10])
            assert scan[0] == o_scan[0] == 1 and np.array_equal(scan[1], o_scan[1]), (what, order)
            assert np.array_equal(scan[2]["exec_index"], o_scan[2][:, 0]), (what, order)
            assert np.array_equal(scan[2]["event_index"], o_scan[2][:, 1]), (what, order)
            assert {bytes(c) for c in ev_tip.cids[scan[3]]} == {bytes(c) for c in o_scan[3]}, (what, order)
            assert scan_any[0] == 1 and np.array_equal(scan_any[1], o_any[1]), (what, order)
            assert np.array_equal(scan_any[2]["event_index"], o_any[2][:, 1]), (what, order)
        assert np.array_equal(got["storage"], want_st), (what, np.nonzero(got["storage"] != want_st)[0][:10])

    args = (ev_tip, ev_claims, st_tip, sc, blocks)
    ref = fresh_engine_results({}, *args)  # a default context
    check_oracle(ref, "default")
    assert ref["fast_verify_calls"] > 0, "the default context must take the route without a mid-call synchronisation"
    check_oracle(run_all(engine, *args), "session engine")
    forced = [{k: "0"} for k in SWITCHES] + [{k: "0" for k in SWITCHES}]
    for env in forced:
        what = ",".join(sorted(env))
        got = fresh_engine_results(env, *args)
        check_oracle(got, what)
        no_fast = "IPCFP_MAILBOX" in env or "IPCFP_AUX_STREAM" in env
        assert (got["fast_verify_calls"] == 0) == no_fast, (what, got["fast_verify_calls"])
        # … and byte for byte what the default context answered, the located events' records included
        assert np.array_equal(got["cid_planted"][0], ref["cid_planted"][0]), what
        assert np.array_equal(got["storage"], ref["storage"]), what
        for order in ("verify-first", "scan-first"):
            assert np.array_equal(got["cid_" + order][0], ref["cid_" + order][0]), (what, order)
            st, scan, scan_any = got["events_" + order]
            r_st, r_scan, r_any = ref["events_" + order]
            assert np.array_equal(st, r_st), (what, order)
            assert same_scan(scan, r_scan) and same_scan(scan_any, r_any), (what, order)
