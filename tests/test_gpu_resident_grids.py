"""GPU: the CID check (k_blake2b256_cid) and the block-order event parse (k_block_events) as RESIDENT grids — a fixed
number of 256-thread workgroups per CU (tuning keys "k1_resident" / "parse_resident"), each looping over the tiles of
256 schedule entries blockIdx.x, blockIdx.x + gridDim.x, …; 0 is one workgroup per tile.  Held to the CPU where the
loop can go wrong: fewer blocks than one tile, a partial last tile, one block more than one stride of the grid (a
workgroup with a second tile of a single entry) and one block less than two strides (a workgroup with no second tile)
for K1; a tipset whose blocks cross one stride, one smaller than a tile row of the grid, and the same tipset under
both forms for the parse.  One stride at residency 1 is CUs × 256 entries."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import fuzz_seed

import ipc_filecoin_proofs_amd as ipcfp
from tools.synth import Tipset

pytestmark = pytest.mark.gpu

E_INVALID = -1
CID_MISMATCH, CID_OK, CID_UNCHECKED = 0, 1, 2
LENGTHS = np.array([0, 1, 127, 128, 129, 255, 256, 1000], dtype=np.uint32)
LONG_BLOCK = 70_000


def stride():
    return torch.cuda.get_device_properties(0).multi_processor_count * 256


@pytest.fixture(scope="module")
def tuned(engine):
    """A context of its own for the settings that are not the default (the shared engine keeps its defaults)."""
    eng = ipcfp.Engine(0)
    yield eng
    eng.close()


def pick(engine, tuned, k1=None, parse=None):
    """the shared engine for the defaults; the private one, with BOTH keys set, for anything else"""
    if k1 is None and parse is None:
        return engine
    assert k1 is not None and parse is not None
    tuned.set_tuning("k1_resident", k1)
    tuned.set_tuning("parse_resident", parse)
    return tuned


# ------------------------------------------------ K1 against hashlib ------------------------------------------------
@pytest.fixture(scope="module")
def k1_corpus():
    """2 × stride − 1 blocks, hashed on the CPU once; every case checks a prefix of it.  Block 0 is the long one, about
    1 % of the digests are wrong (block 1 among them), a few CIDs name another hash function."""
    n = 2 * stride() - 1
    rng = np.random.default_rng(fuzz_seed(1800))
    lens = LENGTHS[rng.integers(0, len(LENGTHS), n)]
    lens[0] = LONG_BLOCK
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = rng.integers(0, 256, int(lens.sum(dtype=np.uint64)), dtype=np.uint8)
    raw = data.tobytes()
    cids = np.zeros((n, 40), dtype=np.uint8)
    cids[:, :6] = np.frombuffer(bytes.fromhex("0171a0e40220"), dtype=np.uint8)
    for i in range(n):
        o = int(off[i])
        cids[i, 6:38] = np.frombuffer(hashlib.blake2b(raw[o:o + int(lens[i])], digest_size=32).digest(), dtype=np.uint8)
    want = np.full(n, CID_OK, dtype=np.uint8)
    bad = rng.random(n) < 0.01
    bad[1] = True
    bad[0] = False
    cids[bad, 6 + rng.integers(0, 32)] ^= 0x10
    want[bad] = CID_MISMATCH
    other = np.array([i for i in (5, 40, 300, stride() - 1, stride(), n - 1) if i < n and not bad[i]])
    cids[other, :38] = 0
    cids[other, :4] = np.frombuffer(bytes.fromhex("01711220"), dtype=np.uint8)  # (v1, dag-cbor, sha2-256, 32)
    cids[other, 4:36] = 0x5a
    cids[other, 4:8] = other.astype("<u4").view(np.uint8).reshape(-1, 4)  # (distinct CIDs)
    want[other] = CID_UNCHECKED
    return data, off, lens, cids, want


def k1_case(eng, corpus, n):
    data, off, lens, cids, want = corpus
    end = int(off[n - 1]) + int(lens[n - 1])
    with eng.witness(data[:end], off[:n], lens[:n], cids[:n]) as w:
        st, n_bad = w.verify_cids()
    assert np.array_equal(st, want[:n]), (np.nonzero(st != want[:n])[0][:10], st[st != want[:n]][:10])
    assert n_bad == int((want[:n] == CID_MISMATCH).sum())


@pytest.mark.parametrize("k1", [None, 0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_k1_tile_edges(engine, tuned, k1_corpus, n, k1):
    k1_case(pick(engine, tuned, k1, None if k1 is None else 0), k1_corpus, n)


@pytest.mark.parametrize("which", ["stride+1", "2*stride-1"])
def test_k1_stride_edges_at_residency_one(engine, tuned, k1_corpus, which):
    """stride + 1: workgroup 0 takes a second tile of one entry; 2·stride − 1: the last workgroup's second tile is partial
    and, on a grid of `stride / 256` workgroups, nobody has a third."""
    n = stride() + 1 if which == "stride+1" else 2 * stride() - 1
    k1_case(pick(engine, tuned, 1, 1), k1_corpus, n)


@pytest.mark.parametrize("k1", [None, 0])
def test_k1_same_witness_both_forms(engine, tuned, k1_corpus, k1):
    k1_case(pick(engine, tuned, k1, None if k1 is None else 0), k1_corpus, 2 * stride() - 1)


# ---------------------------------------------- the parse against the oracle ----------------------------------------------
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
    return want, o_st, o_has, np.asarray(o_trip, dtype=np.int64).reshape(-1, 3)


def run(eng, tip, ts, cl, blob, blob_len):
    """status bytes of the claims, the scan of the same witness (status, has-match map, match triples) and how often the
    parse was launched"""
    eng.profile_enable(True)
    eng.profile_reset()
    try:
        with eng.witness(tip.data, tip.off, tip.lens, tip.cids) as w:
            st = w.verify_event_claims(ts, cl, blob, blob_len)
            s_st, s_has, s_m, _ = w.scan_events(tip.receipts_root, tip.topic0, tip.topic1, actor=tip.filter_actor,
                                                want_touched=False)
            parses = eng.profile_read("event_scan")[0]
    finally:
        eng.profile_enable(False)
    trip = np.stack([s_m["exec_index"], s_m["event_index"], s_m["emitter"]], axis=1) if len(s_m) else np.zeros((0, 3))
    return st, s_st, s_has, np.asarray(trip, dtype=np.int64).reshape(-1, 3), parses


def check(answers, got):
    want, o_st, o_has, o_trip = answers
    st, s_st, s_has, trip, parses = got
    assert parses >= 1  # k_block_events ran
    assert np.array_equal(st, want), (np.nonzero(st != want)[0][:10], st[st != want][:10], want[st != want][:10])
    assert s_st == o_st == 1
    assert np.array_equal(s_has, o_has)
    assert np.array_equal(trip, o_trip)


def test_parse_tipset_crossing_one_stride(tuned, oracle):
    """Between one and two strides of blocks at residency 1: every workgroup has a second tile or none, the last tile is
    partial, and the pool partitions follow the logical wavefront number across both."""
    tip = Tipset(n_receipts=60_000, n_parents=3, n_planted=20, variety=1, max_events=6, no_events_permille=120,
                 seed=fuzz_seed(1810))
    assert stride() < tip.n_blocks < 2 * stride(), (tip.n_blocks, stride())
    ts, cl, blob, blob_len = packed(tip)
    answers = oracle_answers(oracle, tip, ts, cl, blob)
    assert (answers[0] == 1).sum() > len(answers[0]) // 2 and len(answers[3]) > 0
    check(answers, run(pick(None, tuned, 1, 1), tip, ts, cl, blob, blob_len))


@pytest.fixture(scope="module")
def small_tipset(oracle):
    tip = Tipset(n_receipts=300, n_parents=3, n_planted=20, variety=1, max_events=6, no_events_permille=120,
                 seed=fuzz_seed(1811))
    ts, cl, blob, blob_len = packed(tip)
    return tip, (ts, cl, blob, blob_len), oracle_answers(oracle, tip, ts, cl, blob)


@pytest.mark.parametrize("parse", [None, 0])
def test_parse_fewer_blocks_than_the_grid(engine, tuned, small_tipset, parse):
    """Fewer tiles than workgroups the residency allows: the grid is the tile count under both settings."""
    tip, p, answers = small_tipset
    assert tip.n_blocks < stride()
    check(answers, run(pick(engine, tuned, None if parse is None else 0, parse), tip, *p))


def test_parse_both_forms_agree(engine, tuned, oracle):
    tip = Tipset(n_receipts=6000, n_parents=3, n_planted=20, variety=1, max_events=6, no_events_permille=120,
                 seed=fuzz_seed(1812))
    ts, cl, blob, blob_len = packed(tip)
    answers = oracle_answers(oracle, tip, ts, cl, blob)
    a = run(pick(engine, tuned), tip, ts, cl, blob, blob_len)
    b = run(pick(engine, tuned, 0, 0), tip, ts, cl, blob, blob_len)
    for x, y in zip(a[:4], b[:4]):
        assert np.array_equal(x, y)
    check(answers, a)
    check(answers, b)


# --------------------------------------------------- the tuning keys ---------------------------------------------------
@pytest.mark.parametrize("key", ["k1_resident", "parse_resident"])
def test_tuning_keys_range(tuned, key):
    rc = lambda v: tuned.lib.ipcfp_ctx_set_tuning(tuned.h, key.encode(), v)
    assert rc(-1) == E_INVALID
    assert rc(17) == E_INVALID
    assert rc(16) == 0
    assert rc(0) == 0
