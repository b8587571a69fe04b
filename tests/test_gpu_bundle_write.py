"""GPU: the bundle WRITER through the C ABI (ipcfp_bundle_write_json: claim strings on the host, every ProofBlock — frame,
decimal CID bytes, base64 — on the device, kernels/base64_encode.hip).  The expected text always comes from
tests/bundle_ref.py's writer (json.dumps(ensure_ascii=False) for the claims where escapes matter), never from the engine."""
import ctypes as C
import hashlib
import os
import re

import numpy as np
import pytest

from conftest import fuzz_seed

import bundle_ref
import claims
import ipc_filecoin_proofs_amd as ipcfp
from bundle_write_cases import arrays, event_proof, head_text, storage_proof
from tools.synth import Tipset

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bundle_small.json")
CHAIN_PREFIX = bytes.fromhex("0171a0e40220")


def witness_of(engine, blocks):
    return engine.witness(*bundle_ref.tables_from_blocks(blocks))


def write(w, storage=(), events=(), block_ids=None) -> bytes:
    st, ev = arrays(list(storage), list(events))
    return w.write_bundle_json(st.arr, st.n, ev.arr, ev.n, block_ids=block_ids)


def expect(storage, events, blocks) -> bytes:
    return head_text(list(storage), list(events)) + ",".join(bundle_ref.block_json(c, d) for c, d in blocks).encode() + b"]}"


@pytest.fixture(scope="module")
def shapes(oracle):
    """Every block length at which the encoder takes another path (tails 0..11, one wavefront of units = 768 bytes, more
    than one workgroup), empty blocks next to each other and last, and every shape of CID a 40-byte slot can hold."""
    rng = np.random.default_rng(fuzz_seed(0xB64))
    lens = list(range(0, 101)) + [127, 128, 129, 767, 768, 769, 1000, 4096, 65537]
    blocks = []
    for n in lens:
        d = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        blocks.append((bytes(oracle.cid_for_block(d))[:38], d))
    d = rng.integers(0, 256, 50, dtype=np.uint8).tobytes()
    blocks.append((b"\x12\x20" + hashlib.sha256(d).digest(), d))                      # CIDv0, 34 bytes
    blocks.append((bytes.fromhex("01551220") + hashlib.sha256(d).digest(), d + b"x"))  # v1 raw sha2-256, 36 bytes
    blocks.append((bytes.fromhex("01550000"), b""))                                   # identity, 4 bytes
    widths = bytes([0, 9, 10, 99, 100, 255, 1, 199, 200, 7, 70, 170] + list(range(20, 40)))
    blocks.append((CHAIN_PREFIX + widths, rng.integers(0, 256, 13, dtype=np.uint8).tobytes()))
    blocks.append((CHAIN_PREFIX + bytes(range(100, 132)), b""))                       # two adjacent empty blocks …
    blocks.append((CHAIN_PREFIX + bytes(range(101, 133)), b""))
    blocks.append((CHAIN_PREFIX + bytes(range(1, 33)), b"abc"))
    blocks.append((CHAIN_PREFIX + bytes(range(2, 34)), b""))                          # … and an empty block last
    assert len({c for c, _ in blocks}) == len(blocks)
    return blocks


@pytest.fixture(scope="module")
def shapes_witness(engine, shapes):
    w = witness_of(engine, shapes)
    yield w
    w.close()


def test_every_shape_byte_for_byte(shapes_witness, shapes):
    filler = []
    while True:
        want = expect(filler, [], shapes)
        # the test's OWN expected text: the base64 bodies must start at all 16 residues mod 16 (every alignment of the
        # unaligned 16-character stores); filler claims shift the block part until they do
        starts = {(m.end() % 16) for m in re.finditer(rb'"data":"', want[want.index(b'"blocks":['):])}
        if len(starts) == 16 or len(filler) > 16:
            break
        filler.append(storage_proof(actor_id=len(filler)))
    assert len(starts) == 16
    got = write(shapes_witness, filler)
    assert got == want
    if not filler:
        assert got == bundle_ref.bundle_json([], [], shapes).encode()
    parsed = bundle_ref.parse_bundle(got)
    assert parsed["blocks"] == shapes


def test_block_lists(engine, shapes_witness, shapes):
    w, n = shapes_witness, len(shapes)
    rng = np.random.default_rng(fuzz_seed(0xB65))
    assert write(w, block_ids=np.arange(n)) == write(w, block_ids=None) == expect([], [], shapes)
    sub = rng.permutation(n)[: n // 2]
    assert write(w, block_ids=sub) == expect([], [], [shapes[i] for i in sub])
    rep = [108, 3, 108, 108, n - 1, 0, 3, n - 1]
    assert write(w, block_ids=rep) == expect([], [], [shapes[i] for i in rep])
    assert write(w, block_ids=[]) == b'{"storage_proofs":[],"event_proofs":[],"blocks":[]}'
    assert write(w, [storage_proof()], [event_proof()], block_ids=[]) == expect([storage_proof()], [event_proof()], [])
    # an id equal to the block count: refused, the position named; the context is whole afterwards
    for bad_list, at in (([0, 1, n, 2], 2), ([5] * 700 + [n] + [6] * 700 + [n + 7], 700), ([0xFFFFFFFF], 0)):
        with pytest.raises(ipcfp.EngineError) as e:
            write(w, block_ids=bad_list)
        assert "(-1)" in str(e.value) and "block_ids[%d]" % at in str(e.value), str(e.value)
        assert write(w, block_ids=[2, 1]) == expect([], [], [shapes[2], shapes[1]])
    # block_ids == NULL needs n_blocks == the witness's count
    lib, nn = engine.lib, C.c_uint64()
    assert lib.ipcfp_bundle_write_json(engine.h, w.h, None, 0, None, 0, None, n - 1, None, 0, C.byref(nn)) == -1
    assert write(w, block_ids=[7]) == expect([], [], [shapes[7]])


def test_folded_and_malformed_cid_slots(engine, shapes):
    blocks = shapes[40:60]
    data, off, lens, cids = bundle_ref.tables_from_blocks(blocks)
    long_cid = bytes.fromhex("0171c0e40240") + hashlib.blake2b(b"long", digest_size=64).digest()  # blake2b-512: 70 bytes
    cids[11] = ipcfp.cid_slot(long_cid)
    assert cids[11, 0] == 0xFF and cids[11, 1] == 70
    cids[17, 39] = 1          # a well-formed 38-byte CID followed by something that is not padding
    cids[18, :4] = (1, 0x71, 0x12, 0x30)  # the multihash says 48 digest bytes: more than the slot holds
    with engine.witness(data, off, lens, cids) as w:
        good = [i for i in range(len(blocks)) if i not in (11, 17, 18)]
        for ids, at, code in ((None, 11, -5), ([3, 4, 11, 17], 2, -5), ([17, 11], 0, -1), ([0, 18, 11], 1, -1)):
            with pytest.raises(ipcfp.EngineError) as e:
                write(w, block_ids=ids)
            assert "(%d)" % code in str(e.value) and "block_ids[%d]" % at in str(e.value), str(e.value)
            # the same witness WITHOUT those blocks: written, and the context is whole
            assert write(w, block_ids=good) == expect([], [], [blocks[i] for i in good])


def test_buffer_contract(engine, shapes_witness, shapes):
    w, lib = shapes_witness, engine.lib
    ids = np.array([3, 64, 110, 0, 108], dtype=np.uint32)
    storage, events = [storage_proof()], [event_proof(), event_proof(topics=[])]
    want = expect(storage, events, [shapes[i] for i in ids])
    st, ev = arrays(storage, events)

    def call(out, cap):
        n = C.c_uint64(0xDEAD)
        rc = lib.ipcfp_bundle_write_json(engine.h, w.h, C.cast(st.arr, C.c_void_p), st.n, C.cast(ev.arr, C.c_void_p), ev.n,
                                         ids.ctypes.data_as(C.c_void_p), len(ids), out, cap, C.byref(n))
        return rc, int(n.value)

    rc, n = call(None, 0)
    assert rc == 0 and n == len(want)
    buf = np.full(n + 64, 0xA5, dtype=np.uint8)
    rc, n2 = call(buf.ctypes.data_as(C.c_void_p), n)
    assert rc == 0 and n2 == n
    assert buf[:n].tobytes() == want and (buf[n:] == 0xA5).all()
    buf = np.full(n + 64, 0xA5, dtype=np.uint8)
    rc, n3 = call(buf.ctypes.data_as(C.c_void_p), n - 1)
    assert rc == -1 and n3 == n
    assert (buf == 0xA5).all()
    rc, _ = call(None, 5)
    assert rc == -1


def test_golden_round_trip(engine):
    text = open(GOLDEN, "rb").read()
    b = engine.bundle(text)
    try:
        assert b.n_blocks == 71
        assert b.to_json() == text
    finally:
        b.close()


def test_claim_escapes_in_a_whole_bundle(shapes_witness, shapes):
    every = "".join(chr(c) for c in range(1, 0x80))
    storage = [storage_proof(value=every + "\u00e9\u2028\U0001F600")]
    events = [event_proof(topics=[every, "\\\"/"], data="\u00e9")]
    assert write(shapes_witness, storage, events, block_ids=[1, 2]) == expect(storage, events, [shapes[1], shapes[2]])


@pytest.fixture(scope="module")
def tip():
    return Tipset(n_receipts=3000, n_parents=3, dup_permille=60, n_planted=7, variety=1, max_events=5,
                  no_events_permille=100, n_actors=3000, n_contracts=8, slots_per_contract=12, storage_layout_mix=1,
                  n_actor_queries=12)


def test_generate_write_parse_verify(tip, engine, oracle):
    """generate_event_proofs / generate_storage_proofs → the engine's own JSON → parse (device base64 decode) → verify."""
    w = engine.witness(tip.data, tip.off, tip.lens, tip.cids)
    try:
        gs, gm, gmsg, gids = w.generate_event_proofs(tip.parent_cids, tip.child_cid, tip.topic0, tip.topic1)
        assert gs == 1 and len(gm) > 0
        sidx = list(range(len(tip.sc_actor)))
        out, sids = w.generate_storage_proofs(tip.child_cid, tip.sc_actor, tip.sc_slot)
        assert (out["status"] == 1).all()
        ids = sorted(set(gids.tolist()) | set(sids.tolist()), key=lambda i: tip.cids[i, 6:38].tobytes())
        ec = claims.EventClaims(tip, generated=(gm, gmsg))
        sc = claims.StorageClaims(tip, indices=sidx)
        text = w.write_bundle_json(sc.arr, sc.n, ec.arr, ec.n, block_ids=ids)
    finally:
        w.close()
    blocks = [(tip.cids[i, :38].tobytes(), tip.block(i)) for i in ids]
    events = bundle_ref.event_dicts(tip, generated=(gm, gmsg))
    storage = bundle_ref.storage_dicts(tip, sidx)
    assert text == bundle_ref.bundle_json(storage, events, blocks).encode()
    b = engine.bundle(text)
    try:
        assert (b.n_blocks, b.n_events, b.n_storage) == (len(blocks), len(events), len(storage))
        st, bad = b.witness.verify_cids()
        assert bad == 0
        ss, es = b.verify()
    finally:
        b.close()
    parsed = bundle_ref.parse_bundle(text)
    ev, sg = bundle_ref.claims_from_parsed(parsed)
    pst = oracle.store(*bundle_ref.tables_from_blocks(parsed["blocks"]))
    want_e = pst.verify_event_proofs(ev, mode=0)
    want_s = pst.verify_storage_proofs(sg, mode=0)
    pst.close()
    assert np.array_equal(es, want_e) and np.array_equal(ss, want_s)
    assert (es == 1).all() and (ss == 1).all() and len(es) == len(gm) and len(ss) == len(sidx)


def random_cid(rng) -> bytes:
    k = int(rng.integers(0, 10))
    digest = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    if k == 0:
        return b"\x12\x20" + digest
    if k == 1:
        return bytes.fromhex("01551220") + digest
    if k == 2:
        n = int(rng.integers(0, 33))
        return bytes([1, 0x55, 0, n]) + digest[:n]   # identity multihash of any length
    return CHAIN_PREFIX + digest


def test_fuzz_against_the_restated_writer(engine):
    rng = np.random.default_rng(fuzz_seed(0xB66))
    for rnd in range(40):
        n = int(rng.integers(1, 301))
        lens = np.where(rng.random(n) < 0.7, rng.integers(0, 41, n), np.minimum(rng.geometric(1 / 400.0, n), 5000))
        blocks, seen = [], set()
        for ln in lens:
            c = random_cid(rng)
            while c in seen:
                c = random_cid(rng)
            seen.add(c)
            blocks.append((c, rng.integers(0, 256, int(ln), dtype=np.uint8).tobytes()))
        ids = rng.integers(0, n, int(rng.integers(0, 2 * n + 1)))
        k = int(rng.integers(0, 4))          # 0..3 claims, split between the two lists
        ns = int(rng.integers(0, k + 1))
        storage = [storage_proof(actor_id=int(rng.integers(0, 1 << 63)), slot="s" * int(rng.integers(0, 70))) for _ in range(ns)]
        events = [event_proof(child_epoch=int(rng.integers(-(1 << 62), 1 << 62)), topics=["t\n"] * int(rng.integers(0, 5)))
                  for _ in range(k - ns)]
        with witness_of(engine, blocks) as w:
            got = write(w, storage, events, block_ids=ids)
            assert got == expect(storage, events, [blocks[i] for i in ids]), (rnd, n, len(ids))
            if rnd % 8 == 0:
                assert write(w, storage, events) == expect(storage, events, blocks), rnd
