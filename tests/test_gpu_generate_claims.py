"""GPU: generated matches lowered to packed claims on the device (kernels/event_claims_gen.hip,
ipcfp_event_claims_from_matches_device), the generator entry point that leaves them resident
(ipcfp_generate_event_claims) and the way from there to the verifier and to the wire.

The expected claims and blob are always `pack_event_proofs` of the strings tests/claims.py::extract_evm_log and
`Cid::to_string()` give — the repository's independent restatement of `find_matching_events`
(src/proofs/events/generator.rs:262-297, src/proofs/common/evm.rs:13-59); the code under test never supplies its own
expectation.  A record that cannot be lowered has no EventProof: its expected claim is written down here (tipset
0xffffffff, no flags, no blob bytes)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bundle_ref
import claims
import ipc_filecoin_proofs_amd as ipcfp
import pyamt
from event_spellings import spelling_cases
from ipc_filecoin_proofs_amd.binding import _table
from test_gpu_generate import tip  # noqa: F401  (the fixture: 3000 receipts, variety=1)
from test_gpu_limits import make_long_tip

pytestmark = pytest.mark.gpu

PARENT_EPOCH, CHILD_EPOCH = 4_000_123, 4_000_124
NO_BLOCK = 0xFFFFFFFF


class Spellings:
    """The cases packed several to a block so that the items start at every residue mod 16, the last item ending on the
    last byte of the last block; plus the records whose LOCATION is the trouble."""

    def __init__(self):
        cases = spelling_cases()
        blocks, cur, self.items = [], b"", []
        for k, (name, item, emitter, bad) in enumerate(cases):
            if len(cur) > 4000 or (cur and len(item) > 4000):
                blocks.append(cur)
                cur = b""
            cur += b"\x00" * ((k - len(cur)) % 16)  # filler in front: item k starts at residue k mod 16
            self.items.append(dict(name=name, block=len(blocks), off=len(cur), len=len(item), emitter=emitter, bad=bad, bytes=item))
            cur += item
        blocks.append(cur)
        assert {it["off"] % 16 for it in self.items} == set(range(16))
        last = self.items[-1]
        assert last["block"] == len(blocks) - 1 and last["off"] + last["len"] == len(blocks[-1])
        self.blocks = blocks
        self.data, self.off, self.lens = _table(blocks)
        self.cids = ipcfp.cid_slots([pyamt.cid_of(b) for b in blocks])
        # the restatement agrees with the case list about which events are no EVM log
        for it in self.items:
            assert (claims.extract_evm_log(it["bytes"]) is None) == it["bad"], it["name"]
        # locations out of range, and one item cut short by a byte (its last value overruns the item)
        big = next(it for it in self.items if it["name"] == "B d of 257")
        nb = len(blocks)
        self.items += [
            dict(name="block id == block count", block=nb, off=0, len=10, emitter=1, bad=True),
            dict(name="block id beyond", block=nb + 1000, off=0, len=10, emitter=2, bad=True),
            dict(name="no block", block=NO_BLOCK, off=0, len=0, emitter=3, bad=True),
            dict(name="off + len past the block's end", block=0, off=len(blocks[0]) - 10, len=20, emitter=4, bad=True),
            dict(name="off past the block's end", block=0, off=len(blocks[0]) + 1, len=1, emitter=5, bad=True),
            dict(name="cut short by one byte", block=big["block"], off=big["off"], len=big["len"] - 1, emitter=big["emitter"], bad=True),
            dict(name="one byte too many", block=self.items[0]["block"], off=self.items[0]["off"], len=self.items[0]["len"] + 1,
                 emitter=self.items[0]["emitter"], bad=True),
        ]
        rng = np.random.default_rng(0x6E6)
        self.msg = [bytes.fromhex("0171a0e40220") + rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in self.items]
        self.msg[2] = bytes.fromhex("0171c0e40240") + rng.integers(0, 256, 64, dtype=np.uint8).tobytes()  # 70 bytes: crosses folded
        self.msg[3] = b"\x12\x20" + rng.integers(0, 256, 32, dtype=np.uint8).tobytes()                   # CIDv0
        self.parents = [pyamt.cid_of(b"parent %d" % k) for k in range(3)]
        self.child = pyamt.cid_of(b"child")

    def batch(self, idx):
        """(match records, message slots, expected claims, expected blob) of the records idx (positions in self.items)"""
        m = np.zeros(len(idx), dtype=ipcfp.MATCH_DTYPE)
        slots = np.zeros((len(idx), 40), dtype=np.uint8)
        rows, good = [], []
        for k, i in enumerate(idx):
            it = self.items[i]
            m[k] = (3 * k + 1, 1000 - k if k < 1000 else k, it["emitter"], it["block"], it["off"], it["len"], 0)
            slots[k] = ipcfp.cid_slot(self.msg[i])
            if it["bad"]:
                continue
            em, topics, data = claims.extract_evm_log(it["bytes"])
            assert em == it["emitter"]
            good.append(k)
            rows.append(dict(parent_epoch=PARENT_EPOCH, child_epoch=CHILD_EPOCH,
                             parent_tipset_cids=[claims.cid_str(c) for c in self.parents], child_block_cid=claims.cid_str(self.child),
                             message_cid=ipcfp.cid_to_string(self.msg[i]) if len(self.msg[i]) == 34 else claims.cid_str(self.msg[i]),
                             exec_index=int(m["exec_index"][k]), event_index=int(m["event_index"][k]), emitter=it["emitter"],
                             topics=[claims.hex0x(t) for t in topics], data=claims.hex0x(data)))
        ev, _ = bundle_ref.claims_from_parsed({"event_proofs": rows, "storage_proofs": []})
        _, cl, blob = ipcfp.pack_event_proofs(ev.arr, ev.n)
        want = np.zeros(len(idx), dtype=ipcfp.CLAIM_DTYPE)
        want["parent_epoch"], want["child_epoch"] = PARENT_EPOCH, CHILD_EPOCH
        want["exec_index"], want["event_index"], want["emitter"] = m["exec_index"], m["event_index"], m["emitter"]
        want["message_cid"] = slots
        want["tipset"] = NO_BLOCK      # the record that cannot be lowered; the good ones are overwritten below
        if good:
            want[np.array(good)] = cl  # (a record without blob bytes moves nobody's offsets: the blob is in claim order)
        return m, slots, want, blob


@pytest.fixture(scope="module")
def spell():
    return Spellings()


@pytest.fixture(scope="module")
def spell_witness(engine, spell):
    w = engine.witness(spell.data, spell.off, spell.lens, spell.cids)
    yield w
    w.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def lower(w, m, slots, cap=None, canary=0xA5, slack=64):
    """sizing call, then the fill → (rc, blob length of the sizing call, claims, blob buffer incl. slack)"""
    n = len(m)
    d_m, d_s = dev(m), dev(slots)
    rc, size = w.event_claims_from_matches_device(d_m.data_ptr() if n else 0, n, d_s.data_ptr() if n else 0, PARENT_EPOCH, CHILD_EPOCH,
                                                  0, 0, 0, 0)
    assert rc == 0
    cap = size if cap is None else cap
    d_cl = torch.full((max(n, 1) * ipcfp.CLAIM_DTYPE.itemsize,), canary, dtype=torch.uint8, device="cuda")
    d_bl = torch.full((max(cap, 0) + slack,), canary, dtype=torch.uint8, device="cuda")
    rc, size2 = w.event_claims_from_matches_device(d_m.data_ptr() if n else 0, n, d_s.data_ptr() if n else 0, PARENT_EPOCH, CHILD_EPOCH,
                                                   0, d_cl.data_ptr(), d_bl.data_ptr(), cap)
    assert size2 == size
    got_cl = d_cl.cpu().numpy()[: n * ipcfp.CLAIM_DTYPE.itemsize].view(ipcfp.CLAIM_DTYPE)
    return rc, size, got_cl, d_bl.cpu().numpy()


def check_batch(w, spell, idx):
    m, slots, want, blob = spell.batch(idx)
    rc, size, got_cl, got_bl = lower(w, m, slots)
    assert rc == 0 and size == len(blob)
    bad = [k for k in range(len(idx)) if got_cl[k].tobytes() != want[k].tobytes()]
    assert not bad, [(spell.items[idx[k]]["name"], got_cl[k], want[k]) for k in bad[:3]]
    for k, i in enumerate(idx):  # name the case whose bytes are wrong
        o, e = int(want["topics_off"][k]), int(want["data_off"][k]) + int(want["data_len"][k])
        if not spell.items[i]["bad"]:
            assert got_bl[o:e].tobytes() == blob[o:e].tobytes(), spell.items[i]["name"]
    assert got_bl[:size].tobytes() == blob.tobytes()
    assert (got_bl[size:] == 0xA5).all()
    return want, blob


def test_every_spelling(spell_witness, spell):
    idx = list(range(len(spell.items)))
    want, blob = check_batch(spell_witness, spell, idx)
    n_bad = sum(1 for it in spell.items if it["bad"])
    assert n_bad >= 10 and (want["tipset"] == NO_BLOCK).sum() == n_bad
    assert want["n_topics"].max() == 9 and want["data_len"].max() == 70000 and len(blob) > 3 * 65536
    # a good record WITHOUT blob bytes: a Case A log with an empty topics value and no data
    k = next(i for i, it in enumerate(spell.items) if it["name"] == "A topics of 0 without data")
    assert want["tipset"][k] == 0 and want["flags"][k] == 3 and want["n_topics"][k] == 0 and want["data_len"][k] == 0
    # the folded message slot stayed folded
    assert want["message_cid"][2, 0] == 0xFF and want["flags"][2] == 3


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_sizes(spell_witness, spell, n):
    """one lane short of a wavefront, exactly one, one more, more than a workgroup — by repetition of the case list, which
    is rotated so that a batch of one is not always the same record"""
    idx = [int(i) for i in np.resize(np.roll(np.arange(len(spell.items)), -5), n)]
    check_batch(spell_witness, spell, idx)


def test_only_bad_records(spell_witness, spell):
    idx = [i for i, it in enumerate(spell.items) if it["bad"]]
    want, blob = check_batch(spell_witness, spell, idx)
    assert len(blob) == 0 and (want["flags"] == 0).all()


def test_buffer_contract(engine, spell_witness, spell):
    w = spell_witness
    idx = list(range(20))
    m, slots, want, blob = spell.batch(idx)
    # a short buffer: IPCFP_E_INVALID, the exact length reported, neither buffer touched
    rc, size, got_cl, got_bl = lower(w, m, slots, cap=len(blob) - 1)
    assert rc == -1 and size == len(blob)
    assert (got_bl == 0xA5).all() and (got_cl.view(np.uint8) == 0xA5).all()
    rc, size, got_cl, got_bl = lower(w, m, slots, cap=0)
    assert rc == -1 and (got_bl == 0xA5).all()
    # room to spare: only the blob's bytes are written
    rc, size, got_cl, got_bl = lower(w, m, slots, cap=len(blob) + 1000)
    assert rc == 0 and got_bl[:size].tobytes() == blob.tobytes() and (got_bl[size:] == 0xA5).all()
    assert got_cl.tobytes() == want.tobytes()
    # a blob buffer that is not on a 16-byte boundary
    d_m, d_s = dev(m), dev(slots)
    d_cl = torch.zeros(len(m) * ipcfp.CLAIM_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_bl = torch.full((len(blob) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    rc, size = w.event_claims_from_matches_device(d_m.data_ptr(), len(m), d_s.data_ptr(), PARENT_EPOCH, CHILD_EPOCH, 0, d_cl.data_ptr(),
                                                  d_bl.data_ptr() + 5, len(blob))
    out = d_bl.cpu().numpy()
    assert rc == 0 and out[5:5 + size].tobytes() == blob.tobytes() and (out[:5] == 0xA5).all() and (out[5 + size:] == 0xA5).all()
    # a capacity without a buffer, and the context is whole afterwards
    rc, _ = w.event_claims_from_matches_device(d_m.data_ptr(), len(m), d_s.data_ptr(), PARENT_EPOCH, CHILD_EPOCH, 0, d_cl.data_ptr(), 0, 7)
    assert rc == -1
    check_batch(w, spell, idx)


def test_bad_records_verify_as_bad_claims(engine, spell_witness, spell):
    """the convention of ipcfp_expand_event_claims_device: tipset 0xffffffff is ERR_BAD_CLAIM, never followed"""
    idx = [i for i, it in enumerate(spell.items) if it["bad"]][:6]
    m, slots, want, blob = spell.batch(idx)
    ts = np.zeros(1, dtype=ipcfp.TIPSET_DTYPE)
    ts["flags"], ts["n_parents"] = 3, len(spell.parents)
    ts["child"][0] = ipcfp.cid_slot(spell.child)
    for k, c in enumerate(spell.parents):
        ts["parents"][0, k] = ipcfp.cid_slot(c)
    d_cl, d_st = dev(want), torch.zeros(len(idx), dtype=torch.uint8, device="cuda")
    d_bl = torch.zeros(16, dtype=torch.uint8, device="cuda")
    spell_witness.verify_event_claims_device(ts, d_cl.data_ptr(), len(idx), d_bl.data_ptr(), 0, d_st.data_ptr())
    assert (d_st.cpu().numpy() == ipcfp.ST.ERR_BAD_CLAIM).all()


# ---- the generator ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def full(tip, engine):  # noqa: F811
    w = engine.witness(tip.data, tip.off, tip.lens, tip.cids)
    yield w
    w.close()


def tipset_fields(ts):
    return [(int(ts["flags"][k]), int(ts["n_parents"][k]), ts["child"][k].tobytes(), ts["parents"][k].tobytes()) for k in range(len(ts))]


@pytest.mark.parametrize("actor", ["filter", None])
def test_generate_event_claims(tip, full, engine, oracle, actor):  # noqa: F811
    w = full
    a = tip.filter_actor if actor == "filter" else None
    gs, gm, gmsg, gids = w.generate_event_proofs(tip.parent_cids, tip.child_cid, tip.topic0, tip.topic1, actor=a)
    st, g = w.generate_event_claims(tip.parent_cids, tip.child_cid, tip.topic0, tip.topic1, actor=a)
    assert st == gs == 1 and g is not None
    try:
        ec = claims.EventClaims(tip, generated=(gm, gmsg))
        ts, cl, blob = ipcfp.pack_event_proofs(ec.arr, ec.n)
        assert g.n == len(gm) > 0 and g.blob_len == len(blob)
        got_cl, got_bl = g.copy()
        assert got_cl.tobytes() == cl.tobytes()
        assert got_bl.tobytes() == blob.tobytes()
        assert tipset_fields(g.tipsets) == tipset_fields(ts)
        m, msg = g.matches()
        assert m.tobytes() == gm.tobytes() and np.array_equal(msg, gmsg)
        assert np.array_equal(g.block_ids, gids)
        # round trip without the host: the handle's own device pointers against the pruned witness it names
        sub = g.block_ids.astype(np.int64)
        d_st = torch.zeros(g.n, dtype=torch.uint8, device="cuda")
        with engine.witness(tip.data, tip.off[sub], tip.lens[sub], tip.cids[sub]) as pw:
            pw.verify_event_claims_device(g.tipsets, g.claims_ptr, g.n, g.blob_ptr, g.blob_len, d_st.data_ptr())
        got = d_st.cpu().numpy()
        assert (got == 1).all(), got.tolist()
        pst = oracle.store(tip.data, tip.off[sub], tip.lens[sub], tip.cids[sub])
        assert np.array_equal(got, pst.verify_event_proofs(ec, mode=0))
        pst.close()
        # to the wire: the handle's strings through the bundle writer
        p, n = g.proofs()
        assert n == g.n
        text = w.write_bundle_json(None, 0, p, n, block_ids=g.block_ids)
        blocks = [(tip.cids[i, :38].tobytes(), tip.block(i)) for i in g.block_ids]
        assert text == bundle_ref.bundle_json([], bundle_ref.event_dicts(tip, generated=(gm, gmsg)), blocks).encode()
        b = engine.bundle(text)
        try:
            ss, es = b.verify()
        finally:
            b.close()
        assert len(es) == g.n and (es == 1).all() and len(ss) == 0
        # the strings through the string verifier, too
        assert (w.verify_event_proofs(p, n) == 1).all()
    finally:
        g.close()


def test_generate_event_claims_no_match(tip, full):  # noqa: F811
    gs, gm, gmsg, gids = full.generate_event_proofs(tip.parent_cids, tip.child_cid, bytes(32), tip.topic1)
    st, g = full.generate_event_claims(tip.parent_cids, tip.child_cid, bytes(32), tip.topic1)
    assert st == gs == 1 and g is not None
    try:
        assert g.n == 0 and g.blob_len == 0 and len(gm) == 0
        cl, bl = g.copy()
        assert len(cl) == 0 and len(bl) == 0
        assert np.array_equal(g.block_ids, gids) and len(gids) > 3
        p, n = g.proofs()
        assert n == 0
    finally:
        g.close()


def test_generate_event_claims_errors(tip, engine):  # noqa: F811
    """the error cases of test_generate_event_proofs_errors: the old call's status, and no handle"""
    bogus = b"\x01\x71\xa0\xe4\x02\x20" + bytes(range(32))
    cases = [
        ("missing child", None, tip.parent_cids, bogus),
        ("child is not a header", None, tip.parent_cids, tip.receipts_root),
        ("parent is not a header", None, [tip.parent_cids[0], tip.receipts_root], tip.child_cid),
        ("missing parent", None, [bogus], tip.child_cid),
        ("no receipts root", tip.find_block(tip.receipts_root), tip.parent_cids, tip.child_cid),
    ]
    for name, drop, parents, child in cases:
        keep = np.ones(tip.n_blocks, dtype=bool)
        if drop is not None:
            keep[drop] = False
        idx = np.nonzero(keep)[0]
        with engine.witness(tip.data, tip.off[idx], tip.lens[idx], tip.cids[idx]) as w:
            gs, gm, _, gids = w.generate_event_proofs(parents, child, tip.topic0, tip.topic1)
            st, g = w.generate_event_claims(parents, child, tip.topic0, tip.topic1)
            assert st == gs and st >= 64 and g is None, (name, st, gs)


def test_long_cids(engine):
    """CIDs longer than the slot: the claims carry the folds, equal the lowering of the long CID strings and verify; the
    string form does not exist (the bytes of a folded CID are not in the claim)."""
    tip, rw = make_long_tip()  # noqa: F811
    data, off, lens = rw.tables()
    slots = ipcfp.cid_slots(rw.cids)
    child_long = rw.renamed[tip.child_cid[:38]]
    with engine.witness(data, off, lens, slots) as w:
        gs, gm, gmsg, gids = w.generate_event_proofs(tip.parent_cids, child_long, tip.topic0, tip.topic1, actor=tip.filter_actor)
        st, g = w.generate_event_claims(tip.parent_cids, child_long, tip.topic0, tip.topic1, actor=tip.filter_actor)
        assert st == gs == 1 and g is not None and g.n == len(gm) > 0
        try:
            rows = []
            for k in range(len(gm)):
                o = int(off[gm["block"][k]]) + int(gm["off"][k])
                em, topics, dat = claims.extract_evm_log(data[o:o + int(gm["len"][k])].tobytes())
                assert em == int(gm["emitter"][k])
                rows.append(dict(parent_epoch=tip.parent_epoch, child_epoch=tip.child_epoch,
                                 parent_tipset_cids=[claims.cid_str(c) for c in tip.parent_cids], child_block_cid=rw.s(tip.child_cid),
                                 message_cid=rw.s(tip.exec_order[int(gm["exec_index"][k])]), exec_index=int(gm["exec_index"][k]),
                                 event_index=int(gm["event_index"][k]), emitter=em, topics=[claims.hex0x(t) for t in topics],
                                 data=claims.hex0x(dat)))
            ev, _ = bundle_ref.claims_from_parsed({"event_proofs": rows, "storage_proofs": []})
            ts, cl, blob = ipcfp.pack_event_proofs(ev.arr, ev.n)
            got_cl, got_bl = g.copy()
            assert got_cl.tobytes() == cl.tobytes() and got_bl.tobytes() == blob.tobytes()
            assert tipset_fields(g.tipsets) == tipset_fields(ts)
            assert g.tipsets["child"][0, 0] == 0xFF                 # the child header's CID is folded …
            assert (got_cl["message_cid"][:, 0] == 0xFF).any()        # … and so is at least one message CID
            d_st = torch.zeros(g.n, dtype=torch.uint8, device="cuda")
            w.verify_event_claims_device(g.tipsets, g.claims_ptr, g.n, g.blob_ptr, g.blob_len, d_st.data_ptr())
            assert (d_st.cpu().numpy() == 1).all()
            with pytest.raises(ipcfp.EngineError) as e:
                g.proofs()
            assert e.value.rc == -5 and e.value.bad_index == 0  # the child's CID is every proof's: the first proof is named
        finally:
            g.close()
