"""GPU: the table verifier's staging (csrc/kernels/verify_table.hip, verify_window.h) against the CPU oracle.

k_verify_events_table reads a wavefront's claims as one byte range through LDS, and the bytes its usual claims name in the
blob — when their extent fits the wavefront's window — as one byte range too; otherwise the wavefront keeps its per-lane
loads.  Which of the two a wavefront takes is decided by where the claims' entries lie in the blob and by nothing else, so
here packed claims (pack_event_claims) are verified after their blob was RE-LAID by hand: entries in reverse order, 4 KB
apart, shared by a whole wavefront, one lane's data at the far end, behind 1 … 15 junk bytes, from offset 0 to exactly
blob_len.  Re-laying does not change what a claim says: every expected status is the oracle's for the ORIGINAL batch.
Batches of 1, 63, 64, 65, 255, 256, 257 and 321 claims, honest ones mixed with the ladder's lies; claims that point outside
the blob in the middle of a wavefront; usual and other shapes lane by lane; two pairs claim by claim; claims at a device
pointer that is only 8-byte aligned — under fast_verify 1 and 0, with and without a filter.  Locations (the string entry
point lays the blob out itself: contiguous, staged) must equal those of the same claims interleaved with another pair's.
And the deferred TxMeta re-hash, which nothing in the call waits for but its end: a tipset whose only fault it finds, on
small tipsets, through verify_event_claims and verify_and_scan_device, and an honest call on the same context behind it.

No claim is ever left out of a comparison (`compare` asserts it)."""
import itertools

import numpy as np
import pytest

import ipc_filecoin_proofs_amd as ipcfp
from test_gpu_events import txmeta_blocks, with_block
from test_gpu_verify_ladder import NO_BLOCK, REACHED, Batch, compare, spec_of, world  # noqa: F401  (world: the fixture)

pytestmark = pytest.mark.gpu

BAD_CLAIM = 69          # IPCFP_ST_ERR_BAD_CLAIM
SIZES = [1, 63, 64, 65, 255, 256, 257, 321]
JUNK = 0xA5


# ---- packed batches ------------------------------------------------------------------------------------------------------
def pack(T, rows, n_topics=None, data_len=None, data=None):
    rows = np.asarray(rows, dtype=np.int64)
    nt = T.claim_ntopics[rows] if n_topics is None else np.asarray(n_topics, dtype=T.claim_ntopics.dtype)
    dl = T.claim_datalen[rows] if data_len is None else np.asarray(data_len, dtype=T.claim_datalen.dtype)
    dat = T.claim_data[rows] if data is None else data
    return ipcfp.pack_event_claims(T.parent_cids, T.child_cid, T.parent_epoch, T.child_epoch, T.claim_exec[rows], T.claim_event[rows],
                                   T.claim_emitter[rows], T.exec_order[T.claim_exec[rows].astype(np.int64)], nt, T.claim_topics[rows], dl, dat)


def tell_lies(cl, blob, every=3):
    """The ladder's lies, told on the packed form: claim k (k % every == 1) gets lie number k // every.  (All flags stay set:
    the oracle's packed entry point takes no others — the unparsable message and the data without 0x are told as strings
    in test_gpu_verify_ladder.py.)"""
    for k in range(1, len(cl), every):
        lie, nt = (k // every) % 12, int(cl["n_topics"][k])
        t_off, d_off, d_len = int(cl["topics_off"][k]), int(cl["data_off"][k]), int(cl["data_len"][k])
        if lie == 0:
            cl["child_epoch"][k] += 1
        elif lie == 1:
            cl["parent_epoch"][k] -= 1
        elif lie == 2:
            cl["event_index"][k] = 63
        elif lie == 3:
            cl["message_cid"][k, 20] ^= 0x10
        elif lie == 4:
            cl["exec_index"][k] += 1
        elif lie == 5:
            cl["event_index"][k] = 999
        elif lie == 6:
            cl["emitter"][k] += 1
        elif lie == 7 and nt == 2:
            cl["n_topics"][k] = 1
        elif lie == 8 and nt >= 1:
            blob[t_off + 5] ^= 0x40           # a byte of topic 0
        elif lie == 9 and nt >= 2:
            blob[t_off + 33 + 32] ^= 0x01     # the last byte of topic 1
        elif lie == 10 and d_len > 0:
            blob[d_off + d_len - 1] ^= 0x80
        elif lie == 11 and d_len > 0:
            cl["data_len"][k] = d_len - 1     # (the data is the last piece of the entry: the entry just ends a byte earlier)


def usual_batch(W, n, lies=True):
    rows = [i % W.n_rows for i in range(n)]   # the claim table in its own order, again from its head: every shape it has
    ts, cl, blob, blob_len = pack(W.a, rows)
    if lies:
        tell_lies(cl, blob)
    return ts, cl, blob, blob_len


# ---- re-laying the blob ----------------------------------------------------------------------------------------------------
def entries(cl, blob):
    return [(bytes(blob[int(c["topics_off"]): int(c["topics_off"]) + 33 * int(c["n_topics"])]),
             bytes(blob[int(c["data_off"]): int(c["data_off"]) + int(c["data_len"])])) for c in cl]


def relay(cl, blob, order=None, stride=0, prefix=0, share=False, far_data=(), slack=0):
    """The same claims over a blob laid out anew → (claims, blob, blob_len).  order: claim indices in the order their
    entries are laid down (default 0..n-1); stride: distance between entry starts (0: back to back); prefix: junk bytes
    in front; share: equal entries are laid down once; far_data: claims whose data goes to the very end of the blob, behind
    a gap no window spans; slack: junk bytes behind the last entry (0: the last entry ends the blob)."""
    ent = entries(cl, blob)
    n = len(cl)
    out = np.array(cl, copy=True)
    order = list(range(n)) if order is None else list(order)
    pieces, pos, seen = [], prefix, {}
    tail = []
    for i in order:
        topics, data = ent[i]
        here = data if i not in far_data else b""
        key = (topics, here)
        if share and key in seen and i not in far_data:
            t_off = seen[key]
        else:
            t_off = pos
            pieces.append((pos, topics + here))
            pos += max(len(topics) + len(here), stride)
            seen[key] = t_off
        out["topics_off"][i] = t_off
        out["data_off"][i] = t_off + len(topics)
        if i in far_data:
            tail.append(i)
    if tail:
        pos += 20000
        for i in tail:
            out["data_off"][i] = pos
            pieces.append((pos, ent[i][1]))
            pos += len(ent[i][1])
    if stride:  # (the last entry ends where its bytes end, not where the next one would start)
        pos = max(p + len(b) for p, b in pieces) if pieces else prefix
    new = np.full(pos + slack, JUNK, dtype=np.uint8)
    for p, b in pieces:
        new[p: p + len(b)] = np.frombuffer(b, dtype=np.uint8)
    assert entries(out, new) == ent  # the claims say what they said
    return out, new, pos + slack


def layouts(cl, blob):
    n = len(cl)
    yield "reverse order", relay(cl, blob, order=range(n - 1, -1, -1), slack=7)
    yield "4 KB apart", relay(cl, blob, stride=4096)
    yield "from 0 to exactly blob_len", relay(cl, blob)
    if n > 64:
        far = {70 % n}
        yield "one lane's data at the far end", relay(cl, blob, far_data=far, prefix=3)


def run_packed(W, ts, cl, blob, blob_len, want, what, fasts=(1, 0)):
    """every claim against `want` ({filter? → statuses}), under fast_verify 1 and 0, with and without a filter"""
    try:
        for fast, use_filter in itertools.product(fasts, (False, True)):
            W.engine.set_tuning("fast_verify", fast)
            got = W.w.verify_event_claims(ts, cl, blob, blob_len, filt=W.filt if use_filter else None)
            compare(got, want[use_filter], (what, "filter" if use_filter else "no filter", fast))
    finally:
        W.engine.set_tuning("fast_verify", -1)


def oracle_want(W, ts, cl, blob):
    return {f: W.st.verify_event_claims_packed(ts, cl, blob, filt=W.filt if f else None) for f in (False, True)}


@pytest.mark.parametrize("n", SIZES)
def test_relaid_blobs_at_every_batch_size(world, n):
    W = world
    ts, cl, blob, blob_len = usual_batch(W, n)
    want = oracle_want(W, ts, cl, blob)
    if n >= 63:
        assert (want[False] == 1).sum() > n // 3 and len(np.unique(want[False])) >= 6, np.unique(want[False])
    run_packed(W, ts, cl, blob, blob_len, want, ("size %d" % n, "as packed"))
    for name, (cl2, blob2, len2) in layouts(cl, blob):
        assert len(blob2) == len2   # not a byte behind blob_len
        run_packed(W, ts, cl2, blob2, len2, want, ("size %d" % n, name))


def test_junk_prefixes_start_windows_at_every_residue(world):
    W = world
    ts, cl, blob, blob_len = usual_batch(W, 130)
    want = oracle_want(W, ts, cl, blob)
    for prefix in range(1, 16):
        cl2, blob2, len2 = relay(cl, blob, prefix=prefix)
        assert int(cl2["topics_off"][0]) == prefix and len(blob2) == len2
        run_packed(W, ts, cl2, blob2, len2, want, ("prefix", prefix), fasts=(1,))


def test_a_wavefront_sharing_one_entry(world):
    """64 claims that name the same event — the same entry of the blob, laid down once: a window of 98 bytes"""
    W = world
    rows = [int(W.rows_usual[w % len(W.rows_usual)]) for w in range(3) for _ in range(64)] + [int(W.rows_one_topic[0])] * 5
    ts, cl, blob, blob_len = pack(W.a, rows)
    for k in range(2, len(cl), 5):      # lies that leave the entry alone
        cl["emitter"][k] += 1
    cl["event_index"][77] = 999
    want = oracle_want(W, ts, cl, blob)
    cl2, blob2, len2 = relay(cl, blob, share=True, prefix=9)
    assert len(np.unique(cl2["topics_off"])) == 4 and len2 < 9 + 4 * 98 + 1
    run_packed(W, ts, cl2, blob2, len2, want, "shared entry")
    assert (want[False] == 1).sum() > 100


def test_claims_that_point_outside_the_blob(world):
    """in the middle of a wavefront: ERR_BAD_CLAIM for them, the oracle's statuses for their neighbours"""
    W = world
    ts, cl, blob, blob_len = usual_batch(W, 200)
    want = oracle_want(W, ts, cl, blob)
    for name, (cl2, blob2, len2) in itertools.chain([("as packed", (cl, blob[:blob_len].copy(), blob_len))], layouts(cl, blob)):
        cl2 = np.array(cl2, copy=True)
        two = [int(k) for k in np.nonzero(cl2["n_topics"] == 2)[0] if 10 < k < 190]
        bad = two[:8]
        cl2["topics_off"][bad[0]] = 0xFFFFFFF0
        cl2["topics_off"][bad[1]] = len2 - 1
        cl2["data_off"][bad[2]] = 0xFFFFFFF0
        cl2["data_off"][bad[3]] = len2 - 1
        cl2["n_topics"][bad[4]] = 0xFFFFFFF0
        cl2["n_topics"][bad[5]] = (1 << 20) + 1
        cl2["topics_off"][bad[6]], cl2["data_off"][bad[6]] = 0xFFFFFFFF, 0xFFFFFFFF
        cl2["data_len"][bad[7]] = 0xFFFFFFF0
        w2 = {f: np.array(want[f], copy=True) for f in want}
        for f in w2:
            w2[f][bad] = BAD_CLAIM
        run_packed(W, ts, cl2, blob2, len2, w2, ("out of bounds", name))


def test_usual_and_other_shapes_lane_by_lane(world):
    """3 and 4 claimed topics, data of 0 / 33 / 100 bytes, alternating with the usual shape — on the packed and a reversed blob"""
    W = world
    a = W.a
    rows, nts, dls = [], [], []
    for k in range(140):
        kind = k % 7
        if kind in (0, 1):       # four topics claimed of four; three claimed of four
            rows.append(int(W.rows_wide[(k // 7) % len(W.rows_wide)]))
            nts.append(4 if kind == 0 else 3)
            dls.append(int(a.claim_datalen[rows[-1]]))
        else:                    # two topics, data of 32 (the usual claim) / 0 / 33 / 100 bytes
            rows.append(int(W.rows_usual[k % len(W.rows_usual)]))
            nts.append(2)
            dls.append((32, 0, 33, 100, 32)[kind - 2])
    dmax = max(100, a.claim_data.shape[1])
    data = np.full((len(rows), dmax), 0xAB, dtype=np.uint8)
    data[:, : a.claim_data.shape[1]] = a.claim_data[rows]
    ts, cl, blob, blob_len = pack(a, rows, n_topics=nts, data_len=dls, data=data)
    want = oracle_want(W, ts, cl, blob)
    got = want[False]
    assert (got[0::7] == 1).all() and (got[1::7] == 14).all() and (got[2::7] == 1).all()
    assert (got[3::7] == 16).all() and (got[4::7] == 16).all() and (got[5::7] == 16).all() and (got[6::7] == 1).all()
    run_packed(W, ts, cl, blob, blob_len, want, "mixed shapes")
    cl2, blob2, len2 = relay(cl, blob, order=range(len(cl) - 1, -1, -1), prefix=5)
    run_packed(W, ts, cl2, blob2, len2, want, ("mixed shapes", "reverse order"))


def test_two_pairs_claim_by_claim(world):
    """contexts differ within every wavefront: every claim takes the ladder of early returns — its claim still comes out of LDS"""
    W = world
    pa, pb = usual_batch(W, 130), pack(W.b, range(130))
    ts = np.concatenate([pa[0], pb[0]])
    cl = np.concatenate([pa[1], pb[1]])
    cl["tipset"][130:] = 1
    cl["topics_off"][130:] += pa[3]
    cl["data_off"][130:] += pa[3]
    blob = np.concatenate([pa[2][: pa[3]], pb[2]])
    blob_len = pa[3] + pb[3]
    order = np.argsort(np.concatenate([np.arange(130) * 2, np.arange(130) * 2 + 1]), kind="stable")
    cl = np.ascontiguousarray(cl[order])
    cl["emitter"][7::10] += 1
    want = oracle_want(W, ts, cl, blob)
    assert (want[False] == 1).sum() > 100
    run_packed(W, ts, cl, blob, blob_len, want, "two pairs")
    cl2, blob2, len2 = relay(cl, blob, order=range(len(cl) - 1, -1, -1))
    run_packed(W, ts, cl2, blob2, len2, want, ("two pairs", "reverse order"))


def test_claims_at_a_pointer_that_is_only_8_byte_aligned(world):
    import torch
    W = world
    for n in (65, 257):
        ts, cl, blob, blob_len = usual_batch(W, n)
        want = oracle_want(W, ts, cl, blob)[False]
        raw = np.ascontiguousarray(cl).view(np.uint8).reshape(-1)
        d_buf = torch.zeros(8 + raw.size, dtype=torch.uint8, device="cuda")
        assert d_buf.data_ptr() % 16 == 0
        d_buf[8:] = torch.from_numpy(raw).cuda()
        d_blob = torch.from_numpy(blob[:blob_len].copy()).cuda()
        try:
            for fast in (1, 0):
                W.engine.set_tuning("fast_verify", fast)
                d_st = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                W.w.verify_event_claims_device(ts, d_buf.data_ptr() + 8, n, d_blob.data_ptr(), blob_len, d_st.data_ptr())
                W.engine.sync()
                compare(d_st.cpu().numpy(), want, ("pointer + 8", n, fast))
        finally:
            W.engine.set_tuning("fast_verify", -1)


@pytest.mark.parametrize("n", [65, 257])
def test_locations_of_a_staged_run(world, n):
    """the string entry point lays the blob out itself (contiguous: every wavefront stages); the locations are those of
    the same claims interleaved with another pair's (two contexts in every wavefront: the ladder of early returns)"""
    W = world
    specs = [spec_of(W.a, i % W.n_rows) for i in range(n)]
    for k in range(0, n, 7):
        specs[k] = dict(specs[k], emitter=specs[k]["emitter"] + 1)
    for k in range(3, n, 11):
        specs[k] = dict(specs[k], topics=["0x" + "11" * 32] + specs[k]["topics"][1:])
    specs[n - 1] = dict(specs[n - 1], event_index=999)
    batch = Batch(specs)
    mixed = Batch([s for pair in zip(specs, itertools.cycle(W.filler)) for s in pair])
    try:
        for fast, use_filter in itertools.product((1, 0), (False, True)):
            filt = W.filt if use_filter else None
            W.engine.set_tuning("fast_verify", fast)
            tag = ("located", n, fast, use_filter)
            got, loc = W.w.verify_event_proofs_located(batch.arr, batch.n, filt=filt)
            compare(got, W.st.verify_event_proofs(batch, filt=filt, mode=0), tag)
            compare(W.w.verify_event_proofs(batch.arr, batch.n, filt=filt), got, tag + ("plain",))
            got_m, loc_m = W.w.verify_event_proofs_located(mixed.arr, mixed.n, filt=filt)
            compare(got_m, W.st.verify_event_proofs(mixed, filt=filt, mode=0), tag + ("interleaved",))
            for f in ("block", "off", "len"):
                assert np.array_equal(loc[f], loc_m[f][0::2]), tag + (f,)
            reached = np.isin(got, REACHED)
            assert reached.sum() > n // 3
            assert (loc["block"][reached] != NO_BLOCK).all() and (loc["block"][~reached] == NO_BLOCK).all(), tag
    finally:
        W.engine.set_tuning("fast_verify", -1)


def test_a_txmeta_that_does_not_rehash_to_its_cid(world, oracle):
    """The deferred re-hash (k_txmeta_rehash) is a launch of its own that no other kernel of the call waits for: wherever it
    is queued, its error lands before the call's one synchronisation, the call's results are those of fast_verify 0 and
    the oracle's, and an honest call on the same context afterwards is what it always was."""
    import torch
    W = world
    a = W.a
    tx = txmeta_blocks(a)
    b1 = a.block(tx[1])
    data, off, lens, cids = with_block(a, tx[1], b1[:1] + b1[44:87] + b1[1:44])   # the roots swapped: only the re-hash differs
    ts, cl, blob, blob_len = usual_batch(W, 200, lies=False)
    ost = oracle.store(data, off, lens, cids)
    want = ost.verify_event_claims_packed(ts, cl, blob)
    ost.close()
    assert (want == 67).all()   # ERR_TXMETA_MISMATCH, for every claim
    honest_want = oracle_want(W, ts, cl, blob)
    got = {}
    try:
        for fast in (1, 0):
            W.engine.set_tuning("fast_verify", fast)
            with W.engine.witness(data, off, lens, cids) as w:
                for rep in range(2):
                    got[fast, rep] = w.verify_event_claims(ts, cl, blob, blob_len)
                    compare(got[fast, rep], want, ("txmeta", fast, rep))
            with W.engine.witness(data, off, lens, cids) as w:
                d_cl = torch.from_numpy(np.ascontiguousarray(cl).view(np.uint8).reshape(-1)).cuda()
                d_blob = torch.from_numpy(blob[:blob_len].copy()).cuda()
                d_st = torch.full((len(cl),), 77, dtype=torch.uint8, device="cuda")
                d_has = torch.zeros(256 + 16, dtype=torch.uint8, device="cuda")
                d_m = torch.zeros(1024 * 40, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                w.verify_and_scan_device(ts, d_cl.data_ptr(), len(cl), d_blob.data_ptr(), blob_len, d_st.data_ptr(), a.topic0, a.topic1,
                                         None, d_has.data_ptr(), 256 + 16, d_m.data_ptr(), 1024)
                W.engine.sync()
                compare(d_st.cpu().numpy(), want, ("txmeta", "verify and scan", fast))
            # the same context, an honest witness right behind
            with W.engine.witness(a.data, a.off, a.lens, a.cids) as w:
                compare(w.verify_event_claims(ts, cl, blob, blob_len), honest_want[False], ("honest after txmeta", fast))
        assert np.array_equal(got[1, 0], got[0, 0])
    finally:
        W.engine.set_tuning("fast_verify", -1)
