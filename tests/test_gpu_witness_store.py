"""GPU: the crafted-key cases of tests/witness_store_cases.py through the engine.

A (the CID index) and D (the block table) go through EVERY constructor — `engine.witness`, `witness_device`,
`witness_packed` (crafted blake2b CIDs travel as digests, every other form as an escape), `subset` of a superset, a bundle's
JSON, and growth by `put_keyed` — and once more after `rebuild_index()`: `has` (statuses AND block ids), `get`, `amt_get`
(the recording probe of a walk kernel), `read_values` over (block, 0, len) and `verify_cids`, all against the dict / hashlib
answers written next to the cases.  B (the seen-set) goes through `exec_order` (the literal order), the string route, the
packed routes fast and general (`k_exec_insert_flags`; `k_exec_insert` + `k_exec_first`), verify-and-scan and
`generate_event_proofs`.  Each case has a witness of its own; A also runs merged into one witness.  Comparisons are exact."""
import hashlib

import numpy as np
import pytest
import torch

import bundle_ref
import event_chain_cases as ec
import ipc_filecoin_proofs_amd as ipcfp
import pyamt
import test_gpu_event_chain as gec
import witness_store_cases as ws

pytestmark = pytest.mark.gpu

NO_BLOCK = 0xFFFFFFFF
CONSTRUCTORS = ("witness", "device", "packed", "subset", "json")
A_NAMES, D_NAMES, B_NAMES = list(ws.A_CASES), list(ws.D_CASES), list(ws.B_CASES)
STD = ipcfp.STD_CID_PREFIX


class Built:
    """a witness and what has to outlive it"""

    def __init__(self, w, keep=()):
        self.w, self.keep = w, list(keep)

    def __enter__(self):
        return self.w

    def __exit__(self, *a):
        self.w.close()
        for k in self.keep:
            k.close()


def foreign(i: int) -> bytes:
    return b"\x82\x18\x2a" + bytes([i & 0xFF]) * (1 + (i * 37) % 300)


def construct(engine, how, data, off, lens, cids40, cids):
    """`cids`: the binary CIDs themselves (a bundle's JSON carries them at their own length)"""
    n = len(lens)
    if how == "witness":
        return Built(engine.witness(data, off, lens, cids40))
    if how == "device":
        t = [torch.from_numpy(np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), np.zeros(64, np.uint8)])).cuda()
             for a in (data, off, lens, cids40)]  # (never an empty allocation)
        torch.cuda.synchronize()
        b = Built(engine.witness_device(t[0].data_ptr(), data.size, t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(), n))
        b.tensors = t
        return b
    if how == "packed":
        pk = ipcfp.PackedWitnessTables(data, off, lens, cids40)
        std = [bytes(c[:6]) == STD and not c[38:].any() for c in cids40]
        assert pk.esc_index.tolist() == [i for i, s in enumerate(std) if not s]
        return Built(engine.witness_packed(pk))
    if how == "subset":
        # the case's blocks at the odd positions of a superset twice as large, a foreign block in front of each
        blocks, cids = [], []
        for i in range(n):
            f = foreign(i)
            blocks += [f, data[int(off[i]): int(off[i]) + int(lens[i])].tobytes()]
            cids += [pyamt.cid_of(f + b"%d" % i).ljust(40, b"\0"), cids40[i].tobytes()]
        sd, so, sl = _table(blocks)
        sup = engine.witness(sd, so, sl, np.frombuffer(b"".join(cids), dtype=np.uint8).reshape(-1, 40) if n else np.zeros((0, 40), np.uint8))
        return Built(sup.subset(np.arange(1, 2 * n, 2, dtype=np.uint32)), [sup])
    if how == "json":
        rows = [(cids[i], data[int(off[i]): int(off[i]) + int(lens[i])].tobytes()) for i in range(n)]
        b = engine.bundle(bundle_ref.bundle_json([], [], rows).encode())
        assert b.n_blocks == n
        return Built(b.witness, [b])
    raise AssertionError(how)


def _table(blocks):
    lens = np.array([len(b) for b in blocks], dtype=np.uint32)
    off = np.zeros(len(blocks), dtype=np.uint64)
    if len(blocks):
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(blocks), dtype=np.uint8).copy(), off, lens


def cid_status(cid: bytes, block: bytes) -> int:
    """what K1 says of one entry: hashlib over the block where the CID is (v1, *, blake2b-256, 32), else UNCHECKED"""
    if len(cid) == 38 and cid[0] == 1 and cid[1] < 0x80 and cid[2:6] == STD[2:]:
        return int(hashlib.blake2b(block, digest_size=32).digest() == cid[6:])
    return 2


def check_index(w, entries, probes, want, tag, few=6):
    """has / get / amt_get / read_values of one witness against the dict answers → list of differences"""
    wrong = []
    assert w.block_count == len(entries), (tag, w.block_count)
    has, ids = w.has(probes)
    exp_has = [int(x is not None) for x in want]
    exp_ids = [NO_BLOCK if x is None else x[0] for x in want]
    if has.tolist() != exp_has or ids.tolist() != exp_ids:
        bad = [(p.hex()[:24], int(h), int(i), e) for p, h, i, e in zip(probes, has, ids, exp_ids) if int(i) != e or int(h) != int(e != NO_BLOCK)]
        wrong.append((tag, "has", bad[:4], len(bad)))
    present = [(p, x) for p, x in zip(probes, want) if x is not None]
    if present:
        loc = np.zeros(len(present), dtype=ipcfp.LOC_DTYPE)
        loc["block"] = [x[0] for _, x in present]
        loc["len"] = [len(x[1]) for _, x in present]
        got = w.read_values(loc, stride=max(int(loc["len"].max()), 1))
        bad = [p.hex()[:24] for (p, x), g in zip(present, got) if g != x[1]]
        if bad:
            wrong.append((tag, "read_values", bad[:4], len(bad)))
    # `get` of EVERY probe where few is None (the small cases on every constructor, the large ones on the plain one: a get is
    # three round trips); the walker's probe on a handful
    pick = sorted({0, 1, len(present) // 2, len(present) - 1, len(probes) - 1, len(probes) - 2} & set(range(len(probes))))[: few or 6]
    for k in (range(len(probes)) if few is None else pick):
        p, x = probes[k], want[k]
        g = w.get(p)
        if g != (None if x is None else x[1]):
            wrong.append((tag, "get", p.hex()[:24], g))
    for k in pick:
        p, x = probes[k], want[k]
        if x is None or x[1][:8] == bytes.fromhex("8300018341018081"):
            st, loc = w.amt_get(p, 0, "any", [0])
            if x is None:
                ok = int(st[0]) == 65
            else:
                ok = int(st[0]) == 1 and int(loc["block"][0]) == x[0] and w.read_values(loc, stride=16)[0] == ws.value_of(x[1])
            if not ok:
                wrong.append((tag, "amt_get", p.hex()[:24], int(st[0]), int(loc["block"][0])))
    return wrong


def check_cids(w, entries, tag):
    st, nbad = w.verify_cids()
    exp = [cid_status(c, b) for c, b in entries]
    if st.tolist() != exp or nbad != exp.count(0):
        return [(tag, "verify_cids", [i for i, (g, e) in enumerate(zip(st.tolist(), exp)) if g != e][:6], nbad, exp.count(0))]
    return []


def run_case(engine, how, entries, probes, want, tag):
    data, off, lens, cids40 = ws.tables_of(entries)
    wrong = []
    with construct(engine, how, data, off, lens, cids40, [c for c, _ in entries]) as w:
        every = None if len(probes) <= 80 or (how == "witness" and len(probes) <= 1100) else 6
        wrong += check_index(w, entries, probes, want, (tag, how), few=every)
        wrong += check_cids(w, entries, (tag, how))
        w.rebuild_index()
        wrong += check_index(w, entries, probes, want, (tag, how, "rebuilt"), few=None if len(probes) <= 80 else 2)
    return wrong


# ---- A ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", CONSTRUCTORS)
@pytest.mark.parametrize("group", range(3))
def test_index_cases_each_in_a_witness_of_its_own(engine, how, group):
    wrong = []
    for name in A_NAMES[group::3]:
        c = ws.A_CASES[name]
        wrong += run_case(engine, how, c.entries, c.probes, c.want, name)
    assert not wrong, (wrong[:10], len(wrong))


@pytest.mark.parametrize("how", ("witness", "packed", "subset"))
def test_index_cases_merged_into_one_witness(engine, how):
    m = ws.a_merged()
    wrong = run_case(engine, how, m.entries, m.probes, m.want, "merged")
    assert not wrong, (wrong[:10], len(wrong))


def dict_answers(entries, probes):
    table = {}
    for i, (c, b) in enumerate(entries):
        table[c] = (i, b)
    return [table.get(p) for p in probes]


@pytest.mark.parametrize("name,start", [("one_home_last_33", 31), ("one_hash_33", 31), ("abut_33", 31), ("forms_33", 31), ("dup_3_of_33", 31),
                                        ("one_home_last_1025", 1024), ("one_hash_1025", 1024), ("dup_257_of_1025", 1024)])
def test_growth_by_put_keyed(engine, name, start):
    """31 → 32 → 33 blocks (64 slots at load exactly 0.5, then 128) and 1024 → 1025 (2048 → 4096 slots), one put at a time; then
    a put that REPLACES a key in the middle of the chain, one that replaces the chain's head and tail in one batch, and a put of
    an absent probe.  After every put the dict over what has been put so far answers, before and after a rebuild."""
    c = ws.A_CASES[name]
    entries = list(c.entries[:start])
    wrong = []
    data, off, lens, cids40 = ws.tables_of(entries)
    with engine.witness(data, off, lens, cids40) as w:
        steps = [[e] for e in c.entries[start:]]
        mid = c.entries[len(c.entries) // 2][0]
        steps.append([(mid, ws.block_of(7_000_001))])
        steps.append([(c.entries[0][0], ws.block_of(7_000_002)), (c.entries[-1][0], b"\x80")])
        absent = [p for p, x in zip(c.probes, c.want) if x is None]
        steps.append([(absent[0], ws.block_of(7_000_003))])
        for k, batch in enumerate(steps):
            w.put_keyed([cid for cid, _ in batch], [b for _, b in batch])
            entries += batch
            want = dict_answers(entries, c.probes)
            wrong += check_index(w, entries, c.probes, want, (name, "put", k), few=3)
        assert dict_answers(entries, [absent[0]]) == [(len(entries) - 1, ws.block_of(7_000_003))]
        wrong += check_cids(w, entries, (name, "put"))
        w.rebuild_index()
        wrong += check_index(w, entries, c.probes, dict_answers(entries, c.probes), (name, "put", "rebuilt"))
    assert not wrong, (wrong[:10], len(wrong))


# ---- D ------------------------------------------------------------------------------------------------------------------------
def check_blocks(w, d, tag):
    n = len(d.blocks)
    wrong = []
    st, nbad = w.verify_cids()
    if st.tolist() != d.status.tolist() or nbad != int((d.status == 0).sum()):
        wrong.append((tag, "verify_cids", np.nonzero(st != d.status)[0][:6].tolist(), nbad))
    loc = np.zeros(n, dtype=ipcfp.LOC_DTYPE)
    loc["block"] = np.arange(n)
    loc["len"] = d.lens
    small = d.lens <= 1024  # (two strides: a merged table holds 25 k short blocks beside a few hundred long ones)
    got = [None] * n
    for pick in (np.nonzero(small)[0], np.nonzero(~small)[0]):
        if len(pick):
            for i, g in zip(pick, w.read_values(loc[pick], stride=max(int(d.lens[pick].max()), 1))):
                got[i] = g
    bad = [i for i in range(n) if got[i] != d.blocks[i]]
    if bad:
        wrong.append((tag, "read_values", bad[:6], len(bad)))
    cids = [bytes(c[:38]) for c in d.cids]
    want = dict_answers(list(zip(cids, d.blocks)), cids)  # (equal blocks — the empty ones — share a CID: the last one answers)
    has, ids = w.has(cids)
    if not has.all() or ids.tolist() != [x[0] for x in want]:
        wrong.append((tag, "has", np.nonzero(ids != np.array([x[0] for x in want]))[0][:6].tolist()))
    for i in sorted({0, n // 2, n - 1, int(np.argmax(d.lens)), int(np.argmin(d.lens))}):
        if w.get(cids[i]) != want[i][1]:
            wrong.append((tag, "get", i))
    return wrong


@pytest.mark.parametrize("how", CONSTRUCTORS)
@pytest.mark.parametrize("group", range(3))
def test_block_table_cases(engine, how, group):
    wrong = []
    for name in D_NAMES[group::3]:
        d = ws.D_CASES[name]
        with construct(engine, how, d.data, d.off, d.lens, d.cids, [bytes(c[:38]) for c in d.cids]) as w:
            wrong += check_blocks(w, d, (name, how))
            w.rebuild_index()
            wrong += check_blocks(w, d, (name, how, "rebuilt"))
    assert not wrong, (wrong[:10], len(wrong))


@pytest.mark.parametrize("how", ("witness", "device", "packed"))
def test_block_table_cases_merged_into_one_witness(engine, how):
    """all 27 tables as ONE witness of 25 k blocks: every class present, seven scatter tiles, four blocks of the prefix sum"""
    d = ws.d_merged()
    with construct(engine, how, d.data, d.off, d.lens, d.cids, [bytes(c[:38]) for c in d.cids]) as w:
        wrong = check_blocks(w, d, ("merged", how))
        w.rebuild_index()
        wrong += check_blocks(w, d, ("merged", how, "rebuilt"))
    assert not wrong, (wrong[:10], len(wrong))


@pytest.mark.parametrize("name", ["edges_shuffled_ragged", "mixed_4095", "one_class_4096"])
def test_block_table_grown_by_put_keyed(engine, name):
    """the layout is made again by every put: the last two blocks arrive by put_keyed (4095 → 4096 → 4097 crosses the tile)"""
    d = ws.D_CASES[name]
    n = len(d.blocks)
    with engine.witness(d.data, d.off[: n - 2], d.lens[: n - 2], d.cids[: n - 2]) as w:
        for i in (n - 2, n - 1):
            w.put_keyed([bytes(d.cids[i, :38])], [d.blocks[i]])
        wrong = check_blocks(w, d, (name, "put"))
        extra = [b"\x00" * 70001, b""]
        w.put_keyed([pyamt.cid_of(b) for b in extra], extra)
        st, nbad = w.verify_cids()
        assert st[n:].tolist() == [1, 1] and st[:n].tolist() == d.status.tolist()
        assert [w.get(pyamt.cid_of(b)) for b in extra] == extra
    assert not wrong, wrong


# ---- B ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def routed(engine):
    def use(fast):
        engine.set_tuning("fast_verify", fast)
    yield use
    engine.set_tuning("fast_verify", -1)


def seen_set_routes(engine, use, w, t):
    """→ ({route: answer}, took_fast): the execution order itself, then the claims down the string route, the packed route
    fast and general (the index rebuilt in front of each: first contact), verify-and-scan, and the generator"""
    out = {}
    parents, child = t.parts["parents"], t.parts["child"]
    status, got = w.exec_order(parents)
    out["exec_order"] = (status, [bytes(r[:38]) for r in got])
    claims = [c for c, _ in t.claims]
    pr = ec.proofs(claims)
    use(-1)
    out["strings"] = w.verify_event_proofs(pr.arr, pr.n).tolist()
    ts, cl, blob = ipcfp.pack_event_proofs(pr.arr, pr.n)
    took_fast = None
    for fast, tag in ((1, "packed_fast"), (0, "packed_general")):
        use(fast)
        w.rebuild_index()
        engine.profile_reset()
        out[tag] = w.verify_event_claims(ts, cl, blob, len(blob)).tolist()
        if fast:
            took_fast = engine.profile_read("amt_walk")[0] > 0
    use(-1)
    w.rebuild_index()
    n, cap = pr.n, 1 << 13
    d_cl, d_blob = gec.dev(cl), gec.dev(blob)
    d_st = torch.full((n + 64,), 77, dtype=torch.uint8, device="cuda")
    d_has = torch.full((cap,), 9, dtype=torch.uint8, device="cuda")
    d_m = torch.zeros(cap * ipcfp.MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    sst, snr, snm = w.verify_and_scan_device(ts, d_cl.data_ptr(), n, d_blob.data_ptr(), len(blob), d_st.data_ptr(), ec.FILTER[0], ec.FILTER[1],
                                             None, d_has.data_ptr(), cap, d_m.data_ptr(), cap)
    engine.sync()
    m = d_m.cpu().numpy()[: snm * ipcfp.MATCH_DTYPE.itemsize].view(ipcfp.MATCH_DTYPE)
    out["verify_and_scan"] = d_st.cpu().numpy()[:n].tolist()
    out["scan"] = (sst, d_has.cpu().numpy()[:snr].tolist(), [(int(a), int(b), int(c)) for a, b, c in zip(m["exec_index"], m["event_index"], m["emitter"])])
    w.rebuild_index()
    gs, gm, gmsg, _ids = w.generate_event_proofs(parents, child, ec.FILTER[0], ec.FILTER[1])
    out["generate"] = (gs, [(int(a), int(b), int(c), bytes(x[:38])) for a, b, c, x in zip(gm["exec_index"], gm["event_index"], gm["emitter"], gmsg)])
    return out, took_fast


def seen_set_literals(t):
    """what each route must answer, written from the case's literal order: every executed message has ONE good event that
    matches the filter, emitter 2000 + its execution index"""
    want = [s for _, s in t.claims]
    k = len(t.order)
    return {"exec_order": (1, t.order), "strings": want, "packed_fast": want, "packed_general": want, "verify_and_scan": want,
            "scan": (1, [1] * k, [(e, 0, 2000 + e) for e in range(k)]),
            "generate": (1, [(e, 0, 2000 + e, t.order[e]) for e in range(k)])}


@pytest.mark.parametrize("group", range(5))
def test_seen_set_cases_each_in_a_witness_of_its_own(engine, routed, group):
    wrong, fast = [], {}
    engine.profile_enable(True, only="amt_walk")
    try:
        for name in B_NAMES[group::5]:
            t = ws.B_CASES[name]()
            with engine.witness(*t.store.tables()) as w:
                got, took_fast = seen_set_routes(engine, routed, w, t)
            fast[name] = took_fast
            wrong += [(name, r, str(got[r])[:120], str(x)[:120]) for r, x in seen_set_literals(t).items() if got[r] != x]
    finally:
        engine.profile_enable(False)
    assert not wrong, (wrong[:6], len(wrong))
    # the fast route is the packed claims' route on first contact with one tipset, where the dense plan takes the message
    # trees: in every group at least one wrapping chain and one equal-hash case DID take it (k_exec_insert_flags); the
    # general route (k_exec_insert + k_exec_first) is forced, so every case ran it
    print("fast route taken:", fast)
    assert any(took for n, took in fast.items() if ws.B_META[n]["kind"] in ("last", "dups")), fast
    assert any(took for n, took in fast.items() if ws.B_META[n]["kind"] == "one_hash"), fast


@pytest.mark.parametrize("name", [n for n in B_NAMES if ws.B_META[n]["raw"] <= 33])
def test_small_seen_set_cases_down_every_route_of_the_event_chain(engine, routed, name):
    """the eight routes of tests/test_gpu_event_chain.py (device claims, the compact form, the cached second call and the
    located route besides the four above) over the small cases"""
    t = ws.B_CASES[name]()
    claims, want = [c for c, _ in t.claims], [s for _, s in t.claims]
    with engine.witness(*t.store.tables()) as w:
        got = gec.answers(w, routed, t.store.blocks, claims)
    assert not gec.wrong_answers(got, [str(i) for i in range(len(claims))], want)
    # no claim is skipped on a route except those the compact form's CPU converter refuses (a 36-byte message CID)
    pr = ec.proofs(claims)
    pr.rows = claims
    refused = len(claims) - len(gec.compactable(pr))
    assert gec.declined(got) <= refused <= 1, (gec.declined(got), refused)


@pytest.mark.parametrize("which", ["up_to_33_raw_positions", "every_case"])
def test_seen_set_cases_merged_into_one_witness(engine, routed, which):
    """the cases' tipsets in ONE witness (every case: 39 tipsets, the ones of 1024, 1025 and 4097 raw positions among them),
    their claims in one batch: one context per tipset, the general route"""
    names = [n for n in B_NAMES if which == "every_case" or ws.B_META[n]["raw"] <= 33]
    store = pyamt.Store()
    claims, want = [], []
    for n in names:
        t = ws.B_CASES[n]()
        store.blocks.update(t.store.blocks)
        claims += [c for c, _ in t.claims]
        want += [s for _, s in t.claims]
    pr = ec.proofs(claims)
    ts, cl, blob = ipcfp.pack_event_proofs(pr.arr, pr.n)
    assert len(ts) == len(names)
    with engine.witness(*store.tables()) as w:
        assert w.verify_event_proofs(pr.arr, pr.n).tolist() == want
        for fast in (1, 0):
            routed(fast)
            w.rebuild_index()
            assert w.verify_event_claims(ts, cl, blob, len(blob)).tolist() == want, fast
        for n in names:
            t = ws.B_CASES[n]()
            status, got = w.exec_order(t.parts["parents"])
            assert status == 1 and [bytes(r[:38]) for r in got] == t.order, n


# ---- C: walks over crafted links ----------------------------------------------------------------------------------------------
import amt_enum_cases as ae  # noqa: E402
import test_gpu_hamt_get_cases as ghg  # noqa: E402
from test_amt_enum_cases import claim_mismatch, generate_literal, order_mismatch, scan_mismatch  # noqa: E402


@pytest.fixture()
def hamt_routed(engine):
    def use(cfg):
        engine.set_tuning("hamt_coop", -1)
        for k, v in cfg.items():
            engine.set_tuning(k, v)
    yield use
    for k in ("hamt_levels", "hamt_table", "hamt_coop"):
        engine.set_tuning(k, -1)


def triples(m):
    return list(zip(m["exec_index"].tolist(), m["event_index"].tolist(), m["emitter"].tolist()))


@pytest.mark.parametrize("name", list(ws.C_AMT))
def test_relabelled_amt_case_down_every_enumerating_route(engine, routed, name):
    """scan, exec_order, the packed claims on first contact (dense where the plan takes the roots: `amt_walk` says so) and
    forced general, strings, verify-and-scan, the generator, the shard planner and the pulled shards of the crafted bundle —
    against the literals of the honest case; the re-pointed variant answers 65 under the link and 1 beside it"""
    c, b = ws.C_AMT[name]()
    tabs = b.store.tables()
    root, parents, child = b.parts["receipts"], b.parts["parents"], b.parts["child"]
    n = c.meta["n"] if "n" in c.meta else ae.CASES[name.split("__")[0]].order[1]
    wrong = []
    with engine.witness(*tabs) as w:
        st, has, m, _ids = w.scan_events(root, *ae.FILTER)
        wrong += scan_mismatch(c, st, has, triples(m), "scan")
        st, cids = w.exec_order(parents)
        wrong += order_mismatch(c, st, cids, "exec_order")
        pr = ec.proofs([cl for _t, cl, _s in b.claims])
        ts, cl, blob = ipcfp.pack_event_proofs(pr.arr, pr.n)
        engine.profile_enable(True, only="amt_walk")
        try:
            for fast, tag in ((1, "packed_fast"), (0, "packed_general")):
                routed(fast)
                w.rebuild_index()
                engine.profile_reset()
                wrong += claim_mismatch(c, b, w.verify_event_claims(ts, cl, blob, len(blob)), tag)
                walks = engine.profile_read("amt_walk")[0]
                print(name, tag, "amt_walk launches:", walks)
                # the dense route is taken exactly where the plan takes the roots (size_513: yes; 33 parents: no), on the
                # wrapping chain and under one hash alike; the re-pointed tree enters it and hands the anomaly on
                if c.walks is not None and walks != ((1 if c.plan else 0) if fast else 0):
                    wrong.append((name, tag, "amt_walk launches", walks))
        finally:
            engine.profile_enable(False)
        routed(-1)
        w.rebuild_index()
        wrong += claim_mismatch(c, b, w.verify_event_proofs(pr.arr, pr.n), "strings")
        cap = n + 16
        d_cl, d_blob = gec.dev(cl), gec.dev(blob)
        d_st = torch.full((pr.n + 64,), 77, dtype=torch.uint8, device="cuda")
        d_has = torch.full((cap,), 9, dtype=torch.uint8, device="cuda")
        d_m = torch.zeros(cap * ipcfp.MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        w.rebuild_index()
        sst, snr, snm = w.verify_and_scan_device(ts, d_cl.data_ptr(), pr.n, d_blob.data_ptr(), len(blob), d_st.data_ptr(), *ae.FILTER, None,
                                                 d_has.data_ptr(), cap, d_m.data_ptr(), cap)
        engine.sync()
        wrong += claim_mismatch(c, b, d_st.cpu().numpy()[: pr.n], "one_call")
        mm = d_m.cpu().numpy()[: snm * ipcfp.MATCH_DTYPE.itemsize].view(ipcfp.MATCH_DTYPE) if sst == 1 else None
        wrong += scan_mismatch(c, sst, d_has.cpu().numpy()[:snr] if sst == 1 else None, triples(mm) if sst == 1 else None, "one_call")
        w.rebuild_index()
        gst, gm, gmsg, _gids = w.generate_event_proofs(parents, child, *ae.FILTER)
        if gst != generate_literal(c):
            wrong.append((name, "generate", gst, generate_literal(c)))
        elif gst == 1 and triples(gm) != [(i, 0, ae.EMITTER) for i in ae.present_indices(c.scan)]:
            wrong.append((name, "generate", "triples"))
        w.rebuild_index()
        # the planner loads the receipts ROOT and cuts [0, count): the re-pointed child does not concern it
        pst, nr, _bounds, lists = w.shard_plan_tipset_all(parents, child, 2)
        if c.order[0] != 1:  # (the execution order is every shard's: its Err is the plan's)
            if pst != c.order[0]:
                wrong.append((name, "shard_plan_tipset_all", pst, c.order[0]))
        elif (pst, nr) != (1, c.scan[1] if c.scan[0] == 1 else n) or len(lists) != 2:
            wrong.append((name, "shard_plan_tipset_all", pst, nr))
        # … and a rank that holds nothing but the crafted bundle in host memory pulls the same shard (host/shard_pull.cpp
        # builds a CID table of its own over the bundle's CIDs: the third copy of the sizing rule)
        pk = ipcfp.PackedWitnessTables(*tabs, ingest=True)
        ipcfp.host_register(pk.data)
        routed_claims = 0
        try:
            for r in range(2):
                st, lo, hi, n_receipts, ids = w.shard_plan_tipset(parents, child, 2, r)
                pst, pw, plo, phi, pn, stats = engine.witness_shard_pull(pk, parents, child, 2, r)
                # where the planner answers, the pulled shard is the planned one; where the planner meets an Err of the execution
                # order (a message-list link re-pointed) the pull still cuts by the receipts root it can load — "what decides
                # is that the verdicts are the unsharded engine's" (tests/test_gpu_shard_pull_fuzz.py): the claims routed to
                # the shard and its scan must give the literals either way
                if st == 1 and (st, lo, hi, n_receipts) != (pst, plo, phi, pn):
                    wrong.append((name, "shard_pull", r, (st, lo, hi, n_receipts), (pst, plo, phi, pn)))
                if st != 1 and (st != c.order[0] or pst != 1 or (plo, phi) != ipcfp.shard_range(pn, 2, r)):
                    wrong.append((name, "shard_pull under a failing plan", r, st, pst, plo, phi, pn))
                if pst == 1 and pw is None:
                    wrong.append((name, "shard_pull", r, "no witness came back"))
                if pw is not None:
                    if st == 1 and (pw.block_count != len(ids) or not pw.has([bytes(tabs[3][i]) for i in ids])[0].all()):
                        wrong.append((name, "shard_pull", r, "blocks", pw.block_count, len(ids)))
                    pos, c_r, b_r, bl_r = ipcfp.route_event_claims(cl, blob, len(blob), plo, phi, r == 1)
                    if len(pos):
                        got = pw.verify_event_claims(ts, c_r, b_r, bl_r).tolist()
                        lit = [b.claims[int(i)][2] for i in pos]
                        if got != lit:
                            wrong.append((name, "shard_pull", r, "claims", got, lit))
                    routed_claims += len(pos)
                    if c.scan[0] == 1:
                        sst, shas, sm, _ = pw.scan_events(root, *ae.FILTER, want_touched=False)
                        if sst != 1 or shas.tolist() != [1] * (phi - plo) or triples(sm) != [(i, 0, ae.EMITTER) for i in range(plo, phi)]:
                            wrong.append((name, "shard_pull", r, "scan", sst, len(shas)))
                    pw.close()
        finally:
            ipcfp.host_unregister(pk.data)
        assert routed_claims == pr.n, (routed_claims, pr.n)  # every claim was judged on one of the two pulled shards
    assert not wrong, wrong[:12]


@pytest.mark.parametrize("mode", list(ws.MODES))
def test_receipts_tree_written_through_the_crafted_store(engine, mode):
    """600 receipts whose 89 blocks pyamt named from the crafted iterator: the scan (dense) and `amt_get` (the walker)"""
    st, root, items = ws.c_written_receipts(mode)
    n = ws.WRITTEN_N
    idx = [0, 7, 8, 63, 64, 511, 512, n - 1, n, 4095]
    with engine.witness(*st.tables()) as w:
        status, has, m, _ = w.scan_events(root, *ae.FILTER, want_touched=False)
        assert status == 1 and has.tolist() == [1] * n and triples(m) == [(i, 0, ae.EMITTER) for i in range(n)]
        got, loc = w.amt_get(root, 0, "receipt", idx)
        assert got.tolist() == [1] * 8 + [32, 32]
        assert w.read_values(loc[:8], stride=128) == [items[i] for i in idx[:8]]


def test_relabelled_amt_cases_merged_into_one_witness(engine, routed):
    """the wrapping-chain and the one-hash relabellings of both shapes in ONE witness: four tipsets, one chain"""
    names = [n for n in ws.C_AMT if "repointed" not in n]
    store = pyamt.Store()
    for n in names:
        store.blocks.update(ws.C_AMT[n]()[1].store.blocks)
    wrong = []
    with engine.witness(*store.tables()) as w:
        for n in names:
            c, b = ws.C_AMT[n]()
            st, has, m, _ = w.scan_events(b.parts["receipts"], *ae.FILTER, want_touched=False)
            wrong += scan_mismatch(c, st, has, triples(m), "merged scan")
            st, cids = w.exec_order(b.parts["parents"])
            wrong += order_mismatch(c, st, cids, "merged exec_order")
            pr = ec.proofs([cl for _t, cl, _s in b.claims])
            wrong += claim_mismatch(c, b, w.verify_event_proofs(pr.arr, pr.n), "merged strings")
    assert not wrong, wrong[:12]


@pytest.mark.parametrize("mode", list(ws.MODES))
def test_relabelled_hamt_cases_every_route(engine, hamt_routed, mode):
    """the walker, the level path (whole, one-lane parse, two levels then the walker, one level), the node table and the
    default tuning over the relabelled trees, each in a witness of its own, then all of them merged; the composite with the
    link to its first child re-pointed to an absent CID of the same full hash: 65 under it, the literals beside it"""
    wrong = []
    merged = pyamt.Store()
    cases = {n: ws.C_HAMT[n]() for n in ws.C_HAMT if n.endswith("__" + mode)}
    for tree, hops in ws.C_HAMT_REPOINTS:
        cases[f"{tree}__{mode}__repointed"] = ws.c_hamt_repointed(tree, mode, hops)[0]
    cases[f"written_through_the_crafted_store__{mode}"] = ws.c_written_hamt(mode)
    assert len(cases) == 6 + 4 + 1
    for name, c in cases.items():
        w, data, off = ghg.witness_of(engine, c.store)
        with w:
            wrong += ghg.every_route(w, data, off, hamt_routed, name, c)
        if "repointed" not in name:  # (the re-pointed root carries the name of the intact one)
            merged.blocks.update(c.store.blocks)
    w, data, off = ghg.witness_of(engine, merged)
    with w:
        for name, c in cases.items():
            if "repointed" not in name:
                wrong += ghg.every_route(w, data, off, hamt_routed, (name, "merged"), c)
    assert not wrong, wrong[:12]


# ---- E: the claim set of the HAMT levels ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot", [77, 511])
@pytest.mark.parametrize("kind", sorted(ws.hg.COMPOSITE))
def test_claim_set_with_every_child_on_one_home(engine, hamt_routed, kind, slot):
    """the 32-child composite in a table where every child's block id has the SAME home in hamt_claim's 512-slot set (slot 511:
    the chain wraps), its 2048 queries as built, in runs of 256 on one child and interleaved — every route, the same literals"""
    c, ids = ws.e_composite(kind, slot)
    w, data, off = ghg.witness_of(engine, c.store)
    wrong = []
    value_of, it = {}, iter(c.values)
    for k, s in zip(c.keys, c.want):
        if s == ws.hg.TRUE:
            value_of[k] = next(it)
    with w:
        has, got = w.has(list(c.store.blocks)[ids[0]: ids[0] + 1] + list(c.store.blocks)[ids[-1]: ids[-1] + 1])
        assert got.tolist() == [ids[0], ids[-1]]
        for tag, order in ghg.composite_orders(kind).items():
            keys = [c.keys[i] for i in order]
            batch = ws.HamtCase(c.store, c.root, 5, kind, keys, [c.want[i] for i in order], [value_of[k] for k in keys if k in value_of])
            wrong += ghg.every_route(w, data, off, hamt_routed, (kind, slot, tag), batch)
    # … and merged: the same table with the relabelled trees of family C BEHIND it, so that every child keeps its block id
    merged = pyamt.Store()
    merged.blocks = dict(c.store.blocks)
    for n in ws.C_HAMT:
        merged.blocks.update(ws.C_HAMT[n]().store.blocks)
    assert list(merged.blocks)[: len(c.store.blocks)] == list(c.store.blocks) and len(merged.blocks) > len(c.store.blocks) + 300
    w, data, off = ghg.witness_of(engine, merged)
    with w:
        wrong += ghg.every_route(w, data, off, hamt_routed, (kind, slot, "merged"), batch)
    assert not wrong, wrong[:12]
