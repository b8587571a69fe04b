"""GPU: the storage generator over a CHAIN of child headers (kernels/storage_claims_gen_tipsets.inc,
ipcfp_generate_storage_claims_tipsets / _device) — every chain of tests/storage_gen_chain_cases.py on the host-spec and the
device-spec form and on `hamt_table` = 0, 1 and default.

Two references, neither supplied by the code under test: the expected bytes (ipcfp.compact_storage_claims of rows built in
numpy from tests/pystorage_gen.py's answers, per tipset, first_claim shifted) and the single-child call
(ipcfp_generate_storage_claims, one per tipset on the same witness, made once per (child, epoch, spec list) and shared)."""
import ctypes as C

import numpy as np
import pytest
import torch

import bundle_ref
import ipc_filecoin_proofs_amd as ipcfp
import storage_chain_cases as sc
import storage_gen_cases as sg
import storage_gen_chain_cases as gc

pytestmark = pytest.mark.gpu

T = gc.CHAIN
ROUTES = (0, 1, -1)
FORMS = ("host", "device")
E_INVALID, E_UNSUPPORTED = -1, -5


@pytest.fixture()
def routed(engine):
    def use(table):
        engine.set_tuning("hamt_table", table)
    yield use
    engine.set_tuning("hamt_table", -1)


@pytest.fixture(scope="module")
def chain_w(engine):
    w = engine.witness(*T.store.tables())
    yield w
    w.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def pose(w, form, chain_name, spec_name):
    """The chain call on either form → GeneratedStorageClaims"""
    chain = gc.CHAINS[chain_name]
    children, epochs = [T.children[k] for k in chain], gc.epochs_of(chain)
    ids, slots = T.batch(gc.SPECS[spec_name])
    if form == "host":
        return w.generate_storage_claims_tipsets(children, epochs, ids, slots)
    d_ids, d_slots = dev(ids), dev(slots)
    assert d_slots.data_ptr() % 16 == 0
    g = w.generate_storage_claims_tipsets_device(children, epochs, d_ids.data_ptr(), d_slots.data_ptr(), len(ids))
    g._keep = (d_ids, d_slots)
    return g


_SINGLE, _EXPECT = {}, {}


def single(w, child_key, epoch, spec_name):
    """ipcfp_generate_storage_claims for one child: (runs, slot, value, cflags bytes), status, first_error, block ids"""
    key = (child_key, int(epoch), spec_name)
    if key not in _SINGLE:
        ids, slots = T.batch(gc.SPECS[spec_name])
        with w.generate_storage_claims(T.children[child_key], int(epoch), ids, slots) as g:
            _SINGLE[key] = (g.copy(), g.status().tolist(), g.first_error, g.block_ids.tolist())
    return _SINGLE[key]


def expected(chain_name, spec_name):
    """Per tipset compact_storage_claims of the expected rows, first_claim shifted; the literal statuses; the answers"""
    key = (chain_name, spec_name)
    if key not in _EXPECT:
        rows, status, per = gc.expected_rows(ipcfp.SCLAIM_DTYPE, chain_name, spec_name)
        n = len(gc.SPECS[spec_name])
        runs, slot, value, cflags = [], [], [], []
        for t in range(len(gc.CHAINS[chain_name])):
            with ipcfp.compact_storage_claims(rows[t * n:(t + 1) * n]) as cols:
                r = cols.runs.copy()
                r["first_claim"] += t * n
                runs.append(r), slot.append(cols.slot.copy()), value.append(cols.value.copy()), cflags.append(cols.cflags.copy())
        _EXPECT[key] = (b"".join(x.tobytes() for x in runs), b"".join(x.tobytes() for x in slot),
                        b"".join(x.tobytes() for x in value), b"".join(x.tobytes() for x in cflags), status, per)
    return _EXPECT[key]


def first_bad(status):
    bad = [i for i, s in enumerate(status) if s != 1]
    return bad[0] if bad else None


def check_chain(w, g, chain_name, spec_name):
    chain = gc.CHAINS[chain_name]
    n, nt = len(gc.SPECS[spec_name]), len(chain)
    want_runs, want_slot, want_value, want_cflags, lit, per = expected(chain_name, spec_name)
    assert g.n == n * nt and g.n_tipsets == nt
    # against expected bytes
    assert g.status().tolist() == lit
    runs, slot, value, cflags = g.copy()
    assert g.n_runs * 192 == len(want_runs)
    assert runs.tobytes() == want_runs and slot.tobytes() == want_slot
    assert value.tobytes() == want_value and cflags.tobytes() == want_cflags
    assert g.first_error == first_bad(lit)
    for p in (g.runs_ptr, g.slot_ptr, g.value_ptr, g.cflags_ptr):
        assert p and p % 16 == 0
    # against single calls
    singles = [single(w, k, gc.EPOCH0 + t, spec_name) for t, k in enumerate(chain)]
    shifted = []
    for t, s in enumerate(singles):
        r = s[0][0].copy()
        r["first_claim"] += t * n
        shifted.append(r.tobytes())
    assert runs.tobytes() == b"".join(shifted)
    for col, got in ((1, slot), (2, value), (3, cflags)):
        assert got.tobytes() == b"".join(s[0][col].tobytes() for s in singles)
    assert g.status().tolist() == [x for s in singles for x in s[1]]
    for t, s in enumerate(singles):
        assert g.tipset_block_ids(t).tolist() == s[3], t
        assert g.tipset_first_error(t) == s[2] == first_bad(lit[t * n:(t + 1) * n]), t
        if all(a[0] == 1 for a in per[t]):  # … and the restatement's recorded blocks where every spec succeeds
            assert [T.cids[i] for i in s[3]] == sg.union_ord([a[2] for a in per[t]]), t
    assert [T.cids[i] for i in g.block_ids] == sg.union_ord([[T.cids[i] for i in s[3]] for s in singles])


# ---- 1. every chain of the table, both forms, three routes -------------------------------------------------------------
@pytest.mark.parametrize("case", gc.CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def test_chain_against_expected_bytes_and_single_calls(chain_w, routed, case):
    for table in ROUTES:
        routed(table)
        for form in FORMS:
            with pose(chain_w, form, *case) as g:
                check_chain(chain_w, g, *case)


# ---- 2. each tipset's columns against the witness pruned to THAT tipset's blocks --------------------------------------
def _tipset_view(g, t, n, n_runs0):
    """tipset t of the handle as a column form of its own: its run records with first_claim un-shifted (uploaded), and the
    handle's own column pointers advanced to its claims"""
    runs = g.copy()[0][t * n_runs0:(t + 1) * n_runs0].copy()
    runs["first_claim"] -= t * n
    d_runs = dev(runs)
    return d_runs, (d_runs.data_ptr(), n_runs0, g.slot_ptr + 32 * t * n, g.value_ptr + 32 * t * n, g.cflags_ptr + t * n, n)


def _verify_pruned(engine, keep, view):
    data, off, lens, c40 = T.store.tables()
    d_st = torch.zeros(view[-1], dtype=torch.uint8, device="cuda")
    with engine.witness(data, off[keep], lens[keep], c40[keep]) as pw:
        pw.verify_storage_columns_device(*view, d_st.data_ptr())
    return d_st.cpu().numpy()


@pytest.mark.parametrize("table", ROUTES)
def test_pruned_to_each_tipsets_own_blocks(engine, chain_w, routed, table):
    routed(table)
    # (a) a chain with failing specs and a failing tipset: 1 where the generator said 1, ERR_BAD_CLAIM (69) elsewhere
    chain_name, spec_name = "sr_v6_middle", "five_in_three_runs"
    n, lit = len(gc.SPECS[spec_name]), expected(chain_name, spec_name)[4]
    assert set(lit) == {1, 66, 68}
    with pose(chain_w, "host", chain_name, spec_name) as g:
        n_runs0 = g.n_runs // g.n_tipsets
        for t in range(g.n_tipsets):
            keep_alive, view = _tipset_view(g, t, n, n_runs0)
            sub = g.tipset_block_ids(t).astype(np.int64)
            if len(sub) == 0:
                continue
            got = _verify_pruned(engine, sub, view)
            assert got.tolist() == [1 if s == 1 else 69 for s in lit[t * n:(t + 1) * n]], t
    # (b) an all-success chain: every listed block of a tipset is needed by that tipset
    chain_name, spec_name = "t4", "successes"
    n = len(gc.SPECS[spec_name])
    assert all(s == 1 for s in expected(chain_name, spec_name)[4])
    with pose(chain_w, "device", chain_name, spec_name) as g:
        n_runs0 = g.n_runs // g.n_tipsets
        lists = [g.tipset_block_ids(t).astype(np.int64) for t in range(g.n_tipsets)]
        assert len({tuple(l) for l in lists}) == 4 and all(5 < len(l) < len(g.block_ids) for l in lists)
        for t, sub in enumerate(lists):
            keep_alive, view = _tipset_view(g, t, n, n_runs0)
            assert (_verify_pruned(engine, sub, view) == 1).all(), t
            for drop in range(len(sub)):
                assert not (_verify_pruned(engine, np.delete(sub, drop), view) == 1).all(), (t, drop)


# ---- 3. strings: the bundle writer, the parser and both verifiers -------------------------------------------------------
def test_strings_and_the_bundle(engine, chain_w):
    chain_name, spec_name = "t4", "successes"
    chain = gc.CHAINS[chain_name]
    ids, slots = T.batch(gc.SPECS[spec_name])
    per = expected(chain_name, spec_name)[5]
    w = chain_w
    with pose(w, "host", chain_name, spec_name) as g:
        p, n = g.proofs()
        assert n == g.n == len(ids) * len(chain)
        dicts = [dict(child_epoch=gc.EPOCH0 + t, child_block_cid=sc.cid_str(T.children[k]),
                      parent_state_root=sc.cid_str(a[1]["parent_state_root"]), actor_id=int(i),
                      actor_state_cid=sc.cid_str(a[1]["actor_state_cid"]), storage_root=sc.cid_str(a[1]["storage_root"]),
                      slot=sc.hex0x(s.tobytes()), value=sc.hex0x(a[1]["value"]))
                 for t, k in enumerate(chain) for i, s, a in zip(ids, slots, per[t])]
        assert g.proof_rows() == dicts
        text = w.write_bundle_json(p, n, None, 0, block_ids=g.block_ids)
        blocks = [(T.cids[i], T.store.blocks[T.cids[i]]) for i in g.block_ids]
        assert text == bundle_ref.bundle_json(dicts, [], blocks).encode()
        b = engine.bundle(text)
        try:
            ss, es = b.verify()
        finally:
            b.close()
        assert len(ss) == g.n and (ss == 1).all() and len(es) == 0
        assert (w.verify_storage_proofs(p, n) == 1).all()
    with pose(w, "host", "hdr_absent_middle", "five_in_three_runs") as g:  # a failing spec: no proofs, at first_error
        with pytest.raises(ipcfp.EngineError) as e:
            g.proofs()
        assert e.value.rc == E_INVALID and e.value.bad_index == g.first_error


# ---- 4. state around the call --------------------------------------------------------------------------------------------
def _snapshot(g):
    return ([x.tobytes() for x in g.copy()], g.status().tolist(), g.block_ids.tolist(),
            [g.tipset_block_ids(t).tolist() for t in range(g.n_tipsets)], [g.tipset_first_error(t) for t in range(g.n_tipsets)])


def test_state_around_the_call(chain_w):
    w = chain_w
    ids, slots = T.batch(gc.SPECS["n65"])

    def one():
        with w.generate_storage_claims(T.children["h2"], 5, ids, slots) as g:
            assert g.n_tipsets == 1 and g.tipset_block_ids(0).tolist() == g.block_ids.tolist()
            assert g.tipset_first_error(0) == g.first_error
            return _snapshot(g)

    before = one()
    with pose(w, "host", "t65", "own_runs_4") as g:
        chain_a = _snapshot(g)
    assert one() == before
    w.rebuild_index()
    with pose(w, "device", "t65", "own_runs_4") as g:
        assert _snapshot(g) == chain_a
    assert one() == before


# ---- 5. refusals, each with its code; *out is null behind every one -----------------------------------------------------
def test_refusals(engine, chain_w):
    w, lib = chain_w, chain_w.lib
    ids, slots = T.batch(gc.SPECS["five_in_three_runs"])
    children = ipcfp.cid_slots([T.children["h0"], T.children["h1"]])
    epochs = np.array([1, 2], dtype=np.int64)
    d_ids, d_slots = dev(ids), dev(np.concatenate([np.zeros(8, np.uint8), slots.reshape(-1)]))
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def host(cids, ep, nt, a, s, n, ctx=engine.h, wit=w.h):
        h = C.c_void_p(1)
        rc = lib.ipcfp_generate_storage_claims_tipsets(ctx, wit, cids, ep, nt, a, s, n, C.byref(h))
        assert rc != 0 and h.value is None
        return rc

    def device(cids, ep, nt, a, s, n):
        h = C.c_void_p(1)
        rc = lib.ipcfp_generate_storage_claims_tipsets_device(engine.h, w.h, cids, ep, nt, a, s, n, C.byref(h))
        assert rc != 0 and h.value is None
        return rc

    n = len(ids)
    assert host(p(children), p(epochs), 0, p(ids), p(slots), n) == E_INVALID
    assert host(None, p(epochs), 2, p(ids), p(slots), n) == E_INVALID
    assert host(p(children), None, 2, p(ids), p(slots), n) == E_INVALID
    assert host(p(children), p(epochs), 2, None, p(slots), n) == E_INVALID
    assert host(p(children), p(epochs), 2, p(ids), None, n) == E_INVALID
    assert host(p(children), p(epochs), 2, p(ids), p(slots), n, ctx=None) == E_INVALID
    assert host(p(children), p(epochs), 2, p(ids), p(slots), n, wit=None) == E_INVALID
    assert lib.ipcfp_generate_storage_claims_tipsets(engine.h, w.h, p(children), p(epochs), 2, p(ids), p(slots), n, None) == E_INVALID
    assert device(p(children), p(epochs), 2, None, d_slots.data_ptr() + 16, n) == E_INVALID
    assert device(p(children), p(epochs), 2, d_ids.data_ptr(), d_slots.data_ptr() + 8, n) == E_INVALID   # slots off 16
    assert device(p(children), p(epochs), 2, d_ids.data_ptr() + 4, d_slots.data_ptr() + 16, n) == E_INVALID  # ids off 8
    # too many tipsets; too many claims (refused before anything is read: the arrays need not be that long)
    long_chain = gc.CHAINS["refused_4097"]
    many = ipcfp.cid_slots([T.children[k] for k in long_chain])
    many_ep = gc.epochs_of(long_chain)
    assert host(p(many), p(many_ep), 4097, p(ids), p(slots), n) == E_UNSUPPORTED
    assert device(p(many), p(many_ep), 4097, d_ids.data_ptr(), d_slots.data_ptr() + 16, n) == E_UNSUPPORTED
    assert host(p(many), p(many_ep), 4096, p(ids), p(slots), 1 << 20) == E_UNSUPPORTED        # 2^32 claims
    assert 255 * 16843009 == (1 << 32) - 1
    assert host(p(many), p(many_ep), 255, p(ids), p(slots), 16843009) == E_UNSUPPORTED        # exactly 2^32 − 1 claims
    assert host(p(children), p(epochs), 2, p(ids), p(slots), (1 << 32) - 1) == E_UNSUPPORTED
    # 4096 tipsets answer
    with w.generate_storage_claims_tipsets([T.children[k] for k in long_chain[:4096]], many_ep[:4096], ids[:1], slots[:1]) as g:
        assert g.n == g.n_tipsets == 4096 and g.first_error is None
    # no specs: an empty handle that remembers its tipset count
    with w.generate_storage_claims_tipsets([T.children["h0"], T.children["hdr_absent"], T.children["h1"]], [1, 2, 3], ids[:0], slots[:0]) as g:
        assert g.n == 0 and g.n_runs == 0 and g.n_tipsets == 3 and g.first_error is None and len(g.block_ids) == 0
        assert [len(g.tipset_block_ids(t)) for t in range(3)] == [0, 0, 0]
        assert [g.tipset_first_error(t) for t in range(3)] == [None, None, None]
        assert g.proofs()[1] == 0
        nb = C.c_uint64(9)
        assert not lib.ipcfp_generated_storage_claims_tipset_block_ids(g.h, 3, C.byref(nb)) and nb.value == 0  # t out of range
        assert lib.ipcfp_generated_storage_claims_tipset_first_error(g.h, 3) == 2**64 - 1


def test_recorder_larger_than_a_gibibyte_is_refused(engine):
    """4096 rows of ceil(blocks / 32) words pass 2^28 words from 65 537 words a row on: 2^21 + 1 one-byte blocks"""
    n = (1 << 21) + 1
    rng = np.random.default_rng(29)
    cids = np.zeros((n, 40), dtype=np.uint8)
    cids[:, :6] = np.frombuffer(bytes.fromhex("0171a0e40220"), dtype=np.uint8)
    cids[:, 6:14] = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)  # distinct
    cids[:, 14:38] = rng.integers(0, 256, (n, 24), dtype=np.uint8)
    data = np.zeros(n, dtype=np.uint8)
    off, lens = np.arange(n, dtype=np.uint64), np.ones(n, dtype=np.uint32)
    children = np.ascontiguousarray(np.repeat(cids[:1], 4096, axis=0))
    epochs = np.arange(4096, dtype=np.int64)
    ids, slots = np.array([7], dtype=np.uint64), np.zeros((1, 32), dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    with engine.witness(data, off, lens, cids) as w:
        h = C.c_void_p(1)
        rc = w.lib.ipcfp_generate_storage_claims_tipsets(engine.h, w.h, p(children), p(epochs), 4096, p(ids), p(slots), 1, C.byref(h))
        assert rc == E_UNSUPPORTED and h.value is None
        assert b"cut the chain" in w.lib.ipcfp_last_error(engine.h)
        # a short chain over the same witness answers (no block is a header: both claims fail alike)
        with w.generate_storage_claims_tipsets([cids[0, :38].tobytes()] * 2, [1, 2], ids, slots) as g:
            st = g.status().tolist()
            assert g.n == 2 and g.n_tipsets == 2 and st[0] == st[1] != 1 and g.first_error == 0
            assert g.tipset_block_ids(0).tolist() == g.tipset_block_ids(1).tolist() == g.block_ids.tolist() == [0]
