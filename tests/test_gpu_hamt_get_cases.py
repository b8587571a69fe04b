"""GPU: the get primitives' named cases (tests/hamt_get_cases.py) through EVERY route of `ipcfp_hamt_get` — the routes of
tests/test_gpu_hamt_routes.py and the tuning left at its default — against the literal status of each key and the literal
value bytes behind each located value.  One witness per case; all cases' blocks merged into one witness, so that a case's
nodes sit among foreign blocks in the arena's own layout; the composite tree on both sides of the default route's switch to
the level path, with its batch ordered child by child and interleaved; and a subset through `ipcfp_hamt_get_device`, every
buffer resident, the calls issued back to back before one synchronisation."""
import numpy as np
import pytest

import hamt_get_cases as hg
import ipc_filecoin_proofs_amd as ipcfp
from test_gpu_hamt_routes import ROUTES, loc_bytes, routed  # noqa: F401 (`routed` is the fixture that restores the tuning)

pytestmark = pytest.mark.gpu

DEFAULT = ("default", {"hamt_levels": -1, "hamt_table": -1})
ALL_ROUTES = ROUTES + [DEFAULT]
NAMES = [n for n, m in hg.META.items() if m["group"] != "composite"]
GROUPS = 8


def witness_of(engine, store):
    data, off, lens, cids = hg.tables(store)
    return engine.witness(data, off, lens, ipcfp.cid_slots(cids)), data, off


def wrong_answers(tag, keys, want, values, gs, gl, data, off):
    out = [(tag, keys[i][:16], int(gs[i]), want[i]) for i in range(len(keys)) if int(gs[i]) != want[i]]
    if not out:
        got = [b for s, b in zip(gs, loc_bytes(data, off, gl)) if s == hg.TRUE]
        out += [(tag, "value", g[:16], v[:16]) for g, v in zip(got, values) if g != v][:3]
    return out[:6]


def every_route(w, data, off, routed, name, c, routes=ALL_ROUTES):
    wrong = []
    for route, cfg in routes:
        routed(cfg)
        gs, gl = w.hamt_get(c.root, c.bw, c.kind, c.keys)
        wrong += wrong_answers((name, route), c.keys, c.want, c.values, gs, gl, data, off)
    return wrong


@pytest.mark.parametrize("group", range(GROUPS))
def test_every_case_in_a_witness_of_its_own(engine, routed, group):
    wrong = []
    for name in NAMES[group::GROUPS]:
        c = hg.CASES[name]
        w, data, off = witness_of(engine, c.store)
        with w:
            wrong += every_route(w, data, off, routed, name, c)
    assert not wrong, wrong[:20]


@pytest.fixture(scope="module")
def merged(engine):
    w, data, off = witness_of(engine, hg.merged())
    yield w, data, off
    w.close()


@pytest.mark.parametrize("group", range(GROUPS))
def test_all_cases_in_one_witness_one_call_per_root(engine, routed, merged, group):
    w, data, off = merged
    wrong = []
    for name in NAMES[group::GROUPS]:
        wrong += every_route(w, data, off, routed, name, hg.CASES[name])
    assert not wrong, wrong[:20]


@pytest.mark.parametrize("group", range(4))
def test_level_cases_in_batches_wide_enough_for_the_fused_top(engine, routed, merged, group):
    """A case built at level 1 or 3 has three probes, and a batch of three never gets a fused top (it takes two levels from
    32 queries, three from 1024, over a witness of as many blocks).  Here each goes among a thousand keys that stand on
    clear bits of the single-link nodes above it: the forced level path fuses three levels, the default route two."""
    w, data, off = merged
    wrong = []
    for name in hg.LEVEL_CASES[group::4]:
        c = hg.wide(name)
        assert len(c.keys) >= hg.FUSED_TOP_MIN_QUERIES[1] and w.block_count >= hg.FUSED_TOP_MIN_QUERIES[1]
        wrong += every_route(w, data, off, routed, name, c)
    assert not wrong, wrong[:20]


# ---- the composite tree -------------------------------------------------------------------------------------------------------
def composite_batch(kind, order, tree="children"):
    """→ (root, keys, want, values) of a composite tree's probes taken in `order` (indices into its key list, repeats allowed)"""
    st, root, keys, want, values, child, _ = hg.COMPOSITES[tree][kind]
    value_of, it = {}, iter(values)
    for k, s in zip(keys, want):
        if s == hg.TRUE:
            value_of[k] = next(it)
    ks = [keys[i] for i in order]
    return root, ks, [want[i] for i in order], [value_of[k] for k in ks if k in value_of]


def composite_orders(kind, tree="children"):
    child = np.array(hg.COMPOSITES[tree][kind][5])
    by_child = [np.nonzero(child == ci)[0] for ci in range(32)]
    per = min(len(b) for b in by_child)
    runs = np.concatenate([np.tile(b, -(-256 // len(b)))[:256] for b in by_child])  # 256 consecutive queries on one child
    woven = np.stack([b[:per] for b in by_child], axis=1).reshape(-1)                # the 32 children in turn
    assert len(runs) == 32 * 256 and (child[runs[:256]] == 0).all() and (child[woven[:32]] == np.arange(32)).all()
    return {"as_built": np.arange(len(child)), "runs_of_256_on_one_child": runs, "interleaved": woven}


@pytest.mark.parametrize("kind", sorted(hg.COMPOSITE))
@pytest.mark.parametrize("tree", sorted(hg.COMPOSITES))
def test_composite_tree_every_route_every_order(engine, routed, merged, tree, kind):
    w, data, off = merged
    wrong = []
    for tag, order in composite_orders(kind, tree).items():
        root, keys, want, values = composite_batch(kind, order, tree)
        assert len(keys) >= 2048
        for route, cfg in ALL_ROUTES:
            routed(cfg)
            gs, gl = w.hamt_get(root, 5, kind, keys)
            wrong += wrong_answers((tag, route), keys, want, values, gs, gl, data, off)
    assert not wrong, wrong[:20]


@pytest.mark.parametrize("kind", sorted(hg.COMPOSITE))
@pytest.mark.parametrize("n", [hg.LIMITS["levels_switch"] - 1, hg.LIMITS["levels_switch"]])
def test_composite_tree_on_both_sides_of_the_default_switch(engine, routed, kind, n):
    """1023 queries take the walker, 1024 the level path, when nothing is forced; a witness of the tree's own"""
    order = composite_orders(kind)["interleaved"][:n]
    root, keys, want, values = composite_batch(kind, order)
    assert len(keys) == n and {1, 32, 65} <= set(want)
    w, data, off = witness_of(engine, hg.COMPOSITE[kind][0])
    with w:
        routed(DEFAULT[1])
        gs, gl = w.hamt_get(root, 5, kind, keys)
    wrong = wrong_answers((kind, n), keys, want, values, gs, gl, data, off)
    assert not wrong, wrong


# ---- ipcfp_hamt_get_device ----------------------------------------------------------------------------------------------------
def test_device_entry_point_gives_the_same_answers(engine, routed, merged):
    """A subset of the composite tree, the depth chains and the key-length group with keys, offsets and lengths resident;
    every call is issued before the one synchronisation, on the default route (which the batch sizes split between the
    walker and the level path) and with the level path forced."""
    import torch

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()

    w, data, off = merged
    batches = []
    for tree in sorted(hg.COMPOSITES):
        for kind in sorted(hg.COMPOSITE):
            root, keys, want, values = composite_batch(kind, composite_orders(kind, tree)["interleaved"][:1500], tree)
            batches.append((("composite", tree, kind), root, 5, kind, keys, want, values))
    for name in hg.LEVEL_CASES[::5]:
        c = hg.wide(name)
        batches.append(((name, "wide"), c.root, c.bw, c.kind, c.keys, c.want, c.values))
    for name, m in hg.META.items():
        if m["group"] in ("depth", "keys"):
            c = hg.CASES[name]
            batches.append((name, c.root, c.bw, c.kind, c.keys, c.want, c.values))
    assert len(batches) > 50
    wrong = []
    for route, cfg in (DEFAULT, next(r for r in ROUTES if r[0] == "levels")):
        routed(cfg)
        issued = []
        for tag, root, bw, kind, keys, want, values in batches:
            n = len(keys)
            kl = np.array([len(k) for k in keys], dtype=np.uint32)
            ko = np.zeros(n, dtype=np.uint32)
            ko[1:] = np.cumsum(kl[:-1])
            d = [dev(np.frombuffer(b"".join(keys) + bytes(32), dtype=np.uint8)), dev(ko), dev(kl)]
            d_st = torch.full((n + 64,), 77, dtype=torch.uint8, device="cuda")
            d_loc = torch.zeros(n * 12 + 64, dtype=torch.uint8, device="cuda")
            issued.append((d, d_st, d_loc))
        torch.cuda.synchronize()  # torch's uploads and fills are done before the engine's stream writes
        for (tag, root, bw, kind, keys, *_), (d, d_st, d_loc) in zip(batches, issued):
            w.hamt_get_device(root, bw, kind, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), len(keys), d_st.data_ptr(), d_loc.data_ptr())
        engine.sync()
        for (tag, root, bw, kind, keys, want, values), (d, d_st, d_loc) in zip(batches, issued):
            n = len(keys)
            st = d_st.cpu().numpy()
            assert (st[n:] == 77).all(), (tag, route)  # nothing is written past the batch
            gl = d_loc.cpu().numpy()[: n * 12].view(ipcfp.LOC_DTYPE)
            wrong += wrong_answers((tag, route, "device"), keys, want, values, st[:n], gl, data, off)
    assert not wrong, wrong[:20]
