"""CPU: the crafted-key cases of tests/witness_store_cases.py under the judges that need no GPU — the properties each case
is named for (asserted when the module is imported), the oracle's `MemoryBlockstore` over the CID-index cases (its size is
the number of distinct keys; `amt_get` of a block that is an Amtv0 root is a `get`: the LAST block of a key answers),
tests/pyevents.py and the oracle over the seen-set's tipsets, and a guard that reads the hash, the sizing rule and the
layout's constants out of the engine's SOURCE, so that a change of any of them fails here and not silently on the GPU."""
import os
import re

import numpy as np
import pytest

import event_chain_cases as ec
import pyevents
import witness_store_cases as ws
from pyamt import uint
from test_amt_enum_cases import harness, oracle_wrong, plan_wrong, pyevents_wrong  # noqa: F401  (harness: the fixture)
from test_event_chain import oracle_answers
from test_hamt_get_cases import differences, python_answers
from test_hamt_get_cases import oracle_answers as hamt_oracle_answers

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ipc-filecoin-proofs_amd", "csrc")
A_NAMES, B_NAMES = list(ws.A_CASES), list(ws.B_CASES)
BLOCK_MISSING = 65


def test_the_lists_cover_what_they_must():
    assert len(ws.A_CASES) >= 90 and len(ws.D_CASES) >= 27 and len(ws.B_CASES) >= 38
    for n in ws.SIZES:
        kinds = {m["kind"] for name, m in ws.A_META.items() if m["n"] == n}
        assert kinds >= ({"one_home"} if n < 2 else {"wrap", "equal_hash", "dup"}), (n, kinds)
        assert all(f"one_home_{h}_{n}" in ws.A_CASES for h in ws.HOMES) and f"one_hash_{n}" in ws.A_CASES
    for name, c in ws.A_CASES.items():
        assert len(c.probes) == len(c.want) == len(set(c.probes)) and sum(w is None for w in c.want) == ws.A_META[name]["absent"] >= 1
        ids = [w[0] for w in c.want if w is not None]
        assert all(c.entries[i][1] == w[1] and c.entries[i][0] == p for p, w in zip(c.probes, c.want) if w is not None for i in [w[0]])
        assert len(ids) == len({e[0] for e in c.entries})
    m = ws.a_merged()
    assert len(m.entries) == sum(len(c.entries) for c in ws.A_CASES.values()) > 30000 and ws.table_mask(len(m.entries)) == (1 << 17) - 1
    # one home stays one home in the merged table, and a wrapping chain still wraps there: the targets fix 20 bits
    big = ws.table_mask(len(m.entries))
    assert {ws.home(c, big) for c, _ in ws.A_CASES["one_home_last_1025"].entries} == {big}
    # D: the chunk classes at both sides of the cap, every class once, every tile edge; four planted mismatches apiece
    for name, d in ws.D_CASES.items():
        assert 1 <= int((d.status == 0).sum()) <= 4 and len(d.blocks) == len(d.status)
    assert {len(d.blocks) for d in ws.D_CASES.values()} >= set(ws.COUNTS)
    assert sum(d.off[0] != 0 or (np.diff(d.off.astype(np.int64)) < 0).any() for d in ws.D_CASES.values() if len(d.blocks) > 1) >= 8
    # B: every raw count over every number of parents, every family at every count
    for n in ws.RAW_COUNTS:
        assert {m["kind"] for m in ws.B_META.values() if m["raw"] == n} >= set(ws.B_KINDS)


@pytest.mark.parametrize("group", range(4))
def test_the_oracle_store_gives_every_dict_answer(oracle, group):
    """`HashMap::insert` overwrites: the store holds one entry per distinct CID, and what it returns is the LAST block put
    under it.  (The 70-byte CID is left to the engine: the oracle's entry points take a root of at most 40 bytes.)"""
    wrong = []
    for name in A_NAMES[group::4]:
        c = ws.A_CASES[name]
        data, off, lens, _ = ws.tables_of(c.entries)
        st = oracle.store_var(data, off, lens, [cid for cid, _ in c.entries])
        assert st.size() == len({cid for cid, _ in c.entries}), name
        for p, want in zip(c.probes, c.want):
            if len(p) > 40:
                continue
            status, values = st.amt_get(p, 0, "any", [0], cap=16)
            got = (int(status[0]), values[0] if status[0] == 1 else None)
            assert want is None or ws.value_of(want[1]) == uint(want[0])
            if got != ((1, ws.value_of(want[1])) if want is not None else (BLOCK_MISSING, None)):
                wrong.append((name, p.hex(), got, want and want[0]))
        st.close()
    assert not wrong, wrong[:10]


def test_the_merged_witness_changes_no_answer(oracle):
    m = ws.a_merged()
    data, off, lens, _ = ws.tables_of(m.entries)
    st = oracle.store_var(data, off, lens, [cid for cid, _ in m.entries])
    assert st.size() == len({cid for cid, _ in m.entries})
    wrong = []
    for p, want in list(zip(m.probes, m.want))[::7]:
        if len(p) <= 40:
            status, values = st.amt_get(p, 0, "any", [0], cap=16)
            if (int(status[0]), values[0] if status[0] == 1 else None) != ((1, ws.value_of(want[1])) if want else (BLOCK_MISSING, None)):
                wrong.append((p.hex(), int(status[0]), want and want[0]))
    st.close()
    assert not wrong, wrong[:10]
    # a case's answers inside the merged witness are its own, moved by the blocks in front of it
    base = 0
    at = dict(zip(m.probes, m.want))
    for name, c in ws.A_CASES.items():
        assert [at[p] and (at[p][0] - base, at[p][1]) for p in c.probes] == c.want, name
        base += len(c.entries)


@pytest.mark.parametrize("group", range(4))
def test_the_seen_set_cases_under_pyevents_and_the_oracle(oracle, group):
    """the literal execution order and the literal claim statuses under tests/pyevents.py and under the oracle"""
    for name in B_NAMES[group::4]:
        t = ws.B_CASES[name]()
        assert t.order == ws.first_seen(t.raw) and len(t.order) == ws.B_META[name]["distinct"]
        if len(t.raw) <= 64:
            assert t.order == ec.first_seen(ws.spread(t.raw, ws.B_META[name]["parents"]))
        assert pyevents.exec_order(t.store.blocks, t.parts["parents"]) == t.order, name
        st = oracle.store(*t.store.tables())
        status, got = st.exec_order(t.parts["parents"])
        st.close()
        assert status == 1 and [bytes(r).rstrip(b"\0") for r in got] == [c.rstrip(b"\0") for c in t.order], name
        claims, want = [c for c, _ in t.claims], [s for _, s in t.claims]
        assert {1, 7} <= set(want) and (8 in want) == (len(t.order) < len(t.raw)), (name, want)
        few = claims if len(t.raw) <= 1025 else claims[:2] + claims[-1:]
        assert [pyevents.verify(t.store.blocks, c) for c in few] == (want if len(t.raw) <= 1025 else want[:2] + want[-1:]), name
        for entry, g in oracle_answers(oracle, t.store.blocks, claims).items():
            assert g == want, (name, entry, g, want)


# ---- C and E: walks over crafted links, the claim set ------------------------------------------------------------------------------
def test_relabelled_amt_cases_keep_their_literals_and_their_plan(oracle, harness):  # noqa: F811
    """pyevents, the oracle and the dense plan's harness over the relabelled trees: the literals of tests/amt_enum_cases.py,
    65 under the re-pointed link.  Per chain kind at least one shape the plan takes and one it declines."""
    wrong, plans = [], {}
    for name, build in ws.C_AMT.items():
        c, b = build()
        assert len(b.store.blocks) >= 150 and all(len(k) in (36, 38) for k in b.store.blocks)
        wrong += pyevents_wrong(c, b) + oracle_wrong(oracle, c, b) + plan_wrong(harness, c, b)
        plans.setdefault(name.split("__")[1], set()).add(bool(c.plan))
        if "repointed" in name:
            got = [s for _t, _c, s in b.claims]
            assert 65 in got and ((c.scan == (65,) and 1 in got and c.order[0] == 1) or (c.order == (65,) and set(got) == {65} and c.scan[0] == 1)), name
    assert not wrong, wrong[:12]
    assert plans == {"wrap": {True, False}, "one_hash": {True, False}}, plans
    # every shape has a re-pointed receipts link and a re-pointed message-list link, on both kinds of chain
    assert sum("receipts_link_repointed" in n for n in ws.C_AMT) == sum("messages_link_repointed" in n for n in ws.C_AMT) == 2 * len(ws.C_AMT_SHAPES)


@pytest.mark.parametrize("mode", list(ws.MODES))
def test_a_receipts_tree_written_through_the_crafted_store(oracle, mode):
    st, root, items = ws.c_written_receipts(mode)
    n = ws.WRITTEN_N
    status, has, trip, _ = pyevents.scan(st.blocks, root, *ws.ae.FILTER)
    assert (status, has, trip) == (1, [1] * n, [(i, 0, ws.ae.EMITTER) for i in range(n)])
    ost = oracle.store(*st.tables())
    idx = [0, 7, 8, 63, 64, 511, 512, n - 1, n, 4095]
    got, values = ost.amt_get(root, 0, "receipt", idx)
    ost.close()
    assert got.tolist() == [1] * 8 + [32, 32] and values[:8] == [items[i] for i in idx[:8]]


@pytest.mark.parametrize("mode", list(ws.MODES))
def test_a_hamt_written_through_the_crafted_store(oracle, mode):
    c = ws.c_written_hamt(mode)
    assert len(c.keys) > 1300
    few = c._replace(keys=c.keys[::9] + c.keys[-4:], want=c.want[::9] + c.want[-4:], values=c.values[::9])
    wrong = differences(mode, few, *python_answers(c.store.blocks, few)) + differences(mode, c, *hamt_oracle_answers(oracle, c.store, c))
    assert not wrong, wrong[:12]


def test_relabelled_hamt_cases_keep_their_literals(oracle):
    wrong = []
    for name, build in ws.C_HAMT.items():
        c = build()
        if not name.startswith("composite") or name.endswith("any__wrap"):  # (pystorage over 2048 keys takes a second: once)
            wrong += differences(name, c, *python_answers(c.store.blocks, c))
        wrong += differences(name, c, *hamt_oracle_answers(oracle, c.store, c))
    for tree, hops in ws.C_HAMT_REPOINTS:
        for mode in ws.MODES:
            c, under = ws.c_hamt_repointed(tree, mode, hops)
            assert c.want.count(65) >= under > 0
            name = f"{tree}__{mode}__repointed"
            if mode == "one_hash" and tree != "composite_any":  # (pystorage over the composite's 2048 keys takes a second: once)
                wrong += differences(name, c, *python_answers(c.store.blocks, c))
            wrong += differences(name, c, *hamt_oracle_answers(oracle, c.store, c))
    assert not wrong, wrong[:12]
    assert {len(ws.C_HAMT[n]().store.blocks) for n in ws.C_HAMT} >= {12, 43, 51, 52}


@pytest.mark.parametrize("slot", [77, 511])
def test_the_claim_set_composite_puts_every_child_on_one_home(oracle, slot):
    for kind in sorted(ws.hg.COMPOSITE):
        c, ids = ws.e_composite(kind, slot)
        assert len(ids) == 31 and {ws.claim_home(i) for i in ids} == {slot} and len(c.store.blocks) < 1 << 15
        assert (c.keys, c.want, c.values) == ws.hg.COMPOSITE[kind][2:5]  # the same queries, the same literals
        wrong = differences(kind, c, *hamt_oracle_answers(oracle, c.store, c))
        assert not wrong, wrong[:12]


# ---- the source guard ---------------------------------------------------------------------------------------------------------
def _source(*path):
    with open(os.path.join(CSRC, *path), encoding="utf-8") as f:
        return f.read()


def _body(text, signature):
    m = re.search(re.escape(signature) + r"[^{]*\{(.*?)\n\}", text, re.S)
    assert m, signature
    return m.group(1)


def _constant(text, name):
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
    assert m, name
    return int(m.group(1))


def test_source_guard_the_hash_the_sizing_rule_and_the_tiles_are_the_ones_the_cases_were_crafted_against():
    """The crafted CIDs are literals of tests/witness_store_cases.py's restatement of the hash; the engine's hash is read out
    of its source text.  A retuned rotation, multiplier, sizing rule or tile fails HERE and says the cases have to move."""
    dev = _source("kernels", "witness_dev.h")
    for fn, tail in (("uint32_t cid_hash(const CidKey& k)", r"x \*= 0x([0-9A-Fa-f]+)ULL;\s*return uint32_t\(x >> 32\);"),
                     ("uint64_t cid_hash64(const CidKey& k)", r"return x \* 0x([0-9A-Fa-f]+)ULL;")):
        body = _body(dev, fn)
        rot = re.findall(r"\(\(k\.w\[(\d)\] << (\d+)\) \| \(k\.w\[(\d)\] >> (\d+)\)\)", body)
        assert [tuple(map(int, r)) for r in rot] == [(j, ws.ROT[j], j, 64 - ws.ROT[j]) for j in (1, 2, 3)], (fn, rot)
        assert re.search(r"uint64_t x = k\.w\[0\] \^", body) and re.search(r"\^ k\.w\[4\];", body), fn
        m = re.search(tail, body)
        assert m and int(m.group(1), 16) == ws.MULT, fn
    assert re.search(r"uint64_t w\[5\];", dev) and len(re.findall(r"\(a\.w\[\d\] \^ b\.w\[\d\]\)", _body(dev, "bool cid_equal("))) == 5
    # the index's home: the high word under the mask — the builder, the recording probe and its two hand-written copies
    assert len(re.findall(r"uint32_t s = cid_hash\(key\) & mask;", dev)) == 1 and len(re.findall(r"uint32_t s = cid_hash\(key\) & w\.mask;", dev)) == 1
    assert len(re.findall(r"uint32_t s = cid_hash\(key\) & w\.mask;", _source("kernels", "hamt_levels.hip"))) == 1
    assert len(re.findall(r"uint32_t s = cid_hash\(key\) & w\.mask;", _source("kernels", "amt_dense.hip"))) == 1
    assert len(re.findall(r"s = \(s \+ 1\) & (?:w\.)?mask;", dev)) == 2
    # the seen-set: home = high word under the mask, fingerprint = low word, in the three kernels and in exec_find
    ve, vd = _source("kernels", "verify_events.hip"), _source("kernels", "verify_dev.h")
    assert len(re.findall(r"uint32_t s = uint32_t\(h >> 32\) & mask;", ve)) == 3 and len(re.findall(r"uint32_t s = uint32_t\(h >> 32\) & mask;", vd)) == 1
    assert len(re.findall(r"const uint64_t h = cid_hash64\(key\);", ve)) == 3 and len(re.findall(r"const uint64_t h = cid_hash64\(key\);", vd)) == 1
    assert len(re.findall(r"mine = \(\(unsigned long long\)uint32_t\(h\) << 32\) \| i;", ve)) == 2
    assert len(re.findall(r"uint32_t\(cur >> 32\) == uint32_t\(h\)", ve)) == 3 and len(re.findall(r"uint32_t\(cur >> 32\) == uint32_t\(h\)", vd)) == 1
    # the sizing rule, three times
    for path, n in ((("kernels", "cid_index.hip"), "n"), (("host", "exec_state.h"), "n"), (("host", "shard_pull.cpp"), "N")):
        assert re.search(r"uint32_t size = 64;\s*while \(size < 2ull \* %s\) size <<= 1;" % n, _source(*path)), path
    assert [ws.table_mask(n) + 1 for n in (0, 32, 33, 64, 65, 1024, 1025)] == [64, 64, 128, 128, 256, 2048, 4096]
    # the layout: the class cap and the scatter tile
    k1 = _source("kernels", "blake2b_cid.hip")
    assert _constant(k1, "kScatterTile") == ws.SCATTER_TILE
    assert len(re.findall(r"c = c > (\d+) \? \1 : c;", k1)) == 2 and set(re.findall(r"c > (\d+) \? (\d+) : c", k1)) == {(str(ws.CLASS_CAP),) * 2}
    assert re.search(r"chunk_count\(uint32_t len\) \{ return len == 0 \? 1u : \(len \+ 127u\) >> 7; \}", k1)
    assert re.search(r"chunks0 >= %du \? 0xffffffffu : chunks0 \* 128u" % ws.CLASS_CAP, _source("host", "witness.cpp"))
    # the claim set of the HAMT levels
    lv = _source("kernels", "hamt_levels.hip")
    assert _constant(lv, "kClaimSet") == 512 and re.search(r"uint32_t s = \(block \* 2654435761u\) >> 23;", lv)
    assert re.search(r"s = \(s \+ 1u\) & \(kClaimSet - 1u\);", lv)
