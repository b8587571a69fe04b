"""CPU: the get primitives' named cases (tests/hamt_get_cases.py) under three judges — the LITERAL status and value bytes
written next to each key, tests/pystorage.py `hamt_get_bytes` (an independent Python restatement of
`Hamt::load_with_bit_width(..)?.get(key)?`) and the C++ oracle — and the assertions that hold the LIST: every status
occurs, every limit of the engine's fast routes has a case on each side, and those limits are still the ones the source
states."""
import collections
import os
import re

import pytest

import hamt_get_cases as hg
import pystorage

NAMES = list(hg.CASES)
CHECKS = {"actor_state": pystorage.check_actor_state, "vec_u8": pystorage.check_vec_u8, "any": lambda x: x}
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ipc-filecoin-proofs_amd", "csrc")


def python_answers(blocks, c):
    """→ ([status], [value bytes of the TRUE keys]) of pystorage"""
    status, values = [], []
    for key in c.keys:
        try:
            v = pystorage.hamt_get_bytes(blocks, c.root, c.bw, key, CHECKS[c.kind])
            status.append(hg.NOT_FOUND if v is None else hg.TRUE)
            if v is not None:
                values.append(v)
        except pystorage.Err as e:
            status.append(e.status)
    return status, values


def oracle_answers(oracle, store, c):
    data, off, lens, cids = hg.tables(store)
    st = oracle.store_var(data, off, lens, cids)
    status, values = st.hamt_get(c.root, c.bw, c.kind, c.keys, cap=max([len(v) for v in c.values] + [8]) + 8)
    st.close()
    return status.tolist(), [v for s, v in zip(status, values) if s == hg.TRUE]


def differences(name, c, status, values):
    out = [(name, key[:16], got, want) for key, got, want in zip(c.keys, status, c.want) if got != want]
    if not out and values != c.values:
        out.append((name, "values", [v[:16] for v, w in zip(values, c.values) if v != w][:3]))
    return out


@pytest.mark.parametrize("group", range(8))
def test_pystorage_gives_every_literal(group):
    wrong = []
    for name in NAMES[group::8]:
        c = hg.CASES[name]
        wrong += differences(name, c, *python_answers(c.store.blocks, c))
    assert not wrong, wrong[:20]


@pytest.mark.parametrize("group", range(8))
def test_oracle_gives_every_literal(oracle, group):
    wrong = []
    for name in NAMES[group::8]:
        c = hg.CASES[name]
        wrong += differences(name, c, *oracle_answers(oracle, c.store, c))
    assert not wrong, wrong[:20]


def test_merged_witness_changes_no_answer(oracle):
    """All cases' blocks in one store — the arrangement the GPU test uploads once: a case's nodes among foreign blocks."""
    store = hg.merged()
    assert len(store.blocks) > 2000
    wrong = []
    for name, c in hg.CASES.items():
        wrong += differences(name, c, *oracle_answers(oracle, store, c))
    assert not wrong, wrong[:20]
    for name in NAMES[::7]:
        c = hg.CASES[name]
        wrong += differences(name, c, *python_answers(store.blocks, c))
    assert not wrong, wrong[:20]


def limits_with_cases():
    have = collections.defaultdict(set)
    for m in hg.META.values():
        if m["limit"]:
            have[m["limit"][0]].add(m["limit"][1])
    return have


def test_the_list_covers_what_it_must():
    assert 200 <= len(hg.CASES) <= 450
    seen = collections.Counter(s for c in hg.CASES.values() for s in c.want)
    assert {1, 32, 65, 66, 70} <= set(seen), seen
    for kind in ("actor_state", "any"):
        assert sum(1 for c in hg.CASES.values() if c.kind == kind) >= 100
    assert sum(1 for c in hg.CASES.values() if c.kind == "vec_u8") >= 60
    have, L = limits_with_cases(), hg.LIMITS
    # every limit has a case on each side
    assert {L["table_pointers"], L["table_pointers"] + 1} <= have["pointers"]
    assert {L["bitfield_bits"], L["bitfield_bits"] + 1, 256} <= have["bitfield_bits"] and 33 in have["bitfield_bytes"]
    for n in L["stage_entries"] + (L["tab_entries"],):
        assert {n, n + 1} <= have["entries"], n
    assert {97, 256} <= have["bucket"]
    # the BUCKET nodes straddle every stage size.  A link-only node does so at the small stage alone: 32 links cannot fill
    # 4 KB, so the longer link nodes hold more than 32 pointers and every fast route declines them for that before it looks
    # at their length — they are cases of the pointer limit at those lengths, not of the stage edge
    for stage in L["stage_bytes"]:
        edge = stage - hg.STAGE_SLACK
        at = {m["limit"][1] for m in hg.META.values() if m["group"] == "length" and m["shape"] == "buckets"}
        assert {edge - 1, edge, edge + 1} <= at, stage
    edge = L["stage_bytes"][0] - hg.STAGE_SLACK
    tabled_links = {m["limit"][1] for m in hg.META.values() if m["group"] == "length" and m["shape"] == "links" and m["pointers"] <= L["table_pointers"]}
    assert {edge - 1, edge, edge + 1, L["outline_min_len"] - 1, L["outline_min_len"]} <= tabled_links
    assert all(m["pointers"] > L["table_pointers"] for m in hg.META.values() if m.get("shape") == "links" and m["limit"][1] > 2 * L["outline_min_len"])
    assert {L["outline_min_len"] - 1, L["outline_min_len"]} <= have["block_len"]
    assert any(7424 < n < 1 << 16 for n in have["block_len"]) and any(n >= 1 << L["offset_bits"] for n in have["block_len"])
    assert {(1 << L["key_len_bits"]) - 1, 1 << L["key_len_bits"], (1 << L["key_len_bits"]) + 1} <= have["key_len"] | set(hg.KEY_LENGTHS)
    assert {51, 52} <= have["depth5"] and {256, 257} <= have["depth1"] and {32, 33} <= have["depth8"]
    assert {0, 1, 2, 4, 7, 8, 9, 32, (1 << 32) - 1} <= have["width"]
    assert {128} <= have["balance_len"]
    # links: every spelling at the root, at level 1 and at level 3
    for variant in hg.LINK_VARIANTS:
        assert {m["level"] for m in hg.META.values() if m.get("variant") == variant} == {0, 1, 3}, variant
    # every flaw as the first, a middle and the last entry
    for flaw in hg.FLAWS:
        assert sum(1 for n, m in hg.META.items() if m.get("flaw") == flaw and n.endswith("__actor_state")) == 3
    # the over-long chains outrun every count of levels the host queues (14 at the most: csrc/host/primitives.cpp)
    assert all(len(hg.CASES[n].store.blocks) > 14 + 2 for n, m in hg.META.items() if m["group"] == "depth" and hg.MAX_DEPTH in hg.CASES[n].want)


def test_level_cases_go_in_batches_wide_enough_for_the_fused_top(oracle):
    """The cases built at level 1 and 3 reach the fused top levels only in a batch of at least 32 (two levels) and 1024
    (three) queries over a witness of as many blocks: `wide` makes that batch, and its literals hold under both judges."""
    assert hg.FUSED_TOP_MIN_QUERIES == (32, 1024) and len(hg.LEVEL_CASES) >= 60
    store = hg.merged()
    assert len(store.blocks) >= 1024
    assert {hg.META[n].get("variant") for n in hg.LEVEL_CASES} >= set(hg.LINK_VARIANTS)
    assert {(hg.META[n]["level"], hg.CASES[n].kind) for n in hg.LEVEL_CASES} == {(lv, k) for lv in (1, 3) for k in hg.KINDS}
    data, off, lens, cids = hg.tables(store)
    st = oracle.store_var(data, off, lens, cids)
    wrong = []
    for n in hg.LEVEL_CASES:
        c, w = hg.CASES[n], hg.wide(n)
        assert len(w.keys) >= 32 and len(w.keys) >= 1024 and len(set(w.keys)) == len(w.keys)
        assert [s for k, s in zip(w.keys, w.want) if k in c.keys] == c.want and w.values == c.values
        status, values = st.hamt_get(w.root, w.bw, w.kind, w.keys, cap=256)
        wrong += differences(n, w, status.tolist(), [v for s, v in zip(status, values) if s == hg.TRUE])
        if hg.META[n]["level"] == 3 or w.kind == "actor_state":
            wrong += differences(n, w, *python_answers(store.blocks, w))
    st.close()
    assert not wrong, wrong[:20]


def test_the_link_composite_holds_every_spelling_at_two_levels():
    names = [n for n, _ in hg.LINK_COMPOSITE_CHILDREN]
    assert set(hg.LINK_VARIANTS) <= set(names) and {v + "_one_level_down" for v in hg.LINK_VARIANTS} <= set(names)
    for kind, (st, root, keys, want, values, child, lens) in hg.LINK_COMPOSITE.items():
        assert len(keys) >= 2048 and len(set(child)) == 32 and {1, 32, 65, 66} <= set(want)


def test_the_composite_tree_meets_every_size_class():
    for kind, (st, root, keys, want, values, child, lens) in hg.COMPOSITE.items():
        assert len(keys) >= 2048 and len(set(keys)) == len(keys)
        assert {hg.stage_class(n) for n in lens if n is not None} == {0, 1, 2, None}
        assert len(set(child)) == 32 >= 25 and min(collections.Counter(child).values()) >= 32
        assert {1, 32, 65, 66} <= set(want) if kind == "actor_state" else {1, 32, 65} <= set(want)
        # the flawed children are what tells the kinds apart
        assert (want.count(66) > 300) == (kind == "actor_state")


def _source(*path):
    with open(os.path.join(CSRC, *path), encoding="utf-8") as f:
        return f.read()


def _constant(text, name):
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, text)
    assert m, name
    return int(m.group(1))


def test_limit_guard_the_source_still_states_the_limits_the_cases_straddle():
    """The case list's lengths and counts are literals of tests/hamt_get_cases.py; the engine's constants are read out of its
    source text.  A retuning fails HERE and says which cases have to move — it does not silently leave the edge bare."""
    table, levels, host = _source("kernels", "hamt_table.h"), _source("kernels", "hamt_levels.hip"), _source("host", "primitives.cpp")
    L = hg.LIMITS
    assert _constant(table, "kHamtTablePointers") == L["table_pointers"]
    assert _constant(table, "kHamtTabEntries") == L["tab_entries"]
    assert _constant(table, "kHamtOutlineMinLen") == L["outline_min_len"]
    assert tuple(_constant(levels, f"kCoop{s}Stage") for s in ("Small", "Mid", "Big")) == L["stage_bytes"]
    assert tuple(_constant(levels, f"kCoop{s}Entries") for s in ("Small", "Mid", "Big")) == L["stage_entries"]
    slack = set(re.findall(r"len \+ (\d+)u <= kCoop\w*Stage", levels))
    assert slack == {str(hg.STAGE_SLACK)}, slack
    m = re.search(r"\(n >= (\d+) \|\| levels_mode > 0\)", host)
    assert m and int(m.group(1)) == L["levels_switch"]
    # the records' field widths
    assert re.search(r"uint64_t bitfield;", table) and L["bitfield_bits"] == 64
    assert re.search(r"uint16_t ptr_off\[kHamtTablePointers\]", table) and re.search(r"uint16_t key_off, val_off, val_len;", table)
    assert L["offset_bits"] == 16 and re.search(r"uint8_t key_len, pad;", table) and L["key_len_bits"] == 8
    assert re.search(r"uint8_t first\[kHamtTablePointers\]", table) and re.search(r"uint8_t count\[kHamtTablePointers\]", table)
    # … and the case list still straddles them (the literals the cases were built from)
    for stage in L["stage_bytes"]:
        assert {stage - hg.STAGE_SLACK - 1, stage - hg.STAGE_SLACK, stage - hg.STAGE_SLACK + 1} <= set(hg.BLOCK_LENGTHS)
    assert {L["outline_min_len"] - 1, L["outline_min_len"]} <= set(hg.BLOCK_LENGTHS)
    assert set(L["stage_entries"]) | {n + 1 for n in L["stage_entries"][:2]} <= set(hg.ENTRY_TOTALS)
    assert {255, 256} <= set(hg.KEY_LENGTHS)
