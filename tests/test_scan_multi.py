"""CPU: the pieces of the scan over a SET of event specs (ipcfp_scan_events_multi) that run without a GPU.

  * csrc/kernels/filter_set.h (build on the host, probe on the device) compiled for the host as a stand-alone program
    (tests/native/filter_set_harness.cpp) and held to a Python dict: seeded sets of 1 to 1024 specs, the trap keys of
    tests/scan_multi_cases.py, duplicates, emitter filters, and keys that share one home slot.  The same program tells the
    case module which keys collide, so that the GPU test holds a true collision chain.
  * the expected values: pyevents.scan per spec and the oracle's single-filter scan per spec agree on every (tipset, set)
    of the case module, the module's one-walk model equals the per-spec scans, and pyevents.generate equals the oracle's
    generator on the bundle cases.
  * the order contract restated (scan_multi_cases.merge)."""
import os
import subprocess

import numpy as np
import pytest

import event_chain_cases as ec
import pyevents
import scan_multi_cases as mc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "filter_set_harness.cpp")
EXE = os.path.join(HERE, "native", "filter_set_harness")
HDR = os.path.join(HERE, "..", "ipc-filecoin-proofs_amd", "csrc", "kernels", "filter_set.h")


def harness_exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-o", EXE, SRC], check=True)
    return EXE


def slot_of(n_slots, keys):
    text = f"{n_slots} {len(keys)}\n" + "\n".join(k.hex() for k in keys) + "\n"
    out = subprocess.run([harness_exe(), "slots"], input=text.encode(), stdout=subprocess.PIPE, check=True).stdout.split()
    assert len(out) == len(keys)
    return [int(x) for x in out]


def probe(specs, probes):
    """specs [(topic0, topic1, actor | None)], probes [(64-byte key, emitter)] → (n_slots, n_groups, [(group, compares, [spec])])"""
    lines = [str(len(specs))] + [f"{(a + b).hex()} {0 if act is None else 1} {0 if act is None else act}" for a, b, act in specs]
    lines += [str(len(probes))] + [f"{k.hex()} {em}" for k, em in probes]
    out = subprocess.run([harness_exe(), "probe"], input=("\n".join(lines) + "\n").encode(), stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    n_slots, n_groups = (int(x) for x in out[0].split())
    rows = [[int(x) for x in line.split()] for line in out[1:]]
    assert len(rows) == len(probes)
    return n_slots, n_groups, [(r[0], r[1], r[2:]) for r in rows]


def model(specs, probes):
    """the Python dict: key → members in ascending spec index; a probe's answer is the members whose emitter filter passes"""
    groups = {}
    for j, (a, b, act) in enumerate(specs):
        groups.setdefault(a + b, []).append((j, act))
    return len(groups), [None if k not in groups else [j for j, act in groups[k] if act is None or act == em] for k, em in probes]


def held_to_the_dict(specs, probes):
    n_slots, n_groups, got = probe(specs, probes)
    want_groups, want = model(specs, probes)
    assert n_slots >= 2 * len(specs) and n_slots & (n_slots - 1) == 0 and n_groups == want_groups
    for (g, compares, members), w, (k, em) in zip(got, want, probes):
        if w is None:
            assert g == -1 and members == [], (k.hex(), em)
        else:
            assert g >= 0 and compares >= 1 and members == w, (k.hex(), em, members, w)
        assert compares <= n_groups
    return got


def rand_key(rng):
    return bytes(rng.integers(0, 256, 64, dtype=np.uint8))


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 500, 1023, 1024])
def test_probe_equals_a_dict_on_seeded_sets(n):
    rng = np.random.default_rng(9000 + n)
    keys = [rand_key(rng) for _ in range(max(1, n * 2 // 3))]
    specs = []
    for _ in range(n):  # duplicates of keys, with and without emitters
        k = keys[int(rng.integers(len(keys)))]
        specs.append((k[:32], k[32:], None if rng.integers(3) == 0 else int(rng.integers(0, 4))))
    probes = [(k, int(rng.integers(0, 4))) for k in keys] + [(rand_key(rng), 1) for _ in range(64)]
    probes += [(bytes(k[:63]) + bytes([k[63] ^ 1]), 0) for k in keys[:32]] + [(bytes([k[0] ^ 0x80]) + bytes(k[1:]), 0) for k in keys[:32]]
    held_to_the_dict(specs, probes)


def test_probe_on_the_trap_keys_duplicates_and_emitters():
    a, b = mc.pair(0)
    specs = [(a, b, None), (a, mc.flip(b, 31), None), (mc.flip(a, 0), b, None), (b, a, None), (a, a, None), (bytes(32), bytes(32), None),
             (a, b, 8001), (a, b, 0), (a, b, None), (a, b, 8001)]
    probes = [(x + y, em) for x, y, _ in specs for em in (0, 8001, 7)] + [(b + b, 0), (bytes(64), 0), (b"\xff" * 64, 0)]
    got = held_to_the_dict(specs, probes)
    assert got[0][2] == [0, 7, 8] and got[1][2] == [0, 6, 8, 9]  # emitter 0: has_actor = 1, actor = 0 passes; 8001: both 8001 specs


def test_the_recorded_home_slots_are_the_harness_s():
    """tests/golden/scan_multi_home_slots.json, from which the GPU test picks its collision chain, is what the harness says"""
    present, nobody = mc.slot_candidates()
    keys = [a + b for a, b in present + nobody]
    assert mc.recorded_slot_of(mc.CHAIN_SLOTS, keys) == slot_of(mc.CHAIN_SLOTS, keys)
    assert mc.spec_sets_over_edges(mc.recorded_slot_of) == mc.spec_sets_over_edges(slot_of)


def test_keys_forced_onto_one_home_slot():
    """a chain of keys with ONE home slot, present and absent: every present one is found behind the others, every absent
    one costs probes and compares but is never an answer"""
    rng = np.random.default_rng(77)
    cand = [rand_key(rng) for _ in range(4000)]
    size, n_slots = 40, 128
    slots = slot_of(n_slots, cand)
    by = {}
    for k, s in zip(cand, slots):
        by.setdefault(s, []).append(k)
    chain = max(by.values(), key=len)
    assert len(chain) >= 12
    present, absent = chain[: len(chain) // 2], chain[len(chain) // 2:]
    specs = [(k[:32], k[32:], None) for k in present]
    specs += [(k[:32], k[32:], None) for k in cand if k not in chain][: size - len(specs)]
    assert len(specs) == size
    n_slots_got, _, got = probe(specs, [(k, 0) for k in present + absent])
    assert n_slots_got == n_slots
    held_to_the_dict(specs, [(k, 0) for k in present + absent])
    assert [g[0] >= 0 for g in got] == [True] * len(present) + [False] * len(absent)


def test_the_case_module_has_what_the_issue_asks_for():
    clean, failing = mc.rc_split()
    assert len(clean) >= 90 and len(failing) >= 5 and len(clean) + len(failing) == len(ec.RC)
    st, parts, n_rc = mc.edges()
    assert n_rc == len(clean)
    pres = mc.present_pairs(st.blocks, parts["receipts"])
    own = [k for k in pres if k[0] not in ec.T]
    assert len(own) >= 128
    assert sorted(pres[mc.pair(0)]) == [0, 7000, 8001, 8002] and pres[mc.pair(5)] == [7005, 8100, 8101]
    assert mc.pair(9) in pres and (mc.pair(9)[1], mc.pair(9)[0]) in pres
    assert pyevents.scan(st.blocks, parts["receipts"], *ec.FILTER)[0] == pyevents.TRUE
    sets = mc.spec_sets_over_edges(slot_of)
    assert {len(sets[f"size_{n}"]) for n in (1, 2, 63, 64, 65, 1024)} == {1, 2, 63, 64, 65, 1024}
    assert sorted(map(repr, sets["shuffled_0"])) == sorted(map(repr, sets["shuffled_1"])) and sets["shuffled_0"] != sets["shuffled_1"]
    chain = sets["one_home_slot"]
    home = slot_of(64, [a + b for a, b, _ in chain[:6]])
    assert len(set(home[:3])) == 1 and len(set(home[3:6])) == 1 and all((a, b) in pres for a, b, _ in chain[:3])
    assert len(mc.err_tipsets()) == 5
    for _name, est, eparts in mc.err_tipsets():
        assert pyevents.scan(est.blocks, eparts["receipts"], *ec.FILTER)[0] != pyevents.TRUE


def distinct(specs, pad_sample=6):
    """the distinct specs of a set, with only a sample of the padding nobody emits"""
    pads = {(a, b, None) for a, b in mc.NOBODY}
    out, n_pad = [], 0
    for sp in dict.fromkeys(specs):
        if sp in pads:
            n_pad += 1
            if n_pad > pad_sample:
                continue
        out.append(sp)
    return out


def every_tipset_and_set():
    st, parts, _ = mc.edges()
    for name, specs in mc.spec_sets_over_edges(slot_of).items():
        yield f"edges/{name}", st, parts["receipts"], specs, 0, None
    tst, roots = mc.tiles()
    for n, root in roots.items():
        yield f"tiles/{n}", tst, root, mc.TILE_SPECS, 0, None
    for lo, hi in mc.TILE_RANGES:
        yield f"tiles/2049[{lo},{hi})", tst, roots[2049], mc.TILE_SPECS, lo, hi
    sst, sparts = mc.short_order()
    yield "short_order", sst, sparts["receipts"], [(*mc.SHORT_X, None)] + [(a, b, None) for a, b in mc.SHORT_OTHERS], 0, None


def test_the_one_walk_model_equals_pyevents_scan_per_spec():
    n = 0
    for name, st, root, specs, lo, hi in every_tipset_and_set():
        some = distinct(specs)
        assert mc.expected(st.blocks, root, some, lo, hi) == mc.expected_by_scans(st.blocks, root, some, lo, hi), name
        n += len(some)
    assert n > 300
    for name, st, parts in mc.err_tipsets():
        want = pyevents.scan(st.blocks, parts["receipts"], *ec.FILTER)[0]
        assert mc.expected(st.blocks, parts["receipts"], [(*ec.FILTER, None), (*mc.pair(0), 7)])[0] == want != pyevents.TRUE, name


def test_pyevents_scan_and_the_oracle_scan_agree_per_spec(oracle):
    checked = 0
    stores = {}
    for name, st, root, specs, lo, hi in every_tipset_and_set():
        if lo or hi is not None:
            continue  # (the oracle's scan has no receipt range; the range cases rest on pyevents.scan's own)
        if id(st) not in stores:
            stores[id(st)] = oracle.store(*st.tables())
        ost = stores[id(st)]
        some = distinct(specs)
        _st, per, _has, _rec = mc.expected(st.blocks, root, some)
        memo = {}
        for sp, trip in zip(some, per):
            if sp in memo:
                continue
            memo[sp] = True
            want = pyevents.scan(st.blocks, root, *sp) if len(trip) or checked % 7 == 0 else None
            os_, ohas, otrip, otouched = ost.scan_events(root, sp[0], sp[1], actor=sp[2], cap_receipts=1 << 12, cap_matches=1 << 13, cap_touched=1 << 13)
            assert os_ == pyevents.TRUE, (name, os_)
            assert [tuple(int(x) for x in row) for row in otrip] == trip, name
            if want is not None:
                assert ohas.tolist() == want[1] and {bytes(c[:38]) for c in otouched} == want[3], name
            checked += 1
    for ost in stores.values():
        ost.close()
    assert checked > 200
    for name, st, parts in mc.err_tipsets():
        ost = oracle.store(*st.tables())
        for sp in ((*ec.FILTER, None), (*mc.pair(3), 9)):
            assert ost.scan_events(parts["receipts"], sp[0], sp[1], actor=sp[2], cap_receipts=64, cap_matches=64, cap_touched=64)[0] == \
                pyevents.scan(st.blocks, parts["receipts"], *sp)[0] != pyevents.TRUE, name
        ost.close()


def test_pyevents_generate_and_the_oracle_generator_agree_on_the_bundle_cases(oracle):
    seen_err = seen_ok = 0
    for name, st, parts, named in mc.bundle_cases():
        ost = oracle.store(*st.tables())
        for t0, t1, actor in dict.fromkeys((*mc.named_pair(q), actor) for q, actor in named):
            gw = pyevents.generate(st.blocks, parts["parents"], parts["child"], t0, t1, actor)
            gs, gtrip, gmsg, gwit = ost.generate_event_proof(parts["parents"], parts["child"], t0, t1, actor=actor, cap_proofs=1 << 12, cap_witness=1 << 12)
            assert gs == gw[0], (name, gs, gw[0])
            if gs == 1:
                seen_ok += 1
                assert [(*(int(v) for v in t), bytes(m[:38])) for t, m in zip(gtrip, gmsg)] == gw[1], name
                assert {bytes(c[:38]) for c in gwit} == gw[2], name
            else:
                seen_err += 1
        ost.close()
    assert seen_ok > 40 and seen_err >= 2
    # the per-spec Err of short_order: X alone fails with the generator's own Err, the others succeed
    sst, sparts = mc.short_order()
    assert pyevents.generate(sst.blocks, sparts["parents"], sparts["child"], *mc.SHORT_X)[0] == pyevents.ERR
    assert all(pyevents.generate(sst.blocks, sparts["parents"], sparts["child"], a, b)[0] == pyevents.TRUE for a, b in mc.SHORT_OTHERS)


def test_merge_restates_the_order_contract():
    per = [[(0, 0, 5), (2, 1, 6)], [], [(0, 0, 5), (1, 3, 7), (2, 1, 6)], [(2, 0, 9)]]
    assert mc.merge(per) == [(0, 0, 5, 0), (0, 0, 5, 2), (1, 3, 7, 2), (2, 0, 9, 3), (2, 1, 6, 0), (2, 1, 6, 2)]
    # the stable selection spec == j is list j again
    for j, trip in enumerate(per):
        assert [(e, i, em) for e, i, em, s in mc.merge(per) if s == j] == trip
