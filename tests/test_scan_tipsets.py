"""CPU: the pieces of the scan over a CHAIN of tipsets (ipcfp_scan_events_tipsets) that run without a GPU.

  * the library exports both entry points and the binding has both methods;
  * the expected values of tests/scan_tipsets_cases.py: every (chain, tipset) is held to the oracle's single-filter scan per
    spec over the MERGED blocks — the status, the list, the map and the recorded blocks;
  * csrc/host/scan_tipsets_layout.h (the offsets and the prefixes the capacities let through) compiled as a stand-alone
    program with ASan and UBSan (tests/native/scan_tipsets_layout_harness.cpp) and held to scan_tipsets_cases.layout;
  * the case table has every size class the chains are meant to cover."""
import os
import subprocess

import numpy as np

import pyevents
import scan_multi_cases as mc
import scan_tipsets_cases as tc

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "scan_tipsets_layout_harness.cpp")
EXE = os.path.join(HERE, "native", "scan_tipsets_layout_harness")
HDR = os.path.join(HERE, "..", "ipc-filecoin-proofs_amd", "csrc", "host", "scan_tipsets_layout.h")


def test_the_library_exports_both_entry_points_and_the_binding_has_both_methods():
    import ipc_filecoin_proofs_amd as ipcfp

    lib = ipcfp.load_library()
    assert hasattr(lib, "ipcfp_scan_events_tipsets") and hasattr(lib, "ipcfp_scan_events_tipsets_device")
    assert callable(ipcfp.Witness.scan_events_tipsets) and callable(ipcfp.Witness.scan_events_tipsets_device)
    assert ipcfp.MAX_SCAN_TIPSETS == tc.MAX_TIPSETS == 4096
    header = open(os.path.join(HERE, "..", "include", "ipcfp.h")).read()
    assert "#define IPCFP_MAX_SCAN_TIPSETS 4096" in header
    assert ipcfp.binding.KERNEL_IDS["scan_tipsets"] == 25 and "IPCFP_K_SCAN_TIPSETS = 25" in header


# ---- the expected values against the oracle ---------------------------------------------------------------------------------------------
def distinct(specs, pad_sample=4):
    pads = {(a, b, None) for a, b in mc.NOBODY}
    out, n_pad = [], 0
    for sp in dict.fromkeys(specs):
        if sp in pads:
            n_pad += 1
            if n_pad > pad_sample:
                continue
        out.append(sp)
    return out


def test_every_chain_is_held_to_the_oracle_per_tipset_and_per_spec(oracle):
    store, roots = tc.world()
    ost = oracle.store(*store.tables())
    cids = list(store.blocks)
    pairs = left_out = checked = 0
    memo = {}
    try:
        for name, (tipsets, key) in tc.chains().items():
            specs = tc.SPEC_SETS[key]
            for t in tipsets:
                pairs += 1
                if (t, key) in memo:  # (the same root under the same set: the same call of the oracle)
                    continue
                memo[(t, key)] = True
                st, phase, per, has, rec = tc.expected_tipset(t, key)
                got_rec = set()
                has_or = None
                for sp, trip in ((sp, per[specs.index(sp)] if per is not None else None) for sp in distinct(specs)):
                    os_, ohas, otrip, otouched = ost.scan_events(roots[t], sp[0], sp[1], actor=sp[2], cap_receipts=1 << 14, cap_matches=1 << 14,
                                                                 cap_touched=1 << 14)
                    assert os_ == st, (name, t, os_, st)
                    checked += 1
                    if st != pyevents.TRUE:
                        continue
                    assert [tuple(int(x) for x in row) for row in otrip] == trip, (name, t)
                    got_rec |= {bytes(c[:38]) for c in otouched}
                    has_or = ohas.tolist() if has_or is None else [x | y for x, y in zip(has_or, ohas.tolist())]
                if st == pyevents.TRUE:
                    assert has_or == has and got_rec == rec, (name, t)
                    assert phase == 0
                else:
                    assert phase == (1 if tc.receipts_phase_fails(t) else 2)
    finally:
        ost.close()
    assert set(cids) >= {roots[t] for t in roots if t != "own/absent_root"}
    assert left_out <= 0.05 * pairs and pairs > 5000 and checked > 400, (left_out, pairs, checked)


def test_a_chain_of_one_is_the_multi_scan_s_answer():
    store, roots = tc.world()
    for name, (tipsets, key) in tc.chains().items():
        if len(tipsets) != 1:
            continue
        want = mc.expected(store.blocks, roots[tipsets[0]], tc.SPEC_SETS[key])
        e = tc.expected_chain(name)
        assert e["status"] == [want[0]]
        if want[0] == pyevents.TRUE:
            assert e["has"] == want[2] and e["rows"] == mc.merge(want[1]) and e["spec_counts"] == [len(p) for p in want[1]] and e["rec"] == want[3]
        else:
            assert e["has"] == [] and e["rows"] == [] and e["receipt_off"] == e["match_off"] == [0, 0] and e["phase"][0] in (1, 2)


# ---- the layout header -----------------------------------------------------------------------------------------------------------------
def harness_exe():
    if not os.path.exists(EXE) or os.path.getmtime(EXE) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", EXE, SRC], check=True)
    return EXE


def run_layout(status, n_idx, n_match, cap_r, cap_m):
    text = f"{len(status)} {cap_r} {cap_m}\n" + "".join(f"{s} {r} {m}\n" for s, r, m in zip(status, n_idx, n_match))
    p = subprocess.run([harness_exe()], input=text.encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().splitlines()
    head = [int(x) for x in lines[0].split()]
    if head[0] != 0:
        return head, None, None, None
    r_off, m_off = [int(x) for x in lines[1].split()], [int(x) for x in lines[2].split()]
    written = [tuple(int(x) for x in line.split()) for line in lines[3:]]
    assert len(written) == len(status)
    return head, r_off, m_off, written


def held_layout(status, n_idx, n_match, cap_r, cap_m):
    head, r_off, m_off, written = run_layout(status, n_idx, n_match, cap_r, cap_m)
    wr, wm, nr, nm, pr, pm, first = tc.layout(status, n_idx, n_match, cap_r, cap_m)
    assert head == [0, nr, nm, pr, pm, first] and r_off == wr and m_off == wm, (status, cap_r, cap_m)
    for t, (a, b) in enumerate(written):
        assert a == max(0, min(wr[t + 1], pr) - min(wr[t], pr)) and b == max(0, min(wm[t + 1], pm) - min(wm[t], pm))
        if status[t] != 1:
            assert (a, b) == (0, 0) and wr[t] == wr[t + 1] and wm[t] == wm[t + 1]
    assert sum(a for a, _ in written) == pr and sum(b for _, b in written) == pm
    return head


def test_the_layout_header_is_held_to_its_restatement():
    rng = np.random.default_rng(28)
    n_idx, n_match = [5, 0, 7, 3, 9], [2, 0, 4, 0, 6]
    all_caps = lambda r, m: sorted({0, 1, r, m, r + 1, m + 1, 1 << 40})
    # a failing tipset at every position, two, and all of them
    patterns = [[1] * 5] + [[1] * k + [66] + [1] * (4 - k) for k in range(5)] + [[65, 1, 66, 1, 1], [1, 65, 65, 1, 1], [65, 66, 1, 66, 67], [65] * 5]
    for status in patterns:
        wr, wm, nr, nm, *_ = tc.layout(status, n_idx, n_match, 0, 0)
        # caps of 0, 1, inside a tipset, exactly on every boundary, the total and beyond it
        for cap_r in sorted(set(all_caps(nr, nr) + wr + [x + 1 for x in wr] + [max(x - 1, 0) for x in wr])):
            for cap_m in sorted(set(all_caps(nm, nm) + wm + [x + 1 for x in wm])):
                held_layout(status, n_idx, n_match, cap_r, cap_m)
    # T = 1
    for st in (1, 65):
        for cap in (0, 1, 6, 7, 8):
            head = held_layout([st], [7], [7], cap, cap)
            assert head[1] == (7 if st == 1 else 0)
    # T = MAX: seeded shapes, every twentieth tipset failing
    T = tc.MAX_TIPSETS
    status = [66 if t % 20 == 7 else 1 for t in range(T)]
    ri, mi = rng.integers(0, 3000, T).tolist(), rng.integers(0, 50, T).tolist()
    wr, wm, nr, nm, *_ = tc.layout(status, ri, mi, 0, 0)
    for cap_r, cap_m in ((0, 0), (1, 1), (wr[T // 2], wm[T // 2]), (wr[T // 2] + 1, wm[T // 2] - 1), (nr, nm), (nr - 1, nm - 1), (1 << 50, 1 << 50)):
        held_layout(status, ri, mi, cap_r, cap_m)
    # the limits: 2^32 - 1 records over all tipsets are refused, one fewer is not; a failing tipset's numbers count for nothing
    assert run_layout([1, 1], [1, 1], [0xfffffffe, 1], 0, 0)[0][0] == 2
    assert held_layout([1, 1], [1, 1], [0xfffffffd, 1], 0, 0)[2] == 0xfffffffe
    assert held_layout([1, 66, 1], [1, 1 << 63, 1], [0xfffffffd, 0xffffffff, 1], 4, 4)[1:3] == [2, 0xfffffffe]
    assert run_layout([1, 1], [1 << 62, 1 << 62], [0, 0], 0, 0)[0][0] == 1


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
def test_the_case_module_has_what_the_issue_asks_for():
    store, roots = tc.world()
    ch = tc.chains()
    lengths = {len(t) for t, _k in ch.values()}
    assert lengths >= {1, 2, 3, 63, 64, 65, 66, 257, tc.MAX_TIPSETS}
    assert len(tc.refused_chain()) == tc.MAX_TIPSETS + 1
    assert {k for _t, k in ch.values()} == {"1", "2", "8", "1024"} and [len(tc.SPEC_SETS[k]) for k in ("1", "2", "8", "1024")] == [1, 2, 8, 1024]
    exp = {name: tc.expected_chain(name) for name in ch}
    # empty trees first, in the middle, last, two in a row, alone
    empties = {t for t in roots if t != "own/absent_root" and tc.expected_tipset(t, "1")[0] == 1 and tc.expected_tipset(t, "1")[3] == []}
    assert {"ae/size_0", "ae/empty_under_height_1"} <= empties
    pos = {"first": False, "middle": False, "last": False, "row": False, "only": False}
    for tipsets, _k in ch.values():
        e = [t in empties for t in tipsets]
        if len(tipsets) >= 3:
            pos["first"] |= e[0] and not all(e)
            pos["last"] |= e[-1] and not all(e)
            pos["middle"] |= any(e[1:-1]) and not e[0] and not e[-1]
            pos["row"] |= any(a and b for a, b in zip(e, e[1:])) and not all(e)
            pos["only"] |= all(e)
    assert all(pos.values()), pos
    # the same root at two positions; two tipsets that share every block but the root
    assert any(len(set(t)) < len(t) and len(t) <= 8 for t, _k in ch.values())
    a, b = ch["all_blocks_shared_but_the_root"][0]
    assert roots[a] != roots[b] and tc.expected_tipset(a, "8")[2:4] == tc.expected_tipset(b, "8")[2:4]
    # failing tipsets: each phase at the first, a middle and the last position with matching sound tipsets on both sides
    seen = set()
    for name, e in exp.items():
        T = len(e["status"])
        for t, (st, ph) in enumerate(zip(e["status"], e["phase"])):
            if st == 1:
                continue
            where = "first" if t == 0 else "last" if t == T - 1 else "middle"
            left = t == 0 or any(len(r) for r in e["records"][:t])
            right = t == T - 1 or any(len(r) for r in e["records"][t + 1:])
            if T >= 3 and left and right:
                seen.add((ph, where, st))
    for ph in (1, 2):
        for where in ("first", "middle", "last"):
            assert len({st for p, w, st in seen if (p, w) == (ph, where)}) >= 2, (ph, where, seen)
    assert {st for p, _w, st in seen if p == 1} >= {65, 66}  # a root not in the witness, an undecodable node
    assert any({1, 2} <= set(e["phase"]) and 1 in e["status"] for e in exp.values())  # two failing tipsets, one of each phase
    assert any(1 not in e["status"] and len(e["status"]) > 1 for e in exp.values())     # every tipset failing
    # tipset boundaries on the prefix sum's tile: cumulative leaf counts of 1023, 1024, 1025 and 2047, 2048, 2049, with a match
    # at the last receipt of one tipset and the first of the next
    bounds = set()
    for name, (tipsets, key) in ch.items():
        if not name.startswith("tile/"):
            continue
        e = exp[name]
        leaves = 0
        for t in range(len(tipsets) - 1):
            leaves += len(e["maps"][t])  # (dense trees: a map byte per leaf)
            if e["maps"][t] and e["maps"][t + 1] and e["maps"][t][-1] == 1 and e["maps"][t + 1][0] == 1:
                bounds.add(leaves)
    assert bounds >= {1023, 1024, 1025, 2047, 2048, 2049}, bounds
    # heights side by side, one sparse tree among dense ones, all dense with T <= 65 and T = 66, the lies of `count`
    heights = {pyevents.amt_load(store.blocks, roots[t], 0, pyevents.check_receipt).height for t in ch["heights_side_by_side"][0]}
    assert len(heights) >= 4
    sparse = [t for t in ch["one_sparse_among_dense"][0] if sum(1 for _ in tc.expected_tipset(t, "1")[3]) != len(
        list(pyevents.amt_for_each(pyevents.amt_load(store.blocks, roots[t], 0, pyevents.check_receipt))))]
    assert 1 <= len(sparse) < len(ch["one_sparse_among_dense"][0])
    for n in (63, 64, 65, 66):
        assert len(ch[f"dense/{n}"][0]) == n and set(exp[f"dense/{n}"]["status"]) == {1}
    assert set(exp["count_lies"]["status"]) == {1} and pyevents.AMT_COUNT_IS_NOT_CHECKED
    # specs: one event under several specs in two different tipsets, a spec that matches nowhere, an emitter-filtered twin
    e = exp["same_root_twice"]
    twice = [sum(1 for r in rec if r[3] in (0, 6)) for rec in e["records"]]
    assert sum(1 for n in twice if n >= 2) >= 2
    every = [sum(exp[name]["spec_counts"][j] for name, (_t, k) in ch.items() if k == "8") for j in range(8)]
    assert every[3] == 0 and 0 < every[1] < every[0] == every[6] and every[2] > 0 and every[5] > every[7] > 0, every
