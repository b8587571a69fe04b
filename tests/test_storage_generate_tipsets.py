"""CPU: the case table of the storage generator over a chain (tests/storage_gen_chain_cases.py) says what it claims to, the
two judges agree on every (tipset, distinct spec) of it, and the binding exposes the new entry points with the header's
signatures."""
import ctypes as C
import os
import re
import sys

import numpy as np

import ipc_filecoin_proofs_amd as ipcfp
import pystorage_gen as pg
import storage_gen_chain_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import gen_rust_ffi  # noqa: E402

T = gc.CHAIN


def test_case_table_covers_what_it_claims():
    chains, specs = gc.CHAINS, gc.SPECS
    assert sorted({len(c) for c in chains.values()} & {1, 2, 3, 63, 64, 65, 257, 4097}) == [1, 2, 3, 63, 64, 65, 257, 4097]
    assert {len(s) for s in specs.values()} >= {1, 63, 64, 65, 257}
    used_chains, used_specs = {c for c, _ in gc.CASES}, {s for _, s in gc.CASES}
    assert used_chains == set(chains) - {"refused_4097"} and used_specs == set(specs)  # nothing is silently skipped
    assert all(set(c) <= set(T.children) for c in chains.values())
    # run shapes: one run, every spec its own run, one actor in three runs
    def n_runs(name):
        ids = T.batch(specs[name])[0]
        return 1 + int((ids[1:] != ids[:-1]).sum())
    assert n_runs("one_run_4") == 1 and n_runs("own_runs_4") == 4 and n_runs("n65") == 65
    ids = T.batch(specs["one_actor_in_three_runs"])[0]
    starts = [i for i in range(len(ids)) if i == 0 or ids[i] != ids[i - 1]]
    assert sum(int(ids[i]) == gc.AID["flip"] for i in starts) == 3
    # … chosen so that the chain's runs and claims land on and around 256
    sizes = {(len(chains[c]) * n_runs(s), len(chains[c]) * len(specs[s])) for c, s in gc.CASES}
    assert {r for r, _ in sizes} >= {252, 256, 260} and {n for _, n in sizes} >= {252, 256, 260}
    # every failure first, in the middle and last, with sound neighbours
    for kind in gc.FAIL_KINDS:
        for pos, at in (("first", 0), ("middle", 1), ("last", 2)):
            c = chains[f"{kind}_{pos}"]
            assert c[at] == kind and all(k.startswith("h") for i, k in enumerate(c) if i != at)
    assert set(chains["every_tipset_fails"]) == set(gc.FAIL_KINDS)
    twice = chains["same_child_twice"]
    assert twice[0] == twice[1] == twice[3] != twice[2] and twice[4] == twice[5]


def test_literal_statuses_of_the_table():
    """what the table is built to show, as the Python restatement answers it"""
    flip, late, steady, v5 = (T.contracts[n] for n in ("flip", "late", "steady", "v5"))
    old, new = T.py("h0", flip[0], gc.FLIP_SLOT), T.py("h1", flip[0], gc.FLIP_SLOT)
    assert old[0] == new[0] == 1 and old[1]["value"] != new[1]["value"]                   # a slot whose value changes
    assert new[1]["value"] == gc.sc.pad32(gc.FLIP_NEW)
    assert T.py("h1", late[0], late[1][0])[0] == 68 and T.py("h2", late[0], late[1][0])[0] == 1  # a contract that appears
    roots = {T.py(f"h{i}", steady[0], steady[1][0])[1]["storage_root"] for i in range(4)}
    assert roots == {T.steady_root}                                                       # one storage root over four states
    assert len({T.py(f"h{i}", steady[0], steady[1][0])[1]["parent_state_root"] for i in range(4)}) == 4
    a, b = T.py("h2", v5[0], v5[1][0]), T.py("h3", v5[0], v5[1][0])                        # an EVM state that turns V5
    assert a[0] == b[0] == 1 and a[1]["actor_state_cid"] != b[1]["actor_state_cid"] and a[1]["value"] == b[1]["value"]
    want = {"hdr_absent": 65, "hdr_undecodable": 66, "sr_absent": 65, "sr_malformed": 66, "sr_v6": 66}
    for kind, st in want.items():
        got = T.py(kind, flip[0], flip[1][0])
        assert got[0] == st and "storage_root" not in got[1], kind
    seen = set()
    for chain, spec in gc.CASES:
        seen |= set(gc.expected_rows(ipcfp.SCLAIM_DTYPE, chain, spec)[1])
    assert seen == {1, 65, 66, 68}


def test_the_judges_agree_on_every_tipset_and_spec(oracle):
    ost = oracle.store(*T.store.tables())
    checked = 0
    try:
        pairs = set()
        for chain, spec in gc.CASES:
            ids, slots = T.batch(gc.SPECS[spec])
            for key in set(gc.CHAINS[chain]):
                pairs |= {(key, int(a), s.tobytes()) for a, s in zip(ids, slots)}
        for key, aid, slot in sorted(pairs):
            py = T.py(key, aid, slot)
            st, out3, val, wit = T.oracle(ost, key, aid, slot)
            assert st == py[0], (key, aid)
            if st == 1:  # (as test_storage_generate_chain: the oracle gives a failing spec no witness)
                assert wit == py[2], (key, aid)  # the recorded blocks, in `Cid: Ord` order
                for k, f in enumerate(("parent_state_root", "actor_state_cid", "storage_root")):
                    assert pg.cid_of_slot(out3[k]) == py[1][f], (key, aid, f)
                assert bytes(val) == py[1]["value"]
            checked += 1
    finally:
        ost.close()
    # none left out; every child of the table — sound or failing — meets at least the five specs of the failure chains
    assert checked == len(pairs) >= len(T.children) * 5 and {k for k, _, _ in pairs} == set(T.children)


def test_binding_exposes_the_entry_points_with_the_headers_signatures():
    lib = ipcfp.load_library()
    protos = {name: (ret, args) for ret, name, args in gen_rust_ffi.prototypes()}
    vp, u32, u64 = C.c_void_p, C.c_uint32, C.c_uint64
    want = {
        "ipcfp_generate_storage_claims_tipsets": (C.c_int, [vp, vp, vp, vp, u32, vp, vp, u64, C.POINTER(vp)]),
        "ipcfp_generate_storage_claims_tipsets_device": (C.c_int, [vp, vp, vp, vp, u32, vp, vp, u64, C.POINTER(vp)]),
        "ipcfp_generated_storage_claims_tipset_count": (u32, [vp]),
        "ipcfp_generated_storage_claims_tipset_first_error": (u64, [vp, u32]),
        "ipcfp_generated_storage_claims_tipset_block_ids": (vp, [vp, u32, C.POINTER(u64)]),
    }
    for name, (ret, args) in want.items():
        assert name in protos, name
        fn = getattr(lib, name)
        assert fn.restype is ret and list(fn.argtypes) == args, name
        c_args = [a.strip() for a in protos[name][1].split(",")]
        assert len(c_args) == len(args), name
        for c_arg, a in zip(c_args, args):  # a pointer where the header has one, the integer's width where it has none
            if "*" in c_arg:
                assert a in (vp, C.POINTER(vp), C.POINTER(u64)), (name, c_arg)
            else:
                assert a is {"uint32_t": u32, "uint64_t": u64}[c_arg.split()[0]], (name, c_arg)
    header = open(os.path.join(ROOT, "include", "ipcfp.h")).read()
    assert int(re.search(r"#define IPCFP_MAX_GEN_TIPSETS (\d+)", header).group(1)) == 4096
    for m in ("generate_storage_claims_tipsets", "generate_storage_claims_tipsets_device"):
        assert callable(getattr(ipcfp.Witness, m))
    for m in ("n_tipsets", "tipset_first_error", "tipset_block_ids"):
        assert hasattr(ipcfp.GeneratedStorageClaims, m)
    # the null checks are made before anything touches a device: no context, no handle
    h = vp(1)
    assert lib.ipcfp_generate_storage_claims_tipsets(None, None, None, None, 1, None, None, 0, C.byref(h)) == -1
    assert h.value is None
    assert lib.ipcfp_generated_storage_claims_tipset_count(None) == 0
    n = u64(7)
    assert not lib.ipcfp_generated_storage_claims_tipset_block_ids(None, 0, C.byref(n)) and n.value == 0
    assert lib.ipcfp_generated_storage_claims_tipset_first_error(None, 0) == 2**64 - 1
