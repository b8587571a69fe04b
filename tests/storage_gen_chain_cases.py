"""ONE merged store holding a chain of hand-built children for the storage generator over a chain
(ipcfp_generate_storage_claims_tipsets*), composed from the primitives of tests/storage_chain_cases.py, tests/pyhamt.py and
tests/pystorage_gen.py.

Four states that share most of their nodes — each differs from its predecessor in one contract:

    s0  the base
    s1  the slot FLIP_SLOT of contract "flip" changes its value
    s2  contract "late" appears (its actor is absent before)
    s3  the EVM state of contract "v5" turns V5

Contract "steady" keeps ONE storage root over all four.  Sound children are headers of distinct heights over those states;
the failing children are a header nobody stored, a header that does not decode, and headers whose StateRoot is absent,
malformed or of a version above 5.

    CHAINS   name → [child key, …]              (a key of CHILDREN; the caller's epoch of position t is EPOCH0 + t)
    SPECS    name → [(contract, k-th slot), …]   (one list, posed at every child)
    CASES    [(chain name, spec list name), …]

and the judges' answers per (child, distinct spec), cached: a spec's answer is a function of (child, actor, slot)."""
import hashlib

import numpy as np

import pyamt
import pyhamt
import pystorage_gen
import storage_chain_cases as sc
import storage_gen_cases as sg
from pyamt import NULL, array, bstr, link, uint

EPOCH0 = 880_000  # the caller's epoch of the chain's first child; never compared with a header's height
FLIP_SLOT = sc.S[2]
FLIP_NEW = bytes(range(0x30, 0x48))

AID = {"flip": 3001, "late": 3002, "steady": 3003, "v5": 3004, "nobody": 3999}
FAIL_KINDS = ("hdr_absent", "hdr_undecodable", "sr_absent", "sr_malformed", "sr_v6")


class Chain:
    def __init__(self):
        st = self.store = pyamt.Store()
        code, bytecode, info, receipts, messages = (pyamt.cid_of(n.encode()) for n in ("code", "bytecode", "info", "rcpt", "msgs"))
        parent = pyamt.cid_of(b"parent header")

        def evm(root, nonce, v5=False):
            head = [link(bytecode), bstr(hashlib.sha256(b"bytecode").digest()), link(root)]
            return st.put(array(head + ([uint(nonce), NULL] if v5 else [NULL, uint(nonce), NULL])))

        def state(contracts):
            """{name: EVM state CID} → the StateRoot's CID; a dozen bystanders keep the actors HAMT more than one node deep"""
            actors = {}
            for name, astate in contracts.items():
                actors[sc.actor_key(AID[name])] = array([link(code), link(astate), uint(AID[name] % 997), bstr(b"\x00\x05"), NULL])
            for k in range(40):
                aid = 3100 + k
                actors[sc.actor_key(aid)] = array([link(code), link(pyamt.cid_of(b"state of %d" % aid)), uint(1), bstr(b"\x00\x05"), NULL])
            self.actor_roots.append(pyhamt.build_hamt(st, actors))
            return st.put(array([uint(5), link(self.actor_roots[-1]), link(info)]))

        def header(sroot, height):
            return st.put(array([bstr(b"\x00\xe8\x07"), array([bstr(b"vrf")]), NULL, array([]), array([]), array([link(parent)]),
                                 bstr(b"\x00\x01"), uint(height), link(sroot), link(receipts), link(messages), NULL,
                                 uint(1_700_000_000 + height), NULL, uint(0), bstr(b"\x00\x64")]))

        self.actor_roots = []
        flip_pairs_new = [(k, FLIP_NEW if k == FLIP_SLOT else v) for k, v in sc.PAIRS]
        flip_old = st.put(sc.layout("B1", sc.PAIRS)(st))
        flip_new = st.put(sc.layout("B1", flip_pairs_new)(st))
        late_root = st.put(sc.layout("A3", sc.PAIRS[:3])(st))
        steady_root = st.put(sc.layout("C", sc.MANY)(st))
        v5_root = st.put(sc.layout("A2", sc.PAIRS[:5])(st))
        self.steady_root = steady_root
        e_flip_old, e_flip_new = evm(flip_old, 11), evm(flip_new, 12)
        e_late, e_steady = evm(late_root, 21), evm(steady_root, 31)
        e_v5_old, e_v5_new = evm(v5_root, 41), evm(v5_root, 42, v5=True)
        self.states = [
            state({"flip": e_flip_old, "steady": e_steady, "v5": e_v5_old}),
            state({"flip": e_flip_new, "steady": e_steady, "v5": e_v5_old}),
            state({"flip": e_flip_new, "steady": e_steady, "v5": e_v5_old, "late": e_late}),
            state({"flip": e_flip_new, "steady": e_steady, "v5": e_v5_new, "late": e_late}),
        ]
        # what a contract answers: name → [(slot, {state index: literal status})]; 1 everywhere unless said otherwise
        three = [sc.S[2], sc.ABSENT, sc.S[1]]
        self.contracts = {
            "flip": (AID["flip"], three + [sc.S[0]]),
            "late": (AID["late"], [sc.S[0], sc.S[1], sc.ABSENT]),
            "steady": (AID["steady"], [k for k, _ in sc.MANY[:24]] + [sc.slot(f"nobody{i}") for i in range(8)]),
            "v5": (AID["v5"], [sc.S[0], sc.S[4], sc.ABSENT]),
            "nobody": (AID["nobody"], [sc.S[0], sc.S[3]]),
        }
        self.children = {}
        self.state_of = {}
        for i in range(8):  # h0 … h7: two headers per state, in state order twice over
            self.children[f"h{i}"] = header(self.states[i % 4], 1000 + i)
            self.state_of[f"h{i}"] = i % 4
        self.children["hdr_absent"] = pyamt.cid_of(b"a child header nobody stored")
        self.children["hdr_undecodable"] = st.put(array([uint(1), bstr(b"not a header")]))
        self.children["sr_absent"] = header(pyamt.cid_of(b"a StateRoot nobody stored"), 2001)
        self.children["sr_malformed"] = header(st.put(array([uint(5), bstr(b"no link")])), 2002)
        self.children["sr_v6"] = header(st.put(array([uint(6), link(self.actor_roots[0]), link(info)])), 2003)
        self.cids = list(st.blocks)
        self._py, self._orc = {}, {}

    # ---- spec lists: [(contract, k-th slot of it)] → (actor ids u64[n], slots u8[n, 32]) ----
    def batch(self, picks):
        ids = np.array([self.contracts[c][0] for c, _ in picks], dtype=np.uint64)
        slots = np.zeros((len(picks), 32), dtype=np.uint8)
        for i, (c, k) in enumerate(picks):
            s = self.contracts[c][1]
            slots[i] = np.frombuffer(s[k % len(s)], dtype=np.uint8)
        return ids, slots

    def runs(self, shape):
        return [(c, k) for c, n in shape for k in range(n)]

    # ---- the judges, per (child, distinct spec) ----
    def py(self, child_key, aid, slot):
        key = (child_key, int(aid), bytes(slot))
        if key not in self._py:
            self._py[key] = pystorage_gen.generate(self.store.blocks, self.children[child_key], key[1], key[2])
        return self._py[key]

    def oracle(self, ost, child_key, aid, slot):
        key = (child_key, int(aid), bytes(slot))
        if key not in self._orc:
            st, out3, val, wit = ost.generate_storage_proof(self.children[child_key], key[1], key[2])
            self._orc[key] = (st, out3.copy(), val.copy(), [pystorage_gen.cid_of_slot(w) for w in wit])
        return self._orc[key]

    def answers(self, child_key, ids, slots):
        return [self.py(child_key, a, s.tobytes()) for a, s in zip(ids, slots)]


CHAIN = Chain()
C = CHAIN


def _cycle(keys, n):
    return [keys[i % len(keys)] for i in range(n)]


SOUND = [f"h{i}" for i in range(8)]
MIXED = ["h0", "h1", "sr_v6", "h2", "h3", "hdr_absent", "h4", "h5", "h5", "sr_malformed", "h6", "h7", "h1"]

CHAINS = {f"t{n}": _cycle(SOUND, n) for n in (1, 2, 3, 4)}
CHAINS.update({f"t{n}": _cycle(MIXED, n) for n in (63, 64, 65, 257)})
for kind in FAIL_KINDS:  # every failure first, in the middle and last, between sound neighbours
    CHAINS[f"{kind}_first"] = [kind, "h1", "h2"]
    CHAINS[f"{kind}_middle"] = ["h0", kind, "h3"]
    CHAINS[f"{kind}_last"] = ["h2", "h3", kind]
CHAINS["same_child_twice"] = ["h0", "h0", "h2", "h0", "sr_absent", "sr_absent"]  # next to itself and apart
CHAINS["every_tipset_fails"] = list(FAIL_KINDS)
CHAINS["refused_4097"] = _cycle(SOUND, 4097)  # refusal only: never answered

_NAMES = ["flip", "steady", "late", "v5", "nobody"]
SPECS = {
    "n1": [("flip", 0)],
    "five_in_three_runs": C.runs([("flip", 2), ("late", 2), ("v5", 1)]),
    "one_run_4": C.runs([("steady", 4)]),                                   # T·n_specs = 256 at T = 64, R0 = 1
    "own_runs_4": [("flip", 0), ("late", 0), ("v5", 0), ("nobody", 0)],      # T·R0 = 256 at T = 64
    "one_actor_in_three_runs": C.runs([("flip", 2), ("steady", 3), ("flip", 1), ("nobody", 1), ("flip", 2)]),
    "successes": C.runs([("flip", 4), ("steady", 6), ("v5", 3)]),              # status 1 at every sound child
    "n63": C.runs([("steady", 30), ("flip", 4), ("late", 3), ("steady", 26)]),
    "n64": C.runs([("steady", 32), ("v5", 3), ("late", 3), ("flip", 26)]),
    "n65": [(_NAMES[i % 5], i // 5) for i in range(65)],                     # every spec its own run
    "n257": C.runs([("steady", 120), ("flip", 9), ("nobody", 2), ("late", 6), ("steady", 120)]),
}

CASES = (
    [(f"{kind}_{pos}", "five_in_three_runs") for kind in FAIL_KINDS for pos in ("first", "middle", "last")]
    + [("same_child_twice", "one_actor_in_three_runs"), ("every_tipset_fails", "five_in_three_runs")]
    + [("t1", "n1"), ("t1", "n257"), ("t2", "n257"), ("t3", "n65"), ("t4", "n63"), ("t4", "n64"), ("t4", "n65")]
    + [("t63", "one_run_4"), ("t64", "one_run_4"), ("t65", "one_run_4")]      # 252, 256, 260 claims
    + [("t63", "own_runs_4"), ("t64", "own_runs_4"), ("t65", "own_runs_4")]   # 252, 256, 260 runs
    + [("t64", "one_actor_in_three_runs"), ("t257", "n1"), ("t257", "five_in_three_runs"), ("t3", "n63"), ("t4", "successes")]
)


def epochs_of(chain):
    return np.arange(EPOCH0, EPOCH0 + len(chain), dtype=np.int64)


def expected_rows(dtype, chain_name, spec_name):
    """→ (rows of the whole chain in (tipset, spec) order, literal statuses, per-tipset answers)"""
    chain = CHAINS[chain_name]
    ids, slots = C.batch(SPECS[spec_name])
    rows, status, per = [], [], []
    for t, key in enumerate(chain):
        ans = C.answers(key, ids, slots)
        rows.append(sg.expected_rows(dtype, C.children[key], EPOCH0 + t, ids, slots, ans))
        status += [a[0] for a in ans]
        per.append(ans)
    return np.concatenate(rows), status, per
