"""One hand-built state tree under ONE child header for the storage generator (ipcfp_generate_storage_claims*), composed
from tests/storage_chain_cases.py's primitives and tests/pyhamt.py: a contract per layout and per way the chain can fail, so
that one batch holds runs of every kind side by side.

    TREE.store / TREE.child / TREE.contracts: name → (actor id, [(slot32, literal status)])

and what the tests of the generator share: batches over the tree, the two judges' answers per spec (cached: a spec's
answer is a function of (actor, slot)), and the expected rows under the rules of include/ipcfp.h "the storage generator
finished as column claims" built in numpy — the expected columns are ipcfp.compact_storage_claims of those rows.

The actors' HAMT decodes a node as a whole: one malformed ActorState fails every get that passes through its node.  So the
malformed actor lives in a child node of its own — four ids whose keys share the root's index CROWD — and every other
contract's id is chosen off that index."""
import hashlib

import numpy as np

import pyamt
import pyhamt
import pystorage
import pystorage_gen
import storage_chain_cases as sc
from pyamt import NULL, array, bstr, link, uint

EPOCH = 777_001  # `child.height` of the caller's ApiTipset: NOT the header's height (sc.EPOCH), and never compared with it
CROWD = 11       # the root index of the actors HAMT that the malformed actor and its three neighbours crowd into a child node


def _ids(crowded, count, start):
    out, n = [], start
    while len(out) < count:
        if (pyhamt.index_at(sc.actor_key(n), 0, 5) == CROWD) == crowded:
            out.append(n)
        n += 1
    return out


def _path_fork():
    """A layout-C root with two children: slot A's path is sound, slot B's passes a node with one malformed bucket (a text
    where a Vec<u8> belongs) that B itself does not sit in."""
    a, b = sc.slot_with_index(3), sc.slot_with_index(9)

    def root_block(st):
        good = st.put(sc.node(1 << pyhamt.index_at(a, 1, 5), [sc.bucket([(a, sc.vec(b"\x2a"))])]))
        j = pyhamt.index_at(b, 1, 5)
        k = (j + 1) % 32
        ptrs = sorted([(j, sc.bucket([(b, sc.vec(b"\x2b"))])), (k, sc.bucket([(sc.slot("bystander"), sc.text("x"))]))])
        bad = st.put(sc.node((1 << j) | (1 << k), [p for _, p in ptrs]))
        return sc.node((1 << 3) | (1 << 9), [link(good), link(bad)])
    return root_block, a, b


class Tree:
    def __init__(self):
        st = self.store = pyamt.Store()
        code, bytecode, info, receipts, messages = (pyamt.cid_of(n.encode()) for n in ("code", "bytecode", "info", "rcpt", "msgs"))
        self.contracts = {}
        actors = {}
        free = iter(_ids(False, 64, 2000))
        crowd = _ids(True, 4, 5000)

        def evm(root, v5=False, nonce=7):
            head = [link(bytecode), bstr(hashlib.sha256(b"bytecode").digest()), link(root)]
            return array(head + ([uint(nonce), NULL] if v5 else [NULL, uint(nonce), NULL]))

        def actor(aid, state, fields=None):
            f = [link(code), link(state), uint(aid % 997), bstr(b"\x00\x05"), NULL]
            actors[sc.actor_key(aid)] = fields(f) if fields else array(f)

        def contract(name, root_block, slots, aid=None, evm_block=None, actor_fields=None, drop_root=False, state=None):
            aid = next(free) if aid is None else aid
            if state is None:
                made = root_block(st)
                root_bytes = made[0] if type(made) is tuple else made
                root = st.put(root_bytes)
                if drop_root:
                    del st.blocks[root]
                state = st.put(evm_block(root) if evm_block else evm(root, nonce=aid % 1000))
            actor(aid, state, actor_fields)
            self.contracts[name] = (aid, slots)

        three = [(sc.S[2], 1), (sc.ABSENT, 1), (sc.S[1], 1)]  # present, absent, stored zeros
        for L in sc.LAYOUTS:
            contract(L.lower(), sc.layout(L, sc.PAIRS), three)
        many = [(k, 1) for k, _ in sc.MANY] + [(sc.slot(f"nobody{i}"), 1) for i in range(129)]  # 257 distinct slots, half absent
        contract("many5", sc.layout("B1", sc.MANY, 5), many)
        contract("many6", sc.layout("B2", sc.MANY, 6), many[40:90])
        contract("b1_width_0", sc.b1_lying(5, 0), [(sc.MANY[9][0], 66), (sc.ABSENT, 66)])
        contract("b1_width_9", sc.b1_lying(5, 9), [(sc.MANY[9][0], 66)])
        contract("b1_inner_absent", sc.b1_inner_absent(5, pairs=sc.NOWHERE), [(sc.S[0], 65), (sc.ABSENT, 65)])
        contract("root_absent", sc.layout("A3", [(sc.slot("gone"), b"\x01")]), [(sc.S[0], 65), (sc.S[1], 65)], drop_root=True)
        contract("evm_absent", None, [(sc.S[0], 65), (sc.S[2], 65)], state=pyamt.cid_of(b"an EVM state nobody stored"))
        contract("evm_malformed", None, [(sc.S[0], 66)], state=st.put(array([uint(1), uint(2)])))
        contract("evm_v5", sc.layout("A2", sc.PAIRS[:5]), [(sc.S[0], 1), (sc.S[4], 1), (sc.ABSENT, 1)], evm_block=lambda r: evm(r, v5=True))
        contract("actor_malformed", sc.layout("A3", sc.PAIRS[:2]), [(sc.S[0], 66)], aid=crowd[0], actor_fields=lambda f: array(f[:4]))
        for k in (1, 2, 3):  # sound values in the malformed one's node: the node fails as a whole
            contract(f"beside_malformed_{k}", sc.layout("A3", sc.PAIRS[:2]), [(sc.S[0], 66)], aid=crowd[k])
        self.contracts["actor_absent"] = (next(free), [(sc.S[0], 68), (sc.S[3], 68)])
        fork, a, b = _path_fork()
        contract("path_fork", fork, [(a, 1), (b, 66), (a, 1)])
        actors_root = pyhamt.build_hamt(st, actors)
        sroot = st.put(array([uint(5), link(actors_root), link(info)]))
        parent = pyamt.cid_of(b"parent header")
        self.child = st.put(array([bstr(b"\x00\xe8\x07"), array([bstr(b"vrf")]), NULL, array([]), array([]), array([link(parent)]),
                                   bstr(b"\x00\x01"), uint(sc.EPOCH), link(sroot), link(receipts), link(messages), NULL,
                                   uint(1_700_000_000), NULL, uint(0), bstr(b"\x00\x64")]))
        self.cids = list(st.blocks)
        self._py, self._orc = {}, {}

    # ---- batches: [(contract name, k-th slot of it)] → (actor ids u64[n], slots u8[n, 32], literal statuses) ----
    def batch(self, picks):
        ids = np.array([self.contracts[c][0] for c, _ in picks], dtype=np.uint64)
        slots = np.zeros((len(picks), 32), dtype=np.uint8)
        lit = []
        for i, (c, k) in enumerate(picks):
            s, st = self.contracts[c][1][k % len(self.contracts[c][1])]
            slots[i] = np.frombuffer(s, dtype=np.uint8)
            lit.append(st)
        return ids, slots, lit

    def runs(self, shape):
        """[(contract, run length)] → picks: a run walks its contract's slots in order"""
        return [(c, k) for c, n in shape for k in range(n)]

    def successes(self):
        return [c for c, (_, slots) in self.contracts.items() if all(st == 1 for _, st in slots)]

    # ---- the judges, per distinct spec ----
    def py(self, aid, slot):
        key = (int(aid), bytes(slot))
        if key not in self._py:
            self._py[key] = pystorage_gen.generate(self.store.blocks, self.child, key[0], key[1])
        return self._py[key]

    def oracle(self, ost, aid, slot):
        key = (int(aid), bytes(slot))
        if key not in self._orc:
            st, out3, val, wit = ost.generate_storage_proof(self.child, key[0], key[1])
            self._orc[key] = (st, out3.copy(), val.copy(), [pystorage_gen.cid_of_slot(w) for w in wit])
        return self._orc[key]


def slot40(cid: bytes) -> np.ndarray:
    out = np.zeros(40, dtype=np.uint8)
    out[: len(cid)] = np.frombuffer(cid, dtype=np.uint8)
    return out


def expected_rows(dtype, child: bytes, epoch: int, ids, slots, answers):
    """The rows a generated batch must compact to.  answers[i] = pystorage_gen.generate(..)'s (status, fields, recorded) of
    spec i.  status 1: every field and flags 63; a failure behind contract_state: the CIDs, flags 15, value zero; a failure
    before it: the three derived CID slots zero and flags 0."""
    rows = np.zeros(len(ids), dtype=dtype)
    rows["child_epoch"] = epoch
    rows["actor_id"] = ids
    rows["child"][:] = slot40(child)
    rows["slot"] = slots
    for i, (st, out, _) in enumerate(answers):
        if "storage_root" not in out:
            continue
        rows["state_root"][i] = slot40(out["parent_state_root"])
        rows["actor_state"][i] = slot40(out["actor_state_cid"])
        rows["storage_root"][i] = slot40(out["storage_root"])
        rows["flags"][i] = 15
        if st == 1:
            rows["value"][i] = np.frombuffer(out["value"], dtype=np.uint8)
            rows["flags"][i] = 63
    return rows


def union_ord(cid_lists):
    return sorted(set(c for l in cid_lists for c in l), key=pystorage_gen.cid_ord)


TREE = Tree()
