"""Call sequences over resident witnesses: the model, the generator and the two executors.

A real caller keeps one context and a few witnesses resident and issues many different calls on them; a call's answer must
be a function of its arguments and of the witness's blocks, never of the calls before it.  This module states that:

  * an OP is a plain tuple `(kind, witness, args)` of a string, "A" / "B" / "C" and a tuple of small integers, so that a
    sequence is a literal which `replay(ops)` accepts;
  * the MODEL holds, per witness, what the ABI says the witness holds — its blocks in id order (`put_keyed` appends, the
    last block of a CID wins), its receipt range — and per context the tuning words; `Model.apply(op)` is the state change
    of an op and `Model.expect(op)` its answer, from a FRESH oracle store of the witness's current blocks (witnesses A and
    B, synthetic tipsets) or from tests/pyevents.py (witness C, hand-built: two tipset pairs in one witness).  The engine
    is never asked.  Answers are memoised by (witness, block version, receipt range, op);
  * `sequence(seed)` is, per witness, an Eulerian circuit of the complete directed graph (self-loops included) over the op
    kinds of that witness — every ordered pair (X then Y on the same witness) exactly once — with arguments drawn from the
    seed, the three circuits interleaved by a seeded shuffle that keeps each circuit's order, then EXTENDED until the
    coverage conditions of `coverage_gaps` hold (tests/test_call_sequences.py asserts them);
  * `LongLived` runs a sequence through ONE oracle store per witness, rebuilt only where the blocks change (the reference
    held to its own statelessness), and `Runner` runs it through the engine (tests/test_gpu_call_sequences.py).

A receipt range stays on a witness for the scan and every form of the event verifier — their answer is the full answer cut
to the range, the claims routed to it as a host routes them (tests/test_gpu_receipt_leaves_groups.py) — and for the ops
that never read it, whose answers may not move with it; a burst's parts run under the ranges their witnesses have.  The
generator and two failing event calls have it lifted first (`Model.lifts`), which is itself a state change the next call has to survive."""
import hashlib
import re

import numpy as np

import claims as claims_mod
import event_chain_cases as ec
import ipc_filecoin_proofs_amd as ipcfp
import oracle_lib
import pyevents
import pystorage
from conftest import fuzz_seed
from test_gpu_event_table import packed
from tools.synth import Tipset

FULL = (0, (1 << 64) - 1)
CHUNK = 100
BASE_SEED = 7300
ERR_BAD_CLAIM, ERR_MISSING = 69, 65
STD = bytes.fromhex("0171a0e40220")
ABSENT_ROOT = STD + hashlib.blake2b(b"a receipts root no witness holds", digest_size=32).digest()
NO_FILTER = (b"\x5a" * 32, b"\xa5" * 32)  # matches nothing
TUNING = (("fast_verify", (-1, 0, 1)), ("hamt_levels", (-1, 0, 2, 14)), ("hamt_table", (-1, 0, 1)), ("hamt_coop", (-1, 0)))

VERIFY_KINDS = ("verify_event_claims", "verify_event_proofs", "verify_event_claims_compact", "verify_event_proofs_located",
                "verify_and_scan_device", "verify_storage_proofs", "verify_storage_columns")
QUERY_KINDS = ("verify_cids", "scan_events") + VERIFY_KINDS + ("exec_order", "generate_event_proofs", "amt_get", "hamt_get",
                                                               "generate_storage_claims", "has_get")
STATE_KINDS = ("rebuild_index", "put_fresh", "put_replace", "set_receipt_range", "close_and_recreate", "set_tuning")
# (short_scan_cap: the ABI reports a has-match buffer that is too small through *n_receipts > cap_receipts, not through a
#  return code; the "code" of that op is the overflow, and nothing may be written behind the buffer's end)
FAILING_KINDS = ("bad_run_table", "bad_bundle_block_id", "short_scan_cap", "bad_compact_group")
SYNTH_KINDS = QUERY_KINDS + STATE_KINDS + FAILING_KINDS + ("burst",)
HAND_KINDS = ("verify_cids", "scan_events", "verify_event_claims", "verify_event_proofs", "verify_event_claims_compact",
              "verify_event_proofs_located", "verify_and_scan_device", "exec_order", "generate_event_proofs", "amt_get", "has_get",
              "rebuild_index", "put_fresh", "put_replace", "close_and_recreate", "set_tuning", "bad_bundle_block_id",
              "short_scan_cap", "bad_compact_group")
KINDS = {"A": SYNTH_KINDS, "B": SYNTH_KINDS, "C": HAND_KINDS}
# ops whose answer under a receipt range is the full answer cut to the range (ipcfp.h: the scan walks only those receipts,
# every ipcfp_verify_event_* form resolves them by table) …
CUT_BY_RANGE = ("scan_events", "verify_event_claims", "verify_event_claims_compact", "verify_event_proofs",
                "verify_event_proofs_located", "verify_and_scan_device")
# … and the ops a range stays on for: those, and the ones that never read it — whose answers therefore may not move with it.
# A burst keeps it too: its parts are of both sorts.  The others (the generator, the two failing event calls) have the
# range lifted in front of them.
RANGED = CUT_BY_RANGE + ("verify_cids", "exec_order", "amt_get", "hamt_get", "verify_storage_proofs", "verify_storage_columns",
                         "generate_storage_claims", "has_get", "rebuild_index", "put_fresh", "put_replace", "close_and_recreate",
                         "set_receipt_range", "set_tuning", "bad_run_table", "bad_bundle_block_id", "burst")
BLOCK_CHANGING = ("put_fresh", "put_replace")
AFTER = ("rebuild_index", "put_replace", "set_receipt_range", "close_and_recreate")  # every kind directly follows each


def idaddr(i):
    b = bytearray([0])
    while True:
        c = i & 0x7F
        i >>= 7
        if i:
            b.append(c | 0x80)
        else:
            b.append(c)
            return bytes(b)


def slot40(cid: bytes) -> bytes:
    return bytes(cid).ljust(40, b"\0")


def tables_of(cids, blks):
    lens = np.fromiter((len(b) for b in blks), dtype=np.uint32, count=len(blks))
    off = np.zeros(len(blks), dtype=np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = np.frombuffer(b"".join(blks), dtype=np.uint8).copy()
    c40 = np.frombuffer(b"".join(slot40(c) for c in cids), dtype=np.uint8).reshape(-1, 40).copy()
    return data, off, lens, c40


def trust_of(which, parent_epoch, child_epoch):
    """0: none · 1: a window both epochs lie in · 2: a window that ends before the child epoch"""
    if which == 0:
        return None
    hi = child_epoch if which == 1 else parent_epoch
    return claims_mod.TrustPolicy(kind=1, ec_chain_empty=0, min_epoch=parent_epoch, max_epoch=hi)


def events_root_of_receipt(receipt: bytes):
    """the events root a receipt's bytes link to, or None (`[exit_code, return, gas_used, events_root | null]`)"""
    at = receipt.rfind(b"\xd8\x2a\x58\x27\x00" + STD)
    return None if at < 0 else receipt[at + 5: at + 5 + 38]


# ---- the three witnesses ------------------------------------------------------------------------------------------------------
class Synth:
    """What the ops need of one synthetic tipset, computed once; nothing here changes afterwards."""

    hand = False

    def __init__(self, tip):
        self.tip = tip
        self.cids = [tip.cids[i, :38].tobytes() for i in range(tip.n_blocks)]
        self.blks = [tip.block(i) for i in range(tip.n_blocks)]
        self.ts, self.cl, self.blob, self.blob_len = packed(tip)
        self.cl_u32 = self.cl.copy()  # the transport form carries 32-bit indices: the lie "2^64-1" becomes "2^32-1"
        self.cl_u32["event_index"] = np.minimum(self.cl_u32["event_index"], np.uint64(0xFFFFFFFF))
        pairs = {}
        for i in range(len(tip.claim_exec)):
            if tip.claim_ntopics[i] >= 2:
                k = (tip.claim_topics[i, 0].tobytes(), tip.claim_topics[i, 1].tobytes())
                pairs[k] = pairs.get(k, 0) + 1
        own = (tip.topic0, tip.topic1)
        other = max((k for k in sorted(pairs) if k != own), key=lambda k: pairs[k])
        self.filters = (own, other, NO_FILTER)
        self.actors = (None, tip.filter_actor, 7)  # (7: below emitter_base, no event's emitter)
        self.roots = (tip.receipts_root, tip.receipts_root, ABSENT_ROOT)
        self.parents = (list(tip.parent_cids), list(tip.parent_cids)[::-1])
        self.n_receipts = int(tip.params["n_receipts"])
        # string claims: every fifth claim of the tipset's table, a third of them lying
        self.str_idx = np.arange(0, len(tip.claim_exec), 5)
        self._str = {}
        self.str_claims = self.string_claims(FULL)[1]
        # storage claims: a batch under and a batch over the n·16 >= blocks switch to the tabled route (the witness grows by
        # at most a few hundred blocks over a sequence: the margins below hold throughout)
        ns = len(tip.sc_actor)
        small = np.arange(min(ns, 40))
        large = np.resize(np.arange(ns), max(ns, tip.n_blocks // 16 + 64))
        assert len(small) * 16 < tip.n_blocks and len(large) * 16 >= tip.n_blocks + 640
        self.sc = [self._storage_strings(idx) for idx in (small, large)]
        self.scl = [self._storage_packed(idx) for idx in (small, large)]
        keys = [idaddr(int(i)) for i in tip.query_ids]
        keys[5] = b"\x00"       # an id address no actor has
        keys[6] = b"\xff" * 9   # no address at all
        self.keys = (keys[:20], keys, keys[:1024])  # (1024: the smallest batch the default tuning answers level by level)
        assert len(keys) >= 1024, "the default tuning must take the level path"
        # the events roots a replacement exchanges: those of the planted receipts
        ost = oracle_lib.load().store(*tables_of(self.cids, self.blks))
        _, vals = ost.amt_get(tip.receipts_root, 0, "receipt", tip.planted, cap=2048)
        ost.close()
        look = dict(zip(self.cids, self.blks))
        roots = [events_root_of_receipt(v) for v in vals]
        self.event_roots = [(r, look[r]) for r in dict.fromkeys(r for r in roots if r is not None)]
        assert len(self.event_roots) >= 4 and len({b for _, b in self.event_roots}) >= 4
        self.planted = [int(p) for p in tip.planted]
        # … and the storage side's: the contracts' actor-state blocks (a claim's storage root then is another contract's)
        states = [bytes(c[:38]) for c in tip.sc_actor_state]
        self.actor_states = [(c, look[c]) for c in dict.fromkeys(states)]
        assert len(self.actor_states) >= 4 and len({b for _, b in self.actor_states}) >= 4

    def string_claims(self, rng):
        """→ (positions, claims): the string claims whose CLAIMED exec_index lies in the receipt range, and their positions
        in the whole batch (what a host routes to the shard of that range)"""
        if rng not in self._str:
            if rng == FULL:
                ks = np.arange(len(self.str_idx))
            else:
                full = self.string_claims(FULL)[1]
                ks = np.array([k for k in range(full.n) if rng[0] <= full.arr[k].exec_index < rng[1]], dtype=np.int64)
            tip = self.tip
            ecl = claims_mod.EventClaims(tip, indices=self.str_idx[ks])
            for j, k in enumerate(ks):
                lie = int(k) % 12
                if lie == 1:
                    ecl.arr[j].event_index += 1
                elif lie == 2:
                    ecl.arr[j].emitter += 1
                elif lie == 3:
                    ecl.set_str(j, "data", "0x00")
                elif lie == 4:
                    ecl.arr[j].exec_index += 1
                elif lie == 5:
                    ecl.set_str(j, "message_cid", claims_mod.cid_str(tip.child_cid))
                elif lie == 6:
                    ecl.arr[j].parent_epoch -= 1
                elif lie == 7:
                    ecl.arr[j].event_index = 64
            self._str[rng] = (ks, ecl)
        return self._str[rng]

    def _storage_strings(self, idx):
        """tests/test_gpu_context_fallbacks.py::storage_claims over the claims `idx`: a wrong value, a value no padded word
        can equal, a wrong storage root"""
        sc = claims_mod.StorageClaims(self.tip, indices=idx)
        for k in range(3, sc.n, 17):
            if k % 3 == 0:
                sc.set_str(k, "value", "0x" + "ee" * 32)
            elif k % 3 == 1:
                sc.set_str(k, "value", "0x1234")
            else:
                sc.set_str(k, "storage_root", claims_mod.cid_str(self.tip.child_cid))
        for k in range(5, sc.n, 17):  # … and: an actor nobody is, another actor's state, a state root and a child that are none
            if k % 4 == 0:
                sc.arr[k].actor_id += 10 ** 9
            elif k % 4 == 1:
                sc.set_str(k, "actor_state_cid", claims_mod.cid_str(self.tip.child_cid))
            elif k % 4 == 2:
                sc.set_str(k, "parent_state_root", claims_mod.cid_str(self.tip.receipts_root))
            else:
                sc.set_str(k, "child_block_cid", claims_mod.cid_str(self.tip.parent_cids[0]))
        return sc

    def _storage_packed(self, idx):
        T = self.tip
        cl = ipcfp.pack_storage_claims(T.child_cid, T.state_root, T.child_epoch, T.sc_actor[idx], T.sc_actor_state[idx],
                                       T.sc_storage_root[idx], T.sc_slot[idx], T.sc_value[idx])
        n = len(cl)
        cl["value"][np.arange(3, n, 7), 31] ^= 1             # wrong values
        cl["actor_id"][np.arange(5, n, 19)] += 10 ** 9       # actors that do not exist
        cl["storage_root"][np.arange(11, n, 23), 10] ^= 4    # a storage root nobody has
        cl["actor_state"][np.arange(13, n, 29), 12] ^= 8     # an actor state nobody has
        cl["state_root"][np.arange(2, n, 31)] = np.frombuffer(slot40(T.receipts_root), dtype=np.uint8)  # no state root
        cl["child"][np.arange(9, n, 37)] = np.frombuffer(slot40(T.parent_cids[0]), dtype=np.uint8)      # another header
        return cl

    def gen_specs(self, salt):
        """(actor ids, slots) of a generate_storage_claims batch: 24 of the tipset's own pairs, an actor nobody is and a
        slot nobody wrote"""
        T = self.tip
        idx = (np.arange(24) * 5 + salt) % len(T.sc_actor)
        ids = T.sc_actor[idx].copy()
        slots = T.sc_slot[idx].copy()
        ids[7] += 10 ** 9
        slots[13, 5] ^= 0x40
        return ids, slots


class Hand:
    """Two hand-built tipset pairs in one witness (tests/test_gpu_event_chain.py merges them the same way)."""

    hand = True

    def __init__(self):
        a_store, a_claim, a_parts = ec.tipset(salt=1)
        b_store, b_claim, b_parts = ec.second_tipset()
        blocks = {**a_store.blocks, **b_store.blocks}
        self.cids, self.blks = list(blocks), list(blocks.values())
        self.parts = (a_parts, b_parts)
        a = [dict(a_claim), {**a_claim, "emitter": 7}, {**a_claim, "exec_index": 3}, {**a_claim, "event_index": 9},
             {**a_claim, "message_cid": b_claim["message_cid"]}, {**a_claim, "child_block_cid": b_claim["child_block_cid"]},
             {**a_claim, "data": "0x"}]
        b = [dict(b_claim), {**b_claim, "emitter": 7}, {**b_claim, "parent_epoch": ec.PARENT_EPOCH}, {**b_claim, "topics": b_claim["topics"][:1]},
             {**b_claim, "parent_tipset_cids": a_claim["parent_tipset_cids"]}, {**b_claim, "message_cid": a_claim["message_cid"]},
             {**b_claim, "event_index": 1}]
        self.claims = [c for pair in zip(a, b) for c in pair] * 3
        self.proofs = ec.proofs(self.claims)
        self.ts, self.cl, self.blob = ipcfp.pack_event_proofs(self.proofs.arr, self.proofs.n)
        self.blob_len = len(self.blob)
        self.filters = (ec.FILTER, ec.OTHER_FILTER, NO_FILTER)
        self.actors = (None, 1001, 4000)
        self.roots = (a_parts["receipts"], b_parts["receipts"], ABSENT_ROOT)
        self.parents = (a_parts["parents"], b_parts["parents"])
        self.children = (a_parts["child"], b_parts["child"])
        self.trusts = (None, (0, ec.PARENT_EPOCH, ec.CHILD_EPOCH + 10), (0, ec.PARENT_EPOCH, ec.PARENT_EPOCH + 10))
        roots = [r for _i, r in pyevents.amt_for_each(pyevents.amt_load(blocks, a_parts["receipts"], 0, pyevents.check_receipt)) if r is not None]
        self.event_roots = [(r, blocks[r]) for r in dict.fromkeys(roots)]
        assert len(self.event_roots) >= 4


def witnesses(seed):
    """{name: Synth | Hand} of a seed (A and B move with it; C is hand-built)"""
    if seed not in _WITNESSES:
        common = dict(n_parents=3, dup_permille=30, n_planted=10, variety=1, max_events=5, no_events_permille=80, n_contracts=8,
                      slots_per_contract=12, storage_layout_mix=1, n_actor_queries=1200)
        a = Tipset(n_receipts=1500, n_actors=3000, seed=seed + 1, **common)
        b = Tipset(n_receipts=2300, n_actors=4000, events_bit_width=6, seed=seed + 2, **common)
        assert b.n_blocks > a.n_blocks + 700  # (B stays the larger one whatever a sequence puts into A)
        _WITNESSES.clear()
        _WITNESSES[seed] = {"A": Synth(a), "B": Synth(b), "C": Hand()}
    return _WITNESSES[seed]


_WITNESSES = {}


class WState:
    """What the ABI says one witness holds."""

    def __init__(self, base):
        self.base = base
        self.cids, self.blks = list(base.cids), list(base.blks)
        self.version = 0
        self.range = FULL
        self._tables = None

    def tables(self):
        if self._tables is None or self._tables[0] != self.version:
            self._tables = (self.version, tables_of(self.cids, self.blks))
        return self._tables[1]

    def lookup(self):
        return dict(zip(self.cids, self.blks))  # the last block of a CID wins

    def put(self, cid, blk):
        self.cids.append(cid)
        self.blks.append(blk)
        self.version += 1


# ---- ops: their arguments ---------------------------------------------------------------------------------------------------------
def arg_space(kind, wit):
    """Every argument tuple an op of `kind` on `wit` is given, or None where the argument is a salt.  An op kind occurs at
    least as often as its witness has kinds (its row of the circuit), so a sequence walks each of these lists to its end."""
    three = [(x, y) for x in range(3) for y in range(3)]
    if kind == "scan_events":  # (filter, actor, want_touched, root): root 1 is C's second tipset, root 2 is in no witness
        roots = 2 if wit == "C" else 1
        return ([(f, a, (f + a) & 1, (f + a) % roots) for f, a in three] + [(0, 0, 1, 0), (1, 0, 1, 0), (0, 0, 0, 2), (1, 1, 1, 2)] +
                ([(0, 0, 1, 1), (1, 0, 0, 1)] if wit == "C" else []))
    if kind in ("verify_event_claims", "verify_event_proofs", "verify_event_claims_compact", "verify_event_proofs_located"):
        return three  # (filter, trust)
    if kind == "verify_and_scan_device":
        return [(f, t, (f + t) % 3, (f + 2 * t) % 3) for f, t in three]
    if kind in ("exec_order", "verify_storage_proofs", "verify_storage_columns"):
        return [(0,), (1,)]
    if kind == "generate_event_proofs":
        return [(f, a, (f + a) & 1) for f, a in three]
    if kind == "hamt_get":  # (value kind, bit width, 20 keys | all of them)
        return [(k, bw, n) for k in range(3) for bw in range(3) for n in range(2)]
    if kind == "set_receipt_range":
        return [(1,), (2,), (3,)]  # (never the full range: that is what a lift sets)
    if kind == "set_tuning":
        return [(k, v) for k, (_, values) in enumerate(TUNING) for v in range(len(values))]
    if kind == "burst":
        return [(1,), (2,), (3,)]
    if kind == "generate_storage_claims":
        return [(0,), (1,), (2,), (3,), (5,)]
    if kind in ("amt_get", "has_get", "put_fresh", "put_replace"):
        return None
    return [()]


def burst_parts(op):
    """the device entry points a burst queues, as ops: (kind, witness, args)"""
    _, wit, (variant,) = op
    other = "B" if wit == "A" else "A"
    if variant == 0:  # the smaller batch on the smaller witness, then the larger on the larger, both level by level under the
        # default tuning: the context's node tables (sized by block count) grow while the first call is still queued
        return [("hamt_get", "A", (0, 0, 2)), ("hamt_get", "B", (0, 0, 1))]
    if variant == 1:
        return [("verify_event_claims", wit, (1, 0)), ("scan_events", other, (0, 0, 0, 0)), ("hamt_get", wit, (0, 0, 0))]
    if variant == 2:
        return [("verify_and_scan_device", wit, (0, 0, 0, 1)), ("verify_storage_columns", other, (1,)),
                ("generate_storage_claims", wit, (3,)), ("hamt_get", other, (0, 0, 1))]
    return [("scan_events", wit, (1, 1, 0, 0)), ("generate_storage_claims", other, (5,))]


HAMT_TABLE_KINDS = ("actor_state", "vec_u8", "any")  # the value kinds the node table knows (kernels/walk.hip hamt_kind_bit)


def hamt_route(tuning, n_keys, n_blocks, bit_width=5, value_kind="actor_state"):
    """which route a HAMT batch takes (host/primitives.cpp hamt_get_batch): "table" and "levels" use the context's node
    tables (hamt_recs; levels also hamt_scratch and hamt_etabs), sized by the witness's block count; "walker" uses none"""
    if tuning["hamt_table"] == 1 and value_kind in HAMT_TABLE_KINDS:
        return "table"
    levels = tuning["hamt_levels"]
    if levels != 0 and 1 <= bit_width <= 8 and n_blocks > 0 and (n_keys >= 1024 or levels > 0):
        return "levels"
    return "walker"


def witnesses_of(op):
    return sorted({p[1] for p in burst_parts(op)}) if op[0] == "burst" else [op[1]]


def receipt_range(base, which):
    n = base.n_receipts
    return (FULL, (3, n - 5), (n // 3 + 1, 2 * n // 3 + 2), (n // 2 + 3, n))[which]  # (0, FULL: what a lift sets)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
class Model:
    def __init__(self, seed=None):
        self.seed = fuzz_seed(BASE_SEED) if seed is None else seed
        self.base = witnesses(self.seed)
        self.orc = oracle_lib.load()
        self.memo = {}
        self.reset()

    def reset(self):
        self.w = {k: WState(b) for k, b in self.base.items()}
        self.tuning = {k: -1 for k, _ in TUNING}

    # -- state --
    def lifts(self, op):
        """witnesses whose receipt range has to be lifted in front of `op` (and lifts it in the model)"""
        if op[0] in RANGED:
            return []
        out = [w for w in witnesses_of(op) if self.w[w].range != FULL]
        for w in out:
            self.w[w].range = FULL
        return out

    def new_block(self, op):
        """(cid, bytes) that a put op writes"""
        kind, wit, (salt,) = op
        ws = self.w[wit]
        if kind == "put_fresh":
            g = np.random.default_rng([self.seed, salt, len(ws.cids)])
            blk = bytes([0x58, 200]) + g.integers(0, 256, 200, dtype=np.uint8).tobytes()  # a CBOR byte string nothing links to
            return STD + hashlib.blake2b(blk, digest_size=32).digest(), blk
        # put_replace: an events root — or, on the synthetic witnesses, every other time a contract's actor state — takes its
        # neighbour's bytes, or its own again
        roots = ws.base.event_roots if ws.base.hand or salt & 2 == 0 else ws.base.actor_states
        k = (salt >> 2) % len(roots)
        return roots[k][0], (roots[(k + 1) % len(roots)][1] if salt & 1 == 0 else roots[k][1])

    def apply(self, op):
        kind, wit, args = op
        if kind in BLOCK_CHANGING:
            self.w[wit].put(*self.new_block(op))
        elif kind == "set_receipt_range":
            self.w[wit].range = receipt_range(self.base[wit], args[0])
        elif kind == "set_tuning":
            self.tuning[TUNING[args[0]][0]] = TUNING[args[0]][1][args[1]]

    # -- answers --
    def key(self, op):
        kind, wit, args = op
        if kind == "burst":
            return ("burst",) + tuple(self.key(p) for p in burst_parts(op))
        ws = self.w[wit]
        return (wit, ws.version, ws.range if kind in CUT_BY_RANGE else FULL, kind, args)

    def expect(self, op):
        """the answer of `op` in the model's present state, from a fresh store"""
        k = self.key(op)
        if k not in self.memo:
            if op[0] == "burst":
                self.memo[k] = tuple(self.expect(p) for p in burst_parts(op))
            elif answer_model(self.w[op[1]], op) is not NotImplemented:
                self.memo[k] = answer_model(self.w[op[1]], op)
            elif self.base[op[1]].hand:
                self.memo[k] = answer_hand(self.w[op[1]], op)
            else:
                ws = self.w[op[1]]
                store = self.orc.store(*ws.tables())
                try:
                    self.memo[k] = answer_oracle(self.orc, store, ws, op)
                finally:
                    store.close()
        return self.memo[k]


def cut(scan, rng):
    """the oracle's scan answer cut to a receipt range, as tests/test_gpu_receipt_leaves_groups.py cuts it"""
    st, has, trip, touched = scan
    if st != 1:
        return (st,)
    if rng == FULL:
        return (1, bytes(has), tuple(trip), touched)
    lo, hi = rng
    return (1, bytes(has[lo:hi]), tuple(t for t in trip if lo <= t[0] < hi), None)


def in_range(exec_index, rng):
    return np.nonzero((exec_index >= np.uint64(rng[0])) & (exec_index < np.uint64(min(rng[1], (1 << 63)))))[0] if rng != FULL else np.arange(len(exec_index))


def has_get_picks(ws, salt):
    n = len(ws.cids)
    return [ws.cids[(salt * 7 + 1) % n], ws.cids[(salt * 13 + 5) % n], ws.cids[n - 1], ws.base.event_roots[salt % len(ws.base.event_roots)][0],
            STD + hashlib.blake2b(b"absent %d" % salt, digest_size=32).digest()]


def answer_model(ws, op):
    """answers that are a function of the model's blocks alone (no tree is walked)"""
    kind, _wit, args = op
    if kind == "has_get":
        look = ws.lookup()
        return tuple(look.get(c) for c in has_get_picks(ws, args[0]))
    if kind in STATE_KINDS:
        if kind in BLOCK_CHANGING:
            return ("blocks", len(ws.cids) + 1)
        return ("blocks", len(ws.cids)) if kind == "close_and_recreate" else None
    if kind == "bad_bundle_block_id":
        return ("rc", -1)
    return NotImplemented


def bad_group(ws):
    return min(11, len(ws.base.cl) - 1)


def amt_query(ws, args):
    """(root, version, value kind, indices) of an amt_get op"""
    which, salt = args
    b = ws.base
    n = b.n_receipts if not b.hand else 6
    if which == 1:
        return b.event_roots[salt % len(b.event_roots)][0], 3, "stamped_event", [0, 1, 2, 5, 31, 63, 64, 1 << 40]
    own = [p for p in (b.planted if not b.hand else [2, 1])] + [0, salt % n, n - 1, n, 5000, 1 << 40]
    return b.roots[0], (0 if which == 0 else 3), "receipt", own


def answer_oracle(orc, store, ws, op, held=False):
    kind, _wit, args = op
    b, T = ws.base, ws.base.tip
    got = answer_model(ws, op)
    if got is not NotImplemented:
        return got
    if kind == "verify_cids":
        data, off, lens, c40 = ws.tables()
        ok, good = orc.blake2b256_verify(data, off, lens, c40[:, 6:38])
        return (ok.tobytes(), len(ok) - good)
    if kind in ("scan_events", "short_scan_cap"):
        f, a, touched, root = args if kind == "scan_events" else (0, 0, 0, 0)
        s = store.scan_events(b.roots[root], *b.filters[f], actor=b.actors[a], want_touched=bool(touched), threads=1)
        s = (s[0], s[1], [tuple(int(x) for x in t) for t in s[2]], frozenset(bytes(c) for c in s[3]) if touched else None)
        if kind == "short_scan_cap":
            return ("overflow", int(len(s[1]) > SHORT_CAP), bytes(s[1][:SHORT_CAP]), len(s[1]), len(s[2]))
        return cut(s, ws.range)
    if kind in ("verify_event_claims", "verify_event_claims_compact", "bad_compact_group"):
        f, t = args if args else (0, 0)
        cl = b.cl if kind == "verify_event_claims" else b.cl_u32
        st = store.verify_event_claims_packed(b.ts, cl, b.blob, trust=trust_of(t, T.parent_epoch, T.child_epoch),
                                              filt=claims_mod.make_filter(*b.filters[f - 1]) if f else None, threads=1)
        assert (st != 255).all()
        if kind == "bad_compact_group":
            st[bad_group(ws)] = ERR_BAD_CLAIM
        return st[in_range(cl["exec_index"], ws.range)].tobytes()
    if kind in ("verify_event_proofs", "verify_event_proofs_located"):
        f, t = args
        pr = b.str_claims
        st = store.verify_event_proofs(pr, trust=trust_of(t, T.parent_epoch, T.child_epoch),
                                       filt=claims_mod.make_filter(*b.filters[f - 1]) if f else None, mode=2 if held else 1, threads=1)
        ks = b.string_claims(ws.range)[0]  # the full batch's answer, cut to the claims of the range
        if kind == "verify_event_proofs":
            return st[ks].tobytes()
        ev = []
        for i in (int(k) for k in ks):  # the StampedEvent the verifier compared: the one at the CLAIMED indices
            one = None
            if st[i] == 1 or 12 <= st[i] <= 17:
                _, rv = store.amt_get(T.receipts_root, 0, "receipt", [int(pr.arr[i].exec_index)], cap=2048)
                _, evs = store.amt_get(events_root_of_receipt(rv[0]), 3, "stamped_event", [int(pr.arr[i].event_index)], cap=2048)
                one = evs[0]
            ev.append(one)
        return (st[ks].tobytes(), tuple(ev))
    if kind == "verify_and_scan_device":
        f, t, sf, sa = args
        v = answer_oracle(orc, store, ws, ("verify_event_claims", op[1], (f, t)), held)
        return (v, answer_oracle(orc, store, ws, ("scan_events", op[1], (sf, sa, 0, 0)), held))
    if kind == "exec_order":
        st, out = store.exec_order(b.parents[args[0]])
        return (st, out.tobytes()) if st == 1 else (st,)
    if kind == "generate_event_proofs":
        f, a, _ = args
        st, trip, msg, wit = store.generate_event_proof(T.parent_cids, T.child_cid, *b.filters[f], actor=b.actors[a])
        return (st, tuple(tuple(int(x) for x in t) for t in trip), msg.tobytes(), tuple(bytes(c) for c in wit)) if st == 1 else (st,)
    if kind == "amt_get":
        root, version, vkind, idx = amt_query(ws, args)
        st, vals = store.amt_get(root, version, vkind, idx, cap=2048)
        return (st.tobytes(), tuple(v for s, v in zip(st, vals) if s == 1))
    if kind == "hamt_get":
        vk, bw, batch = args
        st, vals = store.hamt_get(T.actors_root, (5, 4, 8)[bw], ("actor_state", "any", "vec_u8")[vk], b.keys[batch], cap=2048, threads=1)
        return (st.tobytes(), tuple(vals[i] for i in np.nonzero(st == 1)[0][:16]))
    if kind == "verify_storage_proofs":
        return store.verify_storage_proofs(b.sc[args[0]], mode=1, threads=1).tobytes()
    if kind == "verify_storage_columns":
        return store.verify_storage_claims_packed(b.scl[args[0]], threads=1).tobytes()
    if kind == "bad_run_table":
        return ("rc", -1)
    if kind == "generate_storage_claims":
        ids, slots = b.gen_specs(args[0])
        st, rows = [], []
        for aid, slot in zip(ids, slots):
            s, out3, val, _wit = store.generate_storage_proof(T.child_cid, int(aid), slot.tobytes())
            st.append(s)
            rows.append((out3.tobytes(), val.tobytes()) if s == 1 else None)
        return (bytes(st), tuple(rows))
    raise KeyError(kind)


SHORT_CAP = 16  # (bytes; C's receipts trees are shorter: the op then fits and its code is 0 — it is no failing op there)


def answer_hand(ws, op):
    kind, _wit, args = op
    b = ws.base
    got = answer_model(ws, op)
    if got is not NotImplemented:
        return got
    blocks = ws.lookup()
    if kind == "verify_cids":
        ok = bytes(int(c == STD + hashlib.blake2b(x, digest_size=32).digest()) for c, x in zip(ws.cids, ws.blks))
        return (ok, ok.count(0))
    if kind in ("scan_events", "short_scan_cap"):
        f, a, touched, root = args if kind == "scan_events" else (0, 0, 0, 0)
        st, has, trip, rec = pyevents.scan(blocks, b.roots[root], *b.filters[f], b.actors[a])
        if kind == "short_scan_cap":
            return ("overflow", int(len(has) > SHORT_CAP), bytes(has[:SHORT_CAP]), len(has), len(trip))
        return (1, bytes(has), tuple(trip), frozenset(slot40(c) for c in rec) if touched else None) if st == 1 else (st,)
    if kind in ("verify_event_claims", "verify_event_proofs", "verify_event_claims_compact", "bad_compact_group", "verify_event_proofs_located"):
        f, t = args if args else (0, 0)
        st = [pyevents.verify(blocks, c, b.trusts[t], b.filters[f - 1] if f else None) for c in b.claims]
        if kind == "bad_compact_group":
            st[bad_group(ws)] = ERR_BAD_CLAIM
        if kind != "verify_event_proofs_located":
            return bytes(st)
        ev = []
        for s, c in zip(st, b.claims):
            ev.append(pyevents.claimed_event(blocks, c) if s == 1 or 12 <= s <= 17 else None)
        return (bytes(st), tuple(ev))
    if kind == "verify_and_scan_device":
        f, t, sf, sa = args
        first = b.claims[0]  # the scan is of tipsets[0]'s child: the first claim's
        child = pystorage.cid_from_string(first["child_block_cid"])
        scan = answer_hand(ws, ("scan_events", op[1], (sf, sa, 0, 0)))  # (roots[0] is that child's receipts root)
        assert pyevents.header(blocks[child]).receipts == b.roots[0]
        return (answer_hand(ws, ("verify_event_claims", op[1], (f, t))), scan)
    if kind == "exec_order":
        try:
            out = pyevents.exec_order(blocks, b.parents[args[0]])
            return (1, b"".join(slot40(c) for c in out))
        except pystorage.Err as e:
            return (e.status,)
    if kind == "generate_event_proofs":
        f, a, which = args
        st, proofs, needed = pyevents.generate(blocks, b.parents[which], b.children[which], *b.filters[f], b.actors[a])
        if st != 1:
            return (st,)
        return (1, tuple(p[:3] for p in proofs), b"".join(slot40(p[3]) for p in proofs), frozenset(needed))
    if kind == "amt_get":
        root, version, vkind, idx = amt_query(ws, args)
        check = pyevents.check_receipt if vkind == "receipt" else pyevents.check_stamped_event
        try:
            amt = pyevents.amt_load(blocks, root, version, check)
        except pystorage.Err as e:
            return (bytes([e.status] * len(idx)), ())
        st, vals = [], []
        for i in idx:
            try:
                v = pyevents.amt_get(amt, i)
                st.append(32 if v is pyevents.ABSENT else 1)
                if v is not pyevents.ABSENT:
                    vals.append(v)
            except pystorage.Err as e:
                st.append(e.status)
        return (bytes(st), tuple(vals))
    raise KeyError(kind)


# ---- sequences ----------------------------------------------------------------------------------------------------------------------
def circuit(kinds, rng):
    """an Eulerian circuit of the complete directed graph with self-loops over `kinds` (Hierholzer, edges in a seeded order):
    len(kinds)² + 1 kinds, every ordered pair adjacent exactly once"""
    k = len(kinds)
    out_edges = {a: [int(x) for x in rng.permutation(k)] for a in range(k)}
    stack, path = [0], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop())
        else:
            path.append(stack.pop())
    path.reverse()
    assert len(path) == k * k + 1
    return [kinds[i] for i in path]


def adjacencies(ops):
    """→ (pairs, after_other, after): {(witness, X, Y)} adjacent in that witness's own order, the kinds that directly follow
    an op on another witness, and {(X, Y)} for X a failing call or one of AFTER with Y next to it in the sequence itself,
    on the same witness"""
    pairs, after_other, after = set(), set(), set()
    last_on = {}
    for i, (kind, wit, _) in enumerate(ops):
        if wit in last_on:
            pairs.add((wit, last_on[wit], kind))
        last_on[wit] = kind
        if i:
            pk, pw, _ = ops[i - 1]
            if pw != wit:
                after_other.add(kind)
            elif pk in AFTER + FAILING_KINDS:
                after.add((pk, kind))
    return pairs, after_other, after


def coverage_gaps(ops):
    """What the conditions of tests/test_call_sequences.py still miss in `ops`, as (previous op kind or None, kind, witness)
    adjacencies to append:
      * every ordered pair of op kinds of a witness is adjacent in that witness's own order;
      * every op kind directly follows an op on another witness;
      * every op kind directly follows EACH of the four failing calls, and each of rebuild_index, put_replace,
        set_receipt_range and close_and_recreate — on the same witness and next to it in the sequence itself (the context,
        not only the witness, carries what such a call leaves)."""
    pairs, after_other, after = adjacencies(ops)
    gaps = []
    for wit, kinds in KINDS.items():
        gaps += [(a, b, wit) for a in kinds for b in kinds if (wit, a, b) not in pairs]
    every = sorted({k for ks in KINDS.values() for k in ks})
    for k in every:
        home = "A" if k in KINDS["A"] else "C"
        if k not in after_other:
            gaps.append((None, k, home))
        for s in AFTER + FAILING_KINDS:
            if (s, k) not in after:
                gaps.append((s, k, home))
    return gaps


def sequence(seed=None):
    """the whole sequence of a seed: [(kind, witness, args)]"""
    seed = fuzz_seed(BASE_SEED) if seed is None else seed
    rng = np.random.default_rng([seed, 1])
    circuits = {w: circuit(list(k), rng) for w, k in KINDS.items()}
    # interleave: runs of one to four ops of one witness, the witness drawn in proportion to what it has left
    at = {w: 0 for w in circuits}
    order = []
    while any(at[w] < len(c) for w, c in circuits.items()):
        left = np.array([len(circuits[w]) - at[w] for w in "ABC"], dtype=float)
        w = "ABC"[int(rng.choice(3, p=left / left.sum()))]
        for _ in range(int(rng.integers(1, 5))):
            if at[w] < len(circuits[w]):
                order.append((circuits[w][at[w]], w))
                at[w] += 1
    # extend until nothing is missing (an appended adjacency X → Y on W: an op on another witness, X on W, Y on W)
    for _ in range(8):
        gaps = coverage_gaps([(k, w, ()) for k, w in order])
        if not gaps:
            break
        for prev, kind, wit in gaps:
            other = "C" if wit != "C" else "A"
            if prev is None:
                order += [("has_get", other), (kind, wit)]
            else:
                order += [("has_get", other), (prev, wit), (kind, wit)]
    assert not coverage_gaps([(k, w, ()) for k, w in order])
    order += [("set_tuning", "A")] * len(TUNING)  # everything goes back to -1 at the end
    # the sequence OPENS with burst 0: default tuning, and no call before it has sized the context's HAMT node tables
    order.insert(0, ("burst", "A"))
    ops, nth, walks, burst_seen = [], {}, {}, False
    for kind, wit in order:
        space = arg_space(kind, wit)
        n = nth[(kind, wit)] = nth.get((kind, wit), -1) + 1
        if kind == "burst" and not burst_seen:
            args, burst_seen = (0,), True
        elif space is None:
            args = (n % 3, int(rng.integers(1 << 16))) if kind == "amt_get" else (int(rng.integers(1 << 16)),)
        else:
            if (kind, wit) not in walks:
                walks[(kind, wit)] = [space[int(i)] for i in rng.permutation(len(space))]
            args = walks[(kind, wit)][n % len(space)]
        ops.append((kind, wit, args))
    for j in range(len(TUNING)):
        ops[len(ops) - len(TUNING) + j] = ("set_tuning", "A", (j, 0))
    return ops


def chunks(ops, size=CHUNK):
    return [(i, ops[i: i + size]) for i in range(0, len(ops), size)]


# ---- the reference, long-lived ----------------------------------------------------------------------------------------------------
class LongLived:
    """The oracle with one store per witness kept across the ops, rebuilt only where the model's blocks change."""

    def __init__(self, model):
        self.model = model
        self.stores = {}

    def answer(self, op):
        if op[0] == "burst":
            return tuple(self.answer(p) for p in burst_parts(op))
        ws = self.model.w[op[1]]
        if ws.base.hand:
            return answer_hand(ws, op)
        held = self.stores.get(op[1])
        if held is None or held[0] != ws.version:
            if held is not None:
                held[1].close()
            held = (ws.version, self.model.orc.store(*ws.tables()))
            self.stores[op[1]] = held
        return answer_oracle(self.model.orc, held[1], ws, op, held=True)

    def close(self):
        for _, s in self.stores.values():
            s.close()
        self.stores = {}


# ---- the engine ---------------------------------------------------------------------------------------------------------------------
def dev(a):
    import torch

    a = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(np.concatenate([a, np.zeros(64, np.uint8)])).cuda()  # (never an empty allocation)


def error_code(e):
    m = re.search(r"\((-\d+)\)", str(e))
    return int(m.group(1)) if m else None


class Runner:
    """One context and the three witnesses kept resident; `run(op)` gives the engine's answer in the model's form."""

    def __init__(self, eng, model):
        self.eng, self.model = eng, model
        self.w = {}
        self.at = None  # the position in the sequence the engine's state stands at (tests/test_gpu_call_sequences.py)

    def open(self, name):
        if name in self.w:
            self.w.pop(name).close()
        ws = self.model.w[name]
        self.w[name] = self.eng.witness(*ws.tables())
        if ws.range != FULL:
            self.w[name].set_receipt_range(*ws.range)

    def adopt(self):
        """bring the engine to the model's present state: fresh witnesses of its blocks, its ranges, its tuning"""
        for name in self.model.w:
            self.open(name)
        for k, v in self.model.tuning.items():
            self.eng.set_tuning(k, v)

    def close(self):
        for w in self.w.values():
            w.close()
        self.w = {}
        for k, _ in TUNING:
            self.eng.set_tuning(k, -1)

    def step(self, op):
        """lift, run, apply: → the engine's answer; the model has moved past `op` afterwards"""
        for name in self.model.lifts(op):
            self.w[name].set_receipt_range(*FULL)
        got = self.run(op)
        self.model.apply(op)
        return got

    def _filters(self, b, f, t):
        if b.hand:
            return ec.trust_policy(b.trusts[t]), (ec.event_filter(b.filters[f - 1]) if f else None)
        return trust_of(t, b.tip.parent_epoch, b.tip.child_epoch), (claims_mod.make_filter(*b.filters[f - 1]) if f else None)

    def _cids(self, ws, ids):
        return frozenset(slot40(ws.cids[int(i)]) for i in ids)

    def _routed(self, ws, cl):
        """the packed claims of the witness's receipt range (the whole batch without one), as a host routes them"""
        b = ws.base
        if ws.range == FULL:
            return cl, b.blob, b.blob_len
        pos, cl2, blob, blob_len = ipcfp.route_event_claims(cl, b.blob, b.blob_len, ws.range[0], ws.range[1], False)
        assert np.array_equal(pos, in_range(cl["exec_index"], ws.range))
        return cl2, blob, blob_len

    def _values(self, w, loc, pick):
        return tuple(w.read_values(loc[pick], stride=2048)) if len(pick) else ()

    # -- device entry points: prepared, then issued back to back, then read after the one synchronisation --
    def prepare(self, op):
        """→ (issue, done) of one device entry point.  Everything of torch's — uploads, output buffers, their canary fills —
        is made HERE; `issue()` is the engine call and nothing else; `done()` reads the outputs once the caller has
        synchronised.  The caller waits for torch's stream between the last prepare and the first issue, so that a fill
        cannot land on top of an engine write; between two issues nothing waits."""
        import torch

        kind, wit, args = op
        ws, w = self.model.w[wit], self.w[wit]
        b = ws.base
        if kind == "hamt_get":
            vk, bw, batch = args
            keys = b.keys[batch]
            kl = np.array([len(k) for k in keys], dtype=np.uint32)
            ko = np.zeros(len(keys), dtype=np.uint32)
            ko[1:] = np.cumsum(kl[:-1])
            d = [dev(np.frombuffer(b"".join(keys), dtype=np.uint8)), dev(ko), dev(kl)]
            d_st = torch.zeros(len(keys) + 64, dtype=torch.uint8, device="cuda")
            d_loc = torch.zeros(len(keys) * 12 + 64, dtype=torch.uint8, device="cuda")

            def issue():
                w.hamt_get_device(b.tip.actors_root, (5, 4, 8)[bw], ("actor_state", "any", "vec_u8")[vk], d[0].data_ptr(),
                                  d[1].data_ptr(), d[2].data_ptr(), len(keys), d_st.data_ptr(), d_loc.data_ptr())

            def done():
                st = d_st.cpu().numpy()[: len(keys)]
                loc = d_loc.cpu().numpy()[: len(keys) * 12].view(ipcfp.LOC_DTYPE)
                return (st.tobytes(), self._values(w, loc, np.nonzero(st == 1)[0][:16]))
            return issue, done
        if kind in ("verify_event_claims", "verify_and_scan_device"):
            f, t = args[:2]
            tp, ft = self._filters(b, f, t)
            cl, blob, blob_len = self._routed(ws, b.cl)
            d_cl, d_blob = dev(cl), dev(blob)
            n = len(cl)
            d_st = torch.full((n + 64,), 77, dtype=torch.uint8, device="cuda")
            if kind == "verify_event_claims":
                def issue():
                    w.verify_event_claims_device(b.ts, d_cl.data_ptr(), n, d_blob.data_ptr(), blob_len, d_st.data_ptr(), trust=tp, filt=ft)
                return issue, lambda: d_st.cpu().numpy()[:n].tobytes()
            sf, sa = args[2:]
            cap_r, cap_m = 4096, 4096
            d_has = torch.full((cap_r + 64,), 9, dtype=torch.uint8, device="cuda")
            d_m = torch.zeros(cap_m * ipcfp.MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            out = []

            def issue():
                out.append(w.verify_and_scan_device(b.ts, d_cl.data_ptr(), n, d_blob.data_ptr(), blob_len, d_st.data_ptr(),
                                                    *b.filters[sf], b.actors[sa], d_has.data_ptr(), cap_r, d_m.data_ptr(), cap_m,
                                                    trust=tp, filt=ft))
            return issue, lambda: (d_st.cpu().numpy()[:n].tobytes(), self._device_scan(*out[0], d_has, d_m, cap_r))
        if kind == "scan_events":
            f, a, _touched, root = args
            cap_r, cap_m = 4096, 4096
            d_has = torch.full((cap_r + 64,), 9, dtype=torch.uint8, device="cuda")
            d_m = torch.zeros(cap_m * ipcfp.MATCH_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            out = []

            def issue():
                out.append(w.scan_events_device(b.roots[root], *b.filters[f], b.actors[a], d_has.data_ptr(), cap_r, d_m.data_ptr(), cap_m))
            return issue, lambda: self._device_scan(*out[0], d_has, d_m, cap_r)
        if kind == "verify_storage_columns":
            cols = ipcfp.compact_storage_claims(b.scl[args[0]])
            d = [dev(cols.runs), dev(cols.slot), dev(cols.value), dev(cols.cflags)]
            n, n_runs = cols.n, cols.n_runs
            cols.close()
            d_st = torch.full((n + 64,), 0xAA, dtype=torch.uint8, device="cuda")

            def issue():
                w.verify_storage_columns_device(d[0].data_ptr(), n_runs, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, d_st.data_ptr())
            return issue, lambda: d_st.cpu().numpy()[:n].tobytes()
        if kind == "generate_storage_claims":
            ids, slots = b.gen_specs(args[0])
            d = [dev(ids), dev(slots)]
            out = []

            def issue():
                out.append(w.generate_storage_claims_device(b.tip.child_cid, b.tip.child_epoch, d[0].data_ptr(), d[1].data_ptr(), len(ids)))

            def done():
                try:
                    return generated_rows(out[0])
                finally:
                    out[0].close()
            return issue, done
        raise KeyError(kind)

    def issue_all(self, parts):
        """the device entry points of `parts` queued back to back with no synchronisation between them, then ONE sync"""
        import torch

        prepared = [self.prepare(p) for p in parts]
        torch.cuda.current_stream().synchronize()  # torch's own stream only: its uploads and fills are through
        for issue, _ in prepared:
            issue()
        self.eng.sync()
        return tuple(done() for _, done in prepared)

    def _device_scan(self, sst, snr, snm, d_has, d_m, cap_r):
        if sst != 1:
            return (sst,)
        has = d_has.cpu().numpy()
        assert snr <= cap_r and (has[cap_r:] == 9).all()
        m = d_m.cpu().numpy()[: snm * ipcfp.MATCH_DTYPE.itemsize].view(ipcfp.MATCH_DTYPE)
        return (1, has[:snr].tobytes(), tuple(zip(m["exec_index"].tolist(), m["event_index"].tolist(), m["emitter"].tolist())), None)

    # -- one op --
    def run(self, op):
        import torch

        kind, wit, args = op
        if kind == "burst":
            return self.issue_all(burst_parts(op))
        ws, w = self.model.w[wit], self.w[wit]
        b = ws.base
        if kind == "verify_cids":
            st, nbad = w.verify_cids()
            return (st.tobytes(), nbad)
        if kind == "scan_events":
            f, a, touched, root = args
            touched = bool(touched) and ws.range == FULL
            gs, has, m, ids = w.scan_events(b.roots[root], *b.filters[f], actor=b.actors[a], want_touched=touched)
            if gs != 1:
                return (gs,)
            trip = tuple(zip(m["exec_index"].tolist(), m["event_index"].tolist(), m["emitter"].tolist()))
            return (1, has.tobytes(), trip, self._cids(ws, ids) if touched else None)
        if kind == "verify_event_claims":
            tp, ft = self._filters(b, *args)
            cl, blob, blob_len = self._routed(ws, b.cl)
            return w.verify_event_claims(b.ts, cl, blob, blob_len, trust=tp, filt=ft).tobytes()
        if kind in ("verify_event_claims_compact", "bad_compact_group"):
            tp, ft = self._filters(b, *(args or (0, 0)))
            cl, blob, blob_len = self._routed(ws, b.cl if b.hand else b.cl_u32)
            groups, cc, cblob, cblob_len = ipcfp.compact_event_claims(cl, blob, blob_len)
            if kind == "bad_compact_group":
                cc = cc.copy()
                cc["group"][bad_group(ws)] = 77
            return w.verify_event_claims_compact(b.ts, groups, cc, cblob, cblob_len, trust=tp, filt=ft).tobytes()
        if kind in ("verify_event_proofs", "verify_event_proofs_located"):
            tp, ft = self._filters(b, *args)
            pr = b.proofs if b.hand else b.string_claims(ws.range)[1]
            if kind == "verify_event_proofs":
                return w.verify_event_proofs(pr.arr, pr.n, trust=tp, filt=ft).tobytes()
            st, loc = w.verify_event_proofs_located(pr.arr, pr.n, trust=tp, filt=ft)
            cmp = [i for i in range(pr.n) if st[i] == 1 or 12 <= st[i] <= 17]
            raw = dict(zip(cmp, w.read_values(loc[cmp], stride=2048))) if cmp else {}
            if b.hand:  # pyevents states the checked event, not its bytes
                raw = {i: pyevents.check_stamped_event(pystorage.decode(v)) for i, v in raw.items()}
            return (st.tobytes(), tuple(raw.get(i) for i in range(pr.n)))
        if kind == "verify_and_scan_device":
            return self.issue_all([op])[0]
        if kind == "exec_order":
            st, out = w.exec_order(b.parents[args[0]])
            return (st, out.tobytes()) if st == 1 else (st,)
        if kind == "generate_event_proofs":
            f, a, which = args
            parents, child = (b.parents[which], b.children[which]) if b.hand else (b.tip.parent_cids, b.tip.child_cid)
            st, m, msg, ids = w.generate_event_proofs(parents, child, *b.filters[f], actor=b.actors[a])
            if st != 1:
                return (st,)
            trip = tuple(zip(m["exec_index"].tolist(), m["event_index"].tolist(), m["emitter"].tolist()))
            wit_cids = [ws.cids[int(i)] for i in ids]
            return (1, trip, msg.tobytes(), frozenset(wit_cids) if b.hand else tuple(slot40(c) for c in wit_cids))
        if kind == "amt_get":
            root, version, vkind, idx = amt_query(ws, args)
            st, loc = w.amt_get(root, version, vkind, idx)
            vals = self._values(w, loc, np.nonzero(st == 1)[0])
            if b.hand:
                check = pyevents.check_receipt if vkind == "receipt" else pyevents.check_stamped_event
                vals = tuple(check(pystorage.decode(v)) for v in vals)
            return (st.tobytes(), vals)
        if kind == "hamt_get":
            vk, bw, batch = args
            st, loc = w.hamt_get(b.tip.actors_root, (5, 4, 8)[bw], ("actor_state", "any", "vec_u8")[vk], b.keys[batch])
            return (st.tobytes(), self._values(w, loc, np.nonzero(st == 1)[0][:16]))
        if kind == "verify_storage_proofs":
            sc = b.sc[args[0]]
            return w.verify_storage_proofs(sc.arr, sc.n).tobytes()
        if kind == "verify_storage_columns":
            with ipcfp.compact_storage_claims(b.scl[args[0]]) as cols:
                return w.verify_storage_columns(cols).tobytes()
        if kind == "generate_storage_claims":
            ids, slots = b.gen_specs(args[0])
            with w.generate_storage_claims(b.tip.child_cid, b.tip.child_epoch, ids, slots) as g:
                return generated_rows(g)
        if kind == "has_get":
            picks = has_get_picks(ws, args[0])
            has, _ids = w.has(picks)
            got = tuple(w.get(c) for c in picks)
            assert has.tolist() == [int(g is not None) for g in got], (has.tolist(), got)
            return got
        # -- state --
        if kind == "rebuild_index":
            w.rebuild_index()
            return None
        if kind in BLOCK_CHANGING:
            cid, blk = self.model.new_block(op)
            w.put_keyed([cid], [blk])
            return ("blocks", w.block_count)
        if kind == "set_receipt_range":
            w.set_receipt_range(*receipt_range(b, args[0]))
            return None
        if kind == "close_and_recreate":
            self.open(wit)  # (a range the model holds is set on the new witness again)
            return ("blocks", self.w[wit].block_count)
        if kind == "set_tuning":
            self.eng.set_tuning(TUNING[args[0]][0], TUNING[args[0]][1][args[1]])
            return None
        # -- failing calls --
        if kind == "bad_run_table":
            with ipcfp.compact_storage_claims(b.scl[0]) as cols:
                runs = cols.runs.copy()
                runs["n_claims"][-1] -= 1  # the table no longer reaches the last claim
                d = [dev(runs), dev(cols.slot), dev(cols.value), dev(cols.cflags)]
                n, n_runs = cols.n, cols.n_runs
            d_st = torch.full((n + 64,), 0xAA, dtype=torch.uint8, device="cuda")
            torch.cuda.current_stream().synchronize()  # (torch's fills are through before the engine writes)
            try:
                w.verify_storage_columns_device(d[0].data_ptr(), n_runs, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), n, d_st.data_ptr())
            except ipcfp.EngineError as e:
                return ("rc", error_code(e))
            return ("rc", 0)
        if kind == "bad_bundle_block_id":
            try:
                w.write_bundle_json(None, 0, None, 0, block_ids=[0, w.block_count, 1])
            except ipcfp.EngineError as e:
                return ("rc", error_code(e))
            return ("rc", 0)
        if kind == "short_scan_cap":
            d_has = torch.full((SHORT_CAP + 64,), 9, dtype=torch.uint8, device="cuda")
            torch.cuda.current_stream().synchronize()  # (torch's fills are through before the engine writes)
            sst, snr, snm = w.scan_events_device(b.roots[0], *b.filters[0], b.actors[0], d_has.data_ptr(), SHORT_CAP)
            self.eng.sync()
            has = d_has.cpu().numpy()
            assert sst == 1 and (has[SHORT_CAP:] == 9).all(), "the scan wrote behind the has-match buffer it was given"
            return ("overflow", int(snr > SHORT_CAP), has[: min(snr, SHORT_CAP)].tobytes(), snr, snm)
        raise KeyError(kind)


def generated_rows(g):
    """a generated storage batch in the model's form: (status bytes, per spec (the three derived CID slots, value) | None)"""
    st = g.status()
    runs, _slot, value, _cflags = g.copy()
    derived = [None] * g.n
    for r in runs:
        for i in range(int(r["first_claim"]), int(r["first_claim"]) + int(r["n_claims"])):
            derived[i] = r["state_root"].tobytes() + r["actor_state"].tobytes() + r["storage_root"].tobytes()
    return (st.tobytes(), tuple((derived[i], value[i].tobytes()) if st[i] == 1 else None for i in range(g.n)))


def replay(ops, seed=None, engine=None):
    """Run a literal sequence from fresh witnesses on a context of its own (or `engine`) → [(position, op, got, want)] of
    the ops whose answer differs from the model's.  What a failure message of tests/test_gpu_call_sequences.py prints is
    an argument of this function."""
    own = engine is None
    if own:
        import torch

        if torch.cuda.is_available():
            torch.cuda.init()
        engine = ipcfp.Engine(0)
    model = Model(seed)
    run = Runner(engine, model)
    wrong = []
    try:
        run.adopt()
        for i, op in enumerate(ops):
            op = (op[0], op[1], tuple(op[2]))
            for name in model.lifts(op):
                run.w[name].set_receipt_range(*FULL)
            want = model.expect(op)
            got = run.run(op)
            model.apply(op)
            if got != want:
                wrong.append((i, op, got, want))
    finally:
        run.close()
        if own:
            engine.close()
    return wrong
