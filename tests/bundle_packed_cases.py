"""Shared case table of the packed bundle writer (ipcfp_bundle_write_packed_json): packed claims as the generators leave them
in HBM — storage claims in column form, event claims + blob + tipset table — and what the call must answer: the head of the
text, `{"storage_proofs":[…],"event_proofs":[…],"blocks":[`, or the refusal (rc, kind, index).

The expected text is built HERE, in Python: bundle_ref.storage_json / event_json over dicts whose CID strings come from
pystorage.cid_to_string.  The engine's host route (unpack_* + ipcfp_bundle_write_claims_json) is a second judge
(tests/test_bundle_packed_cases.py), the device writer the subject (tests/test_gpu_bundle_write_packed.py)."""
import hashlib

import numpy as np

import bundle_ref
import pystorage
from ipc_filecoin_proofs_amd.binding import _SRUN_DTYPE, CLAIM_DTYPE, MAX_PARENTS, SCLAIM_DTYPE, TIPSET_DTYPE

E_INVALID, E_UNSUPPORTED = -1, -5
STORAGE, EVENTS, BLOCKS = 0, 1, 2
HEAD = '{"storage_proofs":[%s],"event_proofs":[%s],"blocks":['

I64_MAX, I64_MIN, U64_MAX = 2**63 - 1, -(2**63), 2**64 - 1
# parent_epoch / child_epoch
EPOCHS = ([0, -1, 9, 10] + [v for k in range(2, 19) for v in (10**k - 1, 10**k)] + [-v for k in range(2, 19) for v in (10**k - 1, 10**k)]
          + [I64_MAX, I64_MIN])
# exec_index, event_index, emitter, actor_id
UINTS = [0] + [v for k in range(1, 20) for v in (10**k - 1, 10**k)] + [2**32 - 1, 2**32, U64_MAX]


def _digest(tag) -> bytes:
    return hashlib.sha256(repr(tag).encode()).digest()


def cid38(tag) -> bytes:
    """the usual CID of the chain: v1, dag-cbor, blake2b-256"""
    return bytes.fromhex("0171a0e40220") + _digest(tag)


# every shape of CID a 40-byte slot can hold whole; lengths mod 5 cover every residue (base32 tails) and 40 fills the slot
SOUND_CIDS = [
    cid38("usual"),
    b"\x12\x20" + bytes(32),                                   # CIDv0, digest all zero
    b"\x12\x20" + b"\xff" * 32,                                # CIDv0, digest all ff
    b"\x12\x20" + _digest("v0"),                               # CIDv0, random
    bytes.fromhex("01550000"),                                 # identity, 4 bytes
    bytes.fromhex("01551220") + _digest(36),                   # 36 bytes
    bytes.fromhex("0191011220") + _digest(37),                 # 37 bytes: two-byte codec varint
    bytes.fromhex("019101a0e40220") + _digest(39),             # 39 bytes
    bytes.fromhex("01808001a0e40220") + _digest(40),           # 40 bytes: the slot is full
]
assert sorted(len(c) for c in SOUND_CIDS) == [4, 34, 34, 34, 36, 37, 38, 39, 40]
assert {len(c) % 5 for c in SOUND_CIDS if len(c) != 34} == {0, 1, 2, 3, 4}


class Raw(bytes):
    """40 bytes that go into a slot as they are (malformed on purpose)"""


FOLDED = Raw(b"\xff\x2a" + _digest("fold") + bytes(6))
TRAILING = Raw(cid38("trail") + b"\x00\x01")                    # a non-zero byte behind the CID
TRUNCATED = Raw(b"\x01\x71" + b"\x80" * 38)                     # a varint that never ends
assert len(FOLDED) == len(TRAILING) == len(TRUNCATED) == 40


def slot(c) -> np.ndarray:
    s = np.zeros(40, dtype=np.uint8)
    s[: len(c)] = np.frombuffer(bytes(c), dtype=np.uint8)
    return s


class Case:
    """Packed inputs + the expected outcome.  storage: runs / slot / value / cflags; events: tipsets / claims / blob."""

    def __init__(self, name):
        self.name = name
        self.runs = np.zeros(0, dtype=_SRUN_DTYPE)
        self.slot = np.zeros((0, 32), dtype=np.uint8)
        self.value = np.zeros((0, 32), dtype=np.uint8)
        self.cflags = np.zeros(0, dtype=np.uint8)
        self.tipsets = np.zeros(0, dtype=TIPSET_DTYPE)
        self.claims = np.zeros(0, dtype=CLAIM_DTYPE)
        self.blob = np.zeros(0, dtype=np.uint8)
        self.keep = []           # arrays the tipsets' more_parents point into
        self.storage_dicts = []  # what a sound case spells
        self.event_dicts = []
        self.refusal = None      # (rc, kind, index or None)

    @property
    def n_storage(self):
        return len(self.cflags)

    @property
    def n_events(self):
        return len(self.claims)

    @property
    def blob_len(self):
        return len(self.blob)

    def head(self) -> bytes:
        assert self.refusal is None
        return (HEAD % (",".join(bundle_ref.storage_json(p) for p in self.storage_dicts),
                        ",".join(bundle_ref.event_json(p) for p in self.event_dicts))).encode()

    def expected(self):
        return self.refusal if self.refusal is not None else self.head()

    def refuse(self, rc, kind, index):
        self.refusal = (rc, kind, index)
        return self


def _cidstr(c):
    return None if isinstance(c, Raw) else pystorage.cid_to_string(bytes(c))


def _rng(name):
    return np.random.default_rng(int.from_bytes(hashlib.sha256(name.encode()).digest()[:8], "little"))


def add_storage(case, run_list):
    """run_list: dicts(epoch, actor, cids=[child, state_root, actor_state, storage_root], n, flags=15, reserved=0); the runs are
    laid end to end (first_claim may be overridden with `first`), slot and value are seeded random bytes, cflags 48"""
    rng = _rng("s:" + case.name)
    runs = np.zeros(len(run_list), dtype=_SRUN_DTYPE)
    at = case.n_storage
    slots, values = [case.slot], [case.value]
    for r, spec in zip(runs, run_list):
        r["child_epoch"], r["actor_id"] = spec["epoch"], spec["actor"]
        for f, c in zip(("child", "state_root", "actor_state", "storage_root"), spec["cids"]):
            r[f] = slot(c)
        r["first_claim"], r["n_claims"] = spec.get("first", at), spec.get("n_claims", spec["n"])
        r["flags"], r["reserved"] = spec.get("flags", 15), spec.get("reserved", 0)
        n = spec["n"]
        s, v = rng.integers(0, 256, (n, 32), dtype=np.uint8), rng.integers(0, 256, (n, 32), dtype=np.uint8)
        slots.append(s)
        values.append(v)
        strs = [_cidstr(c) for c in spec["cids"]]
        for i in range(n):
            case.storage_dicts.append(dict(child_epoch=spec["epoch"], child_block_cid=strs[0], parent_state_root=strs[1],
                                           actor_id=spec["actor"], actor_state_cid=strs[2], storage_root=strs[3],
                                           slot="0x" + s[i].tobytes().hex(), value="0x" + v[i].tobytes().hex()))
        at += n
    case.runs = np.concatenate([case.runs, runs])
    case.slot, case.value = np.concatenate(slots), np.concatenate(values)
    case.cflags = np.concatenate([case.cflags, np.full(at - case.n_storage, 48, dtype=np.uint8)])
    return case


def add_tipset(case, parents, child, flags=3):
    t = np.zeros(1, dtype=TIPSET_DTYPE)
    t["flags"], t["n_parents"] = flags, len(parents)
    t["child"][0] = slot(child)
    for j, p in enumerate(parents[:MAX_PARENTS]):
        t["parents"][0, j] = slot(p)
    if len(parents) > MAX_PARENTS:
        more = np.stack([slot(p) for p in parents[MAX_PARENTS:]])
        case.keep.append(more)
        t["more_parents"] = more.ctypes.data
    case.tipsets = np.concatenate([case.tipsets, t])
    case._tipset_strs = getattr(case, "_tipset_strs", []) + [([_cidstr(p) for p in parents], _cidstr(child))]
    return len(case.tipsets) - 1


def add_event(case, tipset, pe=6, ce=7, exec_index=3, event_index=1, emitter=1234, msg=None, topics=(), data=b"", flags=3,
              topic_flags=None):
    c = np.zeros(1, dtype=CLAIM_DTYPE)
    msg = cid38(("msg", case.name, len(case.claims))) if msg is None else msg
    c["parent_epoch"], c["child_epoch"], c["exec_index"], c["event_index"], c["emitter"] = pe, ce, exec_index, event_index, emitter
    c["message_cid"][0] = slot(msg)
    c["tipset"], c["flags"], c["n_topics"] = tipset, flags, len(topics)
    tf = topic_flags if topic_flags is not None else [1] * len(topics)
    seg = b"".join(bytes([f]) + bytes(t) for f, t in zip(tf, topics))
    c["topics_off"], c["data_off"], c["data_len"] = len(case.blob), len(case.blob) + len(seg), len(data)
    case.blob = np.concatenate([case.blob, np.frombuffer(seg + bytes(data), dtype=np.uint8)])
    case.claims = np.concatenate([case.claims, c])
    if tipset < len(case.tipsets):
        parents, child = case._tipset_strs[tipset]
        case.event_dicts.append(dict(parent_epoch=pe, child_epoch=ce, parent_tipset_cids=parents, child_block_cid=child,
                                     message_cid=_cidstr(msg), exec_index=exec_index, event_index=event_index, emitter=emitter,
                                     topics=["0x" + bytes(t).hex() for t in topics], data="0x" + bytes(data).hex()))
    return case


def _topics(rng, n):
    return [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(n)]


def _run(tag, n, **kw):
    d = dict(epoch=7, actor=1001, cids=[cid38((tag, k)) for k in range(4)], n=n)
    d.update(kw)
    return d


DATA_LENS = [0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 65537]
TOPIC_COUNTS = [0, 1, 4, 5, 8]


def sound_cases():
    out = []
    out.append(Case("empty"))
    # integers: every listed value in every integer field
    c = Case("integers")
    add_storage(c, [_run(("int", i), 1, epoch=EPOCHS[i % len(EPOCHS)], actor=UINTS[i % len(UINTS)]) for i in range(len(EPOCHS))])
    t = add_tipset(c, [cid38("ip")], cid38("ic"))
    for i in range(len(EPOCHS)):
        add_event(c, t, pe=EPOCHS[i], ce=EPOCHS[-1 - i], exec_index=UINTS[i % len(UINTS)], event_index=UINTS[(i + 7) % len(UINTS)],
                  emitter=UINTS[(i + 13) % len(UINTS)])
    out.append(c)
    # CID slots: every sound shape as child, state root, actor state, storage root, parent, tipset child and message CID
    c = Case("cids")
    k = len(SOUND_CIDS)
    add_storage(c, [_run(None, 2, cids=[SOUND_CIDS[(j + d) % k] for d in range(4)]) for j in range(k)])
    for j in range(k):
        t = add_tipset(c, [SOUND_CIDS[j], SOUND_CIDS[(j + 1) % k]], SOUND_CIDS[(j + 2) % k])
        add_event(c, t, msg=SOUND_CIDS[(j + 3) % k], topics=_topics(_rng("cids"), 1), data=b"\x01\x02")
    out.append(c)
    # event counts
    for n in (1, 63, 64, 65, 257):
        c = Case("events_%d" % n)
        t = add_tipset(c, [cid38(("p", j)) for j in range(5)], cid38("c"))
        rng = _rng(c.name)
        for i in range(n):
            add_event(c, t, exec_index=i, event_index=i % 7, topics=_topics(rng, TOPIC_COUNTS[i % 5]),
                      data=rng.integers(0, 256, int(rng.integers(0, 70)), dtype=np.uint8).tobytes())
        out.append(c)
    # data lengths and topic counts
    c = Case("event_shapes")
    t = add_tipset(c, [cid38("sp")], cid38("sc"))
    rng = _rng(c.name)
    for i, n in enumerate(DATA_LENS):
        add_event(c, t, event_index=i, topics=_topics(rng, TOPIC_COUNTS[i % 5]), data=rng.integers(0, 256, n, dtype=np.uint8).tobytes())
    out.append(c)
    # tipset keys of 1, 5, 32 and 33 parents (33: more_parents); claims of two tipsets interleaved; a tipset with bad flags
    # that no claim names
    c = Case("tipsets")
    ts = [add_tipset(c, [cid38(("tp", n, j)) for j in range(n)], cid38(("tc", n))) for n in (1, 5, 32, 33)]
    add_tipset(c, [cid38("unnamed")], cid38("unnamed child"), flags=1)
    add_tipset(c, [FOLDED], TRUNCATED)  # … and one without a string form
    for i in range(12):
        add_event(c, ts[(0, 3, 1, 3, 2, 3)[i % 6]], pe=100 + i, ce=101 + i, exec_index=i, data=bytes([i]) * i)
    out.append(c)
    # storage runs
    c = Case("run_lengths")
    add_storage(c, [_run(("rl", n), n, actor=n) for n in (1, 2, 63, 64, 65, 256, 257)])
    out.append(c)
    for n_runs in (1, 2, 33):
        c = Case("runs_%d" % n_runs)
        add_storage(c, [_run(("rn", n_runs, r), 1 + r % 3, epoch=-r, actor=10**(r % 19)) for r in range(n_runs)])
        out.append(c)
    # The host route judges the EXPANDED claim, flags = run's | claim's == 63: run flags 31 (a column bit set in the run) and
    # cflags 49 (a run bit set in the column) spell the same six bits, so both are sound there — and here
    c = Case("run_flags_31")
    add_storage(c, [_run("a", 3), _run("b", 4, flags=31), _run("c", 2)])
    out.append(c)
    c = Case("cflags_49")
    add_storage(c, [_run("a", 3), _run("b", 70)])
    c.cflags[66] = 49
    out.append(c)
    c = Case("run_flags_14_cflags_49")
    add_storage(c, [_run("a", 3), _run("b", 2, flags=14)])
    c.cflags[3:] = 49
    out.append(c)
    # placement: the first storage claim's actor id grows a digit per case, so everything behind it moves a byte
    for d in range(16):
        c = Case("place_%d" % d)
        add_storage(c, [_run(("pl", 0), 1, actor=10**d), _run(("pl", 1), 2, actor=5)])
        t = add_tipset(c, [cid38("pp")], cid38("pc"))
        add_event(c, t, data=b"\xab" * (d + 1))
        add_event(c, t, topics=_topics(_rng(c.name), 1), data=b"\xcd" * 20)
        out.append(c)
    return out


def _one_event(name, **kw):
    """three claims, the middle one as given"""
    c = Case(name)
    t = add_tipset(c, [cid38("rp")], cid38("rc"))
    add_event(c, t, data=b"\x01" * 8)
    add_event(c, kw.pop("tipset", t), **kw)
    add_event(c, t, data=b"\x02" * 8)
    return c


def refused_cases():
    out = []
    # run flags and the reserved word: the run's first claim
    for flags, reserved in ((14, 0), (0, 0), (64 + 15, 0), (15, 1)):
        c = Case("run_flags_%d_%d" % (flags, reserved))
        add_storage(c, [_run("a", 3), _run("b", 4, flags=flags, reserved=reserved), _run("c", 2)])
        out.append(c.refuse(E_INVALID, STORAGE, 3))
    for cf in (16, 32, 0, 64 + 48):
        c = Case("cflags_%d" % cf)
        add_storage(c, [_run("a", 3), _run("b", 70)])
        c.cflags[66] = cf
        out.append(c.refuse(E_INVALID, STORAGE, 66))
    # a run table that does not tile [0, n)
    c = Case("runs_gap")
    add_storage(c, [_run("a", 3), _run("b", 4)])
    c.runs["first_claim"][1] = 4
    out.append(c.refuse(E_INVALID, STORAGE, None))
    c = Case("runs_overlap")
    add_storage(c, [_run("a", 3), _run("b", 4)])
    c.runs["first_claim"][1] = 2
    out.append(c.refuse(E_INVALID, STORAGE, None))
    c = Case("runs_empty_run")
    add_storage(c, [_run("a", 3), _run("b", 0), _run("c", 4)])
    out.append(c.refuse(E_INVALID, STORAGE, None))
    c = Case("runs_short")
    add_storage(c, [_run("a", 3), _run("b", 4, n_claims=3)])
    out.append(c.refuse(E_INVALID, STORAGE, None))
    # malformed slots, in every position of a run
    for pos in range(4):
        for what, raw, rc in (("folded", FOLDED, E_UNSUPPORTED), ("trailing", TRAILING, E_INVALID), ("truncated", TRUNCATED, E_INVALID)):
            c = Case("run_slot_%d_%s" % (pos, what))
            cids = [cid38(("ok", k)) for k in range(4)]
            cids[pos] = raw
            add_storage(c, [_run("a", 5), _run("b", 2, cids=cids)])
            out.append(c.refuse(rc, STORAGE, 5))
    # events
    c = _one_event("tipset_index", tipset=1)
    out.append(c.refuse(E_INVALID, EVENTS, 1))
    for flags in (0, 1, 2):
        out.append(_one_event("claim_flags_%d" % flags, flags=flags).refuse(E_INVALID, EVENTS, 1))
    t3 = _topics(_rng("zero"), 3)
    out.append(_one_event("topic_flag_zero", topics=t3, topic_flags=[1, 0, 1]).refuse(E_INVALID, EVENTS, 1))
    c = Case("topics_past_blob")
    t = add_tipset(c, [cid38("rp")], cid38("rc"))
    add_event(c, t, data=b"\x01" * 40)
    add_event(c, t, topics=_topics(_rng("tp"), 1))
    c.claims["topics_off"][1] = c.blob_len - 33 + 1
    out.append(c.refuse(E_INVALID, EVENTS, 1))
    c = Case("data_past_blob")
    t = add_tipset(c, [cid38("rp")], cid38("rc"))
    add_event(c, t, data=b"\x01" * 40)
    add_event(c, t, data=b"\x02" * 9)
    c.claims["data_off"][1] = c.blob_len - 9 + 1
    out.append(c.refuse(E_INVALID, EVENTS, 1))
    for what, raw, rc in (("folded", FOLDED, E_UNSUPPORTED), ("trailing", TRAILING, E_INVALID), ("truncated", TRUNCATED, E_INVALID)):
        out.append(_one_event("message_%s" % what, msg=raw).refuse(rc, EVENTS, 1))
        for where in ("parent", "child"):
            c = Case("tipset_%s_%s" % (where, what))
            t = add_tipset(c, [cid38("rp")], cid38("rc"))
            bad = add_tipset(c, [cid38("x"), raw] if where == "parent" else [cid38("x")], cid38("y") if where == "parent" else raw)
            add_event(c, t)
            add_event(c, t)
            add_event(c, bad)
            out.append(c.refuse(rc, EVENTS, 2))
    # the tipset with bad flags of the sound table, with one claim naming it
    for flags in (0, 1, 2):
        c = Case("tipset_flags_%d" % flags)
        t = add_tipset(c, [cid38("rp")], cid38("rc"))
        bad = add_tipset(c, [cid38("unnamed")], cid38("unnamed child"), flags=flags)
        add_event(c, t)
        add_event(c, bad)
        out.append(c.refuse(E_INVALID, EVENTS, 1))
    # two defects in one batch: the lower index wins, whatever its code
    c = Case("two_defects")
    t = add_tipset(c, [cid38("rp")], cid38("rc"))
    for i in range(200):
        add_event(c, t, msg=FOLDED if i == 70 else None, flags=1 if i == 150 else 3)
    out.append(c.refuse(E_UNSUPPORTED, EVENTS, 70))
    c = Case("two_defects_swapped")
    t = add_tipset(c, [cid38("rp")], cid38("rc"))
    for i in range(200):
        add_event(c, t, msg=FOLDED if i == 150 else None, flags=1 if i == 70 else 3)
    out.append(c.refuse(E_INVALID, EVENTS, 70))
    # a storage defect and an event defect: storage is judged first
    c = Case("storage_before_events")
    add_storage(c, [_run("a", 100)])
    c.cflags[99] = 0
    t = add_tipset(c, [cid38("rp")], cid38("rc"))
    add_event(c, t, flags=0)
    out.append(c.refuse(E_INVALID, STORAGE, 99))
    return out


def merge(cases, name="merged"):
    """the sound cases laid end to end in one call: runs, tipset indices and blob offsets shifted"""
    m = Case(name)
    for c in cases:
        assert c.refusal is None
        runs = c.runs.copy()
        runs["first_claim"] += m.n_storage
        claims = c.claims.copy()
        claims["tipset"] += len(m.tipsets)
        claims["topics_off"] += m.blob_len
        claims["data_off"] += m.blob_len
        m.runs = np.concatenate([m.runs, runs])
        m.slot, m.value = np.concatenate([m.slot, c.slot]), np.concatenate([m.value, c.value])
        m.cflags = np.concatenate([m.cflags, c.cflags])
        m.tipsets = np.concatenate([m.tipsets, c.tipsets])
        m.claims = np.concatenate([m.claims, claims])
        m.blob = np.concatenate([m.blob, c.blob])
        m.keep += c.keep
        m.storage_dicts += c.storage_dicts
        m.event_dicts += c.event_dicts
    return m


def expand_rows(case):
    """ipcfp_expand_storage_claims restated: SCLAIM_DTYPE[n], or None where the run table does not tile [0, n)"""
    n = case.n_storage
    rows = np.zeros(n, dtype=SCLAIM_DTYPE)
    at = 0
    for r in case.runs:
        if int(r["n_claims"]) == 0 or int(r["first_claim"]) != at or at + int(r["n_claims"]) > n:
            return None
        for i in range(at, at + int(r["n_claims"])):
            for f in ("child_epoch", "actor_id", "child", "state_root", "actor_state", "storage_root"):
                rows[i][f] = r[f]
            rows[i]["slot"], rows[i]["value"] = case.slot[i], case.value[i]
            rows[i]["flags"], rows[i]["reserved"] = int(r["flags"]) | int(case.cflags[i]), r["reserved"]
        at += int(r["n_claims"])
    return rows if at == n else None


def placement(cases):
    """→ {kind: (start residues, end residues)} mod 16 of the claims' texts over the sound cases"""
    res = {"storage": (set(), set()), "events": (set(), set())}
    for c in cases:
        at = len('{"storage_proofs":[')
        for i, p in enumerate(c.storage_dicts):
            at += 1 if i else 0
            n = len(bundle_ref.storage_json(p))
            res["storage"][0].add(at % 16)
            res["storage"][1].add((at + n) % 16)
            at += n
        at += len('],"event_proofs":[')
        for i, p in enumerate(c.event_dicts):
            at += 1 if i else 0
            n = len(bundle_ref.event_json(p))
            res["events"][0].add(at % 16)
            res["events"][1].add((at + n) % 16)
            at += n
    return res


SOUND = sound_cases()
REFUSED = refused_cases()
ALL = SOUND + REFUSED
assert len({c.name for c in ALL}) == len(ALL)
# the table holds what it promises: a claim's text starts, and ends, at every residue mod 16 of the output
_pl = placement(SOUND)
assert all(len(s) == 16 and len(e) == 16 for s, e in _pl.values()), _pl
