"""Hand-built witnesses whose CIDs are CRAFTED against the engine's own hash: the CID index (K4
`k_index_insert`, probed by `witness_find` and its copies), the execution order's seen-set (`k_exec_insert`,
`k_exec_insert_flags`, `k_exec_first`, `exec_find`) and the arena layout under the index (`launch_k1_layout`).

The store never hashes on insert, `put_keyed` takes any CID and a bundle is untrusted input, so the keys of
these tables are the adversary's.  `cid_hash64` is `x = w0 ^ rotl(w1,13) ^ rotl(w2,27) ^ rotl(w3,41) ^ w4; y = x * MULT`
over the five little-endian words of the 40-byte slot; the multiplier is odd, so `x = y * MULT^-1 mod 2^64`, and word 1
(bytes 8-15) lies inside the digest of every CID form used here: `craft(y, salt)` solves it for ANY target y with every
other digest byte drawn from the salt.  Home slot = high word of y under the table's mask, fingerprint = low word.

    A_CASES[name]  the CID index:   Case(entries [(cid, block)], probes [cid], want [None | (block id, block)])
    B_CASES[name]  the seen-set:    callable() → Tipset(store, parts, raw, order, claims [(claim, status)])   (built once)
    C_AMT[name], C_HAMT[name], c_hamt_repointed(tree, mode, hops), c_written_receipts / c_written_hamt(mode)   walks over
                   crafted links: the named trees of
                   tests/amt_enum_cases.py and tests/hamt_get_cases.py RELABELLED onto one chain, with their literals
    D_CASES[name]  the block table: Blocks(blocks, data, off, lens, cids, status) — honest Blake2b CIDs, up to four flipped
    e_composite(kind, slot)   the claim set of the HAMT levels: every child's block id on one of its 512 homes

Every expected answer is written by plain Python next to the case: a `dict` filled in table order (the last insert wins),
`dict.fromkeys` over the raw positions (the first occurrence stays), `hashlib.blake2b`.  The property a case is named for
— homes, fingerprints, distinctness, chain length — is asserted HERE, on import."""
import collections
import functools
import hashlib
import random

import numpy as np

import event_chain_cases as ec
import ipc_filecoin_proofs_amd as ipcfp
import pyamt
from pyamt import array, bstr, uint

M64 = (1 << 64) - 1
MULT = 0x9E3779B97F4A7C15
MULT_INV = pow(MULT, -1, 1 << 64)
ROT = (0, 13, 27, 41, 0)  # rotation of each slot word before the xor
assert (MULT * MULT_INV) & M64 == 1


def rotl(v, r):
    return ((v << r) | (v >> (64 - r))) & M64 if r else v


def slot_of(cid: bytes) -> bytes:
    """the 40-byte slot of a binary CID: zero padded; longer than the slot: folded by the library (include/ipcfp.h)"""
    cid = bytes(cid)
    return cid.ljust(40, b"\0") if len(cid) <= 40 else ipcfp.cid_slot(cid).tobytes()


def words(slot40: bytes):
    assert len(slot40) == 40
    return [int.from_bytes(slot40[8 * j: 8 * j + 8], "little") for j in range(5)]


def cid_hash64(slot40: bytes) -> int:
    x = 0
    for w, r in zip(words(slot40), ROT):
        x ^= rotl(w, r)
    return (x * MULT) & M64


def h64(cid: bytes) -> int:
    return cid_hash64(slot_of(cid))


def home(cid: bytes, mask: int) -> int:
    return (h64(cid) >> 32) & mask


def fingerprint(cid: bytes) -> int:
    return h64(cid) & 0xFFFFFFFF


def table_mask(n: int) -> int:
    """the sizing rule of cid_index.hip, exec_state.h and shard_pull.cpp: 64 slots, doubled until load ≤ 0.5"""
    size = 64
    while size < 2 * n:
        size <<= 1
    return size - 1


# (prefix, CID length): word 1 — bytes 8..15 — lies inside the digest of each
FORMS = {"blake2b": (bytes.fromhex("0171a0e40220"), 38),   # CIDv1 dag-cbor blake2b-256
         "sha2": (bytes.fromhex("01711220"), 36),          # CIDv1 dag-cbor sha2-256
         "identity": (bytes.fromhex("0155000c"), 16)}      # CIDv1 raw identity, 12 bytes


def craft(y: int, salt, form="blake2b") -> bytes:
    """a CID of `form` whose slot hashes to exactly `y`; every byte but 8..15 comes from the salt"""
    prefix, n = FORMS[form]
    fill = hashlib.blake2b(repr((form, salt)).encode(), digest_size=40).digest()
    s = bytearray((prefix + fill[len(prefix): n]).ljust(40, b"\0"))
    s[8:16] = bytes(8)
    w = words(bytes(s))
    x = (y * MULT_INV) & M64
    for j in (0, 2, 3, 4):
        x ^= rotl(w[j], ROT[j])
    s[8:16] = rotl(x, 64 - ROT[1]).to_bytes(8, "little")
    cid = bytes(s[:n])
    assert cid_hash64(bytes(s)) == y and slot_of(cid) == bytes(s)
    return cid


# high words of y whose low 20 bits are all ones / all zeros / a constant: home = mask / 0 / fixed in EVERY table of up to
# 2^20 slots, so a case keeps its shape when its witness is merged into a larger one or grows by put_keyed
HOME_LAST, HOME_FIRST, HOME_MID = 0xA5FFFFFF, 0x3C700000, 0x5A512345
HOMES = {"last": HOME_LAST, "first": HOME_FIRST, "mid": HOME_MID}
EDGE_FINGERPRINTS = (0, 1, 0xFFFFFFFF, 0xDEADBEEF)


def target(hi: int, fp: int) -> int:
    return ((hi & 0xFFFFFFFF) << 32) | (fp & 0xFFFFFFFF)


def fp_of(salt) -> int:
    return int.from_bytes(hashlib.blake2b(repr(("fp", salt)).encode(), digest_size=4).digest(), "little")


def chain(hi, n, tag, form="blake2b"):
    """n distinct CIDs on the home that `hi` selects, fingerprints all different (the four edge ones first)"""
    fps = list(EDGE_FINGERPRINTS[:n])
    k = 0
    while len(fps) < n:
        f = fp_of((tag, k))
        k += 1
        if f not in fps[:4] and f not in fps[-64:]:
            fps.append(f)
    out = [craft(target(hi, f), (tag, i), form) for i, f in enumerate(fps)]
    assert len(set(out)) == n
    return out


# the check on import the issue names: 40 distinct CIDs per target for every home, fingerprint and mask
for _hi in (0, 1, 0xFFFFFFFE, 0xFFFFFFFF):
    for _fp in EDGE_FINGERPRINTS:
        _c = [craft(target(_hi, _fp), k, "sha2" if k % 3 == 2 else "blake2b") for k in range(40)]
        assert len(set(_c)) == 40 and {h64(c) for c in _c} == {target(_hi, _fp)}
        for _mask in (63, 127, 1023):
            assert {home(c, _mask) for c in _c} == {_hi & _mask} and {fingerprint(c) for c in _c} == {_fp}


class CraftedStore(pyamt.Store):
    """`put()` names each block from the supplied iterator of CIDs instead of hashing it: pyamt.build_amt, pyhamt and
    event_chain_cases.tipset then write trees whose LINKS are crafted (the store never hashes: SURVEY.md A.9)."""

    def __init__(self, names):
        super().__init__()
        self.names = iter(names)

    def put(self, block: bytes, sha256_cid: bool = False) -> bytes:
        c = next(self.names)
        assert c not in self.blocks
        self.blocks[c] = block
        return c


# ================================ A. the CID index ==============================================================================
Case = collections.namedtuple("Case", "entries probes want")
A_CASES = {}
A_META = {}  # name → {"n", "kind": "wrap" | "equal_hash" | …}
SIZES = (0, 1, 2, 31, 32, 33, 64, 65, 1023, 1024, 1025)


def folded(n: int) -> bytes:
    """a 70-byte CID (CIDv1 dag-cbor blake2b-512): longer than the slot, so the library folds it"""
    return bytes.fromhex("0171a0e40240") + hashlib.blake2b(b"a CID longer than the slot %d" % n).digest()


def block_of(tag: int) -> bytes:
    """an Amtv0 root of height 0 whose only value is uint(tag): `amt_get(cid, [0])` is a `get` the oracle answers too"""
    return array([uint(0), uint(1), array([bstr(b"\x01"), array([]), array([uint(tag)])])])


def value_of(block: bytes) -> bytes:
    """the value a block_of() holds at index 0"""
    assert block[:8] == bytes.fromhex("8300018341018081")
    return block[8:]


def a_case(name, cids, absent, kind, base=0):
    entries = [(c, block_of(base + i)) for i, c in enumerate(cids)]
    table = {}
    for i, (c, b) in enumerate(entries):
        table[c] = (i, b)  # the last insert wins
    present = list(table)
    assert not set(absent) & set(table) and len(set(absent)) == len(absent)
    probes = present + list(absent)
    A_CASES[name] = Case(entries, probes, [table.get(p) for p in probes])
    A_META[name] = {"n": len(cids), "kind": kind, "absent": len(absent)}


def run_from(h, n, mask):
    """the slots a chain of n keys on home h fills, whatever order they arrive in"""
    return [(h + k) & mask for k in range(n)]


def _one_home(n):
    mask = table_mask(n)
    for tag, hi in HOMES.items():
        cids = chain(hi, n, ("A", tag, n))
        assert {home(c, mask) for c in cids} <= {hi & mask} and len({fingerprint(c) for c in cids}) == n
        absent = []
        if n:
            absent.append(craft(h64(cids[0]), ("A absent same hash", tag, n)))            # full hash of the chain's head
            absent.append(craft(h64(cids[-1]), ("A absent same hash, sha2", tag, n), "sha2"))
            absent.append(craft(target(hi + n // 2, 7), ("A absent mid", tag, n)))          # home inside the cluster
            absent.append(craft(target(hi + n, 7), ("A absent past", tag, n)))              # home one past its end
            assert home(absent[2], mask) in run_from(hi & mask, n, mask) and home(absent[3], mask) == (hi + n) & mask
            assert home(absent[3], mask) not in run_from(hi & mask, n, mask)
        else:
            absent.append(craft(target(hi, 7), ("A absent, empty witness", tag)))
        if tag == "last" and n >= 2:
            assert run_from(hi & mask, n, mask)[:2] == [mask, 0]  # the chain wraps
        a_case(f"one_home_{tag}_{n}", cids, absent, "wrap" if tag == "last" and n >= 2 else "one_home")


def _one_hash(n):
    y = target(HOME_LAST - 1, 0xDEADBEEF)  # home mask-1: the run of n ≥ 3 equal hashes wraps as well
    cids = [craft(y, ("A one hash", n, i), "sha2" if i % 5 == 4 else "blake2b") for i in range(n)]
    assert len(set(cids)) == n and {h64(c) for c in cids} <= {y}
    absent = [craft(y, ("A one hash absent", n, k), f) for k, f in enumerate(("blake2b", "sha2", "identity"))]
    a_case(f"one_hash_{n}", cids, absent, "equal_hash" if n >= 2 else "one_home")


def _abut(n):
    """cluster 1 ends on the table's LAST slot, cluster 2 starts on slot 0: a probe that enters cluster 1 and is absent walks
    through the wrap and all of cluster 2 before it meets an empty slot"""
    mask = table_mask(n)
    n1 = (n + 1) // 2
    hi1 = HOME_LAST - (n1 - 1)
    c1, c2 = chain(hi1, n1, ("A abut 1", n)), chain(HOME_FIRST, n - n1, ("A abut 2", n))
    assert run_from(hi1 & mask, n1, mask)[-1] == mask and (not c2 or home(c2[0], mask) == 0)
    cids = [c for pair in zip(c1, c2 + [None]) for c in pair if c is not None]  # interleaved in table order
    assert sorted(cids) == sorted(c1 + c2)
    absent = [craft(target(hi1 + n1 // 2, 9), ("A abut absent", n)), craft(target(HOME_LAST, 9), ("A abut absent last", n)),
              craft(target(HOME_FIRST + (n - n1), 9), ("A abut absent past", n)), craft(h64(c1[0]), ("A abut absent same", n))]
    a_case(f"abut_{n}", cids, absent, "wrap")


def _dups(n):
    """k copies of ONE CID among n keys of one wrapping chain: the first copy is block 0 and the last is block n-1 — K4 takes
    the table from both ends at once — the others spread evenly; `has` names block n-1 and `get` returns ITS bytes"""
    for k in sorted({2, 3, 64, 257, n}):
        if k > n:
            continue
        others = chain(HOME_LAST - 2, n - k + 1, ("A dup", n, k))
        d, others = others[0], others[1:]
        at = sorted({(j * (n - 1)) // (k - 1) for j in range(k)})
        assert len(at) == k and at[0] == 0 and at[-1] == n - 1
        it = iter(others)
        cids = [d if i in at else next(it) for i in range(n)]
        assert cids.count(d) == k and len(set(cids)) == n - k + 1
        name = f"dup_{'all' if k == n else k}_of_{n}"
        a_case(name, cids, [craft(h64(d), ("A dup absent", n, k))], "dup")
        c = A_CASES[name]
        assert c.want[c.probes.index(d)] == (n - 1, block_of(n - 1))


def _forms(n):
    """one chain on the home of a FOLDED 70-byte CID (it cannot be crafted: it is simply there), the others crafted onto its
    home — one of each form onto its full 64-bit hash — as sha2-256, identity and blake2b CIDs in turn"""
    mask = table_mask(n)
    y = h64(folded(n))
    hi = y >> 32
    forms = ("blake2b", "sha2", "identity")
    cids = [folded(n)] + [craft(y if i < 4 else target(hi, fp_of(("A forms", n, i))), ("A forms", n, i), forms[i % 3]) for i in range(1, n)]
    assert len(set(cids)) == n and {home(c, mask) for c in cids} == {hi & mask}
    absent = [craft(y, ("A forms absent", n, f), f) for f in forms]
    # the same bytes under another LENGTH are another key only through the bytes: a 36-byte CID and the 38-byte one that
    # extends it by two zero bytes share a slot — the slot is the key (include/ipcfp.h), so no such pair is in a case
    a_case(f"forms_{n}", cids, absent, "forms")


def _one_bit_pairs(seed):
    """for each of the five words a present / absent pair that differs in ONE bit of that word only and shares a home in the
    64-slot table: a compare that drops the word answers the absent CID with the present one's block"""
    rng = random.Random(seed)
    free = {0: range(6 * 8, 8 * 8), 1: range(64), 2: range(64), 3: range(64), 4: range(0, 6 * 8)}  # bytes 6-7 … bytes 32-37
    pairs = []
    for j in range(5):
        for tries in range(1 << 16):
            p = pyamt.cid_of(b"one bit %d %d %d" % (seed, j, rng.getrandbits(32)))
            bit = rng.choice(list(free[j]))
            s = bytearray(slot_of(p))
            s[8 * j + bit // 8] ^= 1 << (bit % 8)
            q = bytes(s[:38])
            if home(p, 63) == home(q, 63):
                break
        wp, wq = words(slot_of(p)), words(slot_of(q))
        assert [a != b for a, b in zip(wp, wq)] == [k == j for k in range(5)] and bin(wp[j] ^ wq[j]).count("1") == 1
        assert home(p, 63) == home(q, 63) and p[:6] == q[:6] and len(q) == 38
        pairs.append((p, q))
    return pairs


def _one_bit_cases():
    pairs = _one_bit_pairs(2718)
    a_case("one_bit_5", [p for p, _ in pairs], [q for _, q in pairs], "one_bit")
    # … and once more with 26 others on the first pair's home, ahead of it in the table (still 64 slots)
    pairs = _one_bit_pairs(3141)
    filler = chain(home(pairs[0][0], 63), 26, "A one bit filler")
    assert {home(c, 63) for c in filler} == {home(pairs[0][0], 63)} and table_mask(31) == 63
    a_case("one_bit_in_a_chain_31", filler + [p for p, _ in pairs], [q for _, q in pairs], "one_bit")


for _n in SIZES:
    _one_home(_n)
    _one_hash(_n)
    if _n >= 2:
        _abut(_n)
        _dups(_n)
    if _n >= 5:
        _forms(_n)
_one_bit_cases()

assert {m["n"] for m in A_META.values()} >= set(SIZES)
assert table_mask(32) == 63 and table_mask(33) == 127 and table_mask(1024) == 2047 and table_mask(1025) == 4095
for _k in ("wrap", "equal_hash", "dup", "forms", "one_bit"):
    assert sum(1 for m in A_META.values() if m["kind"] == _k) >= 2, _k
assert {f"dup_{k}_of_1025" for k in (2, 3, 64, 257, "all")} <= set(A_CASES)


def tables_of(entries):
    """(data, off, lens, cids40) of [(cid, block)] laid back to back"""
    blocks = [b for _, b in entries]
    lens = np.array([len(b) for b in blocks], dtype=np.uint32)
    off = np.zeros(len(blocks), dtype=np.uint64)
    if len(blocks):
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()
    cids = ipcfp.cid_slots([c for c, _ in entries]) if entries else np.zeros((0, 40), np.uint8)
    return data, off, lens, cids


@functools.lru_cache(maxsize=None)
def a_merged():
    """every A case in ONE witness (a 32 k-slot table): each chain among the others' — the dict over ALL entries answers"""
    entries = [e for c in A_CASES.values() for e in c.entries]
    table = {}
    for i, (c, b) in enumerate(entries):
        table[c] = (i, b)
    probes = [p for c in A_CASES.values() for p in c.probes]
    return Case(entries, probes, [table.get(p) for p in probes])


# ================================ D. the block table ============================================================================
Blocks = collections.namedtuple("Blocks", "blocks data off lens cids status")
D_CASES = {}
EDGE_LENGTHS = (0, 1, 127, 128, 129, 32511, 32512, 32513, 32640, 32641, 65536, 70001)
COUNTS = (1, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097)
CLASS_CAP, SCATTER_TILE = 255, 4096


def chunk_class(n: int) -> int:
    return min(CLASS_CAP, 1 if n == 0 else (n + 127) // 128)


def _bytes(n: int, tag: int) -> bytes:
    return (hashlib.blake2b(b"block %d" % tag, digest_size=64).digest() * (n // 64 + 1))[:n]


def d_case(name, lengths, order="given", ragged=False):
    idx = list(range(len(lengths)))
    if order == "ascending":
        idx.sort(key=lambda i: lengths[i])
    elif order == "descending":
        idx.sort(key=lambda i: -lengths[i])
    elif order == "shuffled":
        random.Random(len(lengths)).shuffle(idx)
    blocks = [_bytes(lengths[i], i) for i in idx]
    n = len(blocks)
    lens = np.array([len(b) for b in blocks], dtype=np.uint32)
    # ragged: a gap of 1..7 bytes in front of every block and the blocks in REVERSE order inside the buffer
    gaps = [1 + (7 * i) % 7 for i in range(n)] if ragged else [0] * n
    place = list(reversed(range(n))) if ragged else list(range(n))
    off = np.zeros(n, dtype=np.uint64)
    parts, at = [], 0
    for i in place:
        parts.append(b"\xee" * gaps[i])
        off[i] = at + gaps[i]
        parts.append(blocks[i])
        at += gaps[i] + len(blocks[i])
    data = np.frombuffer(b"".join(parts) + b"\xee" * (3 if ragged else 0), dtype=np.uint8).copy()
    cids = np.zeros((n, 40), dtype=np.uint8)
    for i, b in enumerate(blocks):
        cids[i, :38] = np.frombuffer(pyamt.cid_of(b), dtype=np.uint8)
    # a flipped digest bit at both ends of the schedule (a longest and a shortest block) and of the table
    longest, shortest = max(range(n), key=lambda i: lens[i]), min(range(n), key=lambda i: lens[i])
    status = np.ones(n, dtype=np.uint8)
    for i, (byte, bit) in zip((longest, shortest, 0, n - 1), ((6, 0), (37, 7), (20, 3), (9, 5))):
        if status[i]:
            cids[i, byte] ^= 1 << bit
            status[i] = 0
    for i in range(n):  # the expectation itself: hashlib over the block's own bytes
        assert (hashlib.blake2b(blocks[i], digest_size=32).digest() == cids[i, 6:38].tobytes()) == bool(status[i])
        assert data[int(off[i]): int(off[i]) + int(lens[i])].tobytes() == blocks[i]
    D_CASES[name] = Blocks(blocks, data, off, lens, cids, status)


for _order in ("ascending", "descending", "shuffled"):
    for _ragged in (False, True):
        d_case(f"edges_{_order}_{'ragged' if _ragged else 'tight'}", list(EDGE_LENGTHS), _order, _ragged)
d_case("all_256_classes", [0] + [n for c in range(1, 256) for n in (128 * c - 1, 128 * c)] + [128 * 256 - 1, 128 * 256], "shuffled")
assert {chunk_class(int(n)) for n in D_CASES["all_256_classes"].lens} == set(range(1, 256))  # (class 0 is never used: an empty block is one chunk)
for _n in COUNTS:
    d_case(f"one_class_{_n}", [129 + (37 * i) % 128 for i in range(_n)], ragged=_n % 2 == 0)
    assert {chunk_class(int(n)) for n in D_CASES[f"one_class_{_n}"].lens} == {2}
    _r = random.Random(_n)
    d_case(f"mixed_{_n}", [_r.choice((0, 1, 127, 128, 129, 300, 640, 1000)) for _ in range(_n)], ragged=_n % 2 == 1)
assert {chunk_class(n) for n in EDGE_LENGTHS} == {1, 2, 254, 255} and chunk_class(32512) == 254 and chunk_class(32513) == 255
assert {SCATTER_TILE - 1, SCATTER_TILE, SCATTER_TILE + 1} <= set(COUNTS)


@functools.lru_cache(maxsize=None)
def d_merged():
    """every D case in ONE witness, back to back: some 25 k blocks of every class over seven scatter tiles.  The six `edges`
    tables hold the same twelve blocks (under CIDs that differ where a bit was flipped): duplicates, the last one answers."""
    cases = list(D_CASES.values())
    blocks = [b for d in cases for b in d.blocks]
    lens = np.array([len(b) for b in blocks], dtype=np.uint32)
    off = np.zeros(len(blocks), dtype=np.uint64)
    off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    data = np.frombuffer(b"".join(blocks), dtype=np.uint8).copy()
    assert len(blocks) > 6 * SCATTER_TILE and {chunk_class(int(n)) for n in lens} == set(range(1, 256))
    return Blocks(blocks, data, off, lens, np.concatenate([d.cids for d in cases]), np.concatenate([d.status for d in cases]))


# ================================ B. the seen-set ===============================================================================
Tipset = collections.namedtuple("Tipset", "store parts raw order claims")
B_CASES = {}
B_META = {}
RAW_COUNTS = (32, 33, 1024, 1025, 4097)
PARENTS = (1, 2, 5)


def spread(raw, n_parents):
    """the raw positions over n_parents blocks, each block's share cut 2:1 into bls and secp — in raw order"""
    out, n = [], len(raw)
    for k in range(n_parents):
        part = raw[n * k // n_parents: n * (k + 1) // n_parents]
        cut = (2 * len(part) + 2) // 3
        out.append((part[:cut], part[cut:]))
    assert [c for bls, secp in out for c in bls + secp] == list(raw)
    return out


def first_seen(raw):
    return list(dict.fromkeys(raw))


def claim_for(base, e, message, exec_index=None):
    """`base` re-pointed: message `message`, claimed at exec_index (default e), with the event receipt e holds"""
    c = dict(base)
    c.update(ec.log_fields(ec.good_event(2000 + e)))
    c.update(message_cid=ec.cid_str(message), exec_index=e if exec_index is None else exec_index, event_index=0)
    return c


def b_case(name, raw, n_parents, kind, absent=()):
    raw = list(raw)
    order = first_seen(raw)
    B_META[name] = {"raw": len(raw), "parents": n_parents, "kind": kind, "distinct": len(order)}

    @functools.lru_cache(maxsize=None)
    def build():
        store, base, parts = ec.tipset(msgs=spread(raw, n_parents), receipts="good", at=(0, 0))
        assert parts["order"] == order
        pos = {c: i for i, c in enumerate(order)}
        claims = [(base, 1)]
        # first occurrences: the first, the last, and one in the middle → TRUE
        for e in sorted({len(order) - 1, len(order) // 2}):
            claims.append((claim_for(base, e, order[e]), 1))
        first_at = {}
        for i, c in enumerate(raw):
            first_at.setdefault(c, i)
        dups = [i for i, c in enumerate(raw) if first_at[c] != i]
        for i in sorted(set(dups[:2] + dups[-2:])):
            e = pos[raw[i]]
            assert e < i
            claims.append((claim_for(base, e, raw[i], exec_index=i), 8))       # named at a LATER raw position
            claims.append((claim_for(base, e, raw[i]), 1))                     # … and where it was executed
            nxt = next((c for c in raw[i + 1:] if first_at[c] > i), None)      # the message executed behind the duplicate
            if nxt is not None:
                claims.append((claim_for(base, pos[nxt], nxt), 1))
        for c in absent:  # absent, colliding in full with a present one → not executed
            assert c not in pos
            claims.append((claim_for(base, 0, c), 7))
        return Tipset(store, parts, raw, order, claims)

    B_CASES[name] = build


def _b_family(n, n_parents, kind):
    tag = ("B", kind, n)
    mask = table_mask(n)
    if kind in HOMES:
        raw = chain(HOMES[kind], n, tag)
        assert {home(c, mask) for c in raw} == {HOMES[kind] & mask} and len({fingerprint(c) for c in raw}) == n
        absent = [craft(h64(raw[0]), (tag, "absent")), craft(h64(raw[-1]), (tag, "absent 2"), "sha2")]
    elif kind == "one_hash":
        y = target(HOME_LAST - 3, 0xFFFFFFFF)
        raw = [craft(y, (tag, i)) for i in range(n)]
        assert len(set(raw)) == n and {h64(c) for c in raw} == {y}
        absent = [craft(y, (tag, "absent"))]
    elif kind == "equal_fp_neighbours":
        # ONE fingerprint on a run of neighbouring homes that crosses the wrap, four keys to a home
        raw = [craft(target(HOME_LAST - 2 + i // 4, 0), (tag, i)) for i in range(n)]
        assert len(set(raw)) == n and {fingerprint(c) for c in raw} == {0} and len({home(c, mask) for c in raw}) == (n + 3) // 4
        absent = [craft(h64(raw[n // 2]), (tag, "absent"))]
    elif kind == "dups":
        # colliding CIDs, a quarter of the raw positions copies: behind every third distinct CID d[i] stands a copy of
        # d[i // 2] — next to its original at the head of the list, ever farther behind it later on, so across bls / secp
        # and across parents — and the LAST distinct CID is first seen at n-2 with its copy at n-1, in the last wavefront
        m = n // 4
        d = chain(HOME_LAST - 1, n - m, tag)
        raw, copies = [], 0
        for i, c in enumerate(d):
            raw.append(c)
            if i % 3 == 0 and copies < m - 1 and i < len(d) - 1:
                raw.append(d[i // 2])
                copies += 1
        raw.append(d[-1])
        assert len(raw) == n and raw[0] == raw[1] and raw.index(d[-1]) == n - 2 and first_seen(raw) == d
        absent = [craft(h64(d[0]), (tag, "absent"))]
    elif kind == "one_cid":
        raw = [craft(target(HOME_LAST, 1), tag)] * n
        absent = [craft(target(HOME_LAST, 1), (tag, "absent"))]
    b_case(f"{kind}_{n}_over_{n_parents}", raw, n_parents, kind, absent)


B_KINDS = ("last", "first", "mid", "one_hash", "equal_fp_neighbours", "dups", "one_cid")
for _i, _n in enumerate(RAW_COUNTS):
    for _j, _kind in enumerate(B_KINDS):
        _b_family(_n, PARENTS[(_i + _j) % 3], _kind)
def one_word_twin(cid, j, start=1):
    """a CID of the same length that differs from `cid` in slot word j ONLY and keeps its fingerprint and its home in every
    table of up to 2^12 slots.  The two hashes must differ (the mix is a bijection of the xor of the rotated words), so the
    difference is put where neither the home nor the fingerprint looks: y' = y ^ (k << 44).  Word 4 has 48 free bits (bytes
    32-37): k is searched until the word's difference fits them; word 0 has 16 (bytes 6-7), which no k of 20 bits reaches."""
    s = bytearray(slot_of(cid))
    w, y = words(bytes(s)), h64(cid)
    for k in range(start, 1 << 20):
        d = rotl(((y * MULT_INV) ^ ((y ^ (k << 44)) * MULT_INV)) & M64, (64 - ROT[j]) % 64)
        if j != 4 or d < 1 << 48:
            break
    s[8 * j: 8 * j + 8] = (w[j] ^ d).to_bytes(8, "little")
    q = bytes(s[: len(cid)])
    assert h64(q) == y ^ (k << 44) and fingerprint(q) == fingerprint(cid) and home(q, 4095) == home(cid, 4095)
    assert [a != b for a, b in zip(words(slot_of(q)), w)] == [i == j for i in range(5)]
    return q


# the compare behind a fingerprint match, word by word: P and for each of the words 1-4 a twin that differs in that word only,
# same fingerprint, same home — four of them PRESENT beside P (a compare that drops the word merges the two positions), four
# more ABSENT (it would find them executed), all inside one colliding chain of 33 raw positions
_TW = chain(HOME_LAST - 1, 26, "B twins")
_TWP = [one_word_twin(_TW[5], j) for j in (1, 2, 3, 4)]
_TWA = [one_word_twin(_TW[5], j, start=1 << 19) for j in (1, 2, 3, 4)]  # (other twins of the same CID)
assert len(set(_TW + _TWP + _TWA)) == 34 and {fingerprint(c) for c in _TWP + _TWA} == {fingerprint(_TW[5])}
b_case("one_word_twins_33", _TW[:13] + _TWP[:2] + _TW[13:] + _TWP[2:] + [_TW[5], _TWP[0], _TWP[3]], 2, "twins", _TWA)

# three small cases whose execution order is written out: `seen.insert` keeps the FIRST raw position — a copy inside a
# list, in the secp list of the same block, and in a later parent; one copy stands last, behind a first occurrence at n-2
_P = chain(HOME_LAST, 6, "B literal")
b_case("literal_dups_within_a_list", [_P[0], _P[1], _P[0], _P[2], _P[2], _P[3]] + _P[4:] + [_P[5], _P[0]], 1, "dups", [craft(h64(_P[0]), "B literal absent")])
b_case("literal_dups_across_bls_and_secp", _P[:4] + [_P[1], _P[4], _P[0], _P[5], _P[4]], 1, "dups", [craft(h64(_P[4]), "B literal absent 2")])
b_case("literal_dups_across_parents", _P[:3] + [_P[0], _P[3], _P[4]] + [_P[4], _P[2], _P[5], _P[5]], 3, "dups", [craft(h64(_P[5]), "B literal absent 3")])
assert first_seen([_P[0], _P[1], _P[0], _P[2], _P[2], _P[3]] + _P[4:] + [_P[5], _P[0]]) == _P
assert first_seen(_P[:4] + [_P[1], _P[4], _P[0], _P[5], _P[4]]) == _P and first_seen(_P[:3] + [_P[0], _P[3], _P[4]] + [_P[4], _P[2], _P[5], _P[5]]) == _P

for _name, _m in B_META.items():
    if _m["kind"] == "dups":
        assert _m["distinct"] < _m["raw"], _name
    if _m["kind"] == "one_cid":
        assert _m["distinct"] == 1
assert {(m["raw"], m["parents"]) for m in B_META.values()} >= {(n, p) for n in RAW_COUNTS for p in PARENTS}
assert {m["parents"] for m in B_META.values() if m["kind"] == "one_hash"} == set(PARENTS)


# ================================ C. walks over crafted links ===================================================================
# The named trees of tests/amt_enum_cases.py and tests/hamt_get_cases.py, RELABELLED: every block gets a crafted name and
# every link to it is rewritten (a link carries the CID's bytes verbatim, at the same length), so the literals written next
# to those cases hold unchanged while every `Blockstore::get` of the walk probes one chain.  A TxMeta block is the one block
# the verifier hashes again (`put_cbor(&(bls, secp))`, verifier.rs:64-72): it keeps an honest name — of its REWRITTEN bytes.
import re  # noqa: E402

import amt_enum_cases as ae  # noqa: E402
import hamt_get_cases as hg  # noqa: E402

_CID_RE = re.compile(rb"\x01\x71(?:\xa0\xe4\x02\x20.{32}|\x12\x20.{32})", re.S)
MODES = {"wrap": lambda tag: (lambda i: target(HOME_LAST - 4, fp_of((tag, i)))),      # one home, the chain wraps
         "one_hash": lambda tag: (lambda i: target(HOME_LAST - 4, 0x5EED5EED))}      # one 64-bit hash for every block


def relabel(blocks, mode, tag, honest=()):
    """{cid: block} → ({new cid: rewritten block} in the same order, {old cid: new cid})"""
    y_of = MODES[mode](tag)
    ren = {}
    for i, c in enumerate(blocks):
        if c not in honest and len(c) in (36, 38):
            ren[c] = craft(y_of(i), (tag, mode, i), "blake2b" if len(c) == 38 else "sha2")

    def rewrite(b):
        return _CID_RE.sub(lambda m: ren.get(m.group(0), m.group(0)), b)

    for c in honest:
        ren[c] = pyamt.cid_of(rewrite(blocks[c]))
    out = {ren.get(c, c): rewrite(b) for c, b in blocks.items()}
    assert len(out) == len(blocks) and all(len(out[ren.get(c, c)]) == len(b) for c, b in blocks.items())
    crafted = [ren[c] for c in blocks if c in ren and c not in honest]
    assert len({home(c, table_mask(len(blocks))) for c in crafted}) == 1 and (mode != "one_hash" or len({h64(c) for c in crafted}) == 1)
    return out, ren


def same_hash_absent(cid, tag):
    """a CID of the same form and the same 64-bit hash as `cid` that no store holds"""
    return craft(h64(cid), ("absent twin", tag), "blake2b" if len(cid) == 38 else "sha2")


C_AMT_SHAPES = {"size_513": "the dense plan takes it: four levels of receipts and of messages",
                "roots_33_parents_duplicate_across_the_first_and_the_last": "33 parents: one more than the dense walk's root table holds"}
C_AMT = {}  # name → callable() → (Case with the literals, Built)


# a re-pointed variant per tree: the FIRST link of the named block → an absent CID of the present child's full 64-bit hash.
# (shape, which) → (the literals that change: the rest of the case stands)
_N33 = "roots_33_parents_duplicate_across_the_first_and_the_last"
C_AMT_REPOINTS = {
    # receipts 0..511 of 513 are behind the missing block
    ("size_513", "receipts"): dict(scan=(65,), claims=[("under_the_repointed_link", ae.at(0), 65), ("under_it_as_well", ae.at(511), 65),
                                                        ("beside_it", ae.at(512), 1), ("not_executed", {"e": 513, "msg": ae.OTHER}, 7)]),
    # messages 0..511 of the one BLS list: `reconstruct_execution_order` itself is the Err, whatever the claim names
    ("size_513", "messages"): dict(order=(65,), claims=[("first", ae.at(0), 65), ("beside_the_link", ae.at(512), 65),
                                                        ("not_executed", {"e": 513, "msg": ae.OTHER}, 65)]),
    # 353 receipts: the root's first link covers 0..63
    (_N33, "receipts"): dict(scan=(65,), claims=[("under_the_repointed_link", ae.at(0), 65), ("under_it_as_well", ae.at(63), 65), ("beside_it", ae.at(64), 1),
                                                 ("the_duplicate_in_the_last_parent", {"e": 353, "msg": 0}, 8), ("last", {"e": 352, "msg": 1317}, 1)]),
    # the first parent's BLS list of 65: its root's first link covers 0..63
    (_N33, "messages"): dict(order=(65,), claims=[("first", ae.at(0), 65), ("the_duplicate_in_the_last_parent", {"e": 353, "msg": 0}, 65),
                                                  ("last", {"e": 352, "msg": 1317}, 65)]),
}


def _c_amt(shape, mode, repoint=None):
    name = f"{shape}__{mode}" + (f"__{repoint}_link_repointed" if repoint else "")

    @functools.lru_cache(maxsize=None)
    def build():
        c0, b0 = ae.CASES[shape], ae.build(shape)
        blocks = dict(b0.store.blocks)
        out, ren = relabel(blocks, mode, ("C", shape), honest=b0.parts["txmeta"])
        parts = {"parents": [ren[p] for p in b0.parts["parents"]], "txmeta": [ren[t] for t in b0.parts["txmeta"]],
                 "receipts": ren[b0.parts["receipts"]], "child": ren[b0.parts["child"]],
                 "lists": [(ren[bls], ren[secp]) for bls, secp in b0.parts["lists"]]}
        c = ae.Case()
        for f in ae.Case.__slots__:
            setattr(c, f, getattr(c0, f))
        c.name, claims = name, list(c0.claims)
        if repoint:
            at = parts["receipts"] if repoint == "receipts" else parts["lists"][0][0]
            kid = next(m.group(0) for m in _CID_RE.finditer(out[at]) if m.group(0) in out)
            twin = same_hash_absent(kid, name)
            assert out[at].count(kid) == 1 and twin not in out and h64(twin) == h64(kid)
            out[at] = out[at].replace(kid, twin)
            lit = C_AMT_REPOINTS[(shape, repoint)]
            c.scan, c.order, c.walks, claims = lit.get("scan", c0.scan), lit.get("order", c0.order), None, lit["claims"]
        st = pyamt.Store()
        st.blocks = out
        b = ae.Built()
        b.store, b.parts, b.where = st, parts, {k: ren.get(v, v) for k, v in b0.where.items()}
        b.claims = [(t, ae.claim_of(parts, **spec), s) for t, spec, s in claims]
        return c, b

    C_AMT[name] = build


for _shape in C_AMT_SHAPES:
    for _mode in MODES:
        _c_amt(_shape, _mode)
for (_shape, _which) in C_AMT_REPOINTS:
    for _mode in MODES:
        _c_amt(_shape, _mode, _which)

WRITTEN_N = 600  # 600 receipts: an Amtv0 of height 3 — four levels


@functools.lru_cache(maxsize=None)
def c_written_receipts(mode):
    """a receipts tree WRITTEN through CraftedStore — pyamt.build_amt names every node from the crafted iterator as it links
    it → (store, root, {index: receipt bytes}); every receipt names one events root with the one matching event"""
    import itertools

    y_of = MODES[mode](("C written", WRITTEN_N))
    st = CraftedStore(craft(y_of(i), ("C written", mode, i)) for i in itertools.count())
    ev_root = ec.events_root(st, {0: ae.EVENT})
    items = {i: pyamt.receipt(gas=1000 + i, events_root=ev_root) for i in range(WRITTEN_N)}
    root = pyamt.build_amt(st, items, version=0)
    assert len(st.blocks) == 1 + 75 + 10 + 2 + 1 and len({home(c, table_mask(len(st.blocks))) for c in st.blocks}) == 1
    return st, root, items


WRITTEN_KEYS = 4000  # bit width 5, buckets of 3: 32 children, some 550 grandchildren — three levels


@functools.lru_cache(maxsize=None)
def c_written_hamt(mode):
    """a HAMT WRITTEN through CraftedStore by tests/pyhamt.py → HamtCase: every present key is TRUE with the value written,
    four absent keys are NOT_FOUND (32)"""
    import itertools

    import pyhamt

    y_of = MODES[mode](("C written hamt", WRITTEN_KEYS))
    st = CraftedStore(craft(y_of(i), ("C written hamt", mode, i)) for i in itertools.count())
    keys = [b"\x00" + uint(1000 + i)[0:9] + bytes([i & 0xFF, i >> 8]) for i in range(WRITTEN_KEYS)]
    items = {k: array([uint(i), bstr(bytes([i & 0xFF]) * (i % 7))]) for i, k in enumerate(keys)}
    root = pyhamt.build_hamt(st, items, bit_width=5)
    assert len(st.blocks) > 1 + 32 + 500 and len({home(c, table_mask(len(st.blocks))) for c in st.blocks}) == 1  # (three levels)
    absent = [b"nope", b"", b"\x00\xff\xff", keys[0] + b"\x00"]
    probe = keys[::3] + absent
    return HamtCase(st, root, 5, "any", probe, [hg.TRUE] * len(keys[::3]) + [32] * len(absent), [items[k] for k in keys[::3]])


# HAMTs: the 32-child composites (a state-tree-shaped root over bucket nodes of every size class), a node of 33 pointers, a
# chain of 52 link nodes and a bucket node as the 51st node (both deeper than three levels)
C_HAMT_SHAPES = ("width6_33_pointers__actor_state", "width5_chain_of_52_link_nodes__actor_state", "width5_bucket_node_as_the_51st_node__actor_state",
                 "width5_32_pointers_all_links__any")
HamtCase = collections.namedtuple("HamtCase", "store root bw kind keys want values")
C_HAMT = {}


def _c_hamt(name, mode, get):
    @functools.lru_cache(maxsize=None)
    def build():
        store, root, bw, kind, keys, want, values = get()
        out, ren = relabel(dict(store.blocks), mode, ("C hamt", name))
        st = pyamt.Store()
        st.blocks = out
        return HamtCase(st, ren[root], bw, kind, keys, want, values)

    C_HAMT[f"{name}__{mode}"] = build


def _composite(kind):
    def get():
        st, root, keys, want, values, child, _lens = hg.COMPOSITE[kind]
        return st, root, 5, kind, keys, want, values
    return get


def _named(name):
    def get():
        c = hg.CASES[name]
        return c.store, c.root, c.bw, c.kind, c.keys, c.want, c.values
    return get


for _mode in MODES:
    for _kind in sorted(hg.COMPOSITE):
        _c_hamt(f"composite_{_kind}", _mode, _composite(_kind))
    for _name in C_HAMT_SHAPES:
        _c_hamt(_name, _mode, _named(_name))


# (tree, number of link hops from the root to the node whose first link is re-pointed)
C_HAMT_REPOINTS = (("composite_actor_state", 0), ("composite_any", 0), ("width6_33_pointers__actor_state", 0),
                   ("width5_chain_of_52_link_nodes__actor_state", 3))


def _hamt_source(tree):
    return (_composite(tree[len("composite_"):]) if tree.startswith("composite_") else _named(tree))()


@functools.lru_cache(maxsize=None)
def c_hamt_repointed(tree, mode, hops=0):
    """the tree with one link — the first of the node `hops` links below the root — re-pointed to an absent CID of the present
    child's full hash → (HamtCase with the literals: 65 under the link, the honest case's beside it; number of keys under it)"""
    st, root, bw, kind, keys, want, values = _hamt_source(tree)
    out, ren = relabel(dict(st.blocks), mode, ("C hamt", tree))
    back = {v: k for k, v in ren.items()}
    node = ren[root]
    for _ in range(hops):
        node = next(m.group(0) for m in _CID_RE.finditer(out[node]) if m.group(0) in out)
    kid = next(m.group(0) for m in _CID_RE.finditer(out[node]) if m.group(0) in out)
    twin = same_hash_absent(kid, (tree, mode))
    under = _keys_under(tree, back[kid])
    assert under and (len(under) < len(keys) // 8 or len(keys) < 64)
    it = iter(values)
    new_want, new_values = [], []
    for i, s in enumerate(want):
        v = next(it) if s == hg.TRUE else None
        if i in under:
            new_want.append(65)
        else:
            new_want.append(s)
            if v is not None:
                new_values.append(v)
    # (a node of the 52-node chain names its one child in all 32 slots: every one of them is re-pointed)
    assert out[node].count(kid) in (1, 32) and twin not in out
    out[node] = out[node].replace(kid, twin)
    store = pyamt.Store()
    store.blocks = out
    return HamtCase(store, ren[root], bw, kind, keys, new_want, new_values), len(under)


@functools.lru_cache(maxsize=None)
def _keys_under(tree, kid):
    """indices of the tree's keys whose walk enters block `kid`: those whose answer changes to 65 when the block is taken
    away (tests/pystorage.py is the judge of that, on the HONEST tree — the relabelled one is then held to the same set)"""
    import pystorage

    store, root, bw, kind, keys = _hamt_source(tree)[:5]
    blocks = dict(store.blocks)
    del blocks[kid]
    check = {"actor_state": pystorage.check_actor_state, "vec_u8": pystorage.check_vec_u8, "any": lambda x: x}[kind]

    def status(blk, k):
        try:
            pystorage.hamt_get_bytes(blk, root, bw, k, check)
            return 1
        except pystorage.Err as e:
            return e.status

    return frozenset(i for i, k in enumerate(keys) if status(blocks, k) == 65 and status(store.blocks, k) != 65)


# ================================ E. the claim set of the HAMT levels ===========================================================
CLAIM_SET, CLAIM_MULT, CLAIM_SHIFT = 512, 2654435761, 23


def claim_home(block_id: int) -> int:
    return ((block_id * CLAIM_MULT) & 0xFFFFFFFF) >> CLAIM_SHIFT


@functools.lru_cache(maxsize=None)
def e_composite(kind, slot):
    """the 32-child composite of hamt_get_cases in a witness table laid out with filler blocks so that ALL children's block
    ids share home `slot` of the 512-slot claim set (slot 511: the chain of 32 wraps) → (HamtCase, [children's block ids])"""
    st, root, keys, want, values, child, _lens = hg.COMPOSITE[kind]
    cids = list(st.blocks)
    kids = sorted((c for c in cids if c != root and c in st.blocks[root]), key=st.blocks[root].index)  # in link order
    assert len(kids) == 32 - list(_lens).count(None) >= 31, len(kids)  # (one child of the composite is a link to a block nobody holds)
    ids, i = [], 0
    while len(ids) < len(kids):
        if claim_home(i) == slot:
            ids.append(i)
        i += 1
    rest = [c for c in cids if c not in kids]
    table, place = {}, dict(zip(ids, kids))
    it = iter(rest)
    for pos in range(ids[-1] + 1 + len(rest)):
        if pos in place:
            c = place[pos]
            table[c] = st.blocks[c]
        else:
            c = next(it, None) if pos > ids[-1] or pos % 97 == 5 else None
            if c is None:
                f = b"\x82\x19" + pos.to_bytes(2, "big") + b"\x40"  # a filler: [pos, h'']
                table[pyamt.cid_of(f)] = f
            else:
                table[c] = st.blocks[c]
    for c in it:
        table[c] = st.blocks[c]
    order = list(table)
    got = [order.index(c) for c in kids]
    assert got == ids and {claim_home(b) for b in got} == {slot} and set(cids) <= set(table)
    store = pyamt.Store()
    store.blocks = table
    return HamtCase(store, root, 5, kind, keys, want, values), got
