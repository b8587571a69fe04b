"""Hand-built HAMT nodes for the get primitives `ipcfp_hamt_get` / `ipcfp_hamt_get_device`, one NAMED case per limit a
fast route of the engine has (kernels/hamt_table.h, hamt_levels.hip, walk_dev.h): name → Case(store, root CID, bit
width, value kind, [keys], [expected status per key], [expected value bytes per TRUE key]).  The expected status is a
LITERAL written down from the reference's Rust — `Hamt::load_with_bit_width(root, store, bw)?.get(key)?`,
src/proofs/common/decode.rs:29-39, src/proofs/storage/decode.rs:79-96 — and SURVEY.md A.6; tests/pystorage.py
(`hamt_get_bytes`, an independent restatement) and the oracle must reproduce every literal and every value
(tests/test_hamt_get_cases.py), and every route of the engine must give them too (tests/test_gpu_hamt_get_cases.py).

A case breaks or stresses ONE thing; a case at a limit has its neighbour on the other side.  Every fast route promises
to describe a node exactly or to leave it to the walker, so the answer never depends on the limit — only on the Rust.
The limits themselves stand below as literals (LIMITS); the CPU test reads the engine's constants out of its source and
fails when they no longer match, so that a retuning moves the cases with it.

Where an answer rests on fvm_ipld_hamt's or serde's internals the case is in tests/assumption_cases.py HAMT_GET_CASES
(under one of pystorage's four named assumptions, or the accepted non-minimal head) and runs in this table too.

Statuses (include/ipcfp.h): 1 TRUE · 32 NOT_FOUND · 65 block missing · 66 decode · 70 HAMT max depth."""
import collections
import hashlib

import pyamt
import pyhamt
from pyamt import NULL, array, bstr, head, link, uint
from storage_chain_cases import bucket, cmap, node, text, vec

TRUE, NOT_FOUND, MISSING, DECODE, MAX_DEPTH = 1, 32, 65, 66, 70
KINDS = ("actor_state", "vec_u8", "any")

# what the engine's fast routes are built around today — literals of THIS file, compared with the source by the limit guard
LIMITS = {
    "table_pointers": 32,                 # HamtNodeRec: np and ptr_off[32]
    "bitfield_bits": 64,                  # HamtNodeRec.bitfield
    "tab_entries": 96,                    # HamtEntryTab.e[96]
    "stage_bytes": (1536, 4352, 6912),    # a node is staged when len + 24 <= stage
    "stage_entries": (24, 64, 96),
    "outline_min_len": 2048,
    "levels_switch": 1024,                # queries from which the default route goes level by level
    "offset_bits": 16,                    # ptr_off, key_off, val_off, val_len
    "key_len_bits": 8,                    # HamtEntryTab.Entry.key_len
}
STAGE_SLACK = 24
BLOCK_LENGTHS = (1511, 1512, 1513, 4327, 4328, 4329, 6887, 6888, 6889, 2047, 2048, 7500)
ENTRY_TOTALS = (24, 25, 64, 65, 96)       # (97 needs an over-full bucket: tests/assumption_cases.py)
KEY_LENGTHS = (0, 1, 7, 8, 9, 23, 24, 255, 256, 300)

Case = collections.namedtuple("Case", "store root bw kind keys want values")
CASES = {}  # name → Case
META = {}   # name → {"group", "limit": (what, n) | None, "lens": lengths of the blocks the case is about, …}


# ---- keys by the path their hash takes -------------------------------------------------------------------------------
_POOL = {}  # (bw, depth) → [next candidate number, {path: [keys]}]


def key_with_indices(path, bw, k=0) -> bytes:
    """the k-th key whose first len(path) child indices at bit width `bw` are `path` (a search over SHA-256: keep
    bw · len(path) below about 16 bits)"""
    path = tuple(path)
    pool = _POOL.setdefault((bw, len(path)), [0, {}])
    mask, depth = (1 << bw) - 1, len(path)
    while len(pool[1].get(path, ())) <= k:
        key = b"q%d.%d.%d" % (bw, depth, pool[0])  # (a pool of its own per width and depth: no key comes up twice)
        pool[0] += 1
        h = int.from_bytes(hashlib.sha256(key).digest(), "big") >> (256 - bw * depth) if depth else 0
        pool[1].setdefault(tuple((h >> (bw * (depth - 1 - d))) & mask for d in range(depth)), []).append(key)
    return pool[1][path][k]


def K(prefix, j, k=0, bw=5) -> bytes:
    return key_with_indices(tuple(prefix) + (j,), bw, k)


def pick(prefix, n, bw=5):
    """n keys under `prefix` whose NEXT indices differ pairwise, as the search meets them → [(next index, key)]"""
    out, seen, k = [], set(), 0
    while len(out) < n:
        key = key_with_indices(prefix, bw, k)
        k += 1
        j = pyhamt.index_at(key, len(prefix), bw)
        if j not in seen:
            seen.add(j)
            out.append((j, key))
    return out


# ---- values ------------------------------------------------------------------------------------------------------------
def vi(key: bytes) -> int:
    return int.from_bytes(hashlib.sha256(b"v" + key).digest()[:2], "big")


def astate(i, bal=b"\x00\x05", adr=NULL, seq=None, state=None, code=None):
    """fvm_shared ActorState `[code, state, sequence, balance, delegated_address]`"""
    return array([code or link(pyamt.cid_of(b"code%d" % (i % 5))), state or link(pyamt.cid_of(b"state%d" % i)),
                  seq or uint([0, 7, 23, 24, 255, 256, 70000, 1 << 33][i % 8]), bstr(bal), adr])


def val(kind, key) -> bytes:
    i = vi(key)
    if kind == "actor_state":
        return astate(i)
    if kind == "vec_u8":
        return vec(bytes([i & 0xFF, 0x18, i >> 8][: 1 + i % 3]))
    return [uint(i), bstr(b"any%d" % i), array([uint(i), NULL, text("x")]), astate(i), cmap([("k", uint(i))])][i % 5]


def long_cid(seed: bytes) -> bytes:
    """CIDv1, dag-cbor, blake2b-512: 70 bytes — longer than the engine's 40-byte slot, it crosses the ABI folded"""
    return bytes.fromhex("0171c0e40240") + hashlib.blake2b(seed, digest_size=64).digest()


def sha_cid(seed: bytes) -> bytes:
    return bytes.fromhex("01711220") + hashlib.sha256(seed).digest()


def put(st, block, how="std"):
    if how == "long":
        c = long_cid(block)
        st.blocks[c] = block
        return c
    return st.put(block, sha256_cid=(how == "sha"))


def absent_cid(tag, how="std"):
    seed = b"a block no witness holds: " + tag
    return {"std": pyamt.cid_of, "sha": sha_cid, "long": long_cid}[how](seed)


# ---- nodes -------------------------------------------------------------------------------------------------------------
def raw_node(bitfield_bytes: bytes, pointers) -> bytes:
    return array([bstr(bitfield_bytes), array(pointers)])


def build_node(at: dict) -> bytes:
    """{child index: encoded pointer} → the node"""
    bf = 0
    for j in at:
        bf |= 1 << j
    return node(bf, [at[j] for j in sorted(at)])


def leaf_for(key, value, depth, bw=5) -> bytes:
    """a node at `depth` that holds the one pair in the bucket the key's hash names"""
    return build_node({pyhamt.index_at(key, depth, bw): bucket([(key, value)])})


def plant(st, cid, prefix, bw=5):
    """`cid` hung under single-link nodes along `prefix` → the root CID"""
    for j in reversed(prefix):
        cid = st.put(build_node({j: link(cid)}))
    return cid


def add(name, kind, bw, st, root, probes, group, limit=None, **meta):
    name = f"{name}__{kind}"
    assert name not in CASES, name
    keys = [p[0] for p in probes]
    assert len(set(keys)) == len(keys), name
    assert all((p[1] == TRUE) == (p[2] is not None) for p in probes), name
    CASES[name] = Case(st, root, bw, kind, keys, [p[1] for p in probes], [p[2] for p in probes if p[1] == TRUE])
    META[name] = {"group": group, "limit": limit, **meta}


PREFIX = {0: (), 1: (7,), 3: (7, 11, 2)}


def at_levels(name, builder, group, kinds=KINDS, levels=(0, 1, 3), limit=None, **meta):
    """builder(store, kind, prefix) → (CID of the node — stored or not —, probes, status of any other key by next index)"""
    for kind in kinds:
        for lv in levels:
            st = pyamt.Store()
            cid, probes, _ = builder(st, kind, PREFIX[lv])
            add(f"{name}_level{lv}" if len(levels) > 1 else name, kind, 5, st, plant(st, cid, PREFIX[lv]), probes, group, limit,
                level=lv, **meta)


# ===== pointers and bitfield ==============================================================================================
def _pointers_and_bitfield():
    G = "pointers"
    for kind in KINDS:
        # width 5, all 32 pointers: buckets, links, mixed
        for shape in ("buckets", "links", "mixed"):
            st, at, probes = pyamt.Store(), {}, []
            for j in range(32):
                key = K((), j)
                v = val(kind, key)
                if shape == "buckets" or (shape == "mixed" and j % 2 == 0):
                    at[j] = bucket([(key, v)])
                else:
                    at[j] = link(st.put(leaf_for(key, v, 1)))
                probes.append((key, TRUE, v))
            probes.append((K((), 0, 1), NOT_FOUND, None))
            probes.append((K((), 31, 1), NOT_FOUND, None))
            add(f"width5_32_pointers_all_{shape}", kind, 5, st, st.put(build_node(at)), probes, G, ("pointers", 32))
        # width 6: 32 pointers, then 33 — the 33rd has no place in a record of 32
        for n in (32, 33):
            st, at, probes = pyamt.Store(), {}, []
            for j in range(n):
                key = K((), j, bw=6)
                v = val(kind, key)
                at[j] = bucket([(key, v)]) if j % 3 else link(st.put(leaf_for(key, v, 1, 6)))
                probes.append((key, TRUE, v))
            probes.append((K((), 40, bw=6), NOT_FOUND, None))
            add(f"width6_{n}_pointers", kind, 6, st, st.put(build_node(at)), probes, G, ("pointers", n))
        # the highest bit of a 64-bit bitfield, and the first one past it (9 bitfield bytes).  Bit 9 is a link to a block no
        # witness holds: a key on bit 9 is MISSING, and a key on bit 73, 137 or 201 — the same bit of a 64-bit word shifted
        # modulo 64 — stands on a clear bit.
        for bw, top, tag in ((6, 63, "width6_bit_63_8_byte_bitfield"), (7, 63, "width7_bit_63_8_byte_bitfield"),
                             (8, 63, "width8_bit_63_8_byte_bitfield"),
                             (7, 64, "width7_bit_64_9_byte_bitfield"), (8, 255, "width8_bit_255_32_byte_bitfield")):
            st = pyamt.Store()
            ka, kb, kc = K((), top, bw=bw), K((), 3, bw=bw), K((), 5, bw=bw)
            va, vb = val(kind, ka), val(kind, kb)
            blk = build_node({top: bucket([(ka, va)]), 3: link(st.put(leaf_for(kb, vb, 1, bw))), 9: link(absent_cid(b"behind bit 9"))})
            assert len(bitfield_of(blk)) == top // 8 + 1
            probes = [(ka, TRUE, va), (kb, TRUE, vb), (kc, NOT_FOUND, None), (K((), top, 1, bw=bw), NOT_FOUND, None), (K((), 9, bw=bw), MISSING, None)]
            probes += [(K((), j, bw=bw), NOT_FOUND, None) for j in (64 + 9, 128 + 9, 192 + 9, 64 + 3, 64 + 63) if j < 1 << bw and j != top]
            add(tag, kind, bw, st, st.put(blk), probes, G, ("bitfield_bits", top + 1))
        # 33 bitfield bytes cannot be a 256-bit integer: the node does not decode, whatever the key
        st = pyamt.Store()
        ka, kc = K((), 255, bw=8), K((), 5, bw=8)
        add("width8_33_byte_bitfield", kind, 8, st, st.put(raw_node(b"\x00\x80" + bytes(31), [bucket([(ka, val(kind, ka))])])),
            [(ka, DECODE, None), (kc, DECODE, None)], G, ("bitfield_bytes", 33))
        # leading zero bytes: the integer is the same (A.6: big-endian; a writer strips them, a reader need not care)
        st = pyamt.Store()
        ka, kb, kc = K((), 2), K((), 9), K((), 10)
        va, vb = val(kind, ka), val(kind, kb)
        add("bitfield_with_leading_zero_bytes", kind, 5, st,
            st.put(raw_node(bytes(6) + b"\x02\x04", [bucket([(ka, va)]), bucket([(kb, vb)])])),
            [(ka, TRUE, va), (kb, TRUE, vb), (kc, NOT_FOUND, None)], G)
        st = pyamt.Store()
        add("empty_bitfield_empty_pointers", kind, 5, st, st.put(raw_node(b"", [])), [(K((), j), NOT_FOUND, None) for j in (0, 9, 31)], G)
        # (an empty bitfield over a NON-empty pointer list, popcount ≠ pointer count: tests/assumption_cases.py)


def bitfield_of(block) -> bytes:
    import pystorage

    return pystorage.decode(block)[0]


_pointers_and_bitfield()


# ===== node length: the stage sizes, the outline threshold, 16-bit offsets ================================================
def sized_bucket_node(prefix, L, bw=5):
    """A bucket node of ActorStates of exactly L bytes: buckets of 3 on child indices 0, 1, 2 …, balances (1 … 23 bytes)
    and f4 / f1 addresses padding it → (block, [(key, value)] in node order)"""
    def enc(ents):
        at = {}
        for n, (key, bal) in enumerate(ents):
            at.setdefault(n // 3, []).append((key, value(n, key, bal)))
        return build_node({j: bucket(sorted(p)) for j, p in at.items()})

    def value(n, key, bal):
        adr = [NULL, bstr(b"\x04\x0a" + bytes(range(n % 20))), bstr(b"\x01" + bytes([n]) * 20)][n % 3]
        return astate(vi(key), bal=bytes([n & 1]) + bytes([0x85, 0xD8, 0x2A] * 8)[: bal - 1], adr=adr)

    ents = []
    while len(ents) < 3 * (1 << bw) - 3:
        n = len(ents)
        cand = ents + [(K(prefix, n // 3, n % 3, bw), 1)]
        if len(enc(cand)) > L:
            break
        ents = cand
    n = 0
    while len(enc(ents)) < L:
        assert n < len(ents), L
        if ents[n][1] < 23:
            ents[n] = (ents[n][0], ents[n][1] + 1)
        else:
            n += 1
    blk = enc(ents)
    assert len(blk) == L, (len(blk), L)
    return blk, [(key, value(n, key, bal)) for n, (key, bal) in enumerate(ents)]


def sized_bucket_child(L):
    def builder(st, kind, prefix):
        blk, pairs = sized_bucket_node(prefix, L)
        used = (len(pairs) + 2) // 3
        probes = [(k, TRUE, v) for k, v in (pairs[0], pairs[len(pairs) // 2], pairs[-1])]
        probes.append((K(prefix, 0, 3), NOT_FOUND, None))         # in the first bucket's place, not in it
        probes.append((K(prefix, 31, 0), NOT_FOUND, None))        # on a clear bit
        assert used < 31
        return st.put(blk), probes, lambda j: NOT_FOUND
    return builder


def sized_link_node(st, kind, prefix, L, bw):
    """A link-only node of exactly L bytes on child indices 0 … n-1: links of 43 (the standard CID), 41 (sha2-256) and, at
    width 5 where 32 pointers must do, 75 bytes (blake2b-512).  Three children exist and hold a key each; the others are
    links to blocks no witness holds."""
    found = None
    for n in range(1, (1 << bw) + 1):
        const = 1 + len(bstr(bytes((n + 7) // 8))) + len(head(4, n))
        for c in range(0, (n if bw == 5 else 0) + 1):
            for a in range(n - c, -1, -1):
                if const + 75 * c + 43 * a + 41 * (n - c - a) == L:
                    found = found or (n, c, a)
    assert found, (L, bw)
    n, c, a = found
    hows = ["long"] * c + ["std"] * a + ["sha"] * (n - c - a)
    hows = hows[n // 2:] + hows[: n // 2]  # (so the three kinds of link stand at the probed places, not in one run)
    live = sorted({0, n // 2, n - 1})
    at, probes = {}, []
    for j in range(n):
        if j in live:
            key = K(prefix, j, 0, bw)
            v = val(kind, key)
            at[j] = link(put(st, leaf_for(key, v, len(prefix) + 1, bw), hows[j]))
            probes.append((key, TRUE, v))
        else:
            at[j] = link(absent_cid(b"%d/%d/%d" % (L, bw, j), hows[j]))
    dead = next(j for j in range(n) if j not in live) if n > len(live) else None
    if dead is not None:
        probes.append((K(prefix, dead, 0, bw), MISSING, None))
    if n < 1 << bw:
        probes.append((K(prefix, (1 << bw) - 1, 0, bw), NOT_FOUND, None))
    blk = build_node(at)
    assert len(blk) == L, (len(blk), L)
    return st.put(blk), probes, lambda j: NOT_FOUND if (j in live or j >= n) else MISSING, n


def _node_lengths():
    G = "length"
    for L in BLOCK_LENGTHS:
        for kind in ("actor_state", "any"):  # (the stage sizes and the threshold are the ActorState outline's)
            st = pyamt.Store()
            cid, probes, _ = sized_bucket_child(L)(st, kind, ())
            add(f"bucket_node_of_{L}_bytes", kind, 5, st, cid, probes, G, ("block_len", L), shape="buckets")
            st = pyamt.Store()
            bw = 5 if L <= 2100 else 8
            cid, probes, _, n = sized_link_node(st, kind, (), L, bw)
            add(f"link_node_of_{L}_bytes", kind, bw, st, cid, probes, G, ("block_len", L), shape="links", pointers=n)
    # past 65 535 bytes: one long byte string as a value, and BEHIND it a bucket and a link that keys land on — their
    # offsets do not fit 16 bits
    st = pyamt.Store()
    ka, kb, kc, kd = K((), 1), K((), 6), K((), 20), K((), 25)
    vb, vc = val("any", kb), val("any", kc)
    behind = [bucket([(kb, vb)]), link(st.put(leaf_for(kc, vc, 1)))]
    # … and where those offsets point when they wrap — inside the long string — stand DECOYS: a bucket that gives the key another
    # value, and a link to a block no witness holds
    n = len(vb)
    other = NULL if n == 1 else bstr(b"d" * (n - 1)) if n <= 24 else bstr(b"d" * (n - 2))
    decoys = [bucket([(kb, other)]), link(absent_cid(b"decoy"))]
    assert other != vb and n < 256
    content = bytearray((i * 7 + (i >> 8)) & 0xFF for i in range(66000))
    for _ in range(2):  # (the second pass writes the decoys; no length changes)
        big = bstr(bytes(content))
        blk = build_node({1: bucket([(ka, big)]), 6: behind[0], 20: behind[1]})
        start = blk.index(big) + len(big) - len(content)
        for ptr, decoy in zip(behind, decoys):
            at = blk.index(ptr) - 65536 - start
            assert blk.index(ptr) > 65535 and at >= 0 and len(decoy) == len(ptr)
            content[at: at + len(decoy)] = decoy
    assert len(blk) > 65535 + 100 and all(blk[blk.index(p) - 65536:].startswith(d) for p, d in zip(behind, decoys))
    add("node_past_65535_bytes_pointers_behind_the_64k_mark", "any", 5, st, st.put(blk),
        [(ka, TRUE, big), (kb, TRUE, vb), (kc, TRUE, vc), (kd, NOT_FOUND, None), (K((), 6, 1), NOT_FOUND, None)], G,
        ("block_len", len(blk)), shape="buckets")


_node_lengths()


# ===== entries ==============================================================================================================
def entries_node(kind, prefix, total, bw=5):
    """`total` pairs in sorted buckets of 3 (the last one shorter) on child indices 0, 1, … → (block, pairs in node order)"""
    at, pairs = {}, []
    for j in range((total + 2) // 3):
        keys = sorted(K(prefix, j, k, bw) for k in range(min(3, total - 3 * j)))
        at[j] = bucket([(k, val(kind, k)) for k in keys])
        pairs += [(k, val(kind, k)) for k in keys]
    return build_node(at), pairs


def entries_child(total):
    def builder(st, kind, prefix):
        blk, pairs = entries_node(kind, prefix, total)
        probes = [(pairs[0][0], TRUE, pairs[0][1]), (pairs[-1][0], TRUE, pairs[-1][1]), (K(prefix, 0, 3), NOT_FOUND, None)]
        return st.put(blk), probes, lambda j: NOT_FOUND
    return builder


def _entries():
    for total in ENTRY_TOTALS:
        at_levels(f"node_of_{total}_entries", entries_child(total), "entries", levels=(0,), limit=("entries", total))


_entries()


# ===== keys =================================================================================================================
def key_of(n, salt=0) -> bytes:
    return bytes((7 * i + n + 31 * salt) & 0xFF for i in range(n)) if n else b""


def _same_place(make_pair, bw=5):
    """the first (stored, query) = make_pair(salt) whose two keys land on the same root index"""
    salt = 0
    while True:
        s, q = make_pair(salt)
        if s != q and pyhamt.index_at(s, 0, bw) == pyhamt.index_at(q, 0, bw):
            return s, q
        salt += 1


def _keys():
    G = "keys"
    salt = 0
    while max(collections.Counter(pyhamt.index_at(key_of(n, salt), 0, 5) for n in KEY_LENGTHS).values()) > 3:
        salt += 1
    stored = [key_of(n, salt) for n in KEY_LENGTHS]
    traps = {
        "query_is_the_first_8_bytes_of_a_stored_key": lambda s: (key_of(12, s), key_of(12, s)[:8]),
        "query_is_one_byte_longer_than_a_stored_key": lambda s: (key_of(8, s), key_of(8, s) + b"\x00"),
        "stored_key_of_256_bytes_probed_with_the_empty_key": lambda s: (key_of(256, s), b""),
        "stored_key_of_257_bytes_probed_with_its_first_byte": lambda s: (key_of(257, s), key_of(257, s)[:1]),
        "stored_key_of_255_bytes_probed_with_255_bytes_last_differs": lambda s: (key_of(255, s), key_of(255, s)[:-1] + bytes([key_of(255, s)[-1] ^ 1])),
        "stored_key_of_300_bytes_probed_with_its_first_44": lambda s: (key_of(300, s), key_of(300, s)[:44]),
    }
    for kind in KINDS:
        st, at = pyamt.Store(), {}
        for k in stored:
            at.setdefault(pyhamt.index_at(k, 0, 5), []).append(k)
        blk = build_node({j: bucket([(k, val(kind, k)) for k in sorted(ks)]) for j, ks in at.items()})
        probes = [(k, TRUE, val(kind, k)) for k in stored]
        # queries of the same lengths and other bytes, each one searched so that it lands in its stored key's bucket: the
        # answer comes from the key compare, not from a clear bit
        for n, k in zip(KEY_LENGTHS, stored):
            if n:
                probes.append((_same_place(lambda s: (k, key_of(n, salt + 1000 + s)))[1], NOT_FOUND, None))
        add("bucket_keys_of_every_length", kind, 5, st, st.put(blk), probes, G, ("key_len", 256), key_lens=KEY_LENGTHS)
        for name, make in traps.items():
            s, q = _same_place(make)
            j = pyhamt.index_at(s, 0, 5)
            st = pyamt.Store()
            add(name, kind, 5, st, st.put(build_node({j: bucket([(s, val(kind, s))])})), [(s, TRUE, val(kind, s)), (q, NOT_FOUND, None)],
                G, ("key_len", len(s)))
            st = pyamt.Store()
            pairs = sorted([(s, val(kind, s)), (q, val(kind, q))])
            add(name + "_both_stored", kind, 5, st, st.put(build_node({j: bucket(pairs)})),
                [(s, TRUE, val(kind, s)), (q, TRUE, val(kind, q))], G, ("key_len", len(s)))


_keys()


# ===== links ================================================================================================================
LINK_VARIANTS = {
    # name: (pointer(store, child block) → encoded pointer, status of the key behind it, the whole node fails)
    "standard_43_byte_link": (lambda st, ch: link(st.put(ch)), TRUE, False),
    "sha256_cid_of_36_bytes": (lambda st, ch: link(put(st, ch, "sha")), TRUE, False),
    "cid_longer_than_the_slot": (lambda st, ch: link(put(st, ch, "long")), TRUE, False),
    "link_to_an_absent_block": (lambda st, ch: link(absent_cid(ch)), MISSING, False),
    "link_to_a_block_that_is_no_node": (lambda st, ch: link(st.put(array([uint(1), bstr(ch[:9])]))), DECODE, False),
    "link_without_the_multibase_byte": (lambda st, ch: b"\xd8\x2a" + bstr(st.put(ch)), DECODE, True),
    "tag_42_over_a_text_string": (lambda st, ch: b"\xd8\x2a" + text("bafy2bzace"), DECODE, True),
    "pointer_is_a_map": (lambda st, ch: cmap([("0", link(st.put(ch)))]), DECODE, True),
    "pointer_is_a_uint": (lambda st, ch: uint(7), DECODE, True),
    "pointer_is_null": (lambda st, ch: NULL, DECODE, True),
}


def link_child(variant):
    make, behind, poisons = LINK_VARIANTS[variant]

    def builder(st, kind, prefix):
        (ja, ka), (jb, kb), (jc, kc) = pick(prefix, 3)
        va, vb = val(kind, ka), val(kind, kb)
        blk = build_node({ja: bucket([(ka, va)]), jb: make(st, leaf_for(kb, vb, len(prefix) + 1))})
        if poisons:  # serde decodes the whole node: every key that reaches it fails, also on a clear bit
            return st.put(blk), [(ka, DECODE, None), (kb, DECODE, None), (kc, DECODE, None)], lambda j: DECODE
        probes = [(ka, TRUE, va), (kb, behind, vb if behind == TRUE else None), (kc, NOT_FOUND, None)]
        return st.put(blk), probes, lambda j: behind if (j == jb and behind != TRUE) else NOT_FOUND
    return builder


def _links():
    for variant in LINK_VARIANTS:
        at_levels(variant, link_child(variant), "links", variant=variant)
    # a bucket node's own root missing / no node, under the fused top levels
    at_levels("node_absent", lambda st, kind, prefix: (absent_cid(b"node" + bytes(prefix)), [(k, MISSING, None) for _, k in pick(prefix, 2)],
                                                      lambda j: MISSING), "links")
    at_levels("node_is_a_uint", lambda st, kind, prefix: (st.put(uint(5)), [(k, DECODE, None) for _, k in pick(prefix, 2)], lambda j: DECODE), "links")


_links()


# ===== ActorState values at the outline's spellings ======================================================================
def _routes_flaw(flaw):
    """ONE text of the six flaws: tests/test_gpu_hamt_routes.py actor_state(i, rng, flaw), its random parts seeded by i"""
    def make(i):
        import numpy as np

        from test_gpu_hamt_routes import actor_state

        return actor_state(i, np.random.default_rng(i), flaw)
    return make


FLAWS = {
    **{flaw: _routes_flaw(flaw) for flaw in ("sign", "balance_len", "address_proto", "address_len", "arity", "link")},
    "trailing_sixth_item": lambda i: array([link(pyamt.cid_of(b"code")), link(pyamt.cid_of(b"state")), uint(i % 24), bstr(b"\x00\x05"), NULL, NULL]),
    "balance_of_129_bytes": lambda i: astate(i, bal=b"\x00" + b"\x01" * 128),
}
ANCHOR = b"\x85\xd8\x2a"  # `array(5), tag(42)`: how an ActorState begins
SPELLINGS = {  # accepted ones
    "balance_of_0_bytes": lambda i: astate(i, bal=b""),
    "balance_of_1_byte": lambda i: astate(i, bal=b"\x01"),
    "balance_of_128_bytes": lambda i: astate(i, bal=b"\x00" + b"\xfe" * 127),
    "address_f3_of_49_bytes_header_58_31": lambda i: astate(i, adr=bstr(b"\x03" + bytes(range(48)))),
    "address_f4_with_the_longest_subaddress": lambda i: astate(i, adr=bstr(b"\x04\x0a" + bytes(range(54)))),
    "anchor_bytes_inside_a_digest": lambda i: astate(i, state=link(bytes.fromhex("0171a0e40220") + ANCHOR * 10 + b"\x85\xd8")),
    "anchor_bytes_inside_a_balance": lambda i: astate(i, bal=b"\x00" + ANCHOR * 5),
    "anchor_bytes_inside_an_address": lambda i: astate(i, adr=bstr(b"\x04\x0a" + ANCHOR * 6)),
}


def actor_node(kind, prefix, special=None, at_entry=None, n=9, keys=None):
    """n single-pair buckets under `prefix`; entry `at_entry` (in node order) holds special(i) → (block, pairs in node order)"""
    got = sorted(pick(prefix, n)) if keys is None else keys
    pairs = []
    for e, (j, key) in enumerate(got):
        v = special(vi(key)) if e == at_entry else (val(kind, key) if kind != "any" else astate(vi(key)))
        pairs.append((j, key, v))
    return build_node({j: bucket([(key, v)]) for j, key, v in pairs}), pairs


def flaw_child(flaw, at_entry):
    def builder(st, kind, prefix):
        blk, pairs = actor_node(kind, prefix, FLAWS[flaw], at_entry)
        free = next(j for j in range(32) if j not in {p[0] for p in pairs})
        if kind == "actor_state":  # one flawed value poisons the whole node
            return st.put(blk), [(k, DECODE, None) for _, k, _ in pairs] + [(K(prefix, free), DECODE, None)], lambda j: DECODE
        return st.put(blk), [(k, TRUE, v) for _, k, v in pairs] + [(K(prefix, free), NOT_FOUND, None)], lambda j: NOT_FOUND
    return builder


def _actor_states():
    G = "actor_state"
    for flaw in FLAWS:
        for where, e in (("first", 0), ("middle", 4), ("last", 8)):
            for kind in ("actor_state", "any") if where == "middle" else ("actor_state",):
                # … and only the paths through that node: a sound sibling under the same root answers
                st = pyamt.Store()
                bad, probes, _ = flaw_child(flaw, e)(st, kind, (5,))
                good_blk, good = actor_node(kind, (21,))
                root = st.put(build_node({5: link(bad), 21: link(st.put(good_blk))}))
                probes = probes + [(k, TRUE, v) for _, k, v in good] + [(K((), 9), NOT_FOUND, None)]
                add(f"flaw_{flaw}_in_the_{where}_entry", kind, 5, st, root, probes, G, flaw=flaw)
    for name, spell in SPELLINGS.items():
        for kind in ("actor_state", "any"):
            st = pyamt.Store()
            blk, pairs = actor_node(kind, (), spell, 4)
            add(name, kind, 5, st, st.put(blk), [(k, TRUE, v) for _, k, v in pairs] + [(K((), 31, 7), NOT_FOUND, None)], G,
                ("balance_len", 128) if name == "balance_of_128_bytes" else None)
    # the anchor inside a KEY: the outline finds entries by their shape, a key may look like one
    for kind in KINDS:
        st = pyamt.Store()
        keys = [ANCHOR * 3 + bytes([k]) for k in range(6)] + [b"\x82\x45" + ANCHOR + bytes([k]) for k in range(3)]
        at = {}
        for k in keys:
            at.setdefault(pyhamt.index_at(k, 0, 5), []).append(k)
        assert max(len(v) for v in at.values()) <= 3
        blk = build_node({j: bucket([(k, val(kind, k)) for k in sorted(ks)]) for j, ks in at.items()})
        add("anchor_bytes_inside_keys", kind, 5, st, st.put(blk), [(k, TRUE, val(kind, k)) for k in keys] + [(ANCHOR, NOT_FOUND, None)], G)


_actor_states()


# ===== depth ================================================================================================================
def chain_of_links(st, bw, n_links, last):
    """n_links link-only nodes — every bit set, every pointer a link to the next node, so every key walks them all — above
    the block `last` → root CID"""
    cid = st.put(last)
    for _ in range(n_links):
        cid = st.put(node((1 << (1 << bw)) - 1, [link(cid)] * (1 << bw)))
    return cid


def path_of_links(st, bw, key, n_links, last):
    """n_links single-link nodes along `key`'s own path above `last` (width 8: a full node would hold 256 links)"""
    cid = st.put(last)
    for d in range(n_links - 1, -1, -1):
        cid = st.put(build_node({pyhamt.index_at(key, d, bw): link(cid)}))
    return cid


def _depth():
    G = "depth"
    key, other, third = b"the key of the depth chains", b"another key", b"a third key"
    assert pyhamt.index_at(key, 0, 8) != pyhamt.index_at(other, 0, 8)
    for kind in KINDS:
        v = val(kind, key)
        # width 5: 51 × 5 = 255 bits; the 52nd `next(5)` overruns the 256 (SURVEY.md A.6 "> 256/bw levels ⇒ MaxDepth")
        st = pyamt.Store()
        add("width5_chain_of_52_link_nodes", kind, 5, st, chain_of_links(st, 5, 51, node((1 << 32) - 1, [link(absent_cid(b"53rd"))] * 32)),
            [(key, MAX_DEPTH, None), (other, MAX_DEPTH, None), (b"", MAX_DEPTH, None)], G, ("depth5", 52))
        st = pyamt.Store()
        add("width5_bucket_node_as_the_51st_node", kind, 5, st, chain_of_links(st, 5, 50, leaf_for(key, v, 50, 5)),
            [(key, TRUE, v)] + [(k, NOT_FOUND, None) for k in (other, third, b"")], G, ("depth5", 51))
        # the 52nd node is fetched and decoded, then `next` fails: the key it holds is never looked for
        st = pyamt.Store()
        add("width5_bucket_node_as_the_52nd_node", kind, 5, st, chain_of_links(st, 5, 51, leaf_for(key, v, 51 - 1, 5)),
            [(key, MAX_DEPTH, None), (other, MAX_DEPTH, None)], G, ("depth5", 52))
        for n in (256, 257):
            st = pyamt.Store()
            last = leaf_for(key, v, n - 1, 1) if n == 256 else build_node({0: bucket([(key, v)]), 1: bucket([(other, val(kind, other))])})
            probes = [(key, TRUE, v), (other, NOT_FOUND, None), (third, NOT_FOUND, None)] if n == 256 else [(k, MAX_DEPTH, None) for k in (key, other, third)]
            add(f"width1_{n}_levels", kind, 1, st, chain_of_links(st, 1, n - 1, last), probes, G, ("depth1", n))
        for n in (32, 33):
            st = pyamt.Store()
            last = leaf_for(key, v, n - 1, 8) if n == 32 else build_node({0: bucket([(key, v)])})
            probes = [(key, TRUE if n == 32 else MAX_DEPTH, v if n == 32 else None), (other, NOT_FOUND, None)]
            add(f"width8_{n}_levels", kind, 8, st, path_of_links(st, 8, key, n - 1, last), probes, G, ("depth8", n))


_depth()


# ===== widths ===============================================================================================================
WIDTHS_IN_RANGE = (1, 2, 4, 7, 8)
WIDTHS_OUT_OF_RANGE = (0, 9, 32, (1 << 32) - 1)  # on a root that exists: tests/assumption_cases.py


def width_items(kind):
    keys = [b"width key %d" % i for i in range(40)]
    return keys, {k: val(kind, k) for k in keys}


def _widths():
    for kind in KINDS:
        keys, items = width_items(kind)
        for bw in WIDTHS_IN_RANGE:
            st = pyamt.Store()
            root = pyhamt.build_hamt(st, items, bw)
            add(f"width_{bw}", kind, bw, st, root, [(k, TRUE, items[k]) for k in keys[::6]] + [(b"no such key", NOT_FOUND, None), (b"", NOT_FOUND, None)],
                "widths", ("width", bw))
        # `load_with_bit_width` fetches the root before anything looks at the width (storage/decode.rs:79-80)
        for bw in WIDTHS_IN_RANGE + WIDTHS_OUT_OF_RANGE:
            st = pyamt.Store()
            st.put(leaf_for(keys[0], items[keys[0]], 0))  # (a witness that holds something)
            add(f"width_{bw}_root_missing", kind, bw, st, absent_cid(b"root"), [(keys[0], MISSING, None), (b"", MISSING, None)], "widths", ("width", bw))


_widths()


# ===== the cases that state an assumption about the crates ==============================================================
def _assumption_cases():
    import assumption_cases as ac

    for name, make in ac.HAMT_GET_CASES.items():
        for kind in KINDS:
            made = make(kind)
            if made is not None:
                st, root, bw, probes, limit = made
                add(name, kind, bw, st, root, probes, "assumption", limit)


_assumption_cases()


# ===== one composite tree: 32 children of every sort under one width-5 root =============================================
def _plain_child(n):
    def builder(st, kind, prefix):
        blk, pairs = actor_node(kind, prefix, n=n)
        free = next(j for j in range(32) if j not in {p[0] for p in pairs})
        return st.put(blk), [(k, TRUE, v) for _, k, v in pairs] + [(K(prefix, free), NOT_FOUND, None)], lambda j: NOT_FOUND
    return builder


def _small_link_child(L):
    def builder(st, kind, prefix):
        return sized_link_node(st, kind, prefix, L, 5)[:3]
    return builder


COMPOSITE_CHILDREN = [
    ("bucket_node_of_1512_bytes", sized_bucket_child(1512)), ("bucket_node_of_1513_bytes", sized_bucket_child(1513)),
    ("bucket_node_of_4328_bytes", sized_bucket_child(4328)), ("bucket_node_of_4329_bytes", sized_bucket_child(4329)),
    ("bucket_node_of_6888_bytes", sized_bucket_child(6888)), ("bucket_node_of_6889_bytes", sized_bucket_child(6889)),
    ("bucket_node_of_2047_bytes", sized_bucket_child(2047)), ("bucket_node_of_2048_bytes", sized_bucket_child(2048)),
    ("bucket_node_of_7500_bytes", sized_bucket_child(7500)),
    ("node_absent", lambda st, kind, prefix: (absent_cid(b"composite"), [], lambda j: MISSING)),
    ("node_is_a_uint", lambda st, kind, prefix: (st.put(uint(5)), [], lambda j: DECODE)),
    ("flaw_sign", flaw_child("sign", 0)), ("flaw_balance_len", flaw_child("balance_len", 4)),
    ("flaw_address_proto", flaw_child("address_proto", 8)), ("flaw_address_len", flaw_child("address_len", 0)),
    ("flaw_arity", flaw_child("arity", 4)), ("flaw_link", flaw_child("link", 8)),
    ("standard_43_byte_link", link_child("standard_43_byte_link")), ("sha256_cid_of_36_bytes", link_child("sha256_cid_of_36_bytes")),
    ("cid_longer_than_the_slot", link_child("cid_longer_than_the_slot")), ("link_to_an_absent_block", link_child("link_to_an_absent_block")),
    ("link_without_the_multibase_byte", link_child("link_without_the_multibase_byte")),
    ("link_to_a_block_that_is_no_node", link_child("link_to_a_block_that_is_no_node")),
    ("empty_node", lambda st, kind, prefix: (st.put(raw_node(b"", [])), [], lambda j: NOT_FOUND)),
    ("node_of_96_entries", entries_child(96)), ("node_of_24_entries", entries_child(24)), ("node_of_25_entries", entries_child(25)),
    ("link_node_of_1512_bytes", _small_link_child(1512)), ("link_node_of_1513_bytes", _small_link_child(1513)),
    ("plain_1", _plain_child(1)), ("plain_9", _plain_child(9)), ("plain_20", _plain_child(20)),
]
assert len(COMPOSITE_CHILDREN) == 32


def _one_level_down(builder, j=13):
    """the child's node hung under a single-link node of its own: the case then sits at level 2 of the composite"""
    def wrapped(st, kind, prefix):
        cid, probes, _ = builder(st, kind, tuple(prefix) + (j,))
        return st.put(build_node({j: link(cid)})), probes, lambda jj: None if jj == j else NOT_FOUND
    return wrapped


_absent_child = lambda st, kind, prefix: (absent_cid(b"link composite" + bytes(prefix)), [], lambda j: MISSING)  # noqa: E731
_uint_child = lambda st, kind, prefix: (st.put(uint(5)), [], lambda j: DECODE)  # noqa: E731
# every spelling of a link at level 1 and at level 2 of ONE tree, with sound neighbours: the fused top's lists hold them side by side
LINK_COMPOSITE_CHILDREN = (
    [(v, link_child(v)) for v in LINK_VARIANTS] + [(v + "_one_level_down", _one_level_down(link_child(v))) for v in LINK_VARIANTS]
    + [("node_absent", _absent_child), ("node_is_a_uint", _uint_child),
       ("node_absent_one_level_down", _one_level_down(_absent_child)), ("node_is_a_uint_one_level_down", _one_level_down(_uint_child))]
    + [(f"plain_{n}", _plain_child(n)) for n in (1, 2, 3, 5, 9, 12, 20, 31)])
assert len(LINK_COMPOSITE_CHILDREN) == 32


def composite(kind, children=COMPOSITE_CHILDREN, n_keys=2048):
    """→ (store, root, keys, want, values, child number of each key, [child block length or None])
    keys come child by child: the children's own probes first, then keys on every next index in turn, whose status is what
    the child's case states for a key it does not hold (None: it states none for that index)"""
    st = pyamt.Store()
    at, per_child, lens = {}, [], []
    for ci, (_name, builder) in enumerate(children):
        cid, probes, other = builder(st, kind, (ci,))
        at[ci] = link(cid)
        lens.append(len(st.blocks[cid]) if cid in st.blocks else None)
        have = {p[0] for p in probes}
        j = k = 0
        while len(probes) < n_keys // 32:
            key = K((ci,), j, 10 + k)  # (the children's own keys are the first few of each place)
            if key not in have and other(j) is not None:
                probes.append((key, other(j), None))
            j, k = (j + 1) % 32, k + (j == 31)
        per_child.append(probes)
    root = st.put(build_node(at))
    keys, want, values, child = [], [], [], []
    for ci, probes in enumerate(per_child):
        for key, status, value in probes:
            keys.append(key)
            want.append(status)
            child.append(ci)
            if status == TRUE:
                values.append(value)
    return st, root, keys, want, values, child, lens


COMPOSITE = {kind: composite(kind) for kind in ("actor_state", "any")}
LINK_COMPOSITE = {kind: composite(kind, LINK_COMPOSITE_CHILDREN) for kind in ("actor_state", "any")}
COMPOSITES = {"children": COMPOSITE, "links": LINK_COMPOSITE}


def _composite_cases():
    for name, trees in (("composite_tree_of_32_children", COMPOSITE), ("composite_tree_of_link_spellings", LINK_COMPOSITE)):
        for kind, (st, root, keys, want, values, _child, _lens) in trees.items():
            it = iter(values)
            probes = [(k, w, next(it) if w == TRUE else None) for k, w in zip(keys, want)]
            add(name, kind, 5, st, root, probes, "composite")


_composite_cases()


# ===== batches wide enough for the fused top levels =====================================================================
# The level path fuses its top levels only for a batch that can fill them: two levels from 32 queries, three from 1024, and
# as many blocks in the witness (hamt_levels.hip: 32^(top-1) <= min(queries, blocks)).  A case built at level 1 or 3 has
# three probes; `wide` sends them among keys that stand on clear bits of the single-link nodes above the case's node.
FUSED_TOP_MIN_QUERIES = (32, 1024)
WIDE_QUERIES = 1024 + 64
LEVEL_CASES = [n for n, m in META.items() if m.get("level") in (1, 3)]
_FILL = {}


def _fill(level):
    if level not in _FILL:
        prefix, out = PREFIX[level], []
        for d, per_index in ((2, 1), (1, 3), (0, 40)):  # few keys deep in the tree (each is a search), many at the root
            if d < level:
                out += [K(prefix[:d], j, 10 + k) for k in range(per_index) for j in range(32) if j != prefix[d]]
        _FILL[level] = out[: WIDE_QUERIES]
    return _FILL[level]


def wide(name) -> Case:
    c = CASES[name]
    fill = [k for k in _fill(META[name]["level"]) if k not in c.keys][: WIDE_QUERIES - len(c.keys)]
    half = len(fill) // 2  # (the case's own probes stand in the middle of the batch)
    return c._replace(keys=fill[:half] + c.keys + fill[half:], want=[NOT_FOUND] * half + c.want + [NOT_FOUND] * (len(fill) - half))


def stage_class(length):
    """the level path's size class of a node, by LIMITS (0 small, 1 mid, 2 big, None: not staged)"""
    for c, stage in enumerate(LIMITS["stage_bytes"]):
        if length + STAGE_SLACK <= stage:
            return c
    return None


# ---- helpers the two test files share ------------------------------------------------------------------------------------
def tables(store):
    """→ (data, off, lens, [CID bytes]) — the CIDs as they are, of any length"""
    import numpy as np

    cids = list(store.blocks)
    blocks = [store.blocks[c] for c in cids]
    lens = np.array([len(b) for b in blocks], dtype=np.uint32)
    off = np.zeros(len(cids), dtype=np.uint64)
    if len(cids):
        off[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    return np.frombuffer(b"".join(blocks) or b"\0", dtype=np.uint8).copy(), off, lens, cids


def merged():
    """All cases' blocks in ONE witness (CIDs are content hashes: stores merge by dict union; a block a case needs ABSENT
    is named by a seed no case stores) → store"""
    st = pyamt.Store()
    for name, c in CASES.items():
        for cid, b in c.store.blocks.items():
            assert st.blocks.setdefault(cid, b) == b, name
    for name, c in CASES.items():
        assert (c.root in st.blocks) == (c.root in c.store.blocks), name
    return st
