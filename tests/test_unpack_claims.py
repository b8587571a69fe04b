"""CPU: the host inverse of the claim lowering (csrc/host/unpack_claims.cpp, ipcfp_unpack_event_claims — no GPU):
ipcfp_tipset_ref_t / ipcfp_event_claim_t / blob → the reference's EventProof structs with the strings the reference
writes ("0x" + lowercase hex, `Cid::to_string()`).  Checked as the inverse of ipcfp_pack_event_proofs on the golden
bundle's proofs and on seeded random ones, on every refusal with its code and index, and with one range against eight."""
import os

import numpy as np
import pytest

import bundle_ref
import claims
import ipc_filecoin_proofs_amd as ipcfp
from ipc_filecoin_proofs_amd.binding import unpack_event_claims

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bundle_small.json")
E_INVALID, E_UNSUPPORTED = -1, -5
B58 = "123456789ABCDEFGHJKLMNPQRSTUVWXYZabcdefghijkmnopqrstuvwxyz"


def b58(b: bytes) -> str:
    n, out = int.from_bytes(b, "big"), ""
    while n:
        n, r = divmod(n, 58)
        out = B58[r] + out
    return "1" * (len(b) - len(b.lstrip(b"\0"))) + out


def canonical_cid(cid: bytes) -> str:
    """`Cid::to_string()`: base58btc for a CIDv0, "b" + base32-lower for a CIDv1."""
    return b58(cid) if len(cid) == 34 and cid[:2] == b"\x12\x20" else claims.cid_str(cid)


def random_cid(rng) -> bytes:
    digest = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    return (b"\x12\x20" + digest, bytes.fromhex("01551220") + digest, bytes.fromhex("0171a0e40220") + digest)[int(rng.integers(0, 3))]


def spell_cid(rng, cid: bytes) -> str:
    """One of the spellings `Cid::try_from` takes for this CID (the canonical one most of the time)."""
    k = int(rng.integers(0, 4))
    if len(cid) == 34 or k < 2:
        return canonical_cid(cid)
    if k == 2:
        return "f" + cid.hex()           # base16 multibase
    return claims.cid_str(cid).upper()   # "B" + base32-upper


def random_rows(seed: int, n: int, n_tipsets: int = 3, wide: int = 0):
    """(rows as given to the packer, rows in the reference's spelling)"""
    rng = np.random.default_rng(seed)
    tips = []
    for t in range(n_tipsets):
        parents = [random_cid(rng) for _ in range(wide if (wide and t == 0) else int(rng.integers(0, 6)))]
        tips.append((parents, random_cid(rng), int(rng.integers(-5, 1 << 40))))
    given, canon = [], []
    for i in range(n):
        parents, child, epoch = tips[int(rng.integers(0, n_tipsets))]
        msg = random_cid(rng)
        topics = [rng.integers(0, 256, 32, dtype=np.uint8).tobytes() for _ in range(int(rng.integers(0, 10)))]
        # (the ends of the range in the first rows, whatever the seed draws)
        data = rng.integers(0, 256, (0, 300, 1)[i] if i < 3 else int(rng.integers(0, 301)), dtype=np.uint8).tobytes()
        base = dict(parent_epoch=epoch, child_epoch=epoch + 1, exec_index=int(rng.integers(0, 1 << 63)),
                    event_index=int(rng.integers(0, 1 << 32)), emitter=int(rng.integers(0, 1 << 64, dtype=np.uint64)))
        up = bool(rng.integers(0, 2))
        hx = (lambda b: "0X" + b.hex().upper()) if up else (lambda b: "0x" + b.hex())
        # one tipset = one spelling of its key (the packer groups by the strings)
        given.append(dict(base, parent_tipset_cids=[canonical_cid(c) for c in parents], child_block_cid=canonical_cid(child),
                          message_cid=spell_cid(rng, msg), topics=[hx(t) for t in topics], data=hx(data)))
        canon.append(dict(base, parent_tipset_cids=[canonical_cid(c) for c in parents], child_block_cid=canonical_cid(child),
                          message_cid=canonical_cid(msg), topics=["0x" + t.hex() for t in topics], data="0x" + data.hex()))
    return given, canon


def pack_rows(rows):
    ev, _ = bundle_ref.claims_from_parsed({"event_proofs": rows, "storage_proofs": []})
    return ipcfp.pack_event_proofs(ev.arr, ev.n)


def tipsets_equal(a, b):
    """ipcfp_tipset_ref_t tables: every field but the address in `more_parents`, and what that address names"""
    if len(a) != len(b):
        return False
    for k in range(len(a)):
        for f in ("flags", "n_parents", "child", "parents"):
            if not np.array_equal(a[f][k], b[f][k]):
                return False
        extra = int(a["n_parents"][k]) - 32
        if extra > 0:
            import ctypes as C

            x = C.string_at(int(a["more_parents"][k]), extra * 40)
            y = C.string_at(int(b["more_parents"][k]), extra * 40)
            if x != y:
                return False
    return True


def round_trip(rows, canon):
    ts, cl, blob = pack_rows(rows)
    with unpack_event_claims(ts, cl, blob) as u:
        assert u.n == len(rows)
        assert u.rows() == canon
        ts2, cl2, blob2 = ipcfp.pack_event_proofs(u.ptr, u.n)   # pack → unpack → pack
    assert tipsets_equal(ts, ts2)
    assert cl.tobytes() == cl2.tobytes()
    assert blob.tobytes() == blob2.tobytes()
    return ts, cl, blob


def test_golden_proofs_round_trip():
    rows = bundle_ref.parse_bundle(open(GOLDEN, "rb").read())["event_proofs"]
    assert len(rows) > 0
    round_trip(rows, rows)  # the golden bundle is the reference's own spelling


def test_random_proofs_round_trip():
    given, canon = random_rows(0xC1A1, 200)
    assert given != canon  # some spellings are not the canonical ones
    ts, cl, blob = round_trip(given, canon)
    assert len(ts) == 3 and {int(x) for x in cl["n_topics"]} == set(range(10))
    assert (cl["data_len"] == 0).any() and (cl["data_len"] > 255).any()


def test_empty_batch():
    ts, cl, blob = pack_rows([])
    with unpack_event_claims(ts, cl, blob) as u:
        assert u.n == 0 and u.rows() == []
    with unpack_event_claims(np.zeros(0, ipcfp.TIPSET_DTYPE), np.zeros(0, ipcfp.CLAIM_DTYPE), np.zeros(0, np.uint8)) as u:
        assert u.n == 0


def test_two_tipsets_and_a_wide_key():
    """proofs of one tipset share its string arrays; a key of 33 parents comes through `more_parents`"""
    given, canon = random_rows(0xC1A2, 40, n_tipsets=2, wide=33)
    ts, cl, blob = round_trip(given, canon)
    assert len(ts) == 2 and 33 in ts["n_parents"].tolist() and set(cl["tipset"].tolist()) == {0, 1}
    assert any(len(r["parent_tipset_cids"]) == 33 for r in canon)
    with unpack_event_claims(ts, cl, blob) as u:
        import ctypes as C

        from ipc_filecoin_proofs_amd.binding import EventProofStruct

        arr = (EventProofStruct * u.n).from_address(u.ptr)
        addr = {}
        for k in range(u.n):
            addr.setdefault(int(cl["tipset"][k]), set()).add(C.cast(arr[k].parent_tipset_cids, C.c_void_p).value)
        assert all(len(s) == 1 for s in addr.values())


def refusal(ts, cl, blob, blob_len=None):
    with pytest.raises(ipcfp.EngineError) as e:
        unpack_event_claims(ts, cl, blob, blob_len)
    return e.value.rc, e.value.bad_index


@pytest.fixture(scope="module")
def good():
    given, _ = random_rows(0xC1A3, 12, n_tipsets=2)
    for r in given:  # every claim has a topic and some data, so that every mutation below has something to hit
        if not r["topics"]:
            r["topics"] = ["0x" + "11" * 32]
        if len(r["data"]) == 2:
            r["data"] = "0xabcd"
    ts, cl, blob = pack_rows(given)
    unpack_event_claims(ts, cl, blob).close()
    return ts, cl, blob


def test_refusals(good):
    ts, cl, blob = good
    fold = ipcfp.cid_slot(bytes.fromhex("0171c0e40240") + bytes(range(64)))
    assert fold[0] == 0xFF

    def mutate(i, field=None, value=None):
        c = cl.copy()
        if field:
            c[field][i] = value
        return c

    # a topic whose flag byte is 0: the string was not "0x" + 64 hex digits, and which string it was is gone
    b = blob.copy()
    b[int(cl["topics_off"][5])] = 0
    assert refusal(ts, cl, b) == (E_INVALID, 5)
    b = blob.copy()
    b[int(cl["topics_off"][7]) + 33 * (int(cl["n_topics"][7]) - 1)] = 0   # the LAST topic of a claim
    assert refusal(ts, cl, b) == (E_INVALID, 7)
    # a claim without both flag bits
    for flags in (0, 1, 2):
        assert refusal(ts, mutate(3, "flags", flags), blob) == (E_INVALID, 3)
    # offsets outside the blob
    assert refusal(ts, mutate(4, "topics_off", len(blob) - 32), blob) == (E_INVALID, 4)
    assert refusal(ts, mutate(4, "topics_off", 0xFFFFFFFF), blob) == (E_INVALID, 4)
    assert refusal(ts, mutate(6, "data_off", len(blob) - int(cl["data_len"][6]) + 1), blob) == (E_INVALID, 6)
    assert refusal(ts, mutate(6, "data_len", 0xFFFFFFFF), blob) == (E_INVALID, 6)
    assert refusal(ts, cl, blob, blob_len=len(blob) - 1) == (E_INVALID, len(cl) - 1)  # the last claim's data ends the blob
    # tipset at or beyond n_tipsets
    assert refusal(ts, mutate(2, "tipset", len(ts)), blob) == (E_INVALID, 2)
    assert refusal(ts, mutate(2, "tipset", 0xFFFFFFFF), blob) == (E_INVALID, 2)
    # a tipset without both parsed flags: every claim that names it, so the lowest one
    for flags in (0, 1, 2):
        t = ts.copy()
        t["flags"][1] = flags
        first = int(np.nonzero(cl["tipset"] == 1)[0][0])
        assert refusal(t, cl, blob) == (E_INVALID, first)
    # a slot that holds no CID at all
    c = cl.copy()
    c["message_cid"][8] = 0
    assert refusal(ts, c, blob) == (E_INVALID, 8)
    c = cl.copy()
    c["message_cid"][8, 39] = 1  # something behind the CID that is not padding
    assert refusal(ts, c, blob) == (E_INVALID, 8)
    # a folded slot: the CID's bytes are not there
    c = cl.copy()
    c["message_cid"][9] = fold
    assert refusal(ts, c, blob) == (E_UNSUPPORTED, 9)
    t = ts.copy()
    t["child"][0] = fold
    assert refusal(t, cl, blob) == (E_UNSUPPORTED, int(np.nonzero(cl["tipset"] == 0)[0][0]))
    with_parents = [k for k in range(len(ts)) if ts["n_parents"][k] > 0]
    if with_parents:
        k = with_parents[0]
        t = ts.copy()
        t["parents"][k, int(ts["n_parents"][k]) - 1] = fold
        assert refusal(t, cl, blob) == (E_UNSUPPORTED, int(np.nonzero(cl["tipset"] == k)[0][0]))
    # the untouched batch still unpacks
    unpack_event_claims(ts, cl, blob).close()


def test_two_defects_name_the_lower_one(good):
    ts, cl, blob = good
    fold = ipcfp.cid_slot(bytes.fromhex("0171c0e40240") + bytes(range(64)))
    c = cl.copy()
    c["message_cid"][10] = fold     # UNSUPPORTED at 10 …
    c["flags"][4] = 1               # … INVALID at 4
    assert refusal(ts, c, blob) == (E_INVALID, 4)
    c = cl.copy()
    c["message_cid"][2] = fold      # UNSUPPORTED at 2 …
    c["tipset"][9] = 77             # … INVALID at 9
    assert refusal(ts, c, blob) == (E_UNSUPPORTED, 2)


def test_one_range_against_eight(monkeypatch):
    """3000 claims: checked, sized and written in one range and in eight (IPCFP_HOST_THREADS pins the count)."""
    given, canon = random_rows(0xC1A4, 3000, n_tipsets=4)
    ts, cl, blob = pack_rows(given)
    monkeypatch.setenv("IPCFP_HOST_THREADS", "1")
    with unpack_event_claims(ts, cl, blob) as u:
        one = u.rows()
    monkeypatch.setenv("IPCFP_HOST_THREADS", "8")
    with unpack_event_claims(ts, cl, blob) as u:
        eight = u.rows()
        ts2, cl2, blob2 = ipcfp.pack_event_proofs(u.ptr, u.n)
    assert one == eight == canon
    assert cl.tobytes() == cl2.tobytes() and blob.tobytes() == blob2.tobytes()
    # a refusal in the sixth range of eight and one in the second: the lower one, whatever thread finds it first
    c = cl.copy()
    c["flags"][2000] = 0
    c["tipset"][500] = 99
    assert refusal(ts, c, blob) == (E_INVALID, 500)
    monkeypatch.setenv("IPCFP_HOST_THREADS", "1")
    assert refusal(ts, c, blob) == (E_INVALID, 500)
