"""CPU: the host inverse of the storage claim lowering (csrc/host/unpack_claims.cpp, ipcfp_unpack_storage_claims — no GPU):
ipcfp_storage_claim_t rows → the reference's StorageProof structs as create_proof_claim spells them
(src/proofs/storage/generator.rs:158-178: `Cid::to_string()`, "0x" + 64 lowercase hex digits).  Checked as the inverse of
ipcfp_pack_storage_proofs on the golden bundle's proofs and on seeded ones in other spellings, on every refusal with its
code and index, and with one range against eight."""
import os

import numpy as np
import pytest

import bundle_ref
import ipc_filecoin_proofs_amd as ipcfp
import storage_chain_cases as sc
from ipc_filecoin_proofs_amd.binding import unpack_storage_claims
from test_unpack_claims import canonical_cid, random_cid, spell_cid

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bundle_small.json")
E_INVALID, E_UNSUPPORTED = -1, -5
FIELDS = ("child_epoch", "child_block_cid", "parent_state_root", "actor_id", "actor_state_cid", "storage_root", "slot", "value")


def random_rows(seed: int, n: int):
    """(rows as given to the packer, rows in the reference's spelling).  The three derived CIDs must be canonical strings
    for their flag bits (storage/verifier.rs:110, :126, :144 compare strings); the child CID only has to parse."""
    rng = np.random.default_rng(seed)
    given, canon = [], []
    for i in range(n):
        child, sroot, astate, root = (random_cid(rng) for _ in range(4))
        slot = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
        value = rng.integers(0, 256, 32, dtype=np.uint8).tobytes() if i % 7 else bytes(32)
        base = dict(child_epoch=int(rng.integers(-5, 1 << 40)), actor_id=int(rng.integers(0, 1 << 64, dtype=np.uint64)),
                    parent_state_root=canonical_cid(sroot), actor_state_cid=canonical_cid(astate), storage_root=canonical_cid(root))
        k = int(rng.integers(0, 4))
        slot_s = ("0x" + slot.hex(), "0x0x0x" + slot.hex().upper(), slot.hex(), "0x" + slot.hex().upper())[k]
        value_s = ("0x" + value.hex(), "0X" + value.hex().upper(), "0x" + value.hex().upper(), "0X" + value.hex())[int(rng.integers(0, 4))]
        given.append(dict(base, child_block_cid=spell_cid(rng, child), slot=slot_s, value=value_s))
        canon.append(dict(base, child_block_cid=canonical_cid(child), slot="0x" + slot.hex(), value="0x" + value.hex()))
    return given, canon


def pack_rows(rows):
    pr = sc.proofs(rows)
    return ipcfp.pack_storage_proofs(pr.arr, pr.n)


def round_trip(rows, canon):
    cl = pack_rows(rows)
    assert (cl["flags"] == 63).all()
    with unpack_storage_claims(cl) as u:
        assert u.n == len(rows)
        assert u.rows() == canon
        cl2 = ipcfp.pack_storage_proofs(u.ptr, u.n)   # pack → unpack → pack
    assert cl.tobytes() == cl2.tobytes()
    return cl


def refusal(cl):
    with pytest.raises(ipcfp.EngineError) as e:
        unpack_storage_claims(cl)
    return e.value.rc, e.value.bad_index


def test_golden_proofs_round_trip():
    rows = bundle_ref.parse_bundle(open(GOLDEN, "rb").read())["storage_proofs"]
    assert len(rows) > 0
    rows = [{f: r[f] for f in FIELDS} for r in rows]
    # one of the golden bundle's proofs is a planted bad claim (slot "0x12": no 32 bytes): it lowers to a row without
    # IPCFP_SCLAIM_SLOT_PARSED, which no StorageProof of the generator's spelling lowers to — refused, by its index
    planted = [i for i, r in enumerate(rows) if len(r["slot"]) != 66]
    assert len(planted) == 1
    assert refusal(pack_rows(rows)) == (E_INVALID, planted[0])
    rows = [r for i, r in enumerate(rows) if i not in planted]
    assert len(rows) >= 8
    round_trip(rows, rows)  # the golden bundle is the reference's own spelling


def test_random_proofs_round_trip():
    given, canon = random_rows(0x5C1A1, 200)
    assert sum(g != c for g, c in zip(given, canon)) > 100  # most rows come in another spelling
    assert any(g["child_block_cid"].startswith("f") for g in given) and any(g["child_block_cid"].startswith("B") for g in given)
    assert any(c["parent_state_root"].startswith("Qm") for c in canon) and any(g["slot"].startswith("0x0x") for g in given)
    round_trip(given, canon)


def test_empty_batch():
    with unpack_storage_claims(np.zeros(0, ipcfp.SCLAIM_DTYPE)) as u:
        assert u.n == 0 and u.rows() == []


@pytest.fixture(scope="module")
def good():
    return pack_rows(random_rows(0x5C1A3, 24)[0])


@pytest.mark.parametrize("bit", [1, 2, 4, 8, 16, 32])
def test_a_missing_flag_bit_is_invalid(good, bit):
    c = good.copy()
    c["flags"][7] = 63 & ~bit
    assert refusal(c) == (E_INVALID, 7)


def test_unknown_bits_and_reserved_are_invalid(good):
    c = good.copy()
    c["flags"][3] = 63 | 64
    assert refusal(c) == (E_INVALID, 3)
    c = good.copy()
    c["flags"][23] = 63 | (1 << 31)
    assert refusal(c) == (E_INVALID, 23)
    c = good.copy()
    c[c.dtype.names[-1]][0] = 1  # the reserved word
    assert refusal(c) == (E_INVALID, 0)


@pytest.mark.parametrize("field", ["child", "state_root", "actor_state", "storage_root"])
def test_a_slot_that_is_not_a_cid_is_invalid_and_a_fold_is_unsupported(good, field):
    c = good.copy()
    c[field][5] = 0
    assert refusal(c) == (E_INVALID, 5)
    c = good.copy()
    c[field][5][39] = 1  # bytes behind the CID's end
    assert refusal(c) == (E_INVALID, 5)
    c = good.copy()
    c[field][6] = ipcfp.cid_slot(bytes.fromhex("0171c0e40240") + bytes(range(64)))
    assert int(c[field][6][0]) == 0xFF
    assert refusal(c) == (E_UNSUPPORTED, 6)


def test_two_defects_name_the_lower_one(good):
    fold = ipcfp.cid_slot(bytes.fromhex("0171c0e40240") + bytes(range(64)))
    c = good.copy()
    c["storage_root"][10] = fold    # UNSUPPORTED at 10 …
    c["flags"][4] = 1               # … INVALID at 4
    assert refusal(c) == (E_INVALID, 4)
    c = good.copy()
    c["child"][2] = fold            # UNSUPPORTED at 2 …
    c["flags"][9] = 0               # … INVALID at 9
    assert refusal(c) == (E_UNSUPPORTED, 2)


def test_one_range_against_eight(monkeypatch):
    """9000 claims: checked, sized and written in one range and in eight (IPCFP_HOST_THREADS pins the count)."""
    given, canon = random_rows(0x5C1A4, 9000)
    cl = pack_rows(given)
    monkeypatch.setenv("IPCFP_HOST_THREADS", "1")
    with unpack_storage_claims(cl) as u:
        one = u.rows()
    monkeypatch.setenv("IPCFP_HOST_THREADS", "8")
    with unpack_storage_claims(cl) as u:
        eight = u.rows()
        cl2 = ipcfp.pack_storage_proofs(u.ptr, u.n)
    assert one == eight == canon
    assert cl.tobytes() == cl2.tobytes()
    # a refusal in the sixth range of eight and one in the second: the lower one, whatever thread finds it first
    c = cl.copy()
    c["flags"][6000] = 0
    c["state_root"][1500] = 0
    assert refusal(c) == (E_INVALID, 1500)
    monkeypatch.setenv("IPCFP_HOST_THREADS", "1")
    assert refusal(c) == (E_INVALID, 1500)
