"""CPU: the formatting primitives of csrc/kernels/claim_text_dev.h — decimal, "0x" hex, base32-lower, base58btc, the CID a
slot holds — compiled as host C++ into a stand-alone program (tests/native/claim_text_harness.cpp) that runs as a child
process, plain and under AddressSanitizer + UBSan, and is held to Python: str(), bytes.hex(), pystorage.cid_to_string and
bundle_ref.cid_check over the value lists of tests/bundle_packed_cases.py and 2 000 seeded random values of each kind."""
import os
import subprocess

import numpy as np
import pytest

from conftest import fuzz_seed

import bundle_packed_cases as cases
import bundle_ref
import pystorage

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "claim_text_harness.cpp")
HDR = os.path.join(HERE, "..", "ipc-filecoin-proofs_amd", "csrc", "kernels", "claim_text_dev.h")
BUILDS = {"plain": ["-O2"], "asan": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def harness_exe(kind):
    exe = os.path.join(HERE, "native", "claim_text_harness" + ("" if kind == "plain" else "_" + kind))
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *BUILDS[kind], "-o", exe, SRC], check=True)
    return exe


def run(kind, lines):
    p = subprocess.run([harness_exe(kind)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=False)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout.splitlines()
    assert len(out) == len(lines)
    return [o.split(" ") for o in out]


def slot_expect(raw: bytes):
    """(length, string) of the one CID in front of zero padding; 0: none; -1: a fold"""
    if raw[0] == 0xFF:
        return -1, None
    for n in range(1, 41):
        if any(raw[n:]):
            continue
        try:
            bundle_ref.cid_check(raw[:n])
        except bundle_ref.BundleError:
            continue
        return n, pystorage.cid_to_string(raw[:n])
    return 0, None


@pytest.fixture(scope="module")
def rng():
    return np.random.default_rng(fuzz_seed(0xC7E7))


@pytest.mark.parametrize("kind", list(BUILDS))
def test_integers(kind, rng):
    u = list(cases.UINTS) + [int(rng.integers(0, 2**63)) << int(rng.integers(0, 2)) >> int(rng.integers(0, 64)) for _ in range(2000)]
    i = list(cases.EPOCHS) + [int(rng.integers(-2**63, 2**63)) >> int(rng.integers(0, 64)) for _ in range(2000)]
    for tag, vals in (("u", u), ("i", i)):
        got = run(kind, ["%s %d" % (tag, v) for v in vals])
        for v, g in zip(vals, got):
            assert g == [str(len(str(v))), str(v), str(v)], v


@pytest.mark.parametrize("kind", list(BUILDS))
def test_hex(kind, rng):
    vals = [b"", b"\x00", b"\xff", bytes(range(256))] + [rng.integers(0, 256, int(rng.integers(0, 80)), dtype=np.uint8).tobytes()
                                                        for _ in range(2000)]
    got = run(kind, ["x %s" % (v.hex() or "-") for v in vals])
    for v, g in zip(vals, got):
        assert g == ["0x" + v.hex()] * 2, v


@pytest.mark.parametrize("kind", list(BUILDS))
def test_cid_slots(kind, rng):
    slots = [bytes(cases.slot(c)) for c in cases.SOUND_CIDS + [cases.FOLDED, cases.TRAILING, cases.TRUNCATED]]
    slots += [bytes(40), b"\x01" + bytes(39), b"\x12\x20" + bytes(37) + b"\x01", b"\x12" + bytes(39),
              bytes.fromhex("0155") + b"\x80\x00" + bytes(36),          # a non-minimal varint
              bytes.fromhex("01550041") + bytes(36),                    # digest size 65 > 64
              bytes.fromhex("02711220") + bytes(36)]                    # version 2
    for _ in range(2000):
        mode = int(rng.integers(0, 6))
        d = rng.integers(0, 256, 40, dtype=np.uint8).tobytes()
        if mode == 0:  # CIDv0
            s = b"\x12\x20" + d[:32] + bytes(6)
        elif mode == 1:  # every length 1-40 of a one-byte-varint CIDv1: 4 header bytes + a digest of 0-36
            n = int(rng.integers(0, 37))
            s = bytes([1, int(rng.integers(0, 128)), int(rng.integers(0, 128)), n]) + d[:n]
        elif mode == 2:  # multi-byte codec and multihash code
            n = int(rng.integers(0, 33))
            s = b"\x01" + bytes([0x80 | int(rng.integers(0, 128)), int(rng.integers(1, 128))]) + bytes.fromhex("a0e402") + bytes([n]) + d[:n]
        elif mode == 3:  # a sound CID with one byte changed
            s = bytearray(cases.slot(cases.SOUND_CIDS[int(rng.integers(0, len(cases.SOUND_CIDS)))]))
            s[int(rng.integers(0, 40))] = int(rng.integers(0, 256))
            s = bytes(s)
        elif mode == 4:  # noise in front of zeros
            s = d[: int(rng.integers(0, 8))]
        else:
            s = d
        slots.append((s + bytes(40))[:40])
    got = run(kind, ["c %s" % s.hex() for s in slots])
    seen = set()
    for s, g in zip(slots, got):
        n, text = slot_expect(s)
        seen.add(n)
        assert g == ([str(n)] if n <= 0 else [str(n), str(len(text)), text, text]), s.hex()
    assert seen >= set(range(4, 41)) | {0, -1}  # every length a CIDv1 can have in a slot, hence every base32 tail
