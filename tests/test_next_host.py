"""CPU checks of the next-key-phase lane.

aioquic_amd/csrc/qpp_next.h, what every lane of k_derive_next computes and the
record check qpp_keytab_derive_next runs before it launches, is built for the
host with g++ (tests/next_host.cc) and compared with a stdlib hmac restatement
of next_key_phase (quic/crypto.py:148-168): "quic ku" for both versions, key
and iv of the updated secret, the header-protection key kept.  The same file's
main(), built with -fsanitize=address,undefined and run as a program of its
own, is the out-of-bounds check: its records and outputs live in heap buffers
of exactly their sizes.
"""

import ctypes
import hashlib
import hmac
import os
import struct
import subprocess

import numpy as np
import pytest

from aioquic_amd import layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "next_host.cc")
u32, vp = ctypes.c_uint32, ctypes.c_void_p

# RFC 9001 A.5: the ChaCha20-Poly1305 secret and its "quic ku" output
A5_SECRET = bytes.fromhex("9ac312a7f877468ebe69422748ad00a15443f18203a07d6060f688f30f21632b")
A5_KU = bytes.fromhex("1223504755036d556342ee9361d253421a826c9ecdf3c7148684b36b714881f9")


def expand_label(hashfn, secret: bytes, label: bytes, length: int) -> bytes:
    """HKDF-Expand-Label(secret, label, "", length), RFC 8446 sec. 7.1 over RFC 5869."""
    full = b"tls13 " + label
    info = struct.pack("!HB", length, len(full)) + full + b"\x00"
    out, t, i = b"", b"", 1
    while len(out) < length:
        t = hmac.new(secret, t + info + bytes([i]), hashfn).digest()
        out += t
        i += 1
    return out[:length]


def restate(suite: int, v2: bool, secret: bytes, hp: bytes):
    """(secret', key, iv, hp) of the next phase, unpadded."""
    hashfn = hashlib.sha384 if suite == L.AES_256_GCM else hashlib.sha256
    klen = 16 if suite == L.AES_128_GCM else 32
    nxt = expand_label(hashfn, secret, b"quic ku", hashfn().digest_size)
    pre = b"quicv2 " if v2 else b"quic "
    return nxt, expand_label(hashfn, nxt, pre + b"key", klen), expand_label(hashfn, nxt, pre + b"iv", 12), hp[:klen]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("next_host") / "libnext_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.nx_lane.restype = None
    lib.nx_lane.argtypes = [vp, vp, vp]
    lib.nx_check.restype = u32
    lib.nx_check.argtypes = [vp, u32]
    return lib


def run_lane(lib, rec):
    km = np.full(1, 0xA5, np.uint8).repeat(L.KEY_MATERIAL.itemsize).view(L.KEY_MATERIAL)
    sec = np.full(64, 0xA5, np.uint8)
    lib.nx_lane(rec.ctypes.data, km.ctypes.data, sec.ctypes.data)
    return km[0], sec.tobytes()


def test_rfc9001_a5_on_the_cpu(lib):
    """The key-update vector of RFC 9001 A.5 against the restatement and the lane."""
    assert expand_label(hashlib.sha256, A5_SECRET, b"quic ku", 32) == A5_KU
    rec = L.next_phase_record(L.SLOT_NONE, L.CHACHA20_POLY1305, A5_SECRET, bytes(32), key_phase=1)
    km, sec = run_lane(lib, rec)
    assert sec == A5_KU + bytes(32)
    _, key, iv, _ = restate(L.CHACHA20_POLY1305, False, A5_SECRET, bytes(32))
    assert km["key"].tobytes() == key and km["iv"].tobytes() == iv


@pytest.mark.parametrize("suite", [L.AES_128_GCM, L.AES_256_GCM, L.CHACHA20_POLY1305])
@pytest.mark.parametrize("v2", [False, True])
def test_lane_matches_restatement(lib, suite, v2):
    rng = np.random.default_rng(100 + 2 * suite + v2)
    for slen in (1, 32, 48, 64):
        for fill in (0x00, 0xFF):
            for phase in (0, 1):
                secret = rng.integers(0, 256, slen, dtype=np.uint8).tobytes()
                hp = bytes([fill]) * 32
                slot = L.SLOT_NONE if phase else 5
                rec = L.next_phase_record(slot, suite, secret, hp, key_phase=phase, v2=v2)
                # what lies past secret_len is not the lane's to read
                rec["secret"][0, slen:] = 0xEE
                km, sec = run_lane(lib, rec)
                nxt, key, iv, hp_kept = restate(suite, v2, secret, hp)
                assert sec == nxt.ljust(64, b"\x00"), (slen, fill)
                want = L.key_material(slot, suite, key, iv, hp_kept, phase)[0]
                assert km.tobytes() == want.tobytes(), (slen, fill, phase)


def test_check_each_refusal_alone(lib):
    cap = 8

    def ok(**change):
        rec = L.next_phase_record(3, L.CHACHA20_POLY1305, bytes(range(48)), bytes(32), key_phase=1, v2=True)
        for k, v in change.items():
            rec[k] = v
        return bool(lib.nx_check(rec.ctypes.data, cap))

    assert ok()
    assert ok(slot=0) and ok(slot=cap - 1) and ok(slot=L.SLOT_NONE)
    assert not ok(slot=cap) and not ok(slot=L.SLOT_NONE - 1)
    assert ok(suite=0) and ok(suite=1) and not ok(suite=3) and not ok(suite=0xFF)
    assert ok(secret_len=1) and ok(secret_len=64) and not ok(secret_len=0) and not ok(secret_len=65)
    assert ok(key_phase=0) and not ok(key_phase=2) and not ok(key_phase=0xFF)
    assert ok(flags=0) and not ok(flags=2) and not ok(flags=3) and not ok(flags=0x80)


def test_sanitizer_program(tmp_path):
    """The lane under AddressSanitizer and UBSan, as a program of its own:
    three suites, both versions, secrets of 1, 32, 48 and 64 bytes, records and
    outputs each on a heap buffer of exactly its size."""
    exe = str(tmp_path / "next_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "next_host: ok" in r.stdout
