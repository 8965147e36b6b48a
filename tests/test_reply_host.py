"""CPU checks of the Retry / Version Negotiation assembly.

aioquic_amd/csrc/qpp_reply.h, what every lane of k_reply runs, is built for
the host with g++ (tests/reply_host.cc) and compared -- the candidate's 256
bytes, both descriptors and the reply record, byte for byte -- with the Python
restatement of tests/reply_cases.py, which is written from the reference's
encoders.  Its generic pseudo-packet builder plus the C oracle's AES-128-GCM
reproduces the Retry packets of RFC 9001 A.4 and RFC 9369 A.4.  The same
file's main(), built with -fsanitize=address,undefined and run as a program of
its own, is the out-of-bounds check: every buffer a lane may touch lives on
the heap at exactly its size.
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from aioquic_amd import layout as L
from tests import reply_cases as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "reply_host.cc")
u32, u64, vp, cp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_char_p
POISON = 0x5A


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("reply_host") / "libreply_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.rp_reply.restype = None
    lib.rp_reply.argtypes = [u32, u32, u32, u32, u32, cp, u32, cp, cp, u64, vp, u32, u32, vp, vp, vp, vp]
    lib.rp_pseudo.restype = u32
    lib.rp_pseudo.argtypes = [vp, u32, u32, cp, u32, cp, u32, cp, u32, cp, u32]
    return lib


def poisoned(dtype):
    return np.full(dtype.itemsize, POISON, np.uint8).view(dtype)


def run(lib, a, status, w, data, addr20, rnd, ctr, versions, flags):
    """The host build's outputs, each over poisoned memory, next to the
    restatement's; returns (region, seal, tag, rec) of the host build."""
    region = np.full(R.STRIDE, POISON, np.uint8)
    seal, tag, rec = poisoned(L.DESC), poisoned(L.DESC), poisoned(L.REPLY)
    vs = np.asarray(versions, np.uint32)
    lib.rp_reply(a, status, w["version"], w["dcid_len"], w["scid_len"], data, len(data), addr20, rnd, ctr,
                 vs.ctypes.data, len(vs), flags, region.ctypes.data, seal.ctypes.data, tag.ctypes.data,
                 rec.ctypes.data)
    want = R.restate(a, status, w, data, addr20, rnd, ctr, versions, flags)
    assert region.tobytes() == want[0]
    assert seal.tobytes() == want[1].tobytes() and tag.tobytes() == want[2].tobytes()
    assert rec.tobytes() == want[3].tobytes()
    return region.tobytes(), seal, tag, rec


def test_spelled_out_cases(lib):
    kinds, statuses = set(), set()
    rnd = bytes(range(0xB0, 0xC0))
    for k, (name, status, w, data, addr, versions, flags) in enumerate(R.spelled_cases()):
        a = 1 + k % 5
        region, seal, tag, rec = run(lib, a, status, w, data, R.addr20_of(addr), rnd, 7 << 40 | k, versions, flags)
        kind, st = int(rec["kind"][0]), int(rec["status"][0])
        kinds.add(kind), statuses.add(st)
        if name.startswith("retry-") and kind == L.RP_KIND_RETRY:
            assert st == L.RP_OK and int(tag["hdr_len"][0]) + 16 <= 145, name
        if name.startswith(("silent", "no-flags", "vn-flag-off", "retry-flag-off")):
            assert (kind, st) == (L.RP_KIND_NONE, L.RP_OK) and region == bytes(R.STRIDE), name
        if name in ("dl-21", "sl-21", "cut-vn", "cut-retry", "dl-disagrees", "sl-disagrees", "retry-dl-0",
                    "retry-odd-version"):
            assert (kind, st) == (L.RP_KIND_NONE, L.RP_BOUNDS), name
        if name in ("retry-no-address", "retry-address-5", "retry-address-19"):
            assert (kind, st) == (L.RP_KIND_NONE, L.RP_ADDR), name
        if name in ("vn-ends-at-cids", "retry-ends-at-cids"):
            assert kind != L.RP_KIND_NONE, name
    assert kinds == {L.RP_KIND_NONE, L.RP_KIND_VN, L.RP_KIND_RETRY}
    assert statuses == {L.RP_OK, L.RP_BOUNDS, L.RP_ADDR}


def test_spelled_out_fields(lib):
    """One Retry and one Version Negotiation against numbers written by hand."""
    dcid, scid, rnd = bytes(range(0x11, 0x19)), bytes(range(0x21, 0x25)), bytes(range(0xA0, 0xB0))
    data = R.header(R.V2, dcid, scid, 1200, first=0xD0)
    region, seal, tag, rec = run(lib, 2, L.ACC_NO_TOKEN, R.walk_of(data), data, R.packed_addr(R.IPV4), rnd, 5,
                                 [R.V1, R.V2], L.RP_RETRY)
    tok = 1 + 8 + 7 + 4 + 8
    plain = bytes([6, 192, 0, 2, 33, 0x11, 0x51, 8]) + dcid + bytes([8]) + rnd[:8]
    assert region[:tok] == bytes([8]) + dcid + bytes([0xC0]) + R.V2.to_bytes(4, "big") + bytes([4]) + scid + \
        bytes([8]) + rnd[:8]
    assert region[tok:tok + 8 + len(plain)] == (7).to_bytes(8, "big") + plain
    assert region[tok + 8 + len(plain):] == bytes(R.STRIDE - tok - 8 - len(plain))
    assert (int(seal["in_off"][0]), int(seal["len"][0]), int(seal["hdr_len"][0]), int(seal["pn"][0]),
            int(seal["slot"][0]), int(seal["flags"][0])) == (512 + tok, len(plain), 8, 7, 2, L.F_NO_HP)
    assert (int(tag["in_off"][0]), int(tag["len"][0]), int(tag["hdr_len"][0]), int(tag["pn"][0]),
            int(tag["slot"][0])) == (512, 0, tok + 8 + len(plain) + 16, 0, 1)
    assert (int(rec["off"][0]), int(rec["len"][0]), int(rec["kind"][0])) == \
        (512 + 9, 7 + 4 + 8 + 8 + len(plain) + 16 + 16, L.RP_KIND_RETRY)

    data = R.header(R.GREASE, b"", scid, 1200)
    region, seal, tag, rec = run(lib, 0, L.ACC_VERSION, R.walk_of(data), data, None, rnd, 0, [R.V1, 0xFF00001D],
                                 L.RP_VN)
    assert region[:19] == bytes([0x80 | 0x28, 0, 0, 0, 0, 4]) + scid + bytes([0]) + R.V1.to_bytes(4, "big") + \
        bytes.fromhex("ff00001d")
    assert (int(rec["off"][0]), int(rec["len"][0]), int(rec["kind"][0])) == (0, 19, L.RP_KIND_VN)
    assert int(seal["slot"][0]) == int(tag["slot"][0]) == R.NONE


def test_restatement_against_the_oracle_round_trip():
    """The sealed token of the restatement opens again with the oracle, and a
    Retry is what the repo's own parser reads."""
    from aioquic_amd.buffer import Buffer
    from aioquic_amd.packet import QuicPacketType, pull_quic_header
    from oracle import oracle as orc

    data = R.header(R.V1, R.cid(1, 8), R.cid(2, 5), 1200)
    rnd = bytes(range(16))
    region, seal, tag, rec = R.restate(4, L.ACC_NO_TOKEN, R.walk_of(data), data, R.packed_addr(R.IPV6), rnd, 99,
                                       [R.V1], L.RP_RETRY)
    done, r_seal, r_tag = R.launches(region, seal, tag, 4 * R.STRIDE)
    assert int(r_seal["status"][0]) == int(r_tag["status"][0]) == L.S_OK
    packet = R.reply_bytes(done, rec, 4 * R.STRIDE)
    header = pull_quic_header(Buffer(data=packet), host_cid_length=8)
    assert header.packet_type == QuicPacketType.RETRY and header.version == R.V1
    assert (header.destination_cid, header.source_cid) == (R.cid(2, 5), rnd[:8])
    ctr = int.from_bytes(header.token[:8], "big")
    assert ctr == 99 + 4
    plain = orc.aead_decrypt(L.AES_128_GCM, R.TOKEN_KEY, R.TOKEN_IV, header.token[8:], header.token[:8], ctr)
    assert plain == R.token_plain(R.packed_addr(R.IPV6)[1:19], R.cid(1, 8), rnd[:8])


# RFC 9001 A.4 and RFC 9369 A.4: the client's original DCID, and the Retry
# packet with the token "token", the unused bits 0xf and an empty DCID
ODCID = bytes.fromhex("8394c8f03e515708")
RFC_RETRY = {
    R.V1: bytes.fromhex("ff000000010008f067a5502a4262b5746f6b656e04a265ba2eff4d829058fb3f0f2496ba"),
    R.V2: bytes.fromhex("cf6b3343cf0008f067a5502a4262b5746f6b656ec8646ce8bfe33952d955543665dcc7b6"),
}


@pytest.mark.parametrize("version", [R.V1, R.V2])
def test_generic_builder_reproduces_the_rfc_retry_packets(lib, version):
    from oracle import oracle as orc

    out = np.full(64, POISON, np.uint8)
    scid = bytes.fromhex("f067a5502a4262b5")
    n = lib.rp_pseudo(out.ctypes.data, version, 0xF, ODCID, 8, b"", 0, scid, 8, b"token", 5)
    pseudo = out[:n].tobytes()
    assert n == 1 + 8 + 7 + 8 + 5 and (out[n:] == POISON).all()
    assert pseudo == bytes([8]) + ODCID + R.encode_retry_without_tag(version, scid, b"", b"token", unused=0xF)
    key, nonce = R.RETRY_KEYS[L.RP_SLOT_V2 if version == R.V2 else L.RP_SLOT_V1]
    tag = orc.aead_encrypt(L.AES_128_GCM, key, nonce, b"", pseudo, 0)
    assert pseudo[9:] + tag == RFC_RETRY[version]


def test_token_handler_surface_without_a_device():
    """What RetryTokens does before any cipher runs: counters, the plaintext,
    the address encoding, the short-token refusal."""
    from aioquic_amd.retry import RetryTokens, encode_address, packed_address

    t = RetryTokens(R.TOKEN_KEY, R.TOKEN_IV)
    assert [t.take(3), t.take(0), t.take(1), t.take(5)] == [0, 3, 3, 4] and t.take(1) == 9
    assert RetryTokens(counter=(1 << 64) - 3).take(2) == (1 << 64) - 3
    with pytest.raises(OverflowError):
        RetryTokens(counter=(1 << 64) - 3).take(3)
    assert encode_address(R.IPV4) == bytes([192, 0, 2, 33, 0x11, 0x51])
    assert packed_address(R.IPV6)[0] == 18 and len(packed_address(R.IPV6)) == len(packed_address(R.IPV4)) == 20
    assert t.plaintext(R.IPV4, b"\x01\x02", b"\x03" * 8) == R.token_plain(encode_address(R.IPV4), b"\x01\x02",
                                                                          b"\x03" * 8)
    with pytest.raises(ValueError):
        t.validate_token(R.IPV4, bytes(26))
    with pytest.raises(ValueError):
        RetryTokens(key=bytes(15))
    recs = t.key_records()
    assert recs["slot"].tolist() == [0, 1, 2] and (recs["suite"] == L.AES_128_GCM).all()
    assert recs["key"][2, :16].tobytes() == R.TOKEN_KEY and recs["iv"][2].tobytes() == R.TOKEN_IV


def test_sanitizer_program(tmp_path):
    """The assembly under AddressSanitizer and UBSan, as a program of its own:
    a datagram that ends at 7 + dl + sl, every truncation of it, walk records
    that disagree with the bytes, each on heap buffers of exactly their size."""
    exe = str(tmp_path / "reply_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "reply_host: ok" in r.stdout
