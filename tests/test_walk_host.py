"""CPU checks of the header parsers.

aioquic_amd/csrc/qpp_walk.h, the walk every lane of k_walk runs, is built for
the host with g++ (tests/walk_host.cc) and compared, datagram by datagram,
with a loop of oracle.receive_walk.parse_header (tests/walk_cases.restate_walk).
The same file's main(), built with -fsanitize=address,undefined and run as a
program of its own, is the out-of-bounds check of the walk: its inputs live in
heap buffers of exactly the datagram's size.

tests/golden/header_cases.json holds the reference's own pull_quic_header
expectations (tests/golden/make_header_cases.py); the three parsers of the
project -- aioquic_amd.packet.pull_quic_header, oracle.receive_walk.parse_header
and qpp_walk.h -- are checked against it.
"""

import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import receive_walk as W
from tests import receive_scenario as RS
from tests import walk_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "walk_host.cc")
WALK = np.dtype([("off", "<u4"), ("len", "<u4"), ("version", "<u4"), ("desc", "<u4"), ("pn_off", "<u2"),
                 ("token_len", "<u2"), ("type", "u1"), ("status", "u1"), ("dcid_len", "u1"), ("scid_len", "u1")])
u32, vp, cp = ctypes.c_uint32, ctypes.c_void_p, ctypes.c_char_p


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("walk_host") / "libwalk_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.wk_walk.restype = u32
    lib.wk_walk.argtypes = [cp, u32, u32, vp]
    lib.wk_parse_one.restype = None
    lib.wk_parse_one.argtypes = [cp, u32, u32, u32, vp]
    lib.wk_keyset_of.restype = u32
    lib.wk_keyset_of.argtypes = [u32, u32]
    lib.wk_space_of.restype = u32
    lib.wk_space_of.argtypes = [u32]
    return lib


def walk(lib, data: bytes, cid_len: int) -> list:
    rec = np.zeros(C.WALK_MAX, WALK)
    rec["desc"] = 0x55555555
    n = lib.wk_walk(data, len(data), cid_len, rec.ctypes.data)
    assert n <= C.WALK_MAX
    assert (rec["desc"][:n] == 0xFFFFFFFF).all(), "no descriptor is the header's to name"
    return [{f: int(rec[f][k]) for f in C.FIELDS} for k in range(n)]


def check(lib, data: bytes, cid_len: int, name=""):
    want = C.restate_walk(data, cid_len)
    got = walk(lib, data, cid_len)
    assert got == want, (name, data[:48].hex(), len(data))
    return got


def test_layout_matches_the_package():
    from aioquic_amd import layout as L

    assert L.WALK == WALK
    assert (L.WALK_MAX, L.KEYSETS, L.SPACES, L.DESC_NONE) == (4, 5, 3, 0xFFFFFFFF)
    assert (L.W_OK, L.W_PARSE, L.W_HOST) == (C.W_OK, C.W_PARSE, C.W_HOST)
    assert L.MAX_HDR == C.MAX_HDR


def test_hand_built_cases(lib):
    seen = set()
    for name, data in C.hand_cases():
        for r in check(lib, data, 8, name):
            seen.add((r["type"], r["status"]))
    # every type parsed, a parse error and both ways to QPP_W_HOST were met
    assert {(t, C.W_OK) for t in range(6)} <= seen
    assert (5, C.W_PARSE) in seen and (0, C.W_HOST) in seen and (2, C.W_HOST) in seen


@pytest.mark.parametrize("cid_len", [1, 4, 20])
def test_other_cid_lengths(lib, cid_len):
    for name, data in C.hand_cases(bytes([0xC1]) * cid_len):
        check(lib, data, cid_len, name)


def test_spelled_out(lib):
    cid, scid = b"\xC1" * 8, b"\x5C" * 8
    hs = C.long_packet(0xE1, C.V1, cid, scid, body=bytes(40))
    (r,) = walk(lib, hs, 8)
    assert (r["off"], r["len"], r["version"], r["pn_off"], r["type"], r["status"]) == (0, len(hs), 1, 25, 2, 0)
    assert (r["dcid_len"], r["scid_len"], r["token_len"]) == (8, 8, 0)
    # Length = 2^62 - 1 and Length = remaining + 1: "Packet payload is truncated", nothing moved
    for length, form in (((1 << 62) - 1, 3), (41, 1)):
        (r,) = walk(lib, C.long_packet(0xE1, C.V1, cid, scid, body=bytes(40), length=length, lform=form), 8)
        assert (r["off"], r["len"], r["status"], r["type"]) == (0, 0, C.W_PARSE, 5)
    # five packets: the fourth says "host"; four and a short one: fine
    tiny = C.long_packet(0xE0, C.V1, cid, scid, body=bytes(24))
    assert [r["status"] for r in walk(lib, tiny * 5, 8)] == [0, 0, 0, C.W_HOST]
    assert [r["status"] for r in walk(lib, tiny * 4, 8)] == [0, 0, 0, 0]
    assert [r["type"] for r in walk(lib, tiny * 3 + b"\x40" + cid, 8)] == [2, 2, 2, 5]
    # Version Negotiation: no fixed-bit check, to the datagram's end, pn_off 0
    vn = b"\x80" + bytes(4) + b"\x08" + cid + b"\x08" + scid + b"\x00\x00\x00\x01"
    (r,) = walk(lib, vn, 8)
    assert (r["type"], r["len"], r["pn_off"], r["version"], r["status"]) == (4, len(vn), 0, 0, 0)
    # v2 and grease type codes
    for ver, bits, want in ((C.V2, 1, 0), (C.V2, 2, 1), (C.V2, 3, 2), (C.V2, 0, 3), (C.GREASE, 0, 0),
                            (C.GREASE, 2, 2), (C.V1, 3, 3)):
        p = C.long_packet(0xC0 | bits << 4, ver, cid, scid, token=b"" if want == 0 else None, body=bytes(24))
        assert walk(lib, p, 8)[0]["type"] == want, (hex(ver), bits)
    # the key-set and the space of a packet
    assert [lib.wk_keyset_of(0, v) for v in (C.V1, C.V2, C.GREASE, 0)] == [0, 1, 0xFFFFFFFF, 0xFFFFFFFF]
    assert [lib.wk_keyset_of(t, C.V1) for t in range(6)] == [0, 2, 3, 0xFFFFFFFF, 0xFFFFFFFF, 4]
    assert [lib.wk_space_of(t) for t in (0, 1, 2, 5)] == [0, 2, 1, 2]


def test_every_truncation_of_a_coalesced_datagram(lib):
    name, co = C.hand_cases()[0]
    assert name == "coalesced-1200" and len(co) == 1200
    full = check(lib, co, 8)
    assert [r["type"] for r in full] == [0, 2, 1, 5] and full[-1]["off"] + full[-1]["len"] == 1200
    for cut in range(len(co) + 1):
        got = check(lib, co[:cut], 8, "cut %d" % cut)
        # a parse error, or a shorter valid walk
        assert len(got) <= len(full)
        assert all(r["status"] == C.W_OK for r in got[:-1])
        assert all(r["off"] + r["len"] <= cut for r in got)


def test_scenario_datagrams(lib):
    for client in (False, True):
        _, items = RS.build(client=client)
        for _, data in items:
            check(lib, data, 8)


def test_parse_one_at_positions(lib):
    """parse_one at every position of a coalesced datagram, against parse_header there."""
    _, co = C.hand_cases()[0]
    co = co[:700]
    rec = np.zeros(1, WALK)
    for pos in range(len(co)):
        lib.wk_parse_one(co, len(co), pos, 8, rec.ctypes.data)
        try:
            h = W.parse_header(co, pos, 8)
        except W.ParseError:
            assert rec["status"][0] == C.W_PARSE and rec["len"][0] == 0, pos
            continue
        if C.TYPE[h.packet_type] in (3, 4) or h.encrypted_offset > C.MAX_HDR:
            continue
        assert (rec["status"][0], rec["len"][0], rec["pn_off"][0], rec["type"][0]) == \
            (C.W_OK, h.packet_length, h.encrypted_offset, C.TYPE[h.packet_type]), pos


def test_sanitizer_program(tmp_path):
    """The walk under AddressSanitizer and UBSan, as a program of its own:
    every truncation of a coalesced datagram and the varint cases, each on a
    heap buffer of exactly its size."""
    exe = str(tmp_path / "walk_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "walk_host: ok" in r.stdout


# ----------------------------------------------------- the reference's cases --

def _cases():
    with open(os.path.join(ROOT, "tests", "golden", "header_cases.json")) as f:
        return json.load(f)["cases"]


CASES = _cases()
_ids = [c["name"] for c in CASES]


def test_fixture_is_complete():
    assert len(CASES) == 15
    assert sum(1 for c in CASES if c["error"]) == 7
    assert {c["expect"].get("packet_type") for c in CASES if not c["error"]} == \
        {"INITIAL", "RETRY", "VERSION_NEGOTIATION", "ONE_RTT"}


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_product_parser_against_the_reference_cases(case):
    from aioquic_amd.buffer import Buffer
    from aioquic_amd.packet import QuicPacketType, pull_quic_header

    buf = Buffer(data=bytes.fromhex(case["data"]))
    if case["error"]:
        with pytest.raises(ValueError) as e:  # BufferReadError is a ValueError
            pull_quic_header(buf, host_cid_length=case["host_cid_length"])
        if case["error_text"]:
            assert str(e.value) == case["error_text"]
        return
    h = pull_quic_header(buf, host_cid_length=case["host_cid_length"])
    for k, v in case["expect"].items():
        got = getattr(h, k)
        if k == "packet_type":
            assert got == QuicPacketType[v]
        elif isinstance(got, bytes):
            assert got.hex() == v, k
        else:
            assert got == v, k
    assert buf.tell() == case["tell"]


def _applies(case):
    # the walks are given a CID length: every case but the two Retry ones has one (Retry needs none)
    return 8 if case["host_cid_length"] is None else case["host_cid_length"]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_oracle_parser_against_the_reference_cases(case):
    data = bytes.fromhex(case["data"])
    if case["error"]:
        with pytest.raises(W.ParseError) as e:
            W.parse_header(data, 0, _applies(case))
        if case["error_text"]:
            assert str(e.value) == case["error_text"]
        return
    h = W.parse_header(data, 0, _applies(case))
    x = case["expect"]
    assert h.version == x["version"] and h.packet_type == x["packet_type"]
    assert h.packet_length == x["packet_length"] and h.destination_cid.hex() == x["destination_cid"]
    if h.packet_type != "VERSION_NEGOTIATION":  # the reference's cursor reads the version list too
        assert h.encrypted_offset == case["tell"]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_device_walk_against_the_reference_cases(lib, case):
    data = bytes.fromhex(case["data"])
    got = check(lib, data, _applies(case), case["name"])
    if not data:
        assert got == []
        return
    r = got[0]
    if case["error"]:
        assert (r["status"], r["off"], r["len"]) == (C.W_PARSE, 0, 0) and len(got) == 1
        return
    x = case["expect"]
    assert r["status"] == C.W_OK
    assert r["version"] == (x["version"] or 0) and r["type"] == C.TYPE[x["packet_type"]]
    assert r["len"] == x["packet_length"]
    assert r["dcid_len"] == len(x["destination_cid"]) // 2 and r["scid_len"] == len(x["source_cid"]) // 2
    if x["packet_type"] in ("RETRY", "VERSION_NEGOTIATION"):
        assert r["pn_off"] == 0 and len(got) == 1
    else:
        assert r["pn_off"] == case["tell"]
    if x["packet_type"] == "INITIAL":
        assert r["token_len"] == len(x["token"]) // 2
