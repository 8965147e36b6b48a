"""Shared by tests/test_accept_host.py and tests/test_gpu_accept.py: the Python
restatement of the device's new-connection decision (quic_pp.h:
qpp_route_accept) over the restated walk of tests/walk_cases.py, and the
spelled-out datagrams both tests decide on.
"""

from __future__ import annotations

import numpy as np

from aioquic_amd import layout as L
from tests import walk_cases as C

NONE = 0xFFFFFFFF
MIN_DATAGRAM = 1200  # asyncio/server.py:91


def restate_status(route, recs: list, length: int, accept_flags: int) -> int:
    """The verdict: the first failing test of quic_pp.h's list names it.
    route = (conn, cls) of the datagram, recs = its restated walk."""
    if route != (NONE, L.R_LONG):
        return L.ACC_ROUTED
    if not recs or (recs[0]["status"], recs[0]["type"], recs[0]["off"]) != (C.W_OK, C.TYPE["INITIAL"], 0):
        return L.ACC_NOT_INITIAL
    w = recs[0]
    if w["version"] not in (C.V1, C.V2):
        return L.ACC_VERSION
    if length < MIN_DATAGRAM:
        return L.ACC_SMALL
    if not 1 <= w["dcid_len"] <= 20 or 6 + w["dcid_len"] > length:
        return L.ACC_CID
    if accept_flags & L.A_NEED_TOKEN and w["token_len"] == 0:
        return L.ACC_NO_TOKEN
    return L.ACC_OK


def restate(data: bytes, i: int, off: int, route, recs: list, slot_client: int, slot_server: int,
            accept_flags: int, desc_flags: int):
    """(qpp_initial, qpp_desc or None, qpp_accept_rec) of one candidate, as
    one-element numpy records."""
    st = restate_status(route, recs, len(data), accept_flags)
    ini = np.zeros(1, L.INITIAL)
    acc = np.zeros(1, L.ACCEPT)
    ini["slot_client"] = ini["slot_server"] = NONE
    acc["desc"], acc["status"] = NONE, st
    if st != L.ACC_OK:
        return ini, None, acc
    w = recs[0]
    v2 = w["version"] == C.V2
    ini["slot_client"], ini["slot_server"] = slot_client, slot_server
    ini["cid_len"], ini["flags"] = w["dcid_len"], L.DERIVE_V2 if v2 else 0
    ini["cid"][0, :w["dcid_len"]] = np.frombuffer(data[6:6 + w["dcid_len"]], np.uint8)
    desc = np.zeros(1, L.DESC)
    desc["in_off"] = desc["out_off"] = off
    desc["len"], desc["hdr_len"], desc["flags"], desc["slot"] = w["len"], w["pn_off"], desc_flags, slot_client
    acc["desc"], acc["version"] = i, 1 if v2 else 0
    return ini, desc, acc


def initial(version: int, dcid: bytes, size: int, token: bytes = b"", scid: bytes = b"\x5C" * 8,
            fill: int = 0xA7) -> bytes:
    """An Initial-shaped packet of exactly `size` bytes (its Length covers the
    rest of the datagram); nothing in it is encrypted."""
    first = 0xD0 if version == C.V2 else 0xC0
    head = C.long_packet(first, version, dcid, scid, token=token, body=b"", length=0, lform=1)[:-2]
    body = size - len(head) - 2
    assert body >= 0
    return head + C.varint(body, 1) + bytes([fill]) * body


def spelled_cases() -> list:
    """[(name, datagram, route, accept_flags, expected status)]: every
    QPP_ACC_* status at its boundary."""
    d8 = b"\xD8" * 8
    long_none = (NONE, L.R_LONG)
    out = []

    def add(name, data, want, route=long_none, flags=0):
        out.append((name, bytes(data), route, flags, want))

    add("v1-1200", initial(C.V1, d8, 1200), L.ACC_OK)
    add("v2-1200", initial(C.V2, d8, 1200), L.ACC_OK)
    add("v1-1199", initial(C.V1, d8, 1199), L.ACC_SMALL)
    add("v1-1500", initial(C.V1, d8, 1500), L.ACC_OK)
    add("grease-1200", initial(C.GREASE, d8, 1200), L.ACC_VERSION)
    add("grease-1199", initial(C.GREASE, d8, 1199), L.ACC_VERSION)
    add("dcid-0", initial(C.V1, b"", 1200), L.ACC_CID)
    add("dcid-1", initial(C.V1, b"\x01", 1200), L.ACC_OK)
    add("dcid-20", initial(C.V2, bytes(range(1, 21)), 1200), L.ACC_OK)
    add("token-0", initial(C.V1, d8, 1200), L.ACC_OK)
    add("token-0-need", initial(C.V1, d8, 1200), L.ACC_NO_TOKEN, flags=L.A_NEED_TOKEN)
    add("token-1", initial(C.V1, d8, 1200, token=b"t"), L.ACC_OK)
    add("token-1-need", initial(C.V2, d8, 1200, token=b"t"), L.ACC_OK, flags=L.A_NEED_TOKEN)
    add("dcid-0-need", initial(C.V1, b"", 1200), L.ACC_CID, flags=L.A_NEED_TOKEN)
    add("small-need", initial(C.V1, d8, 1199), L.ACC_SMALL, flags=L.A_NEED_TOKEN)
    # a connection, or another class: never the accepting step's business
    add("routed", initial(C.V1, d8, 1200), L.ACC_ROUTED, route=(3, L.R_LONG))
    add("bad-conn", initial(C.V1, d8, 1200), L.ACC_ROUTED, route=(9, L.R_BAD_CONN))
    add("short-unknown", b"\x41" + d8 + bytes(1300), L.ACC_ROUTED, route=(NONE, L.R_UNKNOWN_CID))
    # long headers to an unknown DCID that are no Initial at the datagram's start
    hs = C.long_packet(0xE0, C.V1, d8, b"", body=bytes(1250))
    zr = C.long_packet(0xD0, C.V1, d8, b"", body=bytes(1250))
    add("handshake", hs, L.ACC_NOT_INITIAL)
    add("zero-rtt", zr, L.ACC_NOT_INITIAL)
    vn = bytes([0x80]) + bytes(4) + bytes([8]) + d8 + bytes([0]) + C.V1.to_bytes(4, "big") * 300
    add("version-negotiation", vn, L.ACC_NOT_INITIAL)
    add("retry", bytes([0xF0]) + C.V1.to_bytes(4, "big") + bytes([8]) + d8 + bytes([0]) + bytes(1300),
        L.ACC_NOT_INITIAL)
    add("parse-error", initial(C.V1, d8, 1200)[:-1] + b"", L.ACC_NOT_INITIAL)
    add("no-fixed-bit", b"\x80" + initial(C.V1, d8, 1200)[1:], L.ACC_NOT_INITIAL)
    big = C.long_packet(0xC0, C.V1, d8, b"", token=b"t" * 1490, tform=1, body=bytes(64))
    add("host-walk", big, L.ACC_NOT_INITIAL)
    # an Initial followed by a 0-RTT packet: packet 0 decides
    co = initial(C.V1, d8, 700) + C.long_packet(0xD0, C.V1, d8, b"", body=bytes(500))
    add("coalesced", co, L.ACC_OK if len(co) >= 1200 else L.ACC_SMALL)
    return out
