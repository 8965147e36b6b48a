"""Shared by tests/test_walk_host.py and tests/test_gpu_walk.py: the Python
restatement of the device header walk (quic_pp.h: qpp_route_walk), built on
oracle.receive_walk.parse_header, and the hand-built datagrams both tests walk.
"""

from __future__ import annotations

from oracle import receive_walk as W

WALK_MAX, MAX_HDR = 4, 1500
W_OK, W_PARSE, W_HOST = 0, 1, 2
TYPE = {"INITIAL": 0, "ZERO_RTT": 1, "HANDSHAKE": 2, "RETRY": 3, "VERSION_NEGOTIATION": 4, "ONE_RTT": 5}
V1, V2, GREASE = 0x00000001, 0x6B3343CF, 0x1A2A3A4A
FIELDS = ("off", "len", "version", "pn_off", "token_len", "type", "status", "dcid_len", "scid_len")


def _varint_at(data: bytes, pos: int):
    """(value, size) of the varint at pos of a header that parsed."""
    n = 1 << (data[pos] >> 6)
    return int.from_bytes(data[pos:pos + n], "big") & ((1 << (8 * n - 2)) - 1), n


def restate_walk(data: bytes, cid_len: int) -> list:
    """The records of qpp_route_walk for one datagram, as dicts of FIELDS: a
    loop of parse_header as oracle.receive_walk.receive runs it, with the
    walk's own rules (at most WALK_MAX packets, pn_off <= MAX_HDR)."""
    recs = []
    pos = 0
    while pos < len(data):
        if len(recs) == WALK_MAX:
            recs[-1]["status"] = W_HOST  # a fifth packet follows
            break
        try:
            h = W.parse_header(data, pos, cid_len)
        except W.ParseError:
            recs.append(dict(off=pos, len=0, version=0, pn_off=0, token_len=0, type=TYPE["ONE_RTT"], status=W_PARSE,
                             dcid_len=0, scid_len=0))
            break
        t = TYPE[h.packet_type]
        pn_off = 0 if h.packet_type in ("RETRY", "VERSION_NEGOTIATION") else h.encrypted_offset
        scid_len = token_len = 0
        if data[pos] & 0x80:
            at = pos + 6 + len(h.destination_cid)
            scid_len = data[at]
            if h.packet_type == "INITIAL":
                token_len, _ = _varint_at(data, at + 1 + scid_len)
        status = W_HOST if pn_off > MAX_HDR else W_OK
        recs.append(dict(off=pos, len=h.packet_length, version=h.version or 0, pn_off=min(pn_off, 0xFFFF),
                         token_len=min(token_len, 0xFFFF), type=t, status=status,
                         dcid_len=len(h.destination_cid), scid_len=scid_len))
        if status != W_OK:
            break
        pos += h.packet_length
    return recs


def varint(v: int, form: int) -> bytes:
    """v in the varint form of 1 << form bytes."""
    n = 1 << form
    assert v < 1 << (8 * n - 2)
    return (v | form << (8 * n - 2)).to_bytes(n, "big")


def long_packet(first: int, version: int, dcid: bytes, scid: bytes, token=None, tform: int = 0, body: bytes = b"",
                length=None, lform: int = 1) -> bytes:
    """flags version dcid scid [token length, token] Length body; Length =
    len(body) unless given."""
    out = bytes([first]) + version.to_bytes(4, "big") + bytes([len(dcid)]) + dcid + bytes([len(scid)]) + scid
    if token is not None:
        out += varint(len(token), tform) + token
    out += varint(len(body) if length is None else length, lform)
    return out + body


def hand_cases(cid: bytes = b"\xC1" * 8) -> list:
    """[(name, datagram)]: the header forms and edge cases of the walk, for an
    endpoint whose CIDs have len(cid) bytes."""
    cl = len(cid)
    scid = b"\x5C" * 8
    body = bytes(range(64))
    cases = []

    def add(name, data):
        cases.append((name, bytes(data)))

    ini = long_packet(0xC1, V1, cid, scid, token=b"tok", body=body * 4)
    hs = long_packet(0xE1, V1, cid, scid, body=body * 3)
    zr = long_packet(0xD1, V1, cid, scid, body=body * 2)
    short = bytes([0x41]) + cid + body
    co = ini + hs + zr + short
    co += bytes(range(256)) * 5
    co = co[:1200]
    add("coalesced-1200", co)
    for cut in range(0, len(co) + 1, 7):
        add("coalesced-cut-%d" % cut, co[:cut])
    for cut in (1, 5, 6, 6 + cl, 7 + cl, len(ini) - 1, len(ini), len(ini) + 1, len(ini) + len(hs) - 1,
                len(ini) + len(hs) + len(zr), len(ini) + len(hs) + len(zr) + 1, len(ini) + len(hs) + len(zr) + cl,
                len(ini) + len(hs) + len(zr) + cl + 1, 1199):
        add("coalesced-cut-%d" % cut, co[:cut])
    # token length and Length in all four varint forms
    for tf in range(4):
        for lf in range(4):
            p = long_packet(0xC0, V1, cid, b"", token=b"T" * 33, tform=tf, body=body[:48], lform=lf)
            add("varint-t%d-l%d" % (tf, lf), p)
            add("varint-t%d-l%d-short" % (tf, lf), p[:-1])
            add("varint-t%d-l%d-then-short" % (tf, lf), p + short)
    # Length = 2^62 - 1 and Length = remaining + 1, in a first and in a second packet
    big = long_packet(0xE0, V1, cid, scid, body=body, length=(1 << 62) - 1, lform=3)
    over = long_packet(0xE0, V1, cid, scid, body=body, length=len(body) + 1)
    tbig = bytes([0xC0]) + V1.to_bytes(4, "big") + bytes([cl]) + cid + b"\x00" + varint((1 << 62) - 1, 3) + body
    tover = bytes([0xC0]) + V1.to_bytes(4, "big") + bytes([cl]) + cid + b"\x00" + varint(len(body) + 1, 1) + body
    for name, p in (("length-max", big), ("length-over", over), ("token-max", tbig), ("token-over", tover)):
        add(name, p)
        add("second-" + name, hs + p)
    # DCID / SCID lengths 0, 20, 21
    for dl in (0, 20, 21):
        for sl in (0, 20, 21):
            hdr = bytes([0xE0]) + V1.to_bytes(4, "big") + bytes([dl]) + b"\xD1" * dl + bytes([sl]) + b"\x51" * sl
            add("cids-%d-%d" % (dl, sl), hdr + varint(len(body), 1) + body)
            add("cids-%d-%d-cut" % (dl, sl), hdr[:-1])
    # the fixed bit clear on long, short (second position) and Version Negotiation
    add("long-no-fixed", long_packet(0x80, V1, cid, scid, body=body))
    add("short-no-fixed", hs + bytes([0x01]) + cid + body)
    vn = bytes([0x80]) + bytes(4) + bytes([cl]) + cid + bytes([8]) + scid + V1.to_bytes(4, "big")
    add("vn-no-fixed", vn)
    add("vn-fixed", bytes([0xC0]) + vn[1:])
    add("vn-odd-tail", vn + b"\x00\x01\x02")
    add("vn-second", hs + vn)
    # type codes of v2 and of a grease version (the v1 table)
    for bits in range(4):
        for ver in (V1, V2, GREASE):
            first = 0xC0 | bits << 4
            tail = b"\x9A" * 24
            is_initial = bits == (1 if ver == V2 else 0)
            add("type-%d-%08x" % (bits, ver),
                long_packet(first, ver, cid, scid, token=b"" if is_initial else None, body=tail))
    # Retry with 15 and 16 bytes after the CIDs
    rt = bytes([0xF0]) + V1.to_bytes(4, "big") + bytes([cl]) + cid + bytes([8]) + scid
    add("retry-15", rt + bytes(15))
    add("retry-16", rt + bytes(16))
    add("retry-token", rt + b"token" + bytes(16))
    add("retry-second", hs + rt + bytes(16))
    # trailing zero padding after a long packet, a short packet at the end and one a byte short of its CID
    add("padding-zeros", hs + bytes(40))
    add("short-after-long", hs + short)
    add("short-cut", hs + short[:cl])
    add("short-exact", hs + short[:cl + 1])
    # two to five coalesced packets
    tiny = long_packet(0xE0, V1, cid, scid, body=b"\x07" * 24)
    for k in (2, 3, 4, 5, 6):
        add("coalesced-x%d" % k, tiny * k)
    add("coalesced-x3-short", tiny * 3 + short)
    add("coalesced-x4-short", tiny * 4 + short)
    add("coalesced-x4-garbage", tiny * 4 + b"\x00")
    # a token that pushes pn_off to 1500 and to 1501
    base = len(long_packet(0xC0, V1, cid, scid, token=b"", tform=1, body=b""))
    for want in (1500, 1501):
        p = long_packet(0xC0, V1, cid, scid, token=b"t" * (want - base), tform=1, body=body)
        assert W.parse_header(p, 0, cl).encrypted_offset == want
        add("pn-off-%d" % want, p)
        add("pn-off-%d-second" % want, hs + p)
    add("one-byte", b"\xC0")
    add("five-bytes", b"\xC0\x00\x00\x00\x01")
    return cases
