"""Shared by tests/test_reply_host.py and tests/test_gpu_reply.py: the Python
restatement of what a server sends instead of accepting an unrouted Initial
(quic_pp.h: qpp_route_reply), written from the reference's encoders --
encode_quic_version_negotiation and encode_quic_retry (quic/packet.py:288-334),
QuicRetryTokenHandler.create_token's buffer (quic/retry.py:25-28) -- with the
C oracle's aead_encrypt for the token's seal and the Retry integrity tag, and
the synthetic candidates both tests run.
"""

from __future__ import annotations

import numpy as np

from aioquic_amd import layout as L
from aioquic_amd.packet import (RETRY_AEAD_KEY_VERSION_1, RETRY_AEAD_KEY_VERSION_2, RETRY_AEAD_NONCE_VERSION_1,
                                RETRY_AEAD_NONCE_VERSION_2)

V1, V2, GREASE = 0x00000001, 0x6B3343CF, 0x0A0A0A0A
NONE = 0xFFFFFFFF
STRIDE = 256
RETRY_KEYS = {L.RP_SLOT_V1: (RETRY_AEAD_KEY_VERSION_1, RETRY_AEAD_NONCE_VERSION_1),
              L.RP_SLOT_V2: (RETRY_AEAD_KEY_VERSION_2, RETRY_AEAD_NONCE_VERSION_2)}
TOKEN_KEY = bytes(range(0x40, 0x50))
TOKEN_IV = bytes(range(0x70, 0x7C))
IPV4 = ("192.0.2.33", 4433)
IPV6 = ("2001:db8::8a2e:370:7334", 50001)
# the statuses of qpp_route_accept that never get a reply
SILENT = (L.ACC_OK, L.ACC_ROUTED, L.ACC_NOT_INITIAL, L.ACC_SMALL, L.ACC_CID)


# ------------------------------------------------ the reference's encoders ----


def encode_vn(first: int, source_cid: bytes, destination_cid: bytes, versions) -> bytes:
    """packet.py:317-334, the random byte given."""
    return (bytes([first | 0x80]) + bytes(4) + bytes([len(destination_cid)]) + destination_cid
            + bytes([len(source_cid)]) + source_cid + b"".join(int(v).to_bytes(4, "big") for v in versions))


def encode_retry_without_tag(version: int, source_cid: bytes, destination_cid: bytes, token: bytes,
                             unused: int = 0) -> bytes:
    """packet.py:288-309: everything the integrity tag is appended to."""
    code = 0 if version == V2 else 3  # PACKET_LONG_TYPE_ENCODE_VERSION_*[RETRY]
    return (bytes([0x80 | 0x40 | code << 4 | unused]) + version.to_bytes(4, "big") + bytes([len(destination_cid)])
            + destination_cid + bytes([len(source_cid)]) + source_cid + token)


def opaque(b: bytes) -> bytes:
    return bytes([len(b)]) + bytes(b)


def token_plain(encoded_addr: bytes, odcid: bytes, retry_scid: bytes) -> bytes:
    """retry.py:25-28."""
    return opaque(encoded_addr) + opaque(odcid) + opaque(retry_scid)


def packed_addr(addr) -> bytes:
    from aioquic_amd.retry import packed_address

    return packed_address(addr)


# -------------------------------------------------------- the restatement ----


def inert(base: int) -> np.ndarray:
    d = np.zeros(1, L.DESC)
    d["in_off"] = d["out_off"] = base
    d["flags"], d["slot"] = L.F_NO_HP, NONE
    return d


def restate(a: int, status: int, w: dict, data: bytes, addr20, rnd: bytes, token_ctr: int, versions, flags: int):
    """Candidate a before the two launches: (its 256 bytes, seal descriptor,
    tag descriptor, reply record).  w: packet 0's walk record (version,
    dcid_len, scid_len); addr20: its 20 address bytes or None; rnd: its 16."""
    base = a * STRIDE
    region = bytearray(STRIDE)
    seal, tag = inert(base), inert(base)
    rec = np.zeros(1, L.REPLY)
    rec["off"] = base
    vn = status == L.ACC_VERSION and flags & L.RP_VN
    retry = status == L.ACC_NO_TOKEN and flags & L.RP_RETRY
    if not (vn or retry):
        return bytes(region), seal, tag, rec
    dl, sl = w["dcid_len"], w["scid_len"]
    if dl > 20 or sl > 20 or 7 + dl + sl > len(data) or data[5] != dl or data[6 + dl] != sl:
        rec["status"] = L.RP_BOUNDS
        return bytes(region), seal, tag, rec
    dcid, scid = data[6:6 + dl], data[7 + dl:7 + dl + sl]
    if vn:
        pkt = encode_vn(rnd[8] & 0x7F, dcid, scid, versions)  # server.py:77-81
        region[:len(pkt)] = pkt
        rec["len"], rec["kind"] = len(pkt), L.RP_KIND_VN
        return bytes(region), seal, tag, rec
    if dl < 1 or w["version"] not in (V1, V2):
        rec["status"] = L.RP_BOUNDS
        return bytes(region), seal, tag, rec
    alen = addr20[0] if addr20 is not None else 0
    if alen not in (6, 18):
        rec["status"] = L.RP_ADDR
        return bytes(region), seal, tag, rec
    retry_scid = rnd[:8]  # server.py:98
    ctr = (token_ctr + a) & 0xFFFFFFFFFFFFFFFF
    plain = token_plain(addr20[1:1 + alen], dcid, retry_scid)
    token = ctr.to_bytes(8, "big") + plain + bytes(16)  # not sealed yet
    packet = encode_retry_without_tag(w["version"], retry_scid, scid, token)  # server.py:100-108
    pseudo = bytes([dl]) + dcid + packet  # RFC 9001 sec. 5.8
    region[:len(pseudo)] = pseudo
    tok = len(pseudo) - len(token)
    seal["in_off"] = seal["out_off"] = base + tok
    seal["len"], seal["hdr_len"], seal["pn"], seal["slot"] = len(plain), 8, ctr, L.RP_SLOT_TOKEN
    tag["hdr_len"], tag["slot"] = len(pseudo), L.RP_SLOT_V2 if w["version"] == V2 else L.RP_SLOT_V1
    rec["off"], rec["len"], rec["kind"] = base + 1 + dl, len(packet) + 16, L.RP_KIND_RETRY
    return bytes(region), seal, tag, rec


def launches(region: bytes, seal, tag, base: int, token_key: bytes = TOKEN_KEY, token_iv: bytes = TOKEN_IV):
    """What the two qpp_protect launches leave of a candidate: (its 256 bytes,
    the seal's result, the tag's result)."""
    from oracle import oracle as orc

    r = bytearray(region)
    res = np.zeros(2, L.RESULT)
    res["status"] = L.S_NO_KEY
    if int(seal["slot"][0]) != NONE:
        o, n, pn = int(seal["in_off"][0]) - base, int(seal["len"][0]), int(seal["pn"][0])
        r[o + 8:o + 8 + n + 16] = orc.aead_encrypt(L.AES_128_GCM, token_key, token_iv, bytes(r[o + 8:o + 8 + n]),
                                                    bytes(r[o:o + 8]), pn)
        res[0] = (pn, L.S_OK, 8, 8 + n + 16)
    if int(tag["slot"][0]) != NONE:
        key, nonce = RETRY_KEYS[int(tag["slot"][0])]
        h = int(tag["hdr_len"][0])
        r[h:h + 16] = orc.aead_encrypt(L.AES_128_GCM, key, nonce, b"", bytes(r[:h]), 0)
        res[1] = (0, L.S_OK, h, h + 16)
    return bytes(r), res[0:1], res[1:2]


def reply_bytes(region: bytes, rec, base: int) -> bytes:
    at = int(rec["off"][0]) - base
    return region[at:at + int(rec["len"][0])]


# ------------------------------------------------------------- candidates ----


def header(version: int, dcid: bytes, scid: bytes, size: int = 0, first: int = 0xC0) -> bytes:
    """A long header's invariant part, then filler up to `size` bytes."""
    h = bytes([first]) + version.to_bytes(4, "big") + bytes([len(dcid)]) + dcid + bytes([len(scid)]) + scid
    return h + bytes((0x90 + k) & 0xFF for k in range(max(0, size - len(h))))


def walk_of(data: bytes, version=None) -> dict:
    """The fields of packet 0's walk record the reply needs, from the bytes."""
    dl = data[5]
    return {"version": int.from_bytes(data[1:5], "big") if version is None else version, "dcid_len": dl,
            "scid_len": data[6 + dl]}


def cid(seed: int, n: int) -> bytes:
    return bytes((seed * 37 + 11 * k + 1) & 0xFF for k in range(n))


def spelled_cases() -> list:
    """[(name, accept status, walk record, datagram, address or None,
    versions, reply_flags)]: both replies over the CID lengths and address
    families, and every reason for none, each alone."""
    both = L.RP_VN | L.RP_RETRY
    two = [V1, V2]
    out = []

    def add(name, status, data, addr=IPV4, versions=two, flags=both, w=None):
        out.append((name, status, walk_of(data) if w is None else w, data, addr, list(versions), flags))

    for version in (V1, V2):
        for dl in (1, 8, 20):
            for sl in (0, 8, 20):
                for addr in (IPV4, IPV6):
                    add("retry-%x-%d-%d-%d" % (version, dl, sl, len(addr[0])), L.ACC_NO_TOKEN,
                        header(version, cid(dl, dl), cid(sl + 3, sl), 7 + dl + sl + 5), addr)
    for dl in (0, 1, 8, 20):
        for sl in (0, 8, 20):
            add("vn-%d-%d" % (dl, sl), L.ACC_VERSION, header(GREASE, cid(dl + 1, dl), cid(sl + 2, sl), 64))
    g = header(GREASE, cid(5, 8), cid(6, 8), 40)
    r = header(V1, cid(7, 8), cid(8, 8), 40)
    add("vn-1-version", L.ACC_VERSION, g, versions=[V1])
    add("vn-16-versions", L.ACC_VERSION, g, versions=[0x1000 + k for k in range(16)])
    add("vn-ends-at-cids", L.ACC_VERSION, g[:7 + 16])
    add("retry-ends-at-cids", L.ACC_NO_TOKEN, r[:7 + 16])
    for st in SILENT:
        add("silent-%d" % st, st, r)
    add("vn-flag-off", L.ACC_VERSION, g, flags=L.RP_RETRY)
    add("retry-flag-off", L.ACC_NO_TOKEN, r, flags=L.RP_VN)
    add("no-flags-vn", L.ACC_VERSION, g, flags=0)
    add("no-flags-retry", L.ACC_NO_TOKEN, r, flags=0)
    # the reasons for QPP_RP_BOUNDS, each alone
    add("dl-21", L.ACC_VERSION, g, w=dict(walk_of(g), dcid_len=21))
    add("sl-21", L.ACC_NO_TOKEN, r, w=dict(walk_of(r), scid_len=21))
    add("cut-vn", L.ACC_VERSION, g[:7 + 16 - 1])
    add("cut-retry", L.ACC_NO_TOKEN, r[:7 + 16 - 1], w=walk_of(r))
    add("dl-disagrees", L.ACC_NO_TOKEN, r, w=dict(walk_of(r), dcid_len=7))
    add("sl-disagrees", L.ACC_VERSION, g, w=dict(walk_of(g), scid_len=9))
    add("retry-dl-0", L.ACC_NO_TOKEN, header(V1, b"", cid(9, 8), 40))
    add("retry-odd-version", L.ACC_NO_TOKEN, g)
    # and for QPP_RP_ADDR
    add("retry-no-address", L.ACC_NO_TOKEN, r, addr=None)
    add("retry-address-5", L.ACC_NO_TOKEN, r, addr=bytes([5]) + bytes(19))
    add("retry-address-19", L.ACC_NO_TOKEN, r, addr=bytes([19]) + bytes(19))
    return out


def addr20_of(addr):
    """A case's address: None, 20 packed bytes as they are, or a (host, port)."""
    if addr is None or isinstance(addr, (bytes, bytearray)):
        return addr
    return packed_addr(addr)


def synthetic(n_acc: int, seed: int = 19):
    """n_acc candidates for the device form, one datagram each, mixing both
    replies, every silent status and the bounds failures: (datagrams, the
    bytes that follow each in the buffer, accept statuses, walk records,
    20-byte addresses, 16 random bytes each).  What follows a datagram that
    ends inside its CIDs is the rest of its header: read, it would make a
    whole one."""
    rng = np.random.default_rng(seed + n_acc)
    kinds = rng.integers(0, 10, n_acc)
    dls, sls = rng.integers(1, 21, n_acc), rng.integers(0, 21, n_acc)
    rnd = rng.integers(0, 256, (n_acc, 16), dtype=np.uint8)
    v6 = rng.integers(0, 2, n_acc)
    datagrams, tails, statuses, walks, addrs = [], [], [], [], []
    for a in range(n_acc):
        k, dl, sl = int(kinds[a]), int(dls[a]), int(sls[a])
        size = 7 + dl + sl + int(rng.integers(0, 40))
        addr = packed_addr(("2001:db8::%x" % (a + 1), 1024 + a % 60000) if v6[a] else
                           ("198.51.%d.%d" % (a >> 8 & 255, a & 255), 1024 + a % 60000))
        tail = b""
        if k < 4:       # a Retry of version 1 or 2
            data, st = header(V2 if k & 1 else V1, cid(a, dl), cid(a + 1, sl), size), L.ACC_NO_TOKEN
        elif k < 7:     # a Version Negotiation, now and then to an empty DCID
            dl = 0 if k == 6 and a % 3 == 0 else dl
            data, st = header(GREASE + a, cid(a, dl), cid(a + 1, sl), size), L.ACC_VERSION
        elif k == 7:    # nothing to say
            data, st = header(V1, cid(a, dl), cid(a + 1, sl), size), SILENT[a % len(SILENT)]
        elif k == 8:    # the datagram ends inside its CIDs
            whole, st = header(V1, cid(a, dl), cid(a + 1, sl), size), L.ACC_NO_TOKEN
            data, tail = whole[:6 + dl + sl], whole[6 + dl + sl:]
        else:           # the record disagrees with the bytes
            data, st = header(GREASE, cid(a, dl), cid(a + 1, sl), size), L.ACC_VERSION
        w = {"version": int.from_bytes(data[1:5], "big"), "dcid_len": dl, "scid_len": sl}
        if k == 9:
            w["scid_len"] = (sl + 1) % 21
        datagrams.append(data), tails.append(tail), statuses.append(st), walks.append(w), addrs.append(addr)
    return datagrams, tails, statuses, walks, addrs, rnd
