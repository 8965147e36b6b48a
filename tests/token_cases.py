"""Shared by tests/test_token_host.py and tests/test_gpu_token.py: the Python
restatement of the device's Retry-token validation (quic_pp.h:
qpp_route_token, qpp_route_accept_tokens), written from
aioquic_amd/retry.py's validate_token and the varint rules of RFC 9000 sec. 16,
with the C oracle's aead_decrypt standing in for the launch that opens the
tokens, and the synthetic candidates both tests run.
"""

from __future__ import annotations

import numpy as np

from aioquic_amd import layout as L
from tests import accept_cases as A
from tests import reply_cases as R
from tests import walk_cases as C

V1, V2 = R.V1, R.V2
NONE = 0xFFFFFFFF
STRIDE = L.TOKEN_STRIDE
TOKEN_KEY, TOKEN_IV = R.TOKEN_KEY, R.TOKEN_IV
OTHER_KEY = bytes(range(0x10, 0x20))
IPV4, IPV6 = R.IPV4, R.IPV6
ALL_TK = {L.TK_OK, L.TK_NONE, L.TK_LENGTH, L.TK_BOUNDS, L.TK_AUTH, L.TK_FORM, L.TK_ADDR}
LONG_NONE = (NONE, L.R_LONG)


# ----------------------------------------------------------------- tokens ----


def seal(ctr: int, plain: bytes, key: bytes = TOKEN_KEY, iv: bytes = TOKEN_IV) -> bytes:
    """retry.py: counter | AEAD(plaintext, aad = counter, pn = counter)."""
    from oracle import oracle as orc

    head = ctr.to_bytes(8, "big")
    return head + orc.aead_encrypt(L.AES_128_GCM, key, iv, plain, head, ctr)


def token_for(ctr: int, addr, odcid: bytes, rscid: bytes, **kw) -> bytes:
    from aioquic_amd.retry import encode_address

    return seal(ctr, R.token_plain(encode_address(addr), odcid, rscid), **kw)


def initial(version: int, dcid: bytes, scid: bytes, token: bytes, tform: int = 0, size: int = 1200) -> bytes:
    """An Initial-shaped datagram of `size` bytes around `token`, its length in
    the varint form of 1 << tform bytes (two at least past 63); nothing in it
    is encrypted.  With size 0 the datagram ends where the token ends."""
    first = 0xD0 if version == V2 else 0xC0
    tform = max(tform, 1) if len(token) > 63 else tform
    head = C.long_packet(first, version, dcid, scid, token=token, tform=tform, body=b"", length=0, lform=1)[:-2]
    if size == 0:
        return head
    body = size - len(head) - 2
    assert body >= 0
    return head + C.varint(body, 1) + bytes((0x31 + k) & 0xFF for k in range(body))


def walk_of(data: bytes) -> dict:
    """Packet 0's walk record as the device walk leaves it."""
    return C.restate_walk(data, 8)[0]


# -------------------------------------------------------- the restatement ----


def restate_locate(data: bytes, dl: int, sl: int, token_len: int):
    """Where the token starts, or None: every bound against len(data)."""
    if dl > 20 or sl > 20 or 7 + dl + sl > len(data) or data[5] != dl or data[6 + dl] != sl:
        return None
    pos = 7 + dl + sl
    if pos >= len(data):
        return None
    n = 1 << (data[pos] >> 6)  # RFC 9000 sec. 16: the two high bits give the length
    if pos + n > len(data):
        return None
    v = int.from_bytes(data[pos:pos + n], "big") & ((1 << (8 * n - 2)) - 1)
    pos += n
    if v != token_len or pos + token_len > len(data):
        return None
    return pos


def inert(a: int, off: int) -> np.ndarray:
    d = np.zeros(1, L.DESC)
    d["in_off"], d["out_off"] = off, a * STRIDE
    d["flags"], d["slot"] = L.F_NO_HP, NONE
    return d


def restate_desc(a: int, acc_status: int, accept_flags: int, w: dict, off: int, data: bytes):
    """(the token's descriptor, its preliminary TK_* status)."""
    d = inert(a, off)
    if acc_status != L.ACC_OK or not accept_flags & L.A_NEED_TOKEN:
        return d, L.TK_NONE
    tl = w["token_len"]
    if not L.TOKEN_MIN <= tl <= L.TOKEN_MAX:
        return d, L.TK_LENGTH
    start = restate_locate(data, w["dcid_len"], w["scid_len"], tl)
    if start is None:
        return d, L.TK_BOUNDS
    d["in_off"], d["len"], d["hdr_len"] = off + start, tl, 8  # AEAD.decrypt: aad | ciphertext | tag
    d["pn"], d["slot"] = int.from_bytes(data[start:start + 8], "big"), L.RP_SLOT_TOKEN
    return d, L.TK_OK


def restate_open(desc, off: int, data: bytes, key: bytes = TOKEN_KEY, iv: bytes = TOKEN_IV):
    """What the launch leaves of one descriptor: (result status, the
    candidate's STRIDE bytes: [counter | plaintext] when it opened)."""
    from oracle import oracle as orc

    if int(desc["slot"][0]) == NONE:
        return L.S_NO_KEY, bytes(STRIDE)
    at, n = int(desc["in_off"][0]) - off, int(desc["len"][0])
    token = data[at:at + n]
    try:
        plain = orc.aead_decrypt(L.AES_128_GCM, key, iv, token[8:], token[:8], int(desc["pn"][0]))
    except ValueError:
        return L.S_DECRYPT, bytes(STRIDE)
    return L.S_OK, (token[:8] + plain).ljust(STRIDE, b"\0")


def token_rec(status: int, odcid: bytes = b"", rscid: bytes = b"") -> np.ndarray:
    r = np.zeros(1, L.TOKEN_REC)
    r["status"], r["odcid_len"], r["rscid_len"] = status, len(odcid), len(rscid)
    r["odcid"][0, :len(odcid)] = np.frombuffer(odcid, np.uint8)
    r["rscid"][0, :len(rscid)] = np.frombuffer(rscid, np.uint8)
    return r


def restate_check(pre: int, res_status: int, token_len: int, opened: bytes, addr20: bytes) -> np.ndarray:
    """The final qpp_token_rec: validate_token after its decrypt, with the two
    divergences quic_pp.h names."""
    if pre != L.TK_OK:
        return token_rec(pre)
    if not L.TOKEN_MIN <= token_len <= L.TOKEN_MAX:
        return token_rec(L.TK_LENGTH)
    if res_status != L.S_OK:
        return token_rec(L.TK_AUTH)
    body = opened[8:8 + token_len - 24]
    fields, at = [], 0
    for _ in range(3):
        if at >= len(body) or at + 1 + body[at] > len(body):
            return token_rec(L.TK_FORM)
        fields.append(body[at + 1:at + 1 + body[at]])
        at += 1 + body[at]
    if len(fields[1]) > 20 or len(fields[2]) > 20:
        return token_rec(L.TK_FORM)
    if addr20[0] not in (6, 18) or fields[0] != addr20[1:1 + addr20[0]]:
        return token_rec(L.TK_ADDR)
    return token_rec(L.TK_OK, fields[1], fields[2])


def restate_accept(data: bytes, i: int, off: int, route, recs: list, slot_client: int, slot_server: int,
                   accept_flags: int, desc_flags: int, trec: np.ndarray):
    """qpp_route_accept's records (accept_cases.restate) under the token's
    verdict: (qpp_initial, qpp_desc or None, qpp_accept_rec, qpp_token_rec)."""
    ini, desc, acc = A.restate(data, i, off, route, recs, slot_client, slot_server, accept_flags, desc_flags)
    tested = int(acc["status"][0]) == L.ACC_OK and accept_flags & L.A_NEED_TOKEN
    if not tested:
        return ini, desc, acc, token_rec(L.TK_NONE)
    if int(trec["status"][0]) == L.TK_OK:
        return ini, desc, acc, trec
    ini, acc = np.zeros(1, L.INITIAL), np.zeros(1, L.ACCEPT)
    ini["slot_client"] = ini["slot_server"] = NONE
    acc["desc"], acc["status"] = NONE, L.ACC_BAD_TOKEN
    return ini, None, acc, trec


# ------------------------------------------------------------------ cases ----

DCID, SCID, ODCID, RSCID = R.cid(3, 8), R.cid(4, 5), R.cid(5, 11), R.cid(6, 8)


def plain_of(addr, odcid: bytes = ODCID, rscid: bytes = RSCID) -> bytes:
    from aioquic_amd.retry import encode_address

    return R.token_plain(encode_address(addr), odcid, rscid)


def spelled_cases() -> list:
    """[(name, datagram, walk record, accept status, accept_flags, 20 address
    bytes, forced result status or None, expected TK_*)].  The token is opened
    by the oracle under TOKEN_KEY unless a result status is forced; then the
    opened bytes are those of the valid token all the same."""
    need = L.A_NEED_TOKEN
    out = []

    def add(name, want, token=None, *, plain=None, tform=0, size=1200, data=None, w=None, acc=L.ACC_OK,
            flags=need, addr=IPV4, forced=None, version=V1):
        if data is None:
            if token is None:
                token = seal(77 + len(out), plain_of(IPV4) if plain is None else plain)
            data = initial(version, DCID, SCID, token, tform, size)
        rec = walk_of(data) if w is None else w
        a20 = addr if isinstance(addr, (bytes, bytearray)) else R.packed_addr(addr)
        out.append((name, data, rec, acc, flags, bytes(a20), forced, want))

    pad = lambda n: seal(5, plain_of(IPV4) + bytes(n - 24 - len(plain_of(IPV4))))
    # lengths: 26 and 129 are never opened; 27 is the shortest (three empty opaques)
    add("len-26", L.TK_LENGTH, seal(1, b"\0\0"))
    add("len-27-empty-fields", L.TK_ADDR, seal(1, b"\0\0\0"))
    add("len-85-largest-issued", L.TK_OK, seal(2, plain_of(IPV6, R.cid(7, 20), R.cid(8, 20))), addr=IPV6)
    add("len-128", L.TK_OK, pad(128))
    add("len-129", L.TK_LENGTH, pad(129))
    # the length's varint in three encodings of the same value
    for tform in (0, 1, 2):
        add("varint-%d" % (1 << tform), L.TK_OK, tform=tform, version=V2 if tform == 1 else V1)
    # a token that ends exactly at the datagram's end, and every truncation of it
    # (the walk would not pass such a datagram on, no Length follows: the record is written by hand)
    whole = initial(V1, DCID, SCID, seal(9, plain_of(IPV4)), 1, 0)
    w_whole = dict(dcid_len=len(DCID), scid_len=len(SCID), token_len=8 + len(plain_of(IPV4)) + 16)
    add("ends-at-end", L.TK_OK, data=whole, w=w_whole)
    for cut in range(len(whole)):
        add("cut-%d" % cut, L.TK_BOUNDS, data=whole[:cut], w=w_whole)
    # the record against the bytes
    d = initial(V1, DCID, SCID, seal(10, plain_of(IPV4)))
    add("dl-disagrees", L.TK_BOUNDS, data=d, w=dict(walk_of(d), dcid_len=7))
    add("sl-disagrees", L.TK_BOUNDS, data=d, w=dict(walk_of(d), scid_len=6))
    add("dl-21", L.TK_BOUNDS, data=d, w=dict(walk_of(d), dcid_len=21))
    add("sl-21", L.TK_BOUNDS, data=d, w=dict(walk_of(d), scid_len=21))
    add("token-len-disagrees", L.TK_BOUNDS, data=d, w=dict(walk_of(d), token_len=walk_of(d)["token_len"] + 1))
    # candidates the accepting step does not bring to the token test
    add("no-token-test-status", L.TK_NONE, data=d, acc=L.ACC_NO_TOKEN)
    add("no-token-test-small", L.TK_NONE, data=d, acc=L.ACC_SMALL)
    add("no-token-test-flag", L.TK_NONE, data=d, flags=0)
    # plaintexts: each field one byte past the end, a missing field, no body at all, trailing bytes
    ok = plain_of(IPV4)
    add("field-0-past-end", L.TK_FORM, plain=bytes([6, 1, 2, 3, 4, 5]))
    add("field-1-past-end", L.TK_FORM, plain=ok[:7] + bytes([4, 1, 2, 3]))
    add("field-2-past-end", L.TK_FORM, plain=ok[:-1])
    add("field-2-missing", L.TK_FORM, plain=ok[:7 + 12])
    add("empty-body", L.TK_LENGTH, seal(11, b""))  # 24 bytes: shorter than any plaintext of three opaques allows
    add("trailing-bytes", L.TK_OK, plain=ok + b"\xEE" * 9)
    add("cid-21-odcid", L.TK_FORM, plain=plain_of(IPV4, R.cid(1, 21), RSCID))
    add("cid-21-rscid", L.TK_FORM, plain=plain_of(IPV4, ODCID, R.cid(2, 21)))
    add("cid-20-both", L.TK_OK, plain=plain_of(IPV4, R.cid(1, 20), R.cid(2, 20)))
    add("cid-0-both", L.TK_OK, plain=plain_of(IPV4, b"", b""))
    # addresses: 6 and 18 bytes that match, that differ in the last port byte, that differ only in length
    add("addr-6", L.TK_OK, plain=plain_of(IPV4), addr=IPV4)
    add("addr-18", L.TK_OK, plain=plain_of(IPV6), addr=IPV6)
    add("addr-6-port", L.TK_ADDR, plain=plain_of(IPV4), addr=(IPV4[0], IPV4[1] ^ 1))
    add("addr-18-port", L.TK_ADDR, plain=plain_of(IPV6), addr=(IPV6[0], IPV6[1] ^ 1))
    p18 = R.packed_addr(IPV6)
    add("addr-length-only", L.TK_ADDR, plain=R.token_plain(p18[1:7], ODCID, RSCID), addr=p18)
    add("addr-length-only-longer", L.TK_ADDR, plain=plain_of(IPV6), addr=bytes([6]) + p18[1:])
    add("addr-record-19", L.TK_ADDR, plain=R.token_plain(p18[1:20], ODCID, RSCID), addr=bytes([19]) + p18[1:])  # equal
    add("addr-record-255", L.TK_ADDR, plain=plain_of(IPV4), addr=bytes([255]) + p18[1:])
    # authentication
    good = seal(12, plain_of(IPV4))
    flip = lambda t, k: t[:k] + bytes([t[k] ^ 0x10]) + t[k + 1:]
    add("tag-bit", L.TK_AUTH, flip(good, len(good) - 1))
    add("ciphertext-bit", L.TK_AUTH, flip(good, 9))
    add("counter-byte", L.TK_AUTH, flip(good, 7))
    add("another-key", L.TK_AUTH, seal(12, plain_of(IPV4), key=OTHER_KEY))
    # the launch says no, whatever lies in the token buffer
    for st in (L.S_DECRYPT, L.S_LENGTH, L.S_NO_KEY, L.S_INTERNAL):
        add("status-%d-over-a-valid-plaintext" % st, L.TK_AUTH, good, forced=st)
    return out


KINDS = ("v4", "v6", "tag", "ciphertext", "counter", "address", "key", "short", "long", "varint2", "varint4",
         "record", "form", "tokenless", "grease")


def synthetic(n_acc: int):
    """n_acc candidates for the device form in a fixed mix of KINDS, one
    datagram of 1200 bytes each: (datagrams, walk records of packet 0,
    addresses as (host, port), kinds)."""
    datagrams, walks, addrs, kinds = [], [], [], []
    for a in range(n_acc):
        kind = KINDS[(a * 7 + a // len(KINDS)) % len(KINDS)]
        v6 = kind == "v6" or (kind not in ("v4",) and a % 3 == 0)
        addr = ("2001:db8::%x" % (a + 1), 1024 + a) if v6 else ("198.51.%d.%d" % (a >> 8 & 255, a & 255), 1024 + a)
        odcid, rscid = R.cid(a, 1 + a % 20), R.cid(a + 1, 8)
        dcid, scid = rscid, R.cid(a + 2, a % 21)
        token = token_for(1000 + a, addr, odcid, rscid)
        version, tform, size = (V2 if a % 2 else V1), 0, 1200 + a % 5
        if kind == "tag":
            token = token[:-1] + bytes([token[-1] ^ 0x01])
        elif kind == "ciphertext":
            token = token[:10] + bytes([token[10] ^ 0x80]) + token[11:]
        elif kind == "counter":
            token = token[:3] + bytes([token[3] ^ 0x01]) + token[4:]
        elif kind == "address":
            token = token_for(1000 + a, (addr[0], addr[1] + 1), odcid, rscid)
        elif kind == "key":
            token = token_for(1000 + a, addr, odcid, rscid, key=OTHER_KEY)
        elif kind == "short":
            token = token[:26]
        elif kind == "long":
            token = (token + bytes(129))[:129]
        elif kind == "varint2":
            tform = 1
        elif kind == "varint4":
            tform = 2
        elif kind == "form":
            token = seal(1000 + a, plain_of(addr, odcid, rscid)[:-1])
        elif kind == "tokenless":
            token = b""
        elif kind == "grease":
            version = R.GREASE
        data = initial(version, dcid, scid, token, tform, size)
        w = walk_of(data)
        if kind == "record":
            w = dict(w, scid_len=(w["scid_len"] + 1) % 21)
        datagrams.append(data), walks.append(w), addrs.append(addr), kinds.append(kind)
    return datagrams, walks, addrs, kinds
