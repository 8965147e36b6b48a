"""numpy views of the C ABI records in include/quic_pp.h."""

import numpy as np

AES_128_GCM, AES_256_GCM, CHACHA20_POLY1305 = 0, 1, 2

PACKET_MAX = 1500
TAG_LEN = 16
MAX_HDR = 1500
# QPP_ITEM_SPAN_MAX: (offset - lowest offset in the item) + extent of every
# packet of a 16-packet item, for input and output alike (quic_pp.h, Buffers)
ITEM_SPAN_MAX = 0xFFFFFF00

# the message of a packet the engine gave up on (S_INTERNAL: a kernel's
# bounded wait ran out; never expected)
INTERNAL_ERROR = "Internal error: the packet was not processed"

F_NO_HP = 1
F_RFC_PN = 2

S_OK, S_LENGTH, S_DECRYPT, S_KEY_PHASE, S_NO_KEY, S_INTERNAL = 0, 1, 2, 3, 4, 5

DESC = np.dtype(
    [
        ("in_off", "<u8"),
        ("out_off", "<u8"),
        ("len", "<u4"),
        ("hdr_len", "<u2"),
        ("flags", "<u2"),
        ("pn", "<u8"),
        ("slot", "<u4"),
        ("rsv", "<u4"),
    ]
)
RESULT = np.dtype([("pn", "<u8"), ("status", "<u2"), ("hdr_len", "<u2"), ("out_len", "<u4")])
KEY_MATERIAL = np.dtype(
    [
        ("slot", "<u4"),
        ("suite", "u1"),
        ("key_phase", "u1"),
        ("rsv", "u1", (2,)),
        ("iv", "u1", (12,)),
        ("key", "u1", (32,)),
        ("hp", "u1", (32,)),
    ]
)
SECRET = np.dtype(
    [
        ("slot", "<u4"),
        ("suite", "u1"),
        ("key_phase", "u1"),
        ("flags", "u1"),
        ("secret_len", "u1"),
        ("updates", "<u4"),
        ("rsv", "<u4"),
        ("secret", "u1", (64,)),
    ]
)
DERIVE_V2 = 1
# qpp_initial: one connection's Initial keys for KeyTable.derive_initial
INITIAL = np.dtype(
    [
        ("slot_client", "<u4"),
        ("slot_server", "<u4"),
        ("cid_len", "u1"),
        ("flags", "u1"),
        ("rsv", "u1", (2,)),
        ("cid", "u1", (20,)),
    ]
)
SLOT_NONE = 0xFFFFFFFF  # QPP_SLOT_NONE: derive this direction but do not install it
# qpp_next_phase: one context's current traffic secret and header-protection
# key for KeyTable.derive_next, and the slot (or SLOT_NONE) of its next phase
NEXT_PHASE = np.dtype(
    [
        ("slot", "<u4"),
        ("suite", "u1"),
        ("key_phase", "u1"),
        ("flags", "u1"),
        ("secret_len", "u1"),
        ("secret", "u1", (64,)),
        ("hp", "u1", (32,)),
    ]
)
assert NEXT_PHASE.itemsize == 104
CID_MAX = 20
# qpp_cid_entry: one connection ID of a CidMap and the caller's connection index
CID_ENTRY = np.dtype(
    [
        ("conn", "<u4"),
        ("cid_len", "u1"),
        ("rsv", "u1", (3,)),
        ("cid", "u1", (20,)),
        ("rsv2", "<u4"),
    ]
)
# qpp_route_rec: where a received datagram belongs (conn, or CONN_NONE) and its R_* class
ROUTE = np.dtype([("conn", "<u4"), ("cls", "u1"), ("rsv", "u1", (3,))])
CONN_NONE = 0xFFFFFFFF
R_SHORT, R_LONG, R_UNKNOWN_CID, R_MALFORMED, R_BAD_CONN = 0, 1, 2, 3, 4
# qpp_walk_rec: one packet of a long-header datagram as qpp_route_walk found it
WALK = np.dtype([("off", "<u4"), ("len", "<u4"), ("version", "<u4"), ("desc", "<u4"), ("pn_off", "<u2"),
                 ("token_len", "<u2"), ("type", "u1"), ("status", "u1"), ("dcid_len", "u1"), ("scid_len", "u1")])
WALK_MAX = 4   # QPP_WALK_MAX: packets walked per datagram
KEYSETS = 5    # QPP_KEYSETS: Initial v1, Initial v2, 0-RTT, Handshake, 1-RTT
SPACES = 3     # QPP_SPACES: Initial, Handshake, application
DESC_NONE = 0xFFFFFFFF
W_OK, W_PARSE, W_HOST = 0, 1, 2
# qpp_accept_rec: the device's verdict on one candidate of qpp_route_accept (an
# unrouted Initial a server may answer): its datagram (= packet 0's descriptor)
# or DESC_NONE, an ACC_* status, and 0 / 1 for QUIC version 1 / 2
ACCEPT = np.dtype([("desc", "<u4"), ("status", "u1"), ("version", "u1"), ("rsv", "u1", (2,))])
ACC_OK, ACC_ROUTED, ACC_NOT_INITIAL, ACC_VERSION, ACC_SMALL, ACC_CID, ACC_NO_TOKEN = 0, 1, 2, 3, 4, 5, 6
A_NEED_TOKEN = 1  # QPP_A_NEED_TOKEN: the server's Retry mode, an Initial must carry a token
# qpp_route_phase: one verdict byte per descriptor (PHASE_NEXT: the descriptor
# was pointed at its connection's next-phase slot), and the per-connection
# next-phase slots it consults (a slot, or SLOT_NONE)
PHASE = np.dtype("u1")
PHASE_CURRENT, PHASE_NEXT = 0, 1
NEXT_SLOT = np.dtype("<u4")
# qpp_reply_rec: what qpp_route_reply built for one candidate: where the packet
# to send lies in the reply buffer (REPLY_STRIDE bytes per candidate), its
# length, an RP_KIND_* and an RP_* status (or the S_* of a failed seal / tag)
REPLY = np.dtype([("off", "<u4"), ("len", "<u2"), ("kind", "u1"), ("status", "u1")])
REPLY_STRIDE = 256          # QPP_REPLY_STRIDE
RP_MAX_VERSIONS = 16        # QPP_RP_MAX_VERSIONS
RP_ADDR_STRIDE, RP_RAND_STRIDE = 20, 16
RP_VN, RP_RETRY = 1, 2      # reply_flags
RP_KIND_NONE, RP_KIND_VN, RP_KIND_RETRY = 0, 1, 2
RP_OK, RP_BOUNDS, RP_ADDR = 0, 0x40, 0x41
# the reply key table's slots: the Retry keys of versions 1 and 2, the server's token key
RP_SLOT_V1, RP_SLOT_V2, RP_SLOT_TOKEN = 0, 1, 2
# qpp_token_rec: the device's verdict on the Retry token of one candidate
# (qpp_route_token, qpp_route_accept_tokens): a TK_* status and, with TK_OK,
# the two CIDs the token was sealed around; a candidate a token fails is
# ACC_BAD_TOKEN.  TOKEN_STRIDE bytes of the token buffer per candidate
TOKEN_REC = np.dtype([("status", "u1"), ("odcid_len", "u1"), ("rscid_len", "u1"), ("rsv", "u1"),
                      ("odcid", "u1", (20,)), ("rscid", "u1", (20,)), ("rsv2", "u1", (4,))])
TOKEN_STRIDE, TOKEN_MIN, TOKEN_MAX = 128, 27, 128
ACC_BAD_TOKEN = 7
TK_OK, TK_NONE, TK_LENGTH, TK_BOUNDS, TK_AUTH, TK_FORM, TK_ADDR = 0, 1, 2, 3, 4, 5, 6
# routed send (qpp_send_fill): SEND_CONN is one connection's send state (its
# next packet number, 1-RTT send slot, the peer's CID and the spin bit),
# SEND_REC what the device built for one payload (an SN_* status, the first
# failing check).  A payload at `off` may have SEND_HEAD bytes written before
# it and SEND_TAIL behind it: the longest header; the largest padding + the tag
SEND_CONN = np.dtype([("next_pn", "<u8"), ("slot", "<u4"), ("cid_len", "u1"), ("spin", "u1"), ("cid", "u1", (20,)),
                      ("rsv", "u1", (6,))])
SEND_REC = np.dtype([("pn", "<u8"), ("hdr_len", "<u2"), ("status", "u1"), ("rsv", "u1", (5,))])
SEND_PN_LEN = 2                         # QPP_SEND_PN_LEN
SEND_HEAD = 1 + CID_MAX + SEND_PN_LEN   # QPP_SEND_HEAD
SEND_TAIL = 1 + TAG_LEN                 # QPP_SEND_TAIL
SN_OK, SN_CONN, SN_CID, SN_NO_KEY, SN_EMPTY, SN_PN, SN_ROOM = 0, 1, 2, 3, 4, 5, 6
assert SEND_CONN.itemsize == 40 and SEND_REC.itemsize == 16
assert REPLY.itemsize == 8 and TOKEN_REC.itemsize == 48
assert DESC.itemsize == 40 and RESULT.itemsize == 16 and KEY_MATERIAL.itemsize == 84
assert WALK.itemsize == 24 and ACCEPT.itemsize == 8
assert SECRET.itemsize == 80 and INITIAL.itemsize == 32
assert CID_ENTRY.itemsize == 32 and ROUTE.itemsize == 8


def key_material(slot: int, suite: int, key: bytes, iv: bytes, hp: bytes, key_phase: int = 0):
    rec = np.zeros(1, dtype=KEY_MATERIAL)
    rec["slot"] = slot
    rec["suite"] = suite
    rec["key_phase"] = key_phase
    rec["iv"][0, : len(iv)] = np.frombuffer(iv, dtype=np.uint8)
    rec["key"][0, : len(key)] = np.frombuffer(key, dtype=np.uint8)
    rec["hp"][0, : len(hp)] = np.frombuffer(hp, dtype=np.uint8)
    return rec


def next_phase_record(slot: int, suite: int, secret: bytes, hp: bytes, *, key_phase: int, v2: bool = False):
    """One qpp_next_phase: a context's current traffic secret and
    header-protection key; `key_phase` is the next phase's bit and `slot`
    where it is installed (SLOT_NONE: derived and returned only)."""
    if not 1 <= len(secret) <= 64:
        raise ValueError("secret must be 1..64 bytes")
    if len(hp) > 32:
        raise ValueError("header-protection key longer than 32 bytes")
    rec = np.zeros(1, dtype=NEXT_PHASE)
    rec["slot"] = slot
    rec["suite"] = suite
    rec["key_phase"] = key_phase
    rec["flags"] = DERIVE_V2 if v2 else 0
    rec["secret_len"] = len(secret)
    rec["secret"][0, : len(secret)] = np.frombuffer(secret, dtype=np.uint8)
    rec["hp"][0, : len(hp)] = np.frombuffer(hp, dtype=np.uint8)
    return rec


def secret_record(slot: int, suite: int, secret: bytes, *, key_phase: int = 0, v2: bool = False,
                  updates: int = 0):
    """One qpp_secret: a connection's traffic secret for KeyTable.derive."""
    if not 1 <= len(secret) <= 64:
        raise ValueError("secret must be 1..64 bytes")
    rec = np.zeros(1, dtype=SECRET)
    rec["slot"] = slot
    rec["suite"] = suite
    rec["key_phase"] = key_phase
    rec["flags"] = DERIVE_V2 if v2 else 0
    rec["secret_len"] = len(secret)
    rec["updates"] = updates
    rec["secret"][0, : len(secret)] = np.frombuffer(secret, dtype=np.uint8)
    return rec


def initial_record(slot_client: int, slot_server: int, cid: bytes, *, v2: bool = False):
    """One qpp_initial: the connection ID a connection's Initial keys come
    from, and the slots (or SLOT_NONE) of its "client in" / "server in" keys."""
    if len(cid) > CID_MAX:
        raise ValueError("connection ID longer than 20 bytes")
    rec = np.zeros(1, dtype=INITIAL)
    rec["slot_client"] = slot_client
    rec["slot_server"] = slot_server
    rec["cid_len"] = len(cid)
    rec["flags"] = DERIVE_V2 if v2 else 0
    rec["cid"][0, : len(cid)] = np.frombuffer(cid, dtype=np.uint8)
    return rec


def send_conn(next_pn: int, slot: int, cid: bytes, spin: bool = False):
    """One qpp_send_conn: a connection's next packet number, its 1-RTT send
    slot (or SLOT_NONE), the peer's connection ID (0..20 bytes) and spin bit."""
    if len(cid) > CID_MAX:
        raise ValueError("connection ID longer than 20 bytes")
    rec = np.zeros(1, dtype=SEND_CONN)
    rec["next_pn"] = next_pn
    rec["slot"] = slot
    rec["cid_len"] = len(cid)
    rec["spin"] = 1 if spin else 0
    rec["cid"][0, : len(cid)] = np.frombuffer(cid, dtype=np.uint8)
    return rec


def cid_entry(cid: bytes, conn: int = 0):
    """One qpp_cid_entry: a connection ID (1..20 bytes) and the connection
    index it routes to (ignored by CidMap.remove)."""
    if not 1 <= len(cid) <= CID_MAX:
        raise ValueError("connection ID must be 1..20 bytes")
    rec = np.zeros(1, dtype=CID_ENTRY)
    rec["conn"] = conn
    rec["cid_len"] = len(cid)
    rec["cid"][0, : len(cid)] = np.frombuffer(cid, dtype=np.uint8)
    return rec
