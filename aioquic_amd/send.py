"""Routed send: a batch of payloads to protected 1-RTT datagrams without a
host header pass, the mirror of receive.receive_routed.

The batched sender so far is QuicPacketBuilder with flush_builders: per packet
the host runs start_packet, _write_header, _padding_for and _Pending.add, and
resolves the key, the peer CID, the key-phase bit and the packet number.
send_routed() hands the device the payloads and a connection index each; the
connections' send state goes up as one array (layout.SEND_CONN) and a kernel
in front of the protect launch writes each packet's short header, its packet
number and the sample padding (qpp_send_fill; what the reference's
QuicPacketBuilder._end_packet writes for a 1-RTT packet,
quic/packet_builder.py:264-296,330-339).  One upload, two launches, one
download.

Only 1-RTT packets, one per datagram (a short header ends its datagram).
Initial and Handshake packets, datagram padding, frames, congestion
accounting and QuicSentPacket stay with the builder.
"""

from __future__ import annotations

import struct
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _crypto
from . import layout as L
from .batch_io import KeySlots, _raise_status, default_slots
from ._crypto import CryptoError
from .crypto import CryptoPair, KeyUnavailableError

__all__ = ["SendConnection", "send_routed"]

# one qpp_send_conn (layout.SEND_CONN) by struct: one record per connection and
# call, where numpy's structured scalars cost microseconds each
_CONN = struct.Struct("<QIBB20s6x")
assert _CONN.size == L.SEND_CONN.itemsize
_CONN_UNUSED = _CONN.pack(0, L.SLOT_NONE, 0, 0, b"")


class SendConnection:
    """What send_routed needs of a connection: its 1-RTT CryptoPair, the
    peer's connection ID, the next packet number and the spin bit."""

    __slots__ = ("crypto", "peer_cid", "packet_number", "spin_bit")

    def __init__(self, crypto: CryptoPair, peer_cid: bytes, packet_number: int = 0, spin_bit: bool = False) -> None:
        if len(peer_cid) > L.CID_MAX:
            raise ValueError("connection ID longer than 20 bytes")
        self.crypto, self.peer_cid = crypto, bytes(peer_cid)
        self.packet_number, self.spin_bit = int(packet_number), bool(spin_bit)


def _padding(size: int) -> int:
    # enough bytes after the packet number for a 16-byte HP sample
    return max(0, 4 - L.SEND_PN_LEN - size)


def _send_error(status: int) -> Exception:
    if status == L.SN_NO_KEY:
        return KeyUnavailableError("Encryption key is not available")
    if status == L.SN_PN:
        return CryptoError("Packet number space exhausted")
    return CryptoError(f"Packet not built (status {status})")


def send_routed(conns: Sequence[SendConnection], items: Sequence[Tuple[int, bytes]], *,
                slots: Optional[KeySlots] = None) -> Tuple[list, list]:
    """(datagrams, packet numbers) of `items` = [(connection index, payload
    bytes)], in order: each payload as one protected 1-RTT packet of its
    connection, numbered from the connection's packet_number on.  The bytes
    are those per-connection QuicPacketBuilders and flush_builders give for
    the same payloads written as one packet each.

    Raised before anything moves: ValueError for an empty payload, an index
    out of range or a payload that cannot fit 1500 bytes; KeyUnavailableError
    for a connection without send keys.  A pending local key update
    (CryptoPair.update_key) of a connection that sends is applied first, once.
    A packet the device refuses is raised as the batched callers raise it.
    Each connection's packet_number advances by its packets only when the
    whole call succeeded."""
    n_conn = len(conns)
    counts = [0] * n_conn
    conn_ix, payloads = [], []
    for ci, payload in items:
        if not 0 <= ci < n_conn:
            raise ValueError("connection index out of range")
        size = len(payload)
        if size == 0:
            raise ValueError("empty payload")
        c = conns[ci]
        if 1 + len(c.peer_cid) + L.SEND_PN_LEN + size + _padding(size) + L.TAG_LEN > L.PACKET_MAX:
            raise ValueError("payload does not fit a 1500-byte packet")
        counts[ci] += 1
        conn_ix.append(ci)
        payloads.append(payload if type(payload) is bytes else bytes(payload))
    used = [ci for ci in range(n_conn) if counts[ci]]
    for ci in used:
        if not conns[ci].crypto.send.is_valid():
            raise KeyUnavailableError("Encryption key is not available")
        if conns[ci].packet_number + counts[ci] > 1 << 62:
            raise ValueError("packet number space exhausted")
    if not payloads:
        return [], []
    # a pending local key update first (crypto.py:194-199), once per pair
    for ci in used:
        pair = conns[ci].crypto
        if pair._update_key_requested:
            pair._update_key("local_update")
    slots = slots or default_slots()
    ctxs = [conns[ci].crypto.send for ci in used]
    per_used = slots.assign([(x.aead, x.hp, x.key_phase) for x in ctxs])
    state = [_CONN_UNUSED] * n_conn
    for ci, slot in zip(used, per_used):
        c = conns[ci]
        state[ci] = _CONN.pack(c.packet_number, slot, len(c.peer_cid), c.spin_bit, c.peer_cid)
    wires, rec, res = _crypto.send_routed(slots.table, b"".join(state), np.asarray(conn_ix, np.uint32).tobytes(),
                                          payloads)
    rec = np.frombuffer(rec, dtype=L.SEND_REC)
    bad = np.flatnonzero(rec["status"] != L.SN_OK)
    if len(bad):
        raise _send_error(int(rec["status"][bad[0]]))
    status = np.frombuffer(res, dtype=L.RESULT)["status"]
    bad = np.flatnonzero(status != L.S_OK)
    if len(bad):
        raise _raise_status(int(status[bad[0]]))
    for ci in used:
        conns[ci].packet_number += counts[ci]
    return wires, rec["pn"].tolist()
