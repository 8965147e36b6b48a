"""Batched receive of many datagrams.

QuicConnection.receive_datagram (quic/connection.py:793-947) walks the
coalesced packets of ONE datagram: pull_quic_header (packet.py:181-267)
gives each packet's header and the offset of its packet number (the
"encrypted offset"), the packet's epoch picks the crypto pair and packet
number space (:889-899), and CryptoPair.decrypt_packet runs per packet
(:905-947).  receive_datagrams does the same walk for a whole batch of
datagrams, possibly of many connections, then decrypts every packet in one
ReceiveBatch (one device launch, a second only for key-phase flips), with
the sequential semantics of the per-packet loop: a packet's expected packet
number reflects the packets before it, and a peer key update rolls the
pair's keys before later packets (batch_io.ReceiveBatch).

Datagrams whose first byte is a short header (the 1-RTT bulk) take a
vectorised path: encrypted offset = 1 + host CID length, one packet per
datagram (a short-header packet always runs to the end of its datagram,
RFC 9000 sec. 12.2), no per-packet header parse.

receive_routed takes raw datagrams nobody has demultiplexed: the device
routes each to its connection by connection ID (route.CidRouter, qpp_route)
in the same call that unprotects it, in place of the server's per-datagram
routing (asyncio/server.py:60-152).

The connection-level checks around the decrypt follow the reference too:
a connection that lists its host CIDs drops packets for other CIDs (clients:
every packet, servers: Handshake packets, "unknown_connection_id",
connection.py:830-848); a packet that authenticates with a reserved header bit
set closes its connection ("reserved_bits", :949-960: the rest of the datagram
is not read and the expected packet number is not raised), and a closed
connection's datagrams are ignored ("connection_closed", :756-757; one record
per datagram, where the reference logs nothing).
"""

from __future__ import annotations

import os
from dataclasses import dataclass, field
from typing import Any, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _crypto
from . import layout as L
from ._crypto import CryptoError
from .batch_io import (ConnectionClosedError, ReceiveBatch, ReservedBitsError, _initial_directions, _install_initial,
                       default_slots, setup_initial_batch, setup_next_phase_batch, update_keys_batch)
from .buffer import Buffer
from .crypto import KeyUnavailableError, cached_next_phase
from .packet import (
    PACKET_FIXED_BIT,
    PACKET_LONG_HEADER,
    QuicHeader,
    QuicPacketType,
    QuicProtocolVersion,
    pull_quic_header,
)
from .tls import Epoch

SMALLEST_MAX_DATAGRAM_SIZE = 1200  # quic/configuration.py; RFC 9000 sec. 14.1

_EPOCH_OF_TYPE = {
    QuicPacketType.INITIAL: Epoch.INITIAL,
    QuicPacketType.ZERO_RTT: Epoch.ZERO_RTT,
    QuicPacketType.HANDSHAKE: Epoch.HANDSHAKE,
    QuicPacketType.ONE_RTT: Epoch.ONE_RTT,
}


@dataclass
class ConnectionKeys:
    """What receive_datagram consults per packet: the crypto pairs per epoch
    (Initial ones per version), the packet number spaces, the CID length,
    the role and the versions the configuration accepts
    (QuicConfiguration.supported_versions, configuration.py:115-120); the
    host CIDs a packet's destination CID must match (connection.py:830-848;
    None: not checked, the batch is already demultiplexed per connection) and
    whether the connection is closing (set by a reserved-bit violation)."""

    cryptos: Dict[Epoch, Any]
    spaces: Dict[Epoch, Any]
    cryptos_initial: Optional[Dict[int, Any]] = None
    host_cid_length: int = 8
    is_client: bool = False
    supported_versions: List[int] = field(
        default_factory=lambda: [QuicProtocolVersion.VERSION_1, QuicProtocolVersion.VERSION_2])
    host_cids: Optional[Sequence[bytes]] = None
    closed: bool = False

    def cid_unknown(self, packet_type: QuicPacketType, dcid: bytes) -> bool:
        """connection.py:830-848: clients check every packet, servers their
        Handshake packets."""
        return (self.host_cids is not None and (self.is_client or packet_type == QuicPacketType.HANDSHAKE)
                and dcid not in self.host_cids)

    def pair_and_space(self, epoch: Epoch, version: Optional[int]):
        if epoch == Epoch.INITIAL:
            pair = (self.cryptos_initial or {}).get(version, self.cryptos.get(Epoch.INITIAL))
        else:
            pair = self.cryptos[epoch]
        space = self.spaces[Epoch.ONE_RTT if epoch == Epoch.ZERO_RTT else epoch]
        return pair, space


class ReceivedPacket(NamedTuple):
    """One packet's outcome, in datagram order (an immutable record; tuple
    construction keeps the batched walk cheap per packet)."""

    datagram: int                 # index of the datagram in the batch
    offset: int                   # packet start within the datagram
    header: Optional[QuicHeader]  # None on the short-header fast path
    packet_type: QuicPacketType
    epoch: Optional[Epoch]
    plain_header: bytes = b""
    plain_payload: bytes = b""
    packet_number: int = -1
    dropped: Optional[str] = None  # the reference's packet_dropped trigger, if any

    @property
    def ok(self) -> bool:
        return self.dropped is None


_new = tuple.__new__
# reserved header bits (connection.py:949-953)
_RSV_SHORT, _RSV_LONG = 0x18, 0x0C
_DROP_OF = {ReservedBitsError: "reserved_bits", ConnectionClosedError: "connection_closed",
            KeyUnavailableError: "key_unavailable"}


def _record(f: tuple, res) -> ReceivedPacket:
    """The record of a queued packet from its ReceiveBatch outcome."""
    if isinstance(res, tuple):
        return _new(ReceivedPacket, f + res + (None,))
    drop = _DROP_OF.get(type(res), "payload_decrypt_error")
    if drop == "connection_closed":
        f = (f[0], 0, None, QuicPacketType.ONE_RTT, None)
    return _new(ReceivedPacket, f + (b"", b"", -1, drop))


def _closed_record(d: int) -> ReceivedPacket:
    return ReceivedPacket(d, 0, None, QuicPacketType.ONE_RTT, None, dropped="connection_closed")


def _walk_long(conn: ConnectionKeys, d: int, data: bytes, out: list, queued: list, add) -> None:
    """One datagram through the header parser, packet by packet.  Packets to
    decrypt go to `add(pair, packet, encrypted_offset, space)` and their
    record fields (datagram, offset, header, type, epoch) to `queued` with a
    placeholder in `out`."""
    buf = Buffer(data=data)
    while not buf.eof():
        start = buf.tell()
        try:
            header = pull_quic_header(buf, host_cid_length=conn.host_cid_length)
        except ValueError:
            out.append(ReceivedPacket(d, start, None, QuicPacketType.ONE_RTT, None, dropped="header_parse_error"))
            return
        ptype = header.packet_type
        if not conn.is_client and ptype == QuicPacketType.INITIAL and len(data) < SMALLEST_MAX_DATAGRAM_SIZE:
            out.append(ReceivedPacket(d, start, header, ptype, Epoch.INITIAL,
                                      dropped="initial_packet_datagram_too_small"))
            return
        if conn.cid_unknown(ptype, header.destination_cid):
            out.append(ReceivedPacket(d, start, header, ptype, None, dropped="unknown_connection_id"))
            return
        if ptype == QuicPacketType.VERSION_NEGOTIATION:
            # not packet-protected: handed back for the connection's own handler
            out.append(ReceivedPacket(d, start, header, ptype, None))
            return
        # a long header of a version the configuration does not accept ends
        # the datagram (connection.py:855-869)
        if header.version is not None and header.version not in conn.supported_versions:
            out.append(ReceivedPacket(d, start, header, ptype, None, dropped="unsupported_version"))
            return
        if ptype == QuicPacketType.RETRY:
            out.append(ReceivedPacket(d, start, header, ptype, None))
            return
        epoch = _EPOCH_OF_TYPE[ptype]
        pair, space = conn.pair_and_space(epoch, header.version)
        enc_off = buf.tell() - start
        end = start + header.packet_length
        buf.seek(end)
        queued.append((len(out), (d, start, header, ptype, epoch)))
        out.append(None)
        add(pair, data[start:end], enc_off, space, conn, _RSV_SHORT if ptype == QuicPacketType.ONE_RTT else _RSV_LONG)


def _receive_short(items: list) -> Optional[List[ReceivedPacket]]:
    """The steady state in C (_crypto.receive_short): every datagram one
    short-header packet.  None (nothing launched) when any is not; the
    caller then walks the batch in Python."""
    conns = _crypto.first_of_each(items)
    if any(c.is_client and c.host_cids is not None for c in conns):
        return None  # DCID checks: the general walk
    pix: dict = {}
    six: dict = {}
    upairs, uspaces, c_pair, c_space, c_cid = [], [], [], [], []
    for conn in conns:
        pair, space = conn.pair_and_space(Epoch.ONE_RTT, None)
        if id(pair) not in pix:
            pix[id(pair)] = len(upairs)
            upairs.append(pair)
        if id(space) not in six:
            six[id(space)] = len(uspaces)
            uspaces.append(space)
        c_pair.append(pix[id(pair)])
        c_space.append(six[id(space)])
        c_cid.append(conn.host_cid_length)
    slots = default_slots()
    keyed = [k for k, p in enumerate(upairs) if p.recv.aead is not None]
    pslot = np.full(len(upairs), 0xFFFFFFFF, np.uint32)
    if keyed:
        rc = [upairs[k].recv for k in keyed]
        pslot[keyed] = slots.assign([(c.aead, c.hp, c.key_phase) for c in rc])
    sexp = np.asarray([sp.expected_packet_number & 0xFFFFFFFFFFFFFFFF for sp in uspaces], np.uint64)
    got = _crypto.receive_short(slots.table, items, conns, np.asarray(c_cid, np.uint32).tobytes(),
                                np.asarray(c_pair, np.uint32).tobytes(), np.asarray(c_space, np.uint32).tobytes(),
                                pslot.tobytes(), sexp.tobytes(), ReceivedPacket, QuicPacketType.ONE_RTT,
                                Epoch.ONE_RTT, bytes(bool(c.closed) for c in conns))
    if got is None:
        return None
    recs, deferred, sexp2, closed = got
    new = np.frombuffer(sexp2, dtype=np.uint64)
    for k in np.flatnonzero(new != sexp).tolist():
        uspaces[k].expected_packet_number = int(new[k])
    for k, f in enumerate(closed):
        if f:
            conns[k].closed = True
    if deferred:
        # key-phase flips and numbers decoded under a stale expected number:
        # the general walk takes them in order from the state left above
        rb = ReceiveBatch(slots=slots)
        for d in deferred:
            conn, data = items[d]
            pair, space = conn.pair_and_space(Epoch.ONE_RTT, None)
            rb.add(pair, data, 1 + conn.host_cid_length, space=space, conn=conn, reserved_mask=_RSV_SHORT)
        for d, res in zip(deferred, rb.run()):
            recs[d] = _record((d, 0, None, QuicPacketType.ONE_RTT, Epoch.ONE_RTT), res)
            if isinstance(res, ReservedBitsError):
                items[d][0].closed = True
    return recs


def receive_datagrams(items: Sequence[Tuple[ConnectionKeys, bytes]],
                      batch: Optional[ReceiveBatch] = None) -> List[ReceivedPacket]:
    """Parse and unprotect every packet of every (connection, datagram) in
    order; returns one ReceivedPacket per packet (or per dropped remainder of
    a datagram, like the reference's early returns).

    Short-header datagrams (the 1-RTT bulk) skip the header parser: their
    encrypted offset is 1 + the host CID length and the packet runs to the
    end of the datagram.  Every packet goes into one ReceiveBatch, whose first
    round (one launch and the in-order walk) runs in C."""
    own = batch is None
    if not items:
        return []
    if own:
        fast = _receive_short(items if isinstance(items, list) else list(items))
        if fast is not None:
            return fast
    batch = batch or ReceiveBatch(slots=default_slots())
    first = np.fromiter((dg[0] if dg else 0 for _, dg in items), np.uint8, len(items))
    short = ((first & (PACKET_LONG_HEADER | PACKET_FIXED_BIT)) == PACKET_FIXED_BIT).tolist()
    out: list = []
    queued: list = []  # (position in out, record fields) of every packet to decrypt
    # runs of short-header datagrams go to the batch in bulk
    r_pairs: list = []
    r_packets: list = []
    r_offs: list = []
    r_spaces: list = []
    r_conns: list = []
    by_conn: dict = {}
    bulk = own or hasattr(batch, "_extend")

    def flush_run():
        if r_pairs:
            if bulk:
                batch._extend(r_pairs, r_packets, r_offs, r_spaces, r_conns, _RSV_SHORT)
            else:
                for a, b, c, e, g in zip(r_pairs, r_packets, r_offs, r_spaces, r_conns):
                    batch.add(a, b, c, space=e, conn=g, reserved_mask=_RSV_SHORT)
            r_pairs.clear(), r_packets.clear(), r_offs.clear(), r_spaces.clear(), r_conns.clear()

    def add(pair, packet, enc_off, space, conn, rsv):
        flush_run()
        batch.add(pair, packet, enc_off, space=space, conn=conn, reserved_mask=rsv)

    one_rtt, ep1 = QuicPacketType.ONE_RTT, Epoch.ONE_RTT
    for d, ((conn, data), is_short) in enumerate(zip(items, short)):
        if conn.closed:
            out.append(_closed_record(d))  # connection.py:756-757
            continue
        if is_short:
            c = by_conn.get(id(conn))
            if c is None:
                pair, space = conn.pair_and_space(ep1, None)
                c = by_conn[id(conn)] = (pair, space, 1 + conn.host_cid_length, conn,
                                         conn.is_client and conn.host_cids is not None)
            if len(data) >= c[2]:
                if c[4] and data[1:c[2]] not in conn.host_cids:
                    out.append(ReceivedPacket(d, 0, None, one_rtt, None, dropped="unknown_connection_id"))
                    continue
                queued.append((len(out), (d, 0, None, one_rtt, ep1)))
                out.append(None)
                r_pairs.append(c[0])
                r_packets.append(data)
                r_offs.append(c[2])
                r_spaces.append(c[1])
                r_conns.append(conn)
                continue
        _walk_long(conn, d, data, out, queued, add)
    flush_run()
    return _finish(items, out, queued, batch.run())


def _finish(items, out: list, queued: list, results: list) -> list:
    """The queued packets' records from their ReceiveBatch outcomes, then the
    closes; `items[d][0]` is datagram d's connection."""
    cut = False
    for (pos, f), res in zip(queued, results):
        out[pos] = _record(f, res)
        cut = cut or not isinstance(res, tuple) and isinstance(res, (ReservedBitsError, ConnectionClosedError))
    return _apply_closes(items, out) if cut else out


def _apply_closes(items, out: list) -> list:
    """A reserved-bit violation closes its connection (connection.py:949-960):
    the rest of its datagram is not read, and every later datagram of the
    connection is ignored (:756-757), one "connection_closed" record each."""
    new: list = []
    closed: set = set()
    k = 0
    while k < len(out):
        d = out[k].datagram
        conn = items[d][0]
        e = k
        while e < len(out) and out[e].datagram == d:
            e += 1
        if id(conn) in closed:
            new.append(_closed_record(d))
        else:
            for r in out[k:e]:
                new.append(r)
                if r.dropped == "reserved_bits":
                    closed.add(id(conn))
                    conn.closed = True
                    break
        k = e
    return new


_V1, _V2 = QuicProtocolVersion.VERSION_1, QuicProtocolVersion.VERSION_2
_TYPE_OF = [QuicPacketType(k) for k in range(6)]  # by qpp_walk_rec.type


def _keysets(conn: ConnectionKeys) -> tuple:
    """The pairs of layout.KEYSETS 0..3 (Initial v1, Initial v2, 0-RTT,
    Handshake) as pair_and_space picks them; None where there is none."""
    ci = conn.cryptos_initial or {}
    dflt = conn.cryptos.get(Epoch.INITIAL)
    return (ci.get(_V1, dflt), ci.get(_V2, dflt), conn.cryptos.get(Epoch.ZERO_RTT),
            conn.cryptos.get(Epoch.HANDSHAKE))


def _long_header(data: bytes, start: int, ptype, version: int, length: int, dl: int, sl: int, tok: int) -> QuicHeader:
    """The QuicHeader of a packet-protected long-header packet from its walk
    record's fields (qpp_walk_rec): the CIDs and the token are cut out of the
    datagram, nothing is parsed again."""
    at = start + 6 + dl
    dcid, scid = data[start + 6:at], data[at + 1:at + 1 + sl]
    token = b""
    if ptype == QuicPacketType.INITIAL:
        at += 1 + sl
        at += 1 << (data[at] >> 6)  # the token length's own bytes
        token = data[at:at + tok]
    return QuicHeader(version, ptype, length, dcid, scid, token=token)


def _routed_long(conns, datagrams, cid_len: int, idx: list, cls, rconn, longs, slots,
                 accepted: Optional[dict] = None) -> Optional[list]:
    """receive_routed for a batch with long headers to known connections,
    from what the fused call returned (_crypto.receive_routed): the device
    has parsed every listed datagram (qpp_walk_rec) and unprotected every
    packet; policy is decided here per packet in the reference's order
    (_walk_long), and the remaining packets go through ReceiveBatch's
    in-order walk over the results already there (ReceiveBatch.preset), in
    datagram order with coalesced packets in order.  Only what that walk
    defers (key-phase flips, stale expected numbers) is launched again.
    None, with no state touched: a datagram the device left to the host walk,
    or an Initial the device had no key-set for; the caller's general path
    takes the batch.
    `accepted` (accept_routed): {datagram: its new connection} for the
    datagrams the device accepted in the same call; `idx` lists them among the
    routed ones.  Packet 0 of such a datagram was unprotected by the fused
    launch with the connection's fresh Initial keys (its descriptor is the
    datagram's); its later packets had no descriptor, so they run in a second
    ReceiveBatch after the first, in order, with whatever keys the connection
    has by then."""
    accepted = accepted or {}
    lidx_b, walk_b, wn_b, desc_b, res_b, out_b = longs
    row_of = {i: r for r, i in enumerate(np.frombuffer(lidx_b, np.uint32).tolist())}
    walk = np.frombuffer(walk_b, dtype=L.WALK).reshape(-1, L.WALK_MAX)
    wn = np.frombuffer(wn_b, np.uint32).tolist()
    live = np.arange(L.WALK_MAX)[None, :] < np.asarray(wn, np.int64)[:, None]
    if ((walk["status"] == L.W_HOST) & live).any():
        return None
    w_off, w_len, w_ver, w_desc = (walk[f].tolist() for f in ("off", "len", "version", "desc"))
    w_pn, w_tok, w_type, w_st = (walk[f].tolist() for f in ("pn_off", "token_len", "type", "status"))
    w_dl, w_sl = walk["dcid_len"].tolist(), walk["scid_len"].tolist()
    one_rtt, ep1, initial = QuicPacketType.ONE_RTT, Epoch.ONE_RTT, QuicPacketType.INITIAL
    out: list = []
    queued: list = []
    pairs, packets, offs, spaces, pconns, rsvs, dix = [], [], [], [], [], [], []
    late: list = []  # packets after packet 0 of accepted datagrams: (queue entry, add() arguments)
    items = {}
    by_conn: dict = {}
    r_short = L.R_SHORT
    for i in idx:
        fresh = i in accepted
        conn = accepted[i] if fresh else conns[rconn[i]]
        data = datagrams[i]
        items[i] = (conn, data)
        if conn.closed:
            out.append(_closed_record(i))  # connection.py:756-757
            continue
        if cls[i] == r_short:
            c = by_conn.get(id(conn))
            if c is None:
                c = by_conn[id(conn)] = conn.pair_and_space(ep1, None)
            queued.append((len(out), (i, 0, None, one_rtt, ep1)))
            out.append(None)
            pairs.append(c[0]), packets.append(data), offs.append(1 + cid_len), spaces.append(c[1])
            pconns.append(conn), rsvs.append(_RSV_SHORT), dix.append(i)
            continue
        r = row_of[i]
        for k in range(wn[r]):
            start = w_off[r][k]
            if w_st[r][k] == L.W_PARSE:
                out.append(ReceivedPacket(i, start, None, one_rtt, None, dropped="header_parse_error"))
                break
            ptype = _TYPE_OF[w_type[r][k]]
            if ptype in (QuicPacketType.VERSION_NEGOTIATION, QuicPacketType.RETRY):
                # the device left the version list and the Retry token unread: the host parser's
                buf = Buffer(data=data)
                buf.seek(start)
                try:
                    header = pull_quic_header(buf, host_cid_length=cid_len)
                except ValueError:
                    out.append(ReceivedPacket(i, start, None, one_rtt, None, dropped="header_parse_error"))
                    break
            elif ptype == one_rtt:
                header = QuicHeader(None, one_rtt, w_len[r][k], data[start + 1:start + 1 + cid_len], b"")
            else:
                header = _long_header(data, start, ptype, w_ver[r][k], w_len[r][k], w_dl[r][k], w_sl[r][k],
                                      w_tok[r][k])
            if not conn.is_client and ptype == initial and len(data) < SMALLEST_MAX_DATAGRAM_SIZE:
                out.append(ReceivedPacket(i, start, header, ptype, Epoch.INITIAL,
                                          dropped="initial_packet_datagram_too_small"))
                break
            if conn.cid_unknown(ptype, header.destination_cid):
                out.append(ReceivedPacket(i, start, header, ptype, None, dropped="unknown_connection_id"))
                break
            if ptype == QuicPacketType.VERSION_NEGOTIATION:
                out.append(ReceivedPacket(i, start, header, ptype, None))
                break
            if header.version is not None and header.version not in conn.supported_versions:
                out.append(ReceivedPacket(i, start, header, ptype, None, dropped="unsupported_version"))
                break
            if ptype == QuicPacketType.RETRY:
                out.append(ReceivedPacket(i, start, header, ptype, None))
                break
            epoch = _EPOCH_OF_TYPE[ptype]
            pair, space = conn.pair_and_space(epoch, header.version)
            if ptype == initial and header.version not in (_V1, _V2) and pair is not None \
                    and pair.recv.aead is not None:
                return None  # keys the device had no key-set for
            rsv = _RSV_SHORT if ptype == one_rtt else _RSV_LONG
            if fresh and k:
                late.append(((len(out), (i, start, header, ptype, epoch)),
                             (pair, data[start:start + w_len[r][k]], w_pn[r][k], space, conn, rsv)))
                out.append(None)
                continue
            queued.append((len(out), (i, start, header, ptype, epoch)))
            out.append(None)
            pairs.append(pair), packets.append(data[start:start + w_len[r][k]]), offs.append(w_pn[r][k])
            spaces.append(space), pconns.append(conn)
            rsvs.append(rsv), dix.append(i if fresh else w_desc[r][k])
    rb = ReceiveBatch(slots=slots)
    rb._extend(pairs, packets, offs, spaces, pconns, rsvs)
    rb.preset(desc_b, res_b, dix, out_b)
    results = rb.run()
    if late:
        # a connection the first walk closed ignores what follows (connection.py:756-757)
        shut = {id(c) for c, res in zip(pconns, results) if isinstance(res, ReservedBitsError)}
        rb = ReceiveBatch(slots=slots)
        todo = [(q, a) for q, a in late if id(a[4]) not in shut and a[0] is not None]
        for _, (pair, packet, off, space, conn, rsv) in todo:
            rb.add(pair, packet, off, space=space, conn=conn, reserved_mask=rsv)
        got = dict(zip((q[0] for q, _ in todo), rb.run()))
        for q, a in late:
            queued.append(q)
            results.append(got.get(q[0], KeyUnavailableError("Decryption key is not available") if a[0] is None
                                   else ConnectionClosedError("Connection is closed")))
    return _finish(items, out, queued, results)


def receive_routed(router, datagrams: Sequence[bytes], *,
                   next_phase: bool = False) -> Tuple[List[ReceivedPacket], List[Tuple[int, int]]]:
    """receive_routed_keys(router, datagrams, next_phase=next_phase), which
    documents it: the entry point as it was before the key schedule of a
    peer's key update had a device form (its parameter list is pinned)."""
    return receive_routed_keys(router, datagrams, next_phase=next_phase)


def receive_routed_keys(router, datagrams: Sequence[bytes], *, next_phase: bool = False,
                        device_keys: bool = False) -> Tuple[List[ReceivedPacket], List[Tuple[int, int]]]:
    """receive_datagrams for raw datagrams nobody has demultiplexed: the
    device routes each to its connection by connection ID (route.CidRouter,
    qpp_route), instead of the reference's per-datagram pull_quic_header and
    dict lookup (asyncio/server.py:60-152).

    Returns (records, unrouted).  `records` are the ReceivedPackets of the
    routed datagrams in order -- what receive_datagrams returns for
    [(router.conns[c], datagram), ...] over them, with the same sequential
    semantics -- and .datagram indexes the caller's list.  `unrouted` is
    [(index, layout.R_* class)] of everything with no connection: an unknown
    CID, a long header with an unknown DCID, a malformed datagram -- the
    caller's new-connection, stateless-reset and drop business (:86-152).

    The batch is staged once and one call routes and unprotects it
    (_crypto.receive_routed).  Long headers to known connections (Handshake
    traffic to a host CID, coalesced Initial + Handshake + 1-RTT datagrams,
    0-RTT) are walked on the device in that same call (qpp_route_walk): the
    walk records give every coalesced packet's offsets and type, policy
    (too-small Initial datagrams, unknown Handshake DCIDs, Version Negotiation
    and Retry, unsupported versions) is decided here in the reference's order,
    and the in-order walk runs over the results of the one launch
    (_routed_long).  Key slots beyond the 1-RTT ones are assigned only to the
    connections that the batch's long headers can reach (by their DCIDs).
    The general path sends the routed datagrams through receive_datagrams
    instead, their bytes then uploaded twice, once to route and once to
    unprotect; it is taken for a client that checks its host CIDs, a datagram
    the device leaves to the host walk (more than layout.WALK_MAX packets, a
    header past layout.MAX_HDR), a keyed Initial of a supported version that
    is neither 1 nor 2, and a key table too small for the reached
    connections' key-sets beside the 1-RTT ones.

    A peer's key update (a short header whose key-phase bit flipped,
    crypto.py:91-96) is deferred to ReceiveBatch by default: the packet and
    every later one of its connection in the batch are uploaded and launched
    again.  With `next_phase`, every keyed 1-RTT receive context also gets a
    slot for its next key phase (crypto.cached_next_phase: the next AEAD key
    under the current header-protection key, which a key update keeps), in the
    same assign() as the batch's other keys, and a kernel ahead of the
    unprotect points each flipped packet's descriptor at it (qpp_route_phase),
    so the one launch decrypts both phases.  The in-order walk then rolls a
    pair at its first next-phase packet that authenticates, as
    CryptoPair.decrypt_packet does (crypto.py:184-192); the rolled pairs adopt
    their cached contexts before anything deferred runs (an old-phase packet
    after the update still is: the reference tries it on the phase after next
    and fails).  A batch on the general path, one whose long headers reach
    known connections (_routed_long), and a key table too small for the next
    slots beside the batch's other keys run without next slots, as by default.

    `device_keys` (looked at only with `next_phase`) takes the key schedule of
    those updates off the host: the next phases that are not cached yet are
    derived and installed by one device call for the whole batch
    (batch_io.setup_next_phase_batch, after the batch's current keys are
    assigned and only if the table has room for them; else the batch runs
    without next slots), the rolled pairs are committed by one more
    (batch_io.update_keys_batch), and what is deferred runs on the same two
    calls.  No per-connection HKDF and no per-object key table is made; the
    records, the contexts' state and the callbacks are those of `next_phase`
    alone."""
    datagrams = datagrams if isinstance(datagrams, list) else list(datagrams)
    if not datagrams:
        return [], []
    conns = router.conns
    general = any(c is not None and c.is_client and c.host_cids is not None for c in conns)
    device_keys = bool(device_keys and next_phase)
    slots, uspaces, sexp, arrays, _, nxt = _routed_arrays_next(router, datagrams, general, next_phase, device_keys)
    closed = bytes(bool(c is not None and c.closed) for c in conns)
    if nxt is None:
        route_b, walked, longs = _crypto.receive_routed(
            slots.table, router.map, router.host_cid_length, datagrams, *arrays, ReceivedPacket,
            QuicPacketType.ONE_RTT, Epoch.ONE_RTT, closed, 0 if general else 1)
        return _routed_finish(router, datagrams, slots, uspaces, sexp, route_b, walked, longs,
                              device_keys=device_keys)
    upairs, pnext = nxt
    route_b, walked, longs = _crypto.receive_routed_phase(
        slots.table, router.map, router.host_cid_length, datagrams, *arrays, ReceivedPacket,
        QuicPacketType.ONE_RTT, Epoch.ONE_RTT, closed, 1, pnext.tobytes())
    if walked is None:
        # a long header reached a connection after all (the host asked the router's own dict, so
        # this is not expected): no state has moved, and the batch runs again without next slots
        return receive_routed(router, datagrams)
    rolled = walked[4]
    return _routed_finish(router, datagrams, slots, uspaces, sexp, route_b, walked[:4], longs,
                          [upairs[k] for k, f in enumerate(rolled) if f], device_keys)


def _routed_arrays(router, datagrams: list, general: bool):
    """_routed_arrays_next without next-phase slots, and without its last item."""
    return _routed_arrays_next(router, datagrams, general, False)[:5]


def _routed_arrays_next(router, datagrams: list, general: bool, next_phase: bool, device_keys: bool = False):
    """What the fused calls of receive_routed and accept_routed take besides
    the datagrams: every key the batch can need is given a slot here, in one
    assign().  Returns (slots, the distinct 1-RTT spaces, their expected
    numbers, the packed per-connection arrays in _crypto.receive_routed's
    order, the DCIDs of the batch's long headers or None, and, only when the
    batch runs with next-phase slots (receive_routed, next_phase=True), the
    distinct 1-RTT pairs and a next-phase slot or SLOT_NONE for each (plus the
    keyless extra one), else None)."""
    conns = router.conns
    pix: dict = {}
    six: dict = {}
    upairs, uspaces, c_pair, c_space = [], [], [], []
    for conn in conns:
        if conn is None:
            c_pair.append(-1)
            c_space.append(-1)
            continue
        pair, space = conn.pair_and_space(Epoch.ONE_RTT, None)
        if id(pair) not in pix:
            pix[id(pair)] = len(upairs)
            upairs.append(pair)
        if id(space) not in six:
            six[id(space)] = len(uspaces)
            uspaces.append(space)
        c_pair.append(pix[id(pair)])
        c_space.append(six[id(space)])
    slots = default_slots()
    keyed = [k for k, p in enumerate(upairs) if p.recv.aead is not None]
    # one more pair (no key) and space than there are: a retired index points at them
    pslot = np.full(len(upairs) + 1, 0xFFFFFFFF, np.uint32)
    # the connections that long-header datagrams of this batch can reach: by
    # the DCID at their start, as qpp_route will find them (None: no long header)
    dcids = None if general else _crypto.long_dcids(datagrams)
    touched = None if dcids is None else sorted({c for c in map(router.index_of, dcids) if c is not None})
    xp: list = []
    if touched:
        # their other key-sets that have keys (a connection past its handshake
        # holds its 1-RTT slot alone)
        sets = {c: _keysets(conns[c]) for c in touched if not conns[c].closed}
        extra = {id(p): p for ks in sets.values() for p in ks if p is not None and p.recv.aead is not None}
        xp = [p for k, p in extra.items() if k not in pix]
    got: list = []
    # next-phase slots: not on the general path, and not when a long header
    # reaches a known connection (_routed_long's walk does not know the rule)
    pnext = None
    if next_phase and not general and not touched and keyed:
        pnext = np.full(len(upairs) + 1, 0xFFFFFFFF, np.uint32)
    if keyed or xp:
        # one assign() for the whole batch: a refill must not take an earlier slot away
        rc = [upairs[k].recv for k in keyed] + [p.recv for p in xp]
        triples = [(c.aead, c.hp, c.key_phase) for c in rc]
        if pnext is not None and device_keys:
            # the batch's current keys first, as without next slots; then the next phases, never
            # by a refill (it would take those away): the missing ones from one device call
            got = slots.assign(triples)
            cur = [upairs[k].recv for k in keyed]
            missing = [c for c in cur if c._next is None]
            unbound = sum(1 for c in cur if c._next is not None
                          and (id(c._next.aead), id(c.hp), int(c._next.key_phase)) not in slots._slot)
            if slots.room() >= len(missing) + unbound:
                setup_next_phase_batch(missing, slots)
                pnext[keyed] = slots.assign([(c._next.aead, c.hp, c._next.key_phase) for c in cur])
            else:
                pnext = None
        elif pnext is not None:
            # the next phase's AEAD key under the current HP key, with the other phase bit
            ahead = [cached_next_phase(upairs[k].recv) for k in keyed]
            try:
                got = slots.assign(triples + [(a.aead, upairs[k].recv.hp, a.key_phase) for a, k in zip(ahead, keyed)])
                pnext[keyed] = got[len(triples):]
                got = got[:len(triples)]
            except OverflowError:
                # the table cannot hold the next slots beside the batch's keys: without them
                pnext = None
        if pnext is None:
            try:
                got = slots.assign(triples)
            except OverflowError:
                if not xp:
                    raise
                # the table cannot hold these key-sets beside the 1-RTT ones: the general path
                dcids, xp = None, []
                got = slots.assign(triples[:len(keyed)])
        pslot[keyed] = got[:len(keyed)]
    sexp = np.asarray([sp.expected_packet_number & 0xFFFFFFFFFFFFFFFF for sp in uspaces] + [0], np.uint64)
    a_pair = np.asarray(c_pair, np.int64)
    a_space = np.asarray(c_space, np.int64)
    a_pair[a_pair < 0] = len(upairs)
    a_space[a_space < 0] = len(uspaces)
    kslot = kexp = b""
    if dcids is not None:
        # the device walk's arrays: a slot per connection and key-set, an
        # expected number per connection and space; only the connections the
        # long headers can reach have more than their 1-RTT entries
        ks_arr = np.full((len(conns), L.KEYSETS), L.SLOT_NONE, np.uint32)
        ke_arr = np.zeros((len(conns), L.SPACES), np.uint64)
        if len(conns):
            ks_arr[:, 4] = pslot[a_pair]
            ks_arr[np.asarray([k for k, c in enumerate(conns) if c is not None and c.closed], np.int64), 4] = L.SLOT_NONE
            ke_arr[:, 2] = sexp[a_space]
        xslot = {id(p): s_ for p, s_ in zip(xp, got[len(keyed):])}
        xslot.update((id(upairs[k]), int(pslot[k])) for k in keyed)
        for c in touched:
            if conns[c].closed:
                continue
            for j, p in enumerate(sets[c]):
                if p is not None:
                    ks_arr[c, j] = xslot.get(id(p), L.SLOT_NONE)
            sp = conns[c].spaces
            for j, e in enumerate((Epoch.INITIAL, Epoch.HANDSHAKE)):
                if e in sp:
                    ke_arr[c, j] = sp[e].expected_packet_number & 0xFFFFFFFFFFFFFFFF
        kslot, kexp = ks_arr.tobytes(), ke_arr.tobytes()
    return slots, uspaces, sexp, (a_pair.astype(np.uint32).tobytes(), a_space.astype(np.uint32).tobytes(),
                                  pslot.tobytes(), sexp.tobytes(), kslot, kexp), dcids, \
        None if pnext is None else (upairs, pnext)


def _routed_finish(router, datagrams: list, slots, uspaces, sexp, route_b, walked, longs, rolled=(),
                   device_keys: bool = False):
    """receive_routed from what its fused call returned; `rolled`: the pairs
    whose keys a packet of the batch updated (next_phase); `device_keys`: they
    are committed, and what is deferred runs, on the batched device calls."""
    conns = router.conns
    route = np.frombuffer(route_b, dtype=L.ROUTE)
    cls, rconn = route["cls"], route["conn"]
    routed = ((cls == L.R_SHORT) | (cls == L.R_LONG)) & (rconn != L.CONN_NONE)
    unrouted = [(int(i), int(cls[i])) for i in np.flatnonzero(~routed)]
    idx = np.flatnonzero(routed)
    if longs is not None:
        recs = _routed_long(conns, datagrams, router.host_cid_length, idx.tolist(), cls, rconn, longs, slots)
        if recs is not None:
            return recs, unrouted
    if walked is None:
        items = [(conns[rconn[i]], datagrams[i]) for i in idx.tolist()]
        back = idx.tolist()
        return [r._replace(datagram=back[r.datagram]) for r in receive_datagrams(items)], unrouted
    recs, deferred, sexp2, closed = walked
    new = np.frombuffer(sexp2, dtype=np.uint64)
    for k in np.flatnonzero(new != sexp).tolist():
        uspaces[k].expected_packet_number = int(new[k])
    for k, f in enumerate(closed):
        if f and conns[k] is not None:
            conns[k].closed = True
    if device_keys:
        # _update_key_cached for all of them: the send directions from one device call
        update_keys_batch(rolled, "remote_update", slots)
        rolled = ()
    for pair in rolled:
        # both directions, as _update_key does; the receive one adopts the
        # cached context, whose slot then is the current one as it stands
        pair._update_key_cached("remote_update")
    if deferred:
        # key-phase flips and numbers decoded under a stale expected number:
        # the general walk takes them in order from the state left above
        rb = ReceiveBatch(slots=slots, device_keys=device_keys)
        at = idx.tolist()
        for j in deferred:
            conn = conns[rconn[at[j]]]
            pair, space = conn.pair_and_space(Epoch.ONE_RTT, None)
            rb.add(pair, datagrams[at[j]], 1 + conn.host_cid_length, space=space, conn=conn, reserved_mask=_RSV_SHORT)
        for j, res in zip(deferred, rb.run()):
            recs[j] = _record((at[j], 0, None, QuicPacketType.ONE_RTT, Epoch.ONE_RTT), res)
            if isinstance(res, ReservedBitsError):
                conns[rconn[at[j]]].closed = True
    return recs, unrouted


def _host_walk_needed(conns, rconn, lidx: list, walk, wn: list) -> bool:
    """_routed_long's two reasons to leave a batch to the general path, asked
    before any state is touched: a datagram the device left to the host walk,
    or a known connection's keyed Initial of a version that is neither 1 nor 2."""
    live = np.arange(L.WALK_MAX)[None, :] < np.asarray(wn, np.int64)[:, None]
    if ((walk["status"] == L.W_HOST) & live).any():
        return True
    odd = live & (walk["status"] == L.W_OK) & (walk["type"] == QuicPacketType.INITIAL.value) \
        & (walk["version"] != int(_V1)) & (walk["version"] != int(_V2))
    for r, k in zip(*np.nonzero(odd)):
        c = int(rconn[lidx[r]])
        if c == L.CONN_NONE or c >= len(conns) or conns[c] is None or conns[c].closed:
            continue
        pair, _ = conns[c].pair_and_space(Epoch.INITIAL, int(walk["version"][r, k]))
        if pair is not None and pair.recv.aead is not None:
            return True
    return False


def accept_routed(router, datagrams: Sequence[bytes], accept, *, need_token: bool = False):
    """receive_routed for a server that also takes on new connections.

    Returns (records, unrouted, accepted).  The first datagrams of a new
    connection no longer stop in `unrouted`: in the same fused call that
    routes, walks and unprotects the batch (_crypto.receive_accept), the
    device looks at the walk record of every long-header datagram whose DCID
    the router does not know, decides whether a server may answer it (an
    Initial of version 1 or 2 at the datagram's start, a datagram of at least
    1200 bytes, a DCID of 1..20 bytes and, with `need_token`, a token: the
    checks of asyncio/server.py:60-152), derives the Initial keys of those it
    accepts from their DCIDs, installs them and unprotects their first packet.
    Nothing is parsed on the host and the bytes are uploaded once.

    The host then decides policy with the header in hand.  For the first
    device-accepted datagram of each distinct DCID, in datagram order,
    `accept(header, datagram_index)` returns the new connection: a server's
    ConnectionKeys of the router's host CID length whose
    cryptos_initial[header.version] is an unset pair and whose Initial space
    expects packet number 0 (ValueError otherwise), or None to refuse; a
    refused datagram, and every later one of its DCID, goes to `unrouted`.
    `accept` runs before the new keys are bound to their slots, so it must not
    protect or unprotect packets itself; it may add the connection's host CIDs
    to the router (server.py:149).  An accepted connection's pair ends exactly
    as pair.setup_initial(dcid, is_client=False, version) leaves it, its two
    slots are bound to its keys, it enters the router under the original DCID
    (server.py:148), and the pairs of its other supported versions get their
    keys from one setup_initial_batch call over all accepted connections
    (connection.py:1509-1515).  The accepted datagrams then join the routed
    ones in the policy pass and the in-order walk, packet 0 from the fused
    launch's results; `accepted` is [(datagram_index, connection)], one entry
    per new connection.

    Candidates are taken in datagram order and cut to the key slots left
    after the batch's own keys were assigned, two per candidate: the table is
    never cleared and refilled on their account, and the candidates cut come
    back in `unrouted`, as from receive_routed.  The same keys are derived
    once per datagram of a DCID on purpose (no cross-lane dedupe on the
    device); the slots nothing adopted -- of candidates the device rejected,
    of refused ones, of second and later datagrams of one DCID -- are cleared
    in one KeyTable.clear and free again when the call returns.

    A batch that receive_routed would leave to its general path (a datagram
    the device leaves to the host walk, and so on) goes through
    receive_routed, and nothing is accepted.  ValueError for a router that
    holds a client connection checking its host CIDs."""
    return _accept_routed(router, datagrams, accept, need_token, None)[:3]


def answer_routed(router, datagrams: Sequence[bytes], addrs: Sequence[Any], accept, *, tokens=None,
                  supported_versions: Sequence[int] = (1, 0x6B3343CF)):
    """accept_routed for a server that also answers what it does not accept.

    Returns (records, unrouted, accepted, replies).  The two verdicts after
    which the reference's server sends a packet and drops the datagram
    (asyncio/server.py:71-111) no longer come back in `unrouted` to be
    answered one AEAD call at a time: in the same fused call
    (_crypto.receive_accept_reply) a kernel assembles a Version Negotiation
    packet for every candidate Initial of a version that is neither 1 nor 2
    (encode_quic_version_negotiation, quic/packet.py:317-334, advertising
    `supported_versions`) and, in Retry mode, a Retry for every Initial
    without a token (encode_quic_retry, quic/packet.py:288-314), and two
    launches over all of them seal the tokens and append the Retry integrity
    tags.  `replies` is [(datagram_index, packet)] in datagram order, each to
    be sent to addrs[datagram_index]; a replied datagram leaves `unrouted`,
    as server.py returns after its sendto.

    `tokens` is a retry.RetryTokens, or None for a server not in Retry mode:
    then no token is demanded (accept_routed's need_token=False) and only
    Version Negotiation replies are built.  With it, an Initial that carries
    a token is accepted on the device as by accept_routed(need_token=True);
    validating the token (tokens.validate_token(addrs[i], header.token)) is
    `accept`'s, as server.py:112-120 does it before it creates a connection.
    A Retry's source CID is 8 random bytes (server.py:98) and its token is
    what tokens.seal gives for the counter it carries; the counters of one
    call are consecutive, taken with tokens.take.

    Everything else is accept_routed's: the candidates are cut to the key
    slots left (two each, whether they end accepted or answered), and a batch
    that accept_routed hands to receive_routed comes back from there with
    nothing accepted and no replies."""
    return _accept_routed(router, datagrams, accept, tokens is not None, (addrs, tokens, supported_versions))


def serve_routed(router, datagrams: Sequence[bytes], addrs: Sequence[Any], accept, *, tokens,
                 supported_versions: Sequence[int] = (1, 0x6B3343CF)):
    """answer_routed for a server in Retry mode whose tokens the device also
    validates: a Retry-mode server's whole policy for unrouted Initials
    (asyncio/server.py:71-131) in the one fused call (_crypto.receive_serve).

    Returns (records, unrouted, accepted, replies, dropped).  `tokens` is a
    retry.RetryTokens and is required (ValueError for None: a server not in
    Retry mode uses answer_routed).  Where answer_routed accepts every Initial
    that carries a token and leaves tokens.validate_token to `accept`, here a
    kernel finds each candidate's token, one AEAD-only launch opens them all
    under the token key, and the accepting kernel compares the address and
    cuts out the two CIDs before it accepts anything: a token that is not
    ours, or not this address's, costs no keys, no slots and no unprotect.
    The differences to answer_routed:

    `accept` is called as accept(header, datagram_index,
    original_destination_connection_id, retry_source_connection_id), the two
    CIDs from the device's token record, as QuicConnection takes them
    (server.py:125-131); it needs no AEAD call.
    A datagram whose token fails comes back in `dropped`, [(datagram_index,
    layout.TK_* reason)] in datagram order, and neither in `unrouted` nor in
    `replies`: the reference drops it silently (server.py:119-120).

    Two kinds of token the host's validate_token would take are refused here,
    neither of which this server issues: a CID of more than 20 bytes
    (TK_FORM) and a token of more than layout.TOKEN_MAX bytes (TK_LENGTH).
    Everything else is answer_routed's, the fallbacks included: a batch that
    goes through receive_routed comes back with nothing accepted, no replies
    and nothing dropped."""
    if tokens is None:
        raise ValueError("serve_routed is a Retry-mode server's: tokens is required (answer_routed takes None)")
    return _accept_routed(router, datagrams, accept, True, (addrs, tokens, supported_versions), True)


_vn_only = None  # the 3-slot reply table of servers not in Retry mode (its token slot is never used)


def _accept_routed(router, datagrams, accept, need_token: bool, answer, serve: bool = False):
    """accept_routed (answer None), answer_routed (answer = (addrs, tokens,
    supported_versions)) and serve_routed (the same, serve: the tokens are
    validated on the device): (records, unrouted, accepted, replies), and
    with serve also dropped."""
    datagrams = datagrams if isinstance(datagrams, list) else list(datagrams)
    none = ([], [], []) if serve else ([], [])
    if not datagrams:
        return ([], []) + none
    conns = router.conns
    if any(c is not None and c.is_client and c.host_cids is not None for c in conns):
        raise ValueError("accept_routed is a server's: the router holds a client connection")
    cid_len = router.host_cid_length
    slots, _, _, arrays, dcids = _routed_arrays(router, datagrams, False)
    # the rows of the device walk as _crypto lists them: first byte, bit 7
    first = np.fromiter((d[0] if d else 0 for d in datagrams), np.uint8, len(datagrams))
    lidx = np.flatnonzero(first & PACKET_LONG_HEADER).tolist()
    rows, cand = [], []
    if dcids is not None:
        for r, i in enumerate(lidx):
            d = datagrams[i]
            if len(d) >= 6 and d[5] <= L.CID_MAX and len(d) >= 6 + d[5] and router.index_of(d[6:6 + d[5]]) is None:
                rows.append(r), cand.append(i)
        keep = min(len(cand), slots.room() // 2)
        rows, cand = rows[:keep], cand[:keep]
    if not cand:
        return receive_routed(router, datagrams) + none
    sent = tokrec = None
    if answer is not None:
        from .retry import RetryTokens, packed_address

        global _vn_only
        addrs, tokens, versions = answer
        if tokens is None and _vn_only is None:
            _vn_only = RetryTokens()
        reply_args = ((tokens or _vn_only).table,
                      b"".join(packed_address(addrs[i]) for i in cand) if tokens is not None else b"",
                      os.urandom(L.RP_RAND_STRIDE * len(cand)), tokens.take(len(cand)) if tokens is not None else 0,
                      np.asarray(list(versions), np.uint32).tobytes(),
                      L.RP_VN | (L.RP_RETRY if tokens is not None else 0))
    taken = slots.reserve(2 * len(cand))  # inside room(): no refill
    try:
        call_args = (slots.table, router.map, cid_len, datagrams, *arrays, ReceivedPacket, QuicPacketType.ONE_RTT,
                     Epoch.ONE_RTT, bytes(bool(c is not None and c.closed) for c in conns), 1,
                     np.asarray(rows, np.uint32).tobytes(), np.asarray(taken, np.uint32).tobytes(),
                     L.A_NEED_TOKEN if need_token else 0)
        if answer is None:
            route_b, _, longs, found = _crypto.receive_accept(*call_args)
        elif serve:
            route_b, _, longs, found, sent, tokrec_b = _crypto.receive_serve(*call_args, *reply_args)
            tokrec = np.frombuffer(tokrec_b, dtype=L.TOKEN_REC)
        else:
            route_b, _, longs, found, sent = _crypto.receive_accept_reply(*call_args, *reply_args)
        route = np.frombuffer(route_b, dtype=L.ROUTE)
        cls, rconn = route["cls"], route["conn"]
        walk = np.frombuffer(longs[1], dtype=L.WALK).reshape(-1, L.WALK_MAX)
        wn = np.frombuffer(longs[2], np.uint32).tolist()
        host = _host_walk_needed(conns, rconn, lidx, walk, wn)
        acc = np.frombuffer(found[0], dtype=L.ACCEPT)
        km = np.frombuffer(found[1], dtype=L.KEY_MATERIAL)
        by_dcid: dict = {}  # DCID -> its connection, or None once refused
        joined: dict = {}   # datagram -> connection
        new: list = []      # (datagram, connection, candidate, header) per new connection
        for a in () if host else np.flatnonzero(acc["status"] == L.ACC_OK).tolist():
            i, w = cand[a], walk[rows[a], 0]
            data = datagrams[i]
            dcid = data[6:6 + int(w["dcid_len"])]
            if dcid not in by_dcid:
                header = _long_header(data, 0, QuicPacketType.INITIAL, int(w["version"]), int(w["len"]),
                                      int(w["dcid_len"]), int(w["scid_len"]), int(w["token_len"]))
                if tokrec is None:
                    conn = accept(header, i)
                else:
                    t = tokrec[a]
                    conn = accept(header, i, t["odcid"][:int(t["odcid_len"])].tobytes(),
                                  t["rscid"][:int(t["rscid_len"])].tobytes())
                by_dcid[dcid] = conn
                if conn is not None:
                    pair = (conn.cryptos_initial or {}).get(header.version)
                    space = conn.spaces.get(Epoch.INITIAL)
                    if conn.is_client or conn.host_cid_length != cid_len or pair is None \
                            or pair.recv.aead is not None or pair.send.aead is not None:
                        raise ValueError("accept() must return a server connection of the router's host CID length "
                                         "whose Initial pair of the header's version is unset")
                    if space is None or space.expected_packet_number != 0:
                        raise ValueError("accept() must return a connection whose Initial space expects packet 0")
                    new.append((i, conn, a, header))
            if by_dcid[dcid] is not None:
                joined[i] = by_dcid[dcid]
        # the new connections' keys are on the device already: bind their slots, free the rest
        built = [_initial_directions(km, found[2], a, False) for _, _, a, _ in new]
        _install_initial(slots, [c.cryptos_initial[h.version] for _, c, _, h in new], built,
                         [h.version for _, _, _, h in new])
    finally:
        slots.give_back(taken)
    if host:
        return receive_routed(router, datagrams) + none
    dropped = []
    if tokrec is not None:
        bad = np.flatnonzero(acc["status"] == L.ACC_BAD_TOKEN).tolist()
        dropped = [(cand[a], int(tokrec["status"][a])) for a in bad]
    replies = []
    if sent is not None:
        rrec = np.frombuffer(sent[1], dtype=L.REPLY)
        for a in np.flatnonzero(rrec["kind"] != L.RP_KIND_NONE).tolist():
            at = int(rrec["off"][a])
            replies.append((cand[a], sent[0][at:at + int(rrec["len"][a])]))
    others = [(c.cryptos_initial[v], h.destination_cid, v) for _, c, _, h in new for v in c.supported_versions
              if v != h.version and v in c.cryptos_initial and c.cryptos_initial[v].recv.aead is None]
    if others:
        setup_initial_batch([o[0] for o in others], [o[1] for o in others], False, [o[2] for o in others], slots)
    for _, conn, _, header in new:
        router.add(header.destination_cid, conn)  # server.py:148
    routed = ((cls == L.R_SHORT) | (cls == L.R_LONG)) & (rconn != L.CONN_NONE)
    here = routed.copy()
    here[np.asarray(list(joined), np.int64)] = True
    gone = here.copy()
    gone[np.asarray([i for i, _ in replies], np.int64)] = True  # answered: server.py returns after sendto
    gone[np.asarray([i for i, _ in dropped], np.int64)] = True  # a token that failed: dropped silently (:119-120)
    unrouted = [(int(i), int(cls[i])) for i in np.flatnonzero(~gone)]
    recs = _routed_long(router.conns, datagrams, cid_len, np.flatnonzero(here).tolist(), cls, rconn, longs, slots,
                        joined)
    assert recs is not None  # _host_walk_needed ruled its reasons out
    return (recs, unrouted, [(i, c) for i, c, _, _ in new], replies) + ((dropped,) if serve else ())
