"""Batch engine: protect / unprotect many packets per launch.

The per-packet API (aioquic_amd.crypto) issues one launch per packet to stay
call-compatible with aioquic.  Real throughput comes from handing the GPU a
whole batch -- every datagram of a ``datagrams_to_send`` call, or every
datagram a server socket read -- as one descriptor array.  This module is that
interface over device-resident buffers (torch tensors on ``cuda``), plus host
helpers that lay out synthetic or real packets into the descriptor format.

Layout (include/quic_pp.h):
  desc     n x 40 B  (in_off, out_off, len, hdr_len, flags, pn, slot)
  results  n x 16 B  (pn, status, hdr_len, out_len)
  keys     one device table of expanded key slots (KeyTable)
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import layout as L
from . import _crypto

__all__ = ["PacketEngine", "MultiDeviceEngine", "KeySpec", "layout_packets"]


@dataclass
class KeySpec:
    slot: int
    suite: int
    key: bytes
    iv: bytes
    hp: bytes
    key_phase: int = 0


def _ptr(t) -> int:
    return int(t.data_ptr())


class PacketEngine:
    """Device key table + launches on device buffers.

    Buffers are torch.uint8 CUDA tensors (or anything with ``data_ptr()``).
    Calls are asynchronous on ``stream`` (default: torch's current stream).

    ``bucket(desc, n)`` sorts a batch by (suite, key slot) on the device
    (qpp_plan_build); launches given ``plan=`` then run each suite over its
    own bucket and write results in the caller's order.  A server batch that
    interleaves connections wants this; a batch already grouped by key does
    not need it.
    """

    def __init__(self, capacity: int):
        self.table = _crypto.KeyTable(int(capacity))
        self._plan = None
        self._plan_cap = 0

    @property
    def capacity(self) -> int:
        return self.table.capacity

    def set_keys(self, specs) -> None:
        recs = np.concatenate(
            [L.key_material(s.slot, s.suite, s.key, s.iv, s.hp, s.key_phase) for s in specs]
        )
        self.table.set(recs.tobytes())

    def derive_keys(self, secrets: np.ndarray) -> np.ndarray:
        """Batched CryptoContext.setup on the device (qpp_keytab_derive):
        `secrets` are layout.SECRET records; returns the derived KEY_MATERIAL."""
        assert secrets.dtype == L.SECRET
        km = self.table.derive(np.ascontiguousarray(secrets).tobytes())
        return np.frombuffer(km, dtype=L.KEY_MATERIAL).copy()

    def derive_next_keys(self, records: np.ndarray):
        """Batched next_key_phase on the device (qpp_keytab_derive_next):
        `records` are layout.NEXT_PHASE records.  Returns (km, secrets): the
        KEY_MATERIAL of every record's next phase (the record's own
        header-protection key kept) and the updated secrets, (n, 64) uint8,
        zero past the hash length.  Records given SLOT_NONE are returned but
        not installed."""
        assert records.dtype == L.NEXT_PHASE
        km, sec = self.table.derive_next(np.ascontiguousarray(records).tobytes())
        return (np.frombuffer(km, dtype=L.KEY_MATERIAL).copy(),
                np.frombuffer(sec, dtype=np.uint8).reshape(len(records), 64).copy())

    def derive_initial_keys(self, records: np.ndarray):
        """Batched CryptoPair.setup_initial on the device
        (qpp_keytab_derive_initial): `records` are layout.INITIAL records.
        Returns (km, secrets): km[i, 0] / km[i, 1] the KEY_MATERIAL of record
        i's "client in" / "server in" keys (shape (n, 2)), secrets (n, 2, 32)
        uint8.  Directions given SLOT_NONE are returned but not installed."""
        assert records.dtype == L.INITIAL
        km, sec = self.table.derive_initial(np.ascontiguousarray(records).tobytes())
        n = len(records)
        return (np.frombuffer(km, dtype=L.KEY_MATERIAL).reshape(n, 2).copy(),
                np.frombuffer(sec, dtype=np.uint8).reshape(n, 2, 32).copy())

    def set_key_records(self, recs: np.ndarray) -> None:
        assert recs.dtype == L.KEY_MATERIAL
        self.table.set(np.ascontiguousarray(recs).tobytes())

    @staticmethod
    def _stream(stream) -> int:
        if stream is None:
            import torch

            return int(torch.cuda.current_stream().cuda_stream)
        if isinstance(stream, int):
            return stream
        return int(stream.cuda_stream)

    def plan(self, n: int):
        """The engine's bucketing scratch for batches of up to n packets."""
        if self._plan is None or self._plan_cap < n:
            self._plan = _crypto.Plan(max(int(n), 1))
            self._plan_cap = max(int(n), 1)
        return self._plan

    def bucket(self, desc, n: int, stream=None):
        """Sort a device descriptor batch by (suite, slot); returns the plan
        to pass to protect / unprotect of descriptors with the same slots."""
        plan = self.plan(n)
        _crypto.plan_build(plan, self.table, _ptr(desc), int(n), self._stream(stream))
        return plan

    def protect(self, desc, n: int, inbuf, outbuf, results, stream=None, plan=None) -> None:
        _crypto.protect(self.table, _ptr(desc), int(n), _ptr(inbuf), _ptr(outbuf),
                        _ptr(results), self._stream(stream), plan)

    def unprotect(self, desc, n: int, inbuf, outbuf, results, stream=None, plan=None) -> None:
        _crypto.unprotect(self.table, _ptr(desc), int(n), _ptr(inbuf), _ptr(outbuf),
                          _ptr(results), self._stream(stream), plan)

    # ------------------------------------------------------- routing ----

    @staticmethod
    def cid_map(capacity: int):
        """A device-resident connection-ID map (qpp_cidmap) for up to
        `capacity` CIDs: .put(records) / .remove(records) of layout.CID_ENTRY
        bytes, .find(cid), .home(cid), .count, .buckets."""
        return _crypto.CidMap(int(capacity))

    def route(self, cid_map, cid_len: int, offs, lens, n: int, inbuf, conn_slot, conn_expected, n_conn: int,
              route, desc=None, flags: int = 0, stream=None) -> None:
        """qpp_route on device buffers: n raw datagrams (uint64 `offs`, uint32
        `lens` into `inbuf`) to ROUTE records and, unless `desc` is None,
        unprotect-ready DESC records, from the per-connection arrays
        `conn_slot` (uint32) and `conn_expected` (uint64) of n_conn entries."""
        _crypto.route(cid_map, int(cid_len), _ptr(offs), _ptr(lens), int(n), _ptr(inbuf), _ptr(conn_slot),
                      _ptr(conn_expected), int(n_conn), int(flags), 0 if desc is None else _ptr(desc), _ptr(route),
                      self._stream(stream))

    def route_unprotect_host(self, cid_map, cid_len: int, offs, lens, data, conn_slot, conn_expected,
                             out_len: int, flags: int = 0):
        """Route and unprotect a host buffer of raw datagrams in one call
        (qpp_session_route_unprotect).  Returns (out, desc, route, results)."""
        out, desc, route, res = _crypto.route_unprotect_host(
            self.table, cid_map, int(cid_len), np.ascontiguousarray(offs, dtype=np.uint64).tobytes(),
            np.ascontiguousarray(lens, dtype=np.uint32).tobytes(), bytes(data),
            np.ascontiguousarray(conn_slot, dtype=np.uint32).tobytes(),
            np.ascontiguousarray(conn_expected, dtype=np.uint64).tobytes(), int(flags), int(out_len))
        return (np.frombuffer(out, dtype=np.uint8), np.frombuffer(desc, dtype=L.DESC),
                np.frombuffer(route, dtype=L.ROUTE), np.frombuffer(res, dtype=L.RESULT))

    def route_walk(self, cid_len: int, offs, lens, n: int, inbuf, route, long_idx, n_long: int, conn_slot,
                   conn_expected, n_conn: int, desc, walk, walk_n, flags: int = 0, stream=None) -> None:
        """qpp_route_walk on device buffers, after route() on the same stream:
        the header walk of the datagrams `long_idx` (uint32, strictly
        increasing) into WALK records (4 per listed datagram), `walk_n` counts
        and DESC records (`desc` holds n + 3 n_long), from `conn_slot`
        (uint32, n_conn x KEYSETS) and `conn_expected` (uint64, n_conn x SPACES)."""
        _crypto.route_walk(int(cid_len), _ptr(offs), _ptr(lens), int(n), _ptr(inbuf), _ptr(route), _ptr(long_idx),
                           int(n_long), _ptr(conn_slot), _ptr(conn_expected), int(n_conn), int(flags), _ptr(desc),
                           _ptr(walk), _ptr(walk_n), self._stream(stream))

    def route_accept(self, offs, lens, n: int, inbuf, route, long_idx, n_long: int, walk, walk_n, acc_row,
                     acc_slot, n_acc: int, ini, desc, acc, accept_flags: int = 0, flags: int = 0,
                     stream=None) -> None:
        """qpp_route_accept on device buffers, after route() and route_walk()
        on the same stream: the unrouted Initials a server may answer among
        the candidates `acc_row` (uint32 rows of `long_idx`, strictly
        increasing), with two key slots each in `acc_slot` (uint32), into
        INITIAL records (`ini`), ACCEPT records (`acc`) and the accepted
        datagrams' DESC records."""
        _crypto.route_accept(_ptr(offs), _ptr(lens), int(n), _ptr(inbuf), _ptr(route), _ptr(long_idx), int(n_long),
                             _ptr(walk), _ptr(walk_n), _ptr(acc_row), _ptr(acc_slot), int(n_acc), int(accept_flags),
                             int(flags), _ptr(ini), _ptr(desc), _ptr(acc), self._stream(stream))

    @staticmethod
    def route_reply(offs, lens, n: int, inbuf, long_idx, n_long: int, walk, acc_row, acc, n_acc: int, addr, rand,
                    token_ctr: int, versions, reply_flags: int, reply, seal, tag, rec, stream=None) -> None:
        """qpp_route_reply on device buffers, after route_accept() on the same
        stream: the Version Negotiation (RP_VN) and Retry (RP_RETRY) packets
        for the candidates the device did not accept, assembled into `reply`
        (REPLY_STRIDE bytes per candidate) with REPLY records (`rec`) and two
        DESC arrays: `seal` and then `tag` go through protect() of the reply
        key table, in place in `reply`, to seal the tokens and append the
        integrity tags.  `addr` (20 bytes per candidate; None without
        RP_RETRY) and `rand` (16 per candidate) are uint8 device buffers,
        `versions` a host sequence of 1..16 version numbers."""
        _crypto.route_reply(_ptr(offs), _ptr(lens), int(n), _ptr(inbuf), _ptr(long_idx), int(n_long), _ptr(walk),
                            _ptr(acc_row), _ptr(acc), int(n_acc), 0 if addr is None else _ptr(addr), _ptr(rand),
                            int(token_ctr), np.asarray(versions, np.uint32).tobytes(), int(reply_flags), _ptr(reply),
                            _ptr(seal), _ptr(tag), _ptr(rec), PacketEngine._stream(stream))

    @staticmethod
    def route_token(offs, lens, n: int, inbuf, route, long_idx, n_long: int, walk, walk_n, acc_row, n_acc: int,
                    tokdesc, tokrec, accept_flags: int = L.A_NEED_TOKEN, stream=None) -> None:
        """qpp_route_token on device buffers, after route() and route_walk()
        on the same stream: where the Retry token of every candidate's Initial
        lies, as AEAD-only DESC records (`tokdesc`) for unprotect() of the
        reply key table -- from `inbuf` into a token buffer of TOKEN_STRIDE
        bytes per candidate -- and the tokens' preliminary TOKEN_REC records
        (`tokrec`)."""
        _crypto.route_token(_ptr(offs), _ptr(lens), int(n), _ptr(inbuf), _ptr(route), _ptr(long_idx), int(n_long),
                            _ptr(walk), _ptr(walk_n), _ptr(acc_row), int(n_acc), int(accept_flags), _ptr(tokdesc),
                            _ptr(tokrec), PacketEngine._stream(stream))

    def route_accept_tokens(self, offs, lens, n: int, inbuf, route, long_idx, n_long: int, walk, walk_n, acc_row,
                            acc_slot, n_acc: int, addr, tok, tokres, ini, desc, acc, tokrec,
                            accept_flags: int = L.A_NEED_TOKEN, flags: int = 0, stream=None) -> None:
        """qpp_route_accept_tokens on device buffers, after route_token() and
        the unprotect() of its descriptors on the same stream: route_accept()
        with the tokens' verdicts.  `addr` (20 bytes per candidate), `tok`
        (the opened tokens) and `tokres` (their RESULT records) are read;
        `tokrec` is read and rewritten with the final TOKEN_REC records.  A
        candidate whose token fails is ACC_BAD_TOKEN: no keys, no descriptor."""
        _crypto.route_accept_tokens(_ptr(offs), _ptr(lens), int(n), _ptr(inbuf), _ptr(route), _ptr(long_idx),
                                    int(n_long), _ptr(walk), _ptr(walk_n), _ptr(acc_row), _ptr(acc_slot), int(n_acc),
                                    int(accept_flags), int(flags), _ptr(addr), _ptr(tok), _ptr(tokres), _ptr(ini),
                                    _ptr(desc), _ptr(acc), _ptr(tokrec), self._stream(stream))

    def route_walk_unprotect_host(self, cid_map, cid_len: int, offs, lens, data, long_idx, conn_slot,
                                  conn_expected, out_len: int, flags: int = 0):
        """Route, walk the long-header datagrams `long_idx` and unprotect a
        host buffer of raw datagrams in one call
        (qpp_session_route_walk_unprotect).  Returns (out, desc, route,
        results, walk, walk_n); desc and results hold n + 3 n_long entries."""
        out, desc, route, res, walk, walk_n = _crypto.route_walk_unprotect_host(
            self.table, cid_map, int(cid_len), np.ascontiguousarray(offs, dtype=np.uint64).tobytes(),
            np.ascontiguousarray(lens, dtype=np.uint32).tobytes(), bytes(data),
            np.ascontiguousarray(long_idx, dtype=np.uint32).tobytes(),
            np.ascontiguousarray(conn_slot, dtype=np.uint32).tobytes(),
            np.ascontiguousarray(conn_expected, dtype=np.uint64).tobytes(), int(flags), int(out_len))
        return (np.frombuffer(out, dtype=np.uint8), np.frombuffer(desc, dtype=L.DESC),
                np.frombuffer(route, dtype=L.ROUTE), np.frombuffer(res, dtype=L.RESULT),
                np.frombuffer(walk, dtype=L.WALK).reshape(-1, L.WALK_MAX), np.frombuffer(walk_n, dtype=np.uint32))

    def route_phase(self, route, next_slots, n_next: int, desc, n: int, inbuf, phase, stream=None) -> None:
        """qpp_route_phase on device buffers, after route() (and route_walk())
        on the same stream and before unprotect(): descriptors [0, n) whose
        short header carries the other key phase are pointed at their
        connection's next-phase slot `next_slots[route.conn]` (uint32; with
        `route` None, `next_slots[i]` per descriptor) and `phase` (uint8, n)
        says which were."""
        _crypto.route_phase(self.table, 0 if route is None else _ptr(route), _ptr(next_slots), int(n_next),
                            _ptr(desc), int(n), _ptr(inbuf), _ptr(phase), self._stream(stream))

    def send_fill(self, send_conns, n_conn: int, offs, lens, conns, seqs, n: int, buf, desc, rec, buf_len=None,
                  stream=None) -> None:
        """qpp_send_fill on device buffers, before protect() of `desc` on the
        same stream with `buf` as its input: the 1-RTT short header, packet
        number and sample padding of n payloads that lie in `buf` at `offs`
        (uint64) with `lens` (uint32), from the SEND_CONN array `send_conns`
        indexed by `conns` (uint32) and each payload's ordinal among its
        connection's, `seqs` (uint32).  Writes DESC records (`desc`) and
        SEND_REC records (`rec`).  The caller keeps the regions [off -
        SEND_HEAD, off + len + SEND_TAIL) pairwise disjoint; `buf_len`
        defaults to the whole of `buf`."""
        if buf_len is None:
            buf_len = buf.numel() * buf.element_size()
        _crypto.send_fill(self.table, _ptr(send_conns), int(n_conn), _ptr(offs), _ptr(lens), _ptr(conns),
                          _ptr(seqs), int(n), _ptr(buf), int(buf_len), _ptr(desc), _ptr(rec), self._stream(stream))

    def send_protect_host(self, send_conns, offs, lens, conns, seqs, data, out_len: int):
        """Build headers and seal a host buffer of staged payloads in one call
        (qpp_session_send_protect).  Returns (out, desc, records, results)."""
        out, desc, rec, res = _crypto.send_protect_host(
            self.table, np.ascontiguousarray(send_conns, dtype=L.SEND_CONN).tobytes(),
            np.ascontiguousarray(offs, dtype=np.uint64).tobytes(), np.ascontiguousarray(lens, dtype=np.uint32).tobytes(),
            np.ascontiguousarray(conns, dtype=np.uint32).tobytes(),
            np.ascontiguousarray(seqs, dtype=np.uint32).tobytes(), bytes(data), int(out_len))
        return (np.frombuffer(out, dtype=np.uint8), np.frombuffer(desc, dtype=L.DESC),
                np.frombuffer(rec, dtype=L.SEND_REC), np.frombuffer(res, dtype=L.RESULT))

    def route_phase_unprotect_host(self, cid_map, cid_len: int, offs, lens, data, long_idx, conn_slot,
                                   conn_expected, conn_next, out_len: int, flags: int = 0):
        """route_walk_unprotect_host with the peers' key updates resolved on
        the device (qpp_session_route_phase_unprotect): `conn_next` names a
        next-phase slot or SLOT_NONE per connection, or is None.  Returns
        (out, desc, route, results, walk, walk_n, phase)."""
        out, desc, route, res, walk, walk_n, phase = _crypto.route_phase_unprotect_host(
            self.table, cid_map, int(cid_len), np.ascontiguousarray(offs, dtype=np.uint64).tobytes(),
            np.ascontiguousarray(lens, dtype=np.uint32).tobytes(), bytes(data),
            np.ascontiguousarray(long_idx, dtype=np.uint32).tobytes(),
            np.ascontiguousarray(conn_slot, dtype=np.uint32).tobytes(),
            np.ascontiguousarray(conn_expected, dtype=np.uint64).tobytes(),
            None if conn_next is None else np.ascontiguousarray(conn_next, dtype=np.uint32).tobytes(),
            int(flags), int(out_len))
        return (np.frombuffer(out, dtype=np.uint8), np.frombuffer(desc, dtype=L.DESC),
                np.frombuffer(route, dtype=L.ROUTE), np.frombuffer(res, dtype=L.RESULT),
                np.frombuffer(walk, dtype=L.WALK).reshape(-1, L.WALK_MAX), np.frombuffer(walk_n, dtype=np.uint32),
                np.frombuffer(phase, dtype=L.PHASE))

    # ----------------------------------------------- host-buffer forms ----

    def protect_host(self, desc: np.ndarray, data, out_len: int):
        out, res = _crypto.protect_host(self.table, np.ascontiguousarray(desc).tobytes(),
                                        bytes(data), int(out_len))
        return np.frombuffer(out, dtype=np.uint8), np.frombuffer(res, dtype=L.RESULT)

    def unprotect_host(self, desc: np.ndarray, data, out_len: int):
        out, res = _crypto.unprotect_host(self.table, np.ascontiguousarray(desc).tobytes(),
                                          bytes(data), int(out_len))
        return np.frombuffer(out, dtype=np.uint8), np.frombuffer(res, dtype=L.RESULT)


    def protect_into(self, desc: np.ndarray, data, out: np.ndarray, results: np.ndarray) -> None:
        """protect_host into caller-owned buffers (out: uint8, results: RESULT
        array of len(desc)), reusable across batches."""
        self._into(_crypto.protect_into, desc, data, out, results)

    def unprotect_into(self, desc: np.ndarray, data, out: np.ndarray, results: np.ndarray) -> None:
        self._into(_crypto.unprotect_into, desc, data, out, results)

    def _into(self, fn, desc, data, out, results) -> None:
        desc = np.ascontiguousarray(desc, dtype=L.DESC)
        data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8)
                                    if not isinstance(data, np.ndarray) else data.view(np.uint8).ravel())
        if not (out.flags.c_contiguous and out.flags.writeable):
            raise ValueError("out must be a writable contiguous array")
        if not (results.flags.c_contiguous and results.flags.writeable) or \
                results.nbytes < len(desc) * L.RESULT.itemsize:
            raise ValueError("results must be a writable contiguous array of len(desc) records")
        # the arrays stay referenced here for the whole call
        fn(self.table, desc.ctypes.data, len(desc), data.ctypes.data, data.nbytes,
           out.ctypes.data, out.nbytes, results.ctypes.data)


class MultiDeviceEngine:
    """Host-buffer batches split over several GPUs of the node (qpp_multi):
    the batch's descriptors are cut into contiguous ranges, one per device,
    each device holds its own replica of the key table and its own pinned
    staging, and the results come back in the caller's order -- the bytes of
    PacketEngine.protect_host on one device.  `devices` defaults to every
    visible GPU; a device may be listed twice (two sessions on one GPU)."""

    def __init__(self, capacity: int, devices=None):
        if devices is None:
            import torch

            devices = list(range(torch.cuda.device_count()))
        self.devices = list(devices)
        self.multi = _crypto.MultiSession(self.devices, int(capacity))

    def set_key_records(self, recs: np.ndarray) -> None:
        assert recs.dtype == L.KEY_MATERIAL
        self.multi.set_keys(np.ascontiguousarray(recs).tobytes())

    def protect_host(self, desc: np.ndarray, data, out_len: int):
        out, res = self.multi.protect(np.ascontiguousarray(desc).tobytes(), bytes(data), int(out_len))
        return np.frombuffer(out, dtype=np.uint8), np.frombuffer(res, dtype=L.RESULT)

    def unprotect_host(self, desc: np.ndarray, data, out_len: int):
        out, res = self.multi.unprotect(np.ascontiguousarray(desc).tobytes(), bytes(data), int(out_len))
        return np.frombuffer(out, dtype=np.uint8), np.frombuffer(res, dtype=L.RESULT)

    def protect_into(self, desc: np.ndarray, data: np.ndarray, out: np.ndarray, results: np.ndarray) -> None:
        """protect_host into caller-owned arrays, reusable across batches."""
        _into_arrays(self.multi.protect_into, desc, data, out, results)

    def unprotect_into(self, desc: np.ndarray, data: np.ndarray, out: np.ndarray, results: np.ndarray) -> None:
        _into_arrays(self.multi.unprotect_into, desc, data, out, results)

    def trace(self, enable=None) -> list:
        """Per device, the host-copy / PCIe / kernel phases of its session's
        last traced pipelined call (qpp_multi_trace); enable=True / False turns
        tracing on / off for the following calls."""
        return self.multi.trace(-1 if enable is None else int(bool(enable)))


def _into_arrays(fn, desc, data, out, results) -> None:
    desc = np.ascontiguousarray(desc, dtype=L.DESC)
    data = np.ascontiguousarray(data).view(np.uint8).ravel()
    if not (out.flags.c_contiguous and out.flags.writeable):
        raise ValueError("out must be a writable contiguous array")
    if not (results.flags.c_contiguous and results.flags.writeable) or \
            results.nbytes < len(desc) * L.RESULT.itemsize:
        raise ValueError("results must be a writable contiguous array of len(desc) records")
    fn(desc.ctypes.data, len(desc), data.ctypes.data, data.nbytes, out.ctypes.data, out.nbytes,
       results.ctypes.data)


def layout_packets(headers, payloads, pns, slots, *, align: int = 1, tag_room: bool = True,
                   flags: int = 0, payload_align: int = 1):
    """Pack (header, payload) pairs into one input buffer and build protect
    descriptors whose outputs go to the same offsets of an output buffer.

    align: each packet starts on a multiple of it.  payload_align: each
    packet is placed so that its payload (after the header) starts on a
    multiple of it instead -- 16 saves the kernels' 16-byte loads and stores
    a second segment each (Payload alignment).

    Returns (inbuf uint8 array, desc array, out_size)."""
    n = len(headers)
    desc = np.zeros(n, dtype=L.DESC)
    sizes = [len(h) + len(p) + (L.TAG_LEN if tag_room else 0) for h, p in zip(headers, payloads)]
    offs = np.zeros(n, dtype=np.int64)
    pos = 0
    for i, s in enumerate(sizes):
        if payload_align > 1:
            hl = len(headers[i])
            pos = (pos + hl + payload_align - 1) // payload_align * payload_align - hl
        else:
            pos = (pos + align - 1) // align * align
        offs[i] = pos
        pos += s
    buf = np.zeros(pos + 16, dtype=np.uint8)
    for i, (h, p) in enumerate(zip(headers, payloads)):
        o = int(offs[i])
        buf[o : o + len(h)] = np.frombuffer(h, dtype=np.uint8)
        buf[o + len(h) : o + len(h) + len(p)] = np.frombuffer(p, dtype=np.uint8)
    desc["in_off"] = offs
    desc["out_off"] = offs
    desc["len"] = [len(p) for p in payloads]
    desc["hdr_len"] = [len(h) for h in headers]
    desc["pn"] = np.asarray(pns, dtype=np.uint64)
    desc["slot"] = np.asarray(slots, dtype=np.uint32)
    desc["flags"] = flags
    return buf, desc, pos + 16
