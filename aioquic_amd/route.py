"""Routing received datagrams to connections by connection ID on the device.

The reference's server demultiplexes one datagram at a time in Python
(asyncio/server.py:60-152: pull_quic_header, then
``self._protocols.get(header.destination_cid)``) and keeps that dict current
from ``_connection_id_issued`` / ``_connection_id_retired`` (server.py:154-170).
CidRouter is that bookkeeping over a device-resident map (``_crypto.CidMap``,
qpp_cidmap): ``add`` and ``retire`` are the two hooks, and
``receive.receive_routed(router, datagrams)`` receives a batch of raw
datagrams nobody has demultiplexed.
"""

from __future__ import annotations

from typing import Dict, List, Optional

from . import _crypto
from . import layout as L

__all__ = ["CidRouter"]


class CidRouter:
    """Connection IDs of one endpoint -> its connections.

    `host_cid_length` is the endpoint's fixed CID length
    (configuration.connection_id_length): every short header is read with it.
    `capacity` bounds the CIDs held at once.  `conns[i]` is the connection
    (receive.ConnectionKeys) of index i, or None once its last CID is retired;
    indices are reused."""

    def __init__(self, host_cid_length: int, capacity: int):
        if not 1 <= host_cid_length <= L.CID_MAX:
            raise ValueError("host_cid_length must be 1..20")
        self.host_cid_length = host_cid_length
        self.map = _crypto.CidMap(int(capacity))
        self.conns: List[Optional[object]] = []
        self._index: Dict[int, int] = {}   # id(connection) -> index
        self._cids: Dict[bytes, int] = {}  # CID -> index
        self._refs: List[int] = []         # CIDs per index
        self._free: List[int] = []

    def __len__(self) -> int:
        return len(self._cids)

    def index_of(self, cid: bytes) -> Optional[int]:
        """The index `cid` routes to, or None."""
        return self._cids.get(bytes(cid))

    def add(self, cid: bytes, conn) -> int:
        """_connection_id_issued: route `cid` to `conn`; returns its index."""
        if conn.host_cid_length != self.host_cid_length:
            raise ValueError("the connection's host_cid_length differs from the router's")
        cid = bytes(cid)
        idx = self._index.get(id(conn))
        fresh = idx is None
        if fresh:
            idx = self._free[-1] if self._free else len(self.conns)
        self.map.put(L.cid_entry(cid, idx).tobytes())  # raises before anything is changed here
        if fresh:
            if self._free:
                self._free.pop()
                self.conns[idx] = conn
            else:
                self.conns.append(conn)
                self._refs.append(0)
            self._index[id(conn)] = idx
        old = self._cids.get(cid)
        if old != idx:
            if old is not None:
                self._unref(old)
            self._cids[cid] = idx
            self._refs[idx] += 1
        return idx

    def retire(self, cid: bytes) -> None:
        """_connection_id_retired: an unknown CID is ignored."""
        cid = bytes(cid)
        idx = self._cids.pop(cid, None)
        if idx is None:
            return
        self.map.remove(L.cid_entry(cid).tobytes())
        self._unref(idx)

    def _unref(self, idx: int) -> None:
        self._refs[idx] -= 1
        if self._refs[idx] == 0:
            del self._index[id(self.conns[idx])]
            self.conns[idx] = None
            self._free.append(idx)
