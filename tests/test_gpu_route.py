"""GPU checks of the routing layer (include/quic_pp.h: qpp_cidmap_*, qpp_route,
qpp_session_route_unprotect) and of receive.receive_routed.

The reference is a restatement written here: a Python dict for the map and a
per-datagram loop for the classes and descriptors (`restate`), the CPU oracle
(oracle.protect_batch, the C restatement of the reference's per-packet path)
for the traffic, and receive_datagrams on pre-demultiplexed items for the
records."""

from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from tests import receive_scenario as RS

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _watchdog():
    from aioquic_amd import _crypto

    yield
    assert _crypto.watchdog_count() == 0


# ------------------------------------------------------------- restatement --

def restate(table: dict, cid_len, offs, lens, buf, conn_slot, conn_exp, flags=0):
    """(DESC array, ROUTE array) of quic_pp.h's qpp_route, datagram by datagram."""
    from aioquic_amd import layout as L

    n = len(offs)
    desc = np.zeros(n, dtype=L.DESC)
    route = np.zeros(n, dtype=L.ROUTE)
    raw = buf.tobytes()
    for i in range(n):
        o, ln = int(offs[i]), int(lens[i])
        d = raw[o:o + ln]
        cls, conn = L.R_MALFORMED, NONE
        if ln and d[0] & 0xC0:
            if not d[0] & 0x80:
                if ln >= 1 + cid_len:
                    conn = table.get(d[1:1 + cid_len], NONE)
                    cls = L.R_SHORT if conn != NONE else L.R_UNKNOWN_CID
            elif ln >= 6 and d[5] <= 20 and ln >= 6 + d[5]:
                cls = L.R_LONG
                conn = table.get(d[6:6 + d[5]], NONE) if d[5] else NONE
        if conn != NONE and conn >= len(conn_slot):
            cls = L.R_BAD_CONN
        desc["in_off"][i] = desc["out_off"][i] = o
        desc["flags"][i] = flags
        desc["slot"][i] = L.SLOT_NONE
        if cls == L.R_SHORT:
            desc["len"][i] = ln
            desc["hdr_len"][i] = 1 + cid_len
            desc["pn"][i] = conn_exp[conn]
            desc["slot"][i] = conn_slot[conn]
        route["conn"][i] = conn
        route["cls"][i] = cls
    return desc, route


def entries(pairs):
    from aioquic_amd import layout as L

    return np.concatenate([L.cid_entry(c, k) for c, k in pairs]).tobytes()


def displaced_map(eng, cid_len, rng, n_good=6, bad_conn=100):
    """A 16-bucket map with 8 entries, one of them displaced from its home:
    n_good CIDs of cid_len for connections 0.., one whose conn is past every
    conn array, and one of another length.  -> (map, dict)."""
    m = eng.cid_map(8)
    assert m.buckets == 16
    cids = []
    while len(cids) < n_good:
        c = rng.bytes(cid_len)
        if c not in cids:
            cids.append(c)
    while True:  # one more that shares the first one's home, so it cannot sit there
        c = bytes([int(rng.integers(256))]) if cid_len == 1 else rng.bytes(cid_len)
        if c not in cids and m.home(c) == m.home(cids[0]):
            cids.append(c)
            break
    other = rng.bytes(5 if cid_len == 20 else 20)
    table = {c: k for k, c in enumerate(cids[:n_good])}
    table[cids[n_good]] = bad_conn
    table[other] = 1
    m.put(entries(table.items()))
    assert m.count == 8
    for c, k in table.items():
        assert m.find(c) == k
    return m, table


def mixed_datagrams(table, cid_len, n, rng, bad_conn=100):
    """n datagrams of every class at odd offsets; the last is a short header of
    exactly 1 + cid_len bytes that ends the buffer.  -> (buf, offs, lens)."""
    good = [c for c, k in table.items() if len(c) == cid_len and k != bad_conn]
    bad = [c for c, k in table.items() if k == bad_conn][0]
    other = [c for c in table if len(c) != cid_len][0]

    def unknown(ln):
        while True:
            c = rng.bytes(ln)
            if c not in table:
                return c

    def long_(dcid, extra=30):
        return bytes([0xC0 | int(rng.integers(0, 64))]) + b"\x00\x00\x00\x01" + bytes([len(dcid)]) + dcid + rng.bytes(extra)

    kinds = [
        lambda: bytes([0x40 | int(rng.integers(0, 64))]) + good[int(rng.integers(len(good)))] + rng.bytes(int(rng.integers(0, 60))),
        lambda: bytes([0x41]) + unknown(cid_len) + rng.bytes(25),
        lambda: long_(good[int(rng.integers(len(good)))]),
        lambda: long_(unknown(cid_len)),
        lambda: long_(other, extra=0),                       # a known DCID of another length, ending the datagram
        lambda: long_(b""),
        lambda: bytes([int(rng.integers(0, 64))]) + rng.bytes(30),  # no fixed bit
        lambda: bytes([0x40]) + good[0][:cid_len - 1],         # short of its CID by one byte
        lambda: bytes([0xC0]) + b"\x00\x00\x00\x01" + bytes([21]) + rng.bytes(40),
        lambda: b"",
        lambda: bytes([0x43]) + bad + rng.bytes(20),
        lambda: long_(bad),
        lambda: long_(good[0])[:5],
        lambda: long_(good[0], extra=0)[:-1],                 # one byte short of the DCID's end
        lambda: bytes([0x80]) + b"\x00\x00\x00\x00" + bytes([len(other)]) + other,
    ]
    dgs = [kinds[i % len(kinds)]() for i in range(max(n - 1, 0))]
    if n:
        dgs.append(bytes([0x40]) + good[-1])
    offs, lens, pos = [], [], 1
    for d in dgs:
        offs.append(pos)
        lens.append(len(d))
        pos += len(d)
        pos += 1 - pos % 2  # the next odd offset
    size = offs[-1] + lens[-1] if n else 1
    buf = rng.integers(0, 256, size, dtype=np.uint8)
    for o, d in zip(offs, dgs):
        buf[o:o + len(d)] = np.frombuffer(d, np.uint8)
    return buf, np.asarray(offs, np.uint64), np.asarray(lens, np.uint32)


def run_route(eng, dev, m, cid_len, offs, lens, buf, conn_slot, conn_exp, flags=0, with_desc=True):
    import torch
    from aioquic_amd import layout as L

    n = len(offs)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_desc = torch.full((max(n, 1) * 40 + 8,), 0xAB, dtype=torch.uint8, device=dev)
    d_route = torch.full((max(n, 1) * 8 + 8,), 0xAB, dtype=torch.uint8, device=dev)
    pad = lambda a, item: a if len(a) else np.zeros(1, a.dtype)
    eng.route(m, cid_len, t(pad(offs, 8)), t(pad(lens, 4)), n, t(buf), t(pad(conn_slot, 4)), t(pad(conn_exp, 8)),
              len(conn_slot), d_route, desc=d_desc if with_desc else None, flags=flags)
    torch.cuda.synchronize()
    desc, route = d_desc.cpu().numpy(), d_route.cpu().numpy()
    assert (desc[n * 40:] == 0xAB).all() and (route[n * 8:] == 0xAB).all(), "wrote past the n records"
    return desc[:n * 40].view(L.DESC) if with_desc else desc, route[:n * 8].view(L.ROUTE)


# ------------------------------------------------------------------ qpp_route --

@pytest.mark.parametrize("cid_len", [1, 4, 8, 20])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_route_matches_restatement(dev, n, cid_len):
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    rng = np.random.default_rng(1000 * cid_len + n)
    eng = PacketEngine(8)
    m, table = displaced_map(eng, cid_len, rng)
    assert any(m.home(c) != b for c, b in _buckets_of(m, table).items()), "no displaced entry"
    buf, offs, lens = mixed_datagrams(table, cid_len, n, rng)
    if n:
        assert int(offs[-1]) + int(lens[-1]) == len(buf) and lens[-1] == 1 + cid_len
        assert (offs % 2 == 1).all()
    conn_slot = np.asarray([3, 0, L.SLOT_NONE, 7, 2, 5, 1, 4], np.uint32)
    conn_exp = rng.integers(0, 1 << 62, 8, dtype=np.uint64)
    want_d, want_r = restate(table, cid_len, offs, lens, buf, conn_slot, conn_exp, flags=L.F_RFC_PN)
    got_d, got_r = run_route(eng, dev, m, cid_len, offs, lens, buf, conn_slot, conn_exp, flags=L.F_RFC_PN)
    assert got_r["conn"].tolist() == want_r["conn"].tolist()
    assert got_r["cls"].tolist() == want_r["cls"].tolist()
    assert got_d.tobytes() == want_d.tobytes()
    if n >= 63:
        assert set(want_r["cls"].tolist()) == {L.R_SHORT, L.R_LONG, L.R_UNKNOWN_CID, L.R_MALFORMED, L.R_BAD_CONN}
        longs = want_r[want_r["cls"] == L.R_LONG]
        assert (longs["conn"] == NONE).any() and (longs["conn"] != NONE).any()
        skipped = want_r["cls"] != L.R_SHORT
        assert (got_d["in_off"][skipped] == offs[skipped]).all() and (got_d["out_off"][skipped] == offs[skipped]).all()
        assert (got_d["slot"][skipped] == L.SLOT_NONE).all() and (got_d["len"][skipped] == 0).all()
    # desc = NULL: only the route records are written
    untouched, only_r = run_route(eng, dev, m, cid_len, offs, lens, buf, conn_slot, conn_exp, with_desc=False)
    assert (untouched == 0xAB).all()
    assert only_r.tobytes() == got_r.tobytes()


def _buckets_of(m, table):
    """Where each CID sits, by the rule the map documents: linear probing from
    home in insertion order (no removals so far)."""
    used, out = set(), {}
    for c in table:
        b = m.home(c)
        while b in used:
            b = (b + 1) % m.buckets
        used.add(b)
        out[c] = b
    return out


def test_route_rejects_bad_cid_len(dev):
    import torch
    from aioquic_amd.batch import PacketEngine

    eng = PacketEngine(1)
    m = eng.cid_map(4)
    z = torch.zeros(64, dtype=torch.uint8, device=dev)
    for bad in (0, 21):
        with pytest.raises(ValueError):
            eng.route(m, bad, z, z, 1, z, z, z, 1, z, desc=z)
    with pytest.raises(ValueError):
        m.put(entries([(b"abcd", 0)]) [:-1])
    with pytest.raises(ValueError):
        eng.cid_map(0)


def test_route_sees_put_and_remove_between_launches(dev):
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    rng = np.random.default_rng(5)
    eng = PacketEngine(4)
    m = eng.cid_map(64)
    cids = [rng.bytes(8) for _ in range(40)]
    table = {c: k % 16 for k, c in enumerate(cids[:20])}
    m.put(entries(table.items()))
    dgs = [bytes([0x40]) + c + rng.bytes(24) for c in cids]
    lens = np.full(len(dgs), 33, np.uint32)
    offs = (np.arange(len(dgs)) * 33).astype(np.uint64)
    buf = np.frombuffer(b"".join(dgs), np.uint8)
    conn_slot = np.arange(16, dtype=np.uint32) % 4
    conn_exp = np.arange(16, dtype=np.uint64) * 1000
    for step in range(3):
        want_d, want_r = restate(table, 8, offs, lens, buf, conn_slot, conn_exp)
        got_d, got_r = run_route(eng, dev, m, 8, offs, lens, buf, conn_slot, conn_exp)
        assert got_r.tobytes() == want_r.tobytes() and got_d.tobytes() == want_d.tobytes()
        assert (want_r["cls"] == L.R_SHORT).sum() == len(table)
        if step == 0:
            # retire half of the old ones, issue new ones, move one to another connection
            gone = cids[:20:2]
            m.remove(entries([(c, 0) for c in gone]))
            for c in gone:
                del table[c]
            new = {c: (k * 7) % 16 for k, c in enumerate(cids[20:35])}
            new[cids[1]] = 15
            m.put(entries(new.items()))
            table.update(new)
        elif step == 1:
            m.remove(entries([(c, 0) for c in list(table)]))
            table.clear()
        assert m.count == len(table)


# ------------------------------------------------------ traffic from the oracle --

class Traffic:
    """n short-header 1-RTT packets over n_conns connections in random arrival
    order, protected by the CPU oracle; connection c uses key slot c and an
    8-byte CID; a few datagrams are then spoilt (unknown CID, no fixed bit)."""

    def __init__(self, n, n_conns, seed, spoil=24):
        from aioquic_amd import layout as L
        from aioquic_amd.bench_data import make_keys
        from aioquic_amd.packet import QuicProtocolVersion
        from oracle import oracle as orc

        rng = np.random.default_rng(seed)
        self.n, self.n_conns = n, n_conns
        self.keys = make_keys(n_conns, [L.AES_128_GCM, L.AES_256_GCM, L.CHACHA20_POLY1305], seed,
                              int(QuicProtocolVersion.VERSION_1), random_suites=True)
        cid = rng.integers(0, 256, (n_conns, 8), dtype=np.uint8)
        cid[:, :4] = np.arange(n_conns, dtype=">u4").view(np.uint8).reshape(n_conns, 4)  # distinct
        self.cids = [cid[c].tobytes() for c in range(n_conns)]
        conn = rng.integers(0, n_conns, n).astype(np.uint32)
        order = np.argsort(conn, kind="stable")
        counts = np.bincount(conn, minlength=n_conns)
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
        pn = np.empty(n, np.int64)
        pn[order] = np.arange(n) - np.repeat(starts, counts)
        plen = rng.integers(24, 120, n)
        size = 11 + plen + 16
        offs = np.concatenate([[1], 1 + np.cumsum(size + (size % 2 == 1))[:-1]]).astype(np.int64)  # odd offsets
        total = int(offs[-1] + size[-1])
        plain = rng.integers(0, 256, total, dtype=np.uint8)
        plain[offs] = 0x41
        for k in range(8):
            plain[offs + 1 + k] = cid[conn, k]
        plain[offs + 9] = (pn >> 8) & 0xFF
        plain[offs + 10] = pn & 0xFF
        tag = (offs + 11 + plen)[:, None] + np.arange(16)[None, :]
        plain[tag.ravel()] = 0
        pdesc = np.zeros(n, dtype=L.DESC)
        pdesc["in_off"] = pdesc["out_off"] = offs
        pdesc["len"] = plen
        pdesc["hdr_len"] = 11
        pdesc["pn"] = pn
        pdesc["slot"] = conn
        wire, res = orc.protect_batch(self.keys, pdesc, plain, total)
        assert (res["status"] == 0).all()
        # gaps between packets: not the oracle's business
        self.offs, self.lens = offs.astype(np.uint64), size.astype(np.uint32)
        self.conn = conn
        self.expect = plain.copy()  # what unprotect leaves: header | plaintext, zeros elsewhere
        gaps = np.ones(total, bool)
        body = offs[:, None] + np.arange(int(size.max()))[None, :]
        keep = np.arange(int(size.max()))[None, :] < (11 + plen)[:, None]
        gaps[body[keep]] = False
        self.expect[gaps] = 0
        for i in rng.choice(n, spoil, replace=False).tolist() if spoil else []:
            o = int(offs[i])
            if i % 2:
                wire[o] &= 0x3F
            else:
                wire[o + 1:o + 5] = 0xFF  # no connection has this CID
            self.expect[o:o + int(size[i])] = 0
        self.wire = wire
        self.table = {c: k for k, c in enumerate(self.cids)}
        self.conn_slot = np.arange(n_conns, dtype=np.uint32)
        self.conn_exp = np.zeros(n_conns, np.uint64)


@pytest.fixture(scope="module")
def big():
    return Traffic(64 * 1024, 4096, seed=0xB16)


@pytest.fixture(scope="module")
def big_restated(big):
    return restate(big.table, 8, big.offs, big.lens, big.wire, big.conn_slot, big.conn_exp)


def _engine_for(tr):
    from aioquic_amd.batch import PacketEngine

    eng = PacketEngine(tr.n_conns)
    eng.set_key_records(tr.keys)
    m = eng.cid_map(tr.n_conns)
    m.put(entries(tr.table.items()))
    return eng, m


def test_64ki_datagrams_route_then_unprotect(dev, big, big_restated):
    import torch
    from aioquic_amd import layout as L

    tr = big
    want_d, want_r = big_restated
    eng, m = _engine_for(tr)
    assert m.count == 4096 and m.buckets == 8192
    n = tr.n
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d_in = t(tr.wire)
    d_desc = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    d_route = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
    eng.route(m, 8, t(tr.offs), t(tr.lens), n, d_in, t(tr.conn_slot), t(tr.conn_exp), tr.n_conns, d_route, desc=d_desc)
    outs = []
    # planned, unplanned, and unplanned over descriptors built on the host
    for desc, planned in ((d_desc, True), (d_desc, False), (t(want_d), False)):
        d_out = torch.zeros(len(tr.wire), dtype=torch.uint8, device=dev)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        plan = eng.bucket(desc, n) if planned else None
        eng.unprotect(desc, n, d_in, d_out, d_res, plan=plan)
        torch.cuda.synchronize()
        outs.append((d_out.cpu().numpy(), d_res.cpu().numpy().view(L.RESULT)))
    got_d, got_r = d_desc.cpu().numpy().view(L.DESC), d_route.cpu().numpy().view(L.ROUTE)
    assert got_r["conn"].tolist() == want_r["conn"].tolist() and got_r["cls"].tolist() == want_r["cls"].tolist()
    assert got_d.tobytes() == want_d.tobytes()
    routed = want_r["cls"] == L.R_SHORT
    assert routed.sum() == n - 24 and (want_r["conn"][routed] == tr.conn[routed]).all()
    for out, res in outs:
        assert (res["status"][routed] == L.S_OK).all() and (res["status"][~routed] == L.S_NO_KEY).all()
        assert np.array_equal(out, tr.expect), "plaintext differs from the oracle's input"
        assert res.tobytes() == outs[2][1].tobytes()
    assert (outs[0][1]["pn"][routed] == _pn_of(tr)[routed]).all()


def _pn_of(tr):
    return (tr.expect[tr.offs.astype(np.int64) + 9].astype(np.uint64) << np.uint64(8)) | \
        tr.expect[tr.offs.astype(np.int64) + 10].astype(np.uint64)


@pytest.fixture(scope="module")
def small():
    return Traffic(300, 8, seed=0x5311, spoil=10)


def test_route_unprotect_host_equals_device_path(dev, small):
    import torch
    from aioquic_amd import layout as L

    tr = small
    eng, m = _engine_for(tr)
    n = tr.n
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    d_in = t(tr.wire)
    d_desc = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    d_route = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(len(tr.wire), dtype=torch.uint8, device=dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    conn_slot = tr.conn_slot.copy()
    conn_slot[3] = L.SLOT_NONE  # a connection without a receive key
    eng.route(m, 8, t(tr.offs), t(tr.lens), n, d_in, t(conn_slot), t(tr.conn_exp), tr.n_conns, d_route, desc=d_desc)
    eng.unprotect(d_desc, n, d_in, d_out, d_res)
    torch.cuda.synchronize()
    out, desc, route, res = eng.route_unprotect_host(m, 8, tr.offs, tr.lens, tr.wire, conn_slot, tr.conn_exp,
                                                     len(tr.wire))
    assert desc.tobytes() == d_desc.cpu().numpy().tobytes()
    assert route["conn"].tolist() == d_route.cpu().numpy().view(L.ROUTE)["conn"].tolist()
    assert route["cls"].tolist() == d_route.cpu().numpy().view(L.ROUTE)["cls"].tolist()
    assert res.tobytes() == d_res.cpu().numpy().tobytes()
    assert np.array_equal(out, d_out.cpu().numpy())
    want_d, want_r = restate(tr.table, 8, tr.offs, tr.lens, tr.wire, conn_slot, tr.conn_exp)
    assert desc.tobytes() == want_d.tobytes() and route["cls"].tolist() == want_r["cls"].tolist()
    ok = (want_r["cls"] == L.R_SHORT) & (tr.conn != 3)
    assert (res["status"][ok] == L.S_OK).all() and (res["status"][~ok] == L.S_NO_KEY).all()
    expect = tr.expect.copy()
    for i in np.flatnonzero(tr.conn == 3).tolist():
        expect[int(tr.offs[i]):int(tr.offs[i]) + int(tr.lens[i])] = 0
    assert np.array_equal(out, expect)
    # an empty batch
    out0, desc0, route0, res0 = eng.route_unprotect_host(m, 8, [], [], b"", conn_slot, tr.conn_exp, 16)
    assert len(desc0) == len(route0) == len(res0) == 0 and not out0.any()


def test_route_unprotect_host_bounds(dev, small):
    """A datagram outside the input or the output buffer: QPP_E_ARG, and the
    caller's output is not touched (the C ABI itself, through ctypes)."""
    import aioquic_amd  # noqa: F401  (binds torch's HIP runtime first)
    from aioquic_amd import layout as L

    lib = ctypes.CDLL(os.path.join(ROOT, "aioquic_amd", "libquicpp.so"))
    vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    lib.qpp_session_route_unprotect.restype = ctypes.c_int
    lib.qpp_session_route_unprotect.argtypes = [vp, vp, vp, u32, vp, vp, u32, vp, sz, vp, vp, u32, ctypes.c_uint16,
                                                vp, sz, vp, vp, vp]
    lib.qpp_cidmap_put.argtypes = [vp, vp, u32, vp]
    for f in (lib.qpp_keytab_destroy, lib.qpp_cidmap_destroy, lib.qpp_session_destroy):
        f.argtypes = [vp]
        f.restype = None
    kt, m, s = vp(), vp(), vp()
    assert lib.qpp_keytab_create(u32(8), ctypes.byref(kt)) == 0
    assert lib.qpp_cidmap_create(u32(8), ctypes.byref(m)) == 0
    assert lib.qpp_session_create(sz(4096), u32(64), ctypes.byref(s)) == 0
    try:
        tr = small
        ent = np.frombuffer(entries(tr.table.items()), np.uint8).copy()
        assert lib.qpp_cidmap_put(m, ent.ctypes.data, len(tr.table), None) == 0
        n = 40
        offs, lens = tr.offs[:n].copy(), tr.lens[:n].copy()
        size = int(offs[-1]) + int(lens[-1])
        wire = tr.wire[:size].copy()
        desc = np.zeros(n, L.DESC)
        route = np.zeros(n, L.ROUTE)
        res = np.zeros(n, L.RESULT)

        def call(offs, lens, in_len, out_len, cid_len=8):
            out = np.full(size + 64, 0x5A, np.uint8)
            rc = lib.qpp_session_route_unprotect(s, kt, m, cid_len, offs.ctypes.data, lens.ctypes.data, n,
                                                 wire.ctypes.data, in_len, tr.conn_slot.ctypes.data,
                                                 tr.conn_exp.ctypes.data, tr.n_conns, 0, out.ctypes.data, out_len,
                                                 desc.ctypes.data, route.ctypes.data, res.ctypes.data)
            return rc, out

        rc, out = call(offs, lens, size, size)
        assert rc == 0 and (out[size:] == 0x5A).all() and not (out[:size] == 0x5A).all()
        assert (res["status"] == L.S_NO_KEY).all()  # no keys installed: routed, nothing decrypted
        assert (route["cls"][:n] == restate(tr.table, 8, offs, lens, wire, tr.conn_slot, tr.conn_exp)[1]["cls"]).all()
        long_last = lens.copy()
        long_last[-1] += 1
        far = offs.copy()
        far[7] = 1 << 40
        wrap = offs.copy()
        wrap[0] = (1 << 64) - 1
        for o, l, il, ol in ((offs, long_last, size, size + 64), (offs, long_last, size + 64, size),
                             (far, lens, size, size), (wrap, lens, size, size), (offs, lens, size - 1, size),
                             (offs, lens, size, size - 1)):
            rc, out = call(o, l, il, ol)
            assert rc == -1
            assert (out == 0x5A).all(), "a refused call wrote to the output"
        for bad in (0, 21):
            rc, out = call(offs, lens, size, size, cid_len=bad)
            assert rc == -1 and (out == 0x5A).all()
    finally:
        lib.qpp_session_destroy(s)
        lib.qpp_cidmap_destroy(m)
        lib.qpp_keytab_destroy(kt)


# ------------------------------------------------------------ receive_routed --

def _record_tuple(p):
    return (p.datagram, p.offset, p.header, p.packet_type, p.epoch, p.plain_header, p.plain_payload,
            p.packet_number, p.dropped)


def _state(conns):
    from aioquic_amd.tls import Epoch

    return [(c.closed, c.spaces[Epoch.ONE_RTT].expected_packet_number, c.spaces[Epoch.HANDSHAKE].expected_packet_number,
             c.spaces[Epoch.INITIAL].expected_packet_number, c.cryptos[Epoch.ONE_RTT].recv.key_phase) for c in conns]


def _routed_vs_demultiplexed(specs, items, extra=()):
    """receive_routed over the raw datagrams against receive_datagrams over
    the items a dict routing pass makes of them, on a second copy of the state."""
    from aioquic_amd import layout as L
    from aioquic_amd import receive as R
    from aioquic_amd.route import CidRouter

    datagrams = [d for _, d in items]
    for pos, d in extra:
        datagrams.insert(pos, d)
    conns_a = [s.product_conn() for s in specs]
    conns_b = [s.product_conn() for s in specs]
    router = CidRouter(8, 64)
    table = {}
    for s, c in zip(specs, conns_a):
        assert router.add(s.cid, c) == s.idx
        table[s.cid] = s.idx
    n = len(datagrams)
    lens = np.asarray([len(d) for d in datagrams], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    _, want_r = restate(table, 8, offs, lens, np.frombuffer(b"".join(datagrams), np.uint8),
                        np.zeros(len(specs), np.uint32), np.zeros(len(specs), np.uint64))
    known = ((want_r["cls"] == L.R_SHORT) | (want_r["cls"] == L.R_LONG)) & (want_r["conn"] != NONE)
    idx = np.flatnonzero(known).tolist()
    want_unrouted = [(i, int(want_r["cls"][i])) for i in range(n) if not known[i]]
    want = R.receive_datagrams([(conns_b[want_r["conn"][i]], datagrams[i]) for i in idx])
    want = [r._replace(datagram=idx[r.datagram]) for r in want]
    got, unrouted = R.receive_routed(router, datagrams)
    assert unrouted == want_unrouted
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert _record_tuple(g) == _record_tuple(w)
    assert _state(conns_a) == _state(conns_b)
    return got, unrouted, want_r


@pytest.mark.parametrize("client", [False, True])
def test_receive_routed_scenario(dev, client):
    """The oracle-built server traffic of tests/receive_scenario.py, long
    headers included: the routed datagrams go through the general walk."""
    from aioquic_amd import layout as L

    specs, items = RS.build(client=client)
    got, unrouted, want_r = _routed_vs_demultiplexed(specs, items)
    kinds = {r.dropped for r in got}
    assert {None, "payload_decrypt_error", "key_unavailable", "reserved_bits", "connection_closed"} <= kinds
    assert {c for _, c in unrouted} >= {L.R_MALFORMED, L.R_LONG}
    assert (want_r["cls"] == L.R_LONG).sum() > len(specs)


def test_receive_routed_all_short(dev, monkeypatch):
    """Every routed datagram a short header: the one-call C path, with a
    key-phase flip, reordered and replayed packet numbers, a reserved-bit
    close, a closed and a keyless connection, and unknown CIDs in between."""
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd import receive as R

    specs, items = RS.build(seed=0x5A, n_conns=7, per_conn=90, client=False)
    items = [(c, d) for c, d in items if not d or not d[0] & 0x80]
    rng = np.random.default_rng(9)
    extra = [(5, bytes([0x41]) + bytes(8) + rng.bytes(40)), (17, b""), (40, bytes([0x42]) + rng.bytes(60)),
             (41, bytes([0xC3]) + b"\x00\x00\x00\x01\x08" + bytes(8) + rng.bytes(30))]
    calls = []
    real = _crypto.receive_routed
    monkeypatch.setattr(_crypto, "receive_routed", lambda *a: calls.append(a[-1]) or real(*a))
    launches = []
    real_short = _crypto.receive_short
    monkeypatch.setattr(_crypto, "receive_short", lambda *a: launches.append(1) or real_short(*a))
    got, unrouted, want_r = _routed_vs_demultiplexed(specs, items, extra)
    assert calls == [1], "the C path with its walk"
    assert launches == [1], "receive_datagrams ran once, for the expected records only"
    assert {None, "payload_decrypt_error", "key_unavailable", "reserved_bits", "connection_closed"} <= \
        {r.dropped for r in got}
    assert {c for _, c in unrouted} == {L.R_MALFORMED, L.R_UNKNOWN_CID, L.R_LONG}
    assert [r.datagram for r in got] == sorted(r.datagram for r in got)
    assert len(got) + len(unrouted) == len(items) + len(extra)


def test_cid_router_bookkeeping(dev):
    from aioquic_amd.route import CidRouter

    from oracle import oracle as O

    rng = np.random.default_rng(3)
    a, b, c = (RS.ConnSpec(rng, k, O.VERSION_1, O.AES_128_GCM).product_conn() for k in range(3))
    r = CidRouter(8, 4)
    assert r.add(b"A" * 8, a) == 0 and r.add(b"B" * 8, b) == 1 and r.add(b"a" * 8, a) == 0
    assert r.conns == [a, b] and len(r) == 3 and r.map.count == 3
    r.retire(b"A" * 8)
    assert r.conns == [a, b] and r.map.find(b"A" * 8) is None and r.map.find(b"a" * 8) == 0
    r.retire(b"a" * 8)
    r.retire(b"never issued")
    assert r.conns == [None, b] and r.map.count == 1
    assert r.add(b"C" * 8, c) == 0 and r.conns == [c, b]  # the index is reused
    assert r.add(b"B" * 8, c) == 0 and r.conns == [c, None]  # a CID moves: b has none left
    c.host_cid_length = 4
    with pytest.raises(ValueError):
        r.add(b"D" * 8, c)
    c.host_cid_length = 8
    r.add(b"D" * 8, c), r.add(b"E" * 8, c)
    with pytest.raises(ValueError):
        r.add(b"F" * 8, c)  # the map is full: nothing changed
    assert len(r) == 4 and r.map.count == 4 and r.map.find(b"F" * 8) is None
    with pytest.raises(ValueError):
        CidRouter(0, 4)
