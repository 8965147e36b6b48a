"""GPU checks of the device header walk (include/quic_pp.h: qpp_route_walk,
qpp_session_route_walk_unprotect) and of receive.receive_routed over batches
with long headers.

The reference is a restatement written here on oracle.receive_walk.parse_header
(tests/walk_cases.restate_walk, `restate_device` below), the C oracle's
unprotect over the restated descriptors, oracle.receive_walk.receive for the
records, and receive_datagrams on the demultiplexed items."""

from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import receive_walk as W
from tests import receive_scenario as RS
from tests import walk_cases as C
from tests.test_gpu_route import _record_tuple, _routed_vs_demultiplexed, entries, restate

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_CONN, BAD_CONN = 6, 100
POISON = 48


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


# --------------------------------------------------------------- the batch --

class World:
    """About 600 datagrams at odd offsets, each followed by poison bytes that
    would complete a truncated header if they were read: the oracle-built
    traffic of six connections (coalesced Initial + Handshake + 0-RTT + 1-RTT,
    lone Handshake and 0-RTT, 1-RTT; the last connection has no 1-RTT keys and
    no connection has the other version's Initial keys) and the hand-built
    headers of tests/walk_cases.py addressed to a known connection, to an
    unknown CID and to a CID whose connection index is out of range."""

    def __init__(self):
        from aioquic_amd import layout as L

        rng = np.random.default_rng(0x3A1C)
        self.specs, items = RS.build(seed=0x11, n_conns=N_CONN, per_conn=14, checks=False, client=False)
        self.table = {s.cid: s.idx for s in self.specs}
        self.unknown, self.bad = b"\x0F" * 8, b"\xBA" * 8
        self.table[self.bad] = BAD_CONN
        # keys: a slot per key-set that has keys
        recs = []
        self.kslot = np.full((N_CONN, L.KEYSETS), L.SLOT_NONE, np.uint32)
        for s in self.specs:
            ctxs = {0 if s.version == O.VERSION_1 else 1: W.Ctx(O.AES_128_GCM, s.initial_secret, s.version),
                    2: W.Ctx(s.suite, s.zrtt_secret, s.version), 3: W.Ctx(O.AES_128_GCM, s.hs_secret, s.version)}
            if s.has_one_rtt:
                ctxs[4] = W.Ctx(s.suite, s.one_secret, s.version)
            for ks, ctx in sorted(ctxs.items()):
                self.kslot[s.idx, ks] = len(recs)
                recs.append(L.key_material(len(recs), ctx.suite, ctx.key, ctx.iv, ctx.hp, ctx.key_phase))
        self.keys = np.concatenate(recs)
        self.kexp = rng.integers(0, 3, (N_CONN, L.SPACES)).astype(np.uint64)
        dgs = [(d, b"") for _, d in items]
        known, unknown, bad = (C.hand_cases(c) for c in (self.specs[0].cid, self.unknown, self.bad))
        co = known[0][1]
        for k, (name, d) in enumerate(known):
            tail = co[len(d):len(d) + POISON] if name.startswith("coalesced-cut-") else b""
            dgs.append((d, tail))
            if k % 3 == 0:
                dgs.append((unknown[k][1], tail))
            if k % 3 == 1:
                dgs.append((bad[k][1], tail))
        order = rng.permutation(len(dgs))
        self.datagrams = [dgs[k][0] for k in order]
        offs, pos, parts = [], 1, [b"\x11"]
        default = bytes(range(0x10, 0x10 + POISON))  # one-byte varints, CID bytes, a short header's start
        for k in order:
            d, tail = dgs[k]
            offs.append(pos)
            fill = d + (tail + default)[:POISON]
            fill += b"\x40" * (1 - (pos + len(fill)) % 2)  # the next odd offset
            parts.append(fill)
            pos += len(fill)
        self.buf = np.frombuffer(b"".join(parts), np.uint8).copy()
        self.offs = np.asarray(offs, np.uint64)
        self.lens = np.asarray([len(d) for d in self.datagrams], np.uint32)
        self.n = len(self.datagrams)
        assert (self.offs % 2 == 1).all() and 550 <= self.n <= 700
        self.conn_slot = np.ascontiguousarray(self.kslot[:, 4])
        self.conn_exp = np.ascontiguousarray(self.kexp[:, 2])
        self.desc0, self.route = restate(self.table, 8, self.offs, self.lens, self.buf, self.conn_slot, self.conn_exp)
        # what may be listed: every long first byte, and now and then another datagram
        self.candidates = [i for i, d in enumerate(self.datagrams) if (d and d[0] & 0x80) or i % 9 == 0]
        # always listed (while they fit): the oracle's coalesced datagrams and one short header
        rs = {d for _, d in items}
        self.must = [i for i, d in enumerate(self.datagrams) if d in rs and len(d) == 1200 and d[0] & 0x80]
        self.must.append(next(i for i, d in enumerate(self.datagrams) if d in rs and not d[0] & 0x80))

    def listing(self, n_long):
        must = self.must[:n_long]
        rest = [c for c in self.candidates if c not in must]
        pick = np.unique(np.linspace(0, len(rest) - 1, n_long - len(must)).round().astype(int)) \
            if n_long > len(must) else []
        out = sorted(must + [rest[k] for k in pick])
        assert len(out) == n_long
        return np.asarray(out, np.uint32)


@pytest.fixture(scope="module")
def world():
    return World()


def restate_device(w, long_idx, flags=0):
    """(DESC[n + 3 n_long], walk records per listed datagram) of qpp_route_walk."""
    from aioquic_amd import layout as L

    n, nl = w.n, len(long_idx)
    desc = np.zeros(n + 3 * nl, L.DESC)
    desc[:n] = w.desc0
    desc["flags"] = flags
    raw = w.buf.tobytes()
    walks = []
    for r, i in enumerate(long_idx.tolist()):
        o, ln = int(w.offs[i]), int(w.lens[i])
        data = raw[o:o + ln]
        extra = desc[n + 3 * r:n + 3 * r + 3]
        extra["in_off"] = extra["out_off"] = o
        extra["slot"] = L.SLOT_NONE
        cls, conn = int(w.route["cls"][i]), int(w.route["conn"][i])
        is_long = cls == L.R_LONG or (cls == L.R_BAD_CONN and ln > 0 and data[0] & 0x80)
        recs = C.restate_walk(data, 8) if is_long else []
        keyed = cls == L.R_LONG and conn != NONE
        for k, rec in enumerate(recs):
            rec["desc"] = NONE
            if keyed and rec["status"] == C.W_OK and rec["type"] in (0, 1, 2, 5):
                at = i if k == 0 else n + 3 * r + k - 1
                ks = {0: {C.V1: 0, C.V2: 1}.get(rec["version"]), 1: 2, 2: 3, 5: 4}[rec["type"]]
                space = {0: 0, 2: 1, 1: 2, 5: 2}[rec["type"]]
                d = desc[at:at + 1]
                d["in_off"] = d["out_off"] = o + rec["off"]
                d["len"] = rec["len"]
                d["hdr_len"] = rec["pn_off"]
                d["pn"] = w.kexp[conn, space]
                d["slot"] = L.SLOT_NONE if ks is None else w.kslot[conn, ks]
                rec["desc"] = at
        walks.append(recs)
    return desc, walks


@pytest.mark.parametrize("n_long", [1, 63, 64, 65, 255, 256, 257])
def test_route_walk_matches_restatement(dev, world, n_long):
    import torch
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    w = world
    eng = PacketEngine(len(w.keys))
    eng.set_key_records(w.keys)
    m = eng.cid_map(16)
    m.put(entries(w.table.items()))
    long_idx = w.listing(n_long)
    n, nd = w.n, w.n + 3 * n_long
    flags = L.F_RFC_PN
    want_d, want_w = restate_device(w, long_idx, flags)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    canary = lambda size: torch.full((size + 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_in, d_off, d_len = t(w.buf), t(w.offs), t(w.lens)
    d_desc, d_route = canary(nd * 40), canary(n * 8)
    d_walk, d_walk_n, d_res = canary(n_long * 4 * 24), canary(n_long * 4), canary(nd * 16)
    d_out = torch.zeros(len(w.buf), dtype=torch.uint8, device=dev)
    eng.route(m, 8, d_off, d_len, n, d_in, t(w.conn_slot), t(w.conn_exp), N_CONN, d_route, desc=d_desc, flags=flags)
    eng.route_walk(8, d_off, d_len, n, d_in, d_route, t(long_idx), n_long, t(w.kslot), t(w.kexp), N_CONN, d_desc,
                   d_walk, d_walk_n, flags=flags)
    eng.unprotect(d_desc, nd, d_in, d_out, d_res)
    torch.cuda.synchronize()
    desc, route = d_desc.cpu().numpy(), d_route.cpu().numpy()
    walk, walk_n, res = d_walk.cpu().numpy(), d_walk_n.cpu().numpy(), d_res.cpu().numpy()
    for a, size in ((desc, nd * 40), (route, n * 8), (walk, n_long * 96), (walk_n, n_long * 4), (res, nd * 16)):
        assert (a[size:] == 0xAB).all(), "wrote past the end"
    assert route[:n * 8].tobytes() == w.route.tobytes(), "d_route is only read"
    got_n = walk_n[:n_long * 4].view(np.uint32)
    assert got_n.tolist() == [len(r) for r in want_w]
    got_w = walk[:n_long * 96].view(L.WALK).reshape(n_long, 4)
    for r, recs in enumerate(want_w):
        for k, rec in enumerate(recs):
            g = got_w[r, k]
            assert {f: int(g[f]) for f in C.FIELDS + ("desc",)} == rec, (r, k, int(long_idx[r]))
        assert not got_w[r, len(recs):].tobytes().strip(b"\0"), "records past the count are zeros"
    got_d = desc[:nd * 40].view(L.DESC)
    for f in L.DESC.names:
        assert got_d[f].tolist() == want_d[f].tolist(), f
    # the unprotect over all n + 3 n_long descriptors against the C oracle
    want_out, want_res = O.unprotect_batch(w.keys, want_d, w.buf, len(w.buf))
    got_res = res[:nd * 16].view(L.RESULT)
    ok = want_res["status"] == L.S_OK
    assert ((got_res["status"] == L.S_OK) == ok).all()
    assert (got_res["status"][want_d["slot"] == L.SLOT_NONE] == L.S_NO_KEY).all()
    for f in ("pn", "hdr_len", "out_len"):
        assert (got_res[f][ok] == want_res[f][ok]).all(), f
    out = d_out.cpu().numpy()
    written = np.zeros(len(w.buf), bool)
    for k in np.flatnonzero(ok).tolist():
        o, ln = int(want_d["out_off"][k]), int(want_res["out_len"][k])
        assert out[o:o + ln].tobytes() == want_out[o:o + ln].tobytes(), k
        written[o:o + ln] = True
    for k in np.flatnonzero(want_d["len"] > 0).tolist():
        written[int(want_d["out_off"][k]):int(want_d["out_off"][k]) + int(want_d["len"][k])] = True
    assert not out[~written].any(), "bytes outside every packet were written"
    if n_long >= 63:
        types = {(rec["type"], rec["status"]) for recs in want_w for rec in recs}
        assert {(t_, C.W_OK) for t_ in ((0, 1, 2, 5) if n_long < 255 else range(6))} <= types
        assert (5, C.W_PARSE) in types
        assert ok[n:].any() and ok[:n].any(), "packets at both placements unprotected"
        listed = w.route[long_idx]
        assert {L.R_LONG, L.R_BAD_CONN} <= set(listed["cls"].tolist())
        assert (listed["conn"] == NONE).any() and (got_n == 0).any()


def test_route_walk_rejects_bad_arguments(dev):
    import torch
    from aioquic_amd.batch import PacketEngine

    eng = PacketEngine(1)
    z = torch.zeros(256, dtype=torch.uint8, device=dev)
    for bad in (0, 21):
        with pytest.raises(ValueError):
            eng.route_walk(bad, z, z, 1, z, z, z, 1, z, z, 1, z, z, z)
    with pytest.raises(ValueError):
        eng.route_walk(8, z, z, 1, z, z, z, 2, z, z, 1, z, z, z)  # more listed than there are


def test_route_walk_skips_an_index_past_the_batch(dev, world):
    """The device form with a listed index >= n: that lane finds no packets,
    writes zeroed records and inert extra descriptors, and the unprotect over
    all n + 3 n_long descriptors reports QPP_S_NO_KEY for them."""
    import torch
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    w = world
    eng = PacketEngine(len(w.keys))
    eng.set_key_records(w.keys)
    m = eng.cid_map(16)
    m.put(entries(w.table.items()))
    n = 40
    good = [i for i in range(n) if w.lens[i] and w.buf[int(w.offs[i])] & 0x80][:3]
    long_idx = np.asarray(good[:2] + [n + 5] + good[2:], np.uint32)
    nl, nd = len(long_idx), n + 3 * len(long_idx)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    fill = lambda size: torch.full((size,), 0xAB, dtype=torch.uint8, device=dev)
    d_in, d_off, d_len = t(w.buf), t(w.offs[:n]), t(w.lens[:n])
    d_desc, d_route, d_walk, d_walk_n, d_res = fill(nd * 40), fill(n * 8), fill(nl * 96), fill(nl * 4), fill(nd * 16)
    d_out = torch.zeros(len(w.buf), dtype=torch.uint8, device=dev)
    eng.route(m, 8, d_off, d_len, n, d_in, t(w.conn_slot), t(w.conn_exp), N_CONN, d_route, desc=d_desc)
    eng.route_walk(8, d_off, d_len, n, d_in, d_route, t(long_idx), nl, t(w.kslot), t(w.kexp), N_CONN, d_desc,
                   d_walk, d_walk_n)
    eng.unprotect(d_desc, nd, d_in, d_out, d_res)
    torch.cuda.synchronize()
    desc = d_desc.cpu().numpy().view(L.DESC)
    walk = d_walk.cpu().numpy().view(L.WALK).reshape(nl, 4)
    walk_n = d_walk_n.cpu().numpy().view(np.uint32)
    res = d_res.cpu().numpy().view(L.RESULT)
    assert walk_n[2] == 0 and not walk[2].tobytes().strip(b"\0")
    extra = desc[n + 6:n + 9]
    assert (extra["slot"] == L.SLOT_NONE).all() and (extra["len"] == 0).all() and (extra["in_off"] == 0).all()
    assert (res["status"][n + 6:n + 9] == L.S_NO_KEY).all()
    for r in (0, 1, 3):  # the lanes beside it did their work
        i = int(long_idx[r])
        want = C.restate_walk(w.buf[int(w.offs[i]):int(w.offs[i]) + int(w.lens[i])].tobytes(), 8) \
            if w.route["cls"][i] in (L.R_LONG, L.R_BAD_CONN) else []
        assert walk_n[r] == len(want)


# ------------------------------------------------------------ session form --

def test_session_form_matches_device_path(dev, world):
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    w = world
    eng = PacketEngine(len(w.keys))
    eng.set_key_records(w.keys)
    m = eng.cid_map(16)
    m.put(entries(w.table.items()))
    long_idx = w.listing(65)
    want_d, want_w = restate_device(w, long_idx)
    before = _crypto.route_walk_launches()
    out, desc, route, res, walk, walk_n = eng.route_walk_unprotect_host(m, 8, w.offs, w.lens, w.buf, long_idx, w.kslot,
                                                                        w.kexp, len(w.buf))
    assert _crypto.route_walk_launches() == before + 1
    assert route.tobytes() == w.route.tobytes() and desc.tobytes() == want_d.tobytes()
    assert walk_n.tolist() == [len(r) for r in want_w]
    for r, recs in enumerate(want_w):
        for k, rec in enumerate(recs):
            assert {f: int(walk[r, k][f]) for f in C.FIELDS + ("desc",)} == rec
        assert not walk[r, len(recs):].tobytes().strip(b"\0"), "records past the count are zeros"
    want_out, want_res = O.unprotect_batch(w.keys, want_d, w.buf, len(w.buf))
    ok = want_res["status"] == L.S_OK
    assert ((res["status"] == L.S_OK) == ok).all() and ok[w.n:].any()
    for k in np.flatnonzero(ok).tolist():
        o, ln = int(want_d["out_off"][k]), int(want_res["out_len"][k])
        assert out[o:o + ln].tobytes() == want_out[o:o + ln].tobytes()
    # n_long == 0: qpp_session_route_unprotect, byte for byte, and no walk launch
    before = _crypto.route_walk_launches()
    a = eng.route_unprotect_host(m, 8, w.offs, w.lens, w.buf, w.conn_slot, w.conn_exp, len(w.buf))
    b = eng.route_walk_unprotect_host(m, 8, w.offs, w.lens, w.buf, [], w.kslot, w.kexp, len(w.buf))
    assert _crypto.route_walk_launches() == before
    for x, y in zip(a, b[:4]):
        assert x.tobytes() == y.tobytes()
    assert len(b[4]) == 0 and len(b[5]) == 0
    assert a[1].tobytes() == w.desc0.tobytes()


def test_session_form_refuses_bad_listings(dev, world):
    """long_idx not strictly increasing, or an index >= n: QPP_E_ARG with
    nothing touched (the C ABI itself, through ctypes)."""
    import aioquic_amd  # noqa: F401  (binds torch's HIP runtime first)
    from aioquic_amd import layout as L

    lib = ctypes.CDLL(os.path.join(ROOT, "aioquic_amd", "libquicpp.so"))
    vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    lib.qpp_session_route_walk_unprotect.restype = ctypes.c_int
    lib.qpp_session_route_walk_unprotect.argtypes = [vp, vp, vp, u32, vp, vp, u32, vp, sz, vp, u32, vp, vp, u32,
                                                     ctypes.c_uint16, vp, sz, vp, vp, vp, vp, vp]
    lib.qpp_route_walk_launches.restype = ctypes.c_uint64
    lib.qpp_cidmap_put.argtypes = [vp, vp, u32, vp]
    for f in (lib.qpp_keytab_destroy, lib.qpp_cidmap_destroy, lib.qpp_session_destroy):
        f.argtypes = [vp]
        f.restype = None
    kt, m, s = vp(), vp(), vp()
    assert lib.qpp_keytab_create(u32(8), ctypes.byref(kt)) == 0
    assert lib.qpp_cidmap_create(u32(16), ctypes.byref(m)) == 0
    assert lib.qpp_session_create(sz(4096), u32(64), ctypes.byref(s)) == 0
    try:
        w = world
        ent = np.frombuffer(entries(w.table.items()), np.uint8).copy()
        assert lib.qpp_cidmap_put(m, ent.ctypes.data, len(w.table), None) == 0
        n = 40
        offs, lens = w.offs[:n].copy(), w.lens[:n].copy()
        size = int(offs[-1]) + int(lens[-1])
        wire = w.buf[:size].copy()
        kslot = np.full((N_CONN, L.KEYSETS), L.SLOT_NONE, np.uint32)

        def call(idx, walk_args=True):
            idx = np.asarray(idx, np.uint32)
            nl = len(idx)
            out = np.full(size + 64, 0x5A, np.uint8)
            desc = np.full((n + 3 * nl) * 40, 0x5A, np.uint8)
            route = np.full(n * 8, 0x5A, np.uint8)
            res = np.full((n + 3 * nl) * 16, 0x5A, np.uint8)
            walk = np.full(max(nl, 1) * 96, 0x5A, np.uint8)
            walk_n = np.full(max(nl, 1) * 4, 0x5A, np.uint8)
            rc = lib.qpp_session_route_walk_unprotect(
                s, kt, m, 8, offs.ctypes.data, lens.ctypes.data, n, wire.ctypes.data, size,
                idx.ctypes.data if nl else None, nl, kslot.ctypes.data, w.kexp.ctypes.data, N_CONN, 0,
                out.ctypes.data, size, desc.ctypes.data, route.ctypes.data, res.ctypes.data,
                walk.ctypes.data if walk_args else None, walk_n.ctypes.data if walk_args else None)
            return rc, (out, desc, route, res, walk, walk_n)

        before = lib.qpp_route_walk_launches()
        for idx in ([3, 3], [5, 4], [0, 1, 2, 2], [n], [0, n], [1, 2, NONE], list(range(n)) + [n - 1]):
            rc, outs = call(idx)
            assert rc == -1, idx
            assert all((a == 0x5A).all() for a in outs), "a refused call wrote to its output"
        rc, outs = call([1, 2], walk_args=False)
        assert rc == -1 and all((a == 0x5A).all() for a in outs)
        assert lib.qpp_route_walk_launches() == before, "a refused call launched"
        long_idx = [i for i in range(n) if lens[i] and wire[int(offs[i])] & 0x80]
        rc, (out, desc, route, res, walk, walk_n) = call(long_idx)
        assert rc == 0 and lib.qpp_route_walk_launches() == before + 1
        assert (out[size:] == 0x5A).all() and route.tobytes() == w.route[:n].tobytes()
        assert (res.view(L.RESULT)["status"] == L.S_NO_KEY).all()  # no keys installed: walked, nothing decrypted
        want = [C.restate_walk(wire[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes(), 8)
                if w.route["cls"][i] in (L.R_LONG, L.R_BAD_CONN) else [] for i in long_idx]
        assert walk_n.view(np.uint32).tolist() == [len(r) for r in want]
    finally:
        lib.qpp_session_destroy(s)
        lib.qpp_cidmap_destroy(m)
        lib.qpp_keytab_destroy(kt)


# ---------------------------------------------------------- receive_routed --

def _oracle_tuple(o):
    return (o.datagram, o.offset, o.packet_type, o.dropped, o.plain_header, o.plain_payload, o.packet_number)


def _product_tuple(p):
    return (p.datagram, p.offset, p.packet_type.name, p.dropped, p.plain_header, p.plain_payload, p.packet_number)


def test_receive_routed_walks_long_headers_on_the_device(dev, monkeypatch):
    """The server traffic of tests/receive_scenario.py through receive_routed:
    one fused launch walks the long headers, and the records are the oracle
    walk's and receive_datagrams' on the demultiplexed items."""
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd import receive as R
    from aioquic_amd.route import CidRouter
    from aioquic_amd.tls import Epoch

    specs, items = RS.build(client=False)
    before = _crypto.route_walk_launches()
    got, unrouted, want_r = _routed_vs_demultiplexed(specs, items)
    assert _crypto.route_walk_launches() == before + 1
    kinds = {r.dropped for r in got}
    assert {None, "payload_decrypt_error", "key_unavailable", "unsupported_version",
            "initial_packet_datagram_too_small", "reserved_bits", "connection_closed"} <= kinds
    assert {r.packet_type.name for r in got if r.ok} >= {"INITIAL", "HANDSHAKE", "ZERO_RTT", "ONE_RTT",
                                                         "VERSION_NEGOTIATION"}
    assert max(r.offset for r in got if r.ok) > 600, "coalesced packets"
    # against the oracle's walk of the routed datagrams
    known = ((want_r["cls"] == L.R_SHORT) | (want_r["cls"] == L.R_LONG)) & (want_r["conn"] != NONE)
    idx = np.flatnonzero(known).tolist()
    oconns = [s.oracle_conn() for s in specs]
    datagrams = [d for _, d in items]
    want = W.receive([(oconns[want_r["conn"][i]], datagrams[i]) for i in idx])
    assert len(got) == len(want)
    for g, o in zip(got, want):
        o.datagram = idx[o.datagram]
        assert _product_tuple(g) == _oracle_tuple(o)
    # again, with the general path taken away: the call does not need it
    conns = [s.product_conn() for s in specs]
    router = CidRouter(8, 64)
    for s, c in zip(specs, conns):
        router.add(s.cid, c)

    def refuse(*a, **k):
        raise AssertionError("receive_routed fell back to receive_datagrams")

    monkeypatch.setattr(R, "receive_datagrams", refuse)
    before = _crypto.route_walk_launches()
    again, unrouted2 = R.receive_routed(router, datagrams)
    assert _crypto.route_walk_launches() == before + 1
    assert unrouted2 == unrouted
    assert [_record_tuple(r) for r in again] == [_record_tuple(r) for r in got]
    for oc, pc in zip(oconns, conns):
        assert oc.expected["ONE_RTT"] == pc.spaces[Epoch.ONE_RTT].expected_packet_number
        assert oc.expected["HANDSHAKE"] == pc.spaces[Epoch.HANDSHAKE].expected_packet_number
        assert oc.expected["INITIAL"] == pc.spaces[Epoch.INITIAL].expected_packet_number
        assert oc.closed == pc.closed
        if oc.pairs["ONE_RTT"].recv is not None:
            assert oc.pairs["ONE_RTT"].recv.key_phase == pc.cryptos[Epoch.ONE_RTT].recv.key_phase


def test_all_short_batch_launches_no_walk(dev):
    from aioquic_amd import _crypto

    specs, items = RS.build(seed=0x5A, n_conns=5, per_conn=30, client=False)
    items = [(c, d) for c, d in items if d and not d[0] & 0x80]
    before = _crypto.route_walk_launches()
    got, unrouted, _ = _routed_vs_demultiplexed(specs, items)
    assert _crypto.route_walk_launches() == before
    assert len(got) > 100


def test_five_packet_datagram_takes_the_fallback(dev):
    """A datagram of five coalesced packets is the host walk's (QPP_W_HOST):
    the whole batch goes the general way, with the same records."""
    from aioquic_amd import _crypto

    specs, items = RS.build(seed=0x77, n_conns=4, per_conn=16, client=False)
    s = specs[0]
    hs = W.Ctx(O.AES_128_GCM, s.hs_secret, s.version)
    parts = []
    for pn in range(40, 45):
        pl = bytes([pn]) * 30
        parts.append(O.protect(hs.suite, hs.key, hs.iv, hs.hp,
                               RS.long_header(s.version, "HANDSHAKE", s.cid, s.scid, b"", pn, 1, len(pl) + 16), pl, pn))
    before = _crypto.route_walk_launches()
    got, unrouted, want_r = _routed_vs_demultiplexed(specs, items, extra=[(len(items) // 2, b"".join(parts))])
    assert _crypto.route_walk_launches() == before + 1, "the fused call ran, then the fallback"
    five = [r for r in got if r.datagram == len(items) // 2]
    assert [r.offset for r in five] == [k * len(parts[0]) for k in range(5)]
    assert all(r.ok and r.packet_number == 40 + k for k, r in enumerate(five))


def test_hand_built_headers_to_a_routed_connection(dev, monkeypatch):
    """The hand-built headers of tests/walk_cases.py that the device walks to
    the end (a Version Negotiation packet with a version list that is no
    multiple of four bytes, which the host parser refuses, among them), sent
    to a known connection between the scenario's datagrams: the records are
    receive_datagrams' on the demultiplexed items, without the fallback."""
    from aioquic_amd import _crypto
    from aioquic_amd import receive as R

    specs, items = RS.build(seed=0x31, n_conns=4, per_conn=16, client=False)
    cases = [(name, d) for name, d in C.hand_cases(specs[0].cid)
             if d and all(r["status"] != C.W_HOST for r in C.restate_walk(d, 8))]
    names = {name for name, _ in cases}
    assert {"vn-odd-tail", "vn-no-fixed", "vn-second", "retry-15", "retry-16", "retry-second", "coalesced-1200",
            "short-no-fixed", "length-max", "pn-off-1500"} <= names
    step = max(len(items) // len(cases), 1)
    extra = [(min(k * (step + 1), len(items) + k), d) for k, (_, d) in enumerate(cases)]
    calls = []
    real = R.receive_datagrams
    monkeypatch.setattr(R, "receive_datagrams", lambda *a, **k: calls.append(1) or real(*a, **k))
    before = _crypto.route_walk_launches()
    got, unrouted, want_r = _routed_vs_demultiplexed(specs, items, extra)
    assert calls == [1], "receive_datagrams ran once, for the expected records only"
    assert _crypto.route_walk_launches() == before + 1
    by_dg = {}
    for r in got:
        by_dg.setdefault(r.datagram, []).append(r)
    datagrams = [d for _, d in items]
    for pos, d in extra:
        datagrams.insert(pos, d)
    odd = datagrams.index(dict(cases)["vn-odd-tail"])
    assert [(r.offset, r.dropped) for r in by_dg[odd]] == [(0, "header_parse_error")]
    vn = datagrams.index(dict(cases)["vn-no-fixed"])
    assert [(r.packet_type.name, r.dropped) for r in by_dg[vn]] == [("VERSION_NEGOTIATION", None)]
    r16 = datagrams.index(dict(cases)["retry-16"])
    assert [(r.packet_type.name, r.dropped) for r in by_dg[r16]] == [("RETRY", None)]
    r15 = datagrams.index(dict(cases)["retry-15"])
    assert [r.dropped for r in by_dg[r15]] == ["header_parse_error"]


def test_key_slots_only_for_the_connections_long_headers_reach(dev, monkeypatch):
    """A router that holds many more keyed key-sets than the key table has
    slots: a batch with long headers needs slots for the 1-RTT keys and for
    the key-sets of the connections its long headers reach, no more."""
    from aioquic_amd import _crypto
    from aioquic_amd import batch_io
    from aioquic_amd import receive as R
    from aioquic_amd.route import CidRouter

    specs, items = RS.build(seed=0x41, n_conns=4, per_conn=16, client=False)
    rng = np.random.default_rng(0x42)
    idle = [RS.ConnSpec(rng, 50 + k, O.VERSION_1, O.AES_128_GCM) for k in range(30)]  # four keyed key-sets each
    small = batch_io.KeySlots(64)  # 16 key-sets of the batch's connections + 30 idle 1-RTT keys fit; 136 do not
    monkeypatch.setattr(R, "default_slots", lambda: small)
    monkeypatch.setattr(batch_io, "default_slots", lambda: small)
    datagrams = [d for _, d in items]
    want = R.receive_datagrams([(c, d) for c, d in _demultiplexed(specs, datagrams)])
    conns = [s.product_conn() for s in specs]
    router = CidRouter(8, 64)
    for s, c in zip(specs, conns):
        router.add(s.cid, c)
    for s in idle:
        router.add(s.cid, s.product_conn())

    def refuse(*a, **k):
        raise AssertionError("receive_routed fell back to receive_datagrams")

    monkeypatch.setattr(R, "receive_datagrams", refuse)
    before = _crypto.route_walk_launches()
    got, unrouted = R.receive_routed(router, datagrams)
    assert _crypto.route_walk_launches() == before + 1
    assert len(got) == len(want)
    for g, x in zip(got, want):
        assert _record_tuple(g)[1:] == _record_tuple(x)[1:]
    small.close()


def _demultiplexed(specs, datagrams):
    """[(connection, datagram)] of the datagrams that route, on fresh connection state."""
    from aioquic_amd import layout as L

    conns = [s.product_conn() for s in specs]
    table = {s.cid: s.idx for s in specs}
    lens = np.asarray([len(d) for d in datagrams], np.uint32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    _, r = restate(table, 8, offs, lens, np.frombuffer(b"".join(datagrams), np.uint8),
                   np.zeros(len(specs), np.uint32), np.zeros(len(specs), np.uint64))
    known = ((r["cls"] == L.R_SHORT) | (r["cls"] == L.R_LONG)) & (r["conn"] != NONE)
    return [(conns[r["conn"][i]], datagrams[i]) for i in np.flatnonzero(known).tolist()]
