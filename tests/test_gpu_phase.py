"""GPU checks of the key-phase resolution (include/quic_pp.h: qpp_route_phase,
qpp_session_route_phase_unprotect) and of receive.receive_routed(...,
next_phase=True), which resolves a peer's key update inside the one fused
call.

The reference is the restatement of tests/phase_cases.py on the C oracle's
header-protection mask, the C oracle's unprotect over the restated
descriptors, oracle.receive_walk.receive for the records, and
receive_datagrams on the demultiplexed items."""

from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from oracle import oracle as O
from oracle import receive_walk as W
from tests import phase_cases as P
from tests import receive_scenario as RS
from tests.test_gpu_route import _record_tuple, _state, entries, restate

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


# ---------------------------------------------------------- qpp_route_phase --

def _check_unprotect(w, want_d, out, res):
    """The unprotect over the resolved descriptors against the C oracle."""
    from aioquic_amd import layout as L

    want_out, want_res = O.unprotect_batch(w.keys, want_d, w.buf, len(w.buf))
    assert res["status"].tolist() == want_res["status"].tolist()
    ok = want_res["status"] == L.S_OK
    for f in ("pn", "hdr_len", "out_len"):
        assert (res[f][ok] == want_res[f][ok]).all(), f
    inside = np.zeros(len(w.buf), bool)
    for k in range(len(want_d)):
        inside[int(want_d["out_off"][k]):int(want_d["out_off"][k]) + int(want_d["len"][k])] = True
    for k in np.flatnonzero(ok).tolist():
        o, ln = int(want_d["out_off"][k]), int(want_res["out_len"][k])
        assert out[o:o + ln].tobytes() == want_out[o:o + ln].tobytes(), k
    for k in np.flatnonzero(want_res["status"] == L.S_DECRYPT).tolist():
        o, ln = int(want_d["out_off"][k]), int(want_d["len"][k])
        assert not out[o + 9 + 4:o + ln].any(), "a failed packet's payload is zeroed"
    assert not out[~inside].any(), "bytes outside every packet were written"
    return want_res


@pytest.mark.parametrize("routed", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_route_phase_matches_restatement(dev, n, routed):
    """One launch mixing the three suites and every condition of
    tests/phase_cases.World, over poisoned outputs: d_desc and d_phase byte for
    byte, then qpp_unprotect over the result against the oracle."""
    import torch
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    w = P.World(n)
    eng = PacketEngine(P.CAP)
    eng.set_key_records(w.keys)
    route = w.route if routed else None
    nxt = w.conn_next if routed else w.next_per_desc
    n_next = P.N_CONN if routed else 0
    want_d, want_p = P.restate(w.desc, route, nxt, n_next, w.table, P.CAP, w.buf)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    canary = lambda size: torch.full((size + 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_in, d_next = t(w.buf), t(nxt)
    d_route = t(w.route) if routed else None
    d_desc = torch.cat([t(w.desc), canary(0)])
    d_phase, d_res = canary(n), canary(n * 16)
    d_out = torch.zeros(len(w.buf), dtype=torch.uint8, device=dev)
    eng.route_phase(d_route, d_next, n_next, d_desc, n, d_in, d_phase)
    eng.unprotect(d_desc, n, d_in, d_out, d_res)
    torch.cuda.synchronize()
    desc, phase, res = d_desc.cpu().numpy(), d_phase.cpu().numpy(), d_res.cpu().numpy()
    for a, size in ((desc, n * 40), (phase, n), (res, n * 16)):
        assert (a[size:] == 0xAB).all(), "wrote past the end"
    assert phase[:n].tobytes() == want_p.tobytes()
    assert desc[:n * 40].tobytes() == want_d.tobytes(), "only the slot of a re-pointed descriptor changes"
    if routed:
        assert d_route.cpu().numpy().tobytes() == w.route.tobytes(), "d_route is only read"
    assert d_next.cpu().numpy().tobytes() == nxt.tobytes() and d_in.cpu().numpy().tobytes() == w.buf.tobytes()
    want_res = _check_unprotect(w, want_d, d_out.cpu().numpy(), res[:n * 16].view(L.RESULT))
    if n == 1:
        assert want_p.tolist() == [1] and want_res["status"].tolist() == [L.S_OK]
    else:
        st = want_res["status"]
        kinds = np.asarray([k for k, _ in w.kind])
        assert (st[(want_p == 1) & (kinds == "flip")] == L.S_OK).all() and ((want_p == 1) & (kinds == "flip")).any()
        assert (st[(want_p == 1) & (kinds == "tamper")] == L.S_DECRYPT).all()
        assert ((want_p == 1) & (kinds == "tamper")).any()
        assert (st[(want_p == 0) & (kinds == "flip")] != L.S_OK).all(), "a flip left alone fails as ever"
        assert {L.S_KEY_PHASE, L.S_NO_KEY, L.S_LENGTH} <= set(st[want_p == 0].tolist())
        flipped = {c for (k, c), p in zip(w.kind, want_p) if p}
        assert {c % 3 for c in flipped} == {0, 1, 2} and {w.table[2 * c][1] for c in flipped} == {0, 1}
        pn_len = (want_res["hdr_len"] - 9)[(want_p == 1) & (st == L.S_OK)]
        assert set(pn_len.tolist()) == {1, 2, 3, 4}


def test_route_phase_arguments(dev):
    import torch
    from aioquic_amd.batch import PacketEngine

    eng = PacketEngine(4)
    z = torch.zeros(256, dtype=torch.uint8, device=dev)

    class Null:
        @staticmethod
        def data_ptr():
            return 0

    for bad in ((None, Null, z, z, z), (None, z, Null, z, z), (None, z, z, Null, z), (None, z, z, z, Null)):
        r, nx, d, i, p = bad
        with pytest.raises(ValueError):
            eng.route_phase(r, nx, 1, d, 1, i, p)
    eng.route_phase(None, Null, 0, Null, 0, Null, Null)  # n == 0: nothing to do


# ------------------------------------------------------------ session form --

def _session_world():
    from aioquic_amd import layout as L

    w = P.World(300, seed=0x51)
    table = {w.cids[c]: c for c in range(P.N_CONN)}
    offs = w.desc["in_off"].astype(np.uint64)
    lens = w.desc["len"].astype(np.uint32)
    kslot = np.full((P.N_CONN, L.KEYSETS), L.SLOT_NONE, np.uint32)
    kslot[:, 4] = w.conn_slot
    kexp = np.zeros((P.N_CONN, L.SPACES), np.uint64)
    kexp[:, 2] = w.conn_exp
    nxt = w.conn_next.copy()
    nxt[9] = NONE  # a slot past the table is refused by the session form: its own test below
    desc0, route = restate(table, 8, offs, lens, w.buf, w.conn_slot, w.conn_exp)
    return w, table, offs, lens, kslot, kexp, nxt, desc0, route


def test_session_form_matches_device_path(dev):
    import torch
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    w, table, offs, lens, kslot, kexp, nxt, desc0, route = _session_world()
    n = w.n
    eng = PacketEngine(P.CAP)
    eng.set_key_records(w.keys)
    m = eng.cid_map(32)
    m.put(entries(table.items()))
    want_d, want_p = P.restate(desc0, route, nxt, P.N_CONN, w.table, P.CAP, w.buf)
    assert want_p.any() and (route["cls"] == L.R_SHORT).all()
    # the device path
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    z = lambda size: torch.zeros(size, dtype=torch.uint8, device=dev)
    d_in, d_desc, d_route, d_phase, d_res, d_out = t(w.buf), z(n * 40), z(n * 8), z(n), z(n * 16), z(len(w.buf))
    eng.route(m, 8, t(offs), t(lens), n, d_in, t(w.conn_slot), t(w.conn_exp), P.N_CONN, d_route, desc=d_desc)
    eng.route_phase(d_route, t(nxt), P.N_CONN, d_desc, n, d_in, d_phase)
    eng.unprotect(d_desc, n, d_in, d_out, d_res)
    torch.cuda.synchronize()
    before = _crypto.route_phase_launches()
    out, desc, rt, res, walk, walk_n, phase = eng.route_phase_unprotect_host(m, 8, offs, lens, w.buf, [], kslot, kexp,
                                                                            nxt, len(w.buf))
    assert _crypto.route_phase_launches() == before + 1
    assert desc.tobytes() == want_d.tobytes() == d_desc.cpu().numpy().tobytes()
    assert phase.tobytes() == want_p.tobytes() == d_phase.cpu().numpy().tobytes()
    assert rt.tobytes() == route.tobytes() == d_route.cpu().numpy().tobytes()
    assert res.tobytes() == d_res.cpu().numpy().tobytes() and out.tobytes() == d_out.cpu().numpy().tobytes()
    _check_unprotect(w, want_d, out, res)
    # no next slot named: the walk form's launches and bytes, phase_out zeros
    a = eng.route_walk_unprotect_host(m, 8, offs, lens, w.buf, [], kslot, kexp, len(w.buf))
    before = _crypto.route_phase_launches()
    for cn in (None, np.full(P.N_CONN, NONE, np.uint32)):
        b = eng.route_phase_unprotect_host(m, 8, offs, lens, w.buf, [], kslot, kexp, cn, len(w.buf))
        for x, y in zip(a, b[:6]):
            assert x.tobytes() == y.tobytes()
        assert len(b[6]) == n and not b[6].any()
    assert _crypto.route_phase_launches() == before, "no next slot: no launch"
    assert a[1].tobytes() == desc0.tobytes()
    # one slot given: one launch, and only that connection's flips move
    one = np.full(P.N_CONN, NONE, np.uint32)
    one[1] = nxt[1]
    b = eng.route_phase_unprotect_host(m, 8, offs, lens, w.buf, [], kslot, kexp, one, len(w.buf))
    assert _crypto.route_phase_launches() == before + 1
    want1_d, want1_p = P.restate(desc0, route, one, P.N_CONN, w.table, P.CAP, w.buf)
    assert b[1].tobytes() == want1_d.tobytes() and b[6].tobytes() == want1_p.tobytes() and want1_p.any()
    assert {int(route["conn"][i]) for i in np.flatnonzero(want1_p)} == {1}


def test_session_form_with_long_headers(dev):
    """The walking kernel and the resolving kernel in one call: the walk's
    extra descriptors are left alone, the short ones are resolved."""
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    w, table, offs, lens, kslot, kexp, nxt, desc0, route = _session_world()
    eng = PacketEngine(P.CAP)
    eng.set_key_records(w.keys)
    m = eng.cid_map(32)
    m.put(entries(table.items()))
    long_idx = np.asarray([3, 40, 299], np.uint32)  # short headers, listed: the walk finds no packets in them
    a = eng.route_walk_unprotect_host(m, 8, offs, lens, w.buf, long_idx, kslot, kexp, len(w.buf))
    b = eng.route_phase_unprotect_host(m, 8, offs, lens, w.buf, long_idx, kslot, kexp, nxt, len(w.buf))
    want_d, want_p = P.restate(a[1][:w.n], route, nxt, P.N_CONN, w.table, P.CAP, w.buf)
    assert b[1][:w.n].tobytes() == want_d.tobytes() and b[6].tobytes() == want_p.tobytes()
    assert b[1][w.n:].tobytes() == a[1][w.n:].tobytes() and (b[1]["slot"][w.n:] == L.SLOT_NONE).all()
    assert b[4].tobytes() == a[4].tobytes() and b[5].tobytes() == a[5].tobytes()
    _check_unprotect(w, want_d, b[0], b[3][:w.n])


def test_session_form_refuses_a_next_slot_outside_the_table(dev):
    """A conn_next entry >= capacity that is not QPP_SLOT_NONE, or conn_next
    without phase_out: QPP_E_ARG with nothing touched and nothing launched (the
    C ABI itself, through ctypes)."""
    import aioquic_amd  # noqa: F401  (binds torch's HIP runtime first)
    from aioquic_amd import layout as L

    lib = ctypes.CDLL(os.path.join(ROOT, "aioquic_amd", "libquicpp.so"))
    vp, u32, sz = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_size_t
    lib.qpp_session_route_phase_unprotect.restype = ctypes.c_int
    lib.qpp_session_route_phase_unprotect.argtypes = [vp, vp, vp, u32, vp, vp, u32, vp, sz, vp, u32, vp, vp, u32, vp,
                                                      ctypes.c_uint16, vp, sz, vp, vp, vp, vp, vp, vp]
    lib.qpp_route_phase_launches.restype = ctypes.c_uint64
    lib.qpp_cidmap_put.argtypes = [vp, vp, u32, vp]
    for f in (lib.qpp_keytab_destroy, lib.qpp_cidmap_destroy, lib.qpp_session_destroy):
        f.argtypes = [vp]
        f.restype = None
    w, table, offs, lens, kslot, kexp, nxt, desc0, route = _session_world()
    n, size = 40, int(offs[39]) + int(lens[39])
    kt, m, s = vp(), vp(), vp()
    assert lib.qpp_keytab_create(u32(8), ctypes.byref(kt)) == 0
    assert lib.qpp_cidmap_create(u32(32), ctypes.byref(m)) == 0
    assert lib.qpp_session_create(sz(4096), u32(64), ctypes.byref(s)) == 0
    try:
        ent = np.frombuffer(entries(table.items()), np.uint8).copy()
        assert lib.qpp_cidmap_put(m, ent.ctypes.data, len(table), None) == 0
        wire = w.buf[:size].copy()

        def call(cn, with_phase=True):
            cn = np.asarray(cn, np.uint32)
            outs = [np.full(k, 0x5A, np.uint8) for k in (size + 64, n * 40, n * 8, n * 16, n)]
            out, desc, rt, res, phase = outs
            rc = lib.qpp_session_route_phase_unprotect(
                s, kt, m, 8, offs.ctypes.data, lens.ctypes.data, n, wire.ctypes.data, size, None, 0,
                kslot.ctypes.data, kexp.ctypes.data, P.N_CONN, cn.ctypes.data, 0, out.ctypes.data, size,
                desc.ctypes.data, rt.ctypes.data, res.ctypes.data, None, None,
                phase.ctypes.data if with_phase else None)
            return rc, outs

        before = lib.qpp_route_phase_launches()
        ok = np.full(P.N_CONN, NONE, np.uint32)
        for c, bad in ((0, 8), (5, 9), (P.N_CONN - 1, 0xFFFFFFFE)):
            cn = ok.copy()
            cn[c] = bad
            rc, outs = call(cn)
            assert rc == -1, (c, bad)
            assert all((a == 0x5A).all() for a in outs), "a refused call wrote to its output"
        cn = ok.copy()
        cn[2] = 7
        rc, outs = call(cn, with_phase=False)
        assert rc == -1 and all((a == 0x5A).all() for a in outs)
        assert lib.qpp_route_phase_launches() == before, "a refused call launched"
        rc, (out, desc, rt, res, phase) = call(cn)  # slot 7 is inside the table (and empty): accepted
        assert rc == 0 and lib.qpp_route_phase_launches() == before + 1
        assert (out[size:] == 0x5A).all() and rt.tobytes() == route[:n].tobytes() and not phase.any()
        assert (res.view(L.RESULT)["status"] == L.S_NO_KEY).all()  # no keys installed
    finally:
        lib.qpp_session_destroy(s)
        lib.qpp_cidmap_destroy(m)
        lib.qpp_keytab_destroy(kt)


# ---------------------------------------------------------- receive_routed --

def _oracle_tuple(o):
    return (o.datagram, o.offset, o.packet_type, o.dropped, o.plain_header, o.plain_payload, o.packet_number)


def _product_tuple(p):
    return (p.datagram, p.offset, p.packet_type.name, p.dropped, p.plain_header, p.plain_payload, p.packet_number)


def _secrets(conns):
    from aioquic_amd.tls import Epoch

    return [(c.cryptos[Epoch.ONE_RTT].recv.secret, c.cryptos[Epoch.ONE_RTT].send.secret,
             c.cryptos[Epoch.ONE_RTT].recv.key_phase, c.cryptos[Epoch.ONE_RTT].send.key_phase) for c in conns]


class Peers:
    """Five connections (the three suites, both versions) as their peers send
    to them: per connection the sender's current context and next packet
    number, so that batches follow one another on the same state."""

    def __init__(self, seed: int):
        self.rng = np.random.default_rng(seed)
        self.specs = [RS.ConnSpec(self.rng, c, (O.VERSION_1, O.VERSION_2)[c % 2], c % 3) for c in range(5)]
        self.ctx = [W.Ctx(s.suite, s.one_secret, s.version) for s in self.specs]
        self.pn = [1] * 5

    def packet(self, c: int, *, ctx=None, reserved: int = 0, tamper: bool = False, pn=None) -> bytes:
        ctx = ctx or self.ctx[c]
        if pn is None:
            pn = self.pn[c]
            self.pn[c] += 1
        hdr = RS.short_header(self.specs[c].cid, ctx.key_phase, pn, 1 + pn % 4, reserved=reserved)
        p = O.protect(ctx.suite, ctx.key, ctx.iv, ctx.hp, hdr, self.rng.bytes(int(self.rng.integers(4, 400))), pn)
        return p[:-2] + bytes([p[-2] ^ 1]) + p[-1:] if tamper else p

    def flip(self, c: int):
        self.ctx[c] = self.ctx[c].next()

    def batch(self, per_conn: int, flip_at: dict) -> list:
        """per_conn packets of every connection, connection c moving to its
        next phase before its packet flip_at[c]; interleaved, each
        connection's own order kept."""
        streams = []
        for c in range(5):
            st = []
            for k in range(per_conn):
                if flip_at.get(c) == k:
                    self.flip(c)
                st.append(self.packet(c))
            streams.append(st)
        return self.interleave(streams)

    def interleave(self, streams) -> list:
        order = np.concatenate([np.full(len(st), c) for c, st in enumerate(streams)])
        self.rng.shuffle(order)
        pos = [0] * len(streams)
        out = []
        for c in order.tolist():
            out.append(streams[c][pos[c]])
            pos[c] += 1
        return out


class Receiver:
    """Three copies of the receivers' state: the routed path's, the
    demultiplexed product path's and the oracle walk's."""

    def __init__(self, specs):
        from aioquic_amd.route import CidRouter

        self.specs = specs
        self.a = [s.product_conn() for s in specs]
        self.b = [s.product_conn() for s in specs]
        self.o = [s.oracle_conn() for s in specs]
        self.router = CidRouter(8, 64)
        self.by_cid = {}
        for s, c in zip(specs, self.a):
            assert self.router.add(s.cid, c) == s.idx
            self.by_cid[s.cid] = s.idx

    def reference(self, datagrams):
        """receive_datagrams on the second copy and the oracle walk on the
        third, checked against each other; returns receive_datagrams'."""
        from aioquic_amd import receive as R

        conn_of = [self.by_cid[d[1:9]] for d in datagrams]
        want = R.receive_datagrams([(self.b[c], d) for c, d in zip(conn_of, datagrams)])
        gold = W.receive([(self.o[c], d) for c, d in zip(conn_of, datagrams)])
        assert [_product_tuple(p) for p in want] == [_oracle_tuple(o) for o in gold]
        return want

    def check(self, got, unrouted, want):
        assert unrouted == []
        assert [_record_tuple(g) for g in got] == [_record_tuple(x) for x in want]
        assert _state(self.a) == _state(self.b) and _secrets(self.a) == _secrets(self.b)
        for c, o in zip(self.a, self.o):
            from aioquic_amd.tls import Epoch

            ctx = c.cryptos[Epoch.ONE_RTT].recv
            assert (ctx.secret, ctx.key_phase) == (o.pairs["ONE_RTT"].recv.secret, o.pairs["ONE_RTT"].recv.key_phase)
            assert c.closed == o.closed


def _count_batches(monkeypatch):
    from aioquic_amd import receive as R

    made = []
    real = R.ReceiveBatch

    def counting(*a, **kw):
        made.append(1)
        return real(*a, **kw)

    monkeypatch.setattr(R, "ReceiveBatch", counting)
    return made


def _forbid_batches(monkeypatch):
    from aioquic_amd import receive as R

    def refuse(*a, **kw):
        raise AssertionError("ReceiveBatch was constructed")

    monkeypatch.setattr(R, "ReceiveBatch", refuse)


def test_clean_key_update_stays_in_the_fused_call(dev, monkeypatch):
    """Four of five connections update their keys partway through the batch,
    nothing reordered across the flip: with next_phase the one fused call
    resolves it all, no ReceiveBatch; without, the same records through one."""
    from aioquic_amd import _crypto
    from aioquic_amd import receive as R

    peers = Peers(0xC1EA)
    datagrams = peers.batch(30, {0: 11, 1: 20, 2: 7, 4: 29})
    rx = Receiver(peers.specs)
    want = rx.reference(datagrams)
    assert all(r.ok for r in want) and len(want) == 150
    rx2 = Receiver(peers.specs)
    with monkeypatch.context() as mp:
        _forbid_batches(mp)
        before = _crypto.route_phase_launches()
        got, unrouted = R.receive_routed(rx.router, datagrams, next_phase=True)
        assert _crypto.route_phase_launches() == before + 1
    rx.check(got, unrouted, want)
    assert [k for _, _, _, _, k in _state(rx.a)] == [1, 1, 1, 0, 1]
    with monkeypatch.context() as mp:
        made = _count_batches(mp)
        before = _crypto.route_phase_launches()
        got2, unrouted2 = R.receive_routed(rx2.router, datagrams, next_phase=False)
        assert made and _crypto.route_phase_launches() == before
    assert unrouted2 == [] and [_record_tuple(g) for g in got2] == [_record_tuple(x) for x in want]
    assert _state(rx2.a) == _state(rx.a) and _secrets(rx2.a) == _secrets(rx.a)


def test_second_batch_flips_back(dev, monkeypatch):
    """A second and a third batch on the same state, each with another update:
    the cached context was adopted (its slot is the current one, nothing is
    launched again) and the polarity flips back."""
    from aioquic_amd import receive as R
    from aioquic_amd.tls import Epoch

    peers = Peers(0x2B)
    rx = Receiver(peers.specs)
    ctxs = [c.cryptos[Epoch.ONE_RTT].recv for c in rx.a]
    for flip_at, phases in (({0: 3, 2: 9}, [1, 0, 1, 0, 0]), ({0: 5, 1: 0, 2: 11}, [0, 1, 0, 0, 0]),
                            ({3: 6}, [0, 1, 0, 1, 0])):
        datagrams = peers.batch(12, flip_at)
        want = rx.reference(datagrams)  # (it may batch as it likes)
        held = [c._next for c in ctxs]  # cached by the batch before, where the connection did not update
        with monkeypatch.context() as mp:
            _forbid_batches(mp)
            got, unrouted = R.receive_routed(rx.router, datagrams, next_phase=True)
        rx.check(got, unrouted, want)
        assert all(r.ok for r in got)
        assert [k for _, _, _, _, k in _state(rx.a)] == phases
        for c, ctx in enumerate(ctxs):
            if c in flip_at:
                assert ctx._next is None, "the cached context was adopted and dropped"
                assert held[c] is None or ctx.aead is held[c].aead, "adopted as it was: nothing re-installed"
            else:
                assert ctx._next is not None and ctx._next.key_phase == 1 - ctx.key_phase
                assert held[c] is None or ctx._next is held[c], "built once per phase"


def _routed_vs_demultiplexed(specs, items, extra=(), next_phase=True):
    """tests/test_gpu_route.py's comparison with the keyword passed on."""
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
    got, unrouted = R.receive_routed(router, datagrams, next_phase=next_phase)
    assert unrouted == want_unrouted
    assert [_record_tuple(g) for g in got] == [_record_tuple(x) for x in want]
    assert _state(conns_a) == _state(conns_b) and _secrets(conns_a) == _secrets(conns_b)
    return got, unrouted


def test_all_short_scenario_with_next_phase(dev):
    """The all-short scenario of tests/test_gpu_route.py: a key update per
    connection, an old-phase replay after it (deferred), a tampered packet, a
    reserved bit after the update, reordering, a closed and a keyless
    connection."""
    from aioquic_amd import _crypto

    specs, items = RS.build(seed=0x5A, n_conns=7, per_conn=90, client=False)
    items = [(c, d) for c, d in items if not d or not d[0] & 0x80]
    rng = np.random.default_rng(9)
    extra = [(5, bytes([0x41]) + bytes(8) + rng.bytes(40)), (17, b""), (40, bytes([0x42]) + rng.bytes(60)),
             (41, bytes([0xC3]) + b"\x00\x00\x00\x01\x08" + bytes(8) + rng.bytes(30))]
    before = _crypto.route_phase_launches()
    got, unrouted = _routed_vs_demultiplexed(specs, items, extra)
    assert _crypto.route_phase_launches() == before + 1
    assert {None, "payload_decrypt_error", "key_unavailable", "reserved_bits", "connection_closed"} <= \
        {r.dropped for r in got}


@pytest.mark.parametrize("client", [False, True])
def test_full_scenario_with_next_phase(dev, client):
    """Long headers that reach known connections (the batch gets no next
    slots) and, with `client`, the general path: results as ever."""
    from aioquic_amd import _crypto

    specs, items = RS.build(client=client)
    before = _crypto.route_phase_launches()
    got, _ = _routed_vs_demultiplexed(specs, items)
    assert _crypto.route_phase_launches() == before
    assert {None, "payload_decrypt_error", "key_unavailable", "reserved_bits", "connection_closed"} <= \
        {r.dropped for r in got}


def test_flipped_packet_with_a_reserved_bit(dev, monkeypatch):
    """The first packet of the next phase carries a reserved bit: the key
    update stands (crypto.py:184-192 runs before connection.py:949-960) and
    the connection closes; the batch still needs no ReceiveBatch."""
    from aioquic_amd import receive as R

    peers = Peers(0x77)
    streams = []
    for c in range(5):
        st = [peers.packet(c) for _ in range(4)]
        if c in (1, 2):
            peers.flip(c)
            st.append(peers.packet(c, reserved=0x10 if c == 1 else 0x08))
        st += [peers.packet(c) for _ in range(3)]
        streams.append(st)
    datagrams = peers.interleave(streams)
    rx = Receiver(peers.specs)
    want = rx.reference(datagrams)
    assert [r.dropped for r in want].count("reserved_bits") == 2
    _forbid_batches(monkeypatch)
    got, unrouted = R.receive_routed(rx.router, datagrams, next_phase=True)
    rx.check(got, unrouted, want)
    assert [(closed, k) for closed, _, _, _, k in _state(rx.a)] == [(False, 0), (True, 1), (True, 1), (False, 0),
                                                                    (False, 0)]


def test_tampered_first_flipped_packet(dev, monkeypatch):
    """The first packet of the next phase fails its tag: payload_decrypt_error
    and no roll; the next one authenticates and rolls."""
    from aioquic_amd import receive as R

    peers = Peers(0x78)
    streams = []
    for c in range(5):
        st = [peers.packet(c) for _ in range(3)]
        if c != 3:
            peers.flip(c)
            st.append(peers.packet(c, tamper=True))
            if c == 4:
                st.append(peers.packet(c, tamper=True))  # and nothing good after: no roll at all
            else:
                st += [peers.packet(c) for _ in range(3)]
        streams.append(st)
    datagrams = peers.interleave(streams)
    rx = Receiver(peers.specs)
    want = rx.reference(datagrams)
    assert [r.dropped for r in want].count("payload_decrypt_error") == 5
    _forbid_batches(monkeypatch)
    got, unrouted = R.receive_routed(rx.router, datagrams, next_phase=True)
    rx.check(got, unrouted, want)
    assert [k for _, _, _, _, k in _state(rx.a)] == [1, 1, 1, 0, 0]


def test_key_table_too_small_for_the_next_slots(dev, monkeypatch):
    """A table that holds the batch's keys but not the next slots beside
    them: the batch runs as with next_phase=False."""
    from aioquic_amd import _crypto
    from aioquic_amd import receive as R
    from aioquic_amd.batch_io import KeySlots

    peers = Peers(0x79)
    datagrams = peers.batch(10, {0: 4, 3: 6})
    rx = Receiver(peers.specs)
    want = rx.reference(datagrams)
    small = KeySlots(7)
    monkeypatch.setattr(R, "default_slots", lambda: small)
    made = _count_batches(monkeypatch)
    before = _crypto.route_phase_launches()
    got, unrouted = R.receive_routed(rx.router, datagrams, next_phase=True)
    assert _crypto.route_phase_launches() == before and made, "no next slots: the flips went through ReceiveBatch"
    rx.check(got, unrouted, want)
    small.close()
