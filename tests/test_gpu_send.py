"""GPU checks of routed send (include/quic_pp.h: qpp_send_fill,
qpp_session_send_protect) and of send.send_routed.

The reference is the restatement of tests/send_cases.py, the C oracle's
protect over the restated descriptors, per-connection QuicPacketBuilders with
flush_builders for the same payloads, and receive_routed of a peer router for
the round trip."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import receive_scenario as RS
from tests import send_cases as S

pytestmark = pytest.mark.gpu


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


def _check_protect(w, want_buf, want_desc, out, res):
    """The protect over the filled buffer against the C oracle over the
    restated one: statuses, the OK packets' bytes, nothing outside a packet."""
    from aioquic_amd import layout as L

    want_out, want_res = O.protect_batch(w.keys, want_desc, want_buf, len(want_buf))
    assert res["status"].tolist() == want_res["status"].tolist()
    ok = want_res["status"] == L.S_OK
    for f in ("pn", "hdr_len", "out_len"):
        assert (res[f][ok] == want_res[f][ok]).all(), f
    inside = np.zeros(len(want_buf), bool)
    for k in np.flatnonzero(ok).tolist():
        o, ln = int(want_desc["out_off"][k]), int(want_res["out_len"][k])
        assert ln == int(want_desc["hdr_len"][k]) + int(want_desc["len"][k]) + 16
        assert out[o:o + ln].tobytes() == want_out[o:o + ln].tobytes(), k
        inside[o:o + ln] = True
    assert not out[~inside].any(), "bytes outside every packet were written"
    return want_res


# ------------------------------------------------------------ qpp_send_fill --

@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_send_fill_matches_restatement(dev, n):
    """One launch over tests/send_cases.World at the workgroup's edges, over
    a poisoned buffer and outputs: buffer, d_desc and d_rec byte for byte, the
    inputs unchanged, then qpp_protect over the result against the oracle."""
    import torch
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    w = S.World(n)
    eng = PacketEngine(S.CAP)
    eng.set_key_records(w.keys[w.keys["suite"] != S.EMPTY])
    want_buf, want_desc, want_rec = S.restate_world(w)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    canary = lambda size: torch.full((size + 64,), 0xAB, dtype=torch.uint8, device=dev)
    d_buf = torch.cat([t(w.buf), canary(0)])
    d_conns, d_off, d_len, d_conn, d_seq = t(w.conns), t(w.off), t(w.len), t(w.conn), t(w.seq)
    d_desc, d_rec, d_res = canary(n * 40), canary(n * 16), canary(n * 16)
    d_out = torch.zeros(len(w.buf), dtype=torch.uint8, device=dev)
    before = _crypto.send_launches()
    eng.send_fill(d_conns, S.N_CONN, d_off, d_len, d_conn, d_seq, n, d_buf, d_desc, d_rec, buf_len=w.buf_len)
    eng.protect(d_desc, n, d_buf, d_out, d_res)
    torch.cuda.synchronize()
    assert _crypto.send_launches() == before + 1
    buf, desc, rec, res = (x.cpu().numpy() for x in (d_buf, d_desc, d_rec, d_res))
    for a, size in ((buf, len(w.buf)), (desc, n * 40), (rec, n * 16), (res, n * 16)):
        assert (a[size:] == 0xAB).all(), "wrote past the end"
    assert rec[:n * 16].tobytes() == want_rec.tobytes()
    assert desc[:n * 40].tobytes() == want_desc.tobytes()
    assert buf[:len(w.buf)].tobytes() == want_buf.tobytes()
    for d, a in ((d_conns, w.conns), (d_off, w.off), (d_len, w.len), (d_conn, w.conn), (d_seq, w.seq)):
        assert d.cpu().numpy().tobytes() == a.tobytes(), "the inputs are only read"
    want_res = _check_protect(w, want_buf, want_desc, d_out.cpu().numpy(), res[:n * 16].view(L.RESULT))
    st = want_res["status"]
    if n == 1:
        assert want_rec["status"].tolist() == [L.SN_OK] and st.tolist() == [L.S_OK]
    else:
        built = want_rec["status"] == L.SN_OK
        assert set(want_rec["status"].tolist()) == {L.SN_OK, L.SN_CONN, L.SN_CID, L.SN_NO_KEY, L.SN_EMPTY, L.SN_PN,
                                                    L.SN_ROOM}
        assert (st[~built] == L.S_NO_KEY).all(), "an inert descriptor is answered, nothing of it is touched"
        kinds = np.asarray(w.kind)
        assert (st[kinds == "over"] == L.S_LENGTH).all() and (kinds == "over").any(), "the length limit is protect's"
        assert (st[built & (kinds == "ok")] == L.S_OK).all()


def test_send_fill_arguments(dev):
    import torch
    from aioquic_amd import _crypto
    from aioquic_amd.batch import PacketEngine

    eng = PacketEngine(4)
    z = torch.zeros(256, dtype=torch.uint8, device=dev)

    class Null:
        @staticmethod
        def data_ptr():
            return 0

    before = _crypto.send_launches()
    for k in range(8):
        a = [z] * 8
        a[k] = Null
        conns, off, ln, cn, sq, buf, desc, rec = a
        with pytest.raises(ValueError):
            eng.send_fill(conns, 1, off, ln, cn, sq, 1, buf, desc, rec, buf_len=256)
    eng.send_fill(Null, 0, Null, Null, Null, Null, 0, Null, Null, Null, buf_len=0)  # n == 0: nothing to do
    assert _crypto.send_launches() == before


# -------------------------------------------------------------- fused form --

def test_fused_form_matches_oracle(dev):
    """_crypto.send_routed at n = 257: the datagrams equal the oracle's
    protection of restated header || payload || padding; one filling launch."""
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    w = S.World(257, fused=True)
    eng = PacketEngine(S.CAP)
    eng.set_key_records(w.keys[w.keys["suite"] != S.EMPTY])
    # the binding lays the payloads out itself: HEAD before each, TAIL behind, no gaps
    assert w.off[0] == L.SEND_HEAD and w.buf_len == int(w.off[-1]) + int(w.len[-1]) + L.SEND_TAIL
    want_buf, want_desc, want_rec = S.restate_world(w)
    want_out, want_res = O.protect_batch(w.keys, want_desc, want_buf, len(want_buf))
    before = _crypto.send_launches()
    wires, rec, res = _crypto.send_routed(eng.table, w.conns.tobytes(), w.conn.tobytes(), list(w.payloads))
    assert _crypto.send_launches() == before + 1
    rec, res = np.frombuffer(rec, L.SEND_REC), np.frombuffer(res, L.RESULT)
    assert rec.tobytes() == want_rec.tobytes()
    assert res["status"].tolist() == want_res["status"].tolist()
    sent = 0
    for k in range(w.n):
        if want_rec["status"][k] != L.SN_OK or want_res["status"][k] != L.S_OK:
            assert wires[k] == b"", k
            continue
        o, ln = int(want_desc["out_off"][k]), int(want_res["out_len"][k])
        c = w.conns[w.conn[k]]
        slot = w.keys[int(c["slot"])]
        suite = int(slot["suite"])
        kl = S.KEY_LEN[suite]
        hdr = S.short_header(int(c["spin"]), int(slot["key_phase"]), w.cids[w.conn[k]], int(want_rec["pn"][k]))
        body = w.payloads[k] + bytes(S.padding_size(len(w.payloads[k])))
        direct = O.protect(suite, slot["key"][:kl].tobytes(), slot["iv"].tobytes(), slot["hp"][:kl].tobytes(), hdr,
                           body, int(want_rec["pn"][k]))
        assert wires[k] == direct == want_out[o:o + ln].tobytes(), k
        sent += 1
    assert sent > 230 and {L.SN_CID, L.SN_NO_KEY, L.SN_EMPTY, L.SN_PN} <= set(rec["status"].tolist())
    assert L.S_LENGTH in res["status"].tolist()
    # the same arrays through the raw host form: the same records and bytes, zeros between the packets
    out, desc, rec2, res2 = eng.send_protect_host(w.conns, w.off, w.len, w.conn, w.seq, w.buf, w.buf_len)
    assert desc.tobytes() == want_desc.tobytes() and rec2.tobytes() == want_rec.tobytes()
    assert res2.tobytes() == res.tobytes()
    _check_protect(w, want_buf, want_desc, out, res2)
    # an empty batch launches nothing
    before = _crypto.send_launches()
    assert _crypto.send_routed(eng.table, w.conns.tobytes(), b"", []) == ([], b"", b"")
    out, desc, rec2, res2 = eng.send_protect_host(w.conns, [], [], [], [], b"", 64)
    assert not out.any() and len(out) == 64 and len(desc) == len(rec2) == len(res2) == 0
    assert _crypto.send_launches() == before


def test_fused_form_refusals(dev):
    """Every host-side refusal is QPP_E_ARG (ValueError) with the launch
    counter unchanged: an overlap, an offset out of order, a region past
    either buffer, a bad connection index, a slot past the table."""
    from aioquic_amd import _crypto
    from aioquic_amd.batch import PacketEngine

    w = S.World(257, fused=True)
    eng = PacketEngine(S.CAP)
    eng.set_key_records(w.keys[w.keys["suite"] != S.EMPTY])

    def call(off=w.off, lens=w.len, conn=w.conn, conns=w.conns, buf=w.buf, out_len=w.buf_len):
        return eng.send_protect_host(conns, off, lens, conn, w.seq, buf, out_len)

    def swapped():
        a = w.off.copy()
        a[[50, 51]] = a[[51, 50]]
        return a

    def moved(k, by):
        a = w.off.copy()
        a[k] = int(a[k]) + by
        return a

    bad_conn = w.conn.copy()
    bad_conn[7] = S.N_CONN
    bad_slot = w.conns.copy()
    bad_slot["slot"][3] = S.CAP
    longer = w.len.copy()
    longer[60] += 1
    refused = [("an overlap", dict(off=moved(100, -1))), ("a longer payload overlaps", dict(lens=longer)),
               ("an offset out of order", dict(off=swapped())), ("in front of the buffer", dict(off=moved(0, -1))),
               ("past the input", dict(buf=w.buf[:w.buf_len - 1])), ("past the output", dict(out_len=w.buf_len - 1)),
               ("a bad conn", dict(conn=bad_conn)), ("a slot past the table", dict(conns=bad_slot))]
    before = _crypto.send_launches()
    for what, kw in refused:
        with pytest.raises(ValueError, match="nothing was launched"):
            call(**kw)
        assert _crypto.send_launches() == before, what
    with pytest.raises(ValueError, match="nothing was launched"):
        _crypto.send_routed(eng.table, w.conns.tobytes(), bad_conn.tobytes(), list(w.payloads))
    with pytest.raises(ValueError, match="nothing was launched"):
        _crypto.send_routed(eng.table, bad_slot.tobytes(), w.conn.tobytes(), list(w.payloads))
    assert _crypto.send_launches() == before
    call()
    assert _crypto.send_launches() == before + 1


# ------------------------------------------------------- send.send_routed --

SUITES = {O.AES_128_GCM: "AES_128_GCM_SHA256", O.AES_256_GCM: "AES_256_GCM_SHA384",
          O.CHACHA20_POLY1305: "CHACHA20_POLY1305_SHA256"}


def _pair(suite, secret):
    from aioquic_amd.crypto import CryptoPair
    from aioquic_amd.tls import CipherSuite

    p = CryptoPair()
    for ctx in (p.send, p.recv):
        ctx.setup(cipher_suite=getattr(CipherSuite, SUITES[suite]), secret=secret, version=O.VERSION_1)
    return p


def _payloads(rng, sizes):
    # one STREAM frame's bytes each: the builder writes the frame type itself
    return [b"\x08" + rng.bytes(size - 1) for size in sizes]


def test_send_routed_equals_flush_builders(dev):
    """Eight connections of mixed suites, one with a local key update
    pending: the same payloads as one packet each through per-connection
    builders and flush_builders give equal datagrams and packet numbers."""
    from aioquic_amd import send
    from aioquic_amd.batch_io import KeySlots
    from aioquic_amd.packet import QuicFrameType, QuicPacketType, QuicProtocolVersion
    from aioquic_amd.packet_builder import QuicPacketBuilder, flush_builders

    rng = np.random.default_rng(0x5E4D)
    cid_lens = (8, 0, 1, 20, 8, 5, 8, 20)
    starts = (0, 0xFFFE, (1 << 32) + 0xFFFD, 77, 1 << 40, 5, 6, 7)
    secrets = [rng.bytes(48 if c % 3 == 1 else 32) for c in range(8)]
    cids = [rng.bytes(k) for k in cid_lens]
    sizes = [1, 2, 3, 1173, 40, 200, 9, 1500 - 16 - 3 - 20, 64, 5] * 4
    items = [(int(c), p) for c, p in zip(rng.integers(0, 8, len(sizes)), _payloads(rng, sizes))]
    items = [(c, p[:S.longest_payload(cid_lens[c])]) for c, p in items]

    def make():
        pairs = [_pair(c % 3, secrets[c]) for c in range(8)]
        pairs[2].update_key()
        pairs[6].update_key()
        return pairs

    # the way a caller does it today
    pairs_b = make()
    builders = [QuicPacketBuilder(host_cid=bytes(8), peer_cid=cids[c], version=QuicProtocolVersion.VERSION_1,
                                  is_client=False, max_datagram_size=1500, packet_number=starts[c], spin_bit=bool(c & 1))
                for c in range(8)]
    for c, p in items:
        builders[c].start_packet(QuicPacketType.ONE_RTT, pairs_b[c])
        builders[c].start_frame(QuicFrameType.STREAM_BASE, capacity=len(p)).push_bytes(p[1:])
    slots_b = KeySlots(32)
    flushed = flush_builders(builders, slots=slots_b)
    per_conn = [iter(zip(dgs, pkts)) for dgs, pkts in flushed]
    want = [next(per_conn[c]) for c, _ in items]
    # routed send
    pairs_s = make()
    conns = [send.SendConnection(pairs_s[c], cids[c], starts[c], bool(c & 1)) for c in range(8)]
    slots_s = KeySlots(32)
    wires, pns = send.send_routed(conns, items, slots=slots_s)
    assert pns == [pkt.packet_number for _, pkt in want]
    assert wires == [dg for dg, _ in want]
    assert [c.packet_number for c in conns] == [b.packet_number for b in builders]
    for c in (2, 6):
        assert pairs_s[c].send.key_phase == 1 == pairs_b[c].send.key_phase and not pairs_s[c]._update_key_requested
    assert pairs_s[0].send.key_phase == 0
    # a second batch goes on where the first stopped, under the updated keys
    more = [(c, p) for c, p in items[:16]]
    for c, p in more:
        builders[c].start_packet(QuicPacketType.ONE_RTT, pairs_b[c])
        builders[c].start_frame(QuicFrameType.STREAM_BASE, capacity=len(p)).push_bytes(p[1:])
    per_conn = [iter(dgs) for dgs, _ in flush_builders(builders, slots=slots_b)]
    wires2, pns2 = send.send_routed(conns, more, slots=slots_s)
    assert wires2 == [next(per_conn[c]) for c, _ in more]
    assert [c.packet_number for c in conns] == [b.packet_number for b in builders]
    slots_b.close(), slots_s.close()


def test_send_routed_round_trip(dev):
    """send_routed's datagrams through receive_routed of a peer router: the
    payloads and packet numbers come back in order; the 1-byte payload comes
    back as two bytes, the second zero."""
    from aioquic_amd import receive as R
    from aioquic_amd import send
    from aioquic_amd.route import CidRouter

    rng = np.random.default_rng(0x7217)
    specs = [RS.ConnSpec(rng, k, O.VERSION_1, k % 3) for k in range(6)]
    peers = [s.product_conn() for s in specs]
    router = CidRouter(8, 16)
    for s, p in zip(specs, peers):
        assert router.add(s.cid, p) == s.idx
    conns = [send.SendConnection(_pair(s.suite, s.one_secret), s.cid, 3 * s.idx, bool(s.idx & 1)) for s in specs]
    sizes = [1, 2, 3, 1173, 40, 1] * 5
    items = [(int(c), p) for c, p in zip(rng.integers(0, 6, len(sizes)), _payloads(rng, sizes))]
    wires, pns = send.send_routed(conns, items)
    assert len(wires) == len(items) and all(wires)
    got, unrouted = R.receive_routed(router, wires)
    assert unrouted == [] and len(got) == len(items)
    seen = [3 * k for k in range(6)]
    for r, (c, p), pn in zip(got, items, pns):
        assert r.ok and r.packet_number == pn == seen[c]
        seen[c] += 1
        assert r.plain_payload == (p + b"\x00" if len(p) == 1 else p)
    assert [c.packet_number for c in conns] == seen
