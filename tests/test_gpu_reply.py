"""GPU checks of the Retry / Version Negotiation replies built on the device
(include/quic_pp.h: qpp_route_reply, qpp_session_accept_reply_unprotect) and
of receive.answer_routed.

The reference is the restatement of tests/reply_cases.py -- the reference's
encoders in Python with the C oracle's AES-128-GCM for the token's seal and
the Retry integrity tag -- and, for answer_routed, accept_routed in Retry mode
with every reply built on the host."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import accept_cases as A
from tests import reply_cases as R
from tests import walk_cases as C
from tests.test_gpu_accept import SCID, Server, _batch, client_initial, initial_keys, new_conn
from tests.test_gpu_route import _record_tuple

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
CANARY = 0xAB
VERSIONS = [R.V1, R.V2]


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


def tokens_of(counter: int = 0):
    from aioquic_amd.retry import RetryTokens

    return RetryTokens(R.TOKEN_KEY, R.TOKEN_IV, counter=counter)


def reply_engine():
    from aioquic_amd.batch import PacketEngine

    eng = PacketEngine(3)
    eng.set_key_records(tokens_of().key_records())
    return eng


class Fenced:
    """A device buffer of `size` bytes with 256 canary bytes on either side."""

    def __init__(self, dev, size):
        import torch

        self.size = size
        self.whole = torch.full((size + 512,), CANARY, dtype=torch.uint8, device=dev)
        self.t = self.whole[256:256 + size]

    def read(self):
        a = self.whole.cpu().numpy()
        assert (a[:256] == CANARY).all() and (a[256 + self.size:] == CANARY).all(), "wrote outside the array"
        return a[256:256 + self.size]


# ------------------------------------------------------------ device form --

@pytest.mark.parametrize("n_acc", [1, 255, 256, 257, 8192, 8193])
def test_route_reply_matches_restatement(dev, n_acc):
    """Hand-built walk and accept records over synthetic headers, one
    datagram per candidate, each followed by bytes that would complete it."""
    import torch
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L

    datagrams, tails, statuses, walks, addrs, rnd = R.synthetic(n_acc)
    ctr0 = (1 << 40) + 5
    flags = L.RP_VN | L.RP_RETRY
    # the buffer: odd offsets, the tail and poison after every datagram
    offs, parts, pos = [], [b"\x11"], 1
    for d, tail in zip(datagrams, tails):
        offs.append(pos)
        fill = d + (tail + bytes(range(0x10, 0x40)))[:48]
        fill += b"\x40" * (1 - (pos + len(fill)) % 2)
        parts.append(fill)
        pos += len(fill)
    buf = np.frombuffer(b"".join(parts), np.uint8).copy()
    lens = np.asarray([len(d) for d in datagrams], np.uint32)
    walk = np.zeros((n_acc, L.WALK_MAX), L.WALK)
    walk["desc"] = NONE
    for f in ("version", "dcid_len", "scid_len"):
        walk[f][:, 0] = [w[f] for w in walks]
    walk["len"][:, 0] = lens
    acc = np.zeros(n_acc, L.ACCEPT)
    acc["desc"], acc["status"] = NONE, statuses
    idx = np.arange(n_acc, dtype=np.uint32)
    # the restatement, before and after the two launches
    want_region, want_seal, want_tag, want_rec, want_done = [], [], [], [], []
    want_res = np.zeros((2, n_acc), L.RESULT)
    for a in range(n_acc):
        region, seal, tag, rec = R.restate(a, statuses[a], walks[a], datagrams[a], addrs[a], rnd[a].tobytes(), ctr0,
                                           VERSIONS, flags)
        done, want_res[0, a:a + 1], want_res[1, a:a + 1] = R.launches(region, seal, tag, a * R.STRIDE)
        want_region.append(region), want_seal.append(seal), want_tag.append(tag), want_rec.append(rec)
        want_done.append(done)
    want_rec = np.concatenate(want_rec)
    if n_acc >= 255:
        assert set(want_rec["kind"].tolist()) == {L.RP_KIND_NONE, L.RP_KIND_VN, L.RP_KIND_RETRY}
        assert L.RP_BOUNDS in want_rec["status"].tolist()

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_in, d_off, d_len, d_idx = t(buf), t(np.asarray(offs, np.uint64)), t(lens), t(idx)
    d_walk, d_acc, d_addr, d_rand = t(walk), t(acc), t(np.frombuffer(b"".join(addrs), np.uint8)), t(rnd)
    reply, seal, tag = Fenced(dev, n_acc * R.STRIDE), Fenced(dev, n_acc * 40), Fenced(dev, n_acc * 40)
    rec, res1, res2 = Fenced(dev, n_acc * 8), Fenced(dev, n_acc * 16), Fenced(dev, n_acc * 16)
    eng = reply_engine()
    before = _crypto.route_reply_launches()
    eng.route_reply(d_off, d_len, n_acc, d_in, d_idx, n_acc, d_walk, d_idx, d_acc, 0, d_addr, d_rand, ctr0, VERSIONS,
                    flags, reply.t, seal.t, tag.t, rec.t)
    torch.cuda.synchronize()
    assert _crypto.route_reply_launches() == before, "no candidates: nothing launched"
    assert (reply.read() == CANARY).all() and (rec.read() == CANARY).all()
    eng.route_reply(d_off, d_len, n_acc, d_in, d_idx, n_acc, d_walk, d_idx, d_acc, n_acc, d_addr, d_rand, ctr0,
                    VERSIONS, flags, reply.t, seal.t, tag.t, rec.t)
    torch.cuda.synchronize()
    assert _crypto.route_reply_launches() == before + 1
    assert reply.read().tobytes() == b"".join(want_region)
    assert seal.read().tobytes() == np.concatenate(want_seal).tobytes()
    assert tag.read().tobytes() == np.concatenate(want_tag).tobytes()
    assert rec.read().tobytes() == want_rec.tobytes()
    eng.protect(seal.t, n_acc, reply.t, reply.t, res1.t)
    eng.protect(tag.t, n_acc, reply.t, reply.t, res2.t)
    torch.cuda.synchronize()
    assert _crypto.route_reply_launches() == before + 1
    got = reply.read().tobytes()
    for a in np.flatnonzero(want_rec["kind"] != L.RP_KIND_NONE).tolist()[:64]:
        assert got[a * R.STRIDE:(a + 1) * R.STRIDE] == want_done[a], a
    assert got == b"".join(want_done)
    assert res1.read().tobytes() == want_res[0].tobytes() and res2.read().tobytes() == want_res[1].tobytes()
    assert rec.read().tobytes() == want_rec.tobytes() and seal.read().tobytes() == np.concatenate(want_seal).tobytes()
    assert d_walk.cpu().numpy().tobytes() == walk.tobytes() and d_acc.cpu().numpy().tobytes() == acc.tobytes()


def test_route_reply_rejects_bad_arguments(dev):
    import torch
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    z = torch.zeros(512, dtype=torch.uint8, device=dev)
    before = _crypto.route_reply_launches()
    call = lambda versions, flags, addr=z, reply=z: PacketEngine.route_reply(
        z, z, 1, z, z, 1, z, z, z, 1, addr, z, 0, versions, flags, reply, z, z, z)
    for versions, flags in (([], L.RP_VN), (list(range(17)), L.RP_VN), ([1], 4), ([1], 7)):
        with pytest.raises(ValueError):
            call(versions, flags)
    with pytest.raises(ValueError):
        call([1], L.RP_RETRY, addr=None)
    with pytest.raises(ValueError):
        _crypto.route_reply(z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), 1, z.data_ptr(), z.data_ptr(),
                            z.data_ptr(), 1, z.data_ptr(), z.data_ptr(), 0, np.asarray([1], np.uint32).tobytes(),
                            L.RP_VN, 0, z.data_ptr(), z.data_ptr(), z.data_ptr(), 0)
    assert _crypto.route_reply_launches() == before


# ------------------------------------- what the reply launches rest on ----

@pytest.mark.parametrize("n", [8192, 8193])
def test_aead_only_empty_payload_long_aad_in_place(dev, n):
    """AEAD-only protect with no payload over 66..160 and 1500 bytes of
    associated data, in place, on the reply table's two Retry keys: what the
    integrity-tag launch is.  (This one needs nothing the reply path adds.)"""
    import torch
    from aioquic_amd import layout as L

    aads = list(range(66, 161)) + [1500]
    rng = np.random.default_rng(n)
    hl = np.asarray([aads[k % len(aads)] for k in range(n)], np.int64)
    space = (hl + 16 + 15) // 16 * 16 + 16 * (np.arange(n) % 3)
    offs = np.concatenate([[0], np.cumsum(space)[:-1]]) + 3
    buf = np.zeros(int(offs[-1] + space[-1]) + 16, np.uint8)
    for k in range(n):
        buf[offs[k]:offs[k] + hl[k]] = rng.integers(0, 256, int(hl[k]), dtype=np.uint8)
    desc = np.zeros(n, L.DESC)
    desc["in_off"] = desc["out_off"] = offs
    desc["hdr_len"], desc["flags"], desc["slot"] = hl, L.F_NO_HP, np.arange(n) % 2
    keys = tokens_of().key_records()
    want, want_res = O.protect_batch(keys, desc, buf, len(buf))
    assert (want_res["status"] == L.S_OK).all() and (want_res["out_len"] == hl + 16).all()
    assert want.tobytes() != buf.tobytes() and (want[offs[5]:offs[5] + hl[5]] == buf[offs[5]:offs[5] + hl[5]]).all()
    eng = reply_engine()
    d_buf, d_desc = torch.from_numpy(buf.copy()).to(dev), torch.from_numpy(desc.view(np.uint8).copy()).to(dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    eng.protect(d_desc, n, d_buf, d_buf, d_res)
    torch.cuda.synchronize()
    assert d_res.cpu().numpy().tobytes() == want_res.tobytes()
    assert d_buf.cpu().numpy().tobytes() == want.tobytes()


# -------------------------------------------------------------- fused form --

def addr_of(i: int, v6=None):
    v6 = i % 2 == 0 if v6 is None else v6
    return ("2001:db8::%x" % (i + 1), 5000 + i) if v6 else ("203.0.113.%d" % (i % 250 + 1), 4000 + i)


def initial_with_token(dcid: bytes, version: int, token: bytes, pn: int = 0, size: int = 1200):
    """A client's protected Initial whose token may be 64 bytes and more."""
    _, key, iv, hp = initial_keys(dcid, version)
    bits = 1 if version == O.VERSION_2 else 0

    def hdr(rest):
        return (bytes([0xC0 | bits << 4 | 1]) + version.to_bytes(4, "big") + bytes([len(dcid)]) + dcid
                + bytes([len(SCID)]) + SCID + C.varint(len(token), 1) + token + (0x4000 | (rest + 2)).to_bytes(2, "big")
                + pn.to_bytes(2, "big"))

    body = size - len(hdr(0)) - 16
    out = O.protect(O.AES_128_GCM, key, iv, hp, hdr(body + 16), (b"\x06\x00\x40\x10" + bytes(body))[:body], pn)
    assert len(out) == size
    return out


class Flood:
    """A server's batch: three known connections' traffic, token-less
    Initials of both versions from both address families, an Initial with a
    token, Initials of a version nobody speaks, a too-small one and a
    Handshake packet to an unknown DCID."""

    DCIDS = (b"\xA1" * 8, b"\xB2" * 20, b"\xC3", b"\xC4" * 5, b"\xA5" * 8)

    def __init__(self, monkeypatch, **kw):
        self.srv = Server(monkeypatch, **kw)
        self.tokenless = [client_initial(d, (O.VERSION_1, O.VERSION_2)[k % 2], fill=k)[0]
                          for k, d in enumerate(self.DCIDS)]
        self.with_token = client_initial(b"\xD5" * 8, O.VERSION_1, token=b"not-ours", fill=9)[0]
        self.grease = [A.initial(R.GREASE, b"\xE6" * 8, 1200), A.initial(R.GREASE, b"\xE7" * 3, 700, scid=b""),
                       A.initial(R.GREASE, b"", 1300)]
        self.small = client_initial(b"\xD4" * 8, O.VERSION_1, size=1199)[0]
        self.handshake = C.long_packet(0xE0, C.V1, b"\x0F" * 8, b"", body=bytes(1250))
        extra = self.tokenless[:2] + [self.with_token, self.grease[0], self.small] + self.tokenless[2:4] + \
            [self.grease[1], self.handshake, self.tokenless[4], self.grease[2]]
        self.datagrams = _batch(self.srv, extra)
        self.addrs = [addr_of(i) for i in range(len(self.datagrams))]
        for k, d in enumerate(self.tokenless):  # both address families among the Retries
            self.addrs[self.datagrams.index(d)] = addr_of(self.datagrams.index(d), v6=bool(k % 2))
        self.lidx = [i for i, d in enumerate(self.datagrams) if d and d[0] & 0x80]
        known = {s.cid for s in self.srv.specs}
        self.rows = [r for r, i in enumerate(self.lidx) if self.datagrams[i][6:6 + self.datagrams[i][5]] not in known]
        self.cand = [self.lidx[r] for r in self.rows]

    def expected(self, rnd: bytes, ctr0: int, flags: int, need_token: bool = True):
        """Per candidate: (its 256 bytes after both launches, its reply record)."""
        from aioquic_amd import layout as L

        out = []
        for a, i in enumerate(self.cand):
            d = self.datagrams[i]
            recs = C.restate_walk(d, 8)
            st = A.restate_status((NONE, L.R_LONG), recs, len(d), L.A_NEED_TOKEN if need_token else 0)
            w = recs[0] if recs else {"version": 0, "dcid_len": 0, "scid_len": 0}
            region, seal, tag, rec = R.restate(a, st, w, d, R.packed_addr(self.addrs[i]), rnd[16 * a:16 * a + 16], ctr0,
                                               VERSIONS, flags)
            out.append((R.launches(region, seal, tag, a * R.STRIDE)[0], rec, st))
        return out

    def call(self, taken, tokens, rnd, ctr0, flags, *, addr=None, versions=VERSIONS, table=None, reply=True):
        from aioquic_amd import _crypto
        from aioquic_amd import layout as L
        from aioquic_amd import receive as RX
        from aioquic_amd.packet import QuicPacketType
        from aioquic_amd.tls import Epoch

        srv = self.srv
        _, _, _, arrays, _ = RX._routed_arrays(srv.router, self.datagrams, False)
        args = (srv.slots.table, srv.router.map, 8, self.datagrams, *arrays, RX.ReceivedPacket, QuicPacketType.ONE_RTT,
                Epoch.ONE_RTT, bytes(len(srv.router.conns)), 1, np.asarray(self.rows, np.uint32).tobytes(),
                np.asarray(taken, np.uint32).tobytes(), L.A_NEED_TOKEN)
        if not reply:
            return _crypto.receive_accept(*args)
        if addr is None:
            addr = b"".join(R.packed_addr(self.addrs[i]) for i in self.cand)
        return _crypto.receive_accept_reply(*args, tokens.table if table is None else table, addr, rnd, ctr0,
                                            np.asarray(versions, np.uint32).tobytes(), flags)


def counters():
    from aioquic_amd import _crypto

    return (_crypto.route_reply_launches(), _crypto.route_accept_launches(), _crypto.route_walk_launches())


def test_fused_form_builds_the_replies(dev, monkeypatch):
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd import receive as RX
    from aioquic_amd.buffer import Buffer
    from aioquic_amd.packet import QuicPacketType, get_retry_integrity_tag, pull_quic_header

    f = Flood(monkeypatch)
    RX.receive_routed(f.srv.router, f.datagrams)  # the known connections' keys get their slots
    tokens = tokens_of()
    n_acc = len(f.cand)
    assert n_acc == 11
    taken = f.srv.slots.reserve(2 * n_acc)
    rnd = np.random.default_rng(5).bytes(16 * n_acc)
    ctr0 = 7 << 32
    flags = L.RP_VN | L.RP_RETRY
    before = counters()
    route, walked, longs, found, sent = f.call(taken, tokens, rnd, ctr0, flags)
    assert counters() == (before[0] + 1, before[1] + 1, before[2] + 1)
    rbuf, rrec = sent[0], np.frombuffer(sent[1], L.REPLY)
    acc = np.frombuffer(found[0], L.ACCEPT)
    want = f.expected(rnd, ctr0, flags)
    retries = vns = 0
    families = set()
    for a, i in enumerate(f.cand):
        region, rec, st = want[a]
        assert int(acc["status"][a]) == st, (a, i)
        assert rbuf[a * R.STRIDE:(a + 1) * R.STRIDE] == region, (a, i)
        assert rrec[a:a + 1].tobytes() == rec.tobytes(), (a, i)
        d = f.datagrams[i]
        packet = R.reply_bytes(region, rec, a * R.STRIDE)
        if d in f.tokenless:
            assert int(rec["kind"][0]) == L.RP_KIND_RETRY
            retries += 1
            families.add(":" in f.addrs[i][0])
            version = int.from_bytes(d[1:5], "big")
            odcid, cscid = d[6:6 + d[5]], SCID
            h = pull_quic_header(Buffer(data=packet), host_cid_length=8)
            assert (h.packet_type, h.version, h.destination_cid) == (QuicPacketType.RETRY, version, cscid)
            assert h.source_cid == rnd[16 * a:16 * a + 8] and h.integrity_tag == packet[-16:]
            assert get_retry_integrity_tag(packet[:-16], odcid, version) == packet[-16:]
            assert tokens.validate_token(f.addrs[i], h.token) == (odcid, h.source_cid)
            assert tokens.seal(ctr0 + a, f.addrs[i], odcid, h.source_cid) == h.token
            assert tokens_of(ctr0 + a).create_token(f.addrs[i], odcid, h.source_cid) == h.token
            with pytest.raises(ValueError):
                tokens.validate_token(addr_of(i + 2), h.token)
            with pytest.raises(ValueError):
                tokens.validate_token((f.addrs[i][0], f.addrs[i][1] + 1), h.token)
            if retries <= 2:
                for k in range(len(h.token)):
                    bad = h.token[:k] + bytes([h.token[k] ^ 0x01]) + h.token[k + 1:]
                    with pytest.raises(ValueError):
                        tokens.validate_token(f.addrs[i], bad)
        elif d in f.grease:
            assert int(rec["kind"][0]) == L.RP_KIND_VN
            vns += 1
            h = pull_quic_header(Buffer(data=packet), host_cid_length=8)
            assert h.packet_type == QuicPacketType.VERSION_NEGOTIATION and h.supported_versions == VERSIONS
            dl = d[5]
            assert (h.source_cid, h.destination_cid) == (d[6:6 + dl], d[7 + dl:7 + dl + d[6 + dl]])
        else:
            assert int(rec["kind"][0]) == L.RP_KIND_NONE and packet == b""
    assert (retries, vns) == (5, 3) and families == {False, True}
    assert int(acc["status"][f.cand.index(f.datagrams.index(f.with_token))]) == L.ACC_OK

    # no reply flag: qpp_session_accept_unprotect, byte for byte
    before = counters()
    plain = f.call(taken, tokens, rnd, ctr0, 0, reply=False)
    quiet = f.call(taken, tokens, rnd, ctr0, 0)
    assert counters() == (before[0], before[1] + 2, before[2] + 2)
    assert quiet[:4] == plain
    assert quiet[4] == (bytes(R.STRIDE * n_acc), bytes(8 * n_acc))
    again = f.call(taken, tokens, rnd, ctr0, flags)
    assert again[:4] == plain and again[4] == sent, "the replies change nothing else, and are the same bytes again"

    # bad arguments: refused before anything is launched
    before = counters()
    ok_addr = b"".join(R.packed_addr(f.addrs[i]) for i in f.cand)
    for kw in (dict(addr=ok_addr[:40] + bytes([5]) + ok_addr[41:]), dict(table=_crypto.KeyTable(2)),
               dict(versions=list(range(1, 18))), dict(versions=[]), dict(ctr0=(1 << 64) - n_acc + 1),
               dict(flags=4)):
        args = dict(ctr0=ctr0, flags=flags)
        args.update(kw)
        with pytest.raises(ValueError):
            f.call(taken, tokens, rnd, args.pop("ctr0"), args.pop("flags"), **args)
    assert counters() == before, "a refused call launched"
    # a reply table without the token key: every Retry's seal reports QPP_S_NO_KEY, and the Retry is
    # not sent with an open token: kind none, that status; the Version Negotiation packets are as before
    half = _crypto.KeyTable(3)
    half.set(tokens.key_records()[:2].tobytes())
    down = np.frombuffer(f.call(taken, tokens, rnd, ctr0, flags, table=half)[4][1], L.REPLY)
    for a in range(n_acc):
        if int(want[a][1]["kind"][0]) == L.RP_KIND_RETRY:
            assert (int(down["kind"][a]), int(down["len"][a]), int(down["status"][a])) == (L.RP_KIND_NONE, 0, L.S_NO_KEY)
        else:
            assert down[a:a + 1].tobytes() == want[a][1].tobytes()
    # Version Negotiation alone needs no addresses, and a counter that would wrap is not looked at
    only_vn = f.call(taken, tokens, rnd, (1 << 64) - 1, L.RP_VN, addr=b"")
    kinds = np.frombuffer(only_vn[4][1], L.REPLY)["kind"]
    assert sorted(kinds.tolist()) == [L.RP_KIND_NONE] * 8 + [L.RP_KIND_VN] * 3
    f.srv.slots.give_back(taken)
    f.srv.slots.close()


# ------------------------------------------------------------ answer_routed --

def test_answer_routed_against_the_long_way(dev, monkeypatch):
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd import receive as RX
    from aioquic_amd.buffer import Buffer
    from aioquic_amd.packet import QuicPacketType, get_retry_integrity_tag, pull_quic_header

    state = {"rng": np.random.default_rng(77), "log": []}

    def fake_urandom(n):
        state["log"].append(state["rng"].bytes(n))
        return state["log"][-1]

    monkeypatch.setattr(RX.os, "urandom", fake_urandom)

    def server_accept(tokens, addrs, seen):
        def accept(header, i):
            try:
                seen.append((i, tokens.validate_token(addrs[i], header.token)))
            except ValueError:
                seen.append((i, None))
                return None
            return new_conn()
        return accept

    # the device's way
    f = Flood(monkeypatch)
    tokens, seen = tokens_of(100), []
    before = counters()
    recs, unrouted, accepted, replies = RX.answer_routed(f.srv.router, f.datagrams, f.addrs,
                                                         server_accept(tokens, f.addrs, seen), tokens=tokens)
    assert counters() == (before[0] + 1, before[1] + 1, before[2] + 1)
    rnd = state["log"][-1]
    assert len(rnd) == 16 * len(f.cand)
    # the long way: accept_routed in Retry mode, then every reply built on the host
    g = Flood(monkeypatch)
    assert g.datagrams == f.datagrams and g.cand == f.cand
    g_tokens, g_seen = tokens_of(100), []
    g_recs, g_unrouted, g_accepted = RX.accept_routed(g.srv.router, g.datagrams,
                                                      server_accept(g_tokens, g.addrs, g_seen), need_token=True)
    ctr0 = g_tokens.take(len(g.cand))
    g_replies = []
    for a, i in enumerate(g.cand):
        d = g.datagrams[i]
        try:
            h = pull_quic_header(Buffer(data=d), host_cid_length=8)
        except ValueError:
            continue
        if h.packet_type != QuicPacketType.INITIAL:
            continue
        if h.version not in VERSIONS:
            g_replies.append((i, R.encode_vn(rnd[16 * a + 8] & 0x7F, h.destination_cid, h.source_cid, VERSIONS)))
        elif len(d) >= 1200 and not h.token:
            scid = rnd[16 * a:16 * a + 8]
            token = g_tokens.seal(ctr0 + a, g.addrs[i], h.destination_cid, scid)
            pkt = R.encode_retry_without_tag(h.version, scid, h.source_cid, token)
            g_replies.append((i, pkt + get_retry_integrity_tag(pkt, h.destination_cid, h.version)))
    assert replies == g_replies and len(replies) == 8
    assert [i for i, _ in replies] == sorted(i for i, _ in replies), "in datagram order"
    replied = {i for i, _ in replies}
    assert unrouted == [u for u in g_unrouted if u[0] not in replied] and len(unrouted) == len(g_unrouted) - 8
    assert {f.datagrams.index(d) for d in (f.small, f.handshake, f.with_token)} <= {i for i, _ in unrouted}
    assert [_record_tuple(r) for r in recs] == [_record_tuple(r) for r in g_recs]
    assert accepted == g_accepted == [] and seen == g_seen == [(f.datagrams.index(f.with_token), None)]

    # the clients come back: the Retry's source CID as DCID, its token in the Initial
    retries = [(i, pull_quic_header(Buffer(data=p), host_cid_length=8)) for i, p in replies
               if f.datagrams[i] in f.tokenless]
    assert len(retries) == 5
    back = [initial_with_token(h.source_cid, h.version, h.token) for _, h in retries]
    batch2 = list(back)
    addrs2 = [f.addrs[i] for i, _ in retries]
    seen2 = []
    recs2, unrouted2, accepted2, replies2 = RX.answer_routed(f.srv.router, batch2, addrs2,
                                                             server_accept(tokens, addrs2, seen2), tokens=tokens)
    assert replies2 == [] and unrouted2 == [] and [i for i, _ in accepted2] == list(range(5))
    assert seen2 == [(k, (f.datagrams[i][6:6 + f.datagrams[i][5]], h.source_cid)) for k, (i, h) in enumerate(retries)]
    assert [(r.datagram, r.packet_number, r.dropped) for r in recs2] == [(k, 0, None) for k in range(5)]

    # a second flood: the counters go on where the first call's ended
    first = sorted(int.from_bytes(h.token[:8], "big") for _, h in retries)
    h2 = Flood(monkeypatch)
    more = RX.answer_routed(h2.srv.router, h2.datagrams, h2.addrs, lambda hd, i: None, tokens=tokens)[3]
    second = sorted(int.from_bytes(pull_quic_header(Buffer(data=p), host_cid_length=8).token[:8], "big")
                    for i, p in more if h2.datagrams[i] in h2.tokenless)
    assert len(second) == 5 and first[0] >= 100 and first[-1] < second[0] and len(set(first + second)) == 10

    # a server not in Retry mode: Version Negotiation only, and the token-less Initials are accepted
    v = Flood(monkeypatch)
    made = []
    out = RX.answer_routed(v.srv.router, v.datagrams, v.addrs, lambda hd, i: made.append(new_conn()) or made[-1])
    assert len(out[3]) == 3 and all(v.datagrams[i] in v.grease for i, _ in out[3])
    assert len(out[2]) == 6, "five without a token and the one with"
    for s in (f, g, h2, v):
        s.srv.slots.close()
