"""GPU checks of the Retry tokens validated on the device (include/quic_pp.h:
qpp_route_token, qpp_route_accept_tokens, qpp_session_serve_unprotect) and of
receive.serve_routed.

The reference is the restatement of tests/token_cases.py -- retry.py's
validate_token and the varint rules in Python, with the C oracle's
AES-128-GCM for the launch that opens the tokens -- and, for serve_routed,
answer_routed in Retry mode with RetryTokens.validate_token in the callback."""

from __future__ import annotations

import numpy as np
import pytest

from oracle import oracle as O
from tests import accept_cases as A
from tests import reply_cases as R
from tests import token_cases as T
from tests.test_gpu_accept import Server, _batch, client_initial, new_conn
from tests.test_gpu_reply import CANARY, Fenced, Flood, addr_of, counters, initial_with_token, reply_engine, tokens_of
from tests.test_gpu_route import _record_tuple

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF
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


# ------------------------------------------------------------ device form --

@pytest.mark.parametrize("n_acc", [1, 255, 256, 257])
def test_token_kernels_match_restatement(dev, n_acc):
    """Hand-built route and walk records over synthetic Initials, one datagram
    per candidate at an odd offset: route_token, the unprotect of its
    descriptors, route_accept_tokens."""
    import torch
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L

    datagrams, walks, addrs, kinds = T.synthetic(n_acc)
    need, flags = L.A_NEED_TOKEN, L.F_RFC_PN
    offs, parts, pos = [], [b"\x11"], 1
    for d in datagrams:
        offs.append(pos)
        fill = d + bytes(range(0x10, 0x40))
        fill += b"\x40" * (1 - (pos + len(fill)) % 2)
        parts.append(fill)
        pos += len(fill)
    buf = np.frombuffer(b"".join(parts), np.uint8).copy()
    assert all(o % 2 for o in offs)
    lens = np.asarray([len(d) for d in datagrams], np.uint32)
    walk = np.zeros((n_acc, L.WALK_MAX), L.WALK)
    walk["desc"] = NONE
    for f in T.C.FIELDS:
        walk[f][:, 0] = [w[f] for w in walks]
    route = np.zeros(n_acc, L.ROUTE)
    route["conn"], route["cls"] = NONE, L.R_LONG
    idx = np.arange(n_acc, dtype=np.uint32)
    slots = (3 + np.arange(2 * n_acc)).astype(np.uint32)
    slots[3::8] = NONE
    addr20 = [R.packed_addr(a) for a in addrs]
    desc0 = np.zeros(n_acc, L.DESC)
    desc0["in_off"] = desc0["out_off"] = offs
    desc0["flags"], desc0["slot"] = flags, NONE

    # the restatement: the descriptors, the launch, the verdicts, the records
    want_tdesc, want_pre, want_trec, want_ini, want_acc, want_res = [], [], [], [], [], []
    want_desc = desc0.copy()
    for a in range(n_acc):
        st = A.restate_status(T.LONG_NONE, [walks[a]], len(datagrams[a]), need)
        d, pre = T.restate_desc(a, st, need, walks[a], offs[a], datagrams[a])
        status, opened = T.restate_open(d, offs[a], datagrams[a])
        trec = T.restate_check(pre, status, walks[a]["token_len"], opened, addr20[a])
        ini, pd, acc, trec = T.restate_accept(datagrams[a], a, offs[a], T.LONG_NONE, [walks[a]], int(slots[2 * a]),
                                              int(slots[2 * a + 1]), need, flags, trec)
        if pd is not None:
            want_desc[a:a + 1] = pd
        want_tdesc.append(d), want_pre.append(T.token_rec(pre)), want_trec.append(trec)
        want_ini.append(ini), want_acc.append(acc), want_res.append(status)
    want_trec, want_acc = np.concatenate(want_trec), np.concatenate(want_acc)
    ok = want_acc["status"] == L.ACC_OK
    assert (want_trec["status"][ok] == L.TK_OK).all()
    if n_acc >= 255:
        assert set(want_trec["status"].tolist()) == T.ALL_TK
        assert {L.ACC_OK, L.ACC_BAD_TOKEN, L.ACC_NO_TOKEN, L.ACC_VERSION} == set(want_acc["status"].tolist())
        assert set(kinds) == set(T.KINDS)
        for kind in ("v4", "v6", "varint2", "varint4"):
            assert all(int(want_acc["status"][a]) == L.ACC_OK for a in range(n_acc) if kinds[a] == kind), kind
        for kind in set(T.KINDS) - {"v4", "v6", "varint2", "varint4"}:
            assert all(int(want_acc["status"][a]) != L.ACC_OK for a in range(n_acc) if kinds[a] == kind), kind
    else:
        assert int(want_acc["status"][0]) == L.ACC_OK

    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_in, d_off, d_len, d_idx = t(buf), t(np.asarray(offs, np.uint64)), t(lens), t(idx)
    d_walk, d_walk_n, d_route = t(walk), t(np.ones(n_acc, np.uint32)), t(route)
    d_slots, d_addr = t(slots), t(np.frombuffer(b"".join(addr20), np.uint8))
    tdesc, trec, tok = Fenced(dev, n_acc * 40), Fenced(dev, n_acc * 48), Fenced(dev, n_acc * L.TOKEN_STRIDE)
    tres, ini, acc = Fenced(dev, n_acc * 16), Fenced(dev, n_acc * 32), Fenced(dev, n_acc * 8)
    desc = Fenced(dev, n_acc * 40)
    tok.t.zero_()
    desc.t.copy_(t(desc0))
    eng = reply_engine()
    before = (_crypto.route_token_launches(), _crypto.route_accept_launches())
    eng.route_token(d_off, d_len, n_acc, d_in, d_route, d_idx, n_acc, d_walk, d_walk_n, d_idx, 0, tdesc.t, trec.t)
    eng.route_accept_tokens(d_off, d_len, n_acc, d_in, d_route, d_idx, n_acc, d_walk, d_walk_n, d_idx, d_slots, 0,
                            d_addr, tok.t, tres.t, ini.t, desc.t, acc.t, trec.t, flags=flags)
    torch.cuda.synchronize()
    assert (_crypto.route_token_launches(), _crypto.route_accept_launches()) == before, "no candidates: no launch"
    assert (tdesc.read() == CANARY).all() and (trec.read() == CANARY).all() and (acc.read() == CANARY).all()

    eng.route_token(d_off, d_len, n_acc, d_in, d_route, d_idx, n_acc, d_walk, d_walk_n, d_idx, n_acc, tdesc.t, trec.t)
    torch.cuda.synchronize()
    assert _crypto.route_token_launches() == before[0] + 1
    assert tdesc.read().tobytes() == np.concatenate(want_tdesc).tobytes()
    assert trec.read().tobytes() == np.concatenate(want_pre).tobytes()
    assert (tok.read() == 0).all()

    eng.unprotect(tdesc.t, n_acc, d_in, tok.t, tres.t)
    torch.cuda.synchronize()
    got_res = tres.read().view(L.RESULT)
    assert got_res["status"].tolist() == want_res
    tok.read()

    eng.route_accept_tokens(d_off, d_len, n_acc, d_in, d_route, d_idx, n_acc, d_walk, d_walk_n, d_idx, d_slots, n_acc,
                            d_addr, tok.t, tres.t, ini.t, desc.t, acc.t, trec.t, flags=flags)
    torch.cuda.synchronize()
    assert (_crypto.route_token_launches(), _crypto.route_accept_launches()) == (before[0] + 1, before[1] + 1)
    assert trec.read().tobytes() == want_trec.tobytes()
    assert acc.read().tobytes() == want_acc.tobytes()
    assert ini.read().tobytes() == np.concatenate(want_ini).tobytes()
    assert desc.read().tobytes() == want_desc.tobytes()
    assert tdesc.read().tobytes() == np.concatenate(want_tdesc).tobytes()
    assert d_in.cpu().numpy().tobytes() == buf.tobytes(), "the datagram buffer is only read"
    assert d_walk.cpu().numpy().tobytes() == walk.tobytes() and d_route.cpu().numpy().tobytes() == route.tobytes()
    # nothing for a rejected candidate: no slot, no CID, the inert descriptor kept
    got_ini = ini.read().view(L.INITIAL)
    assert (got_ini["slot_client"][~ok] == NONE).all() and (got_ini["cid_len"][~ok] == 0).all()
    assert desc.read().view(L.DESC)[~ok].tobytes() == desc0[~ok].tobytes()


def test_token_kernels_reject_bad_arguments(dev):
    import torch
    from aioquic_amd import _crypto
    from aioquic_amd.batch import PacketEngine

    eng = PacketEngine(4)
    z = torch.zeros(512, dtype=torch.uint8, device=dev)
    before = (_crypto.route_token_launches(), _crypto.route_accept_launches())
    with pytest.raises(ValueError):
        eng.route_token(z, z, 1, z, z, z, 1, z, z, z, 1, z, z, accept_flags=3)
    with pytest.raises(ValueError):
        eng.route_accept_tokens(z, z, 1, z, z, z, 1, z, z, z, z, 1, z, z, z, z, z, z, z, accept_flags=2)
    p = z.data_ptr()
    with pytest.raises(ValueError):
        _crypto.route_token(p, p, 1, p, p, p, 1, p, p, p, 1, 1, 0, p, 0)
    with pytest.raises(ValueError):
        _crypto.route_accept_tokens(p, p, 1, p, p, p, 1, p, p, p, p, 1, 1, 0, 0, p, p, p, p, p, p, 0)
    assert (_crypto.route_token_launches(), _crypto.route_accept_launches()) == before


# -------------------------------------------------------------- fused form --

def serve_call(f, taken, table, rnd, ctr0, *, accept_flags=None, reply_flags=None, addr=None, reply=False):
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd import receive as RX
    from aioquic_amd.packet import QuicPacketType
    from aioquic_amd.tls import Epoch

    srv = f.srv
    _, _, _, arrays, _ = RX._routed_arrays(srv.router, f.datagrams, False)
    if addr is None:
        addr = b"".join(R.packed_addr(f.addrs[i]) for i in f.cand)
    args = (srv.slots.table, srv.router.map, 8, f.datagrams, *arrays, RX.ReceivedPacket, QuicPacketType.ONE_RTT,
            Epoch.ONE_RTT, bytes(len(srv.router.conns)), 1, np.asarray(f.rows, np.uint32).tobytes(),
            np.asarray(taken, np.uint32).tobytes(), L.A_NEED_TOKEN if accept_flags is None else accept_flags,
            table, addr, rnd, ctr0, np.asarray(VERSIONS, np.uint32).tobytes(),
            L.RP_VN | L.RP_RETRY if reply_flags is None else reply_flags)
    return (_crypto.receive_accept_reply if reply else _crypto.receive_serve)(*args)


def test_fused_form_and_its_refusals(dev, monkeypatch):
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd import receive as RX

    f = Flood(monkeypatch)
    RX.receive_routed(f.srv.router, f.datagrams)  # the known connections' keys get their slots
    tokens = tokens_of()
    n_acc = len(f.cand)
    taken = f.srv.slots.reserve(2 * n_acc)
    rnd = np.random.default_rng(6).bytes(16 * n_acc)
    ctr0 = 9 << 32
    every = lambda: counters() + (_crypto.route_token_launches(),)

    # refused before anything is launched
    before = every()
    for kw in (dict(addr=b""), dict(accept_flags=0), dict(reply_flags=L.RP_VN), dict(reply_flags=0),
               dict(table=_crypto.KeyTable(2))):
        with pytest.raises(ValueError):
            serve_call(f, taken, kw.pop("table", tokens.table), rnd, ctr0, **kw)
    assert every() == before, "a refused call launched"

    # the token that is not ours is never accepted; everything else is the reply form's
    route, _, longs, found, sent, trec_b = serve_call(f, taken, tokens.table, rnd, ctr0)
    assert every() == (before[0] + 1, before[1] + 1, before[2] + 1, before[3] + 1)
    plain = serve_call(f, taken, tokens.table, rnd, ctr0, reply=True)
    acc, p_acc = np.frombuffer(found[0], L.ACCEPT), np.frombuffer(plain[3][0], L.ACCEPT)
    trec = np.frombuffer(trec_b, L.TOKEN_REC)
    a = f.cand.index(f.datagrams.index(f.with_token))
    assert int(p_acc["status"][a]) == L.ACC_OK and int(acc["status"][a]) == L.ACC_BAD_TOKEN
    assert int(acc["desc"][a]) == NONE and int(trec["status"][a]) == L.TK_LENGTH
    rest = np.arange(n_acc) != a
    assert acc[rest].tobytes() == p_acc[rest].tobytes() and (trec["status"][rest] == L.TK_NONE).all()
    assert not trec["odcid"].any() and not trec["rscid"].any()
    assert sent == plain[4] and route == plain[0], "the replies and the routes are the reply form's"
    km = np.frombuffer(found[1], L.KEY_MATERIAL)
    assert (km["slot"][2 * a:2 * a + 2] == NONE).all(), "derived, never installed"
    i = f.datagrams.index(f.with_token)
    res, p_res = np.frombuffer(longs[4], L.RESULT), np.frombuffer(plain[2][4], L.RESULT)
    assert int(p_res["status"][i]) == L.S_OK and int(res["status"][i]) == L.S_NO_KEY, "and never unprotected"
    others = np.arange(len(res)) != i
    assert res[others].tobytes() == p_res[others].tobytes()
    f.srv.slots.give_back(taken)
    f.srv.slots.close()


# ------------------------------------------------------------ serve_routed --

def one_version_conn(version: int):
    """A server connection that speaks one version: two key slots, not four."""
    from aioquic_amd.tls import Epoch

    c = new_conn()
    c.cryptos_initial = {version: c.cryptos_initial[version]}
    c.cryptos[Epoch.INITIAL] = c.cryptos_initial[version]
    c.supported_versions = [version]
    return c


def both_flights(monkeypatch, serve: bool):
    """A Retry-mode server through two flights: token-less Initials answered
    with Retries (answer_routed), then the clients' second Initials among known
    traffic, new token-less Initials and an odd version -- through
    serve_routed, or through answer_routed with validate_token in the
    callback."""
    from aioquic_amd import _crypto
    from aioquic_amd import receive as RX
    from aioquic_amd.buffer import Buffer
    from aioquic_amd.packet import pull_quic_header
    from aioquic_amd.retry import RetryTokens

    rng = np.random.default_rng(41)
    monkeypatch.setattr(RX.os, "urandom", lambda n: rng.bytes(n))
    srv = Server(monkeypatch)
    known = [d for _, d in srv.items][:12]
    RX.receive_routed(srv.router, known)  # every known key has its slot
    tokens, other = tokens_of(500), RetryTokens(T.OTHER_KEY, R.TOKEN_IV, counter=500)
    dcids = [bytes([0x90 + k]) * (4 + k) for k in range(10)]
    firsts = [client_initial(d, VERSIONS[k % 2], fill=k)[0] for k, d in enumerate(dcids)]
    addrs1 = [addr_of(k) for k in range(10)]
    _, _, accepted, replies = RX.answer_routed(srv.router, firsts, addrs1, lambda *a: pytest.fail("no token yet"),
                                               tokens=tokens)
    assert accepted == [] and [i for i, _ in replies] == list(range(10))
    heads = [pull_quic_header(Buffer(data=p), host_cid_length=8) for _, p in replies]
    back = lambda k, token=None: initial_with_token(heads[k].source_cid, heads[k].version,
                                                    heads[k].token if token is None else token)
    flip = lambda t, at: t[:at] + bytes([t[at] ^ 0x20]) + t[at + 1:]
    second = [(back(k), addrs1[k], "honest") for k in range(5)]
    second.append((back(5), addr_of(77, v6=":" not in addrs1[5][0]), "replayed"))
    second.append((back(6, flip(heads[6].token, 12)), addrs1[6], "tampered"))
    second.append((back(7, flip(heads[7].token, len(heads[7].token) - 1)), addrs1[7], "tampered"))
    second.append((back(8, other.create_token(addrs1[8], dcids[8], heads[8].source_cid)), addrs1[8], "other-key"))
    second.append((back(9), addrs1[9], "honest"))
    second.append((client_initial(b"\xEA" * 8, R.V1, fill=3)[0], addr_of(31), "tokenless"))
    second.append((client_initial(b"\xEB" * 5, R.V2, fill=4)[0], addr_of(32), "tokenless"))
    second.append((A.initial(R.GREASE, b"\xEC" * 8, 1200), addr_of(33), "grease"))
    batch = _batch(srv, [d for d, _, _ in second], limit=12)
    assert len(batch) == 25
    by = {d: (addr, kind) for d, addr, kind in second}
    addrs = [by.get(d, (("192.0.2.1", 9), "known"))[0] for d in batch]
    kinds = [by.get(d, (None, "known"))[1] for d in batch]
    first_of = {batch.index(back(k)): k for k in (0, 1, 2, 3, 4, 5, 9)}
    seen, refused = [], []
    room = srv.slots.room()
    launches = _crypto.route_token_launches()
    if serve:
        def accept(header, i, odcid, rscid):
            seen.append((i, odcid, rscid))
            return one_version_conn(header.version)

        recs, unrouted, accepted, replies2, dropped = RX.serve_routed(srv.router, batch, addrs, accept, tokens=tokens)
        assert _crypto.route_token_launches() == launches + 1
    else:
        def accept(header, i):
            try:
                cids = tokens.validate_token(addrs[i], header.token)
            except ValueError:
                refused.append(i)
                return None
            seen.append((i,) + cids)
            return one_version_conn(header.version)

        recs, unrouted, accepted, replies2 = RX.answer_routed(srv.router, batch, addrs, accept, tokens=tokens)
        dropped = None
        assert _crypto.route_token_launches() == launches
    return dict(srv=srv, tokens=tokens, batch=batch, addrs=addrs, kinds=kinds, dcids=dcids, heads=heads,
                first_of=first_of, seen=seen, refused=refused, room=room, recs=recs, unrouted=unrouted,
                accepted=accepted, replies=replies2, dropped=dropped)


def test_serve_routed_round_trip(dev, monkeypatch):
    from aioquic_amd import layout as L
    from aioquic_amd.buffer import Buffer
    from aioquic_amd.packet import QuicPacketType, pull_quic_header

    s = both_flights(monkeypatch, True)
    h = both_flights(monkeypatch, False)
    assert s["batch"] == h["batch"] and s["addrs"] == h["addrs"]
    batch, kinds, tokens = s["batch"], s["kinds"], s["tokens"]
    where = lambda kind: [i for i, k in enumerate(kinds) if k == kind]
    # the honest ones: accepted, the callback given the first flight's DCID and the Retry's SCID
    assert [i for i, _ in s["accepted"]] == where("honest") and len(s["accepted"]) == 6
    assert s["seen"] == [(i, s["dcids"][s["first_of"][i]], s["heads"][s["first_of"][i]].source_cid)
                         for i in where("honest")]
    assert s["seen"] == h["seen"], "what host validate_token returns"
    versions = set()
    for i, conn in s["accepted"]:
        v = int.from_bytes(batch[i][1:5], "big")
        versions.add(v)
        dcid = batch[i][6:6 + batch[i][5]]
        assert dcid == s["heads"][s["first_of"][i]].source_cid
        pair = conn.cryptos_initial[v]
        assert (pair.recv.secret, pair.send.secret) == O.initial_secrets(dcid, v)
        assert (id(pair.recv.aead), id(pair.recv.hp), 0) in s["srv"].slots._slot
        assert s["srv"].router.index_of(dcid) is not None
    assert versions == set(VERSIONS)
    # packet 0 of each, and every other record, as with host validation in the callback
    assert [_record_tuple(r) for r in s["recs"]] == [_record_tuple(r) for r in h["recs"]]
    firsts = {r.datagram: r for r in s["recs"] if r.offset == 0}
    for i in where("honest"):
        assert (firsts[i].packet_number, firsts[i].dropped) == (0, None)
        assert firsts[i].plain_payload[:4] == b"\x06\x00\x40\x10"
    # the others: dropped with the reason, never handed to the callback, in neither list
    reasons = dict(s["dropped"])
    assert sorted(reasons) == sorted(where("replayed") + where("tampered") + where("other-key")) == sorted(h["refused"])
    assert [reasons[i] for i in where("replayed")] == [L.TK_ADDR]
    assert [reasons[i] for i in where("tampered") + where("other-key")] == [L.TK_AUTH] * 3
    assert [i for i, _ in s["dropped"]] == sorted(reasons), "in datagram order"
    for i in reasons:
        token = pull_quic_header(Buffer(data=batch[i]), host_cid_length=8).token
        with pytest.raises(ValueError):
            tokens.validate_token(s["addrs"][i], token)
        assert not [r for r in s["recs"] if r.datagram == i]
    for i, odcid, rscid in s["seen"]:
        token = pull_quic_header(Buffer(data=batch[i]), host_cid_length=8).token
        assert tokens.validate_token(s["addrs"][i], token) == (odcid, rscid)
    gone = set(reasons) | {i for i, _ in s["replies"]}
    assert not gone & {i for i, _ in s["unrouted"]}
    assert s["unrouted"] == [u for u in h["unrouted"] if u[0] not in reasons]
    # their slots are free again: two per accepted connection, none for a dropped one
    assert s["srv"].slots.room() == s["room"] - 2 * len(s["accepted"])
    assert h["srv"].slots.room() == h["room"] - 2 * len(h["accepted"])
    # token-less Initials and the odd version are answered in the same call
    assert s["replies"] == h["replies"] and [i for i, _ in s["replies"]] == sorted(where("tokenless") + where("grease"))
    types = {i: pull_quic_header(Buffer(data=p), host_cid_length=8).packet_type for i, p in s["replies"]}
    assert [types[i] for i in where("tokenless")] == [QuicPacketType.RETRY] * 2
    assert [types[i] for i in where("grease")] == [QuicPacketType.VERSION_NEGOTIATION]
    s["srv"].slots.close(), h["srv"].slots.close()


def test_serve_routed_needs_tokens_and_falls_back(dev, monkeypatch):
    from aioquic_amd import receive as RX

    srv = Server(monkeypatch)
    known = [d for _, d in srv.items][:12]
    with pytest.raises(ValueError):
        RX.serve_routed(srv.router, known, [("192.0.2.1", 9)] * 12, None, tokens=None)
    # no candidate: receive_routed, with nothing accepted, answered or dropped
    twin = Server(monkeypatch)
    want = RX.receive_routed(twin.router, known)
    recs, unrouted, accepted, replies, dropped = RX.serve_routed(srv.router, known, [("192.0.2.1", 9)] * 12,
                                                                 lambda *a: pytest.fail("no candidate"),
                                                                 tokens=tokens_of())
    assert [_record_tuple(r) for r in recs] == [_record_tuple(r) for r in want[0]] and unrouted == want[1]
    assert (accepted, replies, dropped) == ([], [], [])
    srv.slots.close(), twin.slots.close()
