"""GPU parity of the batched Initial key derivation (qpp_keytab_derive_initial,
SURVEY.md sec. 8(a) row a12 and 8(f) row 4): the device's HKDF-Extract /
"client in" / "server in" / key-iv-hp chain and the slots it installs against
the RFC 9001 / 9369 Appendix-A vectors and the oracle's stdlib restatement of
quic/crypto.py:201-227, and setup_initial_batch against CryptoPair.setup_initial.
Every comparison is bit-exact."""

import numpy as np
import pytest

from tests.golden_cases import gen_bytes, long_header, short_header

pytestmark = pytest.mark.gpu

V2 = 0x6B3343CF
SHAPES = (1, 31, 32, 33, 200)  # 32 connections fill a 64-lane workgroup; 200 is no multiple


def _quiet():
    from aioquic_amd import _crypto

    assert _crypto.watchdog_count() == 0


def _records(n):
    """n records on a table of 2n slots: CID lengths cycling 0..20, versions
    alternating, every fifth client side and every seventh server side not
    installed (record 34 has neither).  Returns (records, versions)."""
    from aioquic_amd import layout as L

    recs, versions = [], []
    for i in range(n):
        cid = gen_bytes(f"initial-cid-{n}-{i}", i % 21)
        recs.append(L.initial_record(L.SLOT_NONE if i % 5 == 4 else 2 * i,
                                     L.SLOT_NONE if i % 7 == 6 else 2 * i + 1, cid, v2=bool(i & 1)))
        versions.append(V2 if i & 1 else 1)
    return np.concatenate(recs), versions


_WANT: dict = {}


def _oracle_material(oracle, n):
    """What the oracle derives for _records(n): (km (n, 2) KEY_MATERIAL,
    secrets (n, 2, 32)), computed once per n and shared (read-only)."""
    from aioquic_amd import layout as L

    if n not in _WANT:
        recs, versions = _records(n)
        km = np.zeros((n, 2), dtype=L.KEY_MATERIAL)
        sec = np.zeros((n, 2, 32), dtype=np.uint8)
        for i, r in enumerate(recs):
            cid = bytes(r["cid"][: r["cid_len"]])
            for d, secret in enumerate(oracle.initial_secrets(cid, versions[i])):
                key, iv, hp = oracle.derive_key_iv_hp(0, secret, versions[i])
                slot = int(r["slot_server"] if d else r["slot_client"])
                km[i, d] = L.key_material(slot, L.AES_128_GCM, key, iv, hp)[0]
                sec[i, d] = np.frombuffer(secret, dtype=np.uint8)
        km.flags.writeable = sec.flags.writeable = False
        _WANT[n] = (km, sec)
    return _WANT[n]


def _one_desc(length, hdr_len, pn, slot):
    from aioquic_amd import layout as L

    d = np.zeros(1, dtype=L.DESC)
    d["len"], d["hdr_len"], d["pn"], d["slot"] = length, hdr_len, pn, slot
    return d


def _status_on(eng, slot):
    """Status of one small packet protected on `slot`."""
    hdr, payload = short_header(b"\x22" * 8, 7, 2, 0), bytes(range(40))
    _, res = eng.protect_host(_one_desc(len(payload), len(hdr), 7, slot), hdr + payload,
                              len(hdr) + len(payload) + 16)
    return int(res["status"][0])


@pytest.mark.parametrize("tag", ["v1", "v2"])
def test_rfc_vectors(tag):
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine
    from tests.rfc import V1, V2 as RV2

    v = V1 if tag == "v1" else RV2
    eng = PacketEngine(2)
    km, sec = eng.derive_initial_keys(L.initial_record(0, 1, v.cid, v2=tag == "v2"))
    assert km.shape == (1, 2) and km.dtype == L.KEY_MATERIAL
    assert sec.shape == (1, 2, 32) and sec.dtype == np.uint8
    for d, (secret, key, iv, hp) in enumerate((v.derive_client, v.derive_server)):
        assert bytes(sec[0, d]) == secret
        assert km[0, d].tobytes() == L.key_material(d, L.AES_128_GCM, key, iv, hp).tobytes()
    # the client's Initial packet opens on the "client in" slot ...
    pkt, hdr = v.long_client_encrypted_packet, v.long_client_plain_header
    assert len(pkt) == 1200
    pn_len = (hdr[0] & 3) + 1
    out, res = eng.unprotect_host(_one_desc(len(pkt), len(hdr) - pn_len, 0, 0), pkt, len(pkt))
    r = res[0]
    assert r["status"] == L.S_OK and r["pn"] == v.long_client_packet_number
    assert r["hdr_len"] == len(hdr)
    assert out[: len(hdr)].tobytes() == hdr
    assert out[len(hdr): r["out_len"]].tobytes() == v.long_client_plain_payload
    # ... and the server's is sealed on the "server in" slot
    hdr, payload = v.long_server_plain_header, v.long_server_plain_payload
    out, res = eng.protect_host(_one_desc(len(payload), len(hdr), v.long_server_packet_number, 1),
                                hdr + payload, len(hdr) + len(payload) + 16)
    assert res[0]["status"] == L.S_OK and res[0]["out_len"] == 135
    assert out[:135].tobytes() == v.long_server_encrypted_packet
    _quiet()


@pytest.mark.parametrize("n", SHAPES)
def test_shapes_match_oracle_and_protect(oracle, n):
    import torch

    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine, layout_packets

    recs, versions = _records(n)
    want_km, want_sec = _oracle_material(oracle, n)
    eng = PacketEngine(2 * n)
    km, sec = eng.derive_initial_keys(recs)
    # every record and secret, the not-installed ones included
    assert km.shape == (n, 2) and sec.shape == (n, 2, 32)
    assert km.tobytes() == want_km.tobytes()
    assert np.array_equal(sec, want_sec)
    none = km["slot"] == L.SLOT_NONE
    assert none.sum() == n // 5 + n // 7

    # two Initial packets per slot of the table, skipped slots too, against
    # the oracle with its own material (a slot it was not given: S_NO_KEY)
    okeys = np.zeros(2 * n, dtype=oracle.KEY_DTYPE)
    okeys["suite"] = 0xFF
    for rec in want_km.reshape(-1):
        if rec["slot"] != L.SLOT_NONE:
            okeys[int(rec["slot"])] = rec
    rng = np.random.default_rng(900 + n)
    headers, payloads, pns, slots = [], [], [], []
    for s in range(2 * n):
        i = s // 2
        cid = bytes(recs[i]["cid"][: recs[i]["cid_len"]])
        for k in range(2):
            j = len(headers)
            plen = (20, 1200)[j] if j < 2 else int(rng.integers(20, 1201))
            pn_len = 1 + j % 4
            headers.append(long_header(versions[i], cid, gen_bytes(f"scid-{s}", 8 * (s & 1)), b"", j, pn_len,
                                       plen + 16))
            payloads.append(rng.bytes(plen))
            pns.append(j)
            slots.append(s)
    m = len(headers)
    inbuf, desc, size = layout_packets(headers, payloads, pns, slots)
    exp, eres = oracle.protect_batch(okeys, desc, inbuf, size)
    skipped = np.repeat(okeys["suite"] == 0xFF, 2)
    assert skipped.sum() == 2 * none.sum()
    assert (eres["status"][~skipped] == L.S_OK).all() and (eres["status"][skipped] == L.S_NO_KEY).all()
    d_out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    d_res = torch.zeros(m * 16, dtype=torch.uint8, device="cuda")
    eng.protect(torch.from_numpy(desc.view(np.uint8).copy()).cuda(), m, torch.from_numpy(inbuf).cuda(),
                d_out, d_res)
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(L.RESULT)
    assert np.array_equal(res["status"], eres["status"])
    assert np.array_equal(res["out_len"], eres["out_len"])
    assert np.array_equal(d_out.cpu().numpy(), exp)
    _quiet()


def test_neighbour_slots_untouched(oracle):
    from aioquic_amd import layout as L
    from aioquic_amd.batch import KeySpec, PacketEngine

    key, iv, hpk = gen_bytes("nb-key", 32), gen_bytes("nb-iv", 12), gen_bytes("nb-hp", 32)
    eng = PacketEngine(5)
    eng.set_keys([KeySpec(2, L.CHACHA20_POLY1305, key, iv, hpk)])
    hdr, payload = short_header(b"\x33" * 8, 99, 2, 0), gen_bytes("nb-payload", 333)
    desc = _one_desc(len(payload), len(hdr), 99, 2)
    total = len(hdr) + len(payload) + 16
    before, res = eng.protect_host(desc, hdr + payload, total)
    assert res[0]["status"] == L.S_OK
    assert before[:total].tobytes() == oracle.protect(L.CHACHA20_POLY1305, key, iv, hpk, hdr, payload, 99)
    eng.derive_initial_keys(np.concatenate([L.initial_record(1, 3, b"\x01" * 8),
                                            L.initial_record(0, 4, b"\x02" * 20, v2=True)]))
    after, res = eng.protect_host(desc, hdr + payload, total)
    assert res[0]["status"] == L.S_OK
    assert np.array_equal(before, after)
    for s in (0, 1, 3, 4):
        assert _status_on(eng, s) == L.S_OK
    _quiet()


def test_rejections_install_nothing():
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    eng = PacketEngine(4)
    cid = b"\x44" * 8
    good = L.initial_record(2, 3, cid)
    bad = []
    bad.append(L.initial_record(0, 4, cid))            # a slot equal to the capacity
    long_cid = L.initial_record(0, 1, cid)
    long_cid["cid_len"] = 21
    bad.append(long_cid)
    flags = L.initial_record(0, 1, cid)
    flags["flags"] = 2
    bad.append(flags)
    bad.append(L.initial_record(1, 1, cid))            # both directions in one slot
    for rec in bad:
        with pytest.raises(ValueError):
            eng.derive_initial_keys(rec)
        # a good record in front of the bad one is not installed either
        with pytest.raises(ValueError):
            eng.derive_initial_keys(np.concatenate([good, rec]))
    with pytest.raises(ValueError):
        eng.table.derive_initial(bytes(33))
    for s in range(4):
        assert _status_on(eng, s) == L.S_NO_KEY
    km, sec = eng.derive_initial_keys(np.zeros(0, dtype=L.INITIAL))
    assert km.shape == (0, 2) and km.dtype == L.KEY_MATERIAL
    assert sec.shape == (0, 2, 32) and sec.dtype == np.uint8
    assert eng.table.derive_initial(b"") == (b"", b"")
    # the table still takes keys after all that
    eng.derive_initial_keys(good)
    assert [_status_on(eng, s) for s in range(4)] == [L.S_NO_KEY, L.S_NO_KEY, L.S_OK, L.S_OK]
    _quiet()


def test_derive_trace_reports_both_kernels():
    """The diagnostic tools/bench_initial_keys.py reads: nothing before a timed
    call, then the two kernels' durations of the last one."""
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    eng = PacketEngine(8)
    recs = np.concatenate([L.initial_record(2 * i, 2 * i + 1, bytes([i]) * 8) for i in range(4)])
    eng.derive_initial_keys(recs)
    assert eng.table.derive_trace() == (0.0, 0.0)
    assert eng.table.derive_trace(1) == (0.0, 0.0)
    km, _ = eng.derive_initial_keys(recs)
    derive_ms, setup_ms = eng.table.derive_trace(0)
    assert 0 < derive_ms < 1000 and 0 < setup_ms < 1000
    km2, _ = eng.derive_initial_keys(recs)
    assert km2.tobytes() == km.tobytes()
    assert eng.table.derive_trace() == (derive_ms, setup_ms)  # off: the last timed call's stay
    _quiet()


def _ctx_state(ctx):
    return (ctx.secret, ctx.cipher_suite, ctx.version, ctx.key_phase, ctx.aead._material(),
            ctx.hp._material())


def test_setup_initial_batch():
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd.batch_io import KeySlots, ReceiveBatch, SendBatch, setup_initial_batch
    from aioquic_amd.crypto import INITIAL_CIPHER_SUITE, CryptoPair

    log = []

    def pair(k):
        return CryptoPair(recv_setup_cb=lambda t: log.append((k, "recv", t)),
                          send_setup_cb=lambda t: log.append((k, "send", t)))

    # 20 connections, each end a pair: 40 pairs, clients at even positions
    pairs, cids, roles, versions = [], [], [], []
    for c in range(20):
        cid = gen_bytes(f"batch-cid-{c}", (0, 8, 20)[c % 3])
        for is_client in (True, False):
            pairs.append(pair(len(pairs)))
            cids.append(cid)
            roles.append(is_client)
            versions.append(V2 if c % 4 >= 2 else 1)
    ks = KeySlots(128)
    setup_initial_batch(pairs, cids, roles, versions, slots=ks)
    assert log == [(k, d, "tls") for k in range(40) for d in ("recv", "send")]
    assert ks._pending == [] and len(ks._keep) == 80 and len(ks._slot) == 80
    twins = []
    for p, cid, is_client, version in zip(pairs, cids, roles, versions):
        t = CryptoPair()
        t.setup_initial(cid, is_client, version)
        twins.append(t)
        for ctx, tctx in ((p.recv, t.recv), (p.send, t.send)):
            assert _ctx_state(ctx) == _ctx_state(tctx)
            assert ctx.cipher_suite == INITIAL_CIPHER_SUITE and len(ctx.secret) == 32

    # one packet each way per connection through that table; nothing new is installed
    sb = SendBatch(slots=ks)
    meta = []
    for k, p in enumerate(pairs):
        peer = k ^ 1
        plen = (20, 1162, 300)[k % 3]
        hdr = long_header(versions[k], cids[k], b"\x55" * 8, b"", k, 1 + k % 4, plen + 16)
        payload = gen_bytes(f"batch-payload-{k}", plen)
        sb.add(p, hdr, payload, k)
        meta.append((peer, hdr, payload, k, len(hdr) - (1 + k % 4)))
    wires = sb.flush()
    assert ks._pending == [] and len(ks._keep) == 80
    rb = ReceiveBatch(slots=ks)
    for (peer, hdr, payload, pn, off), w in zip(meta, wires):
        rb.add(pairs[peer], w, off, expected_packet_number=pn)
    got = rb.run()
    assert rb.launches == 1 and len(ks._keep) == 80
    for k, ((peer, hdr, payload, pn, off), w, o) in enumerate(zip(meta, wires, got)):
        assert o == (hdr, payload, pn)
        assert twins[k].encrypt_packet(hdr, payload, pn) == w
        assert twins[peer].decrypt_packet(w, off, pn) == (hdr, payload, pn)

    # a pair torn down gives its two slots back, cleared on the device
    mine = sorted(ks._slot[(id(c.aead), id(c.hp), 0)] for c in (pairs[0].recv, pairs[0].send))
    pairs[0].teardown()
    assert len(ks._keep) == 78 and sorted(ks._free) == mine
    for s in mine:
        hdr, payload = short_header(b"\x66" * 8, 1, 2, 0), bytes(40)
        _, res = _crypto.protect_host(ks.table, _one_desc(40, len(hdr), 1, s).tobytes(), hdr + payload,
                                      len(hdr) + 56)
        assert np.frombuffer(res, dtype=L.RESULT)["status"][0] == L.S_NO_KEY

    # 140 slots never fit a table of 128; nothing changes
    more = [CryptoPair() for _ in range(70)]
    with pytest.raises(OverflowError):
        setup_initial_batch(more, [b"\x77" * 8] * 70, False, 1, slots=ks)
    assert len(ks._keep) == 78 and all(not p.send.is_valid() for p in more)
    # 60 more do not fit beside the 78 held: the table is cleared and refilled
    # (KeySlots.assign's rule); one value for all roles and versions
    setup_initial_batch(more[:30], [bytes([k]) * 8 for k in range(30)], False, V2, slots=ks)
    assert len(ks._keep) == 60 and ks._pending == []
    t = CryptoPair()
    t.setup_initial(bytes([29]) * 8, False, V2)
    assert _ctx_state(more[29].send) == _ctx_state(t.send) and _ctx_state(more[29].recv) == _ctx_state(t.recv)
    # the refill left no key behind: the slots held before and not bound again are empty on the
    # device, the ones bound again hold keys (one launch over slots 0..79)
    assert sorted(ks._keep) == list(range(60))
    hdr, payload = short_header(b"\x66" * 8, 1, 2, 0), bytes(40)
    probe = np.zeros(80, dtype=L.DESC)
    probe["in_off"] = probe["out_off"] = 128 * np.arange(80)
    probe["len"], probe["hdr_len"], probe["pn"], probe["slot"] = 40, len(hdr), 1, np.arange(80)
    _, res = _crypto.protect_host(ks.table, probe.tobytes(), (hdr + payload).ljust(128, b"\0") * 80, 128 * 80)
    status = np.frombuffer(res, dtype=L.RESULT)["status"]
    assert (status[:60] == L.S_OK).all() and (status[60:] == L.S_NO_KEY).all()
    with pytest.raises(ValueError):
        setup_initial_batch(more[30:31], [bytes(21)], False, 1, slots=ks)
    ks.close()
    _quiet()
