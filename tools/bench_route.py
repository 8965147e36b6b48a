#!/usr/bin/env python3
"""Routing received datagrams by connection ID on the device (qpp_route), timed
on a GPU box.  One process, one GPU.  Prints one JSON object (and writes it to
--out).

The traffic is n datagrams of 1200 B (short header | 8-byte CID | 2-byte packet
number, the bench workload's packet) over C connections (default 4096, three
suites) in random arrival order, for n = 1 Mi and 64 Ki.

  device   on device buffers, timed with events on the stream, per n:
             k_route                  raw datagrams -> descriptors + route records
             bucket + unprotect       qpp_plan_build + qpp_unprotect_planned of
                                      those descriptors (the launch k_route feeds)
             unprotect alone          the planned launch without the plan build
             k_phase                  (--next-phase) the key-phase resolution between
                                      the two, every lane computing its mask and
                                      none finding an update
  host     from a list of bytes, wall time, per n of --host-sizes:
             receive_routed           one call: stage, route + unprotect, walk
             dict + receive_datagrams a Python routing pass (data[1:9] dict
                                      lookup per datagram, the reference's
                                      asyncio/server.py:60-152 without its header
                                      parse) and receive_datagrams of the items

  burst    --burst n (default 65536, 0 = skip) datagrams of a connect burst over
           the same number of connections, every connection with Initial,
           Handshake and 1-RTT keys: each connection's first datagram a
           coalesced Initial + Handshake + 1-RTT of 1200 B, one in 16 of the
           rest a lone Handshake packet, the rest 1-RTT.  The same two host
           ways: receive_routed (the device walks the long headers in the one
           fused call) against a Python routing pass (DCID dict lookup) and
           receive_datagrams of the items (the header walk in Python).

  --next-phase   also time receive_routed(..., next_phase=True): every keyed
           connection gets a slot for its next key phase and a kernel ahead of
           the unprotect resolves the peers' key updates (qpp_route_phase).
           The host part then alternates three ways and reports what the extra
           kernel and the doubled slots cost a batch without an update
           ("receive_routed_next_phase"), its first call (which builds every
           connection's next-phase context) on its own, and that build timed
           alone.  And a key-update workload (--update n datagrams, default
           65536, over --update-conns connections, default 1024): every
           connection's packets in order, each connection moving to its next
           key phase at its midpoint, through receive_routed with next_phase
           off (every flipped packet and all that follow it go through
           ReceiveBatch), on with the next-phase contexts built inside the
           call ("cold": the first batch after an update) and on with them
           built before ("warm").  Every round starts from the first phase.

The ways alternate in one process after --warmup rounds; median, min and max
of --runs rounds.  Every round starts from the same connection state (expected
packet numbers reset outside the timings).  The two host ways' records are
compared at the end: a mismatch fails the run.
"""

from __future__ import annotations

import argparse
import json
import os
import signal
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4),
            "max_ms": round(max(xs), 4)}


class Space:
    expected_packet_number = 0


def connect_burst(n, C, runs, warmup):
    """The connect-burst mix through both host ways -> (numbers, records equal)."""
    from aioquic_amd import batch_io
    from aioquic_amd import receive as R
    from aioquic_amd.crypto import CryptoPair
    from aioquic_amd.packet import QuicPacketType, QuicProtocolVersion, encode_long_header_first_byte
    from aioquic_amd.route import CidRouter
    from aioquic_amd.tls import CipherSuite, Epoch

    rng = np.random.default_rng(0xB0257)
    version = int(QuicProtocolVersion.VERSION_1)
    suites = [(CipherSuite.AES_128_GCM_SHA256, 32), (CipherSuite.AES_256_GCM_SHA384, 48),
              (CipherSuite.CHACHA20_POLY1305_SHA256, 32)]
    # the burst addresses every connection with all three of its key-sets: either way needs a
    # slot for each in one batch, more than the default table of this thread has
    batch_io._per_thread.slots = batch_io.KeySlots(6 * C)
    cid = rng.integers(0, 256, (C, 8), dtype=np.uint8)
    cid[:, :4] = np.arange(C, dtype=">u4").view(np.uint8).reshape(C, 4)  # distinct
    cids = [cid[c].tobytes() for c in range(C)]
    scid = bytes(8)
    send_slots = batch_io.KeySlots(6 * C)
    srv_init = [CryptoPair() for _ in range(C)]
    cli_init = [CryptoPair() for _ in range(C)]
    batch_io.setup_initial_batch(srv_init, cids, False, version)
    batch_io.setup_initial_batch(cli_init, cids, True, version, slots=send_slots)
    conns, senders = [], []
    for c in range(C):
        cs, slen = suites[c % 3]
        pairs = {}
        snd = {Epoch.INITIAL: cli_init[c].send}
        for epoch, suite, ln in ((Epoch.HANDSHAKE, CipherSuite.AES_128_GCM_SHA256, 32), (Epoch.ONE_RTT, cs, slen)):
            secret = rng.bytes(ln)
            pairs[epoch] = CryptoPair()
            pairs[epoch].recv.setup(cipher_suite=suite, secret=secret, version=version)
            peer = CryptoPair()
            peer.send.setup(cipher_suite=suite, secret=secret, version=version)
            snd[epoch] = peer.send
        pairs[Epoch.INITIAL] = srv_init[c]
        conns.append(R.ConnectionKeys(cryptos=pairs, spaces={e: Space() for e in (Epoch.INITIAL, Epoch.HANDSHAKE,
                                                                                  Epoch.ONE_RTT)},
                                      cryptos_initial={version: srv_init[c]}, host_cid_length=8))
        senders.append(snd)

    def long_hdr(ptype, c, pn, rest):
        out = bytes([encode_long_header_first_byte(version, ptype, 1)]) + version.to_bytes(4, "big")
        out += bytes([8]) + cids[c] + bytes([8]) + scid
        if ptype == QuicPacketType.INITIAL:
            out += b"\x00"
        return out + (0x4000 | (rest + 2)).to_bytes(2, "big") + pn.to_bytes(2, "big")

    def short_hdr(c, pn):
        return bytes([0x41]) + cids[c] + pn.to_bytes(2, "big")

    # per connection: the coalesced first datagram, then its share of the rest
    per = [max(n // C, 1)] * C
    sb = batch_io.SendBatch(slots=send_slots)
    shape = []  # per datagram: (connection, packets in it)
    order = np.repeat(np.arange(C), per)
    rng.shuffle(order)
    seen = [0] * C
    pn = [[0, 0, 0] for _ in range(C)]  # Initial, Handshake, application
    k_rest = 0
    for c in order.tolist():
        first = seen[c] == 0
        seen[c] += 1
        if first:
            hi = long_hdr(QuicPacketType.INITIAL, c, 0, 300 + 16)
            hh = long_hdr(QuicPacketType.HANDSHAKE, c, 0, 200 + 16)
            hs = short_hdr(c, 0)
            sb.add(senders[c][Epoch.INITIAL], hi, rng.bytes(300), 0)
            sb.add(senders[c][Epoch.HANDSHAKE], hh, rng.bytes(200), 0)
            sb.add(senders[c][Epoch.ONE_RTT], hs, rng.bytes(1200 - len(hi) - len(hh) - len(hs) - 300 - 200 - 48), 0)
            pn[c] = [1, 1, 1]
            shape.append((c, 3))
            continue
        k_rest += 1
        if k_rest % 16 == 0:
            h = long_hdr(QuicPacketType.HANDSHAKE, c, pn[c][1], 1200 - 27 - 16 + 16)
            sb.add(senders[c][Epoch.HANDSHAKE], h, rng.bytes(1200 - len(h) - 16), pn[c][1])
            pn[c][1] += 1
        else:
            h = short_hdr(c, pn[c][2])
            sb.add(senders[c][Epoch.ONE_RTT], h, rng.bytes(1200 - len(h) - 16), pn[c][2])
            pn[c][2] += 1
        shape.append((c, 1))
    wires = sb.flush()
    datagrams, at = [], 0
    for c, k in shape:
        datagrams.append(b"".join(wires[at:at + k]))
        at += k
    assert all(len(d) == 1200 for d in datagrams)
    del wires
    router = CidRouter(8, C)
    for c, conn in enumerate(conns):
        router.add(cids[c], conn)
    by_cid = {cids[c]: conn for c, conn in enumerate(conns)}

    def reset():
        for conn in conns:
            for sp in conn.spaces.values():
                sp.expected_packet_number = 0

    t_routed, t_dict, t_pass = [], [], []
    got = want = unrouted = None
    for r in range(warmup + runs):
        reset()
        t0 = time.perf_counter()
        got, unrouted = R.receive_routed(router, datagrams)
        t1 = time.perf_counter()
        reset()
        t2 = time.perf_counter()
        items = [(by_cid[d[6:14] if d[0] & 0x80 else d[1:9]], d) for d in datagrams]
        t3 = time.perf_counter()
        want = R.receive_datagrams(items)
        t4 = time.perf_counter()
        if r >= warmup:
            t_routed.append((t1 - t0) * 1e3)
            t_pass.append((t3 - t2) * 1e3)
            t_dict.append((t4 - t2) * 1e3)
        if r + 1 < warmup + runs:
            del got, want, items
    packets = sum(k for _, k in shape)
    eq = not unrouted and len(got) == len(want) == packets and all(
        g == w_ and g.dropped is None for g, w_ in zip(got, want))
    mr, md = statistics.median(t_routed), statistics.median(t_dict)
    nd = len(datagrams)
    return {
        "datagrams": nd, "packets": packets, "connections": C,
        "coalesced_datagrams": sum(1 for _, k in shape if k == 3),
        "lone_handshake_datagrams": sum(1 for d in datagrams if d[0] & 0x80) - sum(1 for _, k in shape if k == 3),
        "receive_routed": dict(_stats(t_routed), datagrams_per_s=round(nd / (mr * 1e-3))),
        "dict_pass_plus_receive_datagrams": dict(_stats(t_dict), dict_pass=_stats(t_pass),
                                                 datagrams_per_s=round(nd / (md * 1e-3))),
        "dict_way_over_routed": round(md / mr, 3),
        "same_records": bool(eq),
    }, bool(eq)


def key_update(n, C, runs, warmup):
    """Every connection updates its keys once mid-batch -> (numbers, records equal)."""
    from aioquic_amd import batch_io
    from aioquic_amd import receive as R
    from aioquic_amd.crypto import CryptoContext, CryptoPair, apply_key_phase, cached_next_phase, next_key_phase
    from aioquic_amd.packet import QuicProtocolVersion
    from aioquic_amd.route import CidRouter
    from aioquic_amd.tls import CipherSuite, Epoch

    rng = np.random.default_rng(0x4B55)
    version = int(QuicProtocolVersion.VERSION_1)
    suites = [(CipherSuite.AES_128_GCM_SHA256, 32), (CipherSuite.AES_256_GCM_SHA384, 48),
              (CipherSuite.CHACHA20_POLY1305_SHA256, 32)]
    batch_io._per_thread.slots = batch_io.KeySlots(4 * C)
    send_slots = batch_io.KeySlots(2 * C)
    cid = rng.integers(0, 256, (C, 8), dtype=np.uint8)
    cid[:, :4] = np.arange(C, dtype=">u4").view(np.uint8).reshape(C, 4)  # distinct
    cids = [cid[c].tobytes() for c in range(C)]
    conns, first, senders = [], [], []
    for c in range(C):
        cs, slen = suites[c % 3]
        secret = rng.bytes(slen)
        pair = CryptoPair()
        pair.recv.setup(cipher_suite=cs, secret=secret, version=version)
        pair.send.setup(cipher_suite=cs, secret=secret[::-1], version=version)
        conns.append(R.ConnectionKeys(cryptos={Epoch.ONE_RTT: pair}, spaces={Epoch.ONE_RTT: Space()},
                                      host_cid_length=8))
        # the first phase of both directions, to return to before every round
        keep = []
        for ctx in (pair.recv, pair.send):
            k = CryptoContext()
            k.aead, k.key_phase, k.secret = ctx.aead, ctx.key_phase, ctx.secret
            keep.append(k)
        first.append(keep)
        peer = CryptoPair()
        peer.send.setup(cipher_suite=cs, secret=secret, version=version)
        # the peer's next phase: the next AEAD key under the header-protection key it keeps
        nxt = next_key_phase(peer.send)
        second = CryptoContext(key_phase=nxt.key_phase)
        second.aead, second.hp = nxt.aead, peer.send.hp
        senders.append((peer.send, second))
    per = max(n // C, 2)
    order = np.repeat(np.arange(C), per)
    rng.shuffle(order)
    sb = batch_io.SendBatch(slots=send_slots)
    pn = [0] * C
    for c in order.tolist():
        ctx = senders[c][pn[c] >= per // 2]
        h = bytes([0x41 | ctx.key_phase << 2]) + cids[c] + pn[c].to_bytes(2, "big")
        sb.add(ctx, h, rng.bytes(1200 - len(h) - 16), pn[c])
        pn[c] += 1
    datagrams = sb.flush()
    assert all(len(d) == 1200 for d in datagrams)
    router = CidRouter(8, C)
    for c, conn in enumerate(conns):
        router.add(cids[c], conn)
    pairs = [conn.cryptos[Epoch.ONE_RTT] for conn in conns]

    def reset(warm):
        for conn, pair, keep in zip(conns, pairs, first):
            conn.spaces[Epoch.ONE_RTT].expected_packet_number = 0
            for ctx, k in zip((pair.recv, pair.send), keep):
                if ctx.aead is not k.aead:
                    apply_key_phase(ctx, k, "reset")
        if warm:
            for pair in pairs:
                cached_next_phase(pair.recv)
        else:
            for pair in pairs:
                pair.recv._drop_next()

    ways = (("next_phase_off", False, False), ("next_phase_on_cold", True, False), ("next_phase_on_warm", True, True))
    times = {name: [] for name, _, _ in ways}
    recs = {}
    for r in range(warmup + runs):
        for name, on, warm in ways:
            reset(warm)
            t0 = time.perf_counter()
            got, unrouted = R.receive_routed(router, datagrams, next_phase=on)
            t1 = time.perf_counter()
            if r >= warmup:
                times[name].append((t1 - t0) * 1e3)
            assert not unrouted
            if r + 1 == warmup + runs:
                recs[name] = got
            del got
    phases = {pair.recv.key_phase for pair in pairs}
    nd = len(datagrams)
    eq = phases == {1} and all(len(v) == nd and all(g.dropped is None for g in v) for v in recs.values()) and \
        recs["next_phase_off"] == recs["next_phase_on_cold"] == recs["next_phase_on_warm"]
    out = {"datagrams": nd, "connections": C, "updates": C, "same_records": bool(eq)}
    for name, _, _ in ways:
        m = statistics.median(times[name])
        out[name] = dict(_stats(times[name]), datagrams_per_s=round(nd / (m * 1e-3)))
    off = statistics.median(times["next_phase_off"])
    out["off_over_on_cold"] = round(off / statistics.median(times["next_phase_on_cold"]), 3)
    out["off_over_on_warm"] = round(off / statistics.median(times["next_phase_on_warm"]), 3)
    return out, bool(eq)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=4096)
    ap.add_argument("--sizes", default="1048576,65536", help="datagrams per batch, device part")
    ap.add_argument("--host-sizes", default="1048576,65536", help="datagrams per batch, host part ('' = skip)")
    ap.add_argument("--burst", type=int, default=65536, help="datagrams of the connect-burst mix (0 = skip)")
    ap.add_argument("--next-phase", action="store_true",
                    help="also time receive_routed(..., next_phase=True), and the key-update workload")
    ap.add_argument("--update", type=int, default=65536, help="datagrams of the key-update workload (0 = skip)")
    ap.add_argument("--update-conns", type=int, default=1024, help="connections of the key-update workload")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=900, help="seconds before the run gives up")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs must be at least 10")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_route: timed out"))
    signal.alarm(a.timeout)

    import torch

    from aioquic_amd import layout as L
    from aioquic_amd import receive as R
    from aioquic_amd.batch import PacketEngine
    from aioquic_amd.bench_data import HDR_LEN, SLOT_BYTES, make_workload
    from aioquic_amd.crypto import CryptoPair, cached_next_phase, derive_key_iv_hp
    from aioquic_amd.packet import QuicProtocolVersion
    from aioquic_amd.route import CidRouter
    from aioquic_amd.tls import CipherSuite, Epoch

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    C = a.conns
    rng = np.random.default_rng(0xC1D)
    suites = [(L.AES_128_GCM, CipherSuite.AES_128_GCM_SHA256, 32), (L.AES_256_GCM, CipherSuite.AES_256_GCM_SHA384, 48),
              (L.CHACHA20_POLY1305, CipherSuite.CHACHA20_POLY1305_SHA256, 32)]
    version = int(QuicProtocolVersion.VERSION_1)
    cid = rng.integers(0, 256, (C, 8), dtype=np.uint8)
    cid[:, :4] = np.arange(C, dtype=">u4").view(np.uint8).reshape(C, 4)  # distinct
    cids = [cid[c].tobytes() for c in range(C)]
    keys = np.zeros(C, dtype=L.KEY_MATERIAL)
    secrets = []
    for c in range(C):
        suite, cs, slen = suites[c % 3]
        secret = rng.bytes(slen)
        secrets.append((cs, secret))
        key, iv, hp = derive_key_iv_hp(cipher_suite=cs, secret=secret, version=version)
        keys[c] = L.key_material(c, suite, key, iv, hp)[0]
    eng = PacketEngine(2 * C if a.next_phase else C)
    eng.set_key_records(keys)
    if a.next_phase:
        # a next-phase slot per connection at C + c: the same HP key, the other phase bit (the AEAD
        # key does not matter: the traffic carries no update, so k_phase re-points nothing)
        ahead = keys.copy()
        ahead["slot"] += C
        ahead["key_phase"] = 1
        eng.set_key_records(ahead)
    cmap = eng.cid_map(C)
    cmap.put(np.concatenate([L.cid_entry(x, c) for c, x in enumerate(cids)]).tobytes())

    def traffic(n):
        """(wire bytes on the device, connection per datagram): the bench
        workload's packets, each with its connection's CID, protected here."""
        w = make_workload(n, n_keys=C, seed=0x70 + n % 251, order="random")
        conn = w.desc["slot"].astype(np.int64)
        view = w.plain[: n * SLOT_BYTES].reshape(n, SLOT_BYTES)
        view[:, 1:9] = cid[conn]
        d_plain = torch.from_numpy(w.plain).to(dev)
        d_wire = torch.zeros(w.wire_size, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        d_desc = torch.from_numpy(w.desc.view(np.uint8)).to(dev)
        eng.protect(d_desc, n, d_plain, d_wire, d_res, plan=eng.bucket(d_desc, n))
        torch.cuda.synchronize()
        assert (d_res.cpu().numpy().view(L.RESULT)["status"] == 0).all()
        return d_wire, conn, w

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    out = {"tool": "bench_route", "next_phase": bool(a.next_phase), "connections": C, "datagram_bytes": SLOT_BYTES, "runs": a.runs,
           "warmup": a.warmup, "map_buckets": cmap.buckets, "device": {}, "host": {}}
    host_sizes = [int(x) for x in a.host_sizes.split(",") if x]
    wires = {}
    for n in [int(x) for x in a.sizes.split(",") if x]:
        d_wire, conn, w = traffic(n)
        if n in host_sizes:
            wires[n] = (d_wire.cpu().numpy(), conn)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev)
        d_off = t(np.arange(n, dtype=np.uint64) * SLOT_BYTES)
        d_len = t(np.full(n, SLOT_BYTES, np.uint32))
        d_slot = t(np.arange(C, dtype=np.uint32))
        d_exp = t(np.zeros(C, np.uint64))
        d_desc = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
        d_route = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
        d_out = torch.zeros(w.wire_size, dtype=torch.uint8, device=dev)
        d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
        route = lambda: eng.route(cmap, 8, d_off, d_len, n, d_wire, d_slot, d_exp, C, d_route, desc=d_desc)
        both = lambda: eng.unprotect(d_desc, n, d_wire, d_out, d_res, plan=eng.bucket(d_desc, n))
        plan = [None]
        alone = lambda: eng.unprotect(d_desc, n, d_wire, d_out, d_res, plan=plan[0])
        t_route, t_both, t_alone, t_phase = [], [], [], []
        if a.next_phase:
            d_next = t(np.arange(C, 2 * C, dtype=np.uint32))
            d_phase = torch.full((n,), 0xAB, dtype=torch.uint8, device=dev)
            phase = lambda: eng.route_phase(d_route, d_next, C, d_desc, n, d_wire, d_phase)
        for r in range(a.warmup + a.runs):
            x = timed(route)
            if a.next_phase:
                p_ = timed(phase)
                if r >= a.warmup:
                    t_phase.append(p_)
            y = timed(both)
            plan[0] = eng.bucket(d_desc, n)
            z = timed(alone)
            if r >= a.warmup:
                t_route.append(x), t_both.append(y), t_alone.append(z)
        torch.cuda.synchronize()
        rr = d_route.cpu().numpy().view(L.ROUTE)
        res = d_res.cpu().numpy().view(L.RESULT)
        ok = bool((rr["cls"] == L.R_SHORT).all() and (rr["conn"] == conn).all() and (res["status"] == 0).all()
                  and np.array_equal(d_out.cpu().numpy().reshape(-1)[: n * SLOT_BYTES].reshape(n, SLOT_BYTES)[:, :HDR_LEN],
                                     w.plain[: n * SLOT_BYTES].reshape(n, SLOT_BYTES)[:, :HDR_LEN]))
        mr, mb = statistics.median(t_route), statistics.median(t_both)
        out["device"][str(n)] = {
            "k_route": _stats(t_route), "bucket_plus_unprotect_planned": _stats(t_both),
            "unprotect_planned_alone": _stats(t_alone),
            "k_route_over_planned_unprotect": round(mr / mb, 4),
            "k_route_ns_per_datagram": round(mr * 1e6 / n, 3),
            "k_route_gb_per_s_at_200B": round(200 * n / (mr * 1e-3) / 1e9, 1),
            "routed_and_unprotected_ok": ok,
        }
        if a.next_phase:
            mp = statistics.median(t_phase)
            ok = ok and not d_phase.cpu().numpy().any()
            out["device"][str(n)]["k_phase"] = dict(_stats(t_phase), over_k_route=round(mp / mr, 3),
                                                   over_planned_unprotect=round(mp / mb, 4),
                                                   ns_per_datagram=round(mp * 1e6 / n, 3))
        if not ok:
            print(json.dumps(out))
            sys.exit("bench_route: the routed batch did not unprotect")
        del d_wire, d_out, d_desc, d_route, d_res, w
        torch.cuda.empty_cache()

    # ---- host part: list of bytes in, records out
    conns = []
    for c in range(C if host_sizes else 0):
        cs, secret = secrets[c]
        pair = CryptoPair()
        pair.recv.setup(cipher_suite=cs, secret=secret, version=version)
        conns.append(R.ConnectionKeys(cryptos={Epoch.ONE_RTT: pair}, spaces={Epoch.ONE_RTT: Space()},
                                      host_cid_length=8))
    router = CidRouter(8, C) if host_sizes else None
    for c, conn in enumerate(conns):
        router.add(cids[c], conn)
    by_cid = {cids[c]: conn for c, conn in enumerate(conns)}

    def reset():
        for conn in conns:
            conn.spaces[Epoch.ONE_RTT].expected_packet_number = 0

    if a.next_phase and host_sizes:
        # a slot for every connection's next phase beside its current one
        from aioquic_amd import batch_io

        batch_io._per_thread.slots = batch_io.KeySlots(2 * C + 64)
    same = True
    for n in host_sizes:
        if n not in wires:
            d_wire, conn, _ = traffic(n)
            wires[n] = (d_wire.cpu().numpy(), conn)
        wire, conn = wires.pop(n)
        raw = wire[: n * SLOT_BYTES].tobytes()
        datagrams = [raw[i * SLOT_BYTES:(i + 1) * SLOT_BYTES] for i in range(n)]
        del raw, wire
        t_routed, t_dict, t_pass, t_next = [], [], [], []
        got = want = None
        first_next = build_next = None
        same_next = True
        if a.next_phase:
            # the first call with next slots builds every connection's next-phase context
            for conn in conns:
                conn.cryptos[Epoch.ONE_RTT].recv._drop_next()
            reset()
            t0 = time.perf_counter()
            ahead, _ = R.receive_routed(router, datagrams, next_phase=True)
            first_next = (time.perf_counter() - t0) * 1e3
            del ahead
            for conn in conns:
                conn.cryptos[Epoch.ONE_RTT].recv._drop_next()
            t0 = time.perf_counter()
            for conn in conns:
                cached_next_phase(conn.cryptos[Epoch.ONE_RTT].recv)
            build_next = (time.perf_counter() - t0) * 1e3
        for r in range(a.warmup + a.runs):
            if a.next_phase:
                reset()
                t0 = time.perf_counter()
                ahead, unrouted = R.receive_routed(router, datagrams, next_phase=True)
                t1 = time.perf_counter()
                if r >= a.warmup:
                    t_next.append((t1 - t0) * 1e3)
                if r + 1 < a.warmup + a.runs:
                    del ahead
            reset()
            t0 = time.perf_counter()
            got, unrouted = R.receive_routed(router, datagrams)
            t1 = time.perf_counter()
            reset()
            t2 = time.perf_counter()
            items = [(by_cid[d[1:9]], d) for d in datagrams]
            t3 = time.perf_counter()
            want = R.receive_datagrams(items)
            t4 = time.perf_counter()
            if r >= a.warmup:
                t_routed.append((t1 - t0) * 1e3)
                t_pass.append((t3 - t2) * 1e3)
                t_dict.append((t4 - t2) * 1e3)
            if r + 1 < a.warmup + a.runs:
                del got, want, items
        eq = not unrouted and len(got) == len(want) == n and all(
            g == w_ and g.dropped is None for g, w_ in zip(got, want))
        same = same and eq
        mr, md = statistics.median(t_routed), statistics.median(t_dict)
        out["host"][str(n)] = {
            "receive_routed": dict(_stats(t_routed), datagrams_per_s=round(n / (mr * 1e-3))),
            "dict_pass_plus_receive_datagrams": dict(_stats(t_dict), dict_pass=_stats(t_pass),
                                                     datagrams_per_s=round(n / (md * 1e-3))),
            "dict_way_over_routed": round(md / mr, 3),
            "same_records": bool(eq),
        }
        if a.next_phase:
            same_next = ahead == got
            same = same and same_next
            mn = statistics.median(t_next)
            out["host"][str(n)]["receive_routed_next_phase"] = dict(
                _stats(t_next), datagrams_per_s=round(n / (mn * 1e-3)), over_default=round(mn / mr, 4),
                first_call_ms=round(first_next, 3), next_contexts_build_ms=round(build_next, 3),
                same_records=bool(same_next))
            del ahead
        del datagrams, got, want
    if a.burst:
        out["connect_burst"], eq = connect_burst(a.burst, C, a.runs, a.warmup)
        same = same and eq
    if a.next_phase and a.update:
        out["key_update"], eq = key_update(a.update, a.update_conns, a.runs, a.warmup)
        same = same and eq
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        sys.exit("bench_route: the two host ways' records differ")


if __name__ == "__main__":
    main()
