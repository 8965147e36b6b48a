#!/usr/bin/env python3
"""What the device form of next_key_phase (qpp_keytab_derive_next) buys the
routed receive path, on the two workloads of DESIGN.md sec. 4, Round 18.

  first     the first next_phase batch over --conns connections (default 4096),
            --first datagrams (default 65536), no connection updating: every
            keyed 1-RTT receive context needs its next phase built and
            installed.  receive_routed(next_phase=True), which builds them on
            the host one connection at a time (crypto.cached_next_phase),
            against receive_routed_keys(next_phase=True, device_keys=True),
            which makes one device call (batch_io.setup_next_phase_batch).
            Both "cold" (no next phase cached) and "warm" (cached by the round
            before: the steady state of a second batch).
  update    --update datagrams (default 65536) over --update-conns connections
            (default 1024), every connection moving to its next key phase at
            its midpoint: the same two ways, cold and warm; the commit of the
            rolled pairs is CryptoPair._update_key_cached per pair against one
            batch_io.update_keys_batch.
  derive    KeyTable.derive_next alone over --conns records: wall time of the
            call and, from the table's timing events (derive_trace), the
            derivation kernel and the slot expansion.

The ways alternate in one process after --warmup rounds; median, min and max
of --runs rounds.  Every round starts from the same connection state (expected
packet numbers, key phases and cached next phases reset outside the timings).
The records of all ways of a workload are compared at the end: a mismatch
fails the run.  One JSON object on stdout (and in --out).
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


def workload(n, C, runs, warmup, update: bool):
    """-> (numbers, records equal).  update: every connection updates mid-batch."""
    from aioquic_amd import batch_io
    from aioquic_amd import receive as R
    from aioquic_amd.crypto import CryptoContext, CryptoPair, apply_key_phase, cached_next_phase, next_key_phase
    from aioquic_amd.packet import QuicProtocolVersion
    from aioquic_amd.route import CidRouter
    from aioquic_amd.tls import CipherSuite, Epoch

    rng = np.random.default_rng(0x4E58)
    version = int(QuicProtocolVersion.VERSION_1)
    suites = [(CipherSuite.AES_128_GCM_SHA256, 32), (CipherSuite.AES_256_GCM_SHA384, 48),
              (CipherSuite.CHACHA20_POLY1305_SHA256, 32)]
    old = getattr(batch_io._per_thread, "slots", None)
    if old is not None:
        old.close()
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
        keep = []
        for ctx in (pair.recv, pair.send):
            k = CryptoContext()
            k.aead, k.key_phase, k.secret = ctx.aead, ctx.key_phase, ctx.secret
            keep.append(k)
        first.append(keep)
        peer = CryptoPair()
        peer.send.setup(cipher_suite=cs, secret=secret, version=version)
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
        ctx = senders[c][update and pn[c] >= per // 2]
        h = bytes([0x41 | ctx.key_phase << 2]) + cids[c] + pn[c].to_bytes(2, "big")
        sb.add(ctx, h, rng.bytes(1200 - len(h) - 16), pn[c])
        pn[c] += 1
    datagrams = sb.flush()
    send_slots.close()
    router = CidRouter(8, C)
    for c, conn in enumerate(conns):
        router.add(cids[c], conn)
    pairs = [conn.cryptos[Epoch.ONE_RTT] for conn in conns]

    def reset(device, warm):
        for conn, pair, keep in zip(conns, pairs, first):
            conn.spaces[Epoch.ONE_RTT].expected_packet_number = 0
            for ctx, k in zip((pair.recv, pair.send), keep):
                if ctx.aead is not k.aead:
                    apply_key_phase(ctx, k, "reset")
        for pair in pairs:
            pair.recv._drop_next()
        if warm and device:
            batch_io.setup_next_phase_batch([pair.recv for pair in pairs])
        elif warm:
            for pair in pairs:
                cached_next_phase(pair.recv)

    ways = (("host_cold", False, False), ("device_cold", True, False), ("host_warm", False, True),
            ("device_warm", True, True))
    times = {name: [] for name, _, _ in ways}
    recs = {}
    for r in range(warmup + runs):
        for name, device, warm in ways:
            reset(device, warm)
            t0 = time.perf_counter()
            if device:
                got, unrouted = R.receive_routed_keys(router, datagrams, next_phase=True, device_keys=True)
            else:
                got, unrouted = R.receive_routed(router, datagrams, next_phase=True)
            t1 = time.perf_counter()
            if r >= warmup:
                times[name].append((t1 - t0) * 1e3)
            assert not unrouted
            if r + 1 == warmup + runs:
                recs[name] = got
            del got
    phases = {pair.recv.key_phase for pair in pairs}
    nd = len(datagrams)
    eq = phases == {1 if update else 0} and \
        all(len(v) == nd and all(g.dropped is None for g in v) for v in recs.values()) and \
        all(v == recs["host_cold"] for v in recs.values())
    out = {"datagrams": nd, "connections": C, "updates": C if update else 0, "same_records": bool(eq)}
    for name, _, _ in ways:
        m = statistics.median(times[name])
        out[name] = dict(_stats(times[name]), datagrams_per_s=round(nd / (m * 1e-3)))
    for kind in ("cold", "warm"):
        out[f"host_over_device_{kind}"] = round(statistics.median(times[f"host_{kind}"]) /
                                                statistics.median(times[f"device_{kind}"]), 3)
    batch_io._per_thread.slots.close()
    return out, bool(eq)


def derive_alone(C, runs, warmup):
    """KeyTable.derive_next over C records, installing C slots."""
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    rng = np.random.default_rng(0x4E59)
    eng = PacketEngine(C)
    recs = np.concatenate([L.next_phase_record(i, i % 3, rng.bytes(48 if i % 3 == 1 else 32), rng.bytes(32),
                                               key_phase=i & 1) for i in range(C)]).tobytes()
    eng.table.derive_trace(1)
    wall, derive, setup = [], [], []
    for r in range(warmup + runs):
        t0 = time.perf_counter()
        eng.table.derive_next(recs)
        t1 = time.perf_counter()
        d, s = eng.table.derive_trace()
        if r >= warmup:
            wall.append((t1 - t0) * 1e3)
            derive.append(d)
            setup.append(s)
    return {"records": C, "call": _stats(wall), "k_derive_next": _stats(derive), "k_key_setup": _stats(setup)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--conns", type=int, default=4096)
    ap.add_argument("--first", type=int, default=65536, help="datagrams of the first-batch workload (0 = skip)")
    ap.add_argument("--update", type=int, default=65536, help="datagrams of the key-update workload (0 = skip)")
    ap.add_argument("--update-conns", type=int, default=1024)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--timeout", type=int, default=540, help="seconds before the run gives up")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    signal.alarm(a.timeout)
    import torch

    assert torch.cuda.is_available(), "bench_next_keys needs a GPU"
    torch.cuda.set_device(0)
    out = {"tool": "bench_next_keys", "runs": a.runs, "warmup": a.warmup, "datagram_bytes": 1200}
    ok = True
    out["derive_next_alone"] = derive_alone(a.conns, max(a.runs, 11), max(a.warmup, 2))
    if a.first:
        out["first_batch"], eq = workload(a.first, a.conns, a.runs, a.warmup, update=False)
        ok = ok and eq
    if a.update:
        out["key_update"], eq = workload(a.update, a.update_conns, a.runs, a.warmup, update=True)
        ok = ok and eq
    out["same_records"] = ok
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
