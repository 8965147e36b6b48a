#!/usr/bin/env python3
"""What routed send (send.send_routed: headers and packet numbers built on the
device) costs against the batched sender a caller has today, from host
payloads, and what the filling kernel costs alone.

  builders  per-connection QuicPacketBuilders: start_packet and one frame's
            bytes per payload, then flush_builders.  The builder's per-packet
            Python is inside the window: it is what the caller pays.
  routed    send.send_routed over the same (connection, payload) list.

The window is from the list of (connection index, payload bytes) to wire
datagrams as bytes objects (the builders return theirs per connection, routed
send in item order; the regrouping for the comparison is outside the window).
Workloads: --payloads payloads (default 65536) of --size bytes (default 1173)
over each of --conns connection counts (default 64 and 4096), mixed suites.
Both ways alternate in one process, --warmup calls (default 3) and --runs timed
calls (default 11) each; median with min and max.  Both ways advance the same
packet numbers call by call, and the last call's datagrams are compared: a
mismatch fails the run.

The builders' window is split into the per-packet loop and flush_builders
(which closes each builder's last packet and protects).  Routed send's window
is also split: the Python around the one C call, and the
C call (staging copy, H2D, two launches, D2H, one bytes object per datagram).
The device's share of it is timed with device events over the same batch
resident in device memory: qpp_send_fill alone (median of 11), and
qpp_send_fill + qpp_protect.  One JSON object on stdout (and in --out).
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
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4), "max_ms": round(max(xs), 4)}


def workload(n, C, size, runs, warmup):
    import torch
    from aioquic_amd import _crypto, send
    from aioquic_amd import layout as L
    from aioquic_amd.batch_io import KeySlots
    from aioquic_amd.crypto import CryptoPair
    from aioquic_amd.packet import QuicFrameType, QuicPacketType, QuicProtocolVersion
    from aioquic_amd.packet_builder import QuicPacketBuilder, flush_builders
    from aioquic_amd.tls import CipherSuite

    rng = np.random.default_rng(0x5E4D + C)
    version = int(QuicProtocolVersion.VERSION_1)
    suites = [(CipherSuite.AES_128_GCM_SHA256, 32), (CipherSuite.AES_256_GCM_SHA384, 48),
              (CipherSuite.CHACHA20_POLY1305_SHA256, 32)]
    secrets = [rng.bytes(suites[c % 3][1]) for c in range(C)]
    cids = [rng.bytes(8) for _ in range(C)]

    def pairs():
        out = []
        for c in range(C):
            p = CryptoPair()
            p.send.setup(cipher_suite=suites[c % 3][0], secret=secrets[c], version=version)
            out.append(p)
        return out

    conn_of = rng.integers(0, C, n).tolist()
    blob = rng.bytes(n * size)
    # one STREAM frame's bytes each: the builder writes the frame type itself
    items = [(c, b"\x08" + blob[k * size + 1:(k + 1) * size]) for k, c in enumerate(conn_of)]
    pairs_b, pairs_s = pairs(), pairs()
    builders = [QuicPacketBuilder(host_cid=bytes(8), peer_cid=cids[c], version=version, is_client=False,
                                  max_datagram_size=1500, packet_number=0) for c in range(C)]
    conns = [send.SendConnection(pairs_s[c], cids[c], 0) for c in range(C)]
    slots_b, slots_s = KeySlots(max(2 * C, 64)), KeySlots(max(2 * C, 64))
    ONE_RTT, STREAM = QuicPacketType.ONE_RTT, QuicFrameType.STREAM_BASE

    build_part = []

    def run_builders():
        t0 = time.perf_counter()
        for c, p in items:
            b = builders[c]
            b.start_packet(ONE_RTT, pairs_b[c])
            b.start_frame(STREAM, len(p)).push_bytes(p[1:])
        build_part.append((time.perf_counter() - t0) * 1e3)
        return flush_builders(builders, slots=slots_b)

    c_call = []
    inner = _crypto.send_routed

    class Timed:  # send.py's view of the extension, its one call timed
        def __getattr__(self, name):
            return getattr(_crypto, name)

        @staticmethod
        def send_routed(*a):
            t0 = time.perf_counter()
            r = inner(*a)
            c_call.append((time.perf_counter() - t0) * 1e3)
            return r

    send._crypto = Timed()

    def run_routed():
        return send.send_routed(conns, items, slots=slots_s)

    times = {"builders": [], "routed": []}
    last = {}
    for r in range(warmup + runs):
        for name, fn in (("builders", run_builders), ("routed", run_routed)):
            t0 = time.perf_counter()
            last[name] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            if r >= warmup:
                times[name].append(dt)
    send._crypto = _crypto
    per_conn = [iter(dgs) for dgs, _ in last["builders"]]
    same = [next(per_conn[c]) for c, _ in items] == last["routed"][0]
    same = same and [b.packet_number for b in builders] == [c.packet_number for c in conns]
    out = {"payloads": n, "payload_bytes": size, "connections": C, "same_datagrams": bool(same)}
    for name in times:
        m = statistics.median(times[name])
        out[name] = dict(_stats(times[name]), packets_per_s=round(n / (m * 1e-3)))
    out["builders_over_routed"] = round(statistics.median(times["builders"]) / statistics.median(times["routed"]), 3)
    bp = build_part[-runs:]
    out["builders_per_packet_python"] = _stats(bp)
    out["builders_flush"] = _stats([t - b for t, b in zip(times["builders"], bp)])
    cc = c_call[-runs:]
    out["routed_c_call"] = _stats(cc)
    out["routed_python"] = _stats([t - c for t, c in zip(times["routed"], cc)])

    # ---- the device's share, over the same batch resident in device memory
    dev = torch.device("cuda", 0)
    lens = np.full(n, size, np.uint32)
    off = (np.arange(n, dtype=np.uint64) * np.uint64(L.SEND_HEAD + size + L.SEND_TAIL)) + np.uint64(L.SEND_HEAD)
    total = int(off[-1]) + size + L.SEND_TAIL
    seq = np.zeros(n, np.uint32)
    count = [0] * C
    for k, c in enumerate(conn_of):
        seq[k] = count[c]
        count[c] += 1
    state = np.zeros(C, L.SEND_CONN)
    ctxs = [p.send for p in pairs_s]
    state["slot"] = slots_s.assign([(x.aead, x.hp, x.key_phase) for x in ctxs])
    state["cid_len"] = 8
    state["cid"][:, :8] = np.frombuffer(b"".join(cids), np.uint8).reshape(C, 8)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_buf = torch.zeros(total, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(total, dtype=torch.uint8, device=dev)
    d_state, d_off, d_len, d_conn, d_seq = t(state), t(off), t(lens), t(np.asarray(conn_of, np.uint32)), t(seq)
    d_desc = torch.zeros(n * 40, dtype=torch.uint8, device=dev)
    d_rec = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    stream = int(torch.cuda.current_stream().cuda_stream)
    ptr = lambda x: int(x.data_ptr())

    def fill():
        _crypto.send_fill(slots_s.table, ptr(d_state), C, ptr(d_off), ptr(d_len), ptr(d_conn), ptr(d_seq), n,
                          ptr(d_buf), total, ptr(d_desc), ptr(d_rec), stream)

    def both():
        fill()
        _crypto.protect(slots_s.table, ptr(d_desc), n, ptr(d_buf), ptr(d_out), ptr(d_res), stream, None)

    for name, fn in (("k_send", fill), ("k_send_and_protect", both)):
        ms = []
        for r in range(3 + 11):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if r >= 3:
                ms.append(a.elapsed_time(b))
        out[name] = _stats(ms)
    rec = d_rec.cpu().numpy().view(L.SEND_REC)
    res = d_res.cpu().numpy().view(L.RESULT)
    out["device_form_ok"] = bool((rec["status"] == L.SN_OK).all() and (res["status"] == L.S_OK).all())
    out["staged_bytes"] = total
    slots_b.close(), slots_s.close()
    return out, bool(same) and out["device_form_ok"]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--payloads", type=int, default=65536)
    ap.add_argument("--size", type=int, default=1173)
    ap.add_argument("--conns", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=540, help="seconds before the run gives up")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    signal.alarm(a.timeout)
    import torch

    assert torch.cuda.is_available(), "bench_send needs a GPU"
    torch.cuda.set_device(0)
    out = {"tool": "bench_send", "runs": a.runs, "warmup": a.warmup, "workloads": []}
    ok = True
    for C in a.conns:
        w, same = workload(a.payloads, C, a.size, a.runs, a.warmup)
        out["workloads"].append(w)
        ok = ok and same
    out["same_datagrams"] = ok
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
