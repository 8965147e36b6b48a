#!/usr/bin/env python3
"""A flood of first flights at a server in Retry mode: two ways of answering
it, timed on a GPU box.  Prints one JSON object (and writes it to --out).

The batch: N client Initials without a token (default 65536, QUIC v1 and v2
alternating, 1200 bytes each, IPv4 and IPv6 senders alternating), every one of
them owed a Retry (asyncio/server.py:95-111).

  a  receive.answer_routed: one upload; the device assembles every Retry,
     seals every token and appends every integrity tag in the same call
  b  what there was before it: receive.accept_routed(need_token=True) (the
     Initials come back unrouted), then per datagram pull_quic_header,
     RetryTokens.create_token (one AEAD.encrypt) and the Retry packet with
     packet.get_retry_integrity_tag (another)

Every timing is taken in a process of its own (--way a or --way b: one warm-up
call over a small batch, then one timed call, wall clock around a call that
ends with its results on the host).  Without --way this is the driver: it
starts --rounds pairs of such processes, the two ways alternating, one at a
time, and reports the median replies per second of each.  Both ways' replies
are checked: one per Initial, every one parsed, its tag recomputed and its
token validated for a sample.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VERSION_1, VERSION_2 = 0x00000001, 0x6B3343CF
SCID = b"\x5C" * 8


def initials(n: int, seed: int):
    """n token-less Initial-shaped datagrams of 1200 bytes (nothing in Retry
    mode decrypts them) and their senders' addresses."""
    import numpy as np

    rng = np.random.default_rng(seed)
    body = rng.bytes(1200)
    out, addrs = [], []
    for k in range(n):
        version = (VERSION_1, VERSION_2)[k % 2]
        head = bytes([0xD0 if version == VERSION_2 else 0xC0]) + version.to_bytes(4, "big") + b"\x08" + \
            k.to_bytes(4, "big") + rng.bytes(4) + bytes([len(SCID)]) + SCID + b"\x00"
        rest = 1200 - len(head) - 2
        out.append(head + (0x4000 | rest).to_bytes(2, "big") + body[:rest])
        addrs.append(("2001:db8::%x:%x" % (k >> 16, k & 0xFFFF), 1024 + k % 60000) if k % 4 >= 2 else
                     ("198.51.%d.%d" % (k >> 8 & 255, k & 255), 1024 + k % 60000))
    return out, addrs


def one(way: str, n: int, warm: int):
    from aioquic_amd import batch_io
    from aioquic_amd import layout as L
    from aioquic_amd import receive as R
    from aioquic_amd.buffer import Buffer
    from aioquic_amd.packet import QuicPacketType, encode_long_header_first_byte, get_retry_integrity_tag, \
        pull_quic_header
    from aioquic_amd.retry import RetryTokens
    from aioquic_amd.route import CidRouter

    slots = batch_io.KeySlots(2 * n + 64)
    R.default_slots = batch_io.default_slots = lambda: slots
    tokens = RetryTokens()
    router = CidRouter(8, 64)
    refuse = lambda header, i: None

    def way_a(dgs, addrs):
        return R.answer_routed(router, dgs, addrs, refuse, tokens=tokens)[3]

    def way_b(dgs, addrs):
        _, unrouted, _ = R.accept_routed(router, dgs, refuse, need_token=True)
        replies = []
        for i, cls in unrouted:
            if cls != L.R_LONG or len(dgs[i]) < 1200:
                continue
            h = pull_quic_header(Buffer(data=dgs[i]), host_cid_length=8)
            if h.packet_type != QuicPacketType.INITIAL or h.token:
                continue
            scid = os.urandom(8)
            token = tokens.create_token(addrs[i], h.destination_cid, scid)
            pkt = bytes([encode_long_header_first_byte(h.version, QuicPacketType.RETRY, 0)]) + \
                h.version.to_bytes(4, "big") + bytes([len(h.source_cid)]) + h.source_cid + bytes([len(scid)]) + scid + \
                token
            replies.append((i, pkt + get_retry_integrity_tag(pkt, h.destination_cid, h.version)))
        return replies

    run = way_a if way == "a" else way_b
    dgs, addrs = initials(n, 19)
    run(dgs[:warm], addrs[:warm])
    t0 = time.perf_counter()
    replies = run(dgs, addrs)
    dt = time.perf_counter() - t0
    ok = [i for i, _ in replies] == list(range(n))
    for i, p in replies[::max(1, n // 257)]:
        h = pull_quic_header(Buffer(data=p), host_cid_length=8)
        d = dgs[i]
        ok = ok and h.packet_type == QuicPacketType.RETRY and h.destination_cid == SCID
        ok = ok and get_retry_integrity_tag(p[:-16], d[6:14], h.version) == p[-16:]
        ok = ok and tokens.validate_token(addrs[i], h.token) == (d[6:14], h.source_cid)
    slots.close()
    return {"way": way, "initials": n, "replies": len(replies), "seconds": round(dt, 6),
            "replies_per_second": round(len(replies) / dt, 1), "replies_ok": bool(ok)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--initials", type=int, default=65536)
    ap.add_argument("--warm", type=int, default=256, help="datagrams of the warm-up call")
    ap.add_argument("--rounds", type=int, default=3, help="driver: pairs of fresh processes")
    ap.add_argument("--way", choices=("a", "b"), default=None, help="one timed call in this process")
    ap.add_argument("--timeout", type=int, default=240, help="driver: seconds one child may take")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.way:
        out = one(a.way, a.initials, a.warm)
    else:
        runs = {"a": [], "b": []}
        for r in range(a.rounds):
            for way in ("ab" if r % 2 == 0 else "ba"):
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--way", way, "--initials",
                                    str(a.initials), "--warm", str(a.warm)], capture_output=True, text=True,
                                   timeout=a.timeout)
                if p.returncode != 0:
                    sys.exit("bench_reply: way %s failed (status %d), nothing more is started\n%s"
                             % (way, p.returncode, p.stderr[-2000:]))
                runs[way].append(json.loads(p.stdout.strip().splitlines()[-1]))
        med = {w: statistics.median(x["replies_per_second"] for x in runs[w]) for w in "ab"}
        out = {"tool": "bench_reply", "initials": a.initials, "rounds": a.rounds,
               "a_answer_routed": {"replies_per_second_median": med["a"],
                                   "seconds": [x["seconds"] for x in runs["a"]]},
               "b_accept_routed_then_host_replies": {"replies_per_second_median": med["b"],
                                                     "seconds": [x["seconds"] for x in runs["b"]]},
               "a_over_b": round(med["a"] / med["b"], 2),
               "replies_ok": all(x["replies_ok"] and x["replies"] == a.initials for w in "ab" for x in runs[w])}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not out["replies_ok"]:
        sys.exit("bench_reply: a reply is missing or wrong")


if __name__ == "__main__":
    main()
