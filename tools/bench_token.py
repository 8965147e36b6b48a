#!/usr/bin/env python3
"""A burst of returning clients at a server in Retry mode: two ways of
validating their tokens, timed on a GPU box.  Prints one JSON object (and
writes it to --out).

The batch: N second Initials (default 4096, QUIC v1 and v2 and IPv4 and IPv6
senders alternating, 1200 bytes each, distinct DCIDs), each protected with the
Initial keys of its DCID and carrying a Retry token of this server
(asyncio/server.py:112-131).  With --forged-every K, every K-th token has a
flipped tag bit.

  a  receive.serve_routed: the device locates, opens and checks every token
     ahead of the accepting kernel; `accept` gets the two CIDs
  b  what there was before it: receive.answer_routed, every Initial with a
     token accepted on the device, RetryTokens.validate_token (one
     AEAD.decrypt) in the `accept` callback

One process: every call runs on a fresh router and key table (set up outside
the timed window), the two ways alternating, --warmup calls of each first,
then --rounds timed ones, wall clock around a call that ends with its results
on the host; the medians are reported.  Both ways' outcomes are checked: the
same connections accepted, the forged ones refused.  Then the two device
stages the feature adds (the locating kernel, the tokens' unprotect) are timed
alone with device events over hand-built records of the same batch.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VERSION_1, VERSION_2 = 0x00000001, 0x6B3343CF
SCID = b"\x5C" * 8


def batch(n: int, tokens, forged_every: int):
    """n protected second Initials, their senders and which are forged."""
    from aioquic_amd import layout as L
    from oracle import oracle as O

    out, addrs, forged = [], [], []
    for k in range(n):
        version = (VERSION_1, VERSION_2)[k % 2]
        addr = ("2001:db8::%x:%x" % (k >> 16, k & 0xFFFF), 1024 + k % 60000) if k % 4 >= 2 else \
            ("198.51.%d.%d" % (k >> 8 & 255, k & 255), 1024 + k % 60000)
        dcid = b"\xA7" + k.to_bytes(3, "big") + b"\x5A\xA5" + (k * 40503 & 0xFFFF).to_bytes(2, "big")
        token = tokens.seal(tokens.take(1), addr, b"\xD0" + k.to_bytes(4, "big") + b"\x0D" * 3, dcid)
        bad = bool(forged_every) and k % forged_every == forged_every - 1
        if bad:
            token = token[:-1] + bytes([token[-1] ^ 0x01])
        secret = O.initial_secrets(dcid, version)[0]
        key, iv, hp = O.derive_key_iv_hp(L.AES_128_GCM, secret, version)
        bits = 1 if version == VERSION_2 else 0

        def hdr(rest):
            return (bytes([0xC0 | bits << 4 | 1]) + version.to_bytes(4, "big") + bytes([len(dcid)]) + dcid
                    + bytes([len(SCID)]) + SCID + (0x4000 | len(token)).to_bytes(2, "big") + token
                    + (0x4000 | (rest + 2)).to_bytes(2, "big") + b"\x00\x00")

        body = 1200 - len(hdr(0)) - 16
        payload = (b"\x06\x00\x40\x10" + bytes(body))[:body]
        out.append(O.protect(L.AES_128_GCM, key, iv, hp, hdr(body + 16), payload, 0))
        addrs.append(addr), forged.append(bad)
    return out, addrs, forged


def new_conn(version: int):
    """What a server's accept callback makes: one version, every pair unset."""
    from aioquic_amd.crypto import CryptoPair
    from aioquic_amd.receive import ConnectionKeys
    from aioquic_amd.tls import Epoch

    class Space:
        expected_packet_number = 0

    pair = CryptoPair()
    return ConnectionKeys(
        cryptos={Epoch.INITIAL: pair, Epoch.HANDSHAKE: CryptoPair(), Epoch.ZERO_RTT: CryptoPair(),
                 Epoch.ONE_RTT: CryptoPair()},
        spaces={e: Space() for e in (Epoch.INITIAL, Epoch.HANDSHAKE, Epoch.ONE_RTT)}, cryptos_initial={version: pair},
        host_cid_length=8, is_client=False, supported_versions=[version])


def one_call(way: str, datagrams, addrs, tokens):
    """(seconds, accepted datagram indices, refused or dropped ones) of one call on a fresh server."""
    from aioquic_amd import batch_io
    from aioquic_amd import receive as RX
    from aioquic_amd.route import CidRouter

    n = len(datagrams)
    slots = batch_io.KeySlots(2 * n + 64)
    RX.default_slots = batch_io.default_slots = lambda: slots
    router = CidRouter(8, 2 * n)
    refused = []
    try:
        if way == "a":
            t0 = time.perf_counter()
            out = RX.serve_routed(router, datagrams, addrs, lambda h, i, odcid, rscid: new_conn(h.version),
                                  tokens=tokens)
            dt = time.perf_counter() - t0
            refused = [i for i, _ in out[4]]
        else:
            def accept(header, i):
                try:
                    tokens.validate_token(addrs[i], header.token)
                except ValueError:
                    refused.append(i)
                    return None
                return new_conn(header.version)

            t0 = time.perf_counter()
            out = RX.answer_routed(router, datagrams, addrs, accept, tokens=tokens)
            dt = time.perf_counter() - t0
        ok = [r.datagram for r in out[0] if r.dropped is None and r.packet_number == 0]
        assert ok == [i for i, _ in out[2]], "every accepted connection's first packet opened"
        return dt, ok, refused
    finally:
        slots.close()


def stages(datagrams, addrs, tokens, rounds: int):
    """Median device-event microseconds of the locating kernel and of the
    tokens' unprotect over the batch, each launched alone."""
    import numpy as np
    import torch

    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    n = len(datagrams)
    dev = torch.device("cuda", 0)
    lens = np.full(n, 1200, np.uint32)
    offs = (np.arange(n, dtype=np.uint64) * 1200)
    walk = np.zeros((n, L.WALK_MAX), L.WALK)
    walk["desc"] = L.DESC_NONE
    for a, d in enumerate(datagrams):
        tl = int.from_bytes(d[23:25], "big") & 0x3FFF
        walk[a, 0] = (0, 1200, int.from_bytes(d[1:5], "big"), L.DESC_NONE, 25 + tl + 2, tl, 0, L.W_OK, 8, 8)
    route = np.zeros(n, L.ROUTE)
    route["conn"], route["cls"] = L.CONN_NONE, L.R_LONG
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    z = lambda size: torch.zeros(size, dtype=torch.uint8, device=dev)
    d_in, d_off, d_len = t(np.frombuffer(b"".join(datagrams), np.uint8)), t(offs), t(lens)
    d_idx = t(np.arange(n, dtype=np.uint32))
    d_walk, d_wn, d_route = t(walk), t(np.ones(n, np.uint32)), t(route)
    tdesc, trec, tok, tres = z(n * 40), z(n * 48), z(n * L.TOKEN_STRIDE), z(n * 16)
    eng = PacketEngine(3)
    eng.set_key_records(tokens.key_records())

    def timed(fn):
        us = []
        for k in range(3 + rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if k >= 3:
                us.append(e0.elapsed_time(e1) * 1000.0)
        return round(statistics.median(us), 1)

    k_token = timed(lambda: eng.route_token(d_off, d_len, n, d_in, d_route, d_idx, n, d_walk, d_wn, d_idx, n, tdesc,
                                            trec))
    opened = timed(lambda: eng.unprotect(tdesc, n, d_in, tok, tres))
    located = int((trec.cpu().numpy().view(L.TOKEN_REC)["status"] == L.TK_OK).sum())
    authentic = int((tres.cpu().numpy().view(L.RESULT)["status"] == L.S_OK).sum())
    return {"k_token_us": k_token, "token_unprotect_us": opened, "located": located, "authentic": authentic}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=11)
    ap.add_argument("--forged-every", type=int, default=0, help="0: every token honest; 2: half of them forged")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch

    from aioquic_amd.retry import RetryTokens

    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    torch.cuda.set_device(0)
    tokens = RetryTokens(bytes(range(0x40, 0x50)), bytes(range(0x70, 0x7C)))
    datagrams, addrs, forged = batch(args.n, tokens, args.forged_every)
    honest = [i for i, f in enumerate(forged) if not f]
    bad = [i for i, f in enumerate(forged) if f]
    times = {"a": [], "b": []}
    for k in range(args.warmup + args.rounds):
        for way in ("ab", "ba")[k % 2]:
            dt, ok, refused = one_call(way, datagrams, addrs, tokens)
            assert ok == honest and refused == bad, (way, len(ok), len(refused))
            if k >= args.warmup:
                times[way].append(dt)
    result = {
        "n": args.n, "forged": len(bad), "warmup": args.warmup, "rounds": args.rounds,
        "serve_routed_ms": round(statistics.median(times["a"]) * 1e3, 2),
        "serve_routed_ms_min_max": [round(min(times["a"]) * 1e3, 2), round(max(times["a"]) * 1e3, 2)],
        "answer_routed_host_validate_ms": round(statistics.median(times["b"]) * 1e3, 2),
        "answer_routed_host_validate_ms_min_max": [round(min(times["b"]) * 1e3, 2), round(max(times["b"]) * 1e3, 2)],
        "stages": stages(datagrams, addrs, tokens, args.rounds),
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
