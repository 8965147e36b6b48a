#!/usr/bin/env python3
"""Initial keys for a burst of new connections (SURVEY.md sec. 8(a) row a12,
8(f) row 4): two ways of reaching the same key-table state, timed on a GPU box.
One process, one GPU.  Prints one JSON object (and writes it to --out).

For C connections x 2 versions (default 4096 x 2 = 8192 derivations, 16384
slots installed, the table of bench config 4):

  a  the way before qpp_keytab_derive_initial: HKDF-Extract and the
     "client in" / "server in" expands with stdlib hmac on the host
     (quic/crypto.py:201-227), then ONE qpp_keytab_derive of the 16384 secrets
  b  ONE qpp_keytab_derive_initial of the 8192 records

Wall time around the synchronous work of each way (the calls end in a stream
synchronise), the two ways alternating in one process, after --warmup rounds;
median and min of --runs rounds.  Building the record arrays from the CIDs /
secrets is outside both timings.  For b the durations of its two kernels come
from device events around them (qpp_keytab_derive_trace) in the same runs.
The two ways' key material is compared at the end: a mismatch fails the run.
"""

from __future__ import annotations

import argparse
import hashlib
import hmac
import json
import os
import signal
import statistics
import struct
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VERSION_1, VERSION_2 = 0x00000001, 0x6B3343CF
SALTS = {VERSION_1: bytes.fromhex("38762cf7f55934b34d179ae6a4c80cadccbb7f0a"),
         VERSION_2: bytes.fromhex("0dede3def700a6db819381be6e269dcbf9bd2ed9")}


def _expand_label(secret: bytes, label: bytes, length: int) -> bytes:
    full = b"tls13 " + label
    info = struct.pack("!HB", length, len(full)) + full + b"\x00"
    return hmac.new(secret, info + b"\x01", hashlib.sha256).digest()[:length]


def host_initial_secrets(cids, versions) -> list:
    """[client secret, server secret, ...] with stdlib hmac, two per connection."""
    out = []
    for cid, version in zip(cids, versions):
        root = hmac.new(SALTS[version], cid, hashlib.sha256).digest()
        out.append(_expand_label(root, b"client in", 32))
        out.append(_expand_label(root, b"server in", 32))
    return out


def _stats(xs):
    return {"median_ms": round(statistics.median(xs), 4), "min_ms": round(min(xs), 4),
            "max_ms": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--conns", type=int, default=4096)
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=300, help="seconds before the run gives up")
    ap.add_argument("--out", default=None, help="also write the JSON object to this file")
    a = ap.parse_args()
    if a.runs < 10:
        ap.error("--runs must be at least 10")
    signal.signal(signal.SIGALRM, lambda *_: sys.exit("bench_initial_keys: timed out"))
    signal.alarm(a.timeout)

    from aioquic_amd import layout as L
    from aioquic_amd._crypto import KeyTable

    rng = np.random.default_rng(12)
    n = 2 * a.conns  # derivations: every connection once per version
    cids = [rng.bytes(8) for _ in range(a.conns)] * 2
    versions = [VERSION_1] * a.conns + [VERSION_2] * a.conns
    v2 = np.asarray([v == VERSION_2 for v in versions])

    ini = np.zeros(n, dtype=L.INITIAL)
    ini["slot_client"] = np.arange(0, 2 * n, 2)
    ini["slot_server"] = np.arange(1, 2 * n, 2)
    ini["cid_len"] = 8
    ini["flags"] = np.where(v2, L.DERIVE_V2, 0)
    ini["cid"][:, :8] = np.frombuffer(b"".join(cids), dtype=np.uint8).reshape(n, 8)
    ini_bytes = ini.tobytes()

    sec = np.zeros(2 * n, dtype=L.SECRET)
    sec["slot"] = np.arange(2 * n)
    sec["suite"] = L.AES_128_GCM
    sec["secret_len"] = 32
    sec["flags"] = np.repeat(np.where(v2, L.DERIVE_V2, 0), 2)

    table = KeyTable(2 * n)
    table.derive_trace(1)
    t_a, t_a_hkdf, t_a_call, t_b, k_derive, k_setup = [], [], [], [], [], []
    km_a = km_b = None
    for r in range(a.warmup + a.runs):
        t0 = time.perf_counter()
        secrets = host_initial_secrets(cids, versions)
        t1 = time.perf_counter()
        sec["secret"][:, :32] = np.frombuffer(b"".join(secrets), dtype=np.uint8).reshape(2 * n, 32)
        sec_bytes = sec.tobytes()
        t2 = time.perf_counter()
        km_a = table.derive(sec_bytes)
        t3 = time.perf_counter()
        km_b, _ = table.derive_initial(ini_bytes)
        t4 = time.perf_counter()
        if r >= a.warmup:
            t_a_hkdf.append((t1 - t0) * 1e3)
            t_a_call.append((t3 - t2) * 1e3)
            t_a.append((t1 - t0 + t3 - t2) * 1e3)
            t_b.append((t4 - t3) * 1e3)
            d, k = table.derive_trace()
            k_derive.append(d)
            k_setup.append(k)
    same = km_a == km_b
    med_a, med_b = statistics.median(t_a), statistics.median(t_b)
    out = {
        "tool": "bench_initial_keys",
        "connections": a.conns, "derivations": n, "slots_installed": 2 * n,
        "runs": a.runs, "warmup": a.warmup,
        "a_host_hkdf_then_keytab_derive": dict(_stats(t_a), host_hkdf=_stats(t_a_hkdf),
                                               keytab_derive_call=_stats(t_a_call)),
        "b_keytab_derive_initial": dict(_stats(t_b), k_derive_initial_events=_stats(k_derive),
                                        k_key_setup_events=_stats(k_setup)),
        "a_over_b": round(med_a / med_b, 3),
        "same_key_material": bool(same),
    }
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not same:
        sys.exit("bench_initial_keys: the two ways' key material differs")


if __name__ == "__main__":
    main()
