"""Seeded inputs of `_crypto.walk_results` and the record of what it returns.

Shared by tests/golden/make_rx_walk.py (which writes tests/golden/rx_walk.json from
a built extension) and tests/test_rx_walk.py (which rebuilds the same inputs and
requires the same record).  walk_results launches nothing, so neither needs a GPU.

A case is 64 packets over 8 contexts: context x uses pair x and, mostly, space x;
contexts 0..5 belong to connection x, 6 and 7 to none.  Keeping a packet's pair,
space and connection together keeps one deferral from blocking the whole case.
"""

import hashlib
import random

import numpy as np

from aioquic_amd import layout as L

N_CASES = 500
N_PACKETS = 64
N_PAIRS = 8
N_SPACES = 8
N_CONNS = 6
NO_CONN = 0xFFFFFFFF

S_OK, S_LENGTH, S_DECRYPT, S_KEY_PHASE, S_NO_KEY = 0, 1, 2, 3, 4
S_RESERVED, S_CLOSED = 0x101, 0x102
# one letter per packet in the record
LETTER = {S_OK: "S", S_LENGTH: "L", S_DECRYPT: "X", S_KEY_PHASE: "P", S_NO_KEY: "K", S_RESERVED: "R", S_CLOSED: "C"}
DEFERRED = "D"


def _decode(trunc, bits, expected):
    """decode_packet_number (RFC 9000 A.3) of a number handed over as a signed C int."""
    if bits == 32 and trunc >= 1 << 31:
        trunc -= 1 << 32
    window = 1 << bits
    half = window // 2
    cand = (expected & ~(window - 1)) | trunc
    if cand <= expected - half and cand < (1 << 62) - window:
        cand += window
    elif cand > expected + half and cand >= window:
        cand -= window
    return max(cand, 0)


def case_inputs(seed):
    """-> the 15 arguments of walk_results for this seed."""
    rng = random.Random(seed)
    n = N_PACKETS
    space_exp = np.zeros(N_SPACES, "<u8")
    for s in range(N_SPACES):
        base = (0, 0, 1000, 1 << 16, (1 << 31) - 40, 1 << 40)[rng.randrange(6)]
        space_exp[s] = base + rng.randrange(300)
    closed = np.array([rng.random() < 0.08 for _ in range(N_CONNS)], "u1")
    nd = n + rng.randrange(5)
    dix = np.array(rng.sample(range(nd), n), "<u4")
    desc = np.zeros(nd, L.DESC)
    res = np.zeros(nd, L.RESULT)
    slots = np.zeros(n, "<u4")
    exp = np.zeros(n, "<u8")
    offs = np.zeros(n, "<u4")
    pair = np.zeros(n, "<u4")
    space = np.zeros(n, "<u4")
    conn = np.zeros(n, "<u4")
    track = np.zeros(n, "u1")
    rsv = np.zeros(n, "u1")
    out = bytearray(rng.randrange(8))  # the first packet need not start the output
    true_pn = [int(x) for x in space_exp]
    for i in range(n):
        ctx = rng.randrange(N_PAIRS)
        pair[i] = ctx
        space[i] = ctx if rng.random() < 0.9 else rng.randrange(N_SPACES)
        conn[i] = ctx if ctx < N_CONNS and rng.random() < 0.95 else NO_CONN
        track[i] = rng.random() < 0.9
        rsv[i] = (0x18, 0x18, 0x18, 0x0C, 0x0C, 0)[rng.randrange(6)]
        slots[i] = NO_CONN if rng.random() < 0.04 else rng.randrange(64)
        sp = int(space[i])
        exp[i] = space_exp[sp]
        step = rng.randrange(3) if rng.random() < 0.95 else (100, 200, 40000)[rng.randrange(3)]
        true_pn[sp] += step
        pn_len = 1 + rng.randrange(4)
        offs[i] = 0xFFFF if rng.random() < 0.02 else 1 + rng.randrange(30)
        u = rng.random()
        status = (S_OK if u < 0.90 else S_DECRYPT if u < 0.95 else S_KEY_PHASE if u < 0.956 else
                  S_NO_KEY if u < 0.978 else S_LENGTH)
        r = res[dix[i]]
        r["status"] = status
        r["pn"] = _decode(true_pn[sp] & ((1 << (8 * pn_len)) - 1), 8 * pn_len, int(exp[i]))
        hdr_len = (int(offs[i]) if offs[i] != 0xFFFF else 7) + pn_len
        r["hdr_len"] = hdr_len
        desc[dix[i]]["out_off"] = len(out)
        if status == S_OK:
            body = bytearray(rng.randbytes(hdr_len + rng.randrange(40)))
            body[0] &= ~int(rsv[i]) & 0xFF
            if rng.random() < 0.03:
                body[0] |= int(rsv[i]) & -int(rsv[i])  # the mask's lowest bit
            r["out_len"] = len(body)
            out += body
    return (slots.tobytes(), exp.tobytes(), offs.tobytes(), pair.tobytes(), space.tobytes(), track.tobytes(),
            space_exp.tobytes(), N_PAIRS, conn.tobytes(), rsv.tobytes(), closed.tobytes(), desc.tobytes(),
            res.tobytes(), dix.tobytes(), bytes(out))


def record(returned):
    """What the golden file keeps of walk_results' return value."""
    outs, res, deferred, space_exp, closed = returned
    status = np.frombuffer(res, L.RESULT)["status"]
    held = set(deferred)
    assert list(deferred) == sorted(held)
    h = hashlib.sha256()
    verdict = []
    for i, o in enumerate(outs):
        if i in held:
            assert o is None
            verdict.append(DEFERRED)
            continue
        assert (o is not None) == (status[i] == S_OK)
        if o is not None:
            header, payload, pn = o
            h.update(header + payload + int(pn).to_bytes(8, "little"))
        verdict.append(LETTER.get(int(status[i]), "?"))
    return {"verdict": "".join(verdict),
            "space_exp": [int(x) for x in np.frombuffer(space_exp, "<u8")],
            "closed": "".join(str(int(x)) for x in np.frombuffer(closed, "u1")),
            "sha256": h.hexdigest()}
