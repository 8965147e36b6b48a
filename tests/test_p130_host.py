"""CPU check of the Poly1305 limb code of the ChaCha20-Poly1305 kernels
(aioquic_amd/csrc/qpp_p130.h, built for the host here through
tests/p130_host.cc) against Python integers mod 2^130 - 5.  No tolerance.

The header's comments state limb bounds; the tests hold the code to them at
the bounds themselves:
  p130_mul    h limbs < 2^29, r limbs < 2^26 + 2^11;
  p130_mac    four products into one p130_carry, h limbs <= 2^27 + 2^14,
              r limbs < 2^26 + 2^11: no 64-bit column sum wraps;
  results     limbs < 2^26 but limb 1, which is < 2^26 + 2^8 (the bound that
              holds: the fold adds at most 5 (d4 >> 26) >> 26 <= 201 there);
  p130_finish any limbs up to 50 * 2^26 (a wave sum of up to ~50 lanes).
The Python restatements of tests/poly_cases.py (the crafted packets' model)
are held to the host build on the same inputs, limb for limb.
"""

import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import poly_cases as pc
from tests.poly_cases import M26, P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H_MUL = (1 << 29) - 1              # "h limbs < 2^29"
H_MAC = (1 << 27) + (1 << 14)      # the chunk sums' operand: a block plus a carried chain
R_MAX = (1 << 26) + (1 << 11) - 1  # "r limbs < 2^26 + 2^11"
OUT1 = (1 << 26) + (1 << 8)        # limb 1 of a p130_mul / p130_carry result stays below this
WAVE = 50 << 26                    # k_lone_chacha's wave sums


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("p130") / "libp130_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "p130_host.cc")], check=True)
    lib = ctypes.CDLL(so)
    vp, ci = ctypes.c_void_p, ctypes.c_int
    for name, args in (("mul", [vp, vp, vp, ci]), ("add", [vp, vp, vp, ci]), ("mac_carry", [vp, vp, ci, vp, vp, ci]),
                       ("block", [vp, vp, ci]), ("r", [vp, vp, ci]), ("finish", [vp, vp, vp, ci]),
                       ("horner", [ctypes.c_char_p, ctypes.c_char_p, ci, vp])):
        f = getattr(lib, "qpp_test_p130_" + name)
        f.argtypes, f.restype = args, None
    return lib


def _u32(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.uint64).astype(np.uint32))


def _mul(lib, hs, rs):
    h, r = _u32(hs), _u32(rs)
    out = np.zeros_like(h)
    lib.qpp_test_p130_mul(h.ctypes.data, r.ctypes.data, out.ctypes.data, len(hs))
    return out.tolist()


def _mac_carry(lib, hs, rs, k):
    """hs, rs: n groups of k limb vectors -> (column sums, carried limbs)"""
    h, r = _u32([x for g in hs for x in g]), _u32([x for g in rs for x in g])
    n = len(hs)
    cols = np.zeros((n, 5), np.uint64)
    out = np.zeros((n, 5), np.uint32)
    lib.qpp_test_p130_mac_carry(h.ctypes.data, r.ctypes.data, k, cols.ctypes.data, out.ctypes.data, n)
    return cols.tolist(), out.tolist()


def _finish(lib, hs, ss):
    h = _u32(hs)
    s = _u32([[(x >> (32 * i)) & 0xFFFFFFFF for i in range(4)] for x in ss])
    tag = np.zeros((len(hs), 4), np.uint32)
    lib.qpp_test_p130_finish(h.ctypes.data, s.ctypes.data, tag.ctypes.data, len(hs))
    return [sum(int(w) << (32 * i) for i, w in enumerate(t)) for t in tag]


def _horner(lib, key, msg):
    assert len(msg) % 16 == 0
    tag = ctypes.create_string_buffer(16)
    lib.qpp_test_p130_horner(key, msg, len(msg) // 16, tag)
    return tag.raw


def _grid(top, rng, n_random):
    """limb vectors on the grid {0, 1, 2^13, 2^25, 2^26 - 1, 2^26, top}: all
    limbs equal, one limb set in zeros and in all-top, single bits, all ones
    below 2^26, and random fill from the grid and from [0, top]"""
    vals = [0, 1, 1 << 13, 1 << 25, M26, 1 << 26, top]
    vals = [v for v in vals if v <= top]
    out = [[v] * 5 for v in vals]
    for i in range(5):
        for v in vals:
            for rest in (0, top):
                x = [rest] * 5
                x[i] = v
                out.append(x)
    for b in range(0, top.bit_length(), 3):
        if (1 << b) <= top:
            out += [[(1 << b) if j == i else 0 for j in range(5)] for i in range(5)]
    for _ in range(n_random):
        out.append([vals[int(k)] for k in rng.integers(0, len(vals), 5)])
        out.append([int(k) for k in rng.integers(0, top + 1, 5)])
    return out


def test_restatements_match_the_host_build(lib):
    """tests/poly_cases.py's p_block, p_r, p_add, p_mul, p_mac, p_carry and
    p_finish give the host build's limbs on the same inputs."""
    rng = np.random.default_rng(130)
    n = 400
    raw = [rng.bytes(16) for _ in range(n)] + [bytes(16), b"\xff" * 16, b"\x01" + bytes(15), bytes(15) + b"\x80"]
    buf = np.frombuffer(b"".join(raw), np.uint8).copy()
    out = np.zeros((len(raw), 5), np.uint32)
    lib.qpp_test_p130_block(buf.ctypes.data, out.ctypes.data, len(raw))
    assert out.tolist() == [pc.p_block(b) for b in raw]
    for b, l in zip(raw, out.tolist()):
        assert pc.value(l) == int.from_bytes(b, "little") + (1 << 128)
    lib.qpp_test_p130_r(buf.ctypes.data, out.ctypes.data, len(raw))
    assert out.tolist() == [pc.p_r(b) for b in raw]
    clamp = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    for b, l in zip(raw, out.tolist()):
        assert pc.value(l) == int.from_bytes(b, "little") & clamp and max(l) <= M26
    hs, rs = _grid(H_MUL, rng, n), _grid(R_MAX, rng, n)
    m = min(len(hs), len(rs))
    hs, rs = hs[:m], rs[:m]
    assert _mul(lib, hs, rs) == [pc.p_mul(h, r) for h, r in zip(hs, rs)]
    a, b = _u32(hs), _u32(rs)
    o = np.zeros_like(a)
    lib.qpp_test_p130_add(a.ctypes.data, b.ctypes.data, o.ctypes.data, m)
    assert o.tolist() == [pc.p_add(x, y) for x, y in zip(hs, rs)]
    h4 = _grid(H_MAC, rng, n)
    groups = len(h4) // 4
    gh = [h4[4 * i : 4 * i + 4] for i in range(groups)]
    gr = [[rs[(4 * i + j) % m] for j in range(4)] for i in range(groups)]
    cols, carried = _mac_carry(lib, gh, gr, 4)
    for hq, rq, c, o in zip(gh, gr, cols, carried):
        d = [0] * 5
        for h, r in zip(hq, rq):
            d = pc.p_mac(d, h, r)
        assert d == c and pc.p_carry(d) == o
    fin = _grid(WAVE, rng, n)
    ss = [int.from_bytes(rng.bytes(16), "little") for _ in fin]
    assert _finish(lib, fin, ss) == [pc.p_finish(h, s) for h, s in zip(fin, ss)]


def _fold(d):
    """what p130_carry's fold adds to limb 1 for the column sums d"""
    d0, d1, d2, d3, d4 = d
    d1 += d0 >> 26
    d2 += d1 >> 26
    d3 += d2 >> 26
    d4 += d3 >> 26
    return ((d4 >> 26) * 5 + (d0 & M26)) >> 26


def _check_result(o, want, where):
    assert pc.value(o) % P == want % P, where
    assert o[0] <= M26 and o[2] <= M26 and o[3] <= M26 and o[4] <= M26 and o[1] < OUT1, (where, o)


def test_mul_on_its_bound_grid(lib):
    """p130_mul at h limbs up to 2^29 - 1 and r limbs up to 2^26 + 2^11 - 1
    (s = 5 r at its maximum still a uint32): the product mod p, and the
    result's limb bound."""
    assert 5 * R_MAX < 1 << 32
    rng = np.random.default_rng(131)
    hs, rs = _grid(H_MUL, rng, 300), _grid(R_MAX, rng, 300)
    pairs = [(h, r) for h in hs[:60] for r in rs[:60]]
    pairs += list(zip(hs, rs * (len(hs) // len(rs) + 1)))
    pairs += [([H_MUL] * 5, [R_MAX] * 5), ([R_MAX] * 5, [R_MAX] * 5)]
    out = _mul(lib, [p[0] for p in pairs], [p[1] for p in pairs])
    worst = 0
    for (h, r), o in zip(pairs, out):
        _check_result(o, pc.value(h) * pc.value(r), (h, r))
        worst = max(worst, _fold(pc.p_mac([0] * 5, h, r)))
    # limb 1 is a 26-bit value plus the fold: the extreme operands reach its most
    assert worst == _fold(pc.p_mac([0] * 5, [H_MUL] * 5, [R_MAX] * 5)) < 1 << 8
    print("p130_mul: %d products, the fold adds at most %d to limb 1" % (len(pairs), worst))


def test_four_macs_into_one_carry_on_their_bound_grid(lib):
    """Four p130_mac into one p130_carry (a chunk's sum) with h limbs up to
    2^27 + 2^14 and r limbs up to 2^26 + 2^11 - 1: the 64-bit column sums equal
    the exact integer sums (nothing wraps), the carried value is the sum of the
    products mod p, and the result's limb bound holds."""
    rng = np.random.default_rng(132)
    hs, rs = _grid(H_MAC, rng, 400), _grid(R_MAX, rng, 400)
    gh, gr = [[[H_MAC] * 5] * 4], [[[R_MAX] * 5] * 4]
    for i in range(0, min(len(hs), len(rs)) - 3, 4):
        gh.append(hs[i : i + 4])
        gr.append(rs[i : i + 4])
        gh.append([hs[i]] * 4)          # the same extreme in all four products
        gr.append([rs[-1 - i]] * 4)
    cols, out = _mac_carry(lib, gh, gr, 4)
    worst = 0
    for hq, rq, c, o in zip(gh, gr, cols, out):
        exact = [0] * 5
        for h, r in zip(hq, rq):
            s = [0] + [5 * x for x in r[1:]]
            exact[0] += h[0] * r[0] + h[1] * s[4] + h[2] * s[3] + h[3] * s[2] + h[4] * s[1]
            exact[1] += h[0] * r[1] + h[1] * r[0] + h[2] * s[4] + h[3] * s[3] + h[4] * s[2]
            exact[2] += h[0] * r[2] + h[1] * r[1] + h[2] * r[0] + h[3] * s[4] + h[4] * s[3]
            exact[3] += h[0] * r[3] + h[1] * r[2] + h[2] * r[1] + h[3] * r[0] + h[4] * s[4]
            exact[4] += h[0] * r[4] + h[1] * r[3] + h[2] * r[2] + h[3] * r[1] + h[4] * r[0]
        assert c == exact and max(exact) < 1 << 61, (hq, rq)
        _check_result(o, sum(pc.value(h) * pc.value(r) for h, r in zip(hq, rq)), (hq, rq))
        worst = max(worst, _fold(exact))
    assert worst == _fold(cols[0]) < 1 << 8  # (the first group: every operand at its bound)
    print("p130_mac x 4 + p130_carry: %d sums, the fold adds at most %d to limb 1" % (len(gh), worst))


def test_add_is_limb_wise(lib):
    rng = np.random.default_rng(133)
    a, b = _grid(H_MUL, rng, 200), _grid(H_MUL, rng, 200)[::-1]
    x, y = _u32(a), _u32(b)
    o = np.zeros_like(x)
    lib.qpp_test_p130_add(x.ctypes.data, y.ctypes.data, o.ctypes.data, len(a))
    for p, q, r in zip(a, b, o.tolist()):
        assert r == [u + v for u, v in zip(p, q)] and pc.value(r) == pc.value(p) + pc.value(q)


# ---------------------------------------------------------- p130_finish ----

FAILING = ([1 << 26, M26, M26, 1, 0], [1 << 26, M26, M26, 3, 0], [(1 << 27) - 2, M26, M26, 1, 7],
           [1 << 26, M26, M26, 2, 0])


def _s_set(res, rng):
    """s values for a residue: none of the final add's word carries fires
    (0; the complement, sum 2^128 - 1), all three fire (all ones, when word 0
    of the residue is not zero; -res, the all-zero tag), random"""
    lo = res % (1 << 128)
    return [0, (1 << 128) - 1 - lo, (1 << 128) - 1, (-lo) % (1 << 128), int.from_bytes(rng.bytes(16), "little")]


def _check_finish(lib, hs, rng):
    """every h with every s of _s_set against (value mod p) + s mod 2^128;
    returns the set of word-carry patterns met"""
    rows, ss = [], []
    for h in hs:
        for s in _s_set(pc.value(h) % P, rng):
            rows.append(h)
            ss.append(s)
    got = _finish(lib, rows, ss)
    seen = set()
    bad = []
    for h, s, t in zip(rows, ss, got):
        res = pc.value(h) % P
        seen.add(tuple(pc.word_carries(res, s)))
        if t != (res + s) % (1 << 128):
            bad.append((h, s))
    assert not bad, "%d of %d wrong, first limbs %s s %#x" % (len(bad), len(rows), [hex(x) for x in bad[0][0]], bad[0][1])
    return seen


def test_finish_on_the_reported_inputs(lib):
    """The four inputs of the report (three wrong before the carry chain was
    completed, one right by luck of the OR)."""
    rng = np.random.default_rng(134)
    for h in FAILING:
        assert pc.second_carry(h)[0]
    assert _check_finish(lib, [list(h) for h in FAILING], rng) >= {(0, 0, 0), (1, 1, 1)}


# p130_finish's input ranges: h0 up to 2^27 with the other limbs < 2^26 + 2^14;
# the limb-wise sum of two p130_mul results as chacha_packet forms it (every
# limb < 2^27 + 2^9); k_lone_chacha's wave sum (every limb up to 50 * 2^26)
RANGES = [("narrow", 1 << 27, (1 << 26) + (1 << 14) - 1), ("chacha_packet", (1 << 27) + (1 << 9), (1 << 27) + (1 << 9)),
          ("k_lone_chacha", WAVE, WAVE)]


def _second_carry_inputs(top0, top):
    """finish inputs with h0 <= top0 and the other limbs <= top on which the
    second h1 -> h2 carry fires while h2 = 2^26 - 1"""
    k0 = top0 >> 26
    k = top >> 26
    h0s = sorted({1 << 26, (1 << 26) + 5, top0, M26 - 4, M26, (k0 << 26) | 1} | {j << 26 for j in (1, k0) if j})
    h1s = sorted({M26, M26 - 1, M26 - k0 + 1 if k0 > 1 else M26, (1 << 26) | M26 if top > (1 << 26) | M26 else M26,
                  ((k - 1) << 26) | M26 if k > 1 else M26})
    h2s = sorted({M26, M26 - 1, M26 - k + 1 if k > 1 else M26, ((k - 1) << 26) | M26 if k > 1 else M26,
                  ((k - 1) << 26) | (M26 - 1) if k > 1 else M26})
    h3s = sorted({0, 1, 2, 3, M26 - 1, M26, (1 << 26) | 1 if top > 1 << 26 else 1, top - 1, top})
    h4s = sorted({0, 1, 7, M26 - 1, M26, top})
    out = []
    for h in itertools.product(h0s, h1s, h2s, h3s, h4s):
        if h[0] <= top0 and max(h[1:]) <= top and pc.second_carry(h)[0]:
            out.append(list(h))
    return out


@pytest.mark.parametrize("caller,top0,top", RANGES)
def test_finish_where_the_second_carry_fires(lib, caller, top0, top):
    """Enumerates finish inputs on which the second h1 -> h2 carry fires while
    h2 = 2^26 - 1, with h3 odd and even at that point, at the input ranges
    RANGES."""
    rng = np.random.default_rng(135)
    hs = _second_carry_inputs(top0, top)
    odd = sum(pc.second_carry(h)[1] & 1 for h in hs)
    assert odd >= 100 and len(hs) - odd >= 100, (len(hs), odd)
    assert _check_finish(lib, hs, rng) >= {(0, 0, 0), (1, 1, 1)}
    print("%s: %d inputs with the second carry, %d with h3 odd" % (caller, len(hs), odd))


def _representations(v, top0, top):
    """Limb forms of every v + k p the ranges hold: the form with limbs 0..3
    below 2^26 and limb 4 taking the rest, and from it every subset of the four
    moves "limb i+1 gives one unit to limb i" (limb i += 2^26), applied from
    the top down, that stays in range (h0 <= top0, the others <= top)."""
    out = []
    k = 0
    while True:
        x = v + k * P
        base = [(x >> (26 * i)) & M26 for i in range(4)] + [x >> 104]
        if base[4] > top:
            break
        for moves in itertools.product((0, 1), repeat=4):
            h = list(base)
            ok = True
            for i in (3, 2, 1, 0):
                if moves[i]:
                    if h[i + 1] == 0:
                        ok = False
                        break
                    h[i + 1] -= 1
                    h[i] += 1 << 26
            if ok and h[0] <= top0 and max(h[1:]) <= top and h not in out:
                out.append(h)
        k = k + 1 if k < 3 else k * 2 + 1
    return out


@pytest.mark.parametrize("caller,top0,top", RANGES)
def test_finish_around_zero_and_p(lib, caller, top0, top):
    """The values 0..9, p - 6 .. p + 9 and 2^130 - 1 (both sides of the
    conditional subtract) in the limb forms of _representations, with s chosen
    so that every one of the final add's three word carries fires and so that
    none does."""
    rng = np.random.default_rng(136)
    hs = []
    for v in list(range(10)) + list(range(P - 6, P + 10)) + [(1 << 130) - 1]:
        reps = _representations(v, top0, top)
        assert len(reps) >= (2 if v else 1), v
        hs += reps
    assert _check_finish(lib, hs, rng) >= {(0, 0, 0), (1, 1, 1)}
    print("%s: %d limb forms" % (caller, len(hs)))


def test_finish_random(lib):
    rng = np.random.default_rng(137)
    hs = [[int(x) for x in rng.integers(0, t + 1, 5)] for t in (M26, 1 << 27, WAVE) for _ in range(3000)]
    _check_finish(lib, hs, rng)


# ------------------------------------------- RFC 8439 A.3's constructions ----


def _poly1305(key, msg):
    """RFC 8439 sec. 2.5.1 over integers (whole blocks)."""
    r = int.from_bytes(key[:16], "little") & 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
    s = int.from_bytes(key[16:], "little")
    acc = 0
    for i in range(0, len(msg), 16):
        acc = (acc + int.from_bytes(msg[i : i + 16], "little") + (1 << 128)) * r % P
    return ((acc + s) % (1 << 128)).to_bytes(16, "little")


def _landing(target):
    """whole blocks whose sum with their 2^128 bits is `target`: under r = 1
    the accumulator reaches it unreduced before the last multiply"""
    for k in range(1, 5):
        rem = target - (k << 128)
        if 0 <= rem <= k * ((1 << 128) - 1):
            out = []
            for _ in range(k):
                take = min(rem, (1 << 128) - 1)
                out.append(take.to_bytes(16, "little"))
                rem -= take
            return b"".join(out)
    raise AssertionError(target)


def edge_messages():
    """(name, 32-byte one-time key, message) in the manner of RFC 8439
    Appendix A.3, described by what they do; the expected tags come from the
    integer definition."""
    ff = (1 << 128) - 1
    out = []
    for r in (1, 2):
        for s in (0, ff, 1):
            key = r.to_bytes(16, "little") + s.to_bytes(16, "little")
            for n in (1, 2, 3, 4, 7):
                out.append(("r=%d s=%#x, %d all-ff blocks" % (r, s, n), key, b"\xff" * (16 * n)))
    for name, t in (("p", P), ("p-1", P - 1), ("p+1", P + 1), ("2^130-1", (1 << 130) - 1), ("2^128", 1 << 128),
                    ("2^130", 1 << 130), ("2p-1", 2 * P - 1)):
        for s in (0, ff, 5):
            key = (1).to_bytes(16, "little") + s.to_bytes(16, "little")
            out.append(("accumulator lands on %s, s=%#x" % (name, s), key, _landing(t)))
            # and goes on from there: one more block after the edge
            out.append(("accumulator passes %s, s=%#x" % (name, s), key, _landing(t) + (3).to_bytes(16, "little")))
    # r at its clamped maximum with all-ff blocks: the largest products
    key = b"\xff" * 32
    out.append(("r and s all ones (clamped), 5 all-ff blocks", key, b"\xff" * 80))
    return out


def test_rfc8439_edge_constructions(lib, oracle):
    """Three voices on each message: the limb primitives in a plain Horner
    loop, the oracle's radix-2^64 Poly1305 (qo_poly1305) and the integer
    definition."""
    msgs = edge_messages()
    assert len(msgs) >= 70
    for name, key, msg in msgs:
        want = _poly1305(key, msg)
        assert _horner(lib, key, msg) == want, name
        assert oracle.poly1305(key, msg) == want, name
    # s = 2^128 - 1 over a residue of 1 wraps the tag to zero
    key = (1).to_bytes(16, "little") + b"\xff" * 16
    assert _poly1305(key, _landing(P + 1)) == bytes(16)
