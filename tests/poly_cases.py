"""Crafted ChaCha20-Poly1305 packets that land the kernels' Poly1305 on its
carry edges, and the limb-exact model that says so (CPU only; the GPU side is
tests/test_gpu_poly_edges.py, the primitives' own test tests/test_p130_host.py).

Restatements.  p_block .. p_finish restate aioquic_amd/csrc/qpp_p130.h over
Python integers with the C types' wrap-around (uint32 limbs, uint64 column
sums); tests/test_p130_host.py holds each of them to the header's host build on
the same inputs.  packet_close() and lone_close() restate, multiply for
multiply, how chacha_packet (k_chacha) and k_lone_chacha (qpp_engine.hip)
arrive at the five limbs they hand to p130_finish:
  packet  the quad's four chains (lane 0: associated data, lane j: chunks
          j - 1, j + 3, ..; per chunk four p130_mac by pw powers and one
          p130_carry), then p130_mul(quad_sum(u), r^(nb+1)) + quad_sum(v): the
          limb-wise sum of two p130_mul results, U' and V;
  lone    one lane per chunk / per four associated-data blocks / the lengths
          block, each lane's Horner value times r^e (prefix products over the
          wave), then the limb-wise sum of all lanes' p130_mul results.
Both return the summands, so the finish input is known exactly per packet.

Steering.  A tag's polynomial gives block i (of m, the lengths block last) the
coefficient r^(m-i), and every summand above is congruent to the part of that
polynomial over its own blocks.  One free 16-byte block X_j therefore moves
its summand to any residue t: X_j += (t - now) r^-(m-j) mod p, a valid block
when the result lies in [2^128, 2^129) (the 2^128 bit p130_block adds), about
one time in four.  r and s come from the oracle's ChaCha20 block 0 for the
key and nonce.  On a miss the packet number moves on by one and every other
block is drawn again from the seeded generator, at most CAP times.

Classes (CLASSES), each for both closes:
  a_odd / a_even  the finish input makes the second h1 -> h2 carry of the
          carry chain (after the fold of h4's carry into h0) fire while h2
          is 2^26 - 1, with h3 odd / even at that point.  The free block's
          summand is steered to limbs Y computed from the other summands'
          limb sum F, so that F + Y has the pattern; the model then confirms
          that the multiply really produced those limbs.
  b       the final residue is 0, 1, 2, 3, 4, p - 2 or p - 1 (both sides of the
          conditional subtract), one packet per residue and shape.
  c_zero  residue + s = 0 mod 2^128: all three word carries of the final add
          fire and the tag is sixteen zero bytes.
  c_carry residue words drawn so that all three word carries fire.
  d       every ciphertext and associated-data byte 0xff (no solve): maximal
          block limbs in the chunk sums.
Shapes (PAYLOADS): 0, 16, 40 and 64 bytes (one chunk; the header's chain is
the packet close's u), 128 (two chunks, one step), 320 (two steps: the
r^13..r^16 chunk sums), 1200.  Even packets of a cell carry a short header
with header protection where the payload holds the sample and the class does
not need the header (the free block is ciphertext); the others are AEAD-only
(QPP_F_NO_HP) with 16..48 bytes of associated data, whose blocks may be the
free one.

Cells that cannot exist (IMPOSSIBLE): a_odd / a_even with the packet close and
no payload.  There u is empty, the finish input is the single p130_mul result
V (limbs < 2^26, limb 1 < 2^26 + 2^8), and the second carry cannot fire: with
limb 1 >= 2^26 the masked limb is < 2^8, with limb 1 < 2^26 nothing carries
into h0 at all.
"""

import functools

import numpy as np

from tests.golden_cases import short_header

P = (1 << 130) - 5
M26 = (1 << 26) - 1
U32 = (1 << 32) - 1
U64 = (1 << 64) - 1
ONE = [1, 0, 0, 0, 0]
ZERO = [0, 0, 0, 0, 0]
F_NO_HP = 1
CHACHA = 2
CAP = 64          # outer attempts per packet (new packet number, new filler)
REDRAW = 48       # class a: draws of the free limbs per attempt

PAYLOADS = (0, 16, 40, 64, 128, 320, 1200)
CLOSES = ("packet", "lone")
CLASSES = ("a_odd", "a_even", "b", "c_zero", "c_carry", "d")
B_RESIDUES = (0, 1, 2, 3, 4, P - 2, P - 1)
IMPOSSIBLE = {
    ("a_odd", "packet", 0): "u is empty: the finish input is one p130_mul result, whose second carry cannot fire",
    ("a_even", "packet", 0): "u is empty: the finish input is one p130_mul result, whose second carry cannot fire",
}
PER_CELL = 4


# ------------------------------------------------- qpp_p130.h, restated ----


def value(h):
    return sum(x << (26 * i) for i, x in enumerate(h))


def limbs(x):
    """canonical limbs of x < 2^130"""
    return [(x >> (26 * i)) & M26 for i in range(5)]


def p_block(b16):
    x = int.from_bytes(b16, "little")
    w = [(x >> (32 * i)) & U32 for i in range(4)]
    return [w[0] & M26, ((w[0] >> 26) | (w[1] << 6)) & M26, ((w[1] >> 20) | (w[2] << 12)) & M26,
            ((w[2] >> 14) | (w[3] << 18)) & M26, (w[3] >> 8) | (1 << 24)]


def p_r(k16):
    x = int.from_bytes(k16, "little")
    k = [(x >> (32 * i)) & U32 for i in range(4)]
    k[0] &= 0x0FFFFFFF
    k[1] &= 0x0FFFFFFC
    k[2] &= 0x0FFFFFFC
    k[3] &= 0x0FFFFFFC
    return [k[0] & M26, ((k[0] >> 26) | (k[1] << 6)) & M26, ((k[1] >> 20) | (k[2] << 12)) & M26,
            ((k[2] >> 14) | (k[3] << 18)) & M26, k[3] >> 8]


def p_add(a, b):
    return [(x + y) & U32 for x, y in zip(a, b)]


def p_mac(d, h, r):
    """the five uint64 column sums d plus h * r"""
    r0, r1, r2, r3, r4 = r
    s1, s2, s3, s4 = (r1 * 5) & U32, (r2 * 5) & U32, (r3 * 5) & U32, (r4 * 5) & U32
    h0, h1, h2, h3, h4 = h
    return [(d[0] + h0 * r0 + h1 * s4 + h2 * s3 + h3 * s2 + h4 * s1) & U64,
            (d[1] + h0 * r1 + h1 * r0 + h2 * s4 + h3 * s3 + h4 * s2) & U64,
            (d[2] + h0 * r2 + h1 * r1 + h2 * r0 + h3 * s4 + h4 * s3) & U64,
            (d[3] + h0 * r3 + h1 * r2 + h2 * r1 + h3 * r0 + h4 * s4) & U64,
            (d[4] + h0 * r4 + h1 * r3 + h2 * r2 + h3 * r1 + h4 * r0) & U64]


def p_carry(d):
    d0, d1, d2, d3, d4 = d
    d1 = (d1 + (d0 >> 26)) & U64
    d2 = (d2 + (d1 >> 26)) & U64
    d3 = (d3 + (d2 >> 26)) & U64
    d4 = (d4 + (d3 >> 26)) & U64
    o = [d0 & M26, d1 & M26, d2 & M26, d3 & M26, d4 & M26]
    c = ((d4 >> 26) * 5 + o[0]) & U64
    o[0] = c & M26
    o[1] = (o[1] + (c >> 26)) & U32
    return o


def p_mul(h, r):
    return p_carry(p_mac([0, 0, 0, 0, 0], h, r))


def p_finish(h, s):
    """the tag as an integer < 2^128; s as an integer < 2^128"""
    h0, h1, h2, h3, h4 = h
    c = h1 >> 26; h1 &= M26; h2 = (h2 + c) & U32
    c = h2 >> 26; h2 &= M26; h3 = (h3 + c) & U32
    c = h3 >> 26; h3 &= M26; h4 = (h4 + c) & U32
    c = h4 >> 26; h4 &= M26; h0 = (h0 + c * 5) & U32
    c = h0 >> 26; h0 &= M26; h1 = (h1 + c) & U32
    c = h1 >> 26; h1 &= M26; h2 = (h2 + c) & U32
    c = h2 >> 26; h2 &= M26; h3 = (h3 + c) & U32
    c = h3 >> 26; h3 &= M26; h4 = (h4 + c) & U32
    c = h4 >> 26; h4 &= M26; h0 = (h0 + c * 5) & U32
    c = h0 >> 26; h0 &= M26; h1 = (h1 + c) & U32
    g0 = (h0 + 5) & U32; c = g0 >> 26; g0 &= M26
    g1 = (h1 + c) & U32; c = g1 >> 26; g1 &= M26
    g2 = (h2 + c) & U32; c = g2 >> 26; g2 &= M26
    g3 = (h3 + c) & U32; c = g3 >> 26; g3 &= M26
    g4 = (h4 + c - (1 << 26)) & U32
    if not g4 >> 31:
        h0, h1, h2, h3, h4 = g0, g1, g2, g3, g4
    w = [(h0 | (h1 << 26)) & U32, ((h1 >> 6) | (h2 << 20)) & U32, ((h2 >> 12) | (h3 << 14)) & U32,
         ((h3 >> 18) | (h4 << 8)) & U32]
    sw = [(s >> (32 * i)) & U32 for i in range(4)]
    f = w[0] + sw[0]
    t = f & U32
    f = w[1] + sw[1] + (f >> 32)
    t |= (f & U32) << 32
    f = w[2] + sw[2] + (f >> 32)
    t |= (f & U32) << 64
    t |= ((w[3] + sw[3] + (f >> 32)) & U32) << 96
    return t


def second_carry(h):
    """(the second h1 -> h2 carry fires while h2 = 2^26 - 1, h3 at that
    point) for a finish input h: the first carry pass h1 -> .. -> h4, the fold
    into h0, h0 -> h1, then the carry in question."""
    h0, h1, h2, h3, h4 = h
    c = h1 >> 26; h1 &= M26; h2 = (h2 + c) & U32
    c = h2 >> 26; h2 &= M26; h3 = (h3 + c) & U32
    c = h3 >> 26; h3 &= M26; h4 = (h4 + c) & U32
    c = h4 >> 26; h4 &= M26; h0 = (h0 + c * 5) & U32
    c = h0 >> 26; h1 = (h1 + c) & U32
    return (h1 >> 26) != 0 and h2 == M26, h3


def word_carries(res, s):
    """the three word carries of (res mod 2^128) + s"""
    f, out = 0, []
    for i in range(3):
        f = ((res >> (32 * i)) & U32) + ((s >> (32 * i)) & U32) + (f >> 32)
        out.append(f >> 32)
    return out


# ----------------------------------------------------------- the closes ----


def _pad16(b):
    return b + bytes(-len(b) % 16)


def blocks_of(data):
    data = _pad16(data)
    return [data[i : i + 16] for i in range(0, len(data), 16)]


def lens_block(hlen, clen):
    return hlen.to_bytes(8, "little") + clen.to_bytes(8, "little")


def packet_close(r16, aad, ct, hlen, clen):
    """chacha_packet's Poly1305: [U', V], the two p130_mul results whose limb
    sum goes to p130_finish.  aad / ct: lists of zero-padded 16-byte blocks."""
    r = p_r(r16)
    n_a, n_c = len(aad), len(ct)
    chunks = (clen + 63) >> 6
    steps = (chunks + 4) >> 2
    r2 = p_mul(r, r)
    r3, r4 = p_mul(r2, r), p_mul(r2, r2)
    r5, r8 = p_mul(r4, r), p_mul(r4, r4)
    r13 = p_mul(r8, r5)
    # pw: one, r .. r^5, r^8, then the chunk sums' r^13 .. r^16
    pw = [ONE, r, r2, r3, r4, r5, r8, p_mul(r13, ONE), p_mul(r13, r), p_mul(r13, r2), p_mul(r8, r8)]
    acc = [ZERO, ZERO, ZERO, ZERO]
    for g in range(n_a):
        acc[0] = p_mul(p_add(acc[0], p_block(aad[g])), r13 if (g == n_a - 1 and 3 < chunks) else r)
    for k in range(steps):
        for sub in range(4):
            c = 4 * k + sub - 1
            inc = 0 <= c < chunks
            nbv = min(4, n_c - 4 * c)
            d = [0, 0, 0, 0, 0]
            for b in range(4):
                valid = inc and b < nbv
                e = 0 if not inc else (16 - b if c + 4 < chunks else (nbv - b if valid else 0))
                m = p_block(ct[4 * c + b]) if valid else ZERO
                if b == 0:
                    m = p_add(m, acc[sub])
                d = p_mac(d, m, pw[e if e < 13 else e - 6])
            acc[sub] = p_carry(d)
    L = chunks & 3
    nb = n_c - 4 * (chunks - 1) if chunks > 0 else 1
    u, v = ZERO, ZERO
    for sub in range(4):
        role = (sub - L - 1) & 3
        a = p_add(acc[sub], p_block(lens_block(hlen, clen))) if role == 3 else acc[sub]
        m = p_mul(a, pw[(6, 4, 0, 1)[role]])
        if role == 3:
            v = p_add(v, m)
        else:
            u = p_add(u, m)
    return [p_mul(u, pw[1 + nb]), v]


def packet_group(n_a, n_c, clen):
    """summand (0: U', 1: V) of every sequence position [aad | ct | lens]"""
    chunks = (clen + 63) >> 6
    L = chunks & 3
    lane = [0] * n_a + [((i >> 2) + 1) & 3 for i in range(n_c)] + [L]
    return [1 if x == L else 0 for x in lane]


@functools.lru_cache(maxsize=8)
def _wave_powers(r16):
    """lane l's r^(l+1) as k_lone_chacha's prefix product leaves it"""
    tp = [p_r(r16)] * 64
    k = 1
    while k < 64:
        tp = [p_mul(tp[l], tp[l - k] if l >= k else ONE) for l in range(64)]
        k <<= 1
    return tp


def _lone_lanes(n_a, n_c, clen):
    """(lane, first position q, count) of k_lone_chacha's working lanes"""
    chunks = (clen + 63) >> 6
    m = n_a + n_c + 1
    out = []
    for lane in range(64):
        g, c0 = lane - 32, 4 * (lane - 1)
        if 1 <= lane <= chunks:
            out.append((lane, n_a + c0, min(4, n_c - c0)))
        elif g >= 0 and 4 * g < n_a:
            out.append((lane, 4 * g, min(4, n_a - 4 * g)))
        elif lane == 63:
            out.append((lane, m - 1, 1))
    return out


def lone_close(r16, aad, ct, hlen, clen):
    """k_lone_chacha's Poly1305: the working lanes' p130_mul results (idle
    lanes add zero limbs), whose limb sum over the wave goes to p130_finish."""
    r = p_r(r16)
    tp = _wave_powers(r16)
    r64 = tp[63]
    seq = aad + ct + [lens_block(hlen, clen)]
    m = len(seq)
    lanes = _lone_lanes(len(aad), len(ct), clen)
    # (an idle lane has e = 1, hi = 0: it never asks for the r^64 multiply)
    his = [(m - (q + cnt - 1) - 1) >> 6 for _, q, cnt in lanes]
    out = []
    for (lane, q, cnt), hi in zip(lanes, his):
        e1 = m - (q + cnt - 1) - 1
        re = tp[e1 & 63]
        for h in (1, 2, 3):
            if any(x >= h for x in his):
                re = p_mul(re, r64 if hi >= h else ONE)
        w = ZERO
        for b in range(cnt):
            w = p_add(w if b == 0 else p_mul(w, r), p_block(seq[q + b]))
        out.append(p_mul(w, re))
    return out


def lone_group(n_a, n_c, clen):
    grp = [0] * (n_a + n_c + 1)
    for k, (_, q, cnt) in enumerate(_lone_lanes(n_a, n_c, clen)):
        for b in range(cnt):
            grp[q + b] = k
    return grp


def limb_sum(parts):
    h = ZERO
    for x in parts:
        h = p_add(h, x)
    return h


def close_model(close, r16, aad, ct, hlen, clen):
    """(summands, summand index of every sequence position)"""
    if close == "packet":
        return packet_close(r16, aad, ct, hlen, clen), packet_group(len(aad), len(ct), clen)
    return lone_close(r16, aad, ct, hlen, clen), lone_group(len(aad), len(ct), clen)


def poly_residue(r, seq):
    """sum X_i r^(m-i) mod p over 16-byte blocks, each with its 2^128 bit"""
    h = 0
    for b in seq:
        h = (h + int.from_bytes(b, "little") + (1 << 128)) * r % P
    return h


# ------------------------------------------------------------ generator ----


def make_key():
    """the one key record every crafted packet is protected under"""
    rng = np.random.default_rng(0x9130)
    return rng.bytes(32), rng.bytes(12), rng.bytes(32)  # key, iv, hp


def nonce_of(iv, pn):
    return iv[:4] + (int.from_bytes(iv[4:], "big") ^ pn).to_bytes(8, "big")


def one_time_key(key, iv, pn):
    from oracle import oracle as orc

    return orc.chacha20_block(key, 0, nonce_of(iv, pn))[:32]


def keystream(key, iv, pn, n):
    from oracle import oracle as orc

    nonce = nonce_of(iv, pn)
    return b"".join(orc.chacha20_block(key, 1 + i, nonce) for i in range((n + 63) // 64))[:n]


def _solve(r, seq, j, delta):
    """block j of seq moved so that its coefficient's share changes by delta
    (mod p), or None when the result is no 16-byte block"""
    m = len(seq)
    x = (int.from_bytes(seq[j], "little") + (1 << 128) + delta * pow(r, -(m - j), P)) % P
    if not (1 << 128) <= x < (1 << 129):
        return None
    return (x - (1 << 128)).to_bytes(16, "little")


def _a_limbs(rng, F, odd):
    """limbs Y (a canonical residue) such that F + Y has the second-carry
    pattern with h3 of the wanted parity"""
    y1 = (M26 - F[1]) & M26
    c = (F[1] + y1) >> 26
    y2 = (M26 - F[2] - c) & M26
    c = (F[2] + y2 + c) >> 26
    y3 = int(rng.integers(0, 1 << 26))
    if ((F[3] + y3 + c) & 1) != odd:
        y3 ^= 1
    c = (F[3] + y3 + c) >> 26
    y4 = int(rng.integers(0, (1 << 26) - 1))
    c = (F[4] + y4 + c) >> 26
    lo = max(0, (1 << 26) - F[0] - 5 * c)
    y0 = int(rng.integers(lo, 1 << 26))
    return [y0, y1, y2, y3, y4]


def holds(cls, want, h, s):
    """the class predicate on a modelled finish input h (want: the class's
    target residue, where it has one)"""
    res = value(h) % P
    if cls in ("a_odd", "a_even"):
        fires, h3 = second_carry(h)
        return fires and (h3 & 1) == (cls == "a_odd")
    if cls == "b":
        return res == want and res in B_RESIDUES
    if cls == "c_zero":
        return (res + s) % (1 << 128) == 0 and word_carries(res, s) == [1, 1, 1]
    if cls == "c_carry":
        return word_carries(res, s) == [1, 1, 1] and (res + s) % (1 << 128) != 0
    return True


def _craft(rng, key, iv, cls, close, plen, k, want):
    """One packet of class cls for `close` (None: either), k-th of its cell.
    -> dict, or raises when CAP attempts did not do."""
    hp_ok = plen >= 16 and cls != "d"
    use_hp = hp_ok and k % 2 == 0
    pn_len = 1 + k % 4
    cid = rng.bytes((8, 5, 13, 20)[(k // 2) % 4])
    aad_len = (16, 32, 48, 20)[(k // 2 + plen // 16) % 4]
    pn0 = int(rng.integers(1 << 20, 1 << 30))
    n_c = (plen + 15) // 16
    full_ct = plen // 16
    for attempt in range(CAP):
        pn = pn0 + attempt
        hdr = short_header(cid, pn, pn_len, 0, spin=k & 1) if use_hp else rng.bytes(aad_len)
        ct = rng.bytes(plen)
        if cls == "d":
            hdr, ct = b"\xff" * len(hdr), b"\xff" * plen
        hlen = len(hdr)
        aad, ctb = blocks_of(hdr), blocks_of(ct)
        n_a = len(aad)
        otk = one_time_key(key, iv, pn)
        r16, s = otk[:16], int.from_bytes(otk[16:], "little")
        r = value(p_r(r16))
        seq = aad + ctb + [lens_block(hlen, plen)]
        free = [n_a + i for i in range(full_ct)]
        if not use_hp:
            free += [i for i in range(hlen // 16)]
        done = cls == "d"
        if cls in ("b", "c_zero", "c_carry"):
            if cls == "b":
                target = want
            elif cls == "c_zero":
                target = (-s) % (1 << 128) + (int(rng.integers(0, 4)) << 128)
            else:
                sw = [(s >> (32 * i)) & U32 for i in range(4)]
                if not (sw[0] and sw[1] and sw[2]):
                    continue
                w = [int(rng.integers((1 << 32) - sw[i], 1 << 32)) for i in range(3)] + [int(rng.integers(0, 1 << 32))]
                target = sum(x << (32 * i) for i, x in enumerate(w)) + (int(rng.integers(0, 4)) << 128)
            if target >= P:
                continue
            j = free[int(rng.integers(0, len(free)))]
            blk = _solve(r, seq, j, target - poly_residue(r, seq))
            if blk is not None:
                seq[j] = blk
                done = True
        elif cls in ("a_odd", "a_even"):
            j = free[int(rng.integers(0, len(free)))]
            parts, grp = close_model(close, r16, aad, ctb, hlen, plen)
            gi = grp[j]
            F = limb_sum(p for i, p in enumerate(parts) if i != gi)
            now = value(parts[gi]) % P
            for _ in range(REDRAW):
                y = _a_limbs(rng, F, cls == "a_odd")
                if value(y) >= P:
                    continue
                blk = _solve(r, seq, j, value(y) - now)
                if blk is None:
                    continue
                trial = list(seq)
                trial[j] = blk
                got, _ = close_model(close, r16, trial[:n_a], trial[n_a:-1], hlen, plen)
                # the multiply produced the limbs asked for, not another form of the residue
                if got[gi] == y and holds(cls, None, limb_sum(got), s):
                    seq = trial
                    done = True
                    break
        if not done:
            continue
        hdr = b"".join(seq[:n_a])[:hlen]
        ct = b"".join(seq[n_a:-1])[:plen]
        assert not use_hp or hdr == short_header(cid, pn, pn_len, 0, spin=k & 1)
        res = poly_residue(r, blocks_of(hdr) + blocks_of(ct) + [lens_block(hlen, plen)])
        fin = {c: limb_sum(close_model(c, r16, blocks_of(hdr), blocks_of(ct), hlen, plen)[0]) for c in CLOSES}
        plain = bytes(a ^ b for a, b in zip(ct, keystream(key, iv, pn, plen)))
        return dict(cls=cls, close=close, plen=plen, hdr=hdr, ct=ct, plain=plain, pn=pn, pn_len=pn_len if use_hp else 0,
                    flags=0 if use_hp else F_NO_HP, s=s, residue=res, want=want, fin=fin,
                    tag=((res + s) % (1 << 128)).to_bytes(16, "little"), attempts=attempt + 1)
    raise AssertionError("no packet of class %s, close %s, payload %d within %d attempts" % (cls, close, plen, CAP))


@functools.lru_cache(maxsize=None)
def crafted():
    """The crafted set: a list of packet dicts (hdr: the plaintext header or
    associated data, ct, plain, pn, pn_len, flags, tag: the integer
    definition's, fin[close]: the modelled finish input, cls / close / plen:
    the cell it was made for, close None: made for both)."""
    key, iv, _ = make_key()
    rng = np.random.default_rng(0xED6E5)
    out = []
    for plen in PAYLOADS:
        for cls in CLASSES:
            if cls in ("a_odd", "a_even"):
                for close in CLOSES:
                    if (cls, close, plen) in IMPOSSIBLE:
                        continue
                    out += [_craft(rng, key, iv, cls, close, plen, k, None) for k in range(PER_CELL)]
            elif cls == "b":
                out += [_craft(rng, key, iv, cls, None, plen, k, want) for k, want in enumerate(B_RESIDUES)]
            else:
                out += [_craft(rng, key, iv, cls, None, plen, k, None) for k in range(PER_CELL)]
    return out


def cells(pk):
    """(class, close, payload) -> the packets whose modelled finish input for
    that close satisfies the class predicate, among those made for the cell"""
    out = {(cls, close, plen): [] for cls in CLASSES for close in CLOSES for plen in PAYLOADS}
    for p in pk:
        for close in CLOSES:
            if p["close"] in (None, close) and holds(p["cls"], p["want"], p["fin"][close], p["s"]):
                out[(p["cls"], close, p["plen"])].append(p)
    return out


def describe(p, close):
    return ("class %s, close %s (made for %s), payload %d, header %d bytes (%s), pn %d, modelled finish limbs %s"
            % (p["cls"], close, p["close"] or "both", p["plen"], len(p["hdr"]),
               "AEAD-only" if p["flags"] else "short header", p["pn"],
               [hex(x) for x in p["fin"][close if close in CLOSES else "packet"]]))
