"""Every payload length through every packet-kernel form launch_packets can
choose, byte for byte against the C oracle (oracle.protect_batch /
oracle.unprotect_batch).  No tolerance anywhere.

The sweep batch (sweep(), one per suite, the same geometry for all): for every
payload length 0..1500 five variants, kept where the packet fits 1500 bytes
and, with header protection, the sample fits (payload + packet number >= 4):
  0-2  short headers, packet-number lengths cycling 1..4, connection ids of
       0, 5, 8, 13, 14 or 20 bytes (headers of 2..25 bytes), spin bit = plen & 1;
  3    an Initial long header whose token pads it to 33, 47, 48, 49, 64 or 81
       bytes (3-6 associated-data blocks);
  4    QPP_F_NO_HP with 0, 1, 15, 16, 17, 32, 40, 48 or 65 bytes of associated
       data (no header protection, no Z block, the tiny loads).
The packets are shuffled with a fixed seed, so the 16 quads of a wave item run
unrelated step counts.  Packet i lies in its own 1600-byte cell of the input
buffer and of a separate output buffer, at offsets whose residues mod 16 are
independent ((5i+3) % 16 in, (7(i//16)+11i+1) % 16 out), with at least 48
bytes of guard on both sides; both buffers hold 0xA5 wherever no packet lies.
test_sweep_has_the_stated_geometry (CPU) asserts what this covers.

Three passes per form: protect; unprotect of the ORACLE's wire image into a
fresh 0xA5 buffer (expected packet number pn + i % 7); and unprotect of that
image with one flipped bit in every third packet (last ciphertext byte, last
tag byte, spin bit, cycling).  The whole output buffer is compared each time:
outside the packets' output extents it must still be 0xA5, a failed packet's
payload region must be zero (its header bytes are not compared) and the bytes
after it 0xA5.  The oracle's three passes are computed once per suite by a
module fixture and saved under pytest's temporary directory; child processes
load that file.

Forms, and what identifies them (launch_packets, qpp_engine.hip):
  lone     one unplanned launch of the batch, n <= lone_max(suite) = 8192:
           k_lone_gcm, one wave per packet                    [launch rule: lone_max]
  pair     consecutive launches of 8 descriptors, no sync between them:
           k_lone_gcm, two waves per packet (n <= 8)          [launch rule: k_lone_gcm's n <= 8]
  lone64   ChaCha20: consecutive launches of 64 descriptors: k_lone_chacha
                                                              [launch rule: lone_max = 64]
  prio     ChaCha20: one unplanned launch of the batch (> 64 packets, at most
           16 waves per CU): k_chacha, priority form          [launch rule: chacha_prio]
  quad1    child process with QPP_LONE=0, one key installed: k_gcm, 512
           threads, two blocks per lane (gcm_two_wg); with QPP_GCM_BPL=1 the
           1024-thread close-from-LDS form, one block         [counter: 0 / 3]
  quad2    the same child, a second key of the suite installed: k_gcm, 1024
           threads, four table entries                        [counter: 0; launch rule: n_suite == 2]
  planned  plan=eng.bucket(...), two slots (holding the same key material, so
           the oracle's bytes serve) with the packets alternating between
           them: k_gcm 1024 threads / k_chacha                [counter: 0]
  tiled    the descriptors tiled R times at offsets shifted by n * 1600, R the
           smallest with R * n > 16 * 16 * CUs, as one unplanned launch with
           one key: k_gcm close-from-LDS with two blocks per lane; k_chacha
           without priority                                   [counter: 3; launch rule: chacha_prio]
The counter is qpp_close_lds_launches(): its delta over a form's three
launches is 3 for the close-from-LDS forms and 0 for every other.
"""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.golden_cases import long_header, short_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUITE_NAMES = {0: "aes128", 1: "aes256", 2: "chacha"}
KEY_LEN = {0: 16, 1: 32, 2: 32}
S_OK, S_DECRYPT = 0, 2  # QPP_S_OK, QPP_S_DECRYPT
F_NO_HP = 1             # QPP_F_NO_HP
TAG = 16
PACKET_MAX = 1500
LONE_MAX = 8192         # lone_max(): unplanned AES-GCM launches up to here run one wave per packet
FILL = 0xA5
CELL, LEAD, PAD = 1600, 64, 24  # packet i starts at LEAD + CELL * i + PAD + residue
CIDS = (0, 5, 8, 13, 14, 20)
LONG_HDRS = (33, 47, 48, 49, 64, 81)
AADS = (0, 1, 15, 16, 17, 32, 40, 48, 65)


def _variants(rng, plen):
    """The up to five (header, flags, pn_len, pn) of one payload length."""
    out = []
    for v in range(5):
        pn = int(rng.integers(0, 1 << 30))
        if v < 3:
            pn_len = 1 + (plen + v) % 4
            cid = CIDS[(plen // 4 + 2 * v) % 6]
            hdr = short_header(rng.bytes(cid), pn, pn_len, 0, spin=plen & 1)
            assert len(hdr) == 1 + cid + pn_len
            flags = 0
        elif v == 3:
            pn_len = 1 + (plen + v) % 4
            want = LONG_HDRS[(plen + plen // 6) % 6]
            # 1 + 4 + (1 + 8) + (1 + 0) + (1 + token) + 2 + pn_len
            hdr = long_header(1, rng.bytes(8), b"", rng.bytes(want - 18 - pn_len), pn, pn_len, plen + TAG)
            assert len(hdr) == want and hdr[0] & 0x80
            flags = 0
        else:
            pn_len = 0
            # (payloads under 16 bytes: 0, 1 or 15 bytes, for the tiny loads)
            hdr = rng.bytes(AADS[(plen + plen // 9) % 9 if plen >= 16 else plen % 3])
            flags = F_NO_HP
        if len(hdr) + plen + TAG > PACKET_MAX or (not flags and plen + pn_len < 4):
            continue
        out.append((hdr, flags, pn_len, pn))
    return out


def _flip(k, hlen, plen, pn_len, flags):
    """(offset within the packet, bit) of the k-th tampered packet's flipped bit."""
    kind = k % 3
    if flags & F_NO_HP:
        if kind == 2 and hlen:
            return hlen - 1, 1 << (k % 8)            # the last associated-data byte
        return hlen + plen + TAG - 1, 1 << (k % 8)   # the last tag byte
    # kinds 0 and 1 must lie outside the header-protection sample (16 bytes
    # from the packet number's offset + 4), so the header parses as it did
    if kind == 0 and plen + pn_len < 21:
        kind = 1
    if kind == 1 and plen + pn_len < 5:
        kind = 2
    if kind == 0:
        return hlen + plen - 1, 1 << (k % 8)         # the last ciphertext byte
    if kind == 1:
        return hlen + plen + TAG - 1, 1 << (k % 8)   # the last tag byte
    return 0, 0x20                                   # the spin bit: header protection leaves it alone


@functools.lru_cache(maxsize=None)
def sweep():
    """The batch, without any key: a dict of per-packet arrays (shuffled order),
    the protect and unprotect descriptors, and the protect input buffer."""
    from oracle.oracle import DESC_DTYPE

    rng = np.random.default_rng(0x1E46785)
    pk = []
    for plen in range(PACKET_MAX + 1):
        for hdr, flags, pn_len, pn in _variants(rng, plen):
            pk.append((hdr, rng.bytes(plen), flags, pn_len, pn))
    order = np.random.default_rng(0x5AFF1E).permutation(len(pk))
    pk = [pk[j] for j in order]
    n = len(pk)
    i = np.arange(n, dtype=np.int64)
    in_off = LEAD + CELL * i + PAD + (5 * i + 3) % 16
    out_off = LEAD + CELL * i + PAD + (7 * (i // 16) + 11 * i + 1) % 16
    hlen = np.array([len(p[0]) for p in pk], np.int64)
    plen = np.array([len(p[1]) for p in pk], np.int64)
    flags = np.array([p[2] for p in pk], np.int64)
    pn_len = np.array([p[3] for p in pk], np.int64)
    pn = np.array([p[4] for p in pk], np.uint64)
    size = LEAD + CELL * n
    inbuf = np.full(size, FILL, np.uint8)
    for j, p in enumerate(pk):
        o = int(in_off[j])
        inbuf[o : o + len(p[0]) + len(p[1])] = np.frombuffer(p[0] + p[1], np.uint8)
    desc = np.zeros(n, DESC_DTYPE)
    desc["in_off"], desc["out_off"] = in_off, out_off
    desc["len"], desc["hdr_len"], desc["flags"], desc["pn"] = plen, hlen, flags, pn
    ud = desc.copy()
    ud["len"] = hlen + plen + TAG
    ud["hdr_len"] = hlen - pn_len
    # (QPP_F_NO_HP: the exact packet number)
    ud["pn"] = np.where(flags & F_NO_HP, pn, pn + (i % 7).astype(np.uint64))
    tampered = i % 3 == 0
    flip_at = np.zeros(n, np.int64)
    flip_bit = np.zeros(n, np.uint8)
    for k, j in enumerate(np.nonzero(tampered)[0]):
        flip_at[j], flip_bit[j] = _flip(k, int(hlen[j]), int(plen[j]), int(pn_len[j]), int(flags[j]))
    return dict(n=n, size=size, in_off=in_off, out_off=out_off, hlen=hlen, plen=plen, flags=flags, pn_len=pn_len,
                pn=pn, inbuf=inbuf, desc=desc, ud=ud, tampered=tampered, flip_at=flip_at, flip_bit=flip_bit)


def gcm_fast_hp(hlen, clen, bpl=2):
    """gcm_fast_hp (qpp_engine.hip) restated: protect with two blocks per lane
    takes the header-protection sample inside the first step."""
    if bpl != 2:
        return False
    n_a, n_c = (hlen + 15) >> 4, (clen + 15) >> 4
    za = 1 if n_a > 0 else 0
    qs = 4 * bpl
    n_g = za + n_c + 1
    pad = qs * ((n_g + qs - 1) // qs) - n_g
    return pad + za <= 6 and clen >= 19


def _keys(suite, same=False):
    """Two key records of the suite on slots 0 and 1; same: slot 1 holds slot
    0's key material (the planned form: two buckets, one oracle pass)."""
    from oracle.oracle import KEY_DTYPE

    rng = np.random.default_rng(0x1E46 + suite)
    recs = np.zeros(2, KEY_DTYPE)
    kl = KEY_LEN[suite]
    for s in range(2):
        recs[s]["slot"] = s
        recs[s]["suite"] = suite
        recs[s]["iv"] = np.frombuffer(rng.bytes(12), np.uint8)
        recs[s]["key"][:kl] = np.frombuffer(rng.bytes(kl), np.uint8)
        recs[s]["hp"][:kl] = np.frombuffer(rng.bytes(kl), np.uint8)
    if same:
        for f in ("iv", "key", "hp"):
            recs[1][f] = recs[0][f]
    return recs


def oracle_passes(suite):
    """The oracle's three passes over the sweep batch: the expected output
    buffers (0xA5 outside the packets' output extents), the result records,
    the two unprotect inputs and the tampered pass's comparison mask."""
    from oracle import oracle as orc

    orc.lib()
    b = sweep()
    n, size, in_off, out_off = b["n"], b["size"], b["in_off"], b["out_off"]
    hlen, plen = b["hlen"], b["plen"]
    recs = _keys(suite)[:1]
    wire_o, res = orc.protect_batch(recs, b["desc"], b["inbuf"], size)
    assert (res["status"] == S_OK).all() and (res["out_len"] == hlen + plen + TAG).all()
    exp_wire = np.full(size, FILL, np.uint8)
    wire_in = np.full(size, FILL, np.uint8)
    for j in range(n):
        o, i, ln = int(out_off[j]), int(in_off[j]), int(res[j]["out_len"])
        exp_wire[o : o + ln] = wire_o[o : o + ln]
        wire_in[i : i + ln] = wire_o[o : o + ln]
    plain_o, ures = orc.unprotect_batch(recs, b["ud"], wire_in, size)
    assert (ures["status"] == S_OK).all() and (ures["pn"] == b["pn"]).all()
    assert (ures["out_len"] == hlen + plen).all() and (ures["hdr_len"] == hlen).all()
    exp_plain = np.full(size, FILL, np.uint8)
    for j in range(n):
        o, i, ln = int(out_off[j]), int(in_off[j]), int(ures[j]["out_len"])
        exp_plain[o : o + ln] = plain_o[o : o + ln]
        assert np.array_equal(plain_o[o : o + ln], b["inbuf"][i : i + ln])  # the round trip
    tampered_in = wire_in.copy()
    for j in np.nonzero(b["tampered"])[0]:
        tampered_in[int(in_off[j]) + int(b["flip_at"][j])] ^= b["flip_bit"][j]
    tplain_o, tres = orc.unprotect_batch(recs, b["ud"], tampered_in, size)
    assert ((tres["status"] == S_DECRYPT) == b["tampered"]).all()
    assert ((tres["status"] == S_OK) == ~b["tampered"]).all()
    exp_tplain = exp_plain.copy()
    tmask = np.ones(size, np.uint8)
    for j in np.nonzero(b["tampered"])[0]:
        o, hl, pl = int(out_off[j]), int(hlen[j]), int(plen[j])
        tmask[o : o + hl] = 0              # a failed packet's header bytes are not compared
        exp_tplain[o : o + hl] = 0
        exp_tplain[o + hl : o + hl + pl] = 0  # no unauthenticated plaintext is left
    return dict(exp_wire=exp_wire, res=res, wire_in=wire_in, exp_plain=exp_plain, ures=ures,
                tampered_in=tampered_in, exp_tplain=exp_tplain, tres=tres, tmask=tmask)


# ------------------------------------------------------------ CPU tests ----


def test_sweep_has_the_stated_geometry():
    """(CPU) The batch is what the module docstring says it is."""
    b = sweep()
    n, hlen, plen, flags, pn_len = b["n"], b["hlen"], b["plen"], b["flags"], b["pn_len"]
    hp = (flags & F_NO_HP) == 0
    assert n <= LONE_MAX and (hlen + plen + TAG).max() == PACKET_MAX
    assert set(range(1471)) <= set(plen[hp].tolist())
    assert len(set(plen.tolist())) >= 1475
    assert (plen[hp] == 0).any() and (plen[~hp] == 0).any()
    assert (plen[hp] + pn_len[hp] >= 4).all()
    short = set(hlen[hp & (hlen < 26)].tolist())
    assert short == {1 + c + p for c in CIDS for p in (1, 2, 3, 4)} and min(short) == 2 and max(short) == 25
    assert {15, 16, 17} <= short  # either side of one associated-data block
    assert set(hlen[hp & (hlen > 26)].tolist()) == set(LONG_HDRS) and set(hlen[~hp].tolist()) == set(AADS)
    assert set(pn_len[hp].tolist()) == {1, 2, 3, 4}
    for hl in LONG_HDRS:  # every long-header length with every packet-number length
        assert set(pn_len[hp & (hlen == hl)].tolist()) == {1, 2, 3, 4}
    # every payload residue against every residue of the payload's position, in and out
    for off in (b["in_off"], b["out_off"]):
        assert len(set(zip((plen % 16).tolist(), ((off + hlen) % 16).tolist()))) == 256
    # in and out residues are independent: every pair occurs
    assert len(set(zip((b["in_off"] % 16).tolist(), (b["out_off"] % 16).tolist()))) == 256
    fast = np.array([gcm_fast_hp(int(h), int(c)) for h, c in zip(hlen, plen)])
    assert (fast & hp).sum() >= 1000 and (~fast & hp).sum() >= 1000
    # k_gcm's sequence [Z | CT | lengths]: every residue of its length mod 8 (two
    # blocks per lane) with a whole and with a partial tail block
    n_g = (hlen > 0).astype(np.int64) + (plen + 15) // 16 + 1
    assert len(set(zip((n_g % 8).tolist(), (plen % 16 == 0).tolist(), hp.tolist()))) == 32
    assert set(((hlen + 15) // 16).tolist()) == set(range(7))
    assert ((hlen + plen < 16)).sum() >= 10           # tiny (protect)
    assert ((hlen + plen < 16) & ~hp).sum() >= 4 and ((hlen + plen < 16) & hp).sum() >= 4
    # k_chacha: chunks = ceil(clen / 64), L = chunks mod 4, nb = blocks of the last chunk
    c = plen[plen > 0]
    chunks = (c + 63) // 64
    nb = (c - 64 * (chunks - 1) + 15) // 16
    assert len(set(zip((chunks % 4).tolist(), nb.tolist(), (c % 16 == 0).tolist()))) == 4 * 4 * 2
    # the lone kernels: positions l, l + 64, l + 128 -- one, two and three blocks per lane,
    # and a pair launch's split at position 64
    n_ac = (hlen + 15) // 16 + (plen + 15) // 16
    assert n_ac.min() == 0 and (n_ac <= 64).sum() > 1000 and (n_ac > 64).sum() > 1000 and n_ac.max() >= 93
    assert {63, 64, 65} <= set(n_ac.tolist())
    # every length class meets every position of an item
    for pos in range(16):
        at = np.arange(n) % 16 == pos
        assert len(set((plen[at] % 16).tolist())) == 16 and (~hp[at]).any() and (hlen[at] > 26).any()
    # own cells, guards of at least 48 bytes, either direction's extents
    ext = hlen + plen + TAG
    for off in (b["in_off"], b["out_off"]):
        assert (off >= LEAD + CELL * np.arange(n)).all() and (off + ext <= LEAD + CELL * (np.arange(n) + 1)).all()
        assert off[0] >= 48 and (off[1:] - (off + ext)[:-1] >= 48).all() and b["size"] - (off + ext)[-1] >= 48
    filled = np.ones(b["size"], bool)
    for o, h, p in zip(b["in_off"], hlen, plen):
        filled[o : o + h + p] = False
    assert (b["inbuf"][filled] == FILL).all()
    # the tampered pass: every third packet, all three kinds, each flip inside its packet
    t = b["tampered"]
    assert t.sum() == (n + 2) // 3
    assert ((b["flip_at"][t] >= 0) & (b["flip_at"][t] < ext[t])).all() and (b["flip_bit"][t] != 0).all()
    last_ct, last_tag = t & (plen > 0) & (b["flip_at"] == hlen + plen - 1), t & (b["flip_at"] == ext - 1)
    assert last_ct.sum() > 500 and last_tag.sum() > 500 and (t & hp & (b["flip_at"] == 0)).sum() > 500
    assert (plen[last_ct & hp] + pn_len[last_ct & hp] >= 21).all()
    assert (plen[last_tag & hp] + pn_len[last_tag & hp] >= 5).all()
    print("sweep: %d packets, %d tampered, %d distinct payload lengths" % (n, t.sum(), len(set(plen.tolist()))))


def test_oracle_accepts_the_sweep(oracle):
    """(CPU) ChaCha20-Poly1305 (the AES-GCM passes take seconds on the oracle's
    bitwise GHASH): every packet QPP_S_OK in both directions, exactly the
    tampered ones QPP_S_DECRYPT (asserted inside oracle_passes)."""
    e = oracle_passes(2)
    b = sweep()
    assert (e["exp_wire"] != FILL).sum() > b["n"] * 500 and not np.array_equal(e["wire_in"], e["tampered_in"])
    assert (e["tmask"] == 0).sum() == b["hlen"][b["tampered"]].sum()


# --------------------------------------------------------------- the check ----


def _counter():
    lib = ctypes.CDLL(os.path.join(ROOT, "aioquic_amd", "libquicpp.so"))
    lib.qpp_close_lds_launches.restype = ctypes.c_uint64
    return lib.qpp_close_lds_launches


def _describe(b, byte, side, chunk):
    """Names the packet of the output byte at `byte`: the nearest one, for a
    guard byte.  side: the pass; chunk: descriptors per launch (0 = all)."""
    n = b["n"]
    tile, best = divmod(max(0, byte - LEAD) // CELL, n)
    ext = b["hlen"] + b["plen"] + (TAG if side == "protect" else 0)

    def dist(j):
        o = int(b["out_off"][j]) + tile * n * CELL
        return 0 if o <= byte < o + int(ext[j]) else min(abs(byte - o), abs(byte - (o + int(ext[j]) - 1)))

    j = min((k for k in (best - 1, best, best + 1) if 0 <= k < n), key=dist)
    o = int(b["out_off"][j]) + tile * n * CELL
    return ("packet %d (tile %d): plen %d hdr_len %d pn_len %d flags %d in_off%%16 %d out_off%%16 %d, position %d of "
            "its item (in descriptor order), %d of its launch; byte %+d from the packet's start (extent %d%s)"
            % (j, tile, b["plen"][j], b["hlen"][j], b["pn_len"][j], b["flags"][j], b["in_off"][j] % 16,
               b["out_off"][j] % 16, j % 16, (tile * n + j) % chunk if chunk else tile * n + j, byte - o,
               ext[j], "" if dist(j) == 0 else ": a guard byte"))


FORMS = {
    # form: (keys installed, descriptors per launch or 0 = all, planned, tiled)
    "lone": (1, 0, False, False),
    "pair": (1, 8, False, False),
    "lone64": (1, 64, False, False),
    "prio": (1, 0, False, False),
    "quad1": (1, 0, False, False),
    "quad2": (2, 0, False, False),
    "planned": (2, 0, True, False),
    "tiled": (1, 0, False, True),
}


def lengths_check(path, suite, form, tag=""):
    """The whole check of one form (module docstring): three launches (or
    trains of launches) on device tensors through PacketEngine.protect /
    .unprotect, every output byte and result record against the oracle's
    passes saved at `path`.  Returns (packets compared per pass, packets
    failed by tampering)."""
    import torch

    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    assert (L.S_OK, L.S_DECRYPT, L.F_NO_HP, L.TAG_LEN, L.PACKET_MAX) == (S_OK, S_DECRYPT, F_NO_HP, TAG, PACKET_MAX)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    b = sweep()
    e = np.load(path)
    n, size = b["n"], b["size"]
    n_keys, chunk, planned, tiled = FORMS[form]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    env = os.environ.get
    lone_on = (env("QPP_LONE") or "1")[0] != "0"
    bpl1 = env("QPP_GCM_BPL") == "1"
    # the launcher's rules this form relies on (launch_packets): the switches are as the form needs them
    if form in ("lone", "pair", "lone64"):
        assert lone_on and n <= LONE_MAX and (suite == 2) == (form == "lone64")
    if form == "prio":
        assert suite == 2 and 64 < n and (n + 15) // 16 <= 16 * cus   # lone_max, chacha_prio
    if form in ("quad1", "quad2"):
        assert suite != 2 and not lone_on and (n + 15) // 16 <= 16 * cus  # gcm_two_wg
    reps = 1
    if tiled:
        reps = 16 * 16 * cus // n + 1
        assert reps * n > 16 * 16 * cus >= (reps - 1) * n and reps * n > LONE_MAX and not bpl1
    lds = (form == "quad1" and bpl1) or (tiled and suite != 2)
    total = reps * n

    recs = _keys(suite, same=planned)[:n_keys].astype(L.KEY_MATERIAL)
    eng = PacketEngine(2)
    eng.set_key_records(recs)

    def tile_desc(d):
        out = np.tile(d, reps)
        shift = np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(n * CELL), n)
        out["in_off"] += shift
        out["out_off"] += shift
        if planned:
            out["slot"] = np.arange(total) & 1
        return out

    def tile_buf(a):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
        return t if reps == 1 else torch.cat([t[:LEAD], t[LEAD:].repeat(reps)])

    count = _counter()
    c0 = count()
    failed = 0
    passes = (("protect", True, b["desc"], b["inbuf"], e["exp_wire"], e["res"], None),
              ("unprotect", False, b["ud"], e["wire_in"], e["exp_plain"], e["ures"], None),
              ("tampered unprotect", False, b["ud"], e["tampered_in"], e["exp_tplain"], e["tres"], e["tmask"]))
    for name, enc, desc, src, exp, exp_res, mask in passes:
        desc = tile_desc(desc)
        d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
        d_in, d_exp = tile_buf(src), tile_buf(exp)
        d_mask = tile_buf(mask).bool() if mask is not None else None
        d_out = torch.full((LEAD + CELL * total,), FILL, dtype=torch.uint8, device=dev)
        d_res = torch.full((total * 16,), 0xEE, dtype=torch.uint8, device=dev)
        assert d_in.numel() == d_out.numel() == d_exp.numel() == LEAD + CELL * total
        # every extent lies inside the buffers
        ext_in = desc["hdr_len"] + desc["len"] if enc else desc["len"]
        assert int((desc["in_off"] + ext_in).max()) <= d_in.numel()
        assert int((desc["out_off"] + np.tile(b["hlen"] + b["plen"] + TAG, reps)).max()) <= d_out.numel()
        run = eng.protect if enc else eng.unprotect
        plan = eng.bucket(d_desc, total) if planned else None
        step = chunk or total
        for at in range(0, total, step):  # (no sync between the launches of a train)
            k = min(step, total - at)
            run(d_desc[40 * at :], k, d_in, d_out, d_res[16 * at :], plan=plan)
        torch.cuda.synchronize()
        where = "%s %s %s" % (SUITE_NAMES[suite], form, name)
        res = d_res.cpu().numpy().view(L.RESULT)
        want = np.tile(exp_res, reps).astype(L.RESULT)
        bad = np.nonzero(res != want)[0]
        if len(bad):
            j = int(bad[0])
            o = int(desc[j]["out_off"])
            raise AssertionError("%s: %d result records differ, first %s: got %s, expected %s"
                                 % (where, len(bad), _describe(b, o, name, chunk), res[j], want[j]))
        ne = d_out != d_exp
        if d_mask is not None:
            ne &= d_mask
        if bool(ne.any()):
            at = int(ne.nonzero()[0, 0])
            raise AssertionError("%s: %d output bytes differ, first at %d: got 0x%02x, expected 0x%02x: %s"
                                 % (where, int(ne.sum()), at, int(d_out[at]), int(d_exp[at]),
                                    _describe(b, at, name, chunk)))
        if mask is not None:
            # exactly the tampered packets failed (the records equal the oracle's, which says so)
            assert ((res["status"] == S_DECRYPT) == np.tile(b["tampered"], reps)).all()
            assert ((res["status"] == S_OK) == ~np.tile(b["tampered"], reps)).all()
            failed = int((res["status"] == S_DECRYPT).sum())
        else:
            assert (res["status"] == S_OK).all()
        del d_in, d_exp, d_out, d_mask, ne
    ran = count() - c0
    assert ran == (3 if lds else 0), "close-from-LDS launches: %d, expected %d" % (ran, 3 if lds else 0)
    assert _crypto.watchdog_count() == 0
    print("lengths_check %s %s%s: %d packets compared per pass, %d failed by tampering, close-from-LDS launches %d"
          % (SUITE_NAMES[suite], form, " QPP_GCM_BPL=1" if bpl1 else "", total, failed, ran))
    if tag:
        print("lengths_check ok", tag)
    return total, failed


def _quad_child(path, suite, tag):
    """QPP_LONE=0: the unplanned batch through k_gcm, with one key installed and with two."""
    lengths_check(path, suite, "quad1")
    lengths_check(path, suite, "quad2", tag)


# ------------------------------------------------------------ GPU tests ----


@pytest.fixture(scope="module")
def expected(tmp_path_factory):
    """suite -> the .npz of the oracle's three passes, computed at first use."""
    d = tmp_path_factory.mktemp("lengths")

    @functools.lru_cache(maxsize=None)
    def get(suite):
        path = str(d / ("sweep_%s.npz" % SUITE_NAMES[suite]))
        np.savez(path, **oracle_passes(suite))
        return path

    return get


IN_PROCESS = [(s, f) for s in (0, 1) for f in ("lone", "pair", "planned", "tiled")] + \
             [(2, f) for f in ("lone64", "prio", "planned", "tiled")]


@pytest.mark.gpu
@pytest.mark.parametrize("suite,form", IN_PROCESS, ids=["%s-%s" % (SUITE_NAMES[s], f) for s, f in IN_PROCESS])
def test_lengths(expected, suite, form):
    """The forms an ordinary process reaches (module docstring): lone, pair /
    lone64, prio, planned, tiled."""
    total, failed = lengths_check(expected(suite), suite, form)
    n = sweep()["n"]
    assert total % n == 0 and failed == total // n * ((n + 2) // 3)


@pytest.mark.gpu
@pytest.mark.parametrize("suite", [0, 1], ids=["aes128", "aes256"])
@pytest.mark.parametrize("bpl", ["2", "1"], ids=["bpl2", "bpl1"])
def test_lengths_quad_unplanned(expected, bpl, suite):
    """k_gcm on the unplanned batch (QPP_LONE=0 in a child process: the
    library reads its switches once).  bpl2: 512 threads with one key
    installed, 1024 threads and four table entries with two; bpl1
    (QPP_GCM_BPL=1): the close-from-LDS form with one key, four entries with
    two.  One child per (switch set, suite)."""
    tag = "%s QPP_LONE=0 bpl%s" % (SUITE_NAMES[suite], bpl)
    code = ("import sys; sys.path.insert(0, %r); from tests.test_gpu_lengths import _quad_child; "
            "_quad_child(%r, %d, %r)" % (ROOT, expected(suite), suite, tag))
    env = dict(os.environ, QPP_LONE="0")
    env.pop("QPP_GCM_BPL", None)
    if bpl == "1":
        env["QPP_GCM_BPL"] = "1"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    print("".join(x + "\n" for x in r.stdout.splitlines() if x.startswith("lengths_check ")), end="")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "lengths_check ok " + tag in r.stdout
    assert r.stdout.count("lengths_check %s quad" % SUITE_NAMES[suite]) == 2
