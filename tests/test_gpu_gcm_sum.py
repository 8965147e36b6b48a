"""The seeded GHASH multiplies of the AES-GCM step loop (qpp_device.h:
gh5_pipeline sums its windows in even groups from an initial accumulator;
ghash_mul_lds5c(a, b, init) / ghash_mul_h4(a, b, .., init) return
init ^ (a ^ b) H^4, so that a step forms neither `acc ^ x0` nor `^ x1` on its
own) and the close-from-LDS form's interior loop, which runs two interior
steps per iteration while two remain.

A packet with a non-empty header takes S = ceil((n_c + 2) / 8) steps
(n_c = ceil(payload / 16)); after the peeled first step the loop counts k from
S - 1 down to 1, takes the paired interior body at k >= 4, the single one at
k = 3 and the general step below.  So S = 1, 2, 3 never reach an interior
step, S = 4 runs one, S = 5 one pair, S = 6 a pair and then a single one.

One pattern of ten 16-packet wave items, whose expected bytes and results the
C oracle computes once per suite:

  items 0-5  every packet of the item at the same S = 5, 6, 4, 3, 2, 1 (whole
             waves reach the paired body), payload lengths at both ends of the
             class, last blocks of 16, 1 and 15 bytes
  items 6-8  lengths on both sides of every boundary of S mixed within items
  item 9     lengths from several classes, 20 bytes to a full-size datagram

with header lengths 11 and 27 (Z without and with a multiply by H^1).  The
pattern is repeated to the smallest packet count that selects each two-block
form of k_gcm (as tests/test_gpu_gcm_interior.py does: close-from-LDS,
four-entry, 512-thread) and ends in an item of 5 packets (S = 5).  The
unprotect also runs on a copy with one flipped ciphertext bit in an interior
block of some packets, which must fail the tag.  A child process runs the
one-block form (QPP_GCM_BPL=1), which shares the multiply.
"""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_gpu_close_lds import LONE_MAX, _counter, _keys, _run
from tests.test_gpu_gcm_interior import _geometry, _repeat_desc, interior_blocks

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("wg512", "four", "lds")
SUITES = [0, 1]
SUITE_IDS = ["aes128", "aes256"]
LONG = 1173  # payload of a full-size datagram
TAIL = 5  # packets of the launch's last item


def _class_lengths(S):
    """Payload lengths of S steps under a non-empty header: n_g = n_c + 2 at
    both ends of 8 S - 7 .. 8 S (n_c >= 2), last blocks of 16, 1 and 15 bytes."""
    lens = []
    for n_g in (max(8 * S - 7, 4), 8 * S):
        n_c = n_g - 2
        lens += [16 * n_c, 16 * (n_c - 1) + 1, 16 * (n_c - 1) + 15]
    for plen in lens:
        assert _geometry(11, plen)[1] == S and _geometry(27, plen)[1] == S
    return lens


def _shape():
    """(header length, payload length) of the pattern's 160 packets."""
    shape = []
    for S in (5, 6, 4, 3, 2, 1):
        lens = _class_lengths(S)
        shape += [((11, 27)[(i // 2) % 2], lens[i % 6]) for i in range(16)]
    combos = [(h, p) for h in (11, 27) for S in range(1, 7) for p in _class_lengths(S)]
    assert len(combos) == 72
    shape += [combos[(11 * i) % 72] for i in range(48)]
    shape += [((11, 27)[i % 2], (LONG, 20, 700, 40, 300, LONG, 520, 1000)[i % 8]) for i in range(16)]
    assert len(shape) == 160 and {_geometry(h, p)[1] for h, p in shape} >= {1, 2, 3, 4, 5, 6}
    assert all(_geometry(h, p)[1] == 5 for h, p in shape[:TAIL])
    return shape


@functools.lru_cache(maxsize=None)
def _pattern(suite):
    """The pattern's inputs and the oracle's outputs, computed once: protect,
    unprotect, and unprotect with one flipped ciphertext bit, inside a block
    that an interior step processes, in every packet that has such a block and
    whose index is 1 or 2 mod 4."""
    from aioquic_amd.batch import layout_packets
    from oracle import oracle as orc

    orc.lib()
    rng = np.random.default_rng(0x2150 + suite)
    recs = _keys(suite)
    shape = _shape()
    headers, payloads, pns = [], [], []
    for i, (hlen, plen) in enumerate(shape):
        pn_len = 1 + i % 4
        pn = int(rng.integers(0, 1 << 30))
        first = (0xC0 if hlen > 25 else 0x40) | (pn_len - 1)
        headers.append(bytes([first]) + rng.bytes(hlen - 1 - pn_len) +
                       (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big"))
        payloads.append(rng.bytes(plen))
        pns.append(pn)
    inbuf, desc, size = layout_packets(headers, payloads, pns, [0] * len(shape), align=1)
    ud = desc.copy()
    ud["len"] = [len(h) + len(p) + 16 for h, p in zip(headers, payloads)]
    ud["hdr_len"] = [len(h) - ((h[0] & 3) + 1) for h in headers]
    ud["pn"] = np.asarray(pns, np.uint64)
    wire, res = orc.protect_batch(recs, desc, inbuf, size)
    assert (res["status"] == 0).all() and (res["out_len"] == ud["len"]).all()
    plain, ures = orc.unprotect_batch(recs, ud, wire, size)
    assert (ures["status"] == 0).all()
    tampered = wire.copy()
    bad = {}
    for p, (hlen, plen) in enumerate(shape):
        # past the header-protection sample (the first 20 ciphertext bytes)
        blocks = [j for j in interior_blocks(hlen, plen) if j >= 2]
        if blocks and p % 4 in (1, 2):
            j = blocks[(3 * p) % len(blocks)]
            assert 16 * j + 16 <= plen
            tampered[int(desc[p]["out_off"]) + hlen + 16 * j + p % 16] ^= 1 << (p % 8)
            bad[p] = j
    # in the last item too, and at S = 4, 5 and 6 (a single interior step, a pair, both)
    assert any(p < TAIL for p in bad) and {_geometry(*shape[p])[1] for p in bad} >= {4, 5, 6}
    bres = orc.unprotect_batch(recs, ud, tampered, size)[1]
    covered = np.zeros(size, bool)  # the bytes an unprotect defines
    wiped = np.zeros(size, bool)  # payloads of the packets that fail
    for p, (hlen, plen) in enumerate(shape):
        o = int(desc[p]["out_off"])
        covered[o : o + hlen + plen] = True
        if p in bad:
            wiped[o + hlen : o + hlen + plen] = True
    # the bytes of the first TAIL packets: the launch's last, partial copy
    span = np.zeros(size, bool)
    span[: int(desc[TAIL]["out_off"])] = True
    assert int(desc[TAIL]["in_off"]) == int(desc[TAIL]["out_off"])
    return dict(recs=recs, shape=shape, inbuf=inbuf, desc=desc, ud=ud, size=size, wire=wire, res=res, plain=plain,
                ures=ures, tampered=tampered, bad=bad, bres=bres, covered=covered, wiped=wiped, span=span)


def gcm_sum_check(form, suite, tag=""):
    """The pattern repeated to the form's smallest launch plus an item of
    TAIL packets: protect, unprotect, and unprotect of the tampered copy, byte
    for byte and result for result against the oracle."""
    import torch

    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    torch.cuda.set_device(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    b = _pattern(suite)
    per = len(b["shape"])
    bpl1 = os.environ.get("QPP_GCM_BPL") == "1"
    # launch_packets: past the lone kernels; the 512-thread shape up to 16 items per CU
    least = 16 * 16 * cus + 1 if form == "lds" and not bpl1 else LONE_MAX + 1
    reps = -(-least // per)
    n = reps * per + TAIL
    assert form == "lds" or n <= 16 * 16 * cus
    size = (reps + 1) * b["size"]

    def tile(a):
        return np.tile(a, reps + 1)

    def rows(a):  # per-packet arrays
        return np.concatenate([np.tile(a, reps), a[:TAIL]])

    def descs(d):
        return _repeat_desc(d, reps + 1, b["size"])[:n]

    live = tile(np.ones(b["size"], bool))
    live[reps * b["size"] :] = b["span"]
    eng = PacketEngine(2)
    eng.set_key_records(b["recs"][: 2 if form == "four" else 1])
    count = _counter()
    c0 = count()
    wire, res = _run(eng, True, descs(b["desc"]), n, tile(b["inbuf"]), size)
    plain, ures = _run(eng, False, descs(b["ud"]), n, tile(b["wire"]), size, fill=0xAA)
    tplain, tres = _run(eng, False, descs(b["ud"]), n, tile(b["tampered"]), size, fill=0xAA)
    assert count() - c0 == (3 if form == "lds" else 0)

    assert (res == rows(b["res"])).all()
    assert np.array_equal(wire[live], tile(b["wire"])[live])
    assert (ures == rows(b["ures"])).all()
    cov = tile(b["covered"]) & live
    assert np.array_equal(plain[cov], tile(b["plain"])[cov])
    # flipped bits: exactly those packets fail and leave no plaintext
    assert (tres == rows(b["bres"])).all()
    failed = np.zeros(per, bool)
    failed[list(b["bad"])] = True
    failed = rows(failed)
    assert ((tres["status"] == L.S_DECRYPT) == failed).all()
    assert ((tres["status"] == L.S_OK) == ~failed).all()
    wiped = tile(b["wiped"]) & live
    assert not tplain[wiped].any()
    good = cov & ~wiped
    assert np.array_equal(tplain[good], tile(b["plain"])[good])
    if tag:
        print("gcm_sum_check ok", tag)


@pytest.mark.parametrize("suite", SUITES, ids=SUITE_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_two_block_forms(form, suite):
    """Both directions and the tampered copy through each two-block form."""
    gcm_sum_check(form, suite)


def test_one_block_form():
    """QPP_GCM_BPL=1 (a child process: the library reads the switch once):
    the close-from-LDS form of the one-block step, both suites."""
    code = ("import sys; sys.path.insert(0, %r); from tests.test_gpu_gcm_sum import gcm_sum_check; "
            "gcm_sum_check('lds', 0, 'aes128 bpl1'); gcm_sum_check('lds', 1, 'aes256 bpl1')" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, QPP_GCM_BPL="1"), capture_output=True,
                       text=True, timeout=180)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "gcm_sum_check ok aes128 bpl1" in r.stdout and "gcm_sum_check ok aes256 bpl1" in r.stdout
