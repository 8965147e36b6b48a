"""The interior step of the two-block AES-GCM step loop (qpp_engine.hip,
gcm_packet): a wave whose active lanes all hold two whole ciphertext blocks,
after the first step and at least three steps from the end, runs a
straight-line body; any other wave-step runs the general one.

A packet's sequence [pad | Z | CT | lengths] has n_g = 1 + n_c + 1 blocks
(n_c = ceil(payload / 16), Z for a non-empty header) and takes
S = ceil(n_g / 8) steps, so the step count changes at n_g = 16 | 17, 24 | 25 and
32 | 33.  The batches here put payload lengths on both sides of those
boundaries, 16 packets of very different lengths in one wave item (so that
in one iteration every active lane is interior and in the next not, and short
packets end while long ones go on), long headers, and flipped ciphertext bytes
inside blocks that an interior step processes.

Every batch is a pattern of a few 16-packet items whose expected bytes and
results the C oracle computes once per suite; the pattern is repeated to the
smallest packet count that selects each form of k_gcm (launch_packets):

  wg512   one key of the suite, 8,193..16 x 16 x CUs packets: two 512-thread
          workgroups per CU, at most one item per wave
  four    two keys of the suite, past 8,192 packets: the four-entry
          1024-thread form
  lds     one key of the suite, past 16 items per CU: the close-from-LDS form
          (the library's launch counter says that it ran)

A repeated packet has the same key, number, header and payload, hence the
same bytes at its own offsets.  The one-block form (QPP_GCM_BPL=1) has no
interior step; tests/test_gpu_close_lds.py and tests/test_gpu_parity.py run it.
"""

import functools

import numpy as np
import pytest

from tests.test_gpu_close_lds import LONE_MAX, _counter, _keys, _run

pytestmark = pytest.mark.gpu

FORMS = ("wg512", "four", "lds")
SUITES = [0, 1]
SUITE_IDS = ["aes128", "aes256"]
LONG = 1173  # payload of a full-size datagram: 1200 bytes with an 11-byte header and the tag


def _geometry(hlen, plen):
    """(q, S) of gcm_packet with two blocks per lane: CT block j sits at
    sequence position q + j, the packet takes S steps of 8 positions."""
    za = 1 if hlen > 0 else 0
    n_c = (plen + 15) // 16
    n_g = za + n_c + 1
    pad = -n_g % 8
    return pad + za, (n_g + pad) // 8


def interior_blocks(hlen, plen):
    """CT blocks that interior steps process: steps 1 .. S - 3 (countdown
    k = S - step >= 3), positions 8 step .. 8 step + 7."""
    q, S = _geometry(hlen, plen)
    return [j for step in range(1, S - 2) for j in range(8 * step - q, 8 * step - q + 8)]


def _boundary_packets():
    """11-byte headers; n_g = 16, 17, 24, 25, 32, 33, each with a tail of 0, 1
    and 15 bytes in its last ciphertext block: 18 lengths, cycled over three
    items so that each meets several positions of an item."""
    lens = []
    for n_g in (16, 17, 24, 25, 32, 33):
        n_c = n_g - 2
        lens += [16 * n_c, 16 * (n_c - 1) + 1, 16 * (n_c - 1) + 15]
    for plen in lens:
        assert _geometry(11, plen)[1] == {16: 2, 17: 3, 24: 3, 25: 4, 32: 4, 33: 5}[1 + (plen + 15) // 16 + 1]
    return [(11, lens[(i + i // 16) % len(lens)]) for i in range(48)]


def _mixed_packets():
    """Full-size payloads among 20-, 40-, 300- and 700-byte ones: one long
    packet among short ones, one short among long ones, and two even mixes."""
    short = (20, 40, 300, 700)
    item_a = [short[i % 4] for i in range(16)]
    item_a[5] = LONG
    item_b = [LONG] * 16
    item_b[9] = 20
    item_c = [(LONG, 20, LONG, 40, 300, LONG, 700, LONG)[i % 8] for i in range(16)]
    item_d = [(700, 300, LONG, LONG, 40, 20, LONG, 300)[i % 8] for i in range(16)]
    return [(11, p) for p in item_a + item_b + item_c + item_d]


def _long_header_packets():
    """Associated data of 17, 33 and 47 bytes (Z takes 1, 2, 2 multiplies by
    H^1 before the first step) with long payloads."""
    return [((17, 33, 47, 11)[i % 4], (LONG, 700, LONG - 36, 1000)[(i // 4) % 4]) for i in range(16)]


PATTERNS = {"boundary": _boundary_packets, "mixed": _mixed_packets, "long_header": _long_header_packets}


@functools.lru_cache(maxsize=None)
def _pattern(kind, suite):
    """The pattern's inputs and the oracle's outputs, computed once: protect,
    unprotect, and unprotect with one flipped ciphertext byte, inside a block
    that an interior step processes, in every packet that has such a block and
    whose index is 1 or 2 mod 4."""
    from aioquic_amd.batch import layout_packets
    from oracle import oracle as orc

    orc.lib()
    rng = np.random.default_rng(0x17E0 + 16 * suite + sorted(PATTERNS).index(kind))
    recs = _keys(suite)
    shape = PATTERNS[kind]()
    assert len(shape) % 16 == 0
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
            at = 16 * j + p % 16
            tampered[int(desc[p]["out_off"]) + hlen + at] ^= 1 << (p % 8)
            bad[p] = at
    bres = orc.unprotect_batch(recs, ud, tampered, size)[1]
    covered = np.zeros(size, bool)
    for p, (hlen, plen) in enumerate(shape):
        o = int(desc[p]["out_off"])
        covered[o : o + hlen + plen] = True
    return dict(recs=recs, shape=shape, inbuf=inbuf, desc=desc, ud=ud, size=size, wire=wire, res=res, plain=plain,
                ures=ures, tampered=tampered, bad=bad, bres=bres, covered=covered)


def _repeat_desc(d, reps, size):
    out = np.tile(d, reps)
    shift = np.repeat(np.arange(reps, dtype=np.uint64) * np.uint64(size), len(d))
    out["in_off"] += shift
    out["out_off"] += shift
    return out


def _launch(form, b, what):
    """The pattern repeated to the form's smallest launch; `what` = the
    unprotect input ("wire" or "tampered").  Returns (reps, protect bytes,
    protect results, unprotect bytes, unprotect results)."""
    import torch

    from aioquic_amd.batch import PacketEngine

    torch.cuda.set_device(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    per = len(b["shape"])
    # launch_packets: past the lone kernels; the 512-thread shape up to 16 items per CU
    least = 16 * 16 * cus + 1 if form == "lds" else LONE_MAX + 1
    reps = -(-least // per)
    n = reps * per
    assert form == "lds" or n <= 16 * 16 * cus
    size = reps * b["size"]
    eng = PacketEngine(2)
    eng.set_key_records(b["recs"][: 2 if form == "four" else 1])
    count = _counter()
    c0 = count()
    wire, res = _run(eng, True, _repeat_desc(b["desc"], reps, b["size"]), n, np.tile(b["inbuf"], reps), size)
    plain, ures = _run(eng, False, _repeat_desc(b["ud"], reps, b["size"]), n, np.tile(b[what], reps), size, fill=0xAA)
    assert count() - c0 == (2 if form == "lds" else 0)
    return reps, wire, res, plain, ures


def _check_clean(form, b):
    """Both directions of the untouched pattern, byte for byte and result for
    result against the oracle."""
    reps, wire, res, plain, ures = _launch(form, b, "wire")
    assert (res == np.tile(b["res"], reps)).all()
    assert np.array_equal(wire, np.tile(b["wire"], reps))
    assert (ures == np.tile(b["ures"], reps)).all()
    cov = np.tile(b["covered"], reps)
    assert np.array_equal(plain[cov], np.tile(b["plain"], reps)[cov])


@pytest.mark.parametrize("suite", SUITES, ids=SUITE_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_boundary_lengths(form, suite):
    """Payload lengths on both sides of each step-count boundary, whole and
    partial last blocks."""
    _check_clean(form, _pattern("boundary", suite))


@pytest.mark.parametrize("suite", SUITES, ids=SUITE_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_mixed_wave_items(form, suite):
    """Items mixing full-size packets with 20-, 40-, 300- and 700-byte ones."""
    _check_clean(form, _pattern("mixed", suite))


@pytest.mark.parametrize("suite", SUITES, ids=SUITE_IDS)
@pytest.mark.parametrize("form", FORMS)
def test_long_headers(form, suite):
    """Headers of more than 16 bytes before long payloads: Z enters through
    the first step, the interior steps follow."""
    _check_clean(form, _pattern("long_header", suite))


@pytest.mark.parametrize("suite", SUITES, ids=SUITE_IDS)
@pytest.mark.parametrize("kind", ["boundary", "mixed"])
@pytest.mark.parametrize("form", FORMS)
def test_tampered_interior_block(form, kind, suite):
    """A flipped ciphertext byte in a block of an interior step: that packet
    fails authentication and leaves no plaintext; its neighbours are intact."""
    from aioquic_amd import layout as L

    b = _pattern(kind, suite)
    assert len(b["bad"]) >= 4
    reps, _, _, plain, ures = _launch(form, b, "tampered")
    assert (ures == np.tile(b["bres"], reps)).all()
    failed = np.zeros(len(b["shape"]), bool)
    failed[list(b["bad"])] = True
    failed = np.tile(failed, reps)
    assert ((ures["status"] == L.S_DECRYPT) == failed).all()
    assert ((ures["status"] == L.S_OK) == ~failed).all()
    good = b["covered"].copy()
    wiped = np.zeros(b["size"], bool)
    for p in b["bad"]:
        hlen, plen = b["shape"][p]
        o = int(b["desc"][p]["out_off"])
        wiped[o + hlen : o + hlen + plen] = True
        good[o : o + hlen + plen] = False
    assert not plain[np.tile(wiped, reps)].any()
    good = np.tile(good, reps)
    assert np.array_equal(plain[good], np.tile(b["plain"], reps)[good])
