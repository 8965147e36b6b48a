"""The step loop of the close-from-LDS form of k_gcm (unplanned 1024-thread
AES-GCM launches, two blocks per lane, one key of the suite in the table),
whose H^4 multiplies take their window addresses in one operation each from
the input split by window parity (qpp_gh5.h).  (The file is named for the
study it came with: the step's two multiplies as independent H^8 and H^4
products, which measured no faster and is not in the kernel, DESIGN.md sec. 4
Round 12.)

The smallest launch that takes the form (one packet past 16 items per CU, as
tests/test_gpu_close_lds.py computes it), both AES-GCM suites.  Payload lengths
cycle over 1..200 and 1100..1200 bytes, and over a few lengths of 225..353
bytes besides: with headers of HDR_LENS bytes the GHASH sequence then takes
1, 2, 3, 4 and 9-10 steps of 8 blocks, its front padding runs over 0..7
blocks (both classes of the first step), and packets of one, two and many
steps share every item.  Packet-number lengths 1-4.  Every packet, both
directions, against the reference's _crypto (tests/ref_crypto.py; the C oracle
where oracle/_ref is not built).  Then an unprotect with one bit flipped in
every 97th packet, and the same batch with a second key of the suite in the
table, which takes the four-entry kernel: the routing did not move.
"""

import functools

import numpy as np
import pytest

from tests.test_gpu_close_lds import HDR_LENS, _counter, _keys, _run

pytestmark = pytest.mark.gpu

PAYLOAD_LENS = tuple(range(1, 201)) + tuple(range(1100, 1201)) + (225, 240, 289, 352, 353)
EVERY = 97


def _n():
    import torch

    return 16 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 1


def steps(hlen, plen):
    """Steps of the two-blocks-per-lane loop and blocks of front padding (gcm_packet)."""
    n_g = (1 if hlen else 0) + (plen + 15) // 16 + 1
    s = (n_g + 7) // 8
    return s, 8 * s - n_g


@functools.lru_cache(maxsize=None)
def _batch(suite, n):
    from aioquic_amd.batch import layout_packets
    from aioquic_amd.bench_data import Workload
    from oracle import oracle as orc
    from tests import ref_crypto

    orc.lib()
    rng = np.random.default_rng(0x48AB + 16 * suite)
    recs = _keys(suite)
    cyc = len(PAYLOAD_LENS)
    headers, payloads, pns = [], [], []
    blob = rng.bytes(n * 64 + 4096)
    for i in range(n):
        # the cycle shifts by one each round, so every length meets every position of an item
        plen = PAYLOAD_LENS[(i + i // cyc) % cyc]
        hlen = HDR_LENS[(i // 3) % len(HDR_LENS)]
        pn_len = 4 if plen < 3 else 1 + i % 4  # the header-protection sample needs 4 bytes of number + payload
        pn = int(rng.integers(0, 1 << 30))
        first = (0xC0 if hlen > 25 else 0x40) | (pn_len - 1)
        at = 64 * i
        headers.append(bytes([first]) + blob[at : at + hlen - 1 - pn_len] +
                       (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big"))
        payloads.append(blob[at + 48 : at + 48 + plen])
        pns.append(pn)
    seen = {steps(len(h), len(p)) for h, p in zip(headers, payloads)}
    assert {1, 2, 3, 4, 9, 10} <= {s for s, _ in seen}
    assert {pad for _, pad in seen} == set(range(8))
    inbuf, desc, size = layout_packets(headers, payloads, pns, [0] * n, align=1)
    ud = desc.copy()
    ud["len"] = [len(h) + len(p) + 16 for h, p in zip(headers, payloads)]
    ud["hdr_len"] = [len(h) - ((h[0] & 3) + 1) for h in headers]
    ud["pn"] = np.asarray(pns, np.uint64)
    ref = ref_crypto.checker("tests/test_gpu_gcm_h8.py::_batch[%d-%d]" % (suite, n))
    if ref is not None:
        w = Workload(n=n, n_keys=2, keys=recs, desc=desc, udesc=ud, plain=inbuf, plain_size=size,
                     wire_size=size, suites=np.full(n, suite))
        wire = ref_crypto.protect_all(ref, w)
        plain, ref_pns = ref_crypto.unprotect_all(ref, w, wire)
        assert np.array_equal(ref_pns, ud["pn"])
    else:
        wire, res = orc.protect_batch(recs, desc, inbuf, size)
        assert (res["status"] == 0).all()
        plain = orc.unprotect_batch(recs, ud, wire, size)[0]
    # one flipped bit in every 97th packet: the last ciphertext byte, the last
    # tag byte or the connection id in turn, always outside the
    # header-protection sample (16 bytes from the packet number's offset + 4),
    # so the header parses as it did and the failure is the tag's
    bad = {}
    tampered = wire.copy()
    for k, p in enumerate(range(0, n, EVERY)):
        o, hl, pl = int(desc[p]["out_off"]), len(headers[p]), len(payloads[p])
        pn_len = (headers[p][0] & 3) + 1
        kind = ("ct", "tag", "hdr")[k % 3]
        if kind == "ct" and pl < 21 - pn_len:
            kind = "tag"
        if kind == "tag" and pl + pn_len < 5:
            kind = "hdr"
        bad[p] = kind
        at = {"ct": o + hl + pl - 1, "tag": o + hl + pl + 15, "hdr": o + 1 + p % 4}[kind]
        tampered[at] ^= 1 << (p % 8)
    assert {"ct", "tag", "hdr"} == set(bad.values())
    covered = np.zeros(size, bool)
    for p in range(n):
        o = int(desc[p]["out_off"])
        covered[o : o + len(headers[p]) + len(payloads[p])] = True
    bad_res = orc.unprotect_batch(recs, ud[sorted(bad)], tampered, size)[1]
    return dict(recs=recs, headers=headers, payloads=payloads, inbuf=inbuf, desc=desc, ud=ud, size=size, wire=wire,
                plain=plain, tampered=tampered, bad=bad, bad_res=bad_res, covered=covered)


def _check(suite, keys, launches):
    import torch

    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    torch.cuda.set_device(0)
    n = _n()
    b = _batch(suite, n)
    desc, ud, size, cov = b["desc"], b["ud"], b["size"], b["covered"]
    count = _counter()
    eng = PacketEngine(2)
    eng.set_key_records(b["recs"][:keys])
    c0 = count()
    wire, res = _run(eng, True, desc, n, b["inbuf"], size)
    plain, ures = _run(eng, False, ud, n, b["wire"], size, fill=0xAA)
    c1 = count()
    tplain, tres = _run(eng, False, ud, n, b["tampered"], size, fill=0xAA)
    c2 = count()
    print("suite %d, %d packets, %d key(s): close-from-LDS launches %d + %d" % (suite, n, keys, c1 - c0, c2 - c1))
    assert (c1 - c0, c2 - c1) == launches
    # protect and unprotect, every packet
    assert (res["status"] == L.S_OK).all() and (res["out_len"] == ud["len"]).all()
    assert np.array_equal(wire, b["wire"])
    assert (ures["status"] == L.S_OK).all() and np.array_equal(ures["pn"], ud["pn"])
    assert np.array_equal(plain[cov], b["plain"][cov])
    # flipped bits: exactly those packets fail and leave no plaintext
    failed = np.zeros(n, bool)
    failed[list(b["bad"])] = True
    assert failed.sum() == (n + EVERY - 1) // EVERY
    assert ((tres["status"] == L.S_DECRYPT) == failed).all()
    assert ((tres["status"] == L.S_OK) == ~failed).all()
    assert (tres[sorted(b["bad"])] == b["bad_res"]).all()
    good = cov.copy()
    for p, kind in b["bad"].items():
        o, hl, pl = int(desc[p]["out_off"]), len(b["headers"][p]), len(b["payloads"][p])
        assert not tplain[o + hl : o + hl + pl].any(), (p, kind)
        good[o : o + hl + pl] = False
    assert np.array_equal(tplain[good], b["plain"][good])


@pytest.mark.parametrize("suite", [0, 1], ids=["aes128", "aes256"])
def test_close_lds_step_loop(suite):
    """One key of the suite: the close-from-LDS form, two launches and then the tampered one."""
    _check(suite, 1, (2, 1))


@pytest.mark.parametrize("suite", [0, 1], ids=["aes128", "aes256"])
def test_two_keys_take_the_four_entry_kernel(suite):
    """A second key of the suite in the table: the unchanged kernel, the same bytes, no LDS-form launch."""
    _check(suite, 2, (0, 0))
