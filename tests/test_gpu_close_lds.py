"""The close-from-LDS form of k_gcm: unplanned 1024-thread AES-GCM launches
with one key of the suite in the table take the multiplies outside the step
loop (associated data beyond 16 bytes by H^1, each lane's closing H^(4-j))
from an LDS copy of the key's 4-bit-window tables instead of global memory.

Every packet of every batch is compared with the C oracle and, where
oracle/_ref is built, with the reference's own _crypto (tests/ref_crypto.py);
the same batches with a second key of the suite installed run the other form
of the kernel and must give the same bytes.  Which form ran is read from the
library's launch counter (qpp_close_lds_launches).

Sizes: 8,193 packets, one past the lone-packet kernels' limit (8192, both
AES-GCM suites), and 4,097 packets of AES-256-GCM (which the lone-packet
kernel takes: no LDS form there), under both step forms.  With two blocks per
lane a step (the default) launches of at most 16 items per CU take the
512-thread shape, which has no LDS to spare and keeps the global tables, so
at 8,193 packets only the one-block form (QPP_GCM_BPL=1, a child process: the
library reads the switch once) reaches the LDS form; one more batch per suite,
one packet past 16 items per CU, reaches it with two blocks per lane.
"""

import ctypes
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY_LEN = {0: 16, 1: 32}
HDR_LENS = (11, 16, 17, 33, 47)  # the associated-data fold runs 0, 0, 1, 2, 2 H^1 multiplies
LONE_MAX = 8192  # launch_packets: unplanned AES-GCM launches up to here run one wave per packet


def _counter():
    lib = ctypes.CDLL(os.path.join(ROOT, "aioquic_amd", "libquicpp.so"))
    lib.qpp_close_lds_launches.restype = ctypes.c_uint64
    return lib.qpp_close_lds_launches


def _keys(suite):
    """Two keys of the suite: slot 0 carries every packet, slot 1 is only
    installed (or not)."""
    from aioquic_amd import layout as L

    rng = np.random.default_rng(0xC105E + suite)
    recs = np.zeros(2, dtype=L.KEY_MATERIAL)
    kl = KEY_LEN[suite]
    for s in range(2):
        recs[s]["slot"] = s
        recs[s]["suite"] = suite
        recs[s]["iv"] = np.frombuffer(rng.bytes(12), np.uint8)
        recs[s]["key"][:kl] = np.frombuffer(rng.bytes(kl), np.uint8)
        recs[s]["hp"][:kl] = np.frombuffer(rng.bytes(kl), np.uint8)
    return recs


@functools.lru_cache(maxsize=None)
def _batch(suite, n, c_oracle=True):
    """n packets on slot 0: payloads of 1..200 bytes cycled (the cycle shifts
    by one each round, so every length meets every position of an item),
    headers of HDR_LENS bytes, packet numbers of 1-4 bytes, no alignment.
    Returns the inputs and the oracle's (and the reference's) outputs.

    c_oracle=False (the large batch: the C oracle's bitwise GHASH takes ~50 us
    a packet and call): the expected wire image of every packet comes from the
    reference's _crypto, and from the C oracle only where oracle/_ref is not
    built; the expected plaintext is the input; the C oracle still judges
    every packet with a flipped bit."""
    from aioquic_amd.batch import layout_packets
    from oracle import oracle as orc
    from tests import ref_crypto

    orc.lib()
    rng = np.random.default_rng(0xC105ED + 16 * suite + n)
    recs = _keys(suite)
    headers, payloads, pns = [], [], []
    for i in range(n):
        plen = 1 + (i + i // 200) % 200
        hlen = HDR_LENS[(i // 3) % len(HDR_LENS)]
        # the header-protection sample needs 4 bytes of packet number + payload
        pn_len = 4 if plen < 3 else 1 + i % 4
        pn = int(rng.integers(0, 1 << 30))
        first = (0xC0 if hlen > 25 else 0x40) | (pn_len - 1)
        headers.append(bytes([first]) + rng.bytes(hlen - 1 - pn_len) +
                       (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big"))
        payloads.append(rng.bytes(plen))
        pns.append(pn)
    inbuf, desc, size = layout_packets(headers, payloads, pns, [0] * n, align=1)
    ref = ref_crypto.checker("tests/test_gpu_close_lds.py::_batch[%d-%d]" % (suite, n))
    ud = desc.copy()
    ud["len"] = [len(h) + len(p) + 16 for h, p in zip(headers, payloads)]
    ud["hdr_len"] = [len(h) - ((h[0] & 3) + 1) for h in headers]
    ud["pn"] = np.asarray(pns, np.uint64)
    out = {}
    if ref is not None:
        from aioquic_amd.bench_data import Workload

        w = Workload(n=n, n_keys=2, keys=recs, desc=desc, udesc=ud, plain=inbuf, plain_size=size,
                     wire_size=size, suites=np.full(n, suite))
        out["ref_wire"] = ref_crypto.protect_all(ref, w)
    if c_oracle or ref is None:
        wire, res = orc.protect_batch(recs, desc, inbuf, size)
        assert (res["status"] == 0).all() and (res["out_len"] == ud["len"]).all()
        out["res"] = res
    else:
        wire = out["ref_wire"]
    if ref is not None:
        out["ref_plain"], out["ref_pns"] = ref_crypto.unprotect_all(ref, w, wire)
    # one flipped bit each in a ciphertext, a tag and a header (the connection
    # id, so the packet still parses): the first and the last packet of a full
    # item, and the last item, which is not full
    assert n % 16 != 0
    bad = {}
    last_full = 16 * ((n // 16) // 2)
    targets = [0, 15, last_full, last_full + 15, 16 * (n // 16), n - 1, 37, 16 * 5 + 2, 16 * 9 + 1]
    kinds = ["ct", "tag", "hdr", "tag", "ct", "hdr", "hdr", "ct", "tag"]
    tampered = wire.copy()
    for p, kind in zip(targets, kinds):
        if p in bad:
            continue
        o, hl, pl = int(desc[p]["out_off"]), len(headers[p]), len(payloads[p])
        pn_len = (headers[p][0] & 3) + 1
        # outside the header-protection sample (16 bytes from the packet
        # number's offset + 4), so that the header still parses as it did and
        # the failure is the tag's: the last ciphertext byte, else the last
        # tag byte, else the connection id
        if kind == "ct" and pl < 21 - pn_len:
            kind = "tag"
        if kind == "tag" and pl + pn_len < 5:
            kind = "hdr"
        bad[p] = kind
        at = {"ct": o + hl + pl - 1, "tag": o + hl + pl + 15, "hdr": o + 1 + p % 4}[kind]
        tampered[at] ^= 1 << (p % 8)
    # the bytes an unprotect defines: header and payload of every packet
    covered = np.zeros(size, bool)
    for p in range(n):
        o = int(desc[p]["out_off"])
        covered[o : o + len(headers[p]) + len(payloads[p])] = True
    if c_oracle:
        out["plain"], out["ures"] = orc.unprotect_batch(recs, ud, wire, size)
        out["bres"] = orc.unprotect_batch(recs, ud, tampered, size)[1]
    else:
        out["plain"] = inbuf  # header and payload at the same offsets
    idx = sorted(bad)
    out["bad_res"] = orc.unprotect_batch(recs, ud[idx], tampered, size)[1]
    out.update(recs=recs, headers=headers, payloads=payloads, pns=ud["pn"], inbuf=inbuf, desc=desc, ud=ud,
               size=size, wire=wire, tampered=tampered, bad=bad, covered=covered)
    return out


def _run(eng, enc, desc, n, data, size, fill=0):
    import torch

    from aioquic_amd import layout as L

    dev = torch.device("cuda", 0)
    d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
    d_in = torch.from_numpy(np.ascontiguousarray(data)).to(dev)
    d_out = torch.full((size,), fill, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    (eng.protect if enc else eng.unprotect)(d_desc, n, d_in, d_out, d_res)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_res.cpu().numpy().view(L.RESULT)


def close_lds_check(suite, n, tag="", c_oracle=True):
    """One batch through the LDS form (one key installed) and through the
    other form (two keys installed), both directions, against the oracles."""
    import torch

    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    torch.cuda.set_device(0)
    b = _batch(suite, n, c_oracle)
    desc, ud, size = b["desc"], b["ud"], b["size"]
    count = _counter()
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    bpl1 = os.environ.get("QPP_GCM_BPL") == "1"
    # launch_packets: the 512-thread shape takes two-block launches of at most 16 items per CU
    lds_form = n > LONE_MAX and (bpl1 or (n + 15) // 16 > 16 * cus)
    print("close_lds_check: suite %d n %d bpl %d lds form expected %s" % (suite, n, 1 if bpl1 else 2, lds_form))

    outs = {}
    for keys in (1, 2):
        eng = PacketEngine(2)
        eng.set_key_records(b["recs"][:keys])
        c0 = count()
        wire, res = _run(eng, True, desc, n, b["inbuf"], size)
        plain, ures = _run(eng, False, ud, n, b["wire"], size, fill=0xAA)
        tplain, tres = _run(eng, False, ud, n, b["tampered"], size, fill=0xAA)
        ran = count() - c0
        print("  keys installed %d: LDS-form launches %d of 3" % (keys, ran))
        assert ran == (3 if keys == 1 and lds_form else 0)
        outs[keys] = (wire, res, plain, ures, tplain, tres)

    wire, res, plain, ures, tplain, tres = outs[1]
    # protect: every packet, against the oracle and the reference
    assert (res["status"] == L.S_OK).all() and (res["out_len"] == ud["len"]).all()
    if "res" in b:
        assert (res == b["res"]).all()
    assert np.array_equal(wire, b["wire"])
    if "ref_wire" in b:
        assert np.array_equal(wire, b["ref_wire"])
    # unprotect of the untouched batch: every packet authenticates
    assert (ures["status"] == L.S_OK).all() and np.array_equal(ures["pn"], b["pns"])
    if "ures" in b:
        assert (ures == b["ures"]).all()
    cov = b["covered"]
    assert np.array_equal(plain[cov], b["plain"][cov])
    if "ref_plain" in b:
        assert np.array_equal(plain[cov], b["ref_plain"][cov])
        assert np.array_equal(ures["pn"], b["ref_pns"])
    # unprotect with flipped bits: exactly those packets fail, with the
    # oracle's status, and leave no plaintext; every other packet as before
    assert (tres[sorted(b["bad"])] == b["bad_res"]).all()
    if "bres" in b:
        assert (tres == b["bres"]).all()
    failed = np.zeros(n, bool)
    failed[list(b["bad"])] = True
    assert ((tres["status"] == L.S_DECRYPT) == failed).all()
    assert ((tres["status"] == L.S_OK) == ~failed).all()
    good = cov.copy()
    for p, kind in b["bad"].items():
        o, hl, pl = int(desc[p]["out_off"]), len(b["headers"][p]), len(b["payloads"][p])
        assert not tplain[o + hl : o + hl + pl].any(), (p, kind)
        good[o : o + hl + pl] = False
    assert np.array_equal(tplain[good], b["plain"][good])
    # a second key of the suite in the table: the other form, the same bytes
    for got, other in zip(outs[1], outs[2]):
        assert np.array_equal(got, other)
    if tag:
        print("close_lds_check ok", tag)


@pytest.mark.parametrize("bpl", ["2", "1"], ids=["bpl2", "bpl1"])
@pytest.mark.parametrize("suite,n", [(0, 8193), (1, 4097), (1, 8193)], ids=["aes128-8193", "aes256-4097", "aes256-8193"])
def test_close_lds_smallest_launch(suite, n, bpl):
    """8,193 packets (one past the lone-packet kernels) and 4,097 of AES-256-GCM, both step forms."""
    if bpl == "1":
        tag = "suite %d QPP_GCM_BPL=1" % suite
        code = ("import sys; sys.path.insert(0, %r); from tests.test_gpu_close_lds import close_lds_check; "
                "close_lds_check(%d, %d, %r)" % (ROOT, suite, n, tag))
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, QPP_GCM_BPL="1"),
                           capture_output=True, text=True, timeout=180)
        print(r.stdout[-2000:])
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        assert "close_lds_check ok " + tag in r.stdout
        return
    close_lds_check(suite, n)


@pytest.mark.parametrize("suite", [0, 1], ids=["aes128", "aes256"])
def test_close_lds_two_block_form(suite):
    """One packet past 16 items per CU: the smallest two-blocks-per-lane
    launch that runs 1024-thread workgroups, so the LDS form."""
    import torch

    n = 16 * 16 * torch.cuda.get_device_properties(0).multi_processor_count + 1
    close_lds_check(suite, n, c_oracle=False)
