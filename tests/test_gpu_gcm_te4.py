"""The four-table AES image and the two-multiply close of the close-from-LDS
form of k_gcm (unplanned 1024-thread AES-GCM launches with one key of the
suite in the table): rounds 3..NR-1 of the step loop read Te2 / Te3 from a
second 64 KiB of the LDS image with plain round keys, and lane j closes its
GHASH chain with H^(4-j) as two multiplies by the LDS copy of H^2 and H^1.

Every packet of every launch is compared with the C oracle's bytes.  The
oracle (bitwise GHASH) runs once per suite on a base set of distinct packets;
a launch cycles through the base set, packed back to back (no alignment), so
every copy lies at another offset and in another lane of its wave item, and
its expected bytes are the oracle's bytes of its base packet.  Where
oracle/_ref is built the reference's own _crypto (tests/ref_crypto.py) also
runs over every packet of every launch, both directions.

Base sets:
  short   655 packets: every payload length 0..130 with every header length
          11, 16, 17, 33, 47 (packet b: b % 131 bytes, header b % 5).  Tiny
          packets, one and two steps with two blocks per lane; every front
          padding 0..7 of the block sequence (so the single-block first step
          too); the H^1 fold of the associated data 0, 1 and 2 times, so
          every lane's two-multiply close runs on non-zero accumulators;
          packet-number lengths 1-4.
  full    20 packets of 1200 bytes on the wire (the bench's size), the five
          header lengths and the four packet-number lengths.

Launches (both AES-GCM suites, protect, unprotect, and unprotect with one
flipped tag bit: that packet fails and leaves no plaintext, every other
packet is as before):
  * 8,193 packets (one past the lone-packet kernels) under QPP_GCM_BPL=1, in
    a child process (the library reads the switch once);
  * one packet past 16 items per CU (CU count from the device properties)
    with two blocks per lane, the short set and the full set;
  * each of them again with a second key of the suite installed: the
    four-entry form runs (qpp_close_lds_launches counts 3 / 0 launches) and
    must give the same bytes;
  * one launch whose packets alternate between two slots, AES-128-GCM in
    slot 0 and AES-256-GCM in slot 1: each suite's launch is the
    close-from-LDS form (one key of its suite), every wave item holds both
    slots' packets, and each launch's copy holds its own suite's slot.  (The
    form is only chosen with one key of the suite installed, so within a
    launch no packet of the launch's suite lies on a slot other than the
    copy's: the global-table close of the form is not reachable through the
    API and is covered by the four-entry form's runs above, which share
    ghash_mul_global with it.)
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
S_OK, S_DECRYPT = 0, 2
TAG = 16


def _counter():
    lib = ctypes.CDLL(os.path.join(ROOT, "aioquic_amd", "libquicpp.so"))
    lib.qpp_close_lds_launches.restype = ctypes.c_uint64
    return lib.qpp_close_lds_launches


@functools.lru_cache(maxsize=None)
def _keys():
    """Slots 0 / 1: the AES-128-GCM / AES-256-GCM key that carries packets;
    slots 2 / 3: a second key of each suite, only installed (or not)."""
    from aioquic_amd import layout as L

    rng = np.random.default_rng(0x7E4)
    recs = np.zeros(4, dtype=L.KEY_MATERIAL)
    for s in range(4):
        suite = s & 1
        kl = KEY_LEN[suite]
        recs[s]["slot"] = s
        recs[s]["suite"] = suite
        recs[s]["iv"] = np.frombuffer(rng.bytes(12), np.uint8)
        recs[s]["key"][:kl] = np.frombuffer(rng.bytes(kl), np.uint8)
        recs[s]["hp"][:kl] = np.frombuffer(rng.bytes(kl), np.uint8)
    return recs


def _udesc(desc, headers, payloads, pns):
    ud = desc.copy()
    ud["len"] = [len(h) + len(p) + TAG for h, p in zip(headers, payloads)]
    ud["hdr_len"] = [len(h) - ((h[0] & 3) + 1) for h in headers]
    ud["pn"] = np.asarray(pns, np.uint64)
    return ud


@functools.lru_cache(maxsize=None)
def _base(kind):
    """The base set's (headers, payloads, pns), the same for both suites."""
    rng = np.random.default_rng(0x7E4000 + len(kind))
    headers, payloads, pns = [], [], []
    m = 131 * 5 if kind == "short" else 20
    for b in range(m):
        hlen = HDR_LENS[b % 5]
        plen = b % 131 if kind == "short" else 1200 - TAG - hlen
        # the header-protection sample needs 4 bytes of packet number + payload
        pn_len = 1 + b % 4
        if plen + pn_len < 4:
            pn_len = 4
        pn = int(rng.integers(0, 1 << 30))
        first = (0xC0 if hlen > 25 else 0x40) | (pn_len - 1)
        headers.append(bytes([first]) + rng.bytes(hlen - 1 - pn_len) +
                       (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big"))
        payloads.append(rng.bytes(plen))
        pns.append(pn)
    if kind == "short":
        assert {(len(p), len(h)) for h, p in zip(headers, payloads)} == {(p, h) for p in range(131) for h in HDR_LENS}
    assert {(h[0] & 3) + 1 for h in headers} == {1, 2, 3, 4}
    return headers, payloads, pns


@functools.lru_cache(maxsize=None)
def _base_wire(kind, slot):
    """The C oracle's wire image of every base packet under slot's key (a
    list of bytes), after the oracle's own unprotect returned the input."""
    from aioquic_amd.batch import layout_packets
    from oracle import oracle as orc

    orc.lib()
    headers, payloads, pns = _base(kind)
    m = len(headers)
    inbuf, desc, size = layout_packets(headers, payloads, pns, [slot] * m, align=1)
    ud = _udesc(desc, headers, payloads, pns)
    wire, res = orc.protect_batch(_keys(), desc, inbuf, size)
    assert (res["status"] == 0).all() and (res["out_len"] == ud["len"]).all()
    plain, ures = orc.unprotect_batch(_keys(), ud, wire, size)
    assert (ures["status"] == 0).all() and np.array_equal(ures["pn"], ud["pn"])
    out = []
    for i in range(m):
        o, hl, pl = int(desc[i]["out_off"]), len(headers[i]), len(payloads[i])
        assert np.array_equal(plain[o : o + hl + pl], inbuf[o : o + hl + pl])
        out.append(wire[o : o + hl + pl + TAG].copy())
    return out


@functools.lru_cache(maxsize=None)
def _launch(kind, n, slots):
    """n packets cycling through the base set, packet i on slot slots[i %
    len(slots)], back to back; the expected wire image from the oracle's base
    bytes, the reference's images where it is built, one flipped tag bit."""
    from aioquic_amd.batch import layout_packets
    from oracle import oracle as orc
    from tests import ref_crypto

    bh, bp, bpn = _base(kind)
    m = len(bh)
    headers = [bh[i % m] for i in range(n)]
    payloads = [bp[i % m] for i in range(n)]
    pns = [bpn[i % m] for i in range(n)]
    slot = [slots[i % len(slots)] for i in range(n)]
    inbuf, desc, size = layout_packets(headers, payloads, pns, slot, align=1)
    ud = _udesc(desc, headers, payloads, pns)
    wire = np.zeros(size, np.uint8)
    covered = np.zeros(size, bool)
    base = {s: _base_wire(kind, s) for s in set(slots)}
    for i, o in enumerate(desc["out_off"].tolist()):
        w = base[slot[i]][i % m]
        wire[o : o + len(w)] = w
        covered[o : o + len(w) - TAG] = True
    out = dict(headers=headers, payloads=payloads, inbuf=inbuf, desc=desc, ud=ud, size=size, wire=wire,
               covered=covered, n=n)
    ref = ref_crypto.checker("tests/test_gpu_gcm_te4.py::_launch[%s-%d-%s]" % (kind, n, slots))
    if ref is not None:
        from aioquic_amd.bench_data import Workload

        w = Workload(n=n, n_keys=4, keys=_keys(), desc=desc, udesc=ud, plain=inbuf, plain_size=size,
                     wire_size=size, suites=np.asarray(slot) & 1)
        out["ref_wire"] = ref_crypto.protect_all(ref, w)
        out["ref_plain"], out["ref_pns"] = ref_crypto.unprotect_all(ref, w, out["ref_wire"])
    # one flipped bit in the last tag byte of a packet in mid-batch whose tag
    # lies outside its header-protection sample (16 bytes from the packet
    # number's offset + 4), so the header parses as it did
    p = n // 2 + 3
    while len(payloads[p]) < 5:
        p += 1
    o, hl, pl = int(desc[p]["out_off"]), len(headers[p]), len(payloads[p])
    tampered = wire.copy()
    tampered[o + hl + pl + TAG - 1] ^= 1 << (p % 8)
    out.update(bad=p, tampered=tampered, bad_res=orc.unprotect_batch(_keys(), ud[p : p + 1], tampered, size)[1])
    assert out["bad_res"]["status"][0] == S_DECRYPT
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


def te4_check(kind, n, slots, tag=""):
    """One launch batch through the close-from-LDS form (one key per suite
    installed) and through the four-entry form (a second key of each suite
    installed), both directions, every packet against the oracles."""
    import torch

    from aioquic_amd.batch import PacketEngine

    torch.cuda.set_device(0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if n is None:
        n = 16 * 16 * cus + 1  # one packet past 16 items per CU
    b = _launch(kind, n, slots)
    desc, ud, size = b["desc"], b["ud"], b["size"]
    count = _counter()
    bpl1 = os.environ.get("QPP_GCM_BPL") == "1"
    # launch_packets: the 512-thread shape takes two-block launches of at most 16 items per CU
    assert n > LONE_MAX and (bpl1 or (n + 15) // 16 > 16 * cus), "the launch must reach the close-from-LDS form"
    print("te4_check: %s n %d slots %s bpl %d" % (kind, n, slots, 1 if bpl1 else 2))

    outs = {}
    for second in (False, True):
        eng = PacketEngine(4)
        keep = sorted(set(slots)) + ([s + 2 for s in sorted(set(slots))] if second else [])
        eng.set_key_records(_keys()[keep])
        c0 = count()
        wire, res = _run(eng, True, desc, n, b["inbuf"], size)
        plain, ures = _run(eng, False, ud, n, b["wire"], size, fill=0xAA)
        tplain, tres = _run(eng, False, ud, n, b["tampered"], size, fill=0xAA)
        ran = count() - c0
        print("  second key installed %s: close-from-LDS launches %d" % (second, ran))
        # one launch per suite present and call
        assert ran == (0 if second else 3 * len(set(slots)))
        outs[second] = (wire, res, plain, ures, tplain, tres)

    wire, res, plain, ures, tplain, tres = outs[False]
    # protect: every packet, against the oracle's bytes and the reference's
    assert (res["status"] == S_OK).all() and (res["out_len"] == ud["len"]).all()
    assert np.array_equal(wire, b["wire"])
    if "ref_wire" in b:
        assert np.array_equal(b["ref_wire"], b["wire"])
        assert np.array_equal(wire, b["ref_wire"])
    # unprotect of the untouched batch: every packet authenticates
    cov = b["covered"]
    assert (ures["status"] == S_OK).all() and np.array_equal(ures["pn"], ud["pn"])
    assert np.array_equal(plain[cov], b["inbuf"][cov])
    if "ref_plain" in b:
        assert np.array_equal(plain[cov], b["ref_plain"][cov])
        assert np.array_equal(ures["pn"], b["ref_pns"])
    # one flipped tag bit: that packet fails with the oracle's result and
    # leaves no plaintext; every other packet as before
    p = b["bad"]
    assert (tres[p : p + 1] == b["bad_res"]).all()
    failed = np.zeros(n, bool)
    failed[p] = True
    assert ((tres["status"] == S_DECRYPT) == failed).all()
    assert ((tres["status"] == S_OK) == ~failed).all()
    assert np.array_equal(tres["pn"][~failed], ud["pn"][~failed])
    o, hl, pl = int(desc[p]["out_off"]), len(b["headers"][p]), len(b["payloads"][p])
    assert not tplain[o + hl : o + hl + pl].any()
    good = cov.copy()
    good[o : o + hl + pl] = False
    assert np.array_equal(tplain[good], b["inbuf"][good])
    # a second key of the suite in the table: the other form, the same bytes
    for got, other in zip(outs[False], outs[True]):
        assert np.array_equal(got, other)
    if tag:
        print("te4_check ok", tag)


@pytest.mark.parametrize("suite", [0, 1], ids=["aes128", "aes256"])
def test_te4_smallest_launch_one_block(suite):
    """8,193 packets of the short set with one block per lane a step."""
    tag = "suite %d QPP_GCM_BPL=1" % suite
    code = ("import sys; sys.path.insert(0, %r); from tests.test_gpu_gcm_te4 import te4_check; "
            "te4_check('short', %d, (%d,), %r)" % (ROOT, LONE_MAX + 1, suite, tag))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, QPP_GCM_BPL="1"),
                       capture_output=True, text=True, timeout=180)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "te4_check ok " + tag in r.stdout


@pytest.mark.parametrize("kind", ["short", "full"])
@pytest.mark.parametrize("suite", [0, 1], ids=["aes128", "aes256"])
def test_te4_two_blocks(suite, kind):
    """One packet past 16 items per CU with two blocks per lane: the short
    set, and 1200-byte packets."""
    te4_check(kind, None, (suite,))


def test_te4_two_slots_alternating():
    """Packets alternating between an AES-128-GCM and an AES-256-GCM slot."""
    te4_check("short", None, (0, 1))
