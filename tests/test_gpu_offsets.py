"""Descriptor offsets past 4 GiB and the item span limit (QPP_ITEM_SPAN_MAX,
include/quic_pp.h, Buffers).

The quad kernels (k_gcm, k_chacha) address the <= 16 packets of one item
through 32-bit buffer views based at the item's lowest offsets; the lone
kernels use 64-bit pointers.  Here every kernel family runs packets above
2^32, either side of it and across it, in place, and with a far packet whose
span from a tiny lowest packet is just under, exactly at and one byte over
the limit, for input and for output separately.  Input and output are two
zero-filled device tensors of 2^32 + 2^20 bytes; packets go in by slice
assignment; the expected bytes and result records are the C oracle's for the
same packets laid out compactly (the oracle does not depend on offsets).
After the per-packet checks the packets' own extents are zeroed on the device
and the whole output tensor must hold no nonzero byte: a store that went
anywhere else (a wrapped offset, a truncated base) shows there.

The three span-edge packets cannot share a launch: their extents in the far
buffer all end within 17 bytes of each other and would overlap.  Each runs in
a launch of its own, with the same tiny lowest packet and ten near ones.

Unprotect runs on the oracle's wire image, so a protect bug cannot mask an
unprotect bug."""

import os
import subprocess
import sys

import numpy as np
import pytest

from tests.golden_cases import long_header, short_header
from tests.test_gpu_parity import _keys

G4 = 1 << 32
BIG = G4 + (1 << 20)
LIMIT = 0xFFFFFF00  # = layout.ITEM_SPAN_MAX = QPP_ITEM_SPAN_MAX (checked below)
SUITE_NAMES = {0: "aes128", 1: "aes256", 2: "chacha"}
SCENARIOS = ("above", "straddle", "span-edge-out", "span-edge-in", "in-place-above")
RAGGED = [4, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1173, 1440]
PAIR_OF_16 = [0, 3, 14, 15]       # payloads 4, 17, 1440 (the one that crosses 2^32) and the long header
PAIR_OF_EDGE = [0, 1, 2, 11]      # the tiny lowest packet, two near ones, the far one
LOW = 256 + 37                    # the tiny lowest packet of the span-edge items


def _ragged_packets():
    """16 (header, payload, pn): short headers with pn lengths 1-4 over the
    ragged payloads, and one long (Initial) header."""
    rng = np.random.default_rng(0x0FF5)
    pkts = []
    for i, n in enumerate(RAGGED):
        pn = 1000 + 77 * i
        pkts.append((short_header(rng.bytes(8), pn, 1 + i % 4, 0), rng.bytes(n), pn))
    pn = 4242
    pkts.append((long_header(1, rng.bytes(8), rng.bytes(5), rng.bytes(61), pn, 2, 300 + 16), rng.bytes(300), pn))
    return pkts


def _edge_packets():
    """The tiny lowest packet (9-byte header, 4-byte payload), ten near ones and
    the three far candidates (header + payload = 3 mod 4 and not 0 mod 16)."""
    rng = np.random.default_rng(0xED6E)
    tiny = (short_header(rng.bytes(7), 5, 1, 0), rng.bytes(4), 5)
    assert len(tiny[0]) == 9
    near = [(short_header(rng.bytes(8), 20 + i, 1 + i % 4, 0), rng.bytes([33, 700, 64, 1, 250, 17, 1173, 48, 5, 129][i]),
             20 + i) for i in range(10)]
    far = [(short_header(rng.bytes(8), 900, 2, 0), rng.bytes(1172), 900),
           (short_header(rng.bytes(8), 901, 3, 0), rng.bytes(263), 901),
           (short_header(rng.bytes(7), 902, 1, 0), rng.bytes(98), 902)]
    return tiny, near, far


def _extents(pkt, direction):
    """(input extent, output extent) of a packet (quic_pp.h, Buffers)."""
    body = len(pkt[0]) + len(pkt[1])
    return (body, body + 16) if direction == "protect" else (body + 16, body)


def launches(scenario, direction):
    """[(packets, in_offs, out_offs, in_place)] of a scenario: one launch each,
    except the span-edge scenarios' three (module docstring)."""
    if scenario in ("above", "in-place-above"):
        pk = _ragged_packets()
        ins = [G4 + 4096 + 3000 * i + (7 * i + 3) % 16 for i in range(16)]
        outs = [G4 + 4096 + 3000 * (15 - i) + (11 * i + 5) % 16 for i in range(16)]
        assert len({o % 16 for o in ins}) > 8 and max(ins + outs) + 1500 < G4 + (1 << 19)
        return [(pk, ins, ins if scenario == "in-place-above" else outs, scenario == "in-place-above")]
    if scenario == "straddle":
        pk = _ragged_packets()

        def offs(a, b):
            o = [G4 - 40000 + 3001 * i + (a * i + b) % 16 if i < 7 else G4 + 2000 + 3001 * (i - 7) + (a * i + b) % 16
                 for i in range(16)]
            o[14] = G4 - 701 - b  # 1440 payload bytes: crosses byte 2^32
            return o

        ins, outs = offs(5, 1), offs(9, 6)
        for o in (ins, outs):
            assert o[14] < G4 < o[14] + 1440 and sum(x < G4 for x in o) == 8
        return [(pk, ins, outs, False)]
    assert scenario in ("span-edge-out", "span-edge-in")
    tiny, near, far = _edge_packets()
    side = 1 if scenario == "span-edge-out" else 0
    out = []
    for k, target in enumerate((LIMIT - 16, LIMIT, LIMIT + 1)):
        pk = [tiny] + near + [far[k]]
        # near side: the tiny packet, >= 1 KiB that must stay zero, the rest
        near_offs = [LOW] + [LOW + 2048 + 1601 * i + (3 * i) % 16 for i in range(11)]
        far_offs = list(near_offs)
        ext = _extents(far[k], direction)[side]
        far_offs[11] = LOW + target - ext
        assert ext % 16 != 0 and (far_offs[11] - LOW) % 4 != 0
        assert far_offs[11] + ext <= BIG and LOW + LIMIT <= BIG  # the view lies inside the allocation
        out.append((pk, far_offs, near_offs, False) if side == 0 else (pk, near_offs, far_offs, False))
    return out


def spans(pk, ins, outs, direction):
    """Per packet: (input span, output span) from the item's lowest offsets."""
    bi, bo = min(ins), min(outs)
    return [(i - bi + _extents(p, direction)[0], o - bo + _extents(p, direction)[1])
            for p, i, o in zip(pk, ins, outs)]


class Rig:
    """One suite's engine (one key slot), the oracle and the two big tensors."""

    def __init__(self, suite, d_in, d_out):
        import torch

        from aioquic_amd import layout as L
        from aioquic_amd.batch import PacketEngine
        from oracle import oracle as orc

        orc.lib()
        assert L.ITEM_SPAN_MAX == LIMIT
        self.torch, self.L, self.orc, self.suite = torch, L, orc, suite
        self.recs = _keys(np.random.default_rng(0x0FF + suite), 1, (suite,))
        self.eng = PacketEngine(1)
        self.eng.set_key_records(self.recs)
        self.d_in, self.d_out = d_in, d_out

    def put(self, t, off, data):
        t[off : off + len(data)] = self.torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(t.device)

    @staticmethod
    def nonzero_anywhere(t):
        step = 1 << 30  # slices of at most 1 GiB: no 32-bit index anywhere
        return any(bool(t[a : min(a + step, t.numel())].any()) for a in range(0, t.numel(), step))

    def run(self, launch, direction, planned, subset=None):
        """One launch; returns (packets QPP_S_OK, packets QPP_S_LENGTH)."""
        torch, L, orc = self.torch, self.L, self.orc
        from aioquic_amd.batch import layout_packets

        pk, ins, outs, in_place = launch
        if subset is not None:
            pk, ins, outs = [pk[i] for i in subset], [ins[i] for i in subset], [outs[i] for i in subset]
        n = len(pk)
        d_in = self.d_in
        d_out = d_in if in_place else self.d_out
        d_in.zero_()
        d_out.zero_()
        # the oracle on the compact layout
        cbuf, cdesc, csize = layout_packets([p[0] for p in pk], [p[1] for p in pk], [p[2] for p in pk], [0] * n)
        c_wire, c_res = orc.protect_batch(self.recs, cdesc, cbuf, csize)
        assert (c_res["status"] == L.S_OK).all()
        desc = cdesc.copy()
        if direction == "protect":
            src = [p[0] + p[1] for p in pk]
            exp_res = c_res
            exp = [c_wire[int(d["out_off"]) : int(d["out_off"]) + int(r["out_len"])] for d, r in zip(cdesc, c_res)]
        else:
            cud = cdesc.copy()
            cud["len"] = c_res["out_len"]
            cud["hdr_len"] = [len(p[0]) - ((p[0][0] & 3) + 1) for p in pk]
            cud["pn"] = [p[2] + (i % 5) for i, p in enumerate(pk)]
            c_back, exp_res = orc.unprotect_batch(self.recs, cud, c_wire, csize)
            assert (exp_res["status"] == L.S_OK).all()
            src = [c_wire[int(d["in_off"]) : int(d["in_off"]) + int(d["len"])].tobytes() for d in cud]
            exp = [c_back[int(d["out_off"]) : int(d["out_off"]) + int(r["out_len"])] for d, r in zip(cud, exp_res)]
            desc = cud.copy()
        desc["in_off"] = np.array(ins, np.uint64)
        desc["out_off"] = np.array(outs, np.uint64)
        ext = [_extents(p, direction) for p in pk]
        for s, (ei, eo), i, o in zip(src, ext, ins, outs):
            assert len(s) == ei and 0 <= i and i + ei <= BIG and 0 <= o and o + eo <= BIG
            self.put(d_in, i, s)
        d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        d_res = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device="cuda")
        plan = self.eng.bucket(d_desc, n) if planned else None
        (self.eng.protect if direction == "protect" else self.eng.unprotect)(d_desc, n, d_in, d_out, d_res, plan=plan)
        torch.cuda.synchronize()
        res = d_res.cpu().numpy().view(L.RESULT)
        n_ok = n_len = 0
        for j, ((si, so), (ei, eo)) in enumerate(zip(spans(pk, ins, outs, direction), ext)):
            st = int(res[j]["status"])
            got = d_out[outs[j] : outs[j] + eo].cpu().numpy()
            what = (j, si - LIMIT, so - LIMIT, st)
            if st == L.S_OK:
                assert res[j] == exp_res[j], (what, res[j], exp_res[j])
                assert len(exp[j]) == eo and np.array_equal(got, exp[j]), what
                n_ok += 1
            else:
                # only a packet over the limit may be refused, and only this way
                assert (si > LIMIT or so > LIMIT) and st == L.S_LENGTH, what
                assert int(res[j]["out_len"]) == 0, what
                # (in place, its own input is still there: nothing of it was written)
                assert np.array_equal(got, np.frombuffer(src[j], np.uint8)[:eo]) if in_place else not got.any(), what
                n_len += 1
            d_out[outs[j] : outs[j] + eo] = 0
            d_in[ins[j] : ins[j] + ei] = 0
        assert not self.nonzero_anywhere(d_out), "a store outside the packets' own output extents"
        assert not self.nonzero_anywhere(d_in), "the input buffer was written outside the packets' extents"
        return n_ok, n_len

    def scenario(self, scenario, direction, path):
        """Runs a scenario on a path; asserts the over-limit rule; returns the
        counts.  path: lone / pair (unplanned), planned, quad (unplanned, in
        a process where the unplanned launches take the quad kernels)."""
        ok = ln = over = 0
        for launch in launches(scenario, direction):
            subset = None
            if path == "pair":
                subset = PAIR_OF_16 if len(launch[0]) == 16 else PAIR_OF_EDGE
            pk, ins, outs = launch[:3]
            if subset is not None:
                pk, ins, outs = [pk[i] for i in subset], [ins[i] for i in subset], [outs[i] for i in subset]
            n_over = sum(si > LIMIT or so > LIMIT for si, so in spans(pk, ins, outs, direction))
            a, b = self.run(launch, direction, path == "planned", subset)
            # the quad kernels must refuse a packet over the limit; nobody may refuse another
            if path in ("planned", "quad"):
                assert b == n_over, (scenario, direction, path, a, b, n_over)
            assert b <= n_over
            ok, ln, over = ok + a, ln + b, over + n_over
        assert over == (1 if scenario.startswith("span-edge") else 0)
        print("offsets %s %s %s %s: ok=%d length=%d" % (scenario, path, SUITE_NAMES[self.suite], direction, ok, ln))
        return ok, ln


def _big_tensors():
    import torch

    return (torch.zeros(BIG, dtype=torch.uint8, device="cuda"), torch.zeros(BIG, dtype=torch.uint8, device="cuda"))


@pytest.fixture(scope="module")
def rigs():
    import torch

    d_in, d_out = _big_tensors()
    r = {s: Rig(s, d_in, d_out) for s in (0, 1, 2)}
    yield r
    r.clear()
    del d_in, d_out
    torch.cuda.empty_cache()  # the two 4 GiB tensors go back to the device


def test_scenarios_have_the_stated_geometry():
    """(CPU) The scenarios are what the module docstring says they are, and the
    limit is the header's."""
    import re

    from aioquic_amd import layout as L

    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "quic_pp.h")).read()
    assert int(re.search(r"#define QPP_ITEM_SPAN_MAX (0x[0-9a-f]+)u", hdr).group(1), 16) == L.ITEM_SPAN_MAX == LIMIT
    for direction in ("protect", "unprotect"):
        for name in ("span-edge-out", "span-edge-in"):
            got = []
            for pk, ins, outs, _ in launches(name, direction):
                sp = spans(pk, ins, outs, direction)
                assert min(ins) == LOW == min(outs) and min(ins[1:] + outs[1:]) >= LOW + 13 + 16 + 1024
                assert all(max(s) < 1 << 20 for s in sp[:-1])
                other, far = sp[-1] if name == "span-edge-out" else sp[-1][::-1]
                assert other < 1 << 20
                got.append(far - LIMIT)
            assert got == [-16, 0, 1]
        for name in ("above", "straddle", "in-place-above"):
            (pk, ins, outs, _), = launches(name, direction)
            assert len(pk) == 16 and all(max(s) < 1 << 20 for s in spans(pk, ins, outs, direction))
            for offs, side in ((ins, 0), (outs, 1)):
                iv = sorted((o, o + _extents(p, direction)[side]) for p, o in zip(pk, offs))
                assert all(a[1] <= b[0] for a, b in zip(iv, iv[1:]))  # no overlap


# (no pair launches for ChaCha20-Poly1305: k_lone_chacha always runs one wave per packet)
PATH_SUITE = [(p, s) for p in ("lone", "pair", "planned") for s in (0, 1, 2) if not (p == "pair" and s == 2)]


@pytest.mark.gpu
@pytest.mark.parametrize("direction", ["protect", "unprotect"])
@pytest.mark.parametrize("path,suite", PATH_SUITE, ids=["%s-%s" % (p, SUITE_NAMES[s]) for p, s in PATH_SUITE])
@pytest.mark.parametrize("scenario", SCENARIOS)
def test_offsets(rigs, scenario, path, suite, direction):
    """lone: unplanned, 16 (span-edge: 12) packets -- k_lone_gcm / k_lone_chacha;
    pair: unplanned, 4 packets, AES-GCM -- k_lone_gcm with two waves per
    packet; planned: plan=eng.bucket(...), one key slot -- k_gcm / k_chacha."""
    rigs[suite].scenario(scenario, direction, path)


def _quad_child():
    d_in, d_out = _big_tensors()
    for suite in (0, 1, 2):
        rig = Rig(suite, d_in, d_out)
        for scenario in SCENARIOS:
            for direction in ("protect", "unprotect"):
                rig.scenario(scenario, direction, "quad")
    from aioquic_amd import _crypto

    assert _crypto.watchdog_count() == 0
    print("offsets quad child ok")


@pytest.mark.gpu
@pytest.mark.parametrize("bpl", ["2", "1"], ids=["bpl2", "bpl1"])
def test_offsets_quad_unplanned(bpl):
    """Every scenario, suite and direction through unplanned launches of the
    quad kernels (QPP_LONE=0 in a child process, as
    test_quad_kernels_at_small_sizes does), with k_gcm's two-block form and
    once more with its one-block form (QPP_GCM_BPL=1)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import sys; sys.path.insert(0, %r); from tests.test_gpu_offsets import _quad_child; _quad_child()" % root)
    env = dict(os.environ, QPP_LONE="0")
    env.pop("QPP_GCM_BPL", None)
    if bpl == "1":
        env["QPP_GCM_BPL"] = "1"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    print("".join(x + "\n" for x in r.stdout.splitlines() if x.startswith("offsets ")), end="")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "offsets quad child ok" in r.stdout
    assert r.stdout.count("offsets span-edge") == 2 * 3 * 2
