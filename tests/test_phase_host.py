"""CPU checks of the key-phase decision.

aioquic_amd/csrc/qpp_phase.h, the decision every lane of k_phase runs, is
built for the host with g++ (tests/phase_host.cc) and compared with the Python
restatement of tests/phase_cases.py: over a batch that meets every condition
of qpp_route_phase, with the mask bytes of the C oracle's header protection
for all three suites, and with every condition failing alone.  The same file's
main(), built with -fsanitize=address,undefined and run as a program of its
own, is the out-of-bounds check: its packets live in heap buffers of exactly
the packet's size.
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from aioquic_amd import layout as L
from oracle import oracle as O
from tests import phase_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "phase_host.cc")
u32, vp = ctypes.c_uint32, ctypes.c_void_p
MASK_FN = ctypes.CFUNCTYPE(None, u32, u32, ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint8))
SLOT = np.dtype([("suite", "<u4"), ("key_phase", "<u4")])
EMPTY = 0xFF


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("phase_host") / "libphase_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    for f, args in ((lib.ph_next_entry, [u32] * 5), (lib.ph_eligible, [vp] + [u32] * 4), (lib.ph_flips, [u32] * 3),
                    (lib.ph_decide, [vp] + [u32] * 6), (lib.ph_lane, [vp, u32, vp, vp, u32, vp, u32, vp, MASK_FN])):
        f.restype = u32
        f.argtypes = args
    return lib


@pytest.fixture(scope="module")
def world():
    return P.World(400)


def slot_array(table: dict, cap: int):
    a = np.zeros(cap, SLOT)
    a["suite"] = EMPTY
    for s, (suite, phase, _) in table.items():
        a[s] = (suite, phase)
    return a


def oracle_mask(table: dict, seen: list):
    """The lane's mask callback: the C oracle's HeaderProtection mask under
    the slot's HP key."""
    def fn(suite, slot, sample, mask):
        want_suite, _, hp = table[slot]
        assert suite == want_suite
        seen.append(slot)
        out = O.hp_mask(suite, hp, bytes(sample[k] for k in range(16)))
        for k in range(16):
            mask[k] = out[k]
    return MASK_FN(fn)


@pytest.mark.parametrize("routed", [True, False])
def test_lane_matches_restatement(lib, world, routed):
    w = world
    route = w.route if routed else None
    nxt = w.conn_next if routed else w.next_per_desc
    n_next = P.N_CONN if routed else 0
    want_d, want_p = P.restate(w.desc, route, nxt, n_next, w.table, P.CAP, w.buf)
    slots = slot_array(w.table, P.CAP)
    seen: list = []
    cb = oracle_mask(w.table, seen)
    desc = w.desc.copy()
    rt = None if route is None else route.copy()
    got = [lib.ph_lane(slots.ctypes.data, P.CAP, None if rt is None else rt.ctypes.data, nxt.ctypes.data, n_next,
                       desc.ctypes.data, i, w.buf.ctypes.data, cb) for i in range(w.n)]
    assert got == want_p.tolist()
    assert desc.tobytes() == want_d.tobytes(), "only the slot of a re-pointed descriptor changes"
    # the batch meets what it says it does
    flipped = {c for (k, c), p in zip(w.kind, want_p) if p}
    assert {c % 3 for c in flipped} == {0, 1, 2}, "all three suites"
    assert {w.table[2 * c][1] for c in flipped} == {0, 1}, "phase 0 -> 1 and 1 -> 0"
    assert {k for (k, c), p in zip(w.kind, want_p) if p} >= {"flip", "tamper"}
    quiet = {(k, c) for (k, c), p in zip(w.kind, want_p) if not p}
    assert {c for k, c in quiet if k == "flip"} >= {6, 7, 8, 9, 10, 11}, "each bad next slot, and an empty current one"
    if routed:
        assert {k for k, _ in quiet} >= {"cur", "short19", "nohp", "cls_long", "cls_unknown", "cls_malformed",
                                         "cls_badconn", "conn_past"}
    else:
        assert {k for (k, c), p in zip(w.kind, want_p) if p} >= {"cls_long", "cls_badconn", "conn_past"}
    assert len(seen) == sum(P.acting(w.desc, route, nxt, n_next, w.table, P.CAP)), \
        "a mask is computed for the eligible lanes only"


def test_next_entry(lib):
    for cls in range(5):
        for conn in (0, 4, 5, 6, P.NONE):
            want = conn if cls == L.R_SHORT and conn < 5 else P.NONE
            assert lib.ph_next_entry(1, cls, conn, 5, 77) == want
            assert lib.ph_next_entry(0, cls, conn, 5, 77) == 77


def _desc(length=60, hdr_len=9, flags=0, slot=0):
    d = np.zeros(1, L.DESC)
    d["len"], d["hdr_len"], d["flags"], d["slot"] = length, hdr_len, flags, slot
    return d


def test_each_condition_failing_alone(lib):
    """eligible() and decide() against the restatement: one good case per
    suite, then every listed condition broken on its own."""
    for suite in range(3):
        for ph in (0, 1):
            good = dict(d=_desc(), s0=(suite, ph), s1=(suite, 1 - ph))
            cases = [("good", good, True),
                     ("no_hp", dict(good, d=_desc(flags=L.F_NO_HP)), False),
                     ("no_hp with rfc", dict(good, d=_desc(flags=L.F_NO_HP | L.F_RFC_PN)), False),
                     ("rfc alone", dict(good, d=_desc(flags=L.F_RFC_PN)), True),
                     ("hdr 0", dict(good, d=_desc(hdr_len=0)), False),
                     ("hdr 1", dict(good, d=_desc(hdr_len=1)), True),
                     ("hdr max", dict(good, d=_desc(length=2000, hdr_len=L.MAX_HDR - 4)), True),
                     ("hdr past max", dict(good, d=_desc(length=2000, hdr_len=L.MAX_HDR - 3)), False),
                     ("len exact", dict(good, d=_desc(length=29)), True),
                     ("len 19 past", dict(good, d=_desc(length=28)), False),
                     ("len 0", dict(good, d=_desc(length=0)), False),
                     ("s0 empty", dict(good, s0=(EMPTY, ph)), False),
                     ("s0 unknown suite", dict(good, s0=(3, ph)), False),
                     ("s1 none", dict(good, s1=(EMPTY, 0)), False),
                     ("s1 other suite", dict(good, s1=((suite + 1) % 3, 1 - ph)), False),
                     ("s1 same phase", dict(good, s1=(suite, ph)), False)]
            for name, c, want in cases:
                d = c["d"]
                got = lib.ph_eligible(d.ctypes.data, c["s0"][0], c["s0"][1], c["s1"][0], c["s1"][1])
                table = {}
                if c["s0"][0] <= 2:
                    table[0] = (c["s0"][0], c["s0"][1], b"")
                if c["s1"][0] <= 2:
                    table[1] = (c["s1"][0], c["s1"][1], b"")
                assert bool(got) == want == P.eligible(d[0], table, 2, 1), (name, suite, ph)
                for b0 in (0x40, 0x44, 0x5B, 0xC4, 0x04):
                    for mask0 in (0x00, 0x04, 0x1F, 0xE4, 0xFF):
                        plain = b0 ^ (mask0 & 0x1F)
                        flips = not plain & 0x80 and ((plain >> 2) & 1) != c["s0"][1]
                        assert bool(lib.ph_flips(b0, mask0, c["s0"][1])) == flips
                        assert bool(lib.ph_decide(d.ctypes.data, b0, mask0, c["s0"][0], c["s0"][1], c["s1"][0],
                                                  c["s1"][1])) == (want and flips), (name, b0, mask0)


def test_sanitizer_program(tmp_path):
    """The lane under AddressSanitizer and UBSan, as a program of its own:
    packets that end with their sample's last byte, every truncation of them,
    and each condition failing alone, each on a heap buffer of exactly the
    packet's size."""
    exe = str(tmp_path / "phase_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "phase_host: ok" in r.stdout
