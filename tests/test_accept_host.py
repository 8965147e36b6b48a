"""CPU checks of the new-connection decision.

aioquic_amd/csrc/qpp_accept.h, the decision every lane of k_accept runs, is
built for the host with g++ (tests/accept_host.cc) and compared -- verdict,
qpp_initial record, descriptor and accept record, byte for byte -- with the
Python restatement of tests/accept_cases.py over the restated walk of
tests/walk_cases.py.  The same file's main(), built with
-fsanitize=address,undefined and run as a program of its own, is the
out-of-bounds check: its inputs live in heap buffers of exactly the datagram's
size.
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from aioquic_amd import layout as L
from tests import accept_cases as A
from tests import walk_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "accept_host.cc")
u32, u64, vp, cp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_char_p
POISON = 0x5A


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("accept_host") / "libaccept_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.ac_accept.restype = u32
    lib.ac_accept.argtypes = [cp, u32, u32, u32, u64, u32, u32, u32, u32, u32, u32, vp, vp, vp]
    lib.ac_accept_rec.restype = u32
    lib.ac_accept_rec.argtypes = [cp, u32, u32, u64, u32, u32, u32, vp, u32, u32, u32, u32, vp, vp, vp]
    return lib


def decide(lib, data: bytes, route, flags: int, *, i=5, off=0x1_0000_0123, slots=(10, 11), desc_flags=2, cid_len=8,
           rec=None):
    """The host build's outputs, each over poisoned memory, next to the
    restatement's; returns the status."""
    ini = np.full(1, POISON, np.uint8).repeat(L.INITIAL.itemsize).view(L.INITIAL)
    desc = np.full(1, POISON, np.uint8).repeat(L.DESC.itemsize).view(L.DESC)
    acc = np.full(1, POISON, np.uint8).repeat(L.ACCEPT.itemsize).view(L.ACCEPT)
    if rec is None:
        recs = C.restate_walk(data, cid_len)
        st = lib.ac_accept(data, len(data), cid_len, i, off, route[0], route[1], slots[0], slots[1], flags,
                           desc_flags, ini.ctypes.data, desc.ctypes.data, acc.ctypes.data)
    else:
        recs = [rec]
        w = np.zeros(1, L.WALK)
        for f in C.FIELDS:
            w[f] = rec[f]
        w["desc"] = A.NONE
        st = lib.ac_accept_rec(data, len(data), i, off, route[0], route[1], 1, w.ctypes.data, slots[0], slots[1],
                               flags, desc_flags, ini.ctypes.data, desc.ctypes.data, acc.ctypes.data)
    w_ini, w_desc, w_acc = A.restate(data, i, off, route, recs, slots[0], slots[1], flags, desc_flags)
    assert st == int(w_acc["status"][0]) == int(acc["status"][0])
    assert ini.tobytes() == w_ini.tobytes() and acc.tobytes() == w_acc.tobytes()
    if w_desc is None:
        assert desc.tobytes() == bytes([POISON]) * L.DESC.itemsize, "a rejected candidate's descriptor is left alone"
    else:
        assert desc.tobytes() == w_desc.tobytes()
    return st


def test_spelled_out_statuses(lib):
    seen = set()
    for name, data, route, flags, want in A.spelled_cases():
        assert decide(lib, data, route, flags) == want, name
        seen.add(want)
    assert seen == set(range(7)), "every QPP_ACC_* status was met"


def test_spelled_out_fields(lib):
    dcid = bytes(range(0x31, 0x31 + 20))
    data = A.initial(C.V2, dcid, 1200, token=b"tok")
    ini = np.zeros(1, L.INITIAL)
    desc = np.zeros(1, L.DESC)
    acc = np.zeros(1, L.ACCEPT)
    st = lib.ac_accept(data, len(data), 8, 77, 4099, A.NONE, L.R_LONG, 6, A.NONE, L.A_NEED_TOKEN, 0,
                       ini.ctypes.data, desc.ctypes.data, acc.ctypes.data)
    assert st == L.ACC_OK
    assert (int(ini["slot_client"][0]), int(ini["slot_server"][0])) == (6, A.NONE)
    assert (int(ini["cid_len"][0]), int(ini["flags"][0])) == (20, L.DERIVE_V2) and ini["cid"][0].tobytes() == dcid
    pn_off = 1 + 4 + 1 + 20 + 1 + 8 + 1 + 3 + 2
    assert (int(desc["in_off"][0]), int(desc["out_off"][0]), int(desc["len"][0]), int(desc["hdr_len"][0])) == \
        (4099, 4099, 1200, pn_off)
    assert (int(desc["pn"][0]), int(desc["slot"][0]), int(desc["flags"][0]), int(desc["rsv"][0])) == (0, 6, 0, 0)
    assert (int(acc["desc"][0]), int(acc["status"][0]), int(acc["version"][0])) == (77, 0, 1)


def test_hand_built_headers(lib):
    """The header forms of the walk's own cases, as unrouted long headers and
    as what the router knew: accepted only when they are whole Initials of at
    least 1200 bytes."""
    met = set()
    for name, data in C.hand_cases():
        for route in ((A.NONE, L.R_LONG), (1, L.R_LONG), (A.NONE, L.R_MALFORMED)):
            for flags in (0, L.A_NEED_TOKEN):
                met.add(decide(lib, data, route, flags))
        # the same header at the start of a datagram of 1200 bytes and more
        if data and data[0] & 0x80:
            for size in (1199, 1200, 1201):
                padded = (data + bytes(size))[:size]
                met.add(decide(lib, padded, (A.NONE, L.R_LONG), 0))
                met.add(decide(lib, padded, (A.NONE, L.R_LONG), L.A_NEED_TOKEN))
    assert {L.ACC_OK, L.ACC_ROUTED, L.ACC_NOT_INITIAL, L.ACC_VERSION, L.ACC_SMALL, L.ACC_NO_TOKEN} <= met


@pytest.mark.parametrize("cid_len", [1, 20])
def test_other_cid_lengths(lib, cid_len):
    for name, data in C.hand_cases(bytes([0xC1]) * cid_len):
        padded = (data + bytes(1200))[:1200]
        decide(lib, padded, (A.NONE, L.R_LONG), 0, cid_len=cid_len)


def test_records_the_walk_would_not_write(lib):
    """The decision takes the record as it finds it: an Initial that is not at
    offset 0, a DCID length past 20 or past the datagram, a non-OK status."""
    data = A.initial(C.V1, b"\xD8" * 8, 1200)
    good = C.restate_walk(data, 8)[0]
    assert decide(lib, data, (A.NONE, L.R_LONG), 0, rec=good) == L.ACC_OK
    for change, want in ((dict(off=1), L.ACC_NOT_INITIAL), (dict(status=C.W_HOST), L.ACC_NOT_INITIAL),
                         (dict(status=C.W_PARSE), L.ACC_NOT_INITIAL), (dict(type=2), L.ACC_NOT_INITIAL),
                         (dict(dcid_len=21), L.ACC_CID), (dict(dcid_len=255), L.ACC_CID),
                         (dict(dcid_len=0), L.ACC_CID), (dict(version=0), L.ACC_VERSION)):
        assert decide(lib, data, (A.NONE, L.R_LONG), 0, rec=dict(good, **change)) == want, change
    # the length test comes before the DCID test, and uses the caller's length
    assert decide(lib, data[:20], (A.NONE, L.R_LONG), 0, rec=good) == L.ACC_SMALL


def test_sanitizer_program(tmp_path):
    """The decision under AddressSanitizer and UBSan, as a program of its own:
    every truncation of an accepted datagram's first 6 + dcid_len bytes, each
    on a heap buffer of exactly its size."""
    exe = str(tmp_path / "accept_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "accept_host: ok" in r.stdout
