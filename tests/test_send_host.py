"""CPU checks of the routed-send lane.

aioquic_amd/csrc/qpp_send.h, what every lane of k_send runs, is built for the
host with g++ -Wall -Werror (tests/send_host.cc) and compared with the Python
restatement of tests/send_cases.py over a poisoned buffer: buffer, descriptors
and records byte for byte, over a batch that meets every case and with every
condition failing alone.  The fused form's host check is the same header's
batch_ok().  The same file's main(), built with -fsanitize=address,undefined
and run as a program of its own, is the out-of-bounds check: its packets live
in heap buffers of exactly the region's size.
"""

import ctypes
import os
import subprocess

import numpy as np
import pytest

from aioquic_amd import layout as L
from tests import send_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "send_host.cc")
u32, u64, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
SLOT = np.dtype([("suite", "<u4"), ("key_phase", "<u4")])


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("send_host") / "libsend_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.sn_lane.restype = u32
    lib.sn_lane.argtypes = [vp, u32, vp, u32, vp, vp, vp, vp, u32, vp, u64, vp, vp]
    lib.sn_batch_ok.restype = u32
    lib.sn_batch_ok.argtypes = [vp, u32, u32, vp, vp, vp, u32, u64, u64]
    lib.sn_const.restype = u32
    lib.sn_const.argtypes = [u32]
    return lib


def slot_array(slots: dict, cap: int):
    a = np.zeros(cap, SLOT)
    a["suite"] = S.EMPTY
    for s, (suite, phase) in slots.items():
        a[s] = (suite, phase)
    return a


def run_lanes(lib, conns, slots, cap, off, lens, conn, seq, buf, buf_len=None):
    """Every lane in turn over a copy of `buf`; descriptors and records start
    as 0xAB, so a field a lane leaves out shows."""
    n = len(off)
    buf = buf.copy()
    sa = slot_array(slots, cap)
    conns = np.ascontiguousarray(conns)
    off, lens = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(lens, np.uint32)
    conn, seq = np.ascontiguousarray(conn, np.uint32), np.ascontiguousarray(seq, np.uint32)
    desc = np.frombuffer(bytearray(b"\xab" * (n * 40)), L.DESC)
    rec = np.frombuffer(bytearray(b"\xab" * (n * 16)), L.SEND_REC)
    st = [lib.sn_lane(sa.ctypes.data, cap, conns.ctypes.data, len(conns), off.ctypes.data, lens.ctypes.data,
                      conn.ctypes.data, seq.ctypes.data, i, buf.ctypes.data, len(buf) if buf_len is None else buf_len,
                      desc.ctypes.data, rec.ctypes.data) for i in range(n)]
    assert st == rec["status"].tolist()
    return buf, desc, rec


def test_constants(lib):
    assert [lib.sn_const(k) for k in range(6)] == [L.SEND_PN_LEN, L.SEND_HEAD, L.SEND_TAIL, 1, L.SEND_CONN.itemsize,
                                                   L.SEND_REC.itemsize]
    assert L.SEND_HEAD == 1 + 20 + 2 and L.SEND_TAIL == 1 + 16


@pytest.mark.parametrize("n,fused", [(1, False), (257, False), (257, True)])
def test_lane_matches_restatement(lib, n, fused):
    w = S.World(n, fused=fused)
    want_buf, want_desc, want_rec = S.restate_world(w)
    buf, desc, rec = run_lanes(lib, w.conns, w.slots(), S.CAP, w.off, w.len, w.conn, w.seq, w.buf, w.buf_len)
    assert rec.tobytes() == want_rec.tobytes()
    assert desc.tobytes() == want_desc.tobytes()
    assert buf.tobytes() == want_buf.tobytes()
    if n == 1:
        assert rec["status"].tolist() == [L.SN_OK] and desc["len"][0] == 2, "the 1-byte payload is padded"
        return
    # the batch meets what it says it does
    ok = rec["status"] == L.SN_OK
    want = {L.SN_OK, L.SN_CID, L.SN_NO_KEY, L.SN_EMPTY, L.SN_PN} | (set() if fused else {L.SN_CONN, L.SN_ROOM})
    assert set(rec["status"].tolist()) == want
    assert [k for k, s in zip(w.kind, rec["status"]) if s != L.SN_OK] == [k for k in w.kind if k not in ("ok", "over")]
    used = w.conns[w.conn[ok]]
    slots = w.slots()
    assert {slots[int(s)][0] for s in used["slot"]} == {0, 1, 2}, "all three suites"
    assert {slots[int(s)][1] for s in used["slot"]} == {0, 1}, "both key phases"
    assert set(used["cid_len"].tolist()) == {0, 1, 8, 20} and set(used["spin"].tolist()) == {0, 1}
    assert {1, 2, 3, 1173} <= set(w.len[ok].tolist())
    assert any(int(h) + int(ln) + 16 == 1500 for h, ln in zip(rec["hdr_len"][ok], w.len[ok])), "the longest that fits"
    pn0 = rec["pn"][ok & (w.conn == 0)]
    assert pn0.min() < 1 << 16 <= pn0.max(), "crosses 2^16 inside one connection's run"
    assert (rec["pn"][ok & (w.conn == 1)] > 1 << 32).all() and (rec["pn"][ok] == S.PN_LIMIT - 1).any()
    # a padded packet's descriptor counts the padding
    one = ok & (w.len == 1)
    assert one.any() and (desc["len"][one] == 2).all()


def one_lane(lib, *, cid_len=8, slot=0, next_pn=5, spin=0, length=30, seq=0, conn=0, p_off=None, room=None,
             slots=None):
    """One lane over one connection; the buffer holds p_off bytes in front of
    the payload and `room` behind it.  Returns (status, agrees with restate)."""
    conns = np.zeros(1, L.SEND_CONN)
    conns["next_pn"], conns["slot"], conns["cid_len"], conns["spin"] = next_pn, slot, cid_len, spin
    conns["cid"][0] = np.arange(0x50, 0x50 + 20)
    slots = {0: (0, 0), 1: (2, 1)} if slots is None else slots
    p_off = L.SEND_HEAD if p_off is None else p_off
    room = L.SEND_TAIL if room is None else room
    buf = np.full(p_off + length + room, 0xEE, np.uint8)
    args = (conns, slots, 4, [p_off], [length], [conn], [seq], buf)
    want = S.restate(*args)
    got = run_lanes(lib, *args)
    same = all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    return int(got[2]["status"][0]), same


def test_each_condition_failing_alone(lib):
    for slot in (0, 1):
        for spin in (0, 1):
            assert one_lane(lib, slot=slot, spin=spin) == (L.SN_OK, True)
    assert one_lane(lib, conn=1) == (L.SN_CONN, True)
    assert one_lane(lib, conn=0xFFFFFFFF) == (L.SN_CONN, True)
    assert one_lane(lib, cid_len=20) == (L.SN_OK, True)
    assert one_lane(lib, cid_len=21, p_off=L.SEND_HEAD + 1) == (L.SN_CID, True)
    for slot in (2, 3, 4, 77, L.SLOT_NONE):  # empty, empty, past the table, none
        assert one_lane(lib, slot=slot) == (L.SN_NO_KEY, True)
    for length, st in ((0, L.SN_EMPTY), (1, L.SN_OK), (2, L.SN_OK), (3, L.SN_OK)):
        assert one_lane(lib, length=length) == (st, True)
    assert one_lane(lib, next_pn=S.PN_LIMIT - 1) == (L.SN_OK, True)
    assert one_lane(lib, next_pn=S.PN_LIMIT) == (L.SN_PN, True)
    assert one_lane(lib, next_pn=S.PN_LIMIT - 2, seq=1) == (L.SN_OK, True)
    assert one_lane(lib, next_pn=S.PN_LIMIT - 2, seq=2) == (L.SN_PN, True)
    assert one_lane(lib, next_pn=(1 << 64) - 1, seq=1) == (L.SN_PN, True), "a wrapping sum"
    assert one_lane(lib, next_pn=(1 << 64) - 3, seq=0xFFFFFFFF) == (L.SN_PN, True)
    for cid_len in (0, 1, 8, 20):
        hs = 1 + cid_len + 2
        assert one_lane(lib, cid_len=cid_len, p_off=hs) == (L.SN_OK, True)
        assert one_lane(lib, cid_len=cid_len, p_off=hs - 1) == (L.SN_ROOM, True)
        for length in (1, 2, 3, 1173):
            need = S.padding_size(length) + 16
            assert one_lane(lib, cid_len=cid_len, length=length, room=need) == (L.SN_OK, True), "the last byte of room"
            assert one_lane(lib, cid_len=cid_len, length=length, room=need - 1) == (L.SN_ROOM, True), "one short"
    # the first failing check names the status
    assert one_lane(lib, conn=1, cid_len=21, slot=9, length=0)[0] == L.SN_CONN
    assert one_lane(lib, cid_len=21, slot=9, length=0, p_off=0)[0] == L.SN_CID
    assert one_lane(lib, slot=9, length=0, next_pn=S.PN_LIMIT, p_off=0)[0] == L.SN_NO_KEY
    assert one_lane(lib, length=0, next_pn=S.PN_LIMIT, p_off=0)[0] == L.SN_EMPTY
    assert one_lane(lib, next_pn=S.PN_LIMIT, p_off=0)[0] == L.SN_PN


def test_header_bytes(lib):
    """The first byte, bit by bit, and the number's low sixteen bits."""
    for slot, phase in ((0, 0), (1, 1)):
        for spin in (0, 1):
            for pn in (0, 0xFFFF, 0x10000, 0x123456789A, S.PN_LIMIT - 1):
                conns = np.zeros(1, L.SEND_CONN)
                conns["next_pn"], conns["slot"], conns["cid_len"], conns["spin"] = pn, slot, 3, spin
                conns["cid"][0, :3] = (1, 2, 3)
                buf = np.full(64, 0xEE, np.uint8)
                got, _, _ = run_lanes(lib, conns, {0: (0, 0), 1: (2, 1)}, 4, [30], [5], [0], [0], buf)
                want = bytes([0x40 | spin << 5 | phase << 2 | 1, 1, 2, 3, (pn >> 8) & 0xFF, pn & 0xFF])
                assert got[24:30].tobytes() == want and (got[:24] == 0xEE).all() and (got[30:] == 0xEE).all()


def test_batch_ok(lib):
    """The fused form's host check: everything it must refuse, one at a time."""
    w = S.World(257, fused=True)

    def ok(off=w.off, lens=w.len, conn=w.conn, conns=w.conns, in_len=w.buf_len, out_len=w.buf_len, cap=S.CAP):
        off, lens = np.ascontiguousarray(off, np.uint64), np.ascontiguousarray(lens, np.uint32)
        conn, conns = np.ascontiguousarray(conn, np.uint32), np.ascontiguousarray(conns)
        return bool(lib.sn_batch_ok(conns.ctypes.data, len(conns), cap, off.ctypes.data, lens.ctypes.data,
                                    conn.ctypes.data, len(off), in_len, out_len))

    assert ok()
    assert ok(in_len=w.buf_len + 9) and ok(out_len=w.buf_len + 9)
    assert not ok(in_len=w.buf_len - 1) and not ok(out_len=w.buf_len - 1), "a region past either buffer"
    off = w.off.copy()
    off[100] -= 1
    assert not ok(off=off), "a region one byte into its predecessor's"
    off = w.off.copy()
    off[0] -= 1
    assert not ok(off=off), "a region in front of the buffer"
    off = w.off.copy()
    off[[50, 51]] = off[[51, 50]]
    assert not ok(off=off), "offsets out of order"
    off = w.off.copy()
    off[51] = off[50]
    assert not ok(off=off), "offsets not strictly increasing"
    lens = w.len.copy()
    lens[60] += 1
    assert not ok(lens=lens), "a longer payload overlaps its successor"
    conn = w.conn.copy()
    conn[7] = S.N_CONN
    assert not ok(conn=conn), "a connection index out of range"
    conns = w.conns.copy()
    conns["slot"][3] = S.CAP
    assert not ok(conns=conns), "a slot past the table"
    assert ok(cap=int(w.conns["slot"][w.conns["slot"] != L.SLOT_NONE].max()) + 1)
    assert not ok(cap=int(w.conns["slot"][w.conns["slot"] != L.SLOT_NONE].max()))
    huge = w.off.copy()
    huge[-1] = (1 << 64) - 5
    assert not ok(off=huge)
    lens = w.len.copy()
    lens[-1] = 0xFFFFFFFF
    assert not ok(lens=lens)


def test_sanitizer_program(tmp_path):
    """The lane under AddressSanitizer and UBSan, as a program of its own: a
    region of exactly header, payload, padding and tag, every truncation of it
    at both ends, and each condition failing alone, each on a heap buffer of
    exactly that size."""
    exe = str(tmp_path / "send_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "send_host: ok" in r.stdout
