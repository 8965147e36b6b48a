"""CPU checks of the routed-send entry points at the drop-in boundary
(include/quic_pp.h: qpp_send_fill, qpp_send_launches, qpp_session_send_protect):
declared, exported, bound, and the records and constants the Python side uses
match the header's.  No device calls."""

import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quic_pp.h")
LIB = os.path.join(ROOT, "aioquic_amd", "libquicpp.so")

ENTRY_POINTS = ["qpp_send_fill", "qpp_send_launches", "qpp_session_send_protect"]
CONN_FIELDS = ["next_pn", "slot", "cid_len", "spin", "cid", "rsv"]
REC_FIELDS = ["pn", "hdr_len", "status", "rsv"]
CONSTANTS = ["QPP_SEND_PN_LEN", "QPP_SEND_HEAD", "QPP_SEND_TAIL", "QPP_SN_OK", "QPP_SN_CONN", "QPP_SN_CID",
             "QPP_SN_NO_KEY", "QPP_SN_EMPTY", "QPP_SN_PN", "QPP_SN_ROOM", "QPP_ABI_VERSION"]


def test_header_declares_and_library_exports_them():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"^\w[\w\s\*]*\b%s\s*\(" % name, src, flags=re.M), name
    assert re.search(r"#define\s+QPP_ABI_VERSION\s+3\b", src), "the change only adds entry points"
    # the comments cite the reference's builder and state the caller's contract
    at = re.search(r"^int qpp_send_fill\(", text, flags=re.M).start()
    comment = text[text.rfind("routed send", 0, at):at]
    for cite in ("packet_builder.py:19-20", "264-296", "330-339", "pairwise disjoint", "QPP_SEND_HEAD",
                 "QPP_SEND_TAIL", "QPP_E_ARG", "QPP_SLOT_NONE", "QPP_S_LENGTH"):
        assert cite in comment, cite
    assert os.path.exists(LIB), "build() first: aioquic_amd/libquicpp.so missing"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(ENTRY_POINTS) <= exported


def test_records_and_constants_match_header(tmp_path):
    """sizeof / offsetof of the two records and the constants as gcc sees the
    header itself."""
    from aioquic_amd import layout as L

    exprs = (["sizeof(qpp_send_conn)"] + ["offsetof(qpp_send_conn, %s)" % f for f in CONN_FIELDS]
             + ["sizeof(qpp_send_rec)"] + ["offsetof(qpp_send_rec, %s)" % f for f in REC_FIELDS] + CONSTANTS)
    src = tmp_path / "sn.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quic_pp.h"\n'
                   'int main(void) { printf("' + "%lu " * len(exprs) + '\\n", '
                   + ", ".join("(unsigned long)(%s)" % e for e in exprs) + '); return 0; }\n')
    exe = str(tmp_path / "sn")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    c, r = L.SEND_CONN.fields, L.SEND_REC.fields
    assert got == ([L.SEND_CONN.itemsize] + [c[f][1] for f in CONN_FIELDS] + [L.SEND_REC.itemsize]
                   + [r[f][1] for f in REC_FIELDS]
                   + [L.SEND_PN_LEN, L.SEND_HEAD, L.SEND_TAIL, L.SN_OK, L.SN_CONN, L.SN_CID, L.SN_NO_KEY, L.SN_EMPTY,
                      L.SN_PN, L.SN_ROOM, 3])
    assert L.SEND_CONN.itemsize == 40 and list(L.SEND_CONN.names) == CONN_FIELDS
    assert L.SEND_REC.itemsize == 16 and list(L.SEND_REC.names) == REC_FIELDS
    assert c["cid"][0].shape == (20,)
    # derived, not guessed: the longest header; the largest padding and the tag
    assert L.SEND_HEAD == 1 + L.CID_MAX + L.SEND_PN_LEN == 23
    assert L.SEND_TAIL == (4 - L.SEND_PN_LEN - 1) + L.TAG_LEN == 17


def test_packing_helper():
    from aioquic_amd import layout as L

    rec = L.send_conn((1 << 40) + 3, 9, b"\x01\x02\x03", spin=True)
    assert rec.dtype == L.SEND_CONN and len(rec) == 1
    r = rec[0]
    assert (r["next_pn"], r["slot"], r["cid_len"], r["spin"]) == ((1 << 40) + 3, 9, 3, 1)
    assert r["cid"].tobytes() == b"\x01\x02\x03" + bytes(17) and r["rsv"].tobytes() == bytes(6)
    none = L.send_conn(0, L.SLOT_NONE, b"")[0]
    assert none["slot"] == L.SLOT_NONE and none["cid_len"] == 0 and none["spin"] == 0
    assert L.send_conn(0, 0, bytes(20))[0]["cid_len"] == 20
    with pytest.raises(ValueError):
        L.send_conn(0, 0, bytes(21))


def test_module_has_the_send_api():
    from aioquic_amd import _crypto, send
    from aioquic_amd.batch import PacketEngine

    for name in ("send_fill", "send_launches", "send_protect_host", "send_routed"):
        assert callable(getattr(_crypto, name)), name
    assert callable(PacketEngine.send_fill) and callable(PacketEngine.send_protect_host)
    p = inspect.signature(send.send_routed).parameters
    assert list(p) == ["conns", "items", "slots"]
    assert p["slots"].kind is inspect.Parameter.KEYWORD_ONLY and p["slots"].default is None
    assert _crypto.abi_version() == 3, "nothing that existed changed"
    assert isinstance(_crypto.send_launches(), int)
    c = send.SendConnection(object(), b"\x01" * 8, packet_number=7, spin_bit=True)
    assert (c.peer_cid, c.packet_number, c.spin_bit) == (b"\x01" * 8, 7, True)
    with pytest.raises(ValueError):
        send.SendConnection(object(), bytes(21))


class _Ctx:
    def __init__(self, valid=True):
        self._valid = valid

    def is_valid(self):
        return self._valid


class _Pair:
    _update_key_requested = True  # must still be pending after a refused call

    def __init__(self, valid=True):
        self.send = _Ctx(valid)

    def _update_key(self, trigger):
        raise AssertionError("a refused call moved a key")


def test_send_routed_refuses_before_anything_moves():
    """Every refusal of send.send_routed's own: raised before a key is
    updated, a slot is assigned or a packet number moves (slots=object()
    would fail on any use)."""
    from aioquic_amd import send
    from aioquic_amd.crypto import KeyUnavailableError

    conns = [send.SendConnection(_Pair(), b"\x01" * 8, 5), send.SendConnection(_Pair(valid=False), b"", 9),
             send.SendConnection(_Pair(), bytes(20), 11)]
    nothing = object()
    assert send.send_routed(conns, [], slots=nothing) == ([], [])
    for items in ([(0, b"x"), (0, b"")], [(3, b"x")], [(-1, b"x")], [(0, bytes(1500 - 16 - 11 + 1))],
                  [(2, bytes(1500 - 16 - 23 + 1))]):
        with pytest.raises(ValueError):
            send.send_routed(conns, items, slots=nothing)
    with pytest.raises(KeyUnavailableError):
        send.send_routed(conns, [(0, b"x"), (1, b"y")], slots=nothing)
    assert [c.packet_number for c in conns] == [5, 9, 11]
