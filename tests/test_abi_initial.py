"""CPU checks of the Initial-key entry point at the drop-in boundary
(qpp_keytab_derive_initial, include/quic_pp.h): declared, exported, and the
record the Python side builds matches the header's struct.  No device calls."""

import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quic_pp.h")
LIB = os.path.join(ROOT, "aioquic_amd", "libquicpp.so")


def test_header_declares_and_library_exports_it():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"^int\s+qpp_keytab_derive_initial\s*\(\s*qpp_keytab\s*\*kt,\s*const\s+qpp_initial\s*\*ini,"
                     r"\s*uint32_t\s+n,\s*qpp_key_material\s*\*km_out,\s*uint8_t\s*\*secrets_out,"
                     r"\s*void\s*\*stream\s*\)\s*;", src, flags=re.M)
    assert re.search(r"#define\s+QPP_SLOT_NONE\s+0xffffffffu", src)
    assert re.search(r"#define\s+QPP_CID_MAX\s+20\b", src)
    assert os.path.exists(LIB), "build() first: aioquic_amd/libquicpp.so missing"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "qpp_keytab_derive_initial" in exported


def test_record_layout_matches_header():
    from aioquic_amd import layout as L

    src = open(HEADER).read()
    m = re.search(r"\}\s*qpp_initial;\s*/\*\s*(\d+) bytes", src)
    assert m and int(m.group(1)) == 32 == L.INITIAL.itemsize
    off = {name: L.INITIAL.fields[name][1] for name in L.INITIAL.names}
    assert off["slot_client"] == 0 and off["slot_server"] == 4
    assert off["cid_len"] == 8 and off["flags"] == 9 and off["cid"] == 12
    assert L.SLOT_NONE == 0xFFFFFFFF and L.CID_MAX == 20

    # the same layout as a C compiler sees it
    class Initial(ctypes.Structure):
        _fields_ = [("slot_client", ctypes.c_uint32), ("slot_server", ctypes.c_uint32),
                    ("cid_len", ctypes.c_uint8), ("flags", ctypes.c_uint8),
                    ("rsv", ctypes.c_uint8 * 2), ("cid", ctypes.c_uint8 * 20)]

    assert ctypes.sizeof(Initial) == 32
    assert Initial.slot_server.offset == 4 and Initial.cid_len.offset == 8 and Initial.cid.offset == 12


def test_initial_record_round_trips():
    from aioquic_amd import layout as L

    cid = bytes(range(1, 9))
    rec = L.initial_record(5, L.SLOT_NONE, cid, v2=True)
    assert rec.dtype == L.INITIAL and rec.shape == (1,)
    raw = rec.tobytes()
    assert len(raw) == 32
    assert raw[:4] == (5).to_bytes(4, "little") and raw[4:8] == b"\xff" * 4
    assert raw[8] == 8 and raw[9] == L.DERIVE_V2 and raw[10:12] == b"\0\0"
    assert raw[12:20] == cid and raw[20:] == bytes(12)
    back = np.frombuffer(raw, dtype=L.INITIAL)[0]
    assert back["slot_client"] == 5 and back["slot_server"] == L.SLOT_NONE
    assert bytes(back["cid"][: back["cid_len"]]) == cid
    assert L.initial_record(0, 1, b"")["cid_len"][0] == 0 and L.initial_record(0, 1, b"")["flags"][0] == 0
    assert L.initial_record(0, 1, bytes(20))["cid_len"][0] == 20
    with pytest.raises(ValueError):
        L.initial_record(0, 1, bytes(21))


def test_abi_version_unchanged():
    import aioquic_amd  # noqa: F401  (binds torch's HIP runtime first)

    lib = ctypes.CDLL(LIB)
    lib.qpp_abi_version.restype = ctypes.c_int
    assert lib.qpp_abi_version() == 3
    assert lib.qpp_keytab_derive_initial
