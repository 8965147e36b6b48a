"""CPU checks of the routing entry points at the drop-in boundary
(include/quic_pp.h: qpp_cidmap_*, qpp_route, qpp_session_route_unprotect):
declared, exported, and the records the Python side builds match the header's
structs.  No device calls."""

import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quic_pp.h")
LIB = os.path.join(ROOT, "aioquic_amd", "libquicpp.so")

ENTRY_POINTS = ["qpp_cidmap_create", "qpp_cidmap_destroy", "qpp_cidmap_count", "qpp_cidmap_put", "qpp_cidmap_remove",
                "qpp_cidmap_find", "qpp_cidmap_home", "qpp_cidmap_buckets", "qpp_route",
                "qpp_session_route_unprotect"]


def test_header_declares_and_library_exports_them():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"^\w[\w\s\*]*\b%s\s*\(" % name, src, flags=re.M), name
    assert re.search(r"#define\s+QPP_CONN_NONE\s+0xffffffffu", src)
    for name, value in (("SHORT", 0), ("LONG", 1), ("UNKNOWN_CID", 2), ("MALFORMED", 3), ("BAD_CONN", 4)):
        assert re.search(r"#define\s+QPP_R_%s\s+%d\b" % (name, value), src)
    assert re.search(r"#define\s+QPP_ABI_VERSION\s+3\b", src)
    assert os.path.exists(LIB), "build() first: aioquic_amd/libquicpp.so missing"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(ENTRY_POINTS) <= exported


def test_record_layouts_match_header():
    from aioquic_amd import layout as L

    src = open(HEADER).read()
    m = re.search(r"\}\s*qpp_cid_entry;\s*/\*\s*(\d+) bytes", src)
    assert m and int(m.group(1)) == 32 == L.CID_ENTRY.itemsize
    m = re.search(r"\}\s*qpp_route_rec;\s*/\*\s*(\d+) bytes", src)
    assert m and int(m.group(1)) == 8 == L.ROUTE.itemsize
    off = {name: L.CID_ENTRY.fields[name][1] for name in L.CID_ENTRY.names}
    assert off == {"conn": 0, "cid_len": 4, "rsv": 5, "cid": 8, "rsv2": 28}
    assert {name: L.ROUTE.fields[name][1] for name in L.ROUTE.names} == {"conn": 0, "cls": 4, "rsv": 5}
    assert L.CONN_NONE == 0xFFFFFFFF

    # the same layouts as a C compiler sees them
    class CidEntry(ctypes.Structure):
        _fields_ = [("conn", ctypes.c_uint32), ("cid_len", ctypes.c_uint8), ("rsv", ctypes.c_uint8 * 3),
                    ("cid", ctypes.c_uint8 * 20), ("rsv2", ctypes.c_uint32)]

    class RouteRec(ctypes.Structure):
        _fields_ = [("conn", ctypes.c_uint32), ("cls", ctypes.c_uint8), ("rsv", ctypes.c_uint8 * 3)]

    assert ctypes.sizeof(CidEntry) == 32 and CidEntry.cid.offset == 8 and CidEntry.rsv2.offset == 28
    assert ctypes.sizeof(RouteRec) == 8 and RouteRec.cls.offset == 4


def test_module_has_the_routing_api():
    from aioquic_amd import _crypto

    assert _crypto.CID_ENTRY_SIZE == 32 and _crypto.ROUTE_SIZE == 8
    for name in ("CidMap", "route", "route_unprotect_host", "receive_routed"):
        assert hasattr(_crypto, name)
    assert _crypto.abi_version() == 3
