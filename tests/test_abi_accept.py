"""CPU checks of the new-connection entry points at the drop-in boundary
(include/quic_pp.h: qpp_route_accept, qpp_keytab_derive_initial_device,
qpp_session_accept_unprotect): declared, exported, and the record and the
constants the Python side uses match the header's.  No device calls."""

import ctypes
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quic_pp.h")
LIB = os.path.join(ROOT, "aioquic_amd", "libquicpp.so")

ENTRY_POINTS = ["qpp_route_accept", "qpp_route_accept_launches", "qpp_keytab_derive_initial_device",
                "qpp_session_accept_unprotect"]
STATUSES = ("OK", "ROUTED", "NOT_INITIAL", "VERSION", "SMALL", "CID", "NO_TOKEN")


def test_header_declares_and_library_exports_them():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"^\w[\w\s\*]*\b%s\s*\(" % name, src, flags=re.M), name
    for value, name in enumerate(STATUSES):
        assert re.search(r"#define\s+QPP_ACC_%s\s+%d\b" % (name, value), src), name
    assert re.search(r"#define\s+QPP_A_NEED_TOKEN\s+1u\b", src)
    assert re.search(r"#define\s+QPP_ABI_VERSION\s+3\b", src)
    assert os.path.exists(LIB), "build() first: aioquic_amd/libquicpp.so missing"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(ENTRY_POINTS) <= exported


def test_record_layout_and_constants_match_header():
    from aioquic_amd import layout as L

    src = open(HEADER).read()
    m = re.search(r"\}\s*qpp_accept_rec;\s*/\*\s*(\d+) bytes", src)
    assert m and int(m.group(1)) == 8 == L.ACCEPT.itemsize
    assert {name: L.ACCEPT.fields[name][1] for name in L.ACCEPT.names} == \
        {"desc": 0, "status": 4, "version": 5, "rsv": 6}
    assert [getattr(L, "ACC_" + name) for name in STATUSES] == list(range(7))
    assert L.A_NEED_TOKEN == 1

    # the same layout as a C compiler sees it
    class AcceptRec(ctypes.Structure):
        _fields_ = [("desc", ctypes.c_uint32), ("status", ctypes.c_uint8), ("version", ctypes.c_uint8),
                    ("rsv", ctypes.c_uint8 * 2)]

    assert ctypes.sizeof(AcceptRec) == 8
    assert (AcceptRec.desc.offset, AcceptRec.status.offset, AcceptRec.version.offset, AcceptRec.rsv.offset) == \
        (0, 4, 5, 6)


def test_header_struct_compiles_to_the_layout(tmp_path):
    """sizeof / offsetof of qpp_accept_rec as gcc sees the header itself."""
    from aioquic_amd import layout as L

    src = tmp_path / "acc.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quic_pp.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %d %u\\n", sizeof(qpp_accept_rec), '
                   'offsetof(qpp_accept_rec, desc), offsetof(qpp_accept_rec, status), '
                   'offsetof(qpp_accept_rec, version), offsetof(qpp_accept_rec, rsv), QPP_ACC_NO_TOKEN, '
                   'QPP_A_NEED_TOKEN); return 0; }\n')
    exe = str(tmp_path / "acc")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    got = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()
    f = L.ACCEPT.fields
    assert [int(x) for x in got] == [L.ACCEPT.itemsize, f["desc"][1], f["status"][1], f["version"][1], f["rsv"][1],
                                     L.ACC_NO_TOKEN, L.A_NEED_TOKEN]


def test_module_has_the_accept_api():
    from aioquic_amd import _crypto, batch_io, receive

    for name in ("route_accept", "receive_accept", "route_accept_launches"):
        assert hasattr(_crypto, name), name
    assert callable(receive.accept_routed) and hasattr(batch_io.KeySlots, "room")
    assert _crypto.abi_version() == 3


def test_accept_routed_refusals_that_need_no_device():
    from aioquic_amd import receive
    from aioquic_amd.receive import ConnectionKeys

    class Router:
        host_cid_length = 8

        def __init__(self, conns):
            self.conns = conns

    called = []
    assert receive.accept_routed(Router([]), [], called.append) == ([], [], [])
    client = ConnectionKeys(cryptos={}, spaces={}, is_client=True, host_cids=[b"\x01" * 8])
    try:
        receive.accept_routed(Router([None, client]), [b"\xc0" + bytes(1199)], called.append)
    except ValueError as e:
        assert "client" in str(e)
    else:
        raise AssertionError("a router that holds a client connection was taken")
    assert not called
