"""CPU checks of the token entry points at the drop-in boundary
(include/quic_pp.h: qpp_route_token, qpp_route_token_launches,
qpp_route_accept_tokens, qpp_session_serve_unprotect): declared, exported,
bound, and the record and the constants the Python side uses match the
header's.  No device calls."""

import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quic_pp.h")
LIB = os.path.join(ROOT, "aioquic_amd", "libquicpp.so")

ENTRY_POINTS = ["qpp_route_token", "qpp_route_token_launches", "qpp_route_accept_tokens",
                "qpp_session_serve_unprotect"]
DEFINES = {"QPP_TOKEN_STRIDE": "128", "QPP_TOKEN_MIN": "27", "QPP_TOKEN_MAX": "128", "QPP_ACC_BAD_TOKEN": "7",
           "QPP_TK_OK": "0", "QPP_TK_NONE": "1", "QPP_TK_LENGTH": "2", "QPP_TK_BOUNDS": "3", "QPP_TK_AUTH": "4",
           "QPP_TK_FORM": "5", "QPP_TK_ADDR": "6", "QPP_ACC_NO_TOKEN": "6"}


def test_header_declares_and_library_exports_them():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"^\w[\w\s\*]*\b%s\s*\(" % name, src, flags=re.M), name
    for name, value in DEFINES.items():
        assert re.search(r"#define\s+%s\s+%s\b" % (name, value), src), name
    # each entry point's comment cites what it replaces
    for name in ("qpp_route_token", "qpp_session_serve_unprotect"):
        at = re.search(r"^int %s\(" % name, text, flags=re.M).start()
        comment = text[text.rfind("\n/* ", 0, at):at]
        for cite in ("server.py:112-120", "retry.py"):
            assert cite in comment, (name, cite)
    assert os.path.exists(LIB), "build() first: aioquic_amd/libquicpp.so missing"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(ENTRY_POINTS) <= exported


def test_record_layout_and_constants_match_header(tmp_path):
    """sizeof / offsetof of qpp_token_rec as gcc sees the header itself."""
    from aioquic_amd import layout as L

    src = tmp_path / "tk.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quic_pp.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d %d %d %d %d %d %d\\n", '
                   'sizeof(qpp_token_rec), offsetof(qpp_token_rec, status), offsetof(qpp_token_rec, odcid_len), '
                   'offsetof(qpp_token_rec, rscid_len), offsetof(qpp_token_rec, rsv), offsetof(qpp_token_rec, odcid), '
                   'offsetof(qpp_token_rec, rscid), offsetof(qpp_token_rec, rsv2), QPP_TOKEN_STRIDE, QPP_TOKEN_MIN, '
                   'QPP_TOKEN_MAX, QPP_ACC_BAD_TOKEN, QPP_TK_OK, QPP_TK_NONE, QPP_TK_LENGTH, QPP_TK_BOUNDS, '
                   'QPP_TK_AUTH, QPP_TK_FORM, QPP_TK_ADDR); return 0; }\n')
    exe = str(tmp_path / "tk")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    f = L.TOKEN_REC.fields
    assert got == [L.TOKEN_REC.itemsize, f["status"][1], f["odcid_len"][1], f["rscid_len"][1], f["rsv"][1],
                   f["odcid"][1], f["rscid"][1], f["rsv2"][1], L.TOKEN_STRIDE, L.TOKEN_MIN, L.TOKEN_MAX,
                   L.ACC_BAD_TOKEN, L.TK_OK, L.TK_NONE, L.TK_LENGTH, L.TK_BOUNDS, L.TK_AUTH, L.TK_FORM, L.TK_ADDR]
    assert L.TOKEN_REC.itemsize == 48 and L.ACC_BAD_TOKEN == L.ACC_NO_TOKEN + 1
    assert L.TOKEN_MIN == 8 + 3 + 16 and 8 + (L.TOKEN_MAX - 24) <= L.TOKEN_STRIDE
    assert len({L.TK_OK, L.TK_NONE, L.TK_LENGTH, L.TK_BOUNDS, L.TK_AUTH, L.TK_FORM, L.TK_ADDR}) == 7


def test_module_has_the_token_api():
    from aioquic_amd import _crypto, receive
    from aioquic_amd.batch import PacketEngine

    for name in ("route_token", "route_token_launches", "route_accept_tokens", "receive_serve"):
        assert hasattr(_crypto, name), name
    assert callable(PacketEngine.route_token) and callable(PacketEngine.route_accept_tokens)
    assert callable(receive.serve_routed)
    assert _crypto.abi_version() == 3, "nothing that existed changed"


def test_serve_routed_surface_and_its_neighbours_unchanged():
    from aioquic_amd import receive

    p = inspect.signature(receive.serve_routed).parameters
    assert list(p) == ["router", "datagrams", "addrs", "accept", "tokens", "supported_versions"]
    assert p["tokens"].kind == p["supported_versions"].kind == inspect.Parameter.KEYWORD_ONLY
    assert p["tokens"].default is inspect.Parameter.empty and tuple(p["supported_versions"].default) == (1, 0x6B3343CF)
    with pytest.raises(ValueError):
        receive.serve_routed(None, [b"x"], [None], None, tokens=None)
    with pytest.raises(TypeError):
        receive.serve_routed(None, [], [], None)
    from aioquic_amd.retry import RetryTokens

    assert receive.serve_routed(None, [], [], None, tokens=RetryTokens()) == ([], [], [], [], [])
    assert receive.answer_routed(None, [], [], None) == ([], [], [], [])
    p = inspect.signature(receive.answer_routed).parameters
    assert list(p) == ["router", "datagrams", "addrs", "accept", "tokens", "supported_versions"]
    assert p["tokens"].default is None
