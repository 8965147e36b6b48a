"""CPU checks of the Retry-token validation.

aioquic_amd/csrc/qpp_token.h, what every lane of k_token and the token step of
k_accept_tokens run, is built for the host with g++ (tests/token_host.cc) and
compared -- the token's descriptor and the token record, byte for byte over
poisoned outputs -- with the Python restatement of tests/token_cases.py, which
is written from retry.py's validate_token and the varint rules, with the C
oracle's aead_decrypt standing in for the launch.  The same file's main(),
built with -fsanitize=address,undefined and run as a program of its own, is
the out-of-bounds check: every buffer a lane may touch lives on the heap at
exactly its size.
"""

import ctypes
import os
import socket
import subprocess
import sys
import types

import numpy as np
import pytest

from aioquic_amd import layout as L
from tests import token_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "token_host.cc")
u32, u64, vp, cp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_char_p
POISON = 0x5A


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("token_host") / "libtoken_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.tk_locate.restype = ctypes.c_int
    lib.tk_locate.argtypes = [cp, u32, u32, u32, u32, vp]
    lib.tk_desc.restype = u32
    lib.tk_desc.argtypes = [u32, u32, u32, u32, u32, u32, u64, cp, u32, vp]
    lib.tk_check.restype = u32
    lib.tk_check.argtypes = [u32, u32, u32, cp, cp, vp]
    return lib


def poisoned(dtype):
    return np.full(dtype.itemsize, POISON, np.uint8).view(dtype)


def run(lib, a, off, data, w, acc, flags, addr20, forced):
    """One candidate through the host build, each output over poisoned
    memory, next to the restatement; returns the final TK_* status."""
    desc, rec = poisoned(L.DESC), poisoned(L.TOKEN_REC)
    pre = lib.tk_desc(a, acc, flags, w["dcid_len"], w["scid_len"], w["token_len"], off, data, len(data),
                      desc.ctypes.data)
    want_desc, want_pre = T.restate_desc(a, acc, flags, w, off, data)
    assert pre == want_pre and desc.tobytes() == want_desc.tobytes()
    status, opened = T.restate_open(want_desc, off, data)
    if forced is not None:
        assert status == L.S_OK, "a forced status goes over a plaintext that would pass"
        status = forced
    got = lib.tk_check(pre, status, w["token_len"], opened, addr20, rec.ctypes.data)
    want = T.restate_check(want_pre, status, w["token_len"], opened, addr20)
    assert rec.tobytes() == want.tobytes() and got == int(want["status"][0])
    return got


def test_spelled_out_cases(lib):
    seen = set()
    names = set()
    for k, (name, data, w, acc, flags, addr20, forced, want) in enumerate(T.spelled_cases()):
        got = run(lib, 1 + k % 7, 3 + 2 * k, data, w, acc, flags, addr20, forced)
        assert got == want, name
        seen.add(got), names.add(name.split("-")[0])
    assert seen == T.ALL_TK
    assert {"len", "varint", "ends", "cut", "dl", "sl", "field", "empty", "trailing", "addr", "cid", "status"} <= names


def test_spelled_out_fields(lib):
    """One token against numbers written by hand."""
    token = T.seal(0x0102030405060708, T.plain_of(T.IPV4))
    data = T.initial(T.V2, T.DCID, T.SCID, token, tform=2)
    w = T.walk_of(data)
    assert (w["dcid_len"], w["scid_len"], w["token_len"]) == (8, 5, 8 + 28 + 16)
    desc, rec = poisoned(L.DESC), poisoned(L.TOKEN_REC)
    assert lib.tk_desc(3, L.ACC_OK, L.A_NEED_TOKEN, 8, 5, 52, 1001, data, len(data), desc.ctypes.data) == L.TK_OK
    start = 7 + 8 + 5 + 4
    assert data[start - 4:start] == bytes([0x80, 0, 0, 52]) and data[start:start + 52] == token
    assert (int(desc["in_off"][0]), int(desc["out_off"][0]), int(desc["len"][0]), int(desc["hdr_len"][0]),
            int(desc["flags"][0]), int(desc["pn"][0]), int(desc["slot"][0]), int(desc["rsv"][0])) == \
        (1001 + start, 3 * 128, 52, 8, L.F_NO_HP, 0x0102030405060708, 2, 0)
    at = u32(0)
    assert lib.tk_locate(data, len(data), 8, 5, 52, ctypes.byref(at)) == 1 and at.value == start
    assert lib.tk_locate(data, start + 51, 8, 5, 52, ctypes.byref(at)) == 0
    opened = (token[:8] + T.plain_of(T.IPV4)).ljust(128, b"\0")
    assert lib.tk_check(L.TK_OK, L.S_OK, 52, opened, T.R.packed_addr(T.IPV4), rec.ctypes.data) == L.TK_OK
    assert (int(rec["status"][0]), int(rec["odcid_len"][0]), int(rec["rscid_len"][0])) == (L.TK_OK, 11, 8)
    assert rec["odcid"][0, :11].tobytes() == T.ODCID and rec["rscid"][0, :8].tobytes() == T.RSCID
    assert not rec["odcid"][0, 11:].any() and not rec["rscid"][0, 8:].any() and not rec["rsv2"].any()


def test_restatement_is_validate_token_without_a_device(monkeypatch):
    """The restatement's verdicts against RetryTokens.validate_token itself,
    its cipher replaced by the oracle's: ValueError exactly where the verdict
    is not TK_OK, the same two CIDs where it is -- but for the two documented
    divergences."""
    from aioquic_amd import retry
    from oracle import oracle as orc

    class OracleAead:
        def decrypt(self, data, aad, pn):
            try:
                return orc.aead_decrypt(L.AES_128_GCM, T.TOKEN_KEY, T.TOKEN_IV, bytes(data), bytes(aad), pn)
            except ValueError:
                raise KeyError("decrypt") from None

    tokens = retry.RetryTokens(T.TOKEN_KEY, T.TOKEN_IV)
    tokens._aead = OracleAead()
    fake = types.ModuleType("aioquic_amd._crypto")
    fake.CryptoError = KeyError
    monkeypatch.setitem(sys.modules, "aioquic_amd._crypto", fake)
    monkeypatch.setattr(sys.modules["aioquic_amd"], "_crypto", fake, raising=False)
    n_ok = 0
    for name, data, w, acc, flags, addr20, forced, want in T.spelled_cases():
        if acc != L.ACC_OK or not flags or forced is not None or want == L.TK_BOUNDS:
            continue
        if addr20[0] not in (6, 18):
            continue
        start = T.restate_locate(data, w["dcid_len"], w["scid_len"], w["token_len"])
        token = data[start:start + w["token_len"]]
        host, port = addr20[1:addr20[0] - 1], int.from_bytes(addr20[addr20[0] - 1:addr20[0] + 1], "big")
        addr = (socket.inet_ntop(socket.AF_INET6 if len(host) == 16 else socket.AF_INET, host), port)
        desc, pre = T.restate_desc(0, acc, flags, w, 0, data)
        status, opened = T.restate_open(desc, 0, data)
        rec = T.restate_check(pre, status, w["token_len"], opened, addr20)
        assert int(rec["status"][0]) == want, name
        if name.startswith(("cid-21", "len-129")):
            continue  # the divergences: the host would return these
        if want == L.TK_OK:
            n_ok += 1
            assert tokens.validate_token(addr, token) == (rec["odcid"][0, :int(rec["odcid_len"][0])].tobytes(),
                                                          rec["rscid"][0, :int(rec["rscid_len"][0])].tobytes()), name
        else:
            with pytest.raises(ValueError):
                tokens.validate_token(addr, token)
    assert n_ok >= 8


def test_sanitizer_program(tmp_path):
    """The token logic under AddressSanitizer and UBSan, as a program of its
    own: a datagram that ends where its token ends, every truncation of it,
    walk records that disagree with the bytes, every plaintext that ends
    early, each on heap buffers of exactly their size."""
    exe = str(tmp_path / "token_host")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "token_host: ok" in r.stdout
