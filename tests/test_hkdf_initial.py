"""CPU check of the Initial key derivation of aioquic_amd/csrc/qpp_hkdf.h
(derive_initial, the function each lane of k_derive_initial runs, built for the
host here) against the RFC 9001 / 9369 Appendix-A vectors and the oracle's
stdlib restatement of quic/crypto.py:201-227."""

import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V2 = 0x6B3343CF


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hkdf_initial") / "libhkdf_initial_host.so")
    subprocess.run(["g++", "-O1", "-std=c++17", "-shared", "-fPIC", "-o", so,
                    os.path.join(ROOT, "tests", "hkdf_initial_host.cc")], check=True)
    lib = ctypes.CDLL(so)
    lib.qpp_test_derive_initial.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_int, ctypes.c_char_p]
    lib.qpp_test_salt_pads.argtypes = [ctypes.c_void_p]
    lib.qpp_test_hmac_init.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_void_p]
    return lib


def _derive(lib, cid, version, server, fill=0):
    """(secret, key, iv, hp); the record's bytes past the cid are `fill`."""
    buf = cid + bytes([fill]) * (20 - len(cid))
    out = ctypes.create_string_buffer(76)
    lib.qpp_test_derive_initial(buf, len(cid), int(version == V2), int(server), out)
    raw = out.raw
    return raw[:32], raw[32:48], raw[48:60], raw[60:76]


@pytest.mark.parametrize("tag", ["v1", "v2"])
def test_rfc_vectors(lib, tag):
    from tests.rfc import V1, V2 as RV2

    v = V1 if tag == "v1" else RV2
    assert _derive(lib, v.cid, v.version, False) == tuple(v.derive_client)
    assert _derive(lib, v.cid, v.version, True) == tuple(v.derive_server)


@pytest.mark.parametrize("version", [1, V2], ids=["v1", "v2"])
@pytest.mark.parametrize("cid_len", [0, 1, 7, 8, 19, 20])
def test_cid_lengths_match_oracle(lib, oracle, version, cid_len):
    rng = np.random.default_rng(1000 * cid_len + (version & 0xFF))
    cid = rng.bytes(cid_len)
    want = oracle.initial_secrets(cid, version)
    for server in (False, True):
        # whatever follows the cid in the record must not matter
        for fill in (0, 0xFF):
            secret, key, iv, hp = _derive(lib, cid, version, server, fill)
            assert secret == want[int(server)]
            assert (key, iv, hp) == oracle.derive_key_iv_hp(0, secret, version)


def test_salt_pad_states_equal_hmac_init(lib, oracle):
    """The pad states the host hands the kernel (word-based code) equal
    hmac_init (the byte-array code) on the salts."""
    got = np.zeros(32, np.uint32)
    lib.qpp_test_salt_pads(got.ctypes.data)
    for k, salt in enumerate((oracle.SALT_V1, oracle.SALT_V2)):
        ref = np.zeros(16, np.uint32)
        lib.qpp_test_hmac_init(salt, len(salt), ref.ctypes.data)
        assert np.array_equal(got[16 * k: 16 * k + 16], ref)
    assert not np.array_equal(got[:16], got[16:])
