"""CPU checks of the next-key-phase entry point at the drop-in boundary
(include/quic_pp.h: qpp_keytab_derive_next): declared, exported, bound, and the
record the Python side packs matches the header's.  No device calls."""

import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quic_pp.h")
LIB = os.path.join(ROOT, "aioquic_amd", "libquicpp.so")

FIELDS = ["slot", "suite", "key_phase", "flags", "secret_len", "secret", "hp"]


def test_header_declares_and_library_exports_it():
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^\w[\w\s\*]*\bqpp_keytab_derive_next\s*\(", src, flags=re.M)
    assert re.search(r"#define\s+QPP_ABI_VERSION\s+3\b", src), "the change only adds an entry point"
    # the comment says what it replaces and why qpp_keytab_derive does not do
    at = re.search(r"^int qpp_keytab_derive_next\(", text, flags=re.M).start()
    comment = text[text.rfind("\n/* ", 0, at):at]
    for cite in ("crypto.py:148-168", "quic ku", "QPP_SLOT_NONE", "QPP_E_ARG"):
        assert cite in comment, cite
    assert os.path.exists(LIB), "build() first: aioquic_amd/libquicpp.so missing"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert "qpp_keytab_derive_next" in exported


def test_record_layout_matches_header(tmp_path):
    """sizeof / offsetof of qpp_next_phase as gcc sees the header itself."""
    from aioquic_amd import layout as L

    src = tmp_path / "nx.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "quic_pp.h"\n'
                   'int main(void) { printf("%zu' + " %zu" * len(FIELDS) + ' %u %u\\n", sizeof(qpp_next_phase), '
                   + ", ".join("offsetof(qpp_next_phase, %s)" % f for f in FIELDS)
                   + ', QPP_SLOT_NONE, QPP_DERIVE_V2); return 0; }\n')
    exe = str(tmp_path / "nx")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)],
                   check=True)
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    f = L.NEXT_PHASE.fields
    assert got == [L.NEXT_PHASE.itemsize] + [f[name][1] for name in FIELDS] + [L.SLOT_NONE, L.DERIVE_V2]
    assert L.NEXT_PHASE.itemsize == 104 and list(L.NEXT_PHASE.names) == FIELDS
    assert f["secret"][0].shape == (64,) and f["hp"][0].shape == (32,)


def test_packing_helper():
    from aioquic_amd import layout as L

    rec = L.next_phase_record(9, L.AES_256_GCM, bytes(range(1, 49)), b"\x07" * 32, key_phase=1, v2=True)
    assert rec.dtype == L.NEXT_PHASE and len(rec) == 1
    r = rec[0]
    assert (r["slot"], r["suite"], r["key_phase"], r["flags"], r["secret_len"]) == (9, 1, 1, L.DERIVE_V2, 48)
    assert r["secret"].tobytes() == bytes(range(1, 49)) + bytes(16) and r["hp"].tobytes() == b"\x07" * 32
    short = L.next_phase_record(L.SLOT_NONE, L.AES_128_GCM, b"s", b"\x01" * 16, key_phase=0)[0]
    assert short["slot"] == L.SLOT_NONE and short["flags"] == 0 and short["hp"].tobytes() == b"\x01" * 16 + bytes(16)
    for bad in (b"", bytes(65)):
        with pytest.raises(ValueError):
            L.next_phase_record(0, 0, bad, bytes(16), key_phase=0)
    with pytest.raises(ValueError):
        L.next_phase_record(0, 0, b"s", bytes(33), key_phase=0)
    # the batched callers pack the same record by struct
    from aioquic_amd import batch_io

    assert batch_io._NEXT_REC.pack(9, 1, 1, L.DERIVE_V2, 48, bytes(range(1, 49)), b"\x07" * 32) == rec.tobytes()


def test_module_has_the_next_phase_api():
    from aioquic_amd import _crypto, batch_io, receive
    from aioquic_amd.batch import PacketEngine

    assert callable(_crypto.KeyTable.derive_next) and callable(_crypto.aead_deferred)
    assert callable(PacketEngine.derive_next_keys)
    assert callable(batch_io.setup_next_phase_batch) and callable(batch_io.update_keys_batch)
    p = inspect.signature(receive.receive_routed_keys).parameters
    assert list(p) == ["router", "datagrams", "next_phase", "device_keys"]
    assert p["device_keys"].kind is inspect.Parameter.KEYWORD_ONLY and p["device_keys"].default is False
    assert p["next_phase"].kind is inspect.Parameter.KEYWORD_ONLY and p["next_phase"].default is False
    # receive_routed keeps the parameter list it had
    assert list(inspect.signature(receive.receive_routed).parameters) == ["router", "datagrams", "next_phase"]
    assert _crypto.abi_version() == 3, "nothing that existed changed"
    assert receive.receive_routed_keys(None, [], next_phase=True, device_keys=True) == ([], [])
    assert receive.receive_routed(None, [], next_phase=True) == ([], [])
    # no device is touched by these: empty batches are no-ops
    batch_io.setup_next_phase_batch([], slots=object())
    batch_io.update_keys_batch([], "local_update", slots=object())


def test_releases_inside_a_block_reach_the_hooks_as_one_call(monkeypatch):
    """crypto._releases_together, which update_keys_batch commits under: what
    the contexts let go of inside the block is handed over once, at its end,
    and outside a block every release goes through at once, as before."""
    from aioquic_amd import crypto as C

    calls = []
    monkeypatch.setattr(C, "_KEY_RELEASE_HOOKS", [lambda *objs: calls.append(objs)])
    a, b, c = object(), object(), object()
    C._release(a)
    assert calls == [(a,)]
    with C._releases_together():
        C._release(b)
        with C._releases_together():
            C._release(c, a)
        assert calls == [(a,)]
    assert calls == [(a,), (b, c, a)]
    with C._releases_together():
        pass
    assert len(calls) == 2
    with pytest.raises(KeyError):
        with C._releases_together():
            C._release(b)
            raise KeyError("a callback failed")
    assert calls[2:] == [(b,)], "handed over although the block raised"
    C._release(c)
    assert calls[3:] == [(c,)]
