"""CPU checks of the key-phase entry points at the drop-in boundary
(include/quic_pp.h: qpp_route_phase, qpp_session_route_phase_unprotect):
declared, exported, bound, and the cached next-phase context of
aioquic_amd.crypto dropped where it must be.  No device calls."""

import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "quic_pp.h")
LIB = os.path.join(ROOT, "aioquic_amd", "libquicpp.so")

ENTRY_POINTS = ["qpp_route_phase", "qpp_route_phase_launches", "qpp_session_route_phase_unprotect"]


def test_header_declares_and_library_exports_them():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in ENTRY_POINTS:
        assert re.search(r"^\w[\w\s\*]*\b%s\s*\(" % name, src, flags=re.M), name
    assert re.search(r"#define\s+QPP_ABI_VERSION\s+3\b", src), "the change only adds entry points"
    assert os.path.exists(LIB), "build() first: aioquic_amd/libquicpp.so missing"
    out = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(ENTRY_POINTS) <= exported


def test_module_has_the_phase_api():
    from aioquic_amd import _crypto, receive
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    for name in ("route_phase", "route_phase_launches", "route_phase_unprotect_host", "receive_routed_phase"):
        assert hasattr(_crypto, name), name
    assert hasattr(PacketEngine, "route_phase") and hasattr(PacketEngine, "route_phase_unprotect_host")
    p = inspect.signature(receive.receive_routed).parameters["next_phase"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    assert L.PHASE.itemsize == 1 and L.NEXT_SLOT.itemsize == 4 and (L.PHASE_CURRENT, L.PHASE_NEXT) == (0, 1)
    assert _crypto.abi_version() == 3
    assert receive.receive_routed(None, [], next_phase=True) == ([], [])


def test_cached_next_phase_is_built_once_and_dropped(monkeypatch):
    """cached_next_phase builds a context's next phase once; setup, teardown
    and apply_key_phase drop it and release its AEAD from the batch key
    tables, unless that AEAD is the one just adopted."""
    from aioquic_amd import crypto as C

    built, released = [], []

    class Key:
        pass

    def fake_next(ctx):
        nxt = C.CryptoContext(key_phase=1 - ctx.key_phase)
        nxt.aead, nxt.secret = Key(), b"next"
        built.append(nxt)
        return nxt

    monkeypatch.setattr(C, "next_key_phase", fake_next)
    monkeypatch.setattr(C, "_KEY_RELEASE_HOOKS", [lambda *objs: released.extend(objs)])
    ctx = C.CryptoContext()
    ctx.aead = first = Key()
    a = C.cached_next_phase(ctx)
    assert C.cached_next_phase(ctx) is a and len(built) == 1 and a.key_phase == 1
    # adopted: kept in the tables, the old key released, the cache empty
    C.apply_key_phase(ctx, a, "remote_update")
    assert (ctx.aead, ctx.key_phase, ctx.secret, ctx._next) == (a.aead, 1, b"next", None)
    assert released == [first]
    # a phase nobody adopted: another context wins, the cached key goes
    b = C.cached_next_phase(ctx)
    assert b is not a and b.key_phase == 0
    other = fake_next(ctx)
    C.apply_key_phase(ctx, other, "local_update")
    assert released == [first, b.aead, a.aead] and ctx._next is None
    # teardown drops it too
    c = C.cached_next_phase(ctx)
    held = ctx.aead
    ctx.teardown()
    assert ctx._next is None and released[3:] == [c.aead, held, None]
