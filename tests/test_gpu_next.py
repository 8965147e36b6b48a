"""GPU checks of the batched next key phase (qpp_keytab_derive_next,
k_derive_next) through every layer: the C entry point against the C oracle and
the stdlib key schedule of oracle/oracle.py, the slots it installs under the
kept header-protection key, its refusals, the full circle with k_phase, the
deferred AEAD, and the batched callers (batch_io.setup_next_phase_batch,
batch_io.update_keys_batch, receive_routed_keys(..., device_keys=True)) against the
per-connection host path they replace, on twin state."""

from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests import receive_scenario as RS
from tests.test_gpu_phase import Peers, Receiver, _secrets
from tests.test_gpu_route import _record_tuple, _state

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CID = bytes(range(0x31, 0x39))
VERSIONS = (O.VERSION_1, O.VERSION_2)


@pytest.fixture(scope="module")
def dev():
    import torch

    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


@pytest.fixture(autouse=True)
def _watchdog():
    from aioquic_amd import _crypto

    yield
    assert _crypto.watchdog_count() == 0


def _klen(suite: int) -> int:
    return 16 if suite == O.AES_128_GCM else 32


def _hlen(suite: int) -> int:
    return 48 if suite == O.AES_256_GCM else 32


def _want_next(suite: int, version: int, secret: bytes, hp: bytes):
    """(secret', key, iv, hp) of the next phase by the oracle's key schedule."""
    nxt = O.next_secret(suite, secret)
    key, iv, _ = O.derive_key_iv_hp(suite, nxt, version)
    return nxt, key, iv, hp[:_klen(suite)]


def _packet64(suite, key, iv, hp, phase: int, pn: int, rng) -> bytes:
    """A 64-byte short-header packet sealed by the C oracle."""
    hdr = RS.short_header(CID, phase, pn, 2)
    return O.protect(suite, key, iv, hp, hdr, rng.bytes(64 - len(hdr) - 16), pn)


def _protect_on_slots(eng, keys: list, rng):
    """One 64-byte packet per slot, protected by the engine and by the oracle
    under keys[slot] = (suite, key, iv, hp, phase); then the oracle's packets
    opened by the engine.  Returns the statuses of the unprotect."""
    from aioquic_amd import layout as L
    from aioquic_amd.batch import layout_packets

    n = len(keys)
    hdrs = [RS.short_header(CID, k[4], 100 + s, 2) for s, k in enumerate(keys)]
    pays = [rng.bytes(64 - len(h) - 16) for h in hdrs]
    pns = [100 + s for s in range(n)]
    buf, desc, size = layout_packets(hdrs, pays, pns, list(range(n)))
    out, res = eng.protect_host(desc, buf.tobytes(), size)
    assert (res["status"] == L.S_OK).all()
    wires = []
    for s, (suite, key, iv, hp, _) in enumerate(keys):
        want = O.protect(suite, key, iv, hp, hdrs[s], pays[s], pns[s])
        o = int(desc["out_off"][s])
        assert out[o:o + 64].tobytes() == want, f"slot {s} protects to other bytes"
        wires.append(want)
    ud = np.zeros(n, L.DESC)
    ud["in_off"] = ud["out_off"] = np.arange(n) * 64
    ud["len"], ud["hdr_len"], ud["pn"], ud["slot"] = 64, 9, pns, np.arange(n)
    back, ures = eng.unprotect_host(ud, b"".join(wires), 64 * n)
    for s in range(n):
        if ures["status"][s] == L.S_OK:
            assert back[64 * s + 11:64 * s + 48].tobytes() == pays[s]
    return ures["status"]


# ------------------------------------------------- qpp_keytab_derive_next --

@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_lanes_at_the_workgroup_edges(dev, n):
    """n records, suites and versions interleaved, every third derive-only:
    km and secrets byte for byte, padding included; every installed slot
    protects under (next key and IV, the record's HP key, the next phase bit);
    the slots the derive-only records would have hit, and the neighbours past
    the batch, still protect to their old bytes."""
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    rng = np.random.default_rng(1000 + n)
    cap = n + 3
    eng = PacketEngine(cap)
    old = []
    for s in range(cap):
        suite = (s + 1 + s // 3) % 3
        old.append((suite, rng.bytes(_klen(suite)), rng.bytes(12), rng.bytes(_klen(suite)), (s // 2) & 1))
    eng.set_key_records(np.concatenate([L.key_material(s, k[0], k[1], k[2], k[3], k[4]) for s, k in enumerate(old)]))
    recs, want_km, want_sec, now = [], [], [], list(old)
    for i in range(n):
        suite, version = (i + i // 3) % 3, VERSIONS[(i // 2) % 2]
        none = i % 3 == 2
        secret = rng.bytes((_hlen(suite), 1, 64, 48, 32)[i % 5])
        hp, phase = rng.bytes(32), (i // 3) & 1  # 32 bytes whatever the suite: those past the key length are not copied
        slot = L.SLOT_NONE if none else i
        recs.append(L.next_phase_record(slot, suite, secret, hp, key_phase=phase, v2=version == O.VERSION_2))
        nxt, key, iv, hp_kept = _want_next(suite, version, secret, hp)
        want_km.append(L.key_material(slot, suite, key, iv, hp_kept, phase))
        want_sec.append(nxt.ljust(64, b"\x00"))
        if not none:
            now[i] = (suite, key, iv, hp_kept, phase)
    recs = np.concatenate(recs)
    assert {(int(r["suite"]), int(r["flags"])) for r in recs} == {(s, f) for s in range(3) for f in range(2)} or n == 1
    km, sec = eng.derive_next_keys(recs)
    assert km.tobytes() == np.concatenate(want_km).tobytes()
    assert sec.tobytes() == b"".join(want_sec)
    status = _protect_on_slots(eng, now, rng)
    assert (status == L.S_OK).all(), "a slot's key phase is not the one it was installed with"
    # and the raw binding returns the same bytes
    km2, sec2 = eng.table.derive_next(recs.tobytes())
    assert km2 == km.tobytes() and sec2 == sec.tobytes()


def test_empty_batch_and_outputs_left_out(dev):
    """n == 0 is QPP_OK; km_out and secrets_out may be NULL and the slots are
    installed all the same."""
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    eng = PacketEngine(4)
    assert eng.table.derive_next(b"") == (b"", b"")
    lib = ctypes.CDLL(os.path.join(ROOT, "aioquic_amd", "libquicpp.so"))
    lib.qpp_keytab_create.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_void_p)]
    lib.qpp_keytab_derive_next.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_void_p]
    lib.qpp_keytab_destroy.argtypes = [ctypes.c_void_p]
    lib.qpp_keytab_destroy.restype = None
    kt = ctypes.c_void_p()
    assert lib.qpp_keytab_create(4, ctypes.byref(kt)) == 0
    try:
        rec = L.next_phase_record(1, L.AES_128_GCM, b"k" * 32, b"h" * 16, key_phase=1)
        assert lib.qpp_keytab_derive_next(kt, None, 0, None, None, None) == 0
        assert lib.qpp_keytab_derive_next(kt, rec.ctypes.data, 1, None, None, None) == 0
        km = np.zeros(1, L.KEY_MATERIAL)
        assert lib.qpp_keytab_derive_next(kt, rec.ctypes.data, 1, km.ctypes.data, None, None) == 0
        _, key, iv, hp = _want_next(L.AES_128_GCM, O.VERSION_1, b"k" * 32, b"h" * 16)
        assert km.tobytes() == L.key_material(1, L.AES_128_GCM, key, iv, hp, 1).tobytes()
        # the pointer-level refusals
        assert lib.qpp_keytab_derive_next(None, rec.ctypes.data, 1, None, None, None) == -1
        assert lib.qpp_keytab_derive_next(kt, None, 1, None, None, None) == -1
        assert lib.qpp_keytab_derive_next(kt, rec.ctypes.data, (1 << 24) + 1, None, None, None) == -1
    finally:
        lib.qpp_keytab_destroy(kt)


def test_refusals_install_nothing(dev):
    """Each QPP_E_ARG case alone, in a batch whose other records are valid:
    ValueError, and a probe packet on every slot the batch named reports
    QPP_S_NO_KEY."""
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    cap = 6
    eng = PacketEngine(cap)
    rng = np.random.default_rng(5)

    def batch():
        return np.concatenate([L.next_phase_record(s, s % 3, rng.bytes(32), rng.bytes(32), key_phase=s & 1,
                                                   v2=bool(s & 2)) for s in range(4)])

    def probe():
        ud = np.zeros(cap, L.DESC)
        ud["in_off"] = ud["out_off"] = np.arange(cap) * 64
        ud["len"], ud["hdr_len"], ud["slot"] = 64, 9, np.arange(cap)
        _, res = eng.unprotect_host(ud, rng.bytes(64 * cap), 64 * cap)
        return res["status"].tolist()

    bad = [("slot", cap), ("slot", L.SLOT_NONE - 1), ("suite", 3), ("suite", 0xFF), ("secret_len", 0),
           ("secret_len", 65), ("key_phase", 2), ("flags", 2), ("flags", L.DERIVE_V2 | 0x80)]
    for at in (0, 2, 3):
        for field, value in bad:
            recs = batch()
            recs[field][at] = value
            with pytest.raises(ValueError):
                eng.table.derive_next(recs.tobytes())
            assert probe() == [L.S_NO_KEY] * cap, (field, value, at)
    with pytest.raises(ValueError):
        eng.table.derive_next(batch().tobytes()[:-1])
    # the table is as usable as before: the same batch, valid, installs its four slots
    eng.derive_next_keys(batch())
    assert [s == L.S_NO_KEY for s in probe()] == [False] * 4 + [True] * 2


def test_full_circle_with_k_phase(dev):
    """A current slot and the next slot derive_next installs for it, through
    qpp_route_phase and qpp_unprotect: a packet of the next phase sealed by the
    oracle (next key and IV, the current HP key) opens on the next slot, one
    of the current phase on the current slot."""
    import torch
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    rng = np.random.default_rng(77)
    conns = [(suite, version, phase) for suite in range(3) for version in VERSIONS for phase in (0, 1)]
    nc = len(conns)
    eng = PacketEngine(2 * nc + 1)
    cur, recs, nxt = [], [], []
    for c, (suite, version, phase) in enumerate(conns):
        secret = rng.bytes(_hlen(suite))
        key, iv, hp = O.derive_key_iv_hp(suite, secret, version)
        cur.append((suite, key, iv, hp, phase))
        recs.append(L.next_phase_record(nc + c, suite, secret, hp, key_phase=1 - phase, v2=version == O.VERSION_2))
        _, nkey, niv, _ = _want_next(suite, version, secret, hp)
        nxt.append((suite, nkey, niv, hp, 1 - phase))
    eng.set_key_records(np.concatenate([L.key_material(c, *k) for c, k in enumerate(cur)]))
    eng.derive_next_keys(np.concatenate(recs))
    packets, want_slot = [], []
    for c in range(nc):
        for flipped in (0, 1, 1, 0):
            k = nxt[c] if flipped else cur[c]
            packets.append(_packet64(k[0], k[1], k[2], k[3], k[4], 10 + len(packets), rng))
            want_slot.append(nc + c if flipped else c)
    n = len(packets)
    desc = np.zeros(n, L.DESC)
    desc["in_off"] = desc["out_off"] = np.arange(n) * 64
    desc["len"], desc["hdr_len"], desc["pn"] = 64, 9, 10 + np.arange(n)
    desc["slot"] = np.repeat(np.arange(nc), 4)
    next_per_desc = (np.repeat(np.arange(nc), 4) + nc).astype(np.uint32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_in, d_desc, d_next = t(np.frombuffer(b"".join(packets), np.uint8)), t(desc), t(next_per_desc)
    d_phase = torch.zeros(n, dtype=torch.uint8, device=dev)
    d_res = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n * 64, dtype=torch.uint8, device=dev)
    eng.route_phase(None, d_next, 0, d_desc, n, d_in, d_phase)
    eng.unprotect(d_desc, n, d_in, d_out, d_res)
    torch.cuda.synchronize()
    got = d_desc.cpu().numpy().view(L.DESC)
    res = d_res.cpu().numpy().view(L.RESULT)
    assert got["slot"].tolist() == want_slot
    assert d_phase.cpu().numpy().tolist() == [int(s >= nc) for s in want_slot]
    assert (res["status"] == L.S_OK).all() and res["pn"].tolist() == (10 + np.arange(n)).tolist()


# ------------------------------------------------------- the deferred AEAD --

def test_deferred_aead_equals_the_eager_one(dev):
    from aioquic_amd import _crypto

    rng = np.random.default_rng(3)
    for name, klen in ((b"aes-128-gcm", 16), (b"aes-256-gcm", 32), (b"chacha20-poly1305", 32)):
        key, iv = rng.bytes(klen), rng.bytes(12)
        eager, lazy = _crypto.AEAD(name, key, iv), _crypto.aead_deferred(name, key, iv)
        assert type(lazy) is _crypto.AEAD and lazy._material() == eager._material()
        for size in (1, 37, 1200):
            data, aad = rng.bytes(size), rng.bytes(1 + size % 30)
            sealed = eager.encrypt(data, aad, 7 + size)
            assert lazy.encrypt(data, aad, 7 + size) == sealed
            assert lazy.decrypt(sealed, aad, 7 + size) == eager.decrypt(sealed, aad, 7 + size) == data
            with pytest.raises(_crypto.CryptoError, match="Payload decryption failed"):
                lazy.decrypt(sealed, aad + b"x", 7 + size)
        # first use by decrypt, and a short IV zero padded as the constructor does
        eager, lazy = _crypto.AEAD(name, key, iv[:8]), _crypto.aead_deferred(name, key, iv[:8])
        sealed = eager.encrypt(b"payload", b"aad", 1)
        assert lazy.decrypt(sealed, b"aad", 1) == b"payload" and lazy._material() == eager._material()
    for args in ((b"aes-128-cbc", bytes(16), bytes(12)), (b"aes-128-gcm", bytes(33), bytes(12)),
                 (b"aes-128-gcm", bytes(16), bytes(13)), (b"aes-128-gcm", bytes(32), bytes(12)),
                 (b"aes-256-gcm", bytes(16), bytes(12)), (b"chacha20-poly1305", bytes(31), bytes(12)),
                 ("aes-128-gcm", bytes(16), bytes(12)), (b"aes-128-gcm", bytes(16))):
        with pytest.raises(Exception) as eager_err:
            _crypto.AEAD(*args)
        with pytest.raises(Exception) as lazy_err:
            _crypto.aead_deferred(*args)
        assert type(lazy_err.value) is type(eager_err.value) and str(lazy_err.value) == str(eager_err.value), args


# ------------------------------------------------------ the batched callers --

class _Counting:
    """A KeySlots' table with its calls counted."""

    def __init__(self, table):
        self.real, self.calls = table, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def counted(*a):
            self.calls.append(name)
            return fn(*a)

        return counted

    def count(self, name: str) -> int:
        return self.calls.count(name)


def _contexts(n: int, log: list, seed: int):
    """n keyed contexts, the three suites and both versions interleaved,
    whose callbacks append (index, trigger) to `log`."""
    from aioquic_amd import crypto as C
    from aioquic_amd.tls import CipherSuite

    cs = (CipherSuite.AES_128_GCM_SHA256, CipherSuite.AES_256_GCM_SHA384, CipherSuite.CHACHA20_POLY1305_SHA256)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ctx = C.CryptoContext(key_phase=(i // 6) & 1, setup_cb=lambda trig, i=i: log.append((i, trig)))
        ctx.setup(cipher_suite=cs[i % 3], secret=rng.bytes(_hlen(i % 3)), version=VERSIONS[(i // 3) % 2])
        out.append(ctx)
    return out


def _open_on_slots(slots, ctxs_keys: list, rng):
    """One oracle-sealed packet per (slot, suite, key, iv, hp, phase): statuses of the table's unprotect."""
    from aioquic_amd import _crypto
    from aioquic_amd import layout as L

    n = len(ctxs_keys)
    wires = [_packet64(su, key, iv, hp, ph, 50 + k, rng) for k, (_, su, key, iv, hp, ph) in enumerate(ctxs_keys)]
    ud = np.zeros(n, L.DESC)
    ud["in_off"] = ud["out_off"] = np.arange(n) * 64
    ud["len"], ud["hdr_len"], ud["pn"] = 64, 9, 50 + np.arange(n)
    ud["slot"] = [k[0] for k in ctxs_keys]
    table = slots.table.real if isinstance(slots.table, _Counting) else slots.table
    _, res = _crypto.unprotect_host(table, ud.tobytes(), b"".join(wires), 64 * n)
    return np.frombuffer(res, L.RESULT)["status"].tolist()


def test_setup_next_phase_batch_against_next_key_phase(dev):
    """70 twin contexts: the batched device call leaves each context's cached
    next phase as next_key_phase builds it, under the context's own HP object,
    in a slot that already holds it; nothing fires; a second call derives
    nothing; a table with no room raises and moves no state."""
    from aioquic_amd import crypto as C
    from aioquic_amd import layout as L
    from aioquic_amd.batch_io import KeySlots, setup_next_phase_batch

    log_a, log_b = [], []
    a, b = _contexts(70, log_a, 11), _contexts(70, log_b, 11)
    assert log_a == log_b == [(i, "tls") for i in range(70)]
    slots = KeySlots(128)
    slots.table = table = _Counting(slots.table)
    try:
        setup_next_phase_batch(a + [C.CryptoContext()] + a[:3], slots)  # a keyless one and repeats are passed over
        assert table.count("derive_next") == 1 and table.count("set") == 0
        rng = np.random.default_rng(12)
        probes = []
        for x, y in zip(a, b):
            want = C.next_key_phase(y)
            got = x._next
            assert got is not None and C.cached_next_phase(x) is got
            assert (got.secret, got.key_phase, got.cipher_suite, got.version) == \
                (want.secret, want.key_phase, want.cipher_suite, want.version)
            assert got.aead._material() == want.aead._material() and got.key_phase == 1 - x.key_phase
            assert got.hp is x.hp and x.hp._material() == y.hp._material()
            suite, key, iv = got.aead._material()
            probes.append((None, suite, key, iv, x.hp._material()[1], got.key_phase))
        assert log_a == log_b, "no callback fired"
        # the slots are bound: a later assign() finds them, installed, with nothing left to set
        got_slots = slots.assign([(x._next.aead, x.hp, x._next.key_phase) for x in a])
        assert table.count("set") == 0 and sorted(got_slots) == list(range(70))
        assert _open_on_slots(slots, [(s,) + p[1:] for s, p in zip(got_slots, probes)], rng) == [L.S_OK] * 70
        setup_next_phase_batch(a, slots)
        setup_next_phase_batch([], slots)
        assert table.count("derive_next") == 1, "a second call derives nothing"
        # adopting one is what apply_key_phase does with any next context; its slot stays
        C.apply_key_phase(a[0], a[0]._next, "remote_update")
        assert log_a[-1] == (0, "remote_update") and a[0]._next is None
        assert slots.assign([(a[0].aead, a[0].hp, a[0].key_phase)]) == [got_slots[0]] and table.count("set") == 0
    finally:
        slots.close()
    small = KeySlots(8)
    small.table = table = _Counting(small.table)
    try:
        fresh = _contexts(6, [], 13)
        small.assign([(c.aead, c.hp, c.key_phase) for c in fresh[:3]])
        calls = list(table.calls)
        with pytest.raises(OverflowError):
            setup_next_phase_batch(fresh, small)
        assert all(c._next is None for c in fresh) and table.calls == calls, "no state moved, nothing cleared"
        setup_next_phase_batch(fresh[:5], small)  # five fit beside the three
        assert table.count("derive_next") == 1 and table.count("clear") == 0
    finally:
        small.close()


def _pairs(n: int, log: list, seed: int):
    from aioquic_amd import crypto as C
    from aioquic_amd.tls import CipherSuite

    cs = (CipherSuite.AES_128_GCM_SHA256, CipherSuite.AES_256_GCM_SHA384, CipherSuite.CHACHA20_POLY1305_SHA256)
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        cb = lambda side, i=i: (lambda trig: log.append((i, side, trig)))
        pair = C.CryptoPair(recv_setup_cb=cb("recv"), send_setup_cb=cb("send"))
        for ctx in (pair.recv, pair.send):
            ctx.setup(cipher_suite=cs[i % 3], secret=rng.bytes(_hlen(i % 3)), version=VERSIONS[(i // 3) % 2])
        out.append(pair)
    return out


def _pair_state(pairs):
    return [(p._update_key_requested, p.key_phase) +
            tuple((c.secret, c.key_phase, c.aead._material(), c.hp._material(), c.cipher_suite, c.version, c._next)
                  for c in (p.recv, p.send)) for p in pairs]


def test_update_keys_batch_against_update_key(dev, monkeypatch):
    """Twin pairs through two consecutive updates (phase 0 -> 1 -> 0): the
    same context state and callback sequence as CryptoPair._update_key, the
    request flag cleared, one release() per call on the table, and the receive
    slots current without a KeyTable.set."""
    from aioquic_amd import crypto as C
    from aioquic_amd import layout as L
    from aioquic_amd.batch_io import KeySlots, setup_next_phase_batch, update_keys_batch

    log_a, log_b = [], []
    a, b = _pairs(12, log_a, 21), _pairs(12, log_b, 21)
    slots = KeySlots(64)
    slots.table = table = _Counting(slots.table)
    releases = []
    real_release = slots.release
    monkeypatch.setattr(slots, "release", lambda objs: (releases.append(list(objs)), real_release(objs))[1])
    rng = np.random.default_rng(22)
    try:
        slots.assign([(p.recv.aead, p.recv.hp, p.recv.key_phase) for p in a])
        for phase in (1, 0):
            # half of the receive directions have their next phase cached and installed already
            setup_next_phase_batch([p.recv for p in a[::2]], slots)
            for p in a[1::3] + b[1::3]:
                p.update_key()
            hp_objs = [(p.recv.hp, p.send.hp) for p in a]
            old = [p.recv.aead for p in a] + [p.send.aead for p in a]
            calls, n_rel = len(table.calls), len(releases)
            with monkeypatch.context() as mp:
                mp.setattr(C, "next_key_phase", lambda ctx: pytest.fail("next_key_phase on the batched path"))
                update_keys_batch(a, "remote_update", slots)
            assert table.calls[calls:] == ["derive_next", "clear"], "one derive, one clear launch, no set"
            assert len(releases) == n_rel + 1 and {id(o) for o in releases[-1]} == {id(o) for o in old}
            for p in b:
                p._update_key("remote_update")  # (its releases reach every live table, this one too)
            assert _pair_state(a) == _pair_state(b) and log_a == log_b
            assert all(p.recv.key_phase == p.send.key_phase == phase and not p._update_key_requested for p in a)
            assert [(p.recv.hp, p.send.hp) for p in a] == hp_objs, "a key update keeps the HP objects"
            # every receive direction is current in its slot as it stands
            triples = [(p.recv.aead, p.recv.hp, p.recv.key_phase) for p in a]
            at = slots.assign(triples)
            assert table.count("set") == 1, "only the first assign() of the test set keys"
            keys = [(s,) + p.recv.aead._material() + (p.recv.hp._material()[1], p.recv.key_phase) for s, p in zip(at, a)]
            assert _open_on_slots(slots, keys, rng) == [L.S_OK] * len(a)
        assert log_a[:24] == [(i, side, "tls") for i in range(12) for side in ("recv", "send")]
        assert log_a[24:48] == [(i, side, "remote_update") for i in range(12) for side in ("recv", "send")]
    finally:
        slots.close()


# ----------------------------------------------- receive_routed, device keys --

def _hook(conns, log: list) -> None:
    from aioquic_amd.tls import Epoch

    for k, conn in enumerate(conns):
        pair = conn.cryptos[Epoch.ONE_RTT]
        pair.recv._setup_cb = lambda trig, k=k: log.append((k, "recv", trig))
        pair.send._setup_cb = lambda trig, k=k: log.append((k, "send", trig))


def _no_host_schedule(mp) -> None:
    """next_key_phase raises wherever the product could reach it."""
    from aioquic_amd import batch_io, crypto

    def refuse(ctx):
        raise AssertionError("next_key_phase was called on the device-keys path")

    mp.setattr(crypto, "next_key_phase", refuse)
    mp.setattr(batch_io, "next_key_phase", refuse)


class Twins:
    """The same receivers twice: `dev` takes receive_routed_keys(next_phase=
    True, device_keys=True) with the host key schedule forbidden, `host` takes
    receive_routed(next_phase=True); `host` is also checked against
    receive_datagrams and the oracle walk (Receiver.reference / check)."""

    def __init__(self, specs):
        self.dev, self.host = Receiver(specs), Receiver(specs)
        self.log_dev, self.log_host = [], []
        _hook(self.dev.a, self.log_dev)
        _hook(self.host.a, self.log_host)

    def run(self, datagrams, monkeypatch, slots=None):
        from aioquic_amd import receive as R

        want = self.host.reference(datagrams)
        with monkeypatch.context() as mp:
            if slots is not None:
                mp.setattr(R, "default_slots", lambda: slots[1])
            got_h, un_h = R.receive_routed(self.host.router, datagrams, next_phase=True)
        self.host.check(got_h, un_h, want)
        with monkeypatch.context() as mp:
            if slots is not None:
                mp.setattr(R, "default_slots", lambda: slots[0])
            _no_host_schedule(mp)
            got_d, un_d = R.receive_routed_keys(self.dev.router, datagrams, next_phase=True, device_keys=True)
        assert un_d == un_h == []
        assert [_record_tuple(g) for g in got_d] == [_record_tuple(g) for g in got_h]
        assert _state(self.dev.a) == _state(self.host.a) and _secrets(self.dev.a) == _secrets(self.host.a)
        assert self.log_dev == self.log_host
        self.material_equal()
        return got_d

    def material_equal(self):
        from aioquic_amd.tls import Epoch

        for x, y in zip(self.dev.a, self.host.a):
            for side in ("recv", "send"):
                cx, cy = getattr(x.cryptos[Epoch.ONE_RTT], side), getattr(y.cryptos[Epoch.ONE_RTT], side)
                assert cx.aead._material() == cy.aead._material() and cx.hp._material() == cy.hp._material()
                assert (cx.key_phase, cx.secret) == (cy.key_phase, cy.secret)


def test_routed_update_in_mid_batch(dev, monkeypatch):
    from aioquic_amd import _crypto

    peers = Peers(0xD1)
    datagrams = peers.batch(30, {0: 11, 1: 20, 2: 7, 4: 29})
    tw = Twins(peers.specs)
    before = _crypto.route_phase_launches()
    got = tw.run(datagrams, monkeypatch)
    assert _crypto.route_phase_launches() == before + 2, "both twins resolved the updates on the device"
    assert all(r.ok for r in got) and len(got) == 150
    assert [k for _, _, _, _, k in _state(tw.dev.a)] == [1, 1, 1, 0, 1]
    assert sorted(tw.log_dev) == sorted((c, side, "remote_update") for c in (0, 1, 2, 4) for side in ("recv", "send"))


def test_routed_second_batch_flips_back(dev, monkeypatch):
    """Three batches on the same state: the next phase of an adopted context
    is derived from the adopted secret, and the polarity flips back."""
    from aioquic_amd.tls import Epoch

    peers = Peers(0xD2)
    tw = Twins(peers.specs)
    ctxs = [c.cryptos[Epoch.ONE_RTT].recv for c in tw.dev.a]
    for flip_at, phases in (({0: 3, 2: 9}, [1, 0, 1, 0, 0]), ({0: 5, 1: 0, 2: 11}, [0, 1, 0, 0, 0]),
                            ({3: 6}, [0, 1, 0, 1, 0])):
        held = [c._next for c in ctxs]
        got = tw.run(peers.batch(12, flip_at), monkeypatch)
        assert all(r.ok for r in got)
        assert [k for _, _, _, _, k in _state(tw.dev.a)] == phases
        for c, ctx in enumerate(ctxs):
            if c in flip_at:
                assert ctx._next is None and (held[c] is None or ctx.aead is held[c].aead)
            else:
                assert ctx._next is not None and ctx._next.key_phase == 1 - ctx.key_phase and ctx._next.hp is ctx.hp
                assert held[c] is None or ctx._next is held[c], "derived once per phase"


def test_routed_tampered_first_flipped_packet(dev, monkeypatch):
    peers = Peers(0xD3)
    streams = []
    for c in range(5):
        st = [peers.packet(c) for _ in range(3)]
        if c != 3:
            peers.flip(c)
            st.append(peers.packet(c, tamper=True))
            if c == 4:
                st.append(peers.packet(c, tamper=True))
            else:
                st += [peers.packet(c) for _ in range(3)]
        streams.append(st)
    tw = Twins(peers.specs)
    got = tw.run(peers.interleave(streams), monkeypatch)
    assert [r.dropped for r in got].count("payload_decrypt_error") == 5
    assert [k for _, _, _, _, k in _state(tw.dev.a)] == [1, 1, 1, 0, 0]


def test_routed_flipped_packet_with_a_reserved_bit(dev, monkeypatch):
    peers = Peers(0xD4)
    streams = []
    for c in range(5):
        st = [peers.packet(c) for _ in range(4)]
        if c in (1, 2):
            peers.flip(c)
            st.append(peers.packet(c, reserved=0x10 if c == 1 else 0x08))
        st += [peers.packet(c) for _ in range(3)]
        streams.append(st)
    tw = Twins(peers.specs)
    got = tw.run(peers.interleave(streams), monkeypatch)
    assert [r.dropped for r in got].count("reserved_bits") == 2
    assert [(closed, k) for closed, _, _, _, k in _state(tw.dev.a)] == [(False, 0), (True, 1), (True, 1), (False, 0),
                                                                       (False, 0)]


def test_routed_old_phase_packet_after_the_update(dev, monkeypatch):
    """A packet of the old phase behind the update is deferred: the walk
    tries it on the phase after next, from the device too, and it fails as on
    the host path."""
    peers = Peers(0xD6)
    streams = []
    for c in range(5):
        st = [peers.packet(c) for _ in range(3)]
        if c in (0, 1, 2):
            late = peers.packet(c)
            peers.flip(c)
            st += [peers.packet(c), peers.packet(c), late, peers.packet(c)]
        streams.append(st)
    datagrams = [d for st in streams for d in st]
    tw = Twins(peers.specs)
    got = tw.run(datagrams, monkeypatch)
    assert [r.dropped for r in got].count("payload_decrypt_error") == 3
    assert [k for _, _, _, _, k in _state(tw.dev.a)] == [1, 1, 1, 0, 0]


def test_routed_key_table_too_small_for_the_next_slots(dev, monkeypatch):
    """The table holds the batch's five keys and has no room for five next
    slots: the run continues without them, the flips go through ReceiveBatch,
    and that still derives on the device."""
    from aioquic_amd import _crypto
    from aioquic_amd.batch_io import KeySlots

    peers = Peers(0xD5)
    datagrams = peers.batch(10, {0: 4, 3: 6})
    tw = Twins(peers.specs)
    small = (KeySlots(7), KeySlots(7))
    before = _crypto.route_phase_launches()
    try:
        got = tw.run(datagrams, monkeypatch, slots=small)
        assert _crypto.route_phase_launches() == before, "no next slots on either twin"
        assert all(r.ok for r in got)
        assert [k for _, _, _, _, k in _state(tw.dev.a)] == [1, 0, 0, 1, 0]
    finally:
        small[0].close()
        small[1].close()
