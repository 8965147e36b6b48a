"""The key table's life cycle through every packet-kernel form launch_packets
can choose: one qpp_keytab of capacity 8 goes through a fixed script of table
operations, and after EVERY operation the same two batches are protected and
unprotected and compared byte for byte and result record for result record
with the C oracle (oracle.protect_batch / oracle.unprotect_batch).  No
tolerance anywhere.  The oracle is given the test's own mirror of the table:
8 KEY_MATERIAL records, suite 0xff for an empty slot (the oracle answers
QPP_S_NO_KEY for those, and for slots past the mirror).

The script (script(); TABLE holds the mirror each step must leave, as
slot: (suite, key phase); A, A', B ... are unrelated random key materials):
   1  nothing                       empty table: every packet QPP_S_NO_KEY,
                                    nothing written, yet every record written
   2  set 0 = AES-128 A
   3  set 0 = AES-128 A'            new key, iv and hp, same key phase.  Also
                                    unprotects the wire image the oracle made
                                    under A: every packet of slot 0 reports
                                    QPP_S_DECRYPT and leaves a zero payload
   4  set 0 = A', key phase 1       short headers with the other phase bit
                                    report QPP_S_KEY_PHASE
   5  set 1 = AES-128 B             two keys of the suite
   6  clear 1
   7  clear 1, 1, 1, 7, 8, 0xffffffff   one call; nothing may change (slot 0
                                    still encrypts: a double decrement of the
                                    host mirror would drop the AES-128 launch)
   8  set 1 = ChaCha20 C (phase 1), 2 = AES-256 D   one call; slot 1 held AES
   9  set 0 = AES-256 E             AES-128 has no key: its launch vanishes;
                                    AES-256 has two
  10  derive 2 = AES-256 / SHA-384 from a 48-byte secret, updates = 1, key
      phase 1                       replaces an installed key; km_out is
                                    checked against oracle.next_secret /
                                    derive_key_iv_hp (it IS the mirror's record)
  11  derive_initial (3, 4) from one CID and (5, QPP_SLOT_NONE) from another
      (v2)                          km_out and the secrets against the oracle
  12  clear 0..7                    everything QPP_S_NO_KEY again
  13  set 4 = ChaCha20 F            one key in a cleared table, on a slot that
                                    held AES-128
A' is the first of a fixed sequence of candidate materials whose
header-protection key leaves the key-phase bit of every slot-0 short header
of A's wire image where the slot's phase expects it, so that step 3's stale
packets fail authentication (QPP_S_DECRYPT), not the phase check; the CPU
tests assert the oracle says so.

The batches (batch(80), batch(48); the same construction): consecutive
descriptors name slots 0..5, 7 (never installed), 8 (= capacity) and
0xffffffff, one shuffled permutation of the nine per nine descriptors (fixed
seed), so every 16-descriptor item mixes at least three table slots and an
empty one.  Payloads of 1..200 bytes (1, 2, 3 and 200 among them) and a few
of 1200; two of three headers short (connection ids of 0, 5, 8 or 20 bytes,
spin bit i & 1, key-phase bit 1 in every fifth), the third an Initial long
header with a token of 0, 7 or 31 bytes; packet-number lengths 1..4.  Packet
i lies in its own 1600-byte cell of the input buffer and of a separate output
buffer at offsets with independent residues mod 16; both buffers hold 0xA5
wherever no packet lies.  80 packets send ChaCha20 through k_chacha, 48
through k_lone_chacha (at most 64 packets).

Every launch is compared as a whole: result records (pre-filled with 0xEE,
so a record nobody wrote shows), and the whole output buffer: 0xA5 outside
the QPP_S_OK packets' extents, a packet that failed authentication leaves
zeros in its payload region (its header bytes are not compared), and a
QPP_S_NO_KEY or QPP_S_KEY_PHASE packet writes nothing.  Unprotect reads the
oracle's wire image of the same step.  Protect launches run on one
non-default stream and unprotect launches on another, alternating; the table
calls keep their own (the null stream); every launch is synchronised before
it is compared.

Forms (all over the same script and batches), and what identifies them
(launch_packets, qpp_engine.hip):
  lone      in process, unplanned: k_lone_gcm, k_lone_chacha at 48 packets
            and k_chacha at 80                        [launch rule: lone_max]
  planned   in process, plan=eng.bucket(...) rebuilt for every launch (a plan
            holds only for unchanged slots; a stale plan is a documented
            precondition and not tested): k_gcm / k_chacha over the buckets
  quad      child process, QPP_LONE=0: k_gcm in the 512-thread shape while a
            suite has one key, the four-entry 1024-thread form once it has two
  quad_lds  child process, QPP_LONE=0 QPP_GCM_BPL=1: the close-from-LDS form
            with the launch pool while a suite has one key, else four entries
The counter qpp_close_lds_launches() identifies the last: its delta over each
unplanned launch must equal the number of AES suites with exactly one
installed slot in the test's mirror (close_lds_expected, launch_packets' rule
restated), which is where a wrong host mirror shows (steps 3, 4, 6, 7, 9 and
13); in every other form the delta is 0.  At the end of every process
qpp_watchdog_count() == 0 and qpp_pool_fallbacks() is unchanged.

After steps 3, 8 and 13, qpp_session_hp_mask for 17 samples (one more than a
16-lane group) over the installed slots against oracle.hp_mask.

Negative control (expectation side only): step 3's protect output is also
compared with the oracle's output under the stale key A (step 2's
expectation), and that comparison must fail.
"""

import ctypes
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from tests.golden_cases import gen_bytes, long_header, short_header

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AES128, AES256, CHACHA = 0, 1, 2
KEY_LEN = {AES128: 16, AES256: 32, CHACHA: 32}
S_OK, S_DECRYPT, S_KEY_PHASE, S_NO_KEY = 0, 2, 3, 4  # QPP_S_*
TAG = 16
CAP = 8
NONE = 0xFFFFFFFF            # QPP_SLOT_NONE; as a descriptor's slot: past every table
EMPTY = 0xFF                 # the mirror's suite of an empty slot
SLOT_VALUES = (0, 1, 2, 3, 4, 5, 7, CAP, NONE)
SIZES = (80, 48)             # k_chacha / k_lone_chacha (lone_max = 64)
LONE_MAX_CHACHA = 64
FILL, UNWRITTEN = 0xA5, 0xEE
CELL, LEAD, PAD = 1600, 64, 24  # packet i starts at LEAD + CELL * i + PAD + residue
CIDS = (0, 5, 8, 20)
TOKENS = (0, 7, 31)
BIG = (7, 26, 45, 64)        # positions of the 1200-byte payloads
FORMS = ("lone", "planned", "quad", "quad_lds")
SEED = {80: 0x11FEC0, 48: 0x11FEC4}  # the first from 0x11FEC0 up with which _geometry() holds

# the mirror every step must leave: slot -> (suite, key phase)
TABLE = (
    {},
    {0: (AES128, 0)},
    {0: (AES128, 0)},
    {0: (AES128, 1)},
    {0: (AES128, 1), 1: (AES128, 0)},
    {0: (AES128, 1)},
    {0: (AES128, 1)},
    {0: (AES128, 1), 1: (CHACHA, 1), 2: (AES256, 0)},
    {0: (AES256, 0), 1: (CHACHA, 1), 2: (AES256, 0)},
    {0: (AES256, 0), 1: (CHACHA, 1), 2: (AES256, 1)},
    {0: (AES256, 0), 1: (CHACHA, 1), 2: (AES256, 1), 3: (AES128, 0), 4: (AES128, 0), 5: (AES128, 0)},
    {},
    {4: (CHACHA, 0)},
)
STALE = 2            # index of step 3: the step that also unprotects step 2's wire image
HP_AFTER = (2, 7, 12)  # indices of steps 3, 8 and 13
# close-from-LDS launches per unplanned launch of the quad_lds form, step by step (the docstring's rule)
CLOSE_LDS = (0, 1, 1, 1, 0, 1, 1, 2, 0, 0, 0, 0, 0)


# ------------------------------------------------------------- the batches ----


@functools.lru_cache(maxsize=None)
def batch(n):
    """The batch of n packets, without any key: per-packet arrays, the protect
    and unprotect descriptors and the protect input buffer."""
    from oracle.oracle import DESC_DTYPE

    rng = np.random.default_rng(SEED[n])
    perms = np.concatenate([rng.permutation(9) for _ in range((n + 8) // 9)])[:n]
    slot = np.array([SLOT_VALUES[k] for k in perms], np.uint32)
    plen = rng.integers(1, 201, n)
    plen[3], plen[17], plen[41], plen[30] = 1, 2, 3, 200
    for i in BIG:
        if i < n:
            plen[i] = 1200
    pk = []
    for i in range(n):
        pl = int(plen[i])
        pn_len = max(1 + i % 4, 4 - pl)  # the header-protection sample needs payload + packet number >= 4
        pn = int(rng.integers(0, 1 << 30))
        if i % 3 == 2:
            hdr = long_header(1, rng.bytes(8), b"", rng.bytes(TOKENS[(i // 3) % 3]), pn, pn_len, pl + TAG)
        else:
            hdr = short_header(rng.bytes(CIDS[(i // 3) % 4]), pn, pn_len, int(i % 5 == 1), spin=i & 1)
        pk.append((hdr, rng.bytes(pl), pn_len, pn))
    i = np.arange(n, dtype=np.int64)
    in_off = LEAD + CELL * i + PAD + (5 * i + 3) % 16
    out_off = LEAD + CELL * i + PAD + (7 * (i // 16) + 11 * i + 1) % 16
    hlen = np.array([len(p[0]) for p in pk], np.int64)
    pn_len = np.array([p[2] for p in pk], np.int64)
    pn = np.array([p[3] for p in pk], np.uint64)
    short = np.array([not p[0][0] & 0x80 for p in pk])
    phase = np.array([(p[0][0] >> 2) & 1 if not p[0][0] & 0x80 else 0 for p in pk], np.int64)
    size = LEAD + CELL * n
    inbuf = np.full(size, FILL, np.uint8)
    for j, p in enumerate(pk):
        o = int(in_off[j])
        inbuf[o : o + len(p[0]) + len(p[1])] = np.frombuffer(p[0] + p[1], np.uint8)
    desc = np.zeros(n, DESC_DTYPE)
    desc["in_off"], desc["out_off"], desc["slot"] = in_off, out_off, slot
    desc["len"], desc["hdr_len"], desc["pn"] = plen, hlen, pn
    ud = desc.copy()
    ud["len"] = hlen + plen + TAG
    ud["hdr_len"] = hlen - pn_len
    ud["pn"] = pn + (i % 7).astype(np.uint64)
    for a in (inbuf, desc, ud):
        a.flags.writeable = False
    return dict(n=n, size=size, in_off=in_off, out_off=out_off, hlen=hlen, plen=plen.astype(np.int64), pn_len=pn_len,
                pn=pn, slot=slot, short=short, phase=phase, inbuf=inbuf, desc=desc, ud=ud)


# -------------------------------------------------------------- the script ----


def _material(tag, slot, suite, phase=0):
    from oracle.oracle import KEY_DTYPE

    kl = KEY_LEN[suite]
    rec = np.zeros(1, KEY_DTYPE)
    rec["slot"], rec["suite"], rec["key_phase"] = slot, suite, phase
    rec["iv"][0] = np.frombuffer(gen_bytes("lifecycle-%s-iv" % tag, 12), np.uint8)
    rec["key"][0, :kl] = np.frombuffer(gen_bytes("lifecycle-%s-key" % tag, kl), np.uint8)
    rec["hp"][0, :kl] = np.frombuffer(gen_bytes("lifecycle-%s-hp" % tag, kl), np.uint8)
    return rec


def _empty_mirror():
    from oracle.oracle import KEY_DTYPE

    m = np.zeros(CAP, KEY_DTYPE)
    m["slot"] = np.arange(CAP)
    m["suite"] = EMPTY
    return m


def _installed(mirror, recs):
    m = mirror.copy()
    for r in recs:
        if int(r["slot"]) != NONE:
            m[int(r["slot"])] = r
    return m


def _cleared(mirror, slots):
    m = mirror.copy()
    for s in slots:
        if int(s) < CAP:
            m[int(s)] = _empty_mirror()[int(s)]
    return m


def _a_prime(mirror_a):
    """A' (module docstring): the first candidate whose header-protection key
    unmasks key-phase bit 0, the slot's, in every short header of slot 0 in
    the wire image made under A."""
    from oracle import oracle as orc

    probes = []
    for n in SIZES:
        b = batch(n)
        w = oracle_step(mirror_a, b)["wire_in"]
        for j in np.nonzero((b["slot"] == 0) & b["short"])[0]:
            o, pn_off = int(b["in_off"][j]), int(b["hlen"][j] - b["pn_len"][j])
            probes.append((int(w[o]), w[o + pn_off + 4 : o + pn_off + 20].tobytes()))
    assert len(probes) >= 6
    for k in range(1 << 16):
        rec = _material("A'-%d" % k, 0, AES128)
        hp = rec["hp"][0, :16].tobytes()
        if all(((b0 ^ (orc.hp_mask(AES128, hp, smp)[0] & 0x1F)) >> 2) & 1 == 0 for b0, smp in probes):
            return rec
    raise AssertionError("no candidate for A'")


@functools.lru_cache(maxsize=None)
def script():
    """The thirteen steps: dicts of name, op ('none', 'set', 'clear', 'derive',
    'derive_initial'), arg (the records / slots of the call), km (what a
    derive call must return) and mirror (the table the step leaves)."""
    from aioquic_amd import layout as L
    from oracle import oracle as orc

    steps = []
    mirror = _empty_mirror()

    def step(name, op, arg=None, km=None):
        nonlocal mirror
        if op in ("set", "derive", "derive_initial"):
            mirror = _installed(mirror, arg if op == "set" else km)
        elif op == "clear":
            mirror = _cleared(mirror, arg)
        m = mirror.copy()
        m.flags.writeable = False
        steps.append(dict(name=name, op=op, arg=arg, km=km, mirror=m))

    step("1 empty table", "none")
    step("2 set 0 = AES-128 A", "set", _material("A", 0, AES128))
    a_prime = _a_prime(mirror)
    step("3 set 0 = AES-128 A'", "set", a_prime)
    flipped = a_prime.copy()
    flipped["key_phase"] = 1
    step("4 set 0 = A', key phase 1", "set", flipped)
    step("5 set 1 = AES-128 B", "set", _material("B", 1, AES128))
    step("6 clear 1", "clear", np.array([1], np.uint32))
    step("7 clear 1, 1, 1, 7, 8, none", "clear", np.array([1, 1, 1, 7, CAP, NONE], np.uint32))
    step("8 set 1 = ChaCha20 C, 2 = AES-256 D", "set",
         np.concatenate([_material("C", 1, CHACHA, 1), _material("D", 2, AES256)]))
    step("9 set 0 = AES-256 E", "set", _material("E", 0, AES256))
    secret = gen_bytes("lifecycle-secret", 48)
    key, iv, hp = orc.derive_key_iv_hp(AES256, orc.next_secret(AES256, secret))
    step("10 derive 2 = AES-256, updates 1", "derive", L.secret_record(2, AES256, secret, key_phase=1, updates=1),
         L.key_material(2, AES256, key, iv, hp, 1))
    cids = (gen_bytes("lifecycle-cid-a", 8), gen_bytes("lifecycle-cid-b", 20))
    recs = np.concatenate([L.initial_record(3, 4, cids[0]), L.initial_record(5, NONE, cids[1], v2=True)])
    km = []
    for cid, version, slots in ((cids[0], orc.VERSION_1, (3, 4)), (cids[1], orc.VERSION_2, (5, NONE))):
        for s, sec in zip(slots, orc.initial_secrets(cid, version)):
            km.append(L.key_material(s, AES128, *orc.derive_key_iv_hp(AES128, sec, version)))
    step("11 derive_initial (3, 4), (5, none)", "derive_initial", recs, np.concatenate(km))
    step("12 clear 0..7", "clear", np.arange(CAP, dtype=np.uint32))
    step("13 set 4 = ChaCha20 F", "set", _material("F", 4, CHACHA))
    return tuple(steps)


def table_of(mirror):
    """The mirror as TABLE states it."""
    return {int(r["slot"]): (int(r["suite"]), int(r["key_phase"])) for r in mirror if r["suite"] != EMPTY}


def close_lds_expected(mirror, form):
    """launch_packets' rule restated: an unplanned k_gcm launch of the
    one-block-per-lane build (QPP_GCM_BPL=1) closes from LDS for every AES
    suite with exactly one installed slot; no other form here does."""
    if form != "quad_lds":
        return 0
    return sum(1 for s in (AES128, AES256) if int((mirror["suite"] == s).sum()) == 1)


# ----------------------------------------------------- the oracle's passes ----


def _expect_unprotect(b, plain_o, ures):
    """The expected output buffer of an unprotect launch and the mask of the
    bytes compared (a failed packet's header bytes are not)."""
    exp = np.full(b["size"], FILL, np.uint8)
    mask = np.ones(b["size"], np.uint8)
    for j in range(b["n"]):
        o, st = int(b["out_off"][j]), int(ures[j]["status"])
        if st == S_OK:
            ln = int(ures[j]["out_len"])
            exp[o : o + ln] = plain_o[o : o + ln]
        elif st == S_DECRYPT:
            hl = int(ures[j]["hdr_len"])
            cl = int(b["ud"][j]["len"]) - hl - TAG
            assert int(b["ud"][j]["hdr_len"]) < hl <= int(b["ud"][j]["hdr_len"]) + 4 and cl >= 0
            mask[o : o + hl] = 0
            exp[o : o + hl] = 0
            exp[o + hl : o + hl + cl] = 0  # no unauthenticated plaintext is left
        else:
            assert st in (S_NO_KEY, S_KEY_PHASE) and ures[j]["out_len"] == 0  # nothing written
    return exp, mask


def oracle_step(mirror, b):
    """The oracle's protect and unprotect of the batch under `mirror`: the
    expected output buffers (0xA5 wherever nothing is written), the result
    records, and the unprotect input (the wire image at the input offsets)."""
    from oracle import oracle as orc

    mirror = np.ascontiguousarray(mirror)
    wire_o, res = orc.protect_batch(mirror, b["desc"], b["inbuf"], b["size"])
    exp_wire = np.full(b["size"], FILL, np.uint8)
    wire_in = np.full(b["size"], FILL, np.uint8)
    for j in range(b["n"]):
        o, i, ln = int(b["out_off"][j]), int(b["in_off"][j]), int(res[j]["out_len"])
        assert res[j]["status"] in (S_OK, S_NO_KEY) and (ln > 0) == (res[j]["status"] == S_OK)
        exp_wire[o : o + ln] = wire_o[o : o + ln]
        wire_in[i : i + ln] = wire_o[o : o + ln]
    plain_o, ures = orc.unprotect_batch(mirror, b["ud"], wire_in, b["size"])
    exp_plain, umask = _expect_unprotect(b, plain_o, ures)
    return dict(exp_wire=exp_wire, res=res, wire_in=wire_in, exp_plain=exp_plain, ures=ures, umask=umask)


@functools.lru_cache(maxsize=None)
def expectations():
    """Every step's oracle passes over both batches, 's<step index>_n<batch>_<name>',
    and step 3's unprotect of step 2's wire image, 'stale_n<batch>_...'.
    Computed once per process; read-only."""
    from oracle import oracle as orc

    t0 = time.perf_counter()
    out = {}
    steps = script()
    for si, st in enumerate(steps):
        for n in SIZES:
            for k, v in oracle_step(st["mirror"], batch(n)).items():
                out["s%d_n%d_%s" % (si, n, k)] = v
    for n in SIZES:
        b = batch(n)
        wire_in = out["s%d_n%d_wire_in" % (STALE - 1, n)]
        plain_o, ures = orc.unprotect_batch(np.ascontiguousarray(steps[STALE]["mirror"]), b["ud"], wire_in, b["size"])
        exp, mask = _expect_unprotect(b, plain_o, ures)
        out.update({"stale_n%d_exp_plain" % n: exp, "stale_n%d_ures" % n: ures, "stale_n%d_umask" % n: mask})
    for v in out.values():
        v.flags.writeable = False
    out["seconds"] = np.array(time.perf_counter() - t0)
    return out


# ------------------------------------------------------------ CPU tests ----


def _geometry(n):
    """What the module docstring says of a batch."""
    b = batch(n)
    slot, plen, hlen, pn_len = b["slot"], b["plen"], b["hlen"], b["pn_len"]
    assert (n <= LONE_MAX_CHACHA) == (n == 48)
    assert set(slot.tolist()) == set(SLOT_VALUES)
    for at in range(0, n, 16):
        item = set(slot[at : at + 16].tolist())
        assert len(item & set(range(6))) >= 3 and item & {7, CAP, NONE}, (n, at)
        # ... and, at the fullest table (step 11), several suites and an empty slot
        suites = {TABLE[10][s][0] for s in item if s in TABLE[10]}
        assert len(suites) == 3, (n, at)
    assert plen.min() == 1 and {1, 2, 3, 200} <= set(plen.tolist()) and (plen == 1200).sum() >= 3
    assert ((plen <= 200) | (plen == 1200)).all() and (plen + pn_len >= 4).all()
    assert set(pn_len.tolist()) == {1, 2, 3, 4}
    assert b["short"].sum() >= n // 2 and (~b["short"]).sum() >= n // 4
    assert set(pn_len[b["short"]].tolist()) == set(pn_len[~b["short"]].tolist()) == {1, 2, 3, 4}
    assert (b["phase"][b["short"]] == 1).sum() >= 5 and (b["phase"][b["short"]] == 0).sum() >= 20
    # every slot meets both header forms, and slot 0 both phase bits
    for s in SLOT_VALUES:
        assert b["short"][slot == s].any() and (~b["short"][slot == s]).any(), (n, s)
    assert set(b["phase"][(slot == 0) & b["short"]].tolist()) == {0, 1}
    # own cells, guards of at least 24 bytes, either direction's extents; independent residues
    ext = hlen + plen + TAG
    for off in (b["in_off"], b["out_off"]):
        cell = LEAD + CELL * np.arange(n)
        assert (off >= cell + PAD).all() and (off + ext + PAD <= cell + CELL).all()
    assert len(set((b["in_off"] % 16).tolist())) == 16 and len(set((b["out_off"] % 16).tolist())) == 16
    assert ((b["in_off"] % 16) != (b["out_off"] % 16)).any()
    filled = np.ones(b["size"], bool)
    for o, h, p in zip(b["in_off"], hlen, plen):
        filled[o : o + h + p] = False
    assert (b["inbuf"][filled] == FILL).all()


def test_scenario_covers_what_it_claims(oracle):
    """(CPU) The batches, the script and the oracle's results are what the
    module docstring says they are."""
    steps = script()
    assert len(steps) == len(TABLE) == len(CLOSE_LDS) == 13
    for st, want in zip(steps, TABLE):
        assert table_of(st["mirror"]) == want, st["name"]
        assert (st["mirror"]["slot"] == np.arange(CAP)).all()
    for si, st in enumerate(steps):
        assert close_lds_expected(st["mirror"], "quad_lds") == CLOSE_LDS[si], st["name"]
        assert close_lds_expected(st["mirror"], "quad") == 0
    # the table operations: a re-key, a phase flip, a suite change, both derives, every clear case
    a, a1, a2 = steps[1]["arg"][0], steps[2]["arg"][0], steps[3]["arg"][0]
    for f in ("key", "iv", "hp"):
        assert not np.array_equal(a[f], a1[f]) and np.array_equal(a1[f], a2[f])
    assert (a["key_phase"], a1["key_phase"], a2["key_phase"]) == (0, 0, 1)
    assert steps[6]["arg"].tolist() == [1, 1, 1, 7, CAP, NONE] and table_of(steps[5]["mirror"]) == TABLE[6]
    assert steps[4]["mirror"][1]["suite"] == AES128 and steps[7]["mirror"][1]["suite"] == CHACHA
    assert steps[9]["arg"]["updates"][0] == 1 and steps[9]["arg"]["suite"][0] == AES256
    assert steps[9]["mirror"][2].tobytes() != steps[8]["mirror"][2].tobytes()
    assert steps[10]["arg"]["slot_server"].tolist() == [4, NONE] and steps[10]["km"]["slot"].tolist() == [3, 4, 5, NONE]
    assert steps[10]["mirror"][4]["suite"] == AES128 and steps[12]["mirror"][4]["suite"] == CHACHA
    assert steps[11]["arg"].tolist() == list(range(CAP))
    # each suite is seen with no key, one key and (AES) several keys
    counts = {s: {sum(1 for v in t.values() if v[0] == s) for t in TABLE} for s in (AES128, AES256, CHACHA)}
    assert counts[AES128] >= {0, 1, 2, 3} and counts[AES256] >= {0, 1, 2} and counts[CHACHA] >= {0, 1}

    for n in SIZES:
        _geometry(n)

    e = expectations()
    seen = set()
    for si in range(13):
        for n in SIZES:
            for k in ("res", "ures"):
                seen |= set(e["s%d_n%d_%s" % (si, n, k)]["status"].tolist())
    for n in SIZES:
        b = batch(n)
        ures = e["stale_n%d_ures" % n]
        seen |= set(ures["status"].tolist())
        on0 = b["slot"] == 0
        # step 3's stale packets: every one of slot 0 fails authentication and leaves zeros
        assert on0.sum() >= 5 and (ures["status"][on0] == S_DECRYPT).all() and (ures["status"][~on0] == S_NO_KEY).all()
        exp = e["stale_n%d_exp_plain" % n]
        for j in np.nonzero(on0)[0]:
            o = int(b["out_off"][j])
            assert (exp[o : o + int(b["hlen"][j] + b["plen"][j])] == 0).all()
        # the key phase check bites where it should: step 4, slot 0's short headers of phase bit 0
        u4 = e["s3_n%d_ures" % n]
        assert ((u4["status"] == S_KEY_PHASE) == (on0 & b["short"] & (b["phase"] == 0))).all()
        # the empty table and the cleared one: all QPP_S_NO_KEY, nothing written
        for si in (0, 11):
            for k in ("res", "ures"):
                assert (e["s%d_n%d_%s" % (si, n, k)]["status"] == S_NO_KEY).all()
            for k in ("exp_wire", "exp_plain"):
                assert (e["s%d_n%d_%s" % (si, n, k)] == FILL).all()
    assert seen == {S_OK, S_DECRYPT, S_KEY_PHASE, S_NO_KEY}
    # the negative control can tell A from A': the two expectations differ
    assert not np.array_equal(e["s1_n80_exp_wire"], e["s2_n80_exp_wire"])
    print("oracle passes of the life cycle: %.3f s" % float(e["seconds"]))


def test_oracle_accepts_every_step(oracle):
    """(CPU) In every step the oracle protects every packet on an installed
    slot (QPP_S_OK) and unprotect gives the plaintext back, but for short
    headers whose key-phase bit is not the slot's (QPP_S_KEY_PHASE); packets
    on every other slot report QPP_S_NO_KEY both ways."""
    e = expectations()
    for si, st in enumerate(script()):
        tab = table_of(st["mirror"])
        for n in SIZES:
            b = batch(n)
            res, ures = e["s%d_n%d_res" % (si, n)], e["s%d_n%d_ures" % (si, n)]
            plain = e["s%d_n%d_exp_plain" % (si, n)]
            held = np.array([int(s) in tab for s in b["slot"]])
            phase_of = np.array([tab.get(int(s), (0, 0))[1] for s in b["slot"]])
            flipped = held & b["short"] & (b["phase"] != phase_of)
            assert (res["status"][held] == S_OK).all() and (res["status"][~held] == S_NO_KEY).all(), st["name"]
            assert (res["out_len"][held] == (b["hlen"] + b["plen"] + TAG)[held]).all()
            assert (ures["status"][~held] == S_NO_KEY).all() and (ures["status"][flipped] == S_KEY_PHASE).all()
            ok = held & ~flipped
            assert (ures["status"][ok] == S_OK).all() and (ures["pn"][ok] == b["pn"][ok]).all(), st["name"]
            assert (ures["hdr_len"][ok] == b["hlen"][ok]).all()
            for j in np.nonzero(ok)[0]:
                o, i, ln = int(b["out_off"][j]), int(b["in_off"][j]), int(b["hlen"][j] + b["plen"][j])
                assert ures[j]["out_len"] == ln and np.array_equal(plain[o : o + ln], b["inbuf"][i : i + ln])
            assert (e["s%d_n%d_umask" % (si, n)] == 1).all()  # nothing fails authentication here
            if tab:
                assert ok.sum() >= 3, st["name"]


# --------------------------------------------------------------- the check ----


def _counters():
    lib = ctypes.CDLL(os.path.join(ROOT, "aioquic_amd", "libquicpp.so"))
    lib.qpp_close_lds_launches.restype = ctypes.c_uint64
    lib.qpp_pool_fallbacks.restype = ctypes.c_uint64
    return lib.qpp_close_lds_launches, lib.qpp_pool_fallbacks


def _describe(b, j):
    return ("packet %d of %d: slot %s plen %d hdr_len %d pn_len %d %s header phase bit %d, position %d of its item"
            % (j, b["n"], "none" if b["slot"][j] == NONE else b["slot"][j], b["plen"][j], b["hlen"][j], b["pn_len"][j],
               "short" if b["short"][j] else "long", b["phase"][j], j % 16))


def compare(where, b, out, res, exp_out, exp_res, mask=None):
    """One launch against the oracle: every result record, then every output
    byte (but a failed packet's header bytes, mask == 0)."""
    bad = np.nonzero(res != exp_res)[0]
    if len(bad):
        j = int(bad[0])
        raise AssertionError("%s: %d result records differ, first %s: got %s, expected %s"
                             % (where, len(bad), _describe(b, j), res[j], exp_res[j]))
    ne = out != exp_out
    if mask is not None:
        ne &= mask.astype(bool)
    if ne.any():
        at = int(np.nonzero(ne)[0][0])
        j = min(max(0, at - LEAD) // CELL, b["n"] - 1)
        raise AssertionError("%s: %d output bytes differ, first at %d (byte %+d from the packet's output start): got "
                             "0x%02x, expected 0x%02x: %s" % (where, int(ne.sum()), at, at - int(b["out_off"][j]),
                                                              int(out[at]), int(exp_out[at]), _describe(b, j)))


def _apply(eng, st):
    """The step's table operation through the binding (the table's own
    stream), a derive call's returns against the oracle's."""
    from oracle import oracle as orc

    op, arg = st["op"], st["arg"]
    if op == "set":
        eng.table.set(np.ascontiguousarray(arg).tobytes())
    elif op == "clear":
        eng.table.clear(np.ascontiguousarray(arg).tobytes())
    elif op == "derive":
        km = eng.derive_keys(arg)
        assert km.tobytes() == st["km"].tobytes(), st["name"]
    elif op == "derive_initial":
        km, sec = eng.derive_initial_keys(arg)
        assert km.reshape(-1).tobytes() == st["km"].tobytes(), st["name"]
        for i, r in enumerate(arg):
            version = orc.VERSION_2 if r["flags"] & 1 else orc.VERSION_1
            want = orc.initial_secrets(bytes(r["cid"][: r["cid_len"]]), version)
            assert [bytes(sec[i, 0]), bytes(sec[i, 1])] == list(want), st["name"]
    else:
        assert op == "none"


def _hp_masks(eng, st):
    """qpp_session_hp_mask of 17 samples over the installed slots against the oracle."""
    from aioquic_amd import _crypto
    from oracle import oracle as orc

    held = [int(r["slot"]) for r in st["mirror"] if r["suite"] != EMPTY]
    slots = np.array([held[k % len(held)] for k in range(17)], np.uint32)
    samples = gen_bytes("lifecycle-samples-" + st["name"], 17 * 16)
    got = _crypto.hp_mask_host(eng.table, slots.tobytes(), samples)
    assert len(got) == 17 * 16
    for k, s in enumerate(slots):
        r = st["mirror"][int(s)]
        suite = int(r["suite"])
        want = orc.hp_mask(suite, r["hp"][: KEY_LEN[suite]].tobytes(), samples[16 * k : 16 * k + 16])
        assert got[16 * k : 16 * k + 5] == want[:5], "%s: header-protection mask %d, slot %d" % (st["name"], k, s)


def lifecycle_check(path, form, tag=""):
    """The whole script through one form (module docstring); the oracle's
    passes come from the file at `path`.  Returns the launches compared."""
    import torch

    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    assert (L.S_OK, L.S_DECRYPT, L.S_KEY_PHASE, L.S_NO_KEY, L.TAG_LEN, L.SLOT_NONE) == \
        (S_OK, S_DECRYPT, S_KEY_PHASE, S_NO_KEY, TAG, NONE)
    env = os.environ.get
    lone_on = (env("QPP_LONE") or "1")[0] != "0"
    bpl1 = env("QPP_GCM_BPL") == "1"
    # the switches are as the form needs them (launch_packets)
    assert form in FORMS and lone_on == (form in ("lone", "planned")) and bpl1 == (form == "quad_lds")
    planned = form == "planned"
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 5 <= 16 * cus  # gcm_two_wg: at most one item per wave, so one key means the 512-thread shape
    e = np.load(path)
    steps = script()
    eng = PacketEngine(CAP)
    assert eng.capacity == CAP
    streams = (torch.cuda.Stream(), torch.cuda.Stream())  # protect, unprotect
    handles = [s.cuda_stream for s in streams]
    assert handles[0] != handles[1] and 0 not in handles  # two streams, neither the table calls' null stream
    count, fallbacks = _counters()
    f0 = fallbacks()
    dd = {}
    for n in SIZES:
        b = batch(n)
        # every extent lies inside the buffers
        ext = b["hlen"] + b["plen"] + TAG
        assert int((b["in_off"] + ext).max()) <= b["size"] and int((b["out_off"] + ext).max()) <= b["size"]
        dd[n] = tuple(torch.from_numpy(b[k].copy().view(np.uint8)).to(dev) for k in ("desc", "ud"))
    launches = 0

    def launch(st, n, enc, src):
        nonlocal launches
        b = batch(n)
        d_desc = dd[n][0 if enc else 1]
        d_in = torch.from_numpy(np.array(src)).to(dev)
        d_out = torch.full((b["size"],), FILL, dtype=torch.uint8, device=dev)
        d_res = torch.full((n * 16,), UNWRITTEN, dtype=torch.uint8, device=dev)
        assert d_in.numel() == d_out.numel() == b["size"]
        torch.cuda.synchronize()
        stream = streams[0 if enc else 1]
        c0 = count()
        plan = eng.bucket(d_desc, n, stream=stream) if planned else None
        (eng.protect if enc else eng.unprotect)(d_desc, n, d_in, d_out, d_res, stream=stream, plan=plan)
        ran = count() - c0
        stream.synchronize()
        want = close_lds_expected(st["mirror"], form)
        assert ran == want, "%s, %d packets, %s: close-from-LDS launches %d, expected %d" % (
            st["name"], n, "protect" if enc else "unprotect", ran, want)
        launches += 1
        return d_out.cpu().numpy(), d_res.cpu().numpy().view(L.RESULT)

    for si, st in enumerate(steps):
        _apply(eng, st)
        for n in SIZES:
            b = batch(n)
            where = "step %s, %s, %d packets" % (st["name"], form, n)
            key = "s%d_n%d_" % (si, n)
            out, res = launch(st, n, True, b["inbuf"])
            compare(where + ", protect", b, out, res, e[key + "exp_wire"], e[key + "res"].astype(L.RESULT))
            if si == STALE:
                # the negative control: the oracle's output under the stale key A must not pass
                old = "s%d_n%d_" % (si - 1, n)
                try:
                    compare(where, b, out, res, e[old + "exp_wire"], e[old + "res"].astype(L.RESULT))
                except AssertionError as err:
                    assert "output bytes differ" in str(err)
                else:
                    raise AssertionError(where + ": the comparison cannot tell key A' from key A")
            out, res = launch(st, n, False, e[key + "wire_in"])
            compare(where + ", unprotect", b, out, res, e[key + "exp_plain"], e[key + "ures"].astype(L.RESULT),
                    e[key + "umask"])
            if si == STALE:
                # packets protected under the old key must not authenticate any more
                out, res = launch(st, n, False, e["s%d_n%d_wire_in" % (si - 1, n)])
                compare(where + ", unprotect of the wire image made under A", b, out, res, e["stale_n%d_exp_plain" % n],
                        e["stale_n%d_ures" % n].astype(L.RESULT), e["stale_n%d_umask" % n])
                assert (res["status"][b["slot"] == 0] == S_DECRYPT).all()
        if si in HP_AFTER:
            _hp_masks(eng, st)
    assert launches == 13 * 4 + 2
    assert _crypto.watchdog_count() == 0
    assert fallbacks() == f0
    print("lifecycle_check %s: 13 steps, %d launches compared" % (form, launches))
    if tag:
        print("lifecycle_check ok", tag)
    return launches


# ------------------------------------------------------------ GPU tests ----


@pytest.fixture(scope="module")
def expected(tmp_path_factory):
    """The .npz of the oracle's passes, computed once."""
    path = str(tmp_path_factory.mktemp("lifecycle") / "lifecycle.npz")
    np.savez(path, **expectations())
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["lone", "planned"])
def test_lifecycle(expected, form):
    """The forms an ordinary process reaches (module docstring)."""
    assert lifecycle_check(expected, form) == 54


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["quad", "quad_lds"])
def test_lifecycle_quad_unplanned(expected, form):
    """k_gcm on the unplanned batches (QPP_LONE=0 in a child process: the
    library reads its switches once); quad_lds adds QPP_GCM_BPL=1.  One child
    per switch set; a child that fails ends the test."""
    tag = "QPP_LONE=0 " + form
    code = ("import sys; sys.path.insert(0, %r); from tests.test_gpu_key_lifecycle import lifecycle_check; "
            "lifecycle_check(%r, %r, %r)" % (ROOT, expected, form, tag))
    env = dict(os.environ, QPP_LONE="0")
    env.pop("QPP_GCM_BPL", None)
    if form == "quad_lds":
        env["QPP_GCM_BPL"] = "1"
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=240)
    print("".join(x + "\n" for x in r.stdout.splitlines() if x.startswith("lifecycle_check ")), end="")
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    assert "lifecycle_check ok " + tag in r.stdout
