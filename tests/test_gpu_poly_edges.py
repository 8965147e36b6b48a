"""The crafted packets of tests/poly_cases.py (Poly1305 carry edges, each with
its modelled p130_finish input) through the ChaCha20-Poly1305 kernels, byte
for byte against the C oracle and the integer definition's tag.

The batch: packet i in its own 1600-byte cell of the input buffer and of a
separate output buffer, at offsets with independent residues mod 16 and 0xA5
wherever no packet lies (the layout of tests/test_gpu_lengths.py).  One key.

Three passes per form, whole output buffer and every result record compared
with the oracle's:
  unprotect of the crafted wire image (the crafted ciphertext under the
      integer definition's tag): QPP_S_OK and the plaintext;
  protect of that plaintext: the crafted ciphertext and that tag;
  unprotect with the top bit of the tag's last byte flipped: QPP_S_DECRYPT for
      every packet, the payload region zeros.
Forms:
  lone64   consecutive unplanned launches of 64 descriptors: k_lone_chacha
           (its close: the wave sum)                  [launch rule: lone_max = 64]
  prio     one unplanned launch of the whole set (more than 64 packets, at most
           16 waves per CU): k_chacha, priority form (chacha_packet's close)
  planned  plan=eng.bucket(...), two slots holding the same key material, the
           packets alternating between them: k_chacha
No launch is built for k_chacha without priority: its template flag only
moves s_setprio, the Poly1305 code is the same instantiation of chacha_packet.

A mismatch names the packet's class, the close it was made for, its shape and
the modelled finish limbs.
"""

import functools

import numpy as np
import pytest

from tests import poly_cases as pc
from tests import ref_crypto

S_OK, S_DECRYPT = 0, 2
TAG = 16
FILL = 0xA5
CELL, LEAD, PAD = 1600, 64, 24
FORMS = {
    # form: (keys installed, descriptors per launch or 0 = all, planned, the close it runs)
    "lone64": (1, 64, False, "lone"),
    "prio": (1, 0, False, "packet"),
    "planned": (2, 0, True, "packet"),
}


def _keys(n):
    from oracle.oracle import KEY_DTYPE

    key, iv, hp = pc.make_key()
    recs = np.zeros(n, KEY_DTYPE)
    for s in range(n):
        recs[s]["slot"] = s
        recs[s]["suite"] = pc.CHACHA
        recs[s]["iv"] = np.frombuffer(iv, np.uint8)
        recs[s]["key"] = np.frombuffer(key, np.uint8)
        recs[s]["hp"] = np.frombuffer(hp, np.uint8)
    return recs


@functools.lru_cache(maxsize=None)
def batch():
    """The crafted set laid out: descriptors of both directions, the protect
    input, and the oracle's three passes (expected buffers and records)."""
    from oracle import oracle as orc
    from oracle.oracle import DESC_DTYPE

    pk = pc.crafted()
    n = len(pk)
    i = np.arange(n, dtype=np.int64)
    in_off = LEAD + CELL * i + PAD + (5 * i + 3) % 16
    out_off = LEAD + CELL * i + PAD + (7 * (i // 16) + 11 * i + 1) % 16
    hlen = np.array([len(p["hdr"]) for p in pk], np.int64)
    plen = np.array([p["plen"] for p in pk], np.int64)
    pn_len = np.array([p["pn_len"] for p in pk], np.int64)
    size = LEAD + CELL * n
    inbuf = np.full(size, FILL, np.uint8)
    for j, p in enumerate(pk):
        o = int(in_off[j])
        inbuf[o : o + len(p["hdr"]) + p["plen"]] = np.frombuffer(p["hdr"] + p["plain"], np.uint8)
    desc = np.zeros(n, DESC_DTYPE)
    desc["in_off"], desc["out_off"] = in_off, out_off
    desc["len"], desc["hdr_len"] = plen, hlen
    desc["flags"] = [p["flags"] for p in pk]
    desc["pn"] = [p["pn"] for p in pk]
    ud = desc.copy()
    ud["len"] = hlen + plen + TAG
    ud["hdr_len"] = hlen - pn_len

    recs = _keys(1)
    wire_o, res = orc.protect_batch(recs, desc, inbuf, size)
    assert (res["status"] == S_OK).all() and (res["out_len"] == hlen + plen + TAG).all()
    exp_wire = np.full(size, FILL, np.uint8)
    wire_in = np.full(size, FILL, np.uint8)
    for j, p in enumerate(pk):
        o, a, ln, h = int(out_off[j]), int(in_off[j]), int(res[j]["out_len"]), int(hlen[j])
        got = wire_o[o : o + ln].tobytes()
        # the oracle's ciphertext is the crafted one and its tag the integer definition's
        assert got[h:] == p["ct"] + p["tag"], pc.describe(p, "oracle")
        assert not p["flags"] or got[:h] == p["hdr"]
        exp_wire[o : o + ln] = wire_o[o : o + ln]
        wire_in[a : a + ln] = wire_o[o : o + ln]
    plain_o, ures = orc.unprotect_batch(recs, ud, wire_in, size)
    assert (ures["status"] == S_OK).all() and (ures["pn"] == desc["pn"]).all()
    assert (ures["out_len"] == hlen + plen).all() and (ures["hdr_len"] == hlen).all()
    exp_plain = np.full(size, FILL, np.uint8)
    for j in range(n):
        o, a, ln = int(out_off[j]), int(in_off[j]), int(ures[j]["out_len"])
        exp_plain[o : o + ln] = plain_o[o : o + ln]
        assert np.array_equal(plain_o[o : o + ln], inbuf[a : a + ln])
    tampered_in = wire_in.copy()
    tampered_in[in_off + hlen + plen + TAG - 1] ^= 0x80
    _, tres = orc.unprotect_batch(recs, ud, tampered_in, size)
    assert (tres["status"] == S_DECRYPT).all()
    exp_t = np.full(size, FILL, np.uint8)
    tmask = np.ones(size, np.uint8)
    for j in range(n):
        o, h, pl = int(out_off[j]), int(hlen[j]), int(plen[j])
        tmask[o : o + h] = 0  # a failed packet's header bytes are not compared
        exp_t[o + h : o + h + pl] = 0
    return dict(pk=pk, n=n, size=size, desc=desc, ud=ud, inbuf=inbuf, wire_in=wire_in, tampered_in=tampered_in,
                exp_wire=exp_wire, exp_plain=exp_plain, exp_t=exp_t, tmask=tmask, res=res, ures=ures, tres=tres)


# ------------------------------------------------------------ CPU tests ----


def test_crafted_set_has_the_stated_geometry():
    """(CPU) Every (class, close, shape) cell the algebra allows holds at
    least 4 packets whose modelled finish input satisfies the class predicate;
    the cells that cannot exist are exactly poly_cases.IMPOSSIBLE (named there
    with the reason); the retry cap empties none.  Prints every cell."""
    pk = pc.crafted()
    cells = pc.cells(pk)
    assert set(cells) == {(c, k, s) for c in pc.CLASSES for k in pc.CLOSES for s in pc.PAYLOADS}
    assert 200 <= len(pk) <= 400
    for key in sorted(cells, key=str):
        held = cells[key]
        if key in pc.IMPOSSIBLE:
            assert not held
            print("cell %-8s %-6s %4d B: cannot exist: %s" % (key + (pc.IMPOSSIBLE[key],)))
            continue
        print("cell %-8s %-6s %4d B: %d packets" % (key + (len(held),)))
        assert len(held) >= pc.PER_CELL, key
    assert set(pc.IMPOSSIBLE) <= set(cells)
    assert max(p["attempts"] for p in pk) < pc.CAP
    for p in pk:
        # the model's limbs represent the tag polynomial's residue, in both closes
        for close in pc.CLOSES:
            assert pc.value(p["fin"][close]) % pc.P == p["residue"], pc.describe(p, close)
            assert pc.p_finish(p["fin"][close], p["s"]).to_bytes(16, "little") == p["tag"], pc.describe(p, close)
        # a packet made for one close has the pattern there
        if p["close"]:
            assert pc.holds(p["cls"], p["want"], p["fin"][p["close"]], p["s"])
        if p["cls"] == "d":
            assert set(p["hdr"] + p["ct"]) <= {0xFF}
    # class a in numbers: h3 parities, both kinds of header, every shape
    a = [p for p in pk if p["cls"] in ("a_odd", "a_even")]
    assert {(p["cls"], p["close"], bool(p["flags"])) for p in a if p["plen"] >= 16} == \
        {(c, k, f) for c in ("a_odd", "a_even") for k in pc.CLOSES for f in (False, True)}
    assert {p["want"] for p in pk if p["cls"] == "b"} == set(pc.B_RESIDUES)
    assert any(p["tag"] == bytes(16) for p in pk if p["cls"] == "c_zero")
    # shapes: no chunk, one chunk whole and partial, two chunks, two steps, a full-size packet
    chunks = {(p["plen"] + 63) // 64 for p in pk}
    assert {0, 1, 2, 5, 19} <= chunks and any(p["plen"] % 16 for p in pk)
    print("crafted set: %d packets, %d of class a, most attempts %d of %d"
          % (len(pk), len(a), max(p["attempts"] for p in pk), pc.CAP))


def test_oracle_accepts_the_crafted_set(oracle, request):
    """(CPU) The oracle protects every crafted plaintext into the crafted
    ciphertext under the integer definition's tag, accepts every crafted wire
    image and rejects every tampered one (asserted inside batch()); where
    oracle/_ref is built, the reference's ChaCha20-Poly1305 says the same."""
    b = batch()
    assert (b["exp_wire"] != FILL).sum() > 50 * b["n"]
    key, iv, _ = pc.make_key()
    ref = ref_crypto.checker(request.node.nodeid)
    if ref is not None:
        aead = ref.AEAD(b"chacha20-poly1305", key, iv)
        for p in b["pk"]:
            assert aead.encrypt(p["plain"], p["hdr"], p["pn"]) == p["ct"] + p["tag"], pc.describe(p, "reference")
            assert aead.decrypt(p["ct"] + p["tag"], p["hdr"], p["pn"]) == p["plain"], pc.describe(p, "reference")


# --------------------------------------------------------------- the check ----


def poly_run(form):
    """The three passes of one form on the GPU.  -> {pass name: indices of the
    packets whose output cell or result record differs from the oracle's}."""
    import torch

    from aioquic_amd import _crypto
    from aioquic_amd import layout as L
    from aioquic_amd.batch import PacketEngine

    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    b = batch()
    n, size = b["n"], b["size"]
    n_keys, chunk, planned, _ = FORMS[form]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    if form == "prio":
        assert 64 < n and (n + 15) // 16 <= 16 * cus  # lone_max, chacha_prio
    eng = PacketEngine(2)
    eng.set_key_records(_keys(n_keys).astype(L.KEY_MATERIAL))
    bad = {}
    passes = (("unprotect", False, b["ud"], b["wire_in"], b["exp_plain"], b["ures"], None),
              ("protect", True, b["desc"], b["inbuf"], b["exp_wire"], b["res"], None),
              ("tampered unprotect", False, b["ud"], b["tampered_in"], b["exp_t"], b["tres"], b["tmask"]))
    for name, enc, desc, src, exp, exp_res, mask in passes:
        desc = desc.copy()
        if planned:
            desc["slot"] = np.arange(n) & 1
        ext_in = desc["hdr_len"] + desc["len"] if enc else desc["len"]
        assert int((desc["in_off"] + ext_in).max()) <= size and int(desc["out_off"].max()) + CELL - 100 <= size
        d_desc = torch.from_numpy(desc.view(np.uint8)).to(dev)
        d_in = torch.from_numpy(np.ascontiguousarray(src)).to(dev)
        d_out = torch.full((size,), FILL, dtype=torch.uint8, device=dev)
        d_res = torch.full((n * 16,), 0xEE, dtype=torch.uint8, device=dev)
        run = eng.protect if enc else eng.unprotect
        plan = eng.bucket(d_desc, n) if planned else None
        step = chunk or n
        for at in range(0, n, step):
            run(d_desc[40 * at :], min(step, n - at), d_in, d_out, d_res[16 * at :], plan=plan)
        torch.cuda.synchronize()
        out = d_out.cpu().numpy()
        res = d_res.cpu().numpy().view(L.RESULT)
        ne = out != exp
        if mask is not None:
            ne &= mask.astype(bool)
        assert not ne[:LEAD].any(), "%s %s: bytes before the first cell changed" % (form, name)
        cell_bad = ne[LEAD:].reshape(n, CELL).any(axis=1)
        rec_bad = res != exp_res.astype(L.RESULT)
        bad[name] = np.nonzero(cell_bad | rec_bad)[0].tolist()
    assert _crypto.watchdog_count() == 0
    return bad


def summarize(form, bad):
    """one line per pass and class of what differed (empty when nothing did)"""
    pk = batch()["pk"]
    close = FORMS[form][3]
    lines = []
    for name, idx in bad.items():
        per = {}
        for j in idx:
            key = (pk[j]["cls"], pk[j]["close"] or "both")
            per[key] = per.get(key, 0) + 1
        for (cls, made), k in sorted(per.items()):
            tot = sum(1 for p in pk if p["cls"] == cls and (p["close"] or "both") == made)
            lines.append("%s %s: class %s made for %s: %d of %d packets differ" % (form, name, cls, made, k, tot))
        if idx:
            lines.append("  first: " + pc.describe(pk[idx[0]], close))
    return lines


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
def test_poly_edges(form):
    """Every crafted packet through k_lone_chacha (lone64) and k_chacha (prio,
    planned), both directions and tampered (module docstring)."""
    bad = poly_run(form)
    lines = summarize(form, bad)
    print("poly_edges %s: %d packets per pass, %s" % (form, batch()["n"], "all agree" if not lines else "DIFFER"))
    assert not lines, "\n".join(lines)
