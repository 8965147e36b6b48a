"""Packet-number decode pinned to the reference's own decode_packet_number
(quic/packet.py:118-132): tests/golden/pn_decode.json holds what that function
returned (tests/golden/make_pn_decode.py) for the grid of the reference's
test_decode_packet_number and for the window edges of every packet-number
length -- expected - half, expected + half, the `candidate >= window` guard,
the 2^62 - window clamp, expected at and above 2^32, and the signed hand-over
of a 4-byte number (_crypto.c:349) beside the unsigned one (QPP_F_RFC_PN).

CPU: every restatement of the function in this repository against every row.
GPU: one small packet per row, built by the oracle, through every unprotect
kernel family's decode_pn (qpp_engine.hip)."""

import importlib.util
import json
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
M64 = (1 << 64) - 1


def load_rows():
    with open(os.path.join(HERE, "golden", "pn_decode.json")) as f:
        return [tuple(r) for r in json.load(f)["rows"]]


ROWS = load_rows()


def _arg(trunc, bits, rfc):
    """The truncated number as the function receives it (see make_pn_decode.py)."""
    return trunc - (1 << 32) if (not rfc and bits == 32 and trunc >= 1 << 31) else trunc


def test_fixture_covers_the_edges():
    assert len(ROWS) > 2000
    ref_grid = {(t, e) for t, b, e, r, _ in ROWS if b == 8 and e in (0, 128, 129, 256)}
    assert len(ref_grid) == 4 * 256
    for pn_len in (1, 2, 3, 4):
        bits, w = 8 * pn_len, 1 << (8 * pn_len)
        h = w >> 1
        sub = [r for r in ROWS if r[1] == bits]
        assert {0, 1, h - 1, h, h + 1, w - 2, w - 1} <= {r[0] for r in sub}
        exps = {r[2] for r in sub}
        for base in (0, w, 1 << 31, 1 << 32, (1 << 62) - 2 * w, (1 << 62) - w, 1 << 62):
            for delta in (-h - 1, -h, -h + 1, -1, 0, 1, h - 1, h, h + 1):
                assert base + delta < 0 or base + delta in exps, (pn_len, base, delta)
    assert all(0 <= r[2] < 1 << 63 for r in ROWS)
    both = {(t, e) for t, b, e, r, _ in ROWS if b == 32 and r == 1}
    assert both and all(t >= 1 << 31 for t, _ in both)
    # the two hand-overs of a 4-byte number differ somewhere, and some results are negative
    res = {(t, b, e, r): v for t, b, e, r, v in ROWS}
    assert any(res[(t, 32, e, 0)] != res[(t, 32, e, 1)] for t, e in both)
    assert any(v < 0 for v in res.values())


def test_product_python_decode_matches_reference_rows():
    from aioquic_amd.packet import decode_packet_number

    for t, bits, exp, rfc, want in ROWS:
        assert decode_packet_number(_arg(t, bits, rfc), bits, exp) == want, (t, bits, exp, rfc)


def test_oracle_decode_matches_reference_rows(oracle):
    for t, bits, exp, rfc, want in ROWS:
        assert oracle.decode_pn(_arg(t, bits, rfc), bits, exp) == want & M64, (t, bits, exp, rfc)


def test_golden_generator_restatement_matches_reference_rows():
    spec = importlib.util.spec_from_file_location("_make_golden", os.path.join(HERE, "golden", "make_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)  # defines the functions only; the reference loads in its main()
    for t, bits, exp, rfc, want in ROWS:
        assert mod.decode_packet_number(_arg(t, bits, rfc), bits, exp) == want, (t, bits, exp, rfc)


def test_receive_walk_c_decode_matches_reference_rows():
    """decode_pn_signed of the binding's receive walks (csrc/qpp_rxwalk.h), which
    always takes a 4-byte number the signed way and reports a negative result
    as -1, through its test hook."""
    from aioquic_amd import _crypto

    n = 0
    for t, bits, exp, rfc, want in ROWS:
        if rfc:
            continue
        assert _crypto._decode_pn_signed(t, bits // 8, exp) == (want if want >= 0 else -1), (t, bits, exp)
        n += 1
    assert n > 2000


# ------------------------------------------------------------------ GPU ----


def _row_packets(oracle, L, rows, recs, slot_of):
    """One packet per row, built by the oracle: 8-byte DCID short header whose
    packet-number bytes are the row's truncated number, 8-byte payload,
    protected under the row's decoded number.  -> (wire, udesc, size, payloads)"""
    from aioquic_amd.batch import layout_packets

    rng = np.random.default_rng(0x9D)
    headers, payloads, pns, slots = [], [], [], []
    for i, (t, bits, exp, rfc, want) in enumerate(rows):
        pn_len = bits // 8
        headers.append(bytes([0x40 | (pn_len - 1)]) + rng.bytes(8) + t.to_bytes(pn_len, "big"))
        payloads.append(rng.bytes(8))
        pns.append(want & M64)
        slots.append(slot_of(i))
    inbuf, desc, size = layout_packets(headers, payloads, pns, slots)
    wire, res = oracle.protect_batch(recs, desc, inbuf, size)
    assert (res["status"] == L.S_OK).all()
    ud = desc.copy()
    ud["len"] = res["out_len"]
    ud["hdr_len"] = 9
    ud["pn"] = np.array([r[2] for r in rows], np.uint64)
    ud["flags"] = [L.F_RFC_PN if r[3] else 0 for r in rows]
    return wire, ud, size, headers, payloads


def _check_rows(oracle, L, eng, rows, recs, slot_of, chunk=None, planned=False):
    import torch

    wire, ud, size, headers, payloads = _row_packets(oracle, L, rows, recs, slot_of)
    exp_out, exp_res = oracle.unprotect_batch(recs, ud, wire, size)
    d_wire = torch.from_numpy(wire).cuda()
    n = len(rows)
    step = chunk or n
    got_res = np.zeros(n, L.RESULT)
    d_out = torch.zeros(size, dtype=torch.uint8, device="cuda")
    for lo in range(0, n, step):
        m = min(step, n - lo)
        d_desc = torch.from_numpy(ud[lo : lo + m].view(np.uint8).copy()).cuda()
        d_res = torch.zeros(m * 16, dtype=torch.uint8, device="cuda")
        plan = eng.bucket(d_desc, m) if planned else None
        eng.unprotect(d_desc, m, d_wire, d_out, d_res, plan=plan)
        torch.cuda.synchronize()
        got_res[lo : lo + m] = d_res.cpu().numpy().view(L.RESULT)
    out = d_out.cpu().numpy()
    bad = np.nonzero(got_res["status"] != L.S_OK)[0]
    assert not len(bad), [(rows[i], int(got_res[i]["status"])) for i in bad[:8]]
    want = np.array([r[4] & M64 for r in rows], np.uint64)
    bad = np.nonzero(got_res["pn"] != want)[0]
    assert not len(bad), [(rows[i], int(got_res[i]["pn"])) for i in bad[:8]]
    assert (got_res == exp_res).all()
    for i in range(n):
        o, hl = int(ud[i]["out_off"]), len(headers[i])
        assert out[o : o + hl + 8].tobytes() == headers[i] + payloads[i], rows[i]
    assert np.array_equal(out, exp_out)


@pytest.fixture(scope="module")
def pn_engine():
    from aioquic_amd.batch import PacketEngine
    from tests.test_gpu_parity import _keys

    recs = _keys(np.random.default_rng(0x9E), 3)  # slot s holds suite s
    eng = PacketEngine(3)
    eng.set_key_records(recs)
    return eng, recs


@pytest.mark.gpu
@pytest.mark.parametrize("planned", [False, True], ids=["unplanned", "planned"])
def test_device_decode_matches_reference_rows(oracle, pn_engine, planned):
    """Every row, the three suites round-robin.  Unplanned: k_lone_gcm for
    both AES-GCM suites and k_chacha (more than 64 ChaCha20 packets); planned:
    k_gcm for both and k_chacha."""
    from aioquic_amd import layout as L

    eng, recs = pn_engine
    _check_rows(oracle, L, eng, ROWS, recs, lambda i: i % 3, planned=planned)


@pytest.mark.gpu
def test_device_decode_lone_chacha_32bit_rows(oracle, pn_engine):
    """Every 4-byte row on the ChaCha20-Poly1305 key in unplanned launches of
    at most 64 packets: k_lone_chacha."""
    from aioquic_amd import layout as L

    eng, recs = pn_engine
    rows = [r for r in ROWS if r[1] == 32]
    assert len(rows) > 300
    _check_rows(oracle, L, eng, rows, recs, lambda i: 2, chunk=64)
