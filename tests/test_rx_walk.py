"""The in-order receive rule (csrc/qpp_rxwalk.h) through `_crypto.walk_results`
against the recorded cases of tests/golden/rx_walk.json (make_rx_walk.py): the
verdict of every packet, the state returned and the bytes of every success.
walk_results launches nothing and the extension imports without a device."""

import json
import os
from collections import Counter

import numpy as np
import pytest

from aioquic_amd import layout as L
from tests import rx_walk_cases as C

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(HERE, "golden", "rx_walk.json")) as f:
        return json.load(f)["cases"]


def test_recorded_mix(golden):
    """Deferrals do not swallow the cases and all seven outcomes occur."""
    assert len(golden) == C.N_CASES
    count = Counter("".join(c["verdict"] for c in golden))
    total = sum(count.values())
    assert total == C.N_CASES * C.N_PACKETS and set(count) == set("SDLXKRC")
    assert count["D"] <= 0.40 * total
    assert all(count[k] >= 0.01 * total for k in "SDLXKRC"), count
    no_conn = untracked = 0
    for c in golden[:20]:
        a = C.case_inputs(c["seed"])
        no_conn += int((np.frombuffer(a[8], "<u4") == C.NO_CONN).sum())
        untracked += int((np.frombuffer(a[5], "u1") == 0).sum())
    assert no_conn and untracked


def test_walk_results_matches_record(golden):
    from aioquic_amd import _crypto

    for c in golden:
        got = C.record(_crypto.walk_results(*C.case_inputs(c["seed"])))
        got["seed"] = c["seed"]
        assert got == c, c["seed"]


def _args():
    return list(C.case_inputs(1))


def test_index_out_of_range():
    from aioquic_amd import _crypto

    msg = "pair, space, connection or descriptor index out of range"
    for pos, dtype, bad in ((3, "<u4", C.N_PAIRS), (4, "<u4", C.N_SPACES), (8, "<u4", C.N_CONNS),
                            (13, "<u4", C.N_PACKETS + 4)):
        a = _args()
        v = np.frombuffer(a[pos], dtype).copy()
        v[5] = bad
        a[pos] = v.tobytes()
        with pytest.raises(ValueError, match=msg):
            _crypto.walk_results(*a)


def test_result_outside_the_output():
    from aioquic_amd import _crypto

    a = _args()
    res = np.frombuffer(a[12], L.RESULT)
    assert (res["status"] == C.S_OK).any()
    a[14] = a[14][:3]
    with pytest.raises(ValueError, match="a result outside the output"):
        _crypto.walk_results(*a)
    a = _args()
    res = np.frombuffer(a[12], L.RESULT).copy()
    dix = np.frombuffer(a[13], "<u4")
    k = int(dix[np.flatnonzero(res["status"][dix] == C.S_OK)[0]])
    res[k]["hdr_len"] = res[k]["out_len"] + 1
    a[12] = res.tobytes()
    with pytest.raises(ValueError, match="a result outside the output"):
        _crypto.walk_results(*a)


def test_uneven_lengths():
    from aioquic_amd import _crypto

    n = C.N_PACKETS
    for pos, name, size in ((0, "slots", 4), (1, "exp", 8), (2, "offs", 4), (3, "pair", 4), (4, "space", 4),
                            (5, "track", 1), (8, "conn", 4), (9, "rsv", 1)):
        a = _args()
        a[pos] = a[pos][:-1]
        with pytest.raises(ValueError, match=f"{name}: {n * size - 1} bytes for {n} items of {size}"):
            _crypto.walk_results(*a)
    a = _args()
    a[6] = a[6][:-1]
    with pytest.raises(ValueError, match="space_exp: whole u64 items"):
        _crypto.walk_results(*a)
    for pos in (11, 12, 13):
        a = _args()
        a[pos] = a[pos][:-1]
        with pytest.raises(ValueError, match="dix: whole u32 items; desc and results: as many whole records"):
            _crypto.walk_results(*a)
