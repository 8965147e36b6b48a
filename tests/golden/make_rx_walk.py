"""Generate tests/golden/rx_walk.json: what `_crypto.walk_results` of a built
extension returns for the seeded inputs of tests/rx_walk_cases.py.

The file pins the in-order receive rule (aioquic_amd/csrc/qpp_rxwalk.h) to what
the binding computed before the rule was gathered into one place: run this from a
checkout whose extension is the one to record, tests/test_rx_walk.py then holds
every later tree to it.  walk_results launches nothing: no GPU is needed.

Per case: one letter per packet (S success, D deferred, or the final status:
L length, X decrypt, K no key, R reserved bits 0x101, C closed 0x102), the
returned space_exp and closed, and a SHA-256 over header + payload + pn (8 bytes,
little endian) of every success in order.

    python tests/golden/make_rx_walk.py
"""

import json
import os
import sys
from collections import Counter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import rx_walk_cases as C  # noqa: E402

OUT = os.path.join(HERE, "rx_walk.json")
SEED = 0x52D7


def check_mix(cases):
    """Deferrals must not swallow the cases, and every outcome must occur."""
    count = Counter("".join(c["verdict"] for c in cases))
    total = sum(count.values())
    share = {k: count[k] / total for k in "SDLXKRC"}
    assert share["D"] <= 0.40, share
    assert all(v >= 0.01 for v in share.values()), share
    assert set(count) <= set("SDLXKRC"), count
    return share


def main():
    from aioquic_amd import _crypto

    cases = []
    for k in range(C.N_CASES):
        rec = C.record(_crypto.walk_results(*C.case_inputs(SEED + k)))
        rec["seed"] = SEED + k
        cases.append(rec)
    share = check_mix(cases)
    with open(OUT, "w") as f:
        f.write('{"cases": [\n' + ",\n".join(json.dumps(c, separators=(",", ":")) for c in cases) + "\n]}\n")
    print(OUT, os.path.getsize(OUT), "bytes;", " ".join(f"{k} {100 * v:.1f}%" for k, v in share.items()))


if __name__ == "__main__":
    main()
