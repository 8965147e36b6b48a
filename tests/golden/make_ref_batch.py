"""Record what the reference's own _crypto (oracle/_ref, built by
``make -C oracle ref``) computes for the three seeded batches of
tests/test_oracle.py::test_reference_batch_checker_matches_oracle, as SHA-256
digests of the wire image, the unprotected image and the decoded packet
numbers, so that the test still holds the C oracle to the reference's results
in a tree where oracle/_ref is not built.

    python tests/golden/make_ref_batch.py     # needs oracle/_ref
"""

import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from aioquic_amd import bench_data  # noqa: E402
from tests import ref_crypto  # noqa: E402


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    ref = ref_crypto.load()
    if ref is None:
        sys.exit("oracle/_ref is not built")
    suites = {}
    for suite in (0, 1, 2):
        w = bench_data.make_workload(256, suite=suite, n_keys=3, seed=0x77 + suite, order="random")
        wire = ref_crypto.protect_all(ref, w)
        back, pns = ref_crypto.unprotect_all(ref, w, wire)
        suites[str(suite)] = {"wire_sha256": digest(wire), "back_sha256": digest(back),
                              "pns_sha256": digest(pns.astype("<u8"))}
    with open(os.path.join(HERE, "ref_batch_checker.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_ref_batch.py",
                   "workload": "bench_data.make_workload(256, suite=s, n_keys=3, seed=0x77 + s, order='random')",
                   "suites": suites}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
