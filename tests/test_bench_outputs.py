"""bench.py --dump-outputs and the plain / --full split.

CPU: dump_outputs on host tensors (names, dtypes, the size bound, the fixed
sample).  GPU: one short plain run of the script itself; its line carries the
headline fields and null for everything --full holds, and the dumped wire
bytes are the oracle's for the same seeded workload."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

NAMES = {"sample_index", "protect_wire", "unprotect_plain", "protect_results", "unprotect_results",
         "protect_wire_sums", "unprotect_plain_sums", "protect_status", "unprotect_status"}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def test_dump_outputs_on_host_tensors(tmp_path):
    import torch

    from aioquic_amd import layout as L

    n, shift = bench.DUMP_PACKETS + 77, 5
    rng = np.random.default_rng(3)
    wire = rng.integers(0, 256, n * 1200 + shift, dtype=np.uint8)
    back = rng.integers(0, 256, n * 1200 + shift, dtype=np.uint8)
    res = np.zeros(n, L.RESULT)
    res["pn"] = np.arange(n) + (1 << 40)
    res["status"] = np.arange(n) % 3
    res["out_len"] = 1200
    t = [torch.from_numpy(a.view(np.uint8).copy()) for a in (wire, back, res, res)]
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), n, shift, *t)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert set(a) == NAMES
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) < 64 << 20
    for k in a:
        assert np.array_equal(a[k], b[k]), k  # the same sample every time
    sel = a["sample_index"].astype(np.int64)
    assert len(sel) == bench.DUMP_PACKETS and len(set(sel)) == len(sel) and sel.max() < n
    slots = wire[shift:].reshape(n, 1200)
    assert np.array_equal(a["protect_wire"], slots[sel].astype(np.float32))
    assert np.array_equal(a["protect_wire_sums"], slots.sum(axis=1, dtype=np.int64).astype(np.float32))
    assert np.array_equal(a["unprotect_plain"], back[shift:].reshape(n, 1200)[sel].astype(np.float32))
    assert np.array_equal(a["protect_results"][:, 0], res["pn"][sel].astype(np.float64))  # exact above 2^32
    assert np.array_equal(a["unprotect_status"], res["status"].astype(np.float32))


@pytest.mark.gpu
def test_plain_run_line_and_dump_match_oracle(tmp_path, oracle):
    from aioquic_amd.bench_data import make_workload

    n = 3000  # not a multiple of the dump sample, several workgroups
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--packets", str(n), "--dump-outputs", out], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["full"] is False
    assert line["value"] > 0 and line["ms_per_step"] > 0
    # value and ms_per_step say the same thing: bytes of 3 steps over their time
    # (ms_per_step is rounded to 0.1 us, under 1 % of a step this short)
    assert line["value"] == pytest.approx(n * 1200 / (line["ms_per_step"] / 1e3) / bench.GIB, rel=1e-2)
    for k in ("cpu_baseline", "cpu_baseline_all_cores", "sustained", "status_ok"):
        assert line[k] is None, k
    assert "e2e" not in line and "key_schedule" not in line and line["roofline"]["attainable_copy"] is None

    d = _load(out)
    assert set(d) == NAMES
    w = make_workload(n, seed=0x9001)  # the north-star config's workload at n packets
    wire, res = oracle.protect_batch(w.keys, w.desc, w.plain, w.wire_size)
    sel = d["sample_index"].astype(np.int64)
    assert np.array_equal(d["protect_wire"], wire.reshape(n, 1200)[sel].astype(np.float32))
    assert np.array_equal(d["protect_wire_sums"], wire.reshape(n, 1200).sum(axis=1, dtype=np.int64).astype(np.float32))
    assert not d["protect_status"].any() and not d["unprotect_status"].any()
    for i, f in enumerate(res.dtype.names):
        assert np.array_equal(d["protect_results"][:, i], res[f][sel].astype(np.float64)), f
    plain = w.plain.reshape(n, 1200)
    assert np.array_equal(d["unprotect_plain"][:, :1184], plain[sel, :1184].astype(np.float32))
