"""CPU check of the host batch path's HIP-free headers, built for the host with
g++ (tests/session_host.cc, a program of its own): aioquic_amd/csrc/qpp_hostcopy.h
-- the non-temporal copy over sizes and alignments around its thresholds, the
copy pool's group life cycle, two callers at once, a forked child -- and
aioquic_amd/csrc/qpp_batch.h -- the overflow-safe bounds check, the pipeline's
chunk count, tiling and chunk input extents against a brute-force restatement,
and qpp_multi's range split with its invariants."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "session_host.cc")


def _build_and_run(tmp_path, flags):
    exe = str(tmp_path / "session_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-pthread", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "session_host: ok" in r.stdout


def test_session_host(tmp_path):
    _build_and_run(tmp_path, ["-O2"])


def test_session_host_sanitized(tmp_path):
    # address + undefined-behaviour sanitizers on the host program itself
    _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])


def test_session_host_thread_sanitized(tmp_path):
    # the pool's locking under ThreadSanitizer (the program leaves the fork case out of this build)
    _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=thread"])
