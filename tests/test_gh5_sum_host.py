"""CPU check of the GCM step loop's seeded window sum (tests/gh5_sum_host.cc,
a program of its own built with g++ from aioquic_amd/csrc/qpp_gh5.h): the six
even groups of windows summed pair by pair from an initial accumulator give
init ^ (a ^ b) H^4 against the oracle's gf128_mul (three keys; random blocks,
all zero, all ones, single bits on both sides of every window boundary, the
3-bit window 25), and the two-block Gh5In equals the one-block one on a ^ b."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "gh5_sum_host.cc")
ORACLE = os.path.join(ROOT, "tests", "gh5_sum_oracle.c")


def _build_and_run(tmp_path, flags):
    exe = str(tmp_path / "gh5_sum_host")
    obj = str(tmp_path / "gh5_sum_oracle.o")
    subprocess.run(["gcc", "-std=c11", "-Wall", *flags, "-I", os.path.join(ROOT, "include"), "-c", "-o", obj, ORACLE],
                   check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC, obj], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "gh5_sum_host: ok" in r.stdout


def test_gh5_sum_host(tmp_path):
    _build_and_run(tmp_path, ["-O2"])


def test_gh5_sum_host_sanitized(tmp_path):
    # address + undefined-behaviour sanitizers on the host program itself
    _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
