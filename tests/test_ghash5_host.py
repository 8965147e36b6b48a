"""CPU check of aioquic_amd/csrc/qpp_gh5.h, built for the host with g++
(tests/ghash5_host.cc, a program of its own): the one-op window addresses of
the close-from-LDS GCM step loop against ((x >> 5w) & 31) << 3, the H^8 table
against the H^4 table's entries times H^4 (bitwise reference, three keys), and
(a ^ x0) H^8 ^ x1 H^4 against ((a ^ x0) H^4 ^ x1) H^4 through the tables."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ghash5_host.cc")


def _build_and_run(tmp_path, flags):
    exe = str(tmp_path / "ghash5_host")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ghash5_host: ok" in r.stdout


def test_ghash5_host(tmp_path):
    _build_and_run(tmp_path, ["-O2"])


def test_ghash5_host_sanitized(tmp_path):
    # address + undefined-behaviour sanitizers on the host program itself
    _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
