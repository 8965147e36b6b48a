"""CPU check of aioquic_amd/csrc/qpp_te4.h, built for the host with g++
(tests/te4_host.cc, a program of its own, linked with the C oracle): the
four-table AES image of the close-from-LDS form of k_gcm, its lookup addresses,
the two-table column combine (rotated key, one rotate) against the four-table
one (plain key, no rotate) for every (x, row) and for random states and keys,
and whole AES-128 / AES-256 blocks through the four-table path against the
oracle's qo_aes_block."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "te4_host.cc")
ORACLE = os.path.join(ROOT, "oracle", "qpp_oracle.c")


def _build_and_run(tmp_path, flags):
    exe = str(tmp_path / "te4_host")
    obj = str(tmp_path / "qpp_oracle.o")
    subprocess.run(["gcc", "-std=c11", "-Wall", *flags, "-c", "-o", obj, ORACLE], check=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", *flags, "-o", exe, SRC, obj], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "te4_host: ok" in r.stdout


def test_te4_host(tmp_path):
    _build_and_run(tmp_path, ["-O2"])


def test_te4_host_sanitized(tmp_path):
    # address + undefined-behaviour sanitizers on the host program itself
    _build_and_run(tmp_path, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
