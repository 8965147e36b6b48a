"""The in-order receive rule (aioquic_amd/csrc/qpp_rxwalk.h) as a program of its
own: tests/rxwalk_host.c is built with gcc under -fsanitize=address,undefined and
run.  Its main() holds the named scenarios, one per rule, with the verdicts and the
final state written out by hand, and the seeded comparison of the two ways the
binding's walks state a packet's facts (see the file's header comment)."""

import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rxwalk_host(tmp_path):
    exe = str(tmp_path / "rxwalk_host")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover",
                    "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "aioquic_amd", "csrc"),
                    "-o", exe, os.path.join(ROOT, "tests", "rxwalk_host.c")], check=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stdout.startswith("ok: 14 scenarios, 400 seeded cases"), run.stdout
