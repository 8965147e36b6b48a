"""Generate tests/golden/pn_decode.json from the REFERENCE's own
decode_packet_number (aioquic src/aioquic/quic/packet.py:118-132).

quic/packet.py cannot be imported here (it needs the absent `cryptography`
package), so the one function is taken out of the file's syntax tree at run
time and executed on its own; nothing of it is written into the repository,
only the numbers it returns.

Rows: [truncated_u32, num_bits, expected, rfc, result]
  truncated_u32  the packet-number bytes of the header, as an unsigned number
  rfc            0: the function receives the number the way
                 HeaderProtection.remove hands it over, a signed C int
                 (_crypto.c:349), so a 32-bit value >= 2^31 goes in minus 2^32;
                 1: it receives the unsigned number (RFC 9000 App. A.3,
                 QPP_F_RFC_PN)
  result         as Python computed it (it may be negative); consumers reduce
                 it mod 2^64, as the "K" format of AEAD.decrypt does
Domain: expected < 2^63.

Run in the build container (needs /root/reference):
    python tests/golden/make_pn_decode.py
"""

import ast
import json
import os
import random

REF = "/root/reference/src/aioquic/quic/packet.py"
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "pn_decode.json")
SEED = 0x9A3D


def reference_function():
    tree = ast.parse(open(REF).read())
    fn = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "decode_packet_number"]
    assert len(fn) == 1
    ns = {}
    exec(compile(ast.Module(body=fn, type_ignores=[]), REF, "exec"), ns)
    return ns["decode_packet_number"]


def rows(decode):
    out, seen = [], set()

    def add(trunc, bits, expected, rfc):
        key = (trunc, bits, expected, rfc)
        if key in seen or expected < 0:
            return
        seen.add(key)
        arg = trunc - (1 << 32) if (not rfc and bits == 32 and trunc >= 1 << 31) else trunc
        out.append([trunc, bits, expected, rfc, decode(arg, bits, expected)])

    # the grid of the reference's own test_decode_packet_number (tests/test_packet.py:30-50)
    for expected in (0, 128, 129, 256):
        for t in range(256):
            add(t, 8, expected, 0)
    # window edges for every packet-number length
    rng = random.Random(SEED)
    for pn_len in (1, 2, 3, 4):
        bits = 8 * pn_len
        w = 1 << bits
        h = w >> 1
        # (thinned to stay under the largest committed fixture: one seeded
        # value per length, and without the bases 5w, 2^32 + w and 2^40)
        truncs = [0, 1, h - 1, h, h + 1, w - 2, w - 1, rng.randrange(2, w - 2)]
        for base in (0, w, 1 << 31, 1 << 32, (1 << 62) - 2 * w, (1 << 62) - w, 1 << 62):
            for delta in (-h - 1, -h, -h + 1, -1, 0, 1, h - 1, h, h + 1):
                for t in truncs:
                    add(t, bits, base + delta, 0)
                    if bits == 32 and t >= 1 << 31:
                        add(t, bits, base + delta, 1)
    return out


def main():
    data = rows(reference_function())
    with open(OUT, "w") as f:
        json.dump({"generator": "tests/golden/make_pn_decode.py",
                   "reference": "decode_packet_number, aioquic src/aioquic/quic/packet.py:118-132",
                   "columns": ["truncated_u32", "num_bits", "expected", "rfc", "result"],
                   "rows": data}, f, separators=(",", ":"))
    print("wrote", OUT, len(data), "rows", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
