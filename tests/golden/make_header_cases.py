"""Extract the reference's own pull_quic_header expectations (its
tests/test_packet.py, the test_pull_* methods of PacketTest) into
tests/golden/header_cases.json: per case the input bytes, host_cid_length, and
either the expected header fields and buf.tell() or the error.

The reference test files are parsed as text with ``ast`` (nothing of the
reference is imported or executed).  Only data is kept: the input bytes, the
literal expectations of the assertions and the error texts.

Run once where the reference checkout is present (make_rfc_vectors.REF):
    python tests/golden/make_header_cases.py
"""

import ast
import binascii
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_rfc_vectors import REF, constants  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "header_cases.json")
# RFC 9000 / RFC 9369 version numbers behind the names the assertions use
VERSIONS = {"NEGOTIATION": 0, "VERSION_1": 0x00000001, "VERSION_2": 0x6B3343CF}


def _eval(node, env):
    """The expression subset of the test methods: literals, unhexlify, the
    imported packet constants, slices, version and packet-type names, lists."""
    if isinstance(node, ast.Constant):
        return node.value
    if isinstance(node, ast.Call) and getattr(node.func, "attr", None) == "unhexlify":
        return binascii.unhexlify(_eval(node.args[0], env))
    if isinstance(node, ast.Name) and node.id in env:
        return env[node.id]
    if isinstance(node, ast.Subscript) and isinstance(node.slice, ast.Slice):
        lo = _eval(node.slice.lower, env) if node.slice.lower else None
        hi = _eval(node.slice.upper, env) if node.slice.upper else None
        return _eval(node.value, env)[lo:hi]
    if isinstance(node, ast.Attribute) and getattr(node.value, "id", None) == "QuicProtocolVersion":
        return VERSIONS[node.attr]
    if isinstance(node, ast.Attribute) and getattr(node.value, "id", None) == "QuicPacketType":
        return node.attr
    if isinstance(node, ast.List):
        return [_eval(e, env) for e in node.elts]
    raise ValueError(ast.dump(node))


def _json(v):
    return v.hex() if isinstance(v, bytes) else v


def case_of(fn, env):
    case = {"name": fn.name, "host_cid_length": None, "expect": {}, "tell": None, "error": None,
            "error_text": None}
    local = dict(env)
    for node in ast.walk(fn):
        if isinstance(node, ast.Assign) and len(node.targets) == 1 and isinstance(node.targets[0], ast.Name):
            try:
                local[node.targets[0].id] = _eval(node.value, local)
            except ValueError:
                pass
    for node in ast.walk(fn):
        if not isinstance(node, ast.Call):
            continue
        name = getattr(node.func, "id", None) or getattr(node.func, "attr", None)
        if name == "Buffer" and "data" not in case:
            case["data"] = _eval(node.keywords[0].value, local).hex()
        elif name == "pull_quic_header":
            for kw in node.keywords:
                if kw.arg == "host_cid_length":
                    case["host_cid_length"] = _eval(kw.value, local)
        elif name == "assertRaises":
            case["error"] = node.args[0].id
        elif name == "assertEqual":
            a, b = node.args[:2]
            if isinstance(a, ast.Attribute) and getattr(a.value, "id", None) == "header":
                case["expect"][a.attr] = _json(_eval(b, local))
            elif isinstance(a, ast.Call) and getattr(a.func, "attr", None) == "tell":
                case["tell"] = _eval(b, local)
            elif isinstance(a, ast.Call) and getattr(a.func, "id", None) == "str":
                case["error_text"] = _eval(b, local)
    return case


def main():
    env = {}
    for tag, fname in (("V1", "test_crypto_v1.py"), ("V2", "test_crypto_v2.py")):
        c = constants(os.path.join(REF, fname))
        env["CLIENT_INITIAL_" + tag] = c["LONG_CLIENT_ENCRYPTED_PACKET"]
        env["SERVER_INITIAL_" + tag] = c["LONG_SERVER_ENCRYPTED_PACKET"]
    tree = ast.parse(open(os.path.join(REF, "test_packet.py")).read())
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "PacketTest"][0]
    cases = [case_of(fn, env) for fn in cls.body
             if isinstance(fn, ast.FunctionDef) and fn.name.startswith("test_pull_")]
    with open(OUT, "w") as f:
        json.dump({"source": "tests/test_packet.py, PacketTest.test_pull_*", "cases": cases}, f, indent=1,
                  sort_keys=True)
    print("wrote", OUT, len(cases), "cases")


if __name__ == "__main__":
    main()
