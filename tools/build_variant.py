#!/usr/bin/env python3
"""Build an A/B variant of libquicpp.so with extra compile flags, or from
another version of qpp_engine.hip, into variants/<name>/libquicpp.so (the
in-tree library is left alone):

    python tools/build_variant.py NAME [--src FILE | --rev GITREV] -DQPP_SWITCH=0 ...

Every other unit of build.HIP_UNITS is linked as the in-tree build left it,
except qpp_session.o beside an engine that still defines the sessions itself
(revisions from before qpp_session.hip).  --rev compiles that revision's
engine beside today's headers, so it takes revisions that still compile there.
The variant links the in-tree source-hash object, so the in-tree _crypto
extension accepts it (a deliberate A/B, not a stale build).
tools/ab_lib.sh runs the bench against such builds via LD_LIBRARY_PATH."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]
name = args.pop(0)
src = os.path.join(ROOT, "aioquic_amd", "csrc", "qpp_engine.hip")
if args and args[0] in ("--src", "--rev"):
    kind, val = args.pop(0), args.pop(0)
    if kind == "--src":
        src = os.path.abspath(val)
    else:
        # the engine of another revision, compiled beside today's headers
        src = os.path.join(ROOT, "aioquic_amd", "csrc", f".variant_{name}.hip")
        with open(src, "w") as f:
            f.write(subprocess.run(["git", "show", f"{val}:aioquic_amd/csrc/qpp_engine.hip"], cwd=ROOT,
                                   check=True, capture_output=True, text=True).stdout)
flags = args
out = os.path.join(ROOT, "variants", name)
os.makedirs(out, exist_ok=True)
obj = os.path.join(out, "qpp_engine.o")
hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
try:
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "aioquic_amd", "csrc"), "-c", "-o", obj] + flags + [src], check=True)
    with open(src) as f:
        own_sessions = "qpp_session_create(" in f.read()  # an engine from before qpp_session.hip
finally:
    if os.path.basename(src).startswith(".variant_"):
        os.remove(src)
# aioquic_amd/build.py, by its path: the list of units and where their objects are
spec = importlib.util.spec_from_file_location("qpp_build", os.path.join(ROOT, "aioquic_amd", "build.py"))
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)
skip = {"qpp_engine.hip"} | ({"qpp_session.hip"} if own_sessions else set())
objs = [obj] + [build._obj(u) for u in build.HIP_UNITS if u not in skip] + \
    [os.path.join(build.OBJ, "qpp_source_hash.o")]
missing = [o for o in objs if not os.path.exists(o)]
if missing:
    sys.exit("build the tree first (python -m aioquic_amd.build): missing " + ", ".join(missing))
subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", os.path.join(out, "libquicpp.so")] + objs,
               check=True)
os.remove(obj)
print(os.path.join(out, "libquicpp.so"))
