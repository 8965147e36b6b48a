"""Every switch left in the native sources is a product or test switch that
some test drives (VERDICT r6 finding 6): study switches are measured, recorded
in DESIGN.md ("Study switches removed") and deleted, not kept beside the
product path.  This reads aioquic_amd/csrc/ and include/ as text: it compiles
nothing and needs no device."""

import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE_DIRS = [os.path.join(ROOT, "aioquic_amd", "csrc"), os.path.join(ROOT, "include")]

# environment switches the library reads, each named by the test that sets it
ENV_SWITCHES = {
    "QPP_GCM_BPL", "QPP_LONE", "QPP_ZERO_COPY", "QPP_LONE_STAGE", "QPP_SPIN_LIMIT", "QPP_PAIR_DELAY",
    "QPP_SESSION_SERIAL", "QPP_PLAN_RADIX",
}
# build-time switches: the instrumented build of tools/probe.hip and tools/lone_probe.hip
BUILD_SWITCHES = {"QPP_PROBE"}
# preprocessor conditions that are no switches: include guards, and the source
# hash the build passes in (aioquic_amd/build.py)
EXEMPT = {"QUIC_PP_H", "QPP_SOURCE_HASH"}

_ENV = re.compile(r'\b(?:getenv|qpp_env_long)\s*\(\s*"(QPP_\w+)"')
_GETENV = re.compile(r"\bgetenv\s*\(\s*([^)]*)\)")
_COND = re.compile(r"^\s*#\s*(ifdef|ifndef|if|elif|else|endif)\b(.*)$")
_DEFINE = re.compile(r"^\s*#\s*define\s+(\w+)")
_NAME = re.compile(r"\b(?:QPP|QUIC_PP)_\w+")


def _sources():
    for d in SOURCE_DIRS:
        for name in sorted(os.listdir(d)):
            if name.endswith((".h", ".hip", ".c")):
                with open(os.path.join(d, name)) as f:
                    yield name, f.read()


def _strip_comment(line):
    return line.split("//")[0].split("/*")[0]


def _scan():
    """(environment names, raw getenv arguments, names tested by the
    preprocessor, names #defined outside every non-exempt condition)."""
    env, raw, tested, fixed = set(), [], set(), set()
    for name, text in _sources():
        env.update(_ENV.findall(text))
        raw += [(name, a.strip()) for a in _GETENV.findall(text)]
        stack = []  # per open condition: is it on exempt names only?
        for line in text.replace("\\\n", " ").split("\n"):
            m = _COND.match(line)
            if m:
                kind, names = m.group(1), set(_NAME.findall(_strip_comment(m.group(2))))
                if kind in ("if", "ifdef", "ifndef"):
                    tested |= names
                    stack.append(bool(names) and names <= EXEMPT)
                elif kind == "elif":
                    tested |= names
                    stack[-1] = False
                elif kind == "else":
                    stack[-1] = False
                else:
                    stack.pop()
                continue
            m = _DEFINE.match(line)
            if m and all(stack):
                fixed.add(m.group(1))
        assert not stack, name
    return env, raw, tested, fixed


def test_environment_switches_are_the_tested_ones():
    env, raw, _, _ = _scan()
    assert env == ENV_SWITCHES
    # one reader: the helper's own getenv(name) is the only direct call
    assert [a for _, a in raw] == ["name"], raw


def test_build_switches_are_the_probe_only():
    _, _, tested, fixed = _scan()
    assert {n for n in tested if n.startswith("QPP_")} - fixed - EXEMPT == BUILD_SWITCHES
    assert tested & EXEMPT == EXEMPT  # the short list names nothing that is not there


def test_every_environment_switch_is_driven_by_a_test():
    tests = os.path.join(ROOT, "tests")
    text = ""
    for name in sorted(os.listdir(tests)):
        if name.endswith(".py") and name != os.path.basename(__file__):
            with open(os.path.join(tests, name)) as f:
                text += f.read()
    for sw in sorted(ENV_SWITCHES):
        assert re.search(r"\b%s\b" % sw, text), sw
