"""The library's environment switches and build variants (CPU, reads the sources): pn_read_switches (csrc/api.hip) is the only
reader of the environment in popnet_amd/csrc, every switch it reads is exercised by a GPU test, and no source file is compiled
differently by a preprocessor condition -- the kernels a test runs are the kernels that ship."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "popnet_amd", "csrc")


def _sources():
    paths = sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))
    assert paths
    return {os.path.basename(p): open(p).read() for p in paths}


def _read_switches_span(text):
    """(start, end) character offsets of pn_read_switches' definition in api.hip."""
    m = re.search(r"^PnSwitches pn_read_switches\(\)\s*\{", text, re.M)
    assert m, "pn_read_switches is not defined in api.hip"
    depth, i = 0, m.end() - 1
    while True:
        depth += {"{": 1, "}": -1}.get(text[i], 0)
        if depth == 0:
            return m.start(), i + 1
        i += 1


def test_getenv_only_in_read_switches():
    srcs = _sources()
    start, end = _read_switches_span(srcs["api.hip"])
    outside = []
    for name, text in srcs.items():
        for m in re.finditer(r"\bgetenv\s*\(", text):
            if name != "api.hip" or not start <= m.start() < end:
                outside.append("%s:%d" % (name, text.count("\n", 0, m.start()) + 1))
    assert not outside, "getenv outside pn_read_switches: %s" % outside
    assert "getenv(" in srcs["api.hip"][start:end]


def test_every_switch_has_a_gpu_test():
    api = _sources()["api.hip"]
    start, end = _read_switches_span(api)
    names = sorted(set(re.findall(r'"(POPNET_[A-Z0-9_]+)"', api[start:end])))
    assert len(names) >= 20, names
    tests = "".join(open(p).read() for p in glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))
    untested = [n for n in names if n not in tests]
    assert not untested, "switches no GPU test sets: %s" % untested


def test_no_conditional_compilation():
    found = []
    for name, text in _sources().items():
        for i, line in enumerate(text.splitlines(), 1):
            if re.match(r"\s*#\s*(if|ifdef|ifndef|elif)\b", line):
                found.append("%s:%d: %s" % (name, i, line.strip()))
    assert not found, "conditional compilation in popnet_amd/csrc:\n" + "\n".join(found)
