"""The PXR_* environment switches: every one the product reads is documented, and every one a test or tool sets is read.

The second half guards a trap of deleting a variant: a test that still sets the deleted variable keeps passing, because it now
compares the default with the default."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "pixel-perfect-sfm_amd")
NAME = r"PXR_[A-Z0-9_]+"


def _sources(top, exts):
    for ext in exts:
        for path in glob.glob(os.path.join(top, "**", "*" + ext), recursive=True):
            if os.sep + "build" + os.sep not in path and os.path.abspath(path) != os.path.abspath(__file__):
                yield path, open(path, errors="replace").read()


def _read_by_the_product():
    names = set()
    for _, text in _sources(os.path.join(PKG, "csrc"), (".hip", ".cpp", ".h")):
        names.update(re.findall(r'getenv\(\s*"(%s)"' % NAME, text))
    for _, text in _sources(os.path.join(PKG, "pixsfm_amd"), (".py",)):
        if "os.environ" in text or "os.getenv" in text:      # (a name may reach os.environ through a variable: take every literal)
            names.update(re.findall(r'["\'](%s)["\']' % NAME, text))
    return names


def _documented():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = text[text.index("### Environment switches"):]
    table = table[:table.index("\n## ")]
    rows = [line for line in table.splitlines() if line.startswith("|")]
    return set(re.findall(NAME, "\n".join(rows)))


def test_every_switch_the_product_reads_is_in_the_environment_table():
    read = _read_by_the_product()
    assert len(read) > 10, "the search found too little: %s" % sorted(read)
    missing = sorted(read - _documented())
    assert not missing, "read by the library but not in INTEGRATION.md's environment table: %s" % missing


def _set_by_tests_and_tools():
    found = {}
    patterns = [r'(?:setenv|delenv)\(\s*["\'](%s)["\']' % NAME,                       # monkeypatch
                r'os\.environ\[\s*["\'](%s)["\']\s*\]\s*=' % NAME,                     # os.environ["X"] = ...
                r'os\.environ\.(?:setdefault|pop)\(\s*["\'](%s)["\']' % NAME,
                r'env\s*=\s*(?:dict\()?[^\n]*?\b(%s)\s*=' % NAME,                      # env=dict(os.environ, X=...)
                r'["\'](%s)["\']\s*:' % NAME,                                          # {"X": ...} of an env= dict
                r'(?:^|[\s;(])(?:export\s+)?(%s)=' % NAME]                             # shell: X=1 command
    for top, exts in ((os.path.join(ROOT, "tests"), (".py", ".sh")), (os.path.join(ROOT, "tools"), (".py", ".sh"))):
        for path, text in _sources(top, exts):
            for pat in patterns:
                for name in re.findall(pat, text, flags=re.M):
                    found.setdefault(name, os.path.relpath(path, ROOT))
    return found


def test_no_test_or_tool_sets_a_switch_that_nothing_reads():
    read = _read_by_the_product()
    bench = set(re.findall(r'["\'](PXR_BENCH_[A-Z0-9_]+)["\']', open(os.path.join(ROOT, "bench.py")).read()))
    ghosts = {n: where for n, where in _set_by_tests_and_tools().items() if n not in read and n not in bench}
    assert not ghosts, "set by a test or tool, read by nothing (a deleted switch?): %s" % ghosts
