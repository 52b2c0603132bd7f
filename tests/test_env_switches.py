"""The library's environment switches are the documented ones.

Every MMC_* name the native sources read with getenv appears in INTEGRATION.md's "Environment
switches" paragraph, and the move driver's former switches -- duplicates of options, and knobs of
experiments whose results are written down -- are gone from the package, the scripts and that
document."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "metropolismontecarlo_amd")
REMOVED = ("MMC_DEVICE_ACCEPT", "MMC_HOST_ACCEPT", "MMC_STEPS_PER_LAUNCH", "MMC_RUN_AHEAD", "MMC_LAUNCH_AT",
           "MMC_TAIL_DIV", "MMC_NO_PRELAUNCH")
TEXT = (".py", ".hip", ".hpp", ".inc", ".h", ".jl", ".sh", ".md", ".txt", ".json", ".c")


def _read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def _files(top):
    if os.path.isfile(top):
        yield top
        return
    for d, _, names in os.walk(top):
        for n in names:
            if n.endswith(TEXT):
                yield os.path.join(d, n)


def _switches_paragraph():
    text = _read(os.path.join(ROOT, "INTEGRATION.md"))
    start = text.index("**Environment switches**")
    end = text.find("\n\n", start)
    return text[start:] if end < 0 else text[start:end]


def test_every_getenv_name_is_documented():
    names = set()
    for path in _files(os.path.join(PKG, "csrc")):
        names |= set(re.findall(r'getenv\(\s*"(MMC_[A-Z0-9_]+)"', _read(path)))
    assert "MMC_RUN_TRACE" in names and "MMC_POOL_BLOCKTIME_US" in names, sorted(names)   # (the search finds them)
    documented = set(re.findall(r"\bMMC_[A-Z0-9_]+\b", _switches_paragraph()))
    assert not names - documented, sorted(names - documented)


def test_removed_driver_switches_are_gone():
    found = []
    for top in (PKG, os.path.join(ROOT, "scripts"), os.path.join(ROOT, "INTEGRATION.md")):
        for path in _files(top):
            text = _read(path)
            found += [(os.path.relpath(path, ROOT), n) for n in REMOVED
                      if re.search(r"\b%s\b" % n, text)]   # (\b: MMC_STEPS_PER_LAUNCH_MAX is a constant, not a switch)
    assert not found, found
