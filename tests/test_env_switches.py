"""The runtime switches libbppo.so reads and the ones DESIGN.md section 6 documents are
the same set: a new switch cannot land without a documented reason, and a documented
switch cannot outlive its code.  Every switch is read through env_set / env_int
(burn-ppo_amd/csrc/bppo_internal.h), so their string literals are the switches."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "burn-ppo_amd", "csrc")

CALL = re.compile(r"\benv_(?:set|int)\(\s*([^,)]*)")
HELPER_DEF = "const char *name"      # the two definitions, the only calls without a literal


def _sources():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(path, encoding="utf-8") as f:
            yield os.path.basename(path), f.read()


def _switches_read():
    names = set()
    for fname, text in _sources():
        for arg in CALL.findall(text):
            if arg.strip() == HELPER_DEF:
                assert fname == "bppo_internal.h"
                continue
            m = re.fullmatch(r'"(BPPO_[A-Z0-9_]+)"', arg.strip())
            assert m, f"{fname}: env_set / env_int takes a BPPO_* string literal, got {arg!r}"
            names.add(m.group(1))
    return names


def _switches_documented():
    with open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8") as f:
        text = f.read()
    table = text[text.index("**Runtime switches**"):]
    rows = []
    for line in table.splitlines()[1:]:
        if line.startswith("|"):
            rows.append(line)
        elif rows:
            break                     # the table's end
    names = [m.group(1) for m in (re.match(r"\|\s*`(BPPO_[A-Z0-9_]+)`\s*\|", r) for r in rows) if m]
    assert len(names) == len(set(names)), "a switch has two rows"
    return set(names)


def test_switches_read_are_the_switches_documented():
    read, documented = _switches_read(), _switches_documented()
    assert read and read == documented, (
        f"read but not in DESIGN.md section 6: {sorted(read - documented)}; "
        f"documented but not read: {sorted(documented - read)}")


def test_getenv_only_in_the_two_helpers():
    hits = [(fname, n) for fname, text in _sources() if (n := len(re.findall(r"\bgetenv\b", text)))]
    assert hits == [("bppo_internal.h", 2)], hits
