"""Device and pinned host memory has one owner, bppo::DeviceMem (burn-ppo_amd/csrc/
bppo_internal.h): the raw HIP allocation calls appear there and in
the shuffle engine, which keeps its own buffers and shutdown order, and nowhere else.  The
hand-kept helpers and error macros the owner replaced do not come back."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "burn-ppo_amd", "csrc")

RAW = re.compile(r"\b(?:hipMalloc|hipFree|hipHostMalloc|hipHostFree)\b")
GONE = re.compile(r"\b(?:dalloc|walloc|oalloc|WHIP|WTRY|PHIP|CHIP)\b")


def _sources():
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        with open(path, encoding="utf-8") as f:
            yield os.path.basename(path), f.read()


def test_raw_allocation_calls_only_in_the_owner_and_the_engine():
    hits = {fname: n for fname, text in _sources() if (n := len(RAW.findall(text)))}
    # the owner and the engine, any count
    assert hits.pop("bppo_internal.h", 0) > 0
    assert hits.pop("shuffle_engine.hip", 0) > 0
    # the static stamp buffers of the two diagnostic builds (#ifdef BPPO_RO_STAMPS /
    # BPPO_MB_STAMPS): allocated once per process, never freed, not in a default build
    assert hits == {"k_rollout.hip": 1, "k_update.hip": 1}, hits
    for fname, macro in (("k_rollout.hip", "BPPO_RO_STAMPS"), ("k_update.hip", "BPPO_MB_STAMPS")):
        text = dict(_sources())[fname]
        site = RAW.search(text).start()
        opened = text.rfind("#ifdef " + macro, 0, site)
        assert opened >= 0 and "#endif" not in text[opened:site], f"{fname}: the raw call is outside #ifdef {macro}"


def test_the_replaced_helpers_and_macros_are_gone():
    hits = [(fname, sorted(set(GONE.findall(text)))) for fname, text in _sources() if GONE.search(text)]
    assert not hits, hits
