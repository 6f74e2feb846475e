#!/usr/bin/env python3
"""Write tests/golden/ratings_ref.json: the restatement's (tests/pl_ref.py) result on every
rating fixture and the spread of its own outputs over 8 random orderings of the same games.
The GPU tests read the file instead of spending ~25 s of pure Python on every run;
tests/test_ratings_ref.py checks the file against the restatement (every reference result, and
the spreads of the fixtures that are cheap to recompute).  Run it after changing a fixture."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pl_ref  # noqa: E402


def record(name):
    r = pl_ref.reference(name)
    return {"rating": [x[0] for x in r.ratings], "uncertainty": [x[1] for x in r.ratings], "gamma": r.gammas,
            "converged": r.converged, "iterations_used": r.iterations_used, "final_delta": r.final_delta,
            "previous_delta": r.deltas[-2] if len(r.deltas) > 1 else None, "n_comparisons": r.n_comparisons,
            "spread": pl_ref.order_spread(name)}


if __name__ == "__main__":
    out = {name: record(name) for name in pl_ref.FIXTURES}
    path = os.path.join(ROOT, "tests", "golden", "ratings_ref.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for name, rec in out.items():
        print(name, rec["iterations_used"], rec["final_delta"], rec["spread"])
