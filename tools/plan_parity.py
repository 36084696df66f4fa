"""csrc/plan_host (the spline planner's CPU build, csrc/spline_plan.h) against scipy's splprep / splev over the
pinned sample of tests/plan_cases.py: knot counts, knot values, and the coefficient / sample differences whose
maximum sets the tests' tolerance (ten times it).  No GPU.

    python tools/plan_parity.py [--cases 4000] [--out profiles/plan_parity.json]
"""
import argparse
import collections
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import plan_cases as P  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=P.SAMPLE_SIZE)
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    start, gates = P.sample(a.cases)
    with tempfile.TemporaryDirectory() as tmp:
        got = P.run_plan_host(start, gates, tmp)
    want = P.scipy_plan(start, gates)
    same_n = got["n"] == want["n"]
    dc = np.abs(got["c"] - want["c"]).reshape(a.cases, -1).max(1)
    dr = np.abs(got["ref"] - want["ref"]).reshape(a.cases, -1).max(1)
    dt = np.abs(got["t"] - want["t"]).reshape(a.cases, -1).max(1)
    ok = same_n
    res = {
        "cases": a.cases,
        "knot_count_equal": int(same_n.sum()),
        "knot_counts": {str(k): int(v) for k, v in sorted(collections.Counter(want["n"].tolist()).items())},
        "status_nonzero_flags": int(((got["status"] & 3) != 0).sum()),
        "p_iterations": {str(k): int(v) for k, v in sorted(collections.Counter(((got["status"] >> 16) & 255).tolist()).items())},
        "knot_value_max_abs": float(dt[ok].max()),
        "coef_max_abs": float(dc[ok].max()), "coef_p99_abs": float(np.percentile(dc[ok], 99)),
        "sample_max_abs": float(dr[ok].max()), "sample_p99_abs": float(np.percentile(dr[ok], 99)),
        "worst_case": int(np.argmax(np.where(ok, np.maximum(dc, dr), -1.0))),
    }
    res["max_abs"] = max(res["coef_max_abs"], res["sample_max_abs"])
    res["p99_abs"] = max(res["coef_p99_abs"], res["sample_p99_abs"])
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    main()
