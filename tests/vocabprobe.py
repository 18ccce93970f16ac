"""Whole-job probe of the flights-shaped vocabulary pipeline (GPU box):
tests/vocab_pipelines.py's csv file at N rows through the public API,
ctx.csv(path) ... collect(), timed from the call to the last row in Python.

Usage: python tests/vocabprobe.py [rows_millions] [runs] [package_root]

package_root names another checkout whose tuplex_amd is timed on the same file
(one without these UDF forms takes the interpreter fallback: mode "fallback").
Prints one JSON line per run; the first run of a process also loads the
kernels."""
import json
import os
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def main():
    mrows = float(sys.argv[1]) if len(sys.argv) > 1 else 1.0
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 2
    pkg_root = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else ROOT
    sys.path.insert(0, pkg_root)
    import tuplex_amd  # the package under test first, then this tree's tests
    assert os.path.dirname(os.path.dirname(os.path.abspath(
        tuplex_amd.__file__))) == pkg_root, tuplex_amd.__file__
    sys.path.insert(0, ROOT)
    from tests import vocab_pipelines as V
    from tests.pipelines import apply_ops

    n = int(mrows * 1e6)
    data = V.make_flights_vocab_csv(n)
    ops = V.flights_vocab_ops()
    with tempfile.TemporaryDirectory() as d:
        p = os.path.join(d, "flights_vocab.csv")
        with open(p, "wb") as f:
            f.write(data)
        for run in range(runs):
            ctx = tuplex_amd.Context()
            t0 = time.perf_counter()
            ds = apply_ops(ctx.csv(p), ops)
            got = ds.collect()
            wall = time.perf_counter() - t0
            print(json.dumps({
                "package": pkg_root, "run": run, "rows_in": n,
                "mb": round(len(data) / 1e6, 1), "rows_out": len(got),
                "exceptions": sum(ds.exception_counts.values()),
                "mode": ds._last_outcome.mode,
                "why": ds._last_outcome.fallback_reason,
                "wall_s": round(wall, 3),
                "rows_per_s": round(n / wall)}), flush=True)


if __name__ == "__main__":
    main()
