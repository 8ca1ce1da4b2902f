"""The many-to-many inner join by the option "mm_heavy_keys" - and the all-copies outer joins by "mm_heavy_outer" - on device tensors, fixed seeds:
  a0 / a1   6M build rows over 3M ids x 5M probe rows (no partition beyond 4096 build rows) with the option 0 / 1
  b         one build key with 100 000 copies among 200 000 background rows, met by 50 probe rows of that key (about a's pair count)
  c         1M build rows with Zipf(1) key frequencies x 1500 probe rows of the same distribution
A case name with the suffix .left or .full (a0.full, b.left, c.full, ...) runs left_join / full_join(duplicates="all") on the same input
with "mm_heavy_outer" in the place of "mm_heavy_keys"; "rows" is then P + u + r and "pairs" P.  The yardstick of an outer case is the inner
case of the same input in the same invocation (the untiled outer joins cost 1.06-1.35x their inner join, EXPERIMENTS.md).
Per run: join_ms (counting launches), emit_ms (the writing pass), total_ms and pairs/s of the emitting pass and of the whole join.
Every case is a child process under its own time limit; the first failure ends the tool.
    python tools/mm_heavy.py [cases, default a0,a1,b,c] [runs, default 5]
    python tools/mm_heavy.py b,b.left,b.full,c,c.left,c.full
    FJ_LIB_VARIANT=<name> python tools/mm_heavy.py a0     # the same on lib/ab/<name>.so (a same-box A/B)"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = -7046029254386353131           # 0x9E3779B97F4A7C15 as int64
LIMITS = {"a0": 300, "a1": 300, "b": 300, "c": 300}


def case_inputs(name):
    import numpy as np
    import torch
    if name in ("a0", "a1"):
        rng = np.random.default_rng(6_000_007)
        bk = rng.integers(0, 3_000_000, size=6_000_000, dtype=np.int64) * np.int64(GOLDEN)
        pk = rng.integers(0, 6_000_001, size=5_000_000, dtype=np.int64) * np.int64(GOLDEN)
    elif name == "b":
        rng = np.random.default_rng(2024)
        bk = np.concatenate([np.full(100_000, 77777, dtype=np.int64), rng.integers(10, 50_010, size=200_000, dtype=np.int64) * np.int64(GOLDEN)])
        rng.shuffle(bk)
        pk = np.concatenate([np.full(50, 77777, dtype=np.int64), rng.integers(10, 100_010, size=30_000, dtype=np.int64) * np.int64(GOLDEN)])
        rng.shuffle(pk)
    else:
        rng = np.random.default_rng(99)
        cdf = np.cumsum(1.0 / np.arange(1, 1_000_001))
        cdf /= cdf[-1]
        bk = (np.searchsorted(cdf, rng.random(1_000_000)) + 1).astype(np.int64) * np.int64(GOLDEN)
        pk = (np.searchsorted(cdf, rng.random(1500)) + 1).astype(np.int64) * np.int64(GOLDEN)
    bv = np.arange(bk.size, dtype=np.int64)
    return tuple(torch.from_numpy(x).cuda() for x in (bk, bv, pk))


def run_case(name, runs):
    sys.path.insert(0, ROOT)
    import flash_join
    flash_join.initialize()
    base, _, form = name.partition(".")
    bk, bv, pk = case_inputs(base)
    try:
        flash_join.set_option("mm_heavy_outer" if form else "mm_heavy_keys", 0 if base == "a0" else 1)
    except RuntimeError:                 # a library from before the option: case a0 is what it can run
        assert name == "a0", name
    if form:                                                                  # the outer forms: (P, u[, r], seconds)
        fn = flash_join.left_join if form == "left" else flash_join.full_join
        join = lambda: fn(bk, bv, pk, duplicates="all")
    else:
        join = lambda: flash_join.inner_join(bk, bv, pk)
    n_count = flash_join.inner_join_count(bk, bv, pk)[0] if not form else join()[0]
    join()                                                                    # warm-up: workspace, kernel attributes
    for r in range(runs):
        res = join()
        n, rows = res[0], sum(res[:-1])
        t = flash_join.last_timings()
        assert n == n_count, (n, n_count)
        print(json.dumps({"case": name, "run": r, "lib": os.environ.get("FJ_LIB_VARIANT", "") or "in-tree", "nb": bk.numel(), "np": pk.numel(),
                          "pairs": n, "rows": rows, "join_ms": round(t["join_ms"], 4), "emit_ms": round(t["emit_ms"], 4), "total_ms": round(t["total_ms"], 4),
                          "lds_retries": t["lds_retries"], "emit_gpairs_s": round(n / t["emit_ms"] / 1e6, 3) if t["emit_ms"] > 0 else None,
                          "emit_write_gb_s": round(16 * n / t["emit_ms"] / 1e6, 1) if t["emit_ms"] > 0 else None,
                          "total_gpairs_s": round(n / t["total_ms"] / 1e6, 3)}), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--case":
        run_case(sys.argv[2], int(sys.argv[3]))
        return 0
    cases = sys.argv[1].split(",") if len(sys.argv) > 1 else ["a0", "a1", "b", "c"]
    runs = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    for name in cases:
        base, _, form = name.partition(".")
        if base not in LIMITS or form not in ("", "left", "full"):
            print(f"unknown case {name!r} (a0, a1, b, c, each also with .left or .full)", file=sys.stderr)
            return 2
        rc = subprocess.call(["timeout", "-k", "10", str(LIMITS[base]), sys.executable, os.path.abspath(__file__), "--case", name, str(runs)], cwd=ROOT)
        if rc != 0:
            print(f"case {name}: exit status {rc}; stopping", file=sys.stderr)
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
