"""The fused full outer join on device tensors against what a caller composes without it: left_join(B, V, P) followed by
anti_join(P, B) (roles swapped), same inputs, same process; and the plain left join of the same inputs beside both (its kernel is
the one the full outer join extends: run this under two builds of the library to compare it across them).

    python tools/full_join_probe.py [--nb 50000000] [--ratio 10] [--unprobed 0.2] [--steps 7] [--warmup 2] [--only left]

Shape: the benchmark's (build : probe = 1 : ratio, half the probe rows hitting), with a known share of the build side never probed:
the build rows are ids 1..lo and 10^9+1..10^9+hi (datagen), the probe side draws from ids 1..lo (hits) and lo+1..2lo (misses).
Device time is last_timings()["total_ms"] of every call, summed for the composition.  The steps of the contenders are interleaved
(fused, composition, left, fused, ...) so that clock and temperature drift hits all alike.  One JSON line per contender: median,
min, max, interquartile range in ms; the last line carries the ratio fused / composition."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=50_000_000)
    ap.add_argument("--ratio", type=int, default=10)
    ap.add_argument("--unprobed", type=float, default=0.2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="", help="'left': the plain left join alone (a build of the library without the full outer join)")
    args = ap.parse_args()
    import torch
    import flash_join
    from flash_hash_join_amd import datagen
    flash_join.initialize()
    hi = int(args.nb * args.unprobed)
    lo = args.nb - hi
    n_p = args.nb * args.ratio
    k1, v1 = datagen.build_device(lo, "cuda:0")
    k2, v2 = datagen.build_device(hi, "cuda:0", first=10**9)
    bk, bv = torch.cat([k1, k2]), torch.cat([v1, v2])
    del k1, k2, v1, v2
    pk, expected = datagen.probe_device(n_p, lo, "cuda:0", seed=1, hit_bp=5000)
    ms = lambda: flash_join.last_timings()["total_ms"]

    def fused():
        m, r, _ = flash_join.full_join(bk, bv, pk)
        assert m == expected and r >= hi, (m, expected, r, hi)
        fused.timings = flash_join.last_timings()
        return ms(), r

    def composition():
        m, _ = flash_join.left_join(bk, bv, pk)
        t = ms()
        u, _ = flash_join.anti_join(pk, bk)
        assert m == expected and u >= hi, (m, expected, u, hi)
        return t + ms(), u

    def left():
        m, _ = flash_join.left_join(bk, bv, pk)
        assert m == expected
        return ms(), 0

    runs = {"left_join": left} if args.only == "left" else {"full_join": fused, "left_join+anti_join": composition, "left_join": left}
    times = {name: [] for name in runs}
    rest = {}
    for i in range(args.warmup + args.steps):
        for name, fn in runs.items():
            t, r = fn()
            torch.cuda.synchronize()
            rest[name] = r
            if i >= args.warmup:
                times[name].append(t)
    assert args.only or rest["full_join"] == rest["left_join+anti_join"], rest
    out = {}
    for name, ts in times.items():
        q = statistics.quantiles(ts, n=4) if len(ts) >= 4 else [min(ts), statistics.median(ts), max(ts)]
        out[name] = statistics.median(ts)
        print(json.dumps({"function": name, "nb": args.nb, "np": n_p, "unprobed_build_rows": rest[name], "steps": len(ts),
                          "median_ms": round(out[name], 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3),
                          "iqr_ms": round(q[2] - q[0], 3), "lib_variant": os.environ.get("FJ_LIB_VARIANT", "")}), flush=True)
    if not args.only:
        print(json.dumps({"fused_over_composition": round(out["full_join"] / out["left_join+anti_join"], 4),
                          "last_full_join_timings": {k: v for k, v in fused.timings.items() if k != "probe_part_kernel_ms"}}), flush=True)


if __name__ == "__main__":
    main()
