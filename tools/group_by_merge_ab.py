"""group_by_merge (partial group-by results combined in ONE call: FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL | FJ_ALGO_AGG_MERGE) and the
GroupByAccumulator on top of it against the composition a user had before: factorize of the concatenated keys plus four torch scatters
over the codes (index_add_ twice, scatter_reduce_ "amin" and "amax").  Device tensors, one process, the forms ALTERNATING round by
round, so that whatever else shares the box touches every form alike; per form the median, the minimum and the maximum over the timed
rounds of the wall time of the synchronised form, and of the device time the library reports for its own calls (the bar's does not
contain torch's cat and scatters).  One JSON line per workload, value type and form, appended to --out.  Before timing, both forms
are compared column by column, aligned by key (floats: multiples of 2^-10 below 2^10, so their sums are exact in any order).

Workloads:
  same_keys    --batches partials of --groups groups each over the SAME keys
  disjoint     --batches partials of --groups groups each over DISJOINT keys
  accumulator  a relation of --rows rows over --groups keys fed to a GroupByAccumulator in --batches batches (update + result), against
               the bar (group_by_agg per batch, then the composition) and against ONE group_by_agg of the whole relation - the floor

    python tools/group_by_merge_ab.py [--groups 1000000] [--batches 8] [--rows 100000000] [--rounds 7] [--warmup 2] [--out profiles/group_by_merge_ab.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SPREAD = 0x9E3779B97F4A7C15 - 2**64          # an odd multiplier: i -> i * SPREAD is one-to-one modulo 2^64 (int64 storage)
KEEP = ("total_ms", "build_phase_ms", "join_ms", "path", "passes", "radix_bits", "fell_back", "partitions")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=1_000_000)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workloads", default="same_keys,disjoint,accumulator")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_by_merge_ab.jsonl"))
    args = ap.parse_args()
    assert args.rounds >= 5, "the median of at least 5 timed rounds"
    import torch
    import flash_join
    flash_join.initialize()
    g, nbatch, dev = args.groups, args.batches, "cuda:0"
    i64 = torch.int64

    def values(n, vtype):
        if vtype == "float64":
            return torch.randint(-2**20, 2**20, (n,), dtype=i64, device=dev).to(torch.float64) * 2.0**-10
        return torch.randint(-2**63, 2**63 - 1, (n,), dtype=i64, device=dev)

    def bar(parts, vtype):
        """the composition: one trip for the codes, then four scattered passes over them"""
        keys, counts, sums, mins, maxs = (torch.cat([p[j] for p in parts]) for j in range(5))
        gg, sec, codes, uniques = flash_join.factorize(keys)
        lo, hi = (float("-inf"), float("inf")) if vtype == "float64" else (-2**63, 2**63 - 1)
        c = torch.zeros(gg, dtype=i64, device=dev).index_add_(0, codes, counts)
        s = torch.zeros(gg, dtype=sums.dtype, device=dev).index_add_(0, codes, sums)
        mn = torch.full((gg,), hi, dtype=mins.dtype, device=dev).scatter_reduce_(0, codes, mins, "amin")
        mx = torch.full((gg,), lo, dtype=maxs.dtype, device=dev).scatter_reduce_(0, codes, maxs, "amax")
        return gg, sec, (gg, sec, uniques, c, s, mn, mx)

    def same(a, b, what):
        assert a[0] == b[0], (what, a[0], b[0])
        oa, ob = torch.argsort(a[2]), torch.argsort(b[2])
        assert torch.equal(a[2][oa], b[2][ob]), (what, "keys")
        for j, name in enumerate(("count", "sum", "min", "max")):
            assert torch.equal(a[3 + j][oa], b[3 + j][ob]), (what, name)

    def measure(workload, vtype, forms, want_g, extra):
        plans = {}
        wall = {name: [] for name, _ in forms}
        devt = {name: [] for name, _ in forms}
        for i in range(args.warmup + args.rounds):
            for name, fn in forms:                                                # alternating: every round runs every form once
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gg, sec, r = fn()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                assert gg == want_g, (name, gg, want_g)
                plans[name] = {k: flash_join.last_timings()[k] for k in KEEP}     # (of the form's last library call)
                del r
                if i >= args.warmup:
                    wall[name].append((t1 - t0) * 1e3)
                    devt[name].append(sec * 1e3)
        with open(args.out, "a") as out:
            for name, _ in forms:
                line = json.dumps({"workload": workload, "values": vtype, "name": name, "rounds": args.rounds, **extra,
                                   "wall_median_ms": round(statistics.median(wall[name]), 3), "wall_min_ms": round(min(wall[name]), 3),
                                   "wall_max_ms": round(max(wall[name]), 3), "device_median_ms": round(statistics.median(devt[name]), 3),
                                   "device_min_ms": round(min(devt[name]), 3), "device_max_ms": round(max(devt[name]), 3),
                                   "last_call": plans[name]})
                print(line, flush=True)
                out.write(line + "\n")
        torch.cuda.empty_cache()

    for workload in [w for w in args.workloads.split(",") if w in ("same_keys", "disjoint")]:
        for vtype in ("int64", "float64"):
            kw = {"float64": True} if vtype == "float64" else {"signed": True}
            parts = []
            for b in range(nbatch):
                base = b * g if workload == "disjoint" else 0
                keys = (torch.randperm(g, dtype=i64, device=dev) + base) * SPREAD
                v1, v2 = values(g, vtype), values(g, vtype)
                sums = (v1 + v2) if vtype == "float64" else v1                    # (an int64 sum wraps: any word will do)
                parts.append((keys, torch.randint(1, 1000, (g,), dtype=i64, device=dev), sums, torch.minimum(v1, v2), torch.maximum(v1, v2)))
            want_g = g * nbatch if workload == "disjoint" else g

            def merged():
                r = flash_join.group_by_merge(*[[p[j] for p in parts] for j in range(5)], **kw)
                return r[0], r[1], r

            same(merged()[2], bar(parts, vtype)[2], (workload, vtype))
            measure(workload, vtype, [("group_by_merge", merged), ("factorize_and_scatters", lambda: bar(parts, vtype))], want_g,
                    {"partials": nbatch, "rows_per_partial": g})
            del parts

    if "accumulator" in args.workloads.split(","):
        n = args.rows
        keys = torch.randint(0, g, (n,), dtype=i64, device=dev)
        keys[:g] = torch.arange(g, dtype=i64, device=dev)                        # every key occurs
        keys *= SPREAD
        cuts = [n * b // nbatch for b in range(nbatch + 1)]
        for vtype in ("int64", "float64"):
            kw = {"float64": True} if vtype == "float64" else {"signed": True}
            vals = values(n, vtype)
            batches = [(keys[a:b], vals[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]

            def accumulated():
                sec = 0.0
                with flash_join.GroupByAccumulator(**kw) as acc:
                    for k, v in batches:
                        sec += acc.update(k, v)[1]
                    r = acc.result()
                return r[0], sec + r[1], r

            def batches_then_bar():
                parts, sec = [], 0.0
                for k, v in batches:
                    r = flash_join.group_by_agg(k, v, **kw)
                    sec += r[1]
                    parts.append(r[2:])
                gg, s2, r = bar(parts, vtype)
                return gg, sec + s2, r

            def whole():
                r = flash_join.group_by_agg(keys, vals, **kw)
                return r[0], r[1], r

            a = accumulated()[2]
            same(a, batches_then_bar()[2], ("accumulator", vtype, "bar"))
            same(a, whole()[2], ("accumulator", vtype, "whole"))
            del a
            measure("accumulator", vtype, [("accumulator", accumulated), ("batches_then_factorize_and_scatters", batches_then_bar),
                                           ("one_group_by_agg", whole)], g, {"rows": n, "batches": nbatch, "distinct": g})
            del vals, batches


if __name__ == "__main__":
    main()
