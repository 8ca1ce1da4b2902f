"""group_by_agg (count, sum, min and max of a column in ONE call: FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ALL) against the composition it
replaces - group_by_count + group_by_sum + group_by_min + group_by_max, with and without the three alignments by key
(api._align_by_key: two argsorts of g keys each) - and against one group_by_sum, on device tensors.  One process, the forms
ALTERNATING round by round, so that whatever else shares the box touches every form alike; per form the median, the minimum and the
maximum over the timed rounds of (a) the wall time of the synchronised call and (b) the device time the library reports (the sum over
the calls of a composition; it does not contain the alignment, which is torch's).  One JSON line per form and value type, appended to
--out; before timing, the single call's columns are compared with the composition's, aligned by key (integers: equal; floats: the
"exact" value domain - multiples of 2^-10 below 2^10 - so equal too).

    python tools/group_by_agg_ab.py [--rows 100000000] [--distinct 1000000] [--rounds 7] [--warmup 2] [--out profiles/group_by_agg_ab.jsonl]

The bar is "four_calls" (no alignment): the single call must come in under it by more than the spread of the repeated rounds."""
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
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--distinct", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_by_agg_ab.jsonl"))
    args = ap.parse_args()
    assert args.rounds >= 5, "the median of at least 5 timed rounds"
    import torch
    import flash_join
    from flash_hash_join_amd import api
    flash_join.initialize()
    n, g = args.rows, args.distinct
    dev = "cuda:0"
    keys = torch.randint(0, g, (n,), dtype=torch.int64, device=dev)
    keys[:g] = torch.arange(g, dtype=torch.int64, device=dev)                    # every key occurs
    keys *= SPREAD
    columns = {"int64": (torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev), {}),
               "float64": (torch.randint(-2**20, 2**20, (n,), dtype=torch.int64, device=dev).to(torch.float64) * 2.0**-10, {"float64": True})}
    out = open(args.out, "a")
    for vtype, (vals, kw) in columns.items():
        def single():
            r = flash_join.group_by_agg(keys, vals, **kw)
            return r[0], r[1], r

        def single_bounded():
            r = flash_join.group_by_agg(keys, vals, max_groups=g, **kw)
            return r[0], r[1], r

        def four(align):
            g0, s0, k0, c0 = flash_join.group_by_count(keys)
            g1, s1, k1, v1 = flash_join.group_by_sum(keys, vals, **kw)
            g2, s2, k2, v2 = flash_join.group_by_min(keys, vals, **kw)
            g3, s3, k3, v3 = flash_join.group_by_max(keys, vals, **kw)
            assert g0 == g1 == g2 == g3
            if align:
                v1, v2, v3 = api._align_by_key(k0, k1, v1), api._align_by_key(k0, k2, v2), api._align_by_key(k0, k3, v3)
            return g0, s0 + s1 + s2 + s3, (g0, 0.0, k0, c0, v1, v2, v3)

        def one_sum():
            r = flash_join.group_by_sum(keys, vals, **kw)
            return r[0], r[1], r

        forms = [("group_by_agg", single), ("group_by_agg_max_groups", single_bounded), ("four_calls", lambda: four(False)),
                 ("four_calls_aligned", lambda: four(True)), ("group_by_sum", one_sum)]
        # results first: the single call's columns equal the aligned composition's
        a, b = single()[2], four(True)[2]
        assert a[0] == b[0] == g, (a[0], b[0], g)
        oa, ob = torch.argsort(a[2]), torch.argsort(b[2])
        assert torch.equal(a[2][oa], b[2][ob]), "keys"
        for j, name in enumerate(("count", "sum", "min", "max")):
            assert torch.equal(a[3 + j][oa], b[3 + j][ob]), (vtype, name)
        del a, b, oa, ob
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
                assert gg == g
                plans[name] = {k: flash_join.last_timings()[k] for k in KEEP}     # (of the form's last library call)
                del r
                if i >= args.warmup:
                    wall[name].append((t1 - t0) * 1e3)
                    devt[name].append(sec * 1e3)
        for name, _ in forms:
            line = json.dumps({"rows": n, "distinct": g, "values": vtype, "name": name, "rounds": args.rounds,
                               "wall_median_ms": round(statistics.median(wall[name]), 3), "wall_min_ms": round(min(wall[name]), 3),
                               "wall_max_ms": round(max(wall[name]), 3), "device_median_ms": round(statistics.median(devt[name]), 3),
                               "device_min_ms": round(min(devt[name]), 3), "device_max_ms": round(max(devt[name]), 3),
                               "last_call": plans[name]})
            print(line, flush=True)
            out.write(line + "\n")
        out.flush()
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
