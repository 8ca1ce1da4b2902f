"""group_by_argmin (the row that holds each group's minimum, ONE call: FJ_ALGO_GROUP_BY | FJ_ALGO_AGG_ARG | FJ_ALGO_AGG_MIN) against the
composition it replaces and against its floor, on device tensors:

    group_by_argmin          the row indices alone
    group_by_argmin_values   ... with return_values=True (the same library call: the second plane is sliced as well)
    group_by_min             ONE call of the single form - the floor: the same plan minus the positions, the value gather and the
                             resolve phase.  The difference to it is what those cost.
    three_calls              group_by_min, lookup of that minimum back onto every row and a compare, a second group_by_min over the
                             surviving rows' positions, and the alignment of the positions with the first call's keys
                             (api._align_by_key: two argsorts of g keys)
    hot_key_argmin           for information: group_by_argmin where one key owns 10 % of the rows (one workgroup streams it, twice)

One process, the forms ALTERNATING round by round, so that whatever else shares the box touches every form alike; per form the median,
the minimum and the maximum over the timed rounds of (a) the wall time of the synchronised call and (b) the device time the library
reports (the sum over the calls of the composition; it does not contain the compare, the compaction and the alignment, which are
torch's).  One JSON line per form and value type, appended to --out; before timing, the single call's row indices are compared with the
composition's, aligned by key (random 64-bit integers: no ties; floats from the "exact" domain - multiples of 2^-10 below 2^10, no -0.0 -
tie often, and both sides keep the smallest position).

    python tools/group_by_arg_ab.py [--rows 100000000] [--distinct 1000000] [--rounds 7] [--warmup 2] [--out profiles/group_by_arg_ab.jsonl]
"""
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
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_by_arg_ab.jsonl"))
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
    hot = keys.clone()
    hot[torch.randperm(n, device=dev)[:n // 10]] = 12345                         # one key owns 10 % of the rows
    g_hot = int(torch.unique(hot).numel())
    keys *= SPREAD
    hot *= SPREAD
    columns = {"int64": (torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=dev), {}),
               "float64": (torch.randint(-2**20, 2**20, (n,), dtype=torch.int64, device=dev).to(torch.float64) * 2.0**-10, {"float64": True})}
    out = open(args.out, "a")
    for vtype, (vals, kw) in columns.items():
        def argmin(k=keys, **more):
            r = flash_join.group_by_argmin(k, vals, **kw, **more)
            return r[0], r[1], r

        def one_min():
            r = flash_join.group_by_min(keys, vals, **kw)
            return r[0], r[1], r

        def three():
            g1, s1, k1, m1 = flash_join.group_by_min(keys, vals, **kw)
            words = lambda t: t.view(torch.int64)
            _, s2, rowmin = flash_join.lookup(k1, words(m1), keys)               # every key is among k1
            rows = torch.nonzero(rowmin.view(vals.dtype) == vals).reshape(-1)    # the rows that hold their group's minimum
            g3, s3, k3, p3 = flash_join.group_by_min(keys[rows], rows, signed=True)
            assert g1 == g3
            return g1, s1 + s2 + s3, (g1, 0.0, k1, api._align_by_key(k1, k3, p3))

        forms = [("group_by_argmin", lambda: argmin()), ("group_by_argmin_values", lambda: argmin(return_values=True)),
                 ("group_by_min", one_min), ("three_calls", three), ("hot_key_argmin", lambda: argmin(hot))]
        expect = {name: g for name, _ in forms}
        expect["hot_key_argmin"] = g_hot
        # results first: the single call's row indices equal the composition's, and gather the minima
        a, b = argmin(return_values=True)[2], three()[2]
        assert a[0] == b[0] == g, (a[0], b[0], g)
        oa, ob = torch.argsort(a[2]), torch.argsort(b[2])
        assert torch.equal(a[2][oa], b[2][ob]), "keys"
        assert torch.equal(a[3][oa], b[3][ob]), (vtype, "row_index")
        assert torch.equal(keys[a[3]], a[2]) and torch.equal(vals[a[3]], a[4]), (vtype, "gather")
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
                assert gg == expect[name], (name, gg)
                plans[name] = {k: flash_join.last_timings()[k] for k in KEEP}     # (of the form's last library call)
                del r
                if i >= args.warmup:
                    wall[name].append((t1 - t0) * 1e3)
                    devt[name].append(sec * 1e3)
        for name, _ in forms:
            line = json.dumps({"rows": n, "distinct": expect[name], "values": vtype, "name": name, "rounds": args.rounds,
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
