"""Group-by on one relation (unique / distinct_count / group_by_count / group_by_sum / group_by_min / group_by_max, FJ_ALGO_GROUP_BY)
and its inverse (factorize, FJ_ALGO_INVERSE) on device tensors next to the composition a user runs without them.  One JSON line per
form, appended to --out:

  (a) unique, unique(return_index=True), distinct_count, group_by_count, group_by_sum, group_by_min, group_by_max, factorize,
      factorize followed by zeros(g).index_add_(0, codes, values) (the sums from the ids: one grouping, then any aggregate);
      the float64 aggregates (float64=True) beside their integer forms: group_by_sum_f64 / group_by_min_f64, group_join_sum and
      group_join_sum_f64 (the g distinct keys as the build side), Index.group_sum and Index.group_sum_f64 (an index on them, built
      outside the timed region), and factorize+index_add_f64, the torch composition on a float64 column;
      group_rows (FJ_ALGO_GROUP_ROWS): the rows of every group as a CSR of row indices - group keys, offsets, row_index
  (b) the composition: torch.unique(keys, return_counts=True) (counts), torch.unique(keys, return_inverse=True) alone (the ids), or
      followed by zeros(g).index_add_(0, inverse, values) (sums) / full(g, INT64_MAX).scatter_reduce_(0, inverse, values, "amin")
      (minima) - the wall time of the steps between two device synchronisations;
      the two ways to the CSR of group_rows without it: "factorize+sort+bincount+cumsum" (factorize, a stable torch.sort of the
      codes, bincount and cumsum) and "torch.unique(return_inverse+return_counts)+argsort" (a stable argsort of the inverse, cumsum)

    python tools/group_by_probe.py [--workloads u1m,distinct,hot,b1g] [--forms a,b] [--names factorize,...] [--steps 8] [--warmup 2]
                                   [--out profiles/group_by_probe.jsonl]

Workloads: u1m = 100M rows over 1M distinct keys, uniform; distinct = 100M rows, all distinct; b1g = 1B rows over 100M distinct keys;
hot = 100M rows over 1M keys of which one owns every tenth row.  Two-column keys (not in the default list): p1k = 100M rows over
1000 x 1000 values, p10k = 100M rows over 10 000 x 10 000 values - the lines factorize_columns and "factorize x3 + multiply-add", its
composition from the single-key entry (_pair_workload), and group_by_agg_columns beside "factorize_columns + group_by_agg + 2
gathers", the composition it replaces, the two alternating step by step (_pair_agg_lines).  Times of (a) are device times (core_duration_sec, HIP events); (b) is
torch kernels, so its figure is wall time around a synchronised region, and (a) is reported that way too ("wall_median_ms") so that
the two compare like with like.  "timings" of (a) carry the split: build_phase_ms = the relation's passes, join_ms = the kernel - for
the hot workload the kernel's time is the one long work item's (the hot key's partition)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PAIR_WORKLOADS = {"p1k": (100_000_000, 1000, 1000), "p10k": (100_000_000, 10_000, 10_000)}     # rows, values of column a, values of column b
WORKLOADS = {"u1m": (100_000_000, 1_000_000), "distinct": (100_000_000, 100_000_000), "b1g": (1_000_000_000, 100_000_000), "hot": (100_000_000, 1_000_000)}
KEEP = ("total_ms", "build_phase_ms", "probe_phase_ms", "join_ms", "emit_ms", "path", "passes", "radix_bits", "fell_back")
SPREAD = 0x9E3779B97F4A7C15 - 2**64          # an odd multiplier: i -> i * SPREAD is one-to-one modulo 2^64 (int64 storage)


def _timed(fn, want, steps, warmup):
    """medians of the device time fn reports (r[1]; None: a torch composition) and of the wall time of the synchronised call"""
    import torch
    dev, wall = [], []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        assert r[0] == want, (r[0], want)
        if i >= warmup:
            if r[1] is not None:
                dev.append(r[1] * 1e3)
            wall.append((t1 - t0) * 1e3)
        del r
    return (statistics.median(dev) if dev else None), (min(dev) if dev else None), statistics.median(wall)


def _pair_workload(flash_join, torch, wl, args, out):
    """two-column keys (FJ_ALGO_KEY_PAIR): factorize_columns next to its composition from the single-key entry - factorize(a),
    factorize(b), a multiply-add of the two code columns, a third factorize.  Both report device times (the composition: the sum of
    its three calls); the composition's last call runs factorize's kernel over the very groups factorize_columns finds, so its
    join_ms beside factorize_columns' join_ms is what the pair kernel's position atomics and verification gathers cost."""
    n, na, nb = PAIR_WORKLOADS[wl]
    a = torch.randint(0, na, (n,), dtype=torch.int64, device="cuda:0") * SPREAD
    b = torch.randint(0, nb, (n,), dtype=torch.int64, device="cuda:0") * SPREAD

    def composed():
        ga, s1, ca, _ = flash_join.factorize(a)
        gb, s2, cb, _ = flash_join.factorize(b)
        g, s3, codes, _ = flash_join.factorize(ca * gb + cb)
        return g, s1 + s2 + s3, codes

    g = composed()[0]                                                         # the two forms check each other's group count
    runs = [("a", "factorize_columns", lambda: flash_join.factorize_columns((a, b))), ("a", "factorize x3 + multiply-add", composed)]
    if args.names:
        runs = [r for r in runs if r[1] in args.names.split(",")]
    for form, name, fn in runs:
        d_med, d_min, w_med = _timed(fn, g, args.steps, args.warmup)
        lt = flash_join.last_timings()                                        # (the composition: its third call's)
        line = json.dumps({"workload": wl, "rows": n, "distinct": g, "form": form, "name": name, "device_median_ms": round(d_med, 3),
                           "device_min_ms": round(d_min, 3), "wall_median_ms": round(w_med, 3), "timings": {k: lt[k] for k in KEEP}})
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
        torch.cuda.empty_cache()
    _pair_agg_lines(flash_join, torch, wl, a, b, args, out)


def _by_pair(torch, ga, gb, *cols):
    """the columns in (a, b) order: a stable sort by b, then by a"""
    o = torch.argsort(gb, stable=True)
    o = o[torch.argsort(ga[o], stable=True)]
    return [c[o] for c in (ga, gb) + cols]


def _pair_agg_lines(flash_join, torch, wl, a, b, args, out):
    """four aggregates per pair (FJ_ALGO_KEY_PAIR | FJ_ALGO_AGG_ALL): group_by_agg_columns next to the composition it replaces -
    factorize_columns, group_by_agg over the codes and the two gathers through first_index.  The two results are compared, aligned
    by pair, before anything is timed; then the forms ALTERNATE step by step in this one process.  device_median_ms is the library's
    own time (the composition: the sum of its two calls; its gathers are torch kernels and show in wall_median_ms only); "timings"
    carries the split of every library call."""
    names = ("group_by_agg_columns", "factorize_columns + group_by_agg + 2 gathers")
    if args.names and not any(nm in args.names.split(",") for nm in names):
        return
    n = a.numel()
    v = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device=a.device)
    split = {}

    def fused():
        g, sec, (ga, gb), cnt, sm, mn, mx = flash_join.group_by_agg_columns((a, b), v)
        split[names[0]] = {k: flash_join.last_timings()[k] for k in KEEP}
        return g, sec, ga, gb, cnt, sm, mn, mx

    def composed():
        g, s1, codes, first = flash_join.factorize_columns((a, b))
        t1 = {k: flash_join.last_timings()[k] for k in KEEP}
        g2, s2, gk, cnt, sm, mn, mx = flash_join.group_by_agg(codes, v)
        split[names[1]] = {"factorize_columns": t1, "group_by_agg": {k: flash_join.last_timings()[k] for k in KEEP}}
        rows = first[gk]
        return g2, s1 + s2, a[rows], b[rows], cnt, sm, mn, mx

    rf, rc = fused(), composed()
    assert rf[0] == rc[0], (rf[0], rc[0])
    for x, y in zip(_by_pair(torch, *rf[2:]), _by_pair(torch, *rc[2:])):
        assert torch.equal(x, y), "group_by_agg_columns and its composition disagree"
    g = rf[0]
    del rf, rc, x, y
    torch.cuda.empty_cache()
    fns = (fused, composed)
    dev, wall = ([], []), ([], [])
    for i in range(args.warmup + args.steps):
        for j, fn in enumerate(fns):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            assert r[0] == g, (r[0], g)
            if i >= args.warmup:
                dev[j].append(r[1] * 1e3)
                wall[j].append((t1 - t0) * 1e3)
            del r
    for j, name in enumerate(names):
        line = json.dumps({"workload": wl, "rows": n, "distinct": g, "form": "a", "name": name, "alternating": True,
                           "device_median_ms": round(statistics.median(dev[j]), 3), "device_min_ms": round(min(dev[j]), 3),
                           "wall_median_ms": round(statistics.median(wall[j]), 3), "timings": split[name]})
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="u1m,distinct,hot")
    ap.add_argument("--forms", default="a,b")
    ap.add_argument("--names", default="", help="comma-separated names of the lines to run (default: every line of the chosen forms)")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "group_by_probe.jsonl"))
    args = ap.parse_args()
    import torch
    import flash_join
    flash_join.initialize()
    forms = args.forms.split(",")
    out = open(args.out, "a")
    for wl in args.workloads.split(","):
        if wl in PAIR_WORKLOADS:
            _pair_workload(flash_join, torch, wl, args, out)
            continue
        n, g = WORKLOADS[wl]
        if g == n:
            keys = torch.arange(n, dtype=torch.int64, device="cuda:0")[torch.randperm(n, device="cuda:0")] * SPREAD
        else:
            keys = torch.randint(0, g, (n,), dtype=torch.int64, device="cuda:0")
            keys[:g] = torch.arange(g, dtype=torch.int64, device="cuda:0")        # every key occurs
            keys *= SPREAD
        if wl == "hot":
            keys[::10] = keys[12345].clone()                                      # (key 12345 sits at row 12345)
        vals = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device="cuda:0")

        def composed_count():
            uk, cnt = torch.unique(keys, return_counts=True)
            return uk.numel(), None, uk, cnt

        def composed_sum():
            uk, inv = torch.unique(keys, return_inverse=True)
            return uk.numel(), None, uk, torch.zeros(uk.numel(), dtype=torch.int64, device=keys.device).index_add_(0, inv, vals)

        def composed_min():
            uk, inv = torch.unique(keys, return_inverse=True)
            return uk.numel(), None, uk, torch.full((uk.numel(),), 2**63 - 1, dtype=torch.int64, device=keys.device).scatter_reduce_(0, inv, vals, "amin")

        def composed_inverse():
            uk, inv = torch.unique(keys, return_inverse=True)
            return uk.numel(), None, uk, inv

        def composed_rows_factorize():
            n_g, _, codes, uk = flash_join.factorize(keys)
            _, row_index = torch.sort(codes, stable=True)
            offsets = torch.zeros(n_g + 1, dtype=torch.int64, device=keys.device)
            torch.cumsum(torch.bincount(codes, minlength=n_g), 0, out=offsets[1:])
            return n_g, None, uk, offsets, row_index

        def composed_rows_unique():
            uk, inv, cnt = torch.unique(keys, return_inverse=True, return_counts=True)
            row_index = torch.argsort(inv, stable=True)
            offsets = torch.zeros(uk.numel() + 1, dtype=torch.int64, device=keys.device)
            torch.cumsum(cnt, 0, out=offsets[1:])
            return uk.numel(), None, uk, offsets, row_index

        def factorize_sum(v=vals):
            n_g, sec, codes, uk = flash_join.factorize(keys)
            return n_g, sec, uk, torch.zeros(n_g, dtype=v.dtype, device=keys.device).index_add_(0, codes, v)

        fvals = torch.randint(-2**20, 2**20, (n,), dtype=torch.int64, device="cuda:0").to(torch.float64) * 2.0**-10      # (exact sums in any order)
        dkeys = flash_join.unique(keys)[2]                                        # the build side of the join forms: every row has a partner
        index = []                                                                # built on first use, outside the timed region

        def joined(fn):
            """a join form's (P or m, seconds, ...) as (g, seconds): every row of `keys` has its partner among the g distinct keys"""
            def run():
                if fn.__code__.co_argcount and not index:
                    index.append(flash_join.build_index(dkeys))
                r = fn(index[0]) if fn.__code__.co_argcount else fn()
                assert r[0] == n, (r[0], n)
                return (g,) + tuple(r[1:])
            return run

        runs = []
        if "a" in forms:
            runs += [("a", "unique", lambda: flash_join.unique(keys)),
                     ("a", "unique_return_index", lambda: flash_join.unique(keys, return_index=True)),
                     ("a", "distinct_count", lambda: flash_join.distinct_count(keys)),
                     ("a", "group_by_count", lambda: flash_join.group_by_count(keys)),
                     ("a", "group_by_sum", lambda: flash_join.group_by_sum(keys, vals)),
                     ("a", "group_by_min", lambda: flash_join.group_by_min(keys, vals)),
                     ("a", "group_by_max", lambda: flash_join.group_by_max(keys, vals)),
                     ("a", "factorize", lambda: flash_join.factorize(keys)),
                     ("a", "factorize+index_add", factorize_sum),
                     ("a", "group_by_sum_f64", lambda: flash_join.group_by_sum(keys, fvals, float64=True)),
                     ("a", "group_by_min_f64", lambda: flash_join.group_by_min(keys, fvals, float64=True)),
                     ("a", "group_join_sum", joined(lambda: flash_join.group_join_sum(dkeys, keys, vals))),
                     ("a", "group_join_sum_f64", joined(lambda: flash_join.group_join_sum(dkeys, keys, fvals, float64=True))),
                     ("a", "Index.group_sum", joined(lambda ix: ix.group_sum(keys, vals))),
                     ("a", "Index.group_sum_f64", joined(lambda ix: ix.group_sum(keys, fvals, float64=True))),
                     ("a", "factorize+index_add_f64", lambda: factorize_sum(fvals)),
                     ("a", "group_rows", lambda: flash_join.group_rows(keys))]
        if "b" in forms:
            runs += [("b", "torch.unique(return_counts)", composed_count), ("b", "torch.unique(return_inverse)", composed_inverse),
                     ("b", "torch.unique(return_inverse)+index_add", composed_sum),
                     ("b", "torch.unique(return_inverse)+scatter_reduce_amin", composed_min),
                     ("b", "factorize+sort+bincount+cumsum", composed_rows_factorize),
                     ("b", "torch.unique(return_inverse+return_counts)+argsort", composed_rows_unique)]
        if args.names:
            runs = [r for r in runs if r[1] in args.names.split(",")]
        for form, name, fn in runs:
            d_med, d_min, w_med = _timed(fn, g, args.steps, args.warmup)
            lt = flash_join.last_timings() if form == "a" else None
            line = json.dumps({"workload": wl, "rows": n, "distinct": g, "form": form, "name": name,
                               "device_median_ms": None if d_med is None else round(d_med, 3),
                               "device_min_ms": None if d_min is None else round(d_min, 3), "wall_median_ms": round(w_med, 3),
                               "timings": {k: lt[k] for k in KEEP} if lt else None})
            print(line, flush=True)
            out.write(line + "\n")
            out.flush()
            torch.cuda.empty_cache()
        for ix in index:
            ix.close()
        del keys, vals, fvals, dkeys
        torch.cuda.empty_cache()
    out.close()


if __name__ == "__main__":
    main()
