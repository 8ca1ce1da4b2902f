"""Aggregates onto a prepared build side (Index.group_count / group_sum / group_min, FJ_ALGO_BUILD_ORDER | FJ_ALGO_REUSE_BUILD) on device
tensors next to the two ways of getting the same numbers without them.  One JSON line per (shape, form):

  "prepared"   Index.group_*(probe_keys[, probe_values])                       a fresh, filled output per call
  "accumulate" Index.group_*(..., out=acc[, counts_out=cacc])                   FJ_ALGO_ACCUMULATE into one buffer, no fill
  "one_shot"   group_join_*(build_keys, probe_keys[, probe_values])             the build side's passes in every call
  "torch"      Index.lookup_indices(probe_keys), then torch.bincount / index_add_ / scatter_reduce_ over the rows with a partner

alternating call by call in one run.  The build keys are distinct (datagen.build_device), so the four agree bit for bit; the first
round checks that.

    python tools/prepared_group_probe.py [--shapes 100M:1M,100M:10M,100M:100M,1M:100M] [--steps 8] [--warmup 2] [--out FILE]

"device_*" is the device time the library reports (HIP events; "torch": the lookup_indices call alone - its torch half is in the wall
time only); "wall_*" the wall time of the whole call between two device synchronisations, output allocation included.  50 % of the
probe rows hit."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEEP = ("total_ms", "build_phase_ms", "probe_phase_ms", "join_ms", "path", "passes", "radix_bits", "fell_back")
UNITS = {"K": 1_000, "M": 1_000_000, "B": 1_000_000_000}
FORMS = ("count", "sum", "min_s", "sum+counts")


def _rows(s):
    return int(float(s[:-1]) * UNITS[s[-1]]) if s[-1] in UNITS else int(s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100M:1M,100M:10M,100M:100M,1M:100M")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    import torch
    import flash_join
    from flash_hash_join_amd import datagen
    flash_join.initialize()
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        return r, (t1 - t0) * 1e3

    shapes = [tuple(_rows(x) for x in s.split(":")) for s in args.shapes.split(",")]
    built = None                                                          # (nb, bk, index): one build side serves its batches
    for nb, n_p in shapes:
        if built is None or built[0] != nb:
            if built is not None:
                built[2].close()
            built = None
            flash_join.trim_workspace()
            torch.cuda.empty_cache()
            bk, _ = datagen.build_device(nb, "cuda:0")
            built = (nb, bk, flash_join.build_index(bk))                  # keys only: no build value is read
        _, bk, index = built
        pk, want = datagen.probe_device(n_p, nb, "cuda:0", seed=1, hit_bp=5000)
        pv = (pk * -7046029254386353131) ^ (pk >> 7)                      # full-range int64 words: the sums wrap, both signs occur
        for form in FORMS:
            acc = torch.zeros(nb, dtype=torch.int64, device="cuda:0")
            cacc = torch.zeros(nb, dtype=torch.int64, device="cuda:0")
            if form == "min_s":
                acc.fill_(2**63 - 1)

            def torch_way():
                m, sec, idx = index.lookup_indices(pk)
                hit = idx >= 0
                rows = idx[hit]
                if form == "count":
                    return m, sec, torch.bincount(rows, minlength=nb)
                if form == "min_s":
                    out = torch.full((nb,), 2**63 - 1, dtype=torch.int64, device="cuda:0")
                    return m, sec, out.scatter_reduce_(0, rows, pv[hit], "amin", include_self=True)
                out = torch.zeros(nb, dtype=torch.int64, device="cuda:0").index_add_(0, rows, pv[hit])
                return (m, sec, out, torch.bincount(rows, minlength=nb)) if form == "sum+counts" else (m, sec, out)

            calls = {
                "count": {"prepared": lambda: index.group_count(pk), "accumulate": lambda: index.group_count(pk, out=cacc),
                          "one_shot": lambda: flash_join.group_join_count(bk, pk)},
                "sum": {"prepared": lambda: index.group_sum(pk, pv), "accumulate": lambda: index.group_sum(pk, pv, out=acc),
                        "one_shot": lambda: flash_join.group_join_sum(bk, pk, pv)},
                "min_s": {"prepared": lambda: index.group_min(pk, pv, signed=True), "accumulate": lambda: index.group_min(pk, pv, out=acc, signed=True),
                          "one_shot": lambda: flash_join.group_join_min(bk, pk, pv, signed=True)},
                "sum+counts": {"prepared": lambda: index.group_sum(pk, pv, return_counts=True),
                               "accumulate": lambda: index.group_sum(pk, pv, out=acc, counts_out=cacc),
                               "one_shot": lambda: flash_join.group_join_sum(bk, pk, pv, return_counts=True)},
            }[form]
            calls["torch"] = torch_way
            res = {name: ([], [], None) for name in calls}
            for i in range(args.warmup + args.steps):
                first = {}
                for name, fn in calls.items():
                    r, wall = once(fn)
                    assert r[0] == want, (name, r[0], want)
                    if i == 0 and name != "accumulate":                   # the four ways agree (distinct build keys)
                        first[name] = r[2:]
                    if i >= args.warmup:
                        res[name][0].append(r[1] * 1e3)
                        res[name][1].append(wall)
                    res[name] = (res[name][0], res[name][1], flash_join.last_timings())
                    del r
                if i == 0:
                    for name in ("one_shot", "torch"):
                        for x, y in zip(first["prepared"], first[name]):
                            assert bool((x == y).all()), (form, name)
                    del first
            rec = {"what": "group", "nb": nb, "np": n_p, "hit_bp": 5000, "form": form}
            for name, (d, w, lt) in res.items():
                rec[name] = {"device_median_ms": round(statistics.median(d), 3), "device_min_ms": round(min(d), 3),
                             "wall_median_ms": round(statistics.median(w), 3), "timings": {k: lt[k] for k in KEEP}}
            p = rec["prepared"]
            rec["device_ratio_vs_one_shot"] = round(p["device_median_ms"] / rec["one_shot"]["device_median_ms"], 4)
            rec["wall_ratio_vs_one_shot"] = round(p["wall_median_ms"] / rec["one_shot"]["wall_median_ms"], 4)
            rec["wall_ratio_vs_torch"] = round(p["wall_median_ms"] / rec["torch"]["wall_median_ms"], 4)
            rec["device_ratio_accumulate_vs_fill"] = round(rec["accumulate"]["device_median_ms"] / p["device_median_ms"], 4)
            rec["wall_ratio_accumulate_vs_fill"] = round(rec["accumulate"]["wall_median_ms"] / p["wall_median_ms"], 4)
            emit(rec)
            del acc, cacc
            torch.cuda.empty_cache()
        del pk, pv
        torch.cuda.empty_cache()
    if built is not None:
        built[2].close()


if __name__ == "__main__":
    main()
