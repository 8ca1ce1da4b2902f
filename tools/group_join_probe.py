"""Build-order aggregate joins (group_join_count / group_join_sum / group_join_min / group_join_max, FJ_ALGO_BUILD_ORDER) on device
tensors next to what a user had to compose before them, and next to the counting join as the floor of the shared partition passes.
One JSON line per form:

  (a) group_join_count, group_join_sum, group_join_sum(return_counts=True)
  (m) group_join_min and group_join_max, signed and unsigned, and group_join_min(return_counts=True); their yardstick is the sum form
      of (a) in the same run (identical bytes moved)
  (b) the composition: join_indices(how="inner", many_to_many=True), then torch.bincount(build_idx, minlength=nb) (counts),
      zeros(nb).index_add_(0, build_idx, pv[probe_idx]) (sums) or full(nb, INT64_MAX).scatter_reduce_(0, build_idx, pv[probe_idx],
      "amin") (minima) - the wall time of the steps between two device synchronisations, and the join's own device time beside it
  (c) hash_join_count_radix: the counting join of the same sizes
  (d) the hot-key shape: one key owns 10 % of the probe rows (workload "hot": 1M x 1B), forms (a) and (m) only

    python tools/group_join_probe.py [--workloads c3,c2,hot] [--forms a,m,b,c] [--steps 8] [--warmup 2]

(b) and (c) call nothing these extensions added, so they can be timed on a build of the parent commit through FJ_LIB_VARIANT=<name>
(--forms b,c).  Times of (a) and (c) are device times (core_duration_sec, HIP events); (b) has torch kernels in it, so its figure is
wall time around a synchronised region, and (a) is reported that way too ("wall_median_ms") so that the two compare like with like."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"c3": (100_000_000, 1_000_000_000, 5000), "c2": (1_000_000, 100_000_000, 5000), "hot": (1_000_000, 1_000_000_000, 5000)}
KEEP = ("total_ms", "build_phase_ms", "probe_phase_ms", "join_ms", "emit_ms", "probe_part_kernel_ms", "path", "passes", "fell_back")


def _timed(fn, want, steps, warmup):
    """medians of the device time fn reports (r[1]) and of the wall time of the synchronised call"""
    import torch
    import flash_join
    dev, wall = [], []
    for i in range(warmup + steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        assert r[0] == want, (r[0], want)
        if i >= warmup:
            dev.append(r[1] * 1e3)
            wall.append((t1 - t0) * 1e3)
        del r
    return statistics.median(dev), min(dev), statistics.median(wall), flash_join.last_timings()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c2")
    ap.add_argument("--forms", default="a,m,b,c")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import flash_join
    from flash_hash_join_amd import datagen
    flash_join.initialize()
    forms = args.forms.split(",")
    for wl in args.workloads.split(","):
        nb, n_p, hit_bp = WORKLOADS[wl]
        bk, bv = datagen.build_device(nb, "cuda:0")
        pk, expected = datagen.probe_device(n_p, nb, "cuda:0", seed=1, hit_bp=hit_bp)
        if wl == "hot":                                                # one build key takes every tenth probe row
            hot = pk[::10]
            expected += int((~torch.isin(hot, bk)).sum())             # (the generator's build keys are unique: a hit counts once)
            hot.copy_(bk[12345].expand_as(hot))
            del hot
        pv = torch.randint(-2**63, 2**63 - 1, (n_p,), dtype=torch.int64, device="cuda:0")

        def composed_count():
            n, sec, pi, bi = flash_join.join_indices(bk, pk, how="inner", many_to_many=True)
            return n, sec, torch.bincount(bi, minlength=nb)

        def composed_sum():
            n, sec, pi, bi = flash_join.join_indices(bk, pk, how="inner", many_to_many=True)
            return n, sec, torch.zeros(nb, dtype=torch.int64, device=bk.device).index_add_(0, bi, pv[pi])

        def composed_min():
            n, sec, pi, bi = flash_join.join_indices(bk, pk, how="inner", many_to_many=True)
            return n, sec, torch.full((nb,), 2**63 - 1, dtype=torch.int64, device=bk.device).scatter_reduce_(0, bi, pv[pi], "amin")

        runs = []
        if "a" in forms:
            runs += [("a", "group_join_count", lambda: flash_join.group_join_count(bk, pk)),
                     ("a", "group_join_sum", lambda: flash_join.group_join_sum(bk, pk, pv)),
                     ("a", "group_join_sum_counts", lambda: flash_join.group_join_sum(bk, pk, pv, return_counts=True))]
        if "m" in forms:
            runs += [("m", "group_join_min", lambda: flash_join.group_join_min(bk, pk, pv)),
                     ("m", "group_join_min_unsigned", lambda: flash_join.group_join_min(bk, pk, pv, signed=False)),
                     ("m", "group_join_max", lambda: flash_join.group_join_max(bk, pk, pv)),
                     ("m", "group_join_max_unsigned", lambda: flash_join.group_join_max(bk, pk, pv, signed=False)),
                     ("m", "group_join_min_counts", lambda: flash_join.group_join_min(bk, pk, pv, return_counts=True))]
        if "b" in forms and wl != "hot":
            runs += [("b", "join_indices_m2m+bincount", composed_count), ("b", "join_indices_m2m+index_add", composed_sum),
                     ("b", "join_indices_m2m+scatter_reduce_amin", composed_min)]
        if "c" in forms:
            runs += [("c", "hash_join_count_radix", lambda: flash_join.hash_join_count_radix(bk, bv, pk))]
        for form, name, fn in runs:
            d_med, d_min, w_med, lt = _timed(fn, expected, args.steps, args.warmup)
            print(json.dumps({"workload": wl, "nb": nb, "np": n_p, "hit_bp": hit_bp, "form": form, "name": name,
                              "lib_variant": os.environ.get("FJ_LIB_VARIANT", ""),
                              "device_median_ms": round(d_med, 3), "device_min_ms": round(d_min, 3), "wall_median_ms": round(w_med, 3),
                              "timings": {k: lt[k] for k in KEEP}}), flush=True)
            torch.cuda.empty_cache()
        del bk, bv, pk, pv
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
