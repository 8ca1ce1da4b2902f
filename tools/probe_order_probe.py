"""Probe-order joins (lookup / isin / lookup_indices, FJ_ALGO_PROBE_ORDER) on device tensors next to what a user had to compose
before them, and next to left_join as the lower bound of the shared partition passes.  One JSON line per form:

  (a) lookup, lookup(return_mask=True), isin, lookup_indices
  (b) the composition: join_indices(how="left"), then vals = where(bi >= 0, bv[bi], fill), then out[pi] = vals in torch - the wall
      time of the three steps between two device synchronisations, and the join's own device time beside it
  (c) left_join(return_arrays=True)

    python tools/probe_order_probe.py [--workloads c3,c2] [--forms a,b,c] [--steps 10] [--warmup 2]

(b) and (c) call nothing this extension added, so they can be timed on a build of the parent commit through FJ_LIB_VARIANT=<name>
(tools/mk_lib_variant.sh; --forms b,c).  Times of (a) and (c) are device times (core_duration_sec, HIP events); (b) has torch
kernels in it, so its figure is wall time around a synchronised region, and (a) is reported that way too ("wall_median_ms") so that
the two compare like with like."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"c3": (100_000_000, 1_000_000_000, 5000), "c2": (1_000_000, 100_000_000, 5000)}
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
    ap.add_argument("--forms", default="a,b,c")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import flash_join
    from flash_hash_join_amd import datagen
    flash_join.initialize()
    forms = args.forms.split(",")
    fill = 7
    for wl in args.workloads.split(","):
        nb, n_p, hit_bp = WORKLOADS[wl]
        bk, bv = datagen.build_device(nb, "cuda:0")
        pk, expected = datagen.probe_device(n_p, nb, "cuda:0", seed=1, hit_bp=hit_bp)

        def composed():
            m, sec, pi, bi = flash_join.join_indices(bk, pk, how="left")
            vals = torch.where(bi >= 0, bv[bi.clamp(min=0)], torch.full_like(bi, fill))
            out = torch.empty_like(vals)
            out[pi] = vals
            return m, sec, out

        runs = []
        if "a" in forms:
            runs += [("a", "lookup", lambda: flash_join.lookup(bk, bv, pk)),
                     ("a", "lookup_mask", lambda: flash_join.lookup(bk, bv, pk, return_mask=True)),
                     ("a", "lookup_mask_fill", lambda: flash_join.lookup(bk, bv, pk, fill_value=fill, return_mask=True)),
                     ("a", "isin", lambda: flash_join.isin(pk, bk)),
                     ("a", "lookup_indices", lambda: flash_join.lookup_indices(bk, pk))]
        if "b" in forms:
            runs += [("b", "join_indices_left+gather+scatter", composed)]
        if "c" in forms:
            runs += [("c", "left_join", lambda: flash_join.left_join(bk, bv, pk, return_arrays=True))]
        for form, name, fn in runs:
            d_med, d_min, w_med, lt = _timed(fn, expected, args.steps, args.warmup)
            print(json.dumps({"workload": wl, "nb": nb, "np": n_p, "hit_bp": hit_bp, "form": form, "name": name,
                              "lib_variant": os.environ.get("FJ_LIB_VARIANT", ""),
                              "device_median_ms": round(d_med, 3), "device_min_ms": round(d_min, 3), "wall_median_ms": round(w_med, 3),
                              "timings": {k: lt[k] for k in KEEP}}), flush=True)
            torch.cuda.empty_cache()
        del bk, bv, pk
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
