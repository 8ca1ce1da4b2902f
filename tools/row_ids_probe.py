"""Row-index gather maps (join_indices, FJ_ALGO_ROW_IDS) on device tensors against the key-returning forms on the same inputs, in
one process.  One JSON line per pair: join_indices(how="inner") against the yardstick hash_join_radix(return_arrays=True),
how="left" against left_join(return_arrays=True), how="anti" against anti_join(return_arrays=True) - medians of the device time
(core_duration_sec), last_timings() of the last step of each, and the probe side's partition-pass bandwidth with and without the
index plane (probe_part_kernel_ms), pass by pass.

    python tools/row_ids_probe.py [--workloads c3,c2] [--steps 10] [--warmup 2]

Probe-pass traffic from the algorithm: a first pass reads 8 B per key and writes 8 B (keys only) or reads 8 / writes 16 (keys +
positions made in the pass); a later pass reads and writes 8 B (keys only) or 16 + 16 (keys + positions)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"c3": (100_000_000, 1_000_000_000, 5000), "c2": (1_000_000, 100_000_000, 5000)}


def _pass_bytes(n_p, i, plane):
    """algorithmic bytes of the probe side's i-th partition pass"""
    if i == 0:
        return (8 + (16 if plane else 8)) * n_p
    return (32 if plane else 16) * n_p


def _timed(fn, want, steps, warmup):
    import torch
    import flash_join
    times = []
    for i in range(warmup + steps):
        r = fn()
        assert r[0] == want, (r[0], want)
        if i >= warmup:
            times.append(r[1] * 1e3)
        del r
        torch.cuda.synchronize()
    return statistics.median(times), min(times), flash_join.last_timings()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="c3,c2")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    import torch
    import flash_join
    from flash_hash_join_amd import datagen
    flash_join.initialize()
    for wl in args.workloads.split(","):
        nb, n_p, hit_bp = WORKLOADS[wl]
        bk, bv = datagen.build_device(nb, "cuda:0")
        pk, expected = datagen.probe_device(n_p, nb, "cuda:0", seed=1, hit_bp=hit_bp)
        u_exp = n_p - expected
        pairs = {
            "inner": (lambda: flash_join.join_indices(bk, pk), "hash_join_radix", lambda: flash_join.hash_join_radix(bk, bv, pk, return_arrays=True), expected),
            "left": (lambda: flash_join.join_indices(bk, pk, how="left"), "left_join", lambda: flash_join.left_join(bk, bv, pk, return_arrays=True), expected),
            "anti": (lambda: flash_join.join_indices(bk, pk, how="anti"), "anti_join", lambda: flash_join.anti_join(bk, pk, return_arrays=True), u_exp),
        }
        for how, (fn_ids, base_name, fn_base, want) in pairs.items():
            b_med, b_min, b_t = _timed(fn_base, want, args.steps, args.warmup)
            r_med, r_min, r_t = _timed(fn_ids, want, args.steps, args.warmup)
            passes = r_t["passes"]
            # bytes per second of each probe-side pass, with the index plane and keys only (the same pass of the same plan)
            r_bw = [_pass_bytes(n_p, i, True) / (r_t["probe_part_kernel_ms"][i] * 1e-3) for i in range(passes)]
            b_bw = [_pass_bytes(n_p, i, False) / (b_t["probe_part_kernel_ms"][i] * 1e-3) for i in range(passes)]
            keep = ("total_ms", "build_phase_ms", "probe_phase_ms", "join_ms", "emit_ms", "probe_part_kernel_ms", "path", "passes",
                    "fell_back", "lds_retries")
            print(json.dumps({"workload": wl, "nb": nb, "np": n_p, "hit_bp": hit_bp, "how": how, "baseline": base_name,
                              "row_ids_median_ms": round(r_med, 3), "row_ids_min_ms": round(r_min, 3),
                              "baseline_median_ms": round(b_med, 3), "baseline_min_ms": round(b_min, 3),
                              "ratio": round(r_med / b_med, 3),
                              "probe_pass_bytes_per_s": [round(x) for x in r_bw], "baseline_probe_pass_bytes_per_s": [round(x) for x in b_bw],
                              "probe_pass_bw_ratio": [round(x / y, 3) for x, y in zip(r_bw, b_bw)],
                              "row_ids_timings": {k: r_t[k] for k in keep}, "baseline_timings": {k: b_t[k] for k in keep}}), flush=True)
        del bk, bv, pk
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
