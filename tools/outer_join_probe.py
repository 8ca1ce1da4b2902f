"""Left outer and anti joins on device tensors against the materialising inner join on the same inputs (the yardstick:
hash_join_radix(return_arrays=True)).  One JSON line per (workload, function): median device ms over the timed steps
(core_duration_sec), join_ms of the last step, algorithmic bytes and the fraction of 8 TB/s they make of the median.

    python tools/outer_join_probe.py [--workloads c3,c2] [--steps 10] [--warmup 2]

Algorithmic bytes: every probe key read once (8 B), every build row read once (8 B key, + 8 B value where a value is needed),
every output row written once (8 B key, + 8 B value where the output has values)."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKLOADS = {"c3": (100_000_000, 1_000_000_000, 5000), "c2": (1_000_000, 100_000_000, 5000)}
PEAK = 8e12


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
        runs = {
            "hash_join_radix": (lambda: flash_join.hash_join_radix(bk, bv, pk, return_arrays=True), expected, 8 * n_p + 16 * nb + 16 * expected),
            "left_join": (lambda: flash_join.left_join(bk, bv, pk, return_arrays=True), expected, 8 * n_p + 16 * nb + 16 * n_p),
            "anti_join": (lambda: flash_join.anti_join(bk, pk, return_arrays=True), u_exp, 8 * n_p + 8 * nb + 8 * u_exp),
            "anti_join_count": (lambda: flash_join.anti_join_count(bk, pk), u_exp, 8 * n_p + 8 * nb),
        }
        for name, (fn, want, nbytes) in runs.items():
            times = []
            for i in range(args.warmup + args.steps):
                r = fn()
                assert r[0] == want, (wl, name, r[0], want)
                if i >= args.warmup:
                    times.append(r[1] * 1e3)
                del r
                torch.cuda.synchronize()
            t = flash_join.last_timings()
            med = statistics.median(times)
            print(json.dumps({"workload": wl, "nb": nb, "np": n_p, "hit_bp": hit_bp, "function": name, "median_ms": round(med, 3),
                              "min_ms": round(min(times), 3), "join_ms": round(t["join_ms"], 3), "path": t["path"],
                              "passes": t["passes"], "fell_back": t["fell_back"], "algorithmic_bytes": nbytes,
                              "fraction_of_peak": round(nbytes / (med * 1e-3) / PEAK, 3),
                              "join_fraction_of_peak": round(nbytes / (t["join_ms"] * 1e-3) / PEAK, 3) if t["join_ms"] > 0 else None}), flush=True)
        del bk, bv, pk
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
