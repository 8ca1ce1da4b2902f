"""A prepared build side (build_index / Index, FJ_ALGO_RETAIN_BUILD / FJ_ALGO_REUSE_BUILD) on device tensors next to the one-shot
functions of the same name: one dictionary probed by batches of several sizes.  One JSON line per (shape, form):

  Index.lookup / Index.isin / Index.lookup_indices   against   lookup / isin / lookup_indices   on the same inputs,

alternating call by call in one run, and one line per build side for the cost of build_index itself next to one one-shot lookup -
build_index as a user calls it (a context of its own is created, its workspace and the prepared side's memory are allocated: hipMalloc
is most of it) and, "retain_warm", FJ_ALGO_RETAIN_BUILD again on that context through the C ABI: the workspace is there, the prepared
side is freed and allocated again.

    python tools/prepared_probe.py [--shapes 100M:1M,100M:10M,100M:100M,100M:1B,1M:100M] [--steps 8] [--warmup 2] [--out FILE]

"device_*" is the device time the call reports (core_duration_sec, HIP events: for a reuse the probe side's passes and the join kernel,
for the one-shot call the build side's passes as well); "wall_*" the wall time of the call between two device synchronisations, output
allocation included.  50 % of the probe rows hit."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KEEP = ("total_ms", "build_phase_ms", "probe_phase_ms", "join_ms", "path", "passes", "radix_bits", "fell_back")
UNITS = {"K": 1_000, "M": 1_000_000, "B": 1_000_000_000}


def _rows(s):
    return int(float(s[:-1]) * UNITS[s[-1]]) if s[-1] in UNITS else int(s)


def _once(fn, want):
    import torch
    import flash_join
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    assert r[0] == want, (r[0], want)
    return r[1] * 1e3, (t1 - t0) * 1e3, flash_join.last_timings()


def _pair(prepared, one_shot, want, steps, warmup):
    """the two calls alternating; medians of device and wall time of each, the last timings of each"""
    res = {"prepared": ([], [], None), "one_shot": ([], [], None)}
    for i in range(warmup + steps):
        for name, fn in (("prepared", prepared), ("one_shot", one_shot)):
            d, w, lt = _once(fn, want)
            if i >= warmup:
                res[name][0].append(d)
                res[name][1].append(w)
            res[name] = (res[name][0], res[name][1], lt)
    out = {}
    for name, (d, w, lt) in res.items():
        out[name] = {"device_median_ms": round(statistics.median(d), 3), "device_min_ms": round(min(d), 3),
                     "wall_median_ms": round(statistics.median(w), 3), "timings": {k: lt[k] for k in KEEP}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="100M:1M,100M:10M,100M:100M,100M:1B,1M:100M")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the JSON lines to this file too")
    args = ap.parse_args()
    import torch
    import flash_join
    from flash_hash_join_amd import _lib, api, datagen
    flash_join.initialize()
    L = _lib.load()
    cnt, tw = ctypes.c_uint64(0), _lib.FjTimings()
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    shapes = [tuple(_rows(x) for x in s.split(":")) for s in args.shapes.split(",")]
    built = None                                                          # (nb, bk, bv, index): one build side serves its batches
    for nb, n_p in shapes:
        if built is None or built[0] != nb:
            if built is not None:
                built[3].close()
            built = None
            flash_join.trim_workspace()
            torch.cuda.empty_cache()
            bk, bv = datagen.build_device(nb, "cuda:0")
            pk1, want1 = datagen.probe_device(min(nb, 1_000_000), nb, "cuda:0", seed=9, hit_bp=5000)
            b_dev, b_wall, o_dev, o_wall = [], [], [], []
            for i in range(args.warmup + args.steps):                     # build_index itself next to ONE one-shot lookup of a small batch
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                index = flash_join.build_index(bk, bv)
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                lt = flash_join.last_timings()
                assert index.num_keys == nb
                d, w, lt1 = _once(lambda: flash_join.lookup(bk, bv, pk1), want1)
                if i >= args.warmup:
                    b_dev.append(lt["total_ms"]); b_wall.append((t1 - t0) * 1e3); o_dev.append(d); o_wall.append(w)
                if i + 1 < args.warmup + args.steps:
                    index.close()
            w_dev, w_wall = [], []
            for i in range(args.warmup + args.steps):                     # the replacement on a warm context (index._ctx: the tool looks inside)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                _lib.check(L.fj_join_device(index._ctx, api.ALGO_PROBE_ORDER | api.ALGO_RETAIN_BUILD, 0, 1, bk.data_ptr(), bv.data_ptr(), nb, None, 0,
                                            torch.cuda.current_stream(0).cuda_stream, 64, ctypes.byref(cnt), None, None, 0, ctypes.byref(tw)))
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                assert cnt.value == nb
                if i >= args.warmup:
                    w_dev.append(tw.total_ms); w_wall.append((t1 - t0) * 1e3)
            emit({"what": "build_index", "nb": nb, "one_shot_np": int(pk1.numel()),
                  "retain_warm": {"device_median_ms": round(statistics.median(w_dev), 3), "wall_median_ms": round(statistics.median(w_wall), 3)},
                  "build_index": {"device_median_ms": round(statistics.median(b_dev), 3), "wall_median_ms": round(statistics.median(b_wall), 3),
                                  "timings": {k: lt[k] for k in KEEP}},
                  "one_shot_lookup": {"device_median_ms": round(statistics.median(o_dev), 3), "wall_median_ms": round(statistics.median(o_wall), 3),
                                      "timings": {k: lt1[k] for k in KEEP}}})
            del pk1
            built = (nb, bk, bv, index)
        _, bk, bv, index = built
        pk, want = datagen.probe_device(n_p, nb, "cuda:0", seed=1, hit_bp=5000)
        forms = [("lookup", lambda: index.lookup(pk), lambda: flash_join.lookup(bk, bv, pk)),
                 ("isin", lambda: index.isin(pk), lambda: flash_join.isin(pk, bk)),
                 ("lookup_indices", lambda: index.lookup_indices(pk), lambda: flash_join.lookup_indices(bk, pk))]
        for name, prepared, one_shot in forms:
            r = _pair(prepared, one_shot, want, args.steps, args.warmup)
            emit({"what": "probe", "nb": nb, "np": n_p, "hit_bp": 5000, "form": name, **r,
                  "device_ratio": round(r["prepared"]["device_median_ms"] / r["one_shot"]["device_median_ms"], 4),
                  "wall_ratio": round(r["prepared"]["wall_median_ms"] / r["one_shot"]["wall_median_ms"], 4)})
            torch.cuda.empty_cache()
        del pk
        torch.cuda.empty_cache()
    if built is not None:
        built[3].close()


if __name__ == "__main__":
    main()
