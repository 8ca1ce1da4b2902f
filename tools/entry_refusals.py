"""Every refusal of fj_join_device and fj_join_host that needs no device, over a grid of algo words, materialize, null patterns, sizes
and (device entry) capacities, hash_top_bits and misaligned pointers - on a machine WITHOUT a GPU, where a call that passes every
check ends in "null context" (device entry, ctx = NULL) or "HIP device 0 not available" (host entry) within microseconds.

    python tools/entry_refusals.py                    totals and a digest of every (inputs -> rc, message) of the library FJ_LIB_VARIANT names
    python tools/entry_refusals.py --against parent   the same walk on that library and lib/ab/parent.so side by side (tools/mk_lib_variant.sh):
                                                      fails unless both refuse the same inputs and the device entry's messages are byte-identical;
                                                      prints the host entry's message changes grouped by (old, new) with the numbers masked

The host entry gets real 100-row arrays (500 words for the value / plane input): no pointer it is handed is ever invalid.  The device
entry gets made-up aligned addresses that are never dereferenced.  --jobs N walks the algo words in N processes (default: the CPUs)."""
import argparse, ctypes, hashlib, itertools, os, re, sys
from collections import Counter
from multiprocessing import Pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HDR = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
FLAGS = {n: int(v, 16) for n, v in re.findall(r"#define FJ_ALGO_([A-Z_]+)\s+(0x[0-9a-fA-F]+)", HDR)}
assert len(FLAGS) == 22, FLAGS
F = FLAGS
GB_MODS = [F[n] for n in ("AGG_MIN", "AGG_MAX", "AGG_SIGNED", "AGG_FLOAT", "ROW_IDS", "INVERSE", "AGG_ALL", "AGG_ARG", "AGG_MERGE", "KEY_PAIR", "GROUP_ROWS")]
BO_MODS = [F[n] for n in ("AGG_MIN", "AGG_MAX", "AGG_SIGNED", "AGG_FLOAT", "RETAIN_BUILD", "REUSE_BUILD", "ACCUMULATE")]
PO_MODS = [F[n] for n in ("ROW_IDS", "RETAIN_BUILD", "REUSE_BUILD")]
MULTI_COUNT = F["FULL_OUTER"] | F["ALL_COPIES"]
BIG = 2**40 + 1
SIZES = [(0, 0), (100, 0), (0, 100), (100, 100), (100, 99), (BIG, BIG)]     # the last pair: device entry only (the host entry would read its arrays past their end)


def subsets(bits, at_most=None):
    for k in range((len(bits) if at_most is None else at_most) + 1):
        for c in itertools.combinations(bits, k):
            yield sum(c)


def algo_words():
    words = set(subsets(list(F.values()), 3))
    words |= {F["GROUP_BY"] | m for m in subsets(GB_MODS)}
    words |= {F["BUILD_ORDER"] | m for m in subsets(BO_MODS)}
    words |= {F["PROBE_ORDER"] | m for m in subsets(PO_MODS)}
    return sorted(w | base for w in words for base in (0, 1, 2, 3)) + [-1]


def load(path):
    L = ctypes.CDLL(path)
    vp, i32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    L.fj_last_error.restype = ctypes.c_char_p
    L.fj_join_device.restype = i32
    L.fj_join_device.argtypes = [vp, i32, i32, i32, vp, vp, sz, vp, sz, vp, i32, vp, vp, vp, sz, vp]
    L.fj_join_host.restype = i32
    L.fj_join_host.argtypes = [i32, i32, i32, vp, vp, sz, vp, sz, vp, vp, vp, vp]
    assert L.fj_device_count() == 0, "a HIP device is present: an accepted call would run"
    return L


def walk(words, libs):
    """Yields (entry, inputs, [(rc, message) per library]) over the grid for these algo words."""
    import numpy as np
    k, v, p = np.arange(100, dtype=np.uint64), np.arange(500, dtype=np.uint64), np.arange(100, dtype=np.uint64)
    cnt = (ctypes.c_uint64 * 3)()
    sec = ctypes.c_double()
    hok, hov = ctypes.c_void_p(), ctypes.c_void_p()
    CNT, SEC, HOK, HOV = (ctypes.addressof(x) for x in (cnt, sec, hok, hov))
    # device entry: (capacity, hash_top_bits, offset of d_build_vals, of d_out_keys, of d_out_vals)
    variants = [(c, 64, 0, 0, 0) for c in (0, 99, 100, 200)] + [(200, 48, 0, 0, 0), (200, 32, 0, 0, 0), (200, 64, 8, 0, 0), (200, 64, 0, 4, 0), (200, 64, 0, 0, 4)]
    for algo in words:
        counts = (CNT, None) if algo >= 0 and algo & MULTI_COUNT else (CNT,)
        for mat in (0, 1):
            for pat in range(32):
                ok, ov, bk, bv, pk = (bool(pat & (1 << i)) for i in range(5))
                for nb, n_p in SIZES:
                    for oc in counts:
                        for cap, top, mis_bv, mis_ok, mis_ov in variants:
                            args = (None, algo, 0, mat, 0x10000 if bk else None, 0x20000 + mis_bv if bv else None, nb, 0x30000 if pk else None, n_p, None, top,
                                    oc, 0x40000 + mis_ok if ok else None, 0x50000 + mis_ov if ov else None, cap, None)
                            yield "device", (algo, mat, pat, nb, n_p, oc is not None, cap, top, mis_bv, mis_ok, mis_ov), [(L.fj_join_device(*args), L.fj_last_error()) for L in libs]
                        if nb != BIG:
                            args = (algo, 0, mat, k.ctypes.data if bk else None, v.ctypes.data if bv else None, nb, p.ctypes.data if pk else None, n_p,
                                    oc, SEC, HOK if ok else None, HOV if ov else None)
                            res = [(L.fj_join_host(*args), L.fj_last_error()) for L in libs]
                            assert not hok.value and not hov.value
                            yield "host", (algo, mat, pat, nb, n_p, oc is not None), res


ACCEPTED = {"device": b"fj_join_device: null context", "host": b"fj_ctx_create: HIP device 0 not available"}
mask = lambda m: re.sub(rb"\d+", b"N", m)


def work(job):
    words, paths = job
    libs = [load(p) for p in paths]
    tot, digest = Counter(), hashlib.sha256()
    changed, bad = Counter(), []
    for entry, inputs, res in walk(words, libs):
        tot[entry, "calls"] += 1
        for i, (rc, msg) in enumerate(res):
            assert rc != 0, (entry, inputs)
            tot[entry, i, "accepted" if msg.startswith(ACCEPTED[entry]) else "refused"] += 1
        digest.update(repr((entry, inputs, res[-1])).encode())
        if len(res) == 2 and res[0] != res[1]:
            (_, old), (_, new) = res
            if old.startswith(ACCEPTED[entry]) != new.startswith(ACCEPTED[entry]):
                tot[entry, "refused set differs"] += 1
                if len(bad) < 5:
                    bad.append((entry, inputs, old, new))
            elif entry == "device":
                tot[entry, "message differs"] += 1
                if len(bad) < 5:
                    bad.append((entry, inputs, old, new))
            else:
                changed[mask(old), mask(new)] += 1
    return tot, changed, bad, digest.hexdigest()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--against", help="name of a second library under lib/ab/ to compare with (the OLD one)")
    ap.add_argument("--jobs", type=int, default=len(os.sched_getaffinity(0)))
    a = ap.parse_args()
    from flash_hash_join_amd import _lib
    paths = ([os.path.join(os.path.dirname(_lib.PRODUCT_LIB_PATH), "ab", a.against + ".so")] if a.against else []) + [_lib.LIB_PATH]
    words = algo_words()
    chunks = [words[i::a.jobs * 8] for i in range(a.jobs * 8)]
    tot, changed, bad, digests = Counter(), Counter(), [], []
    with Pool(a.jobs) as pool:
        for t, c, b, d in pool.imap(work, [(w, paths) for w in chunks]):
            tot.update(t); changed.update(c); bad += b; digests.append(d)
    names = [os.path.relpath(p, ROOT) for p in paths]
    print(f"grid: {len(words)} algo words x materialize 0/1 x 32 null patterns x sizes {SIZES[:-1]} + device entry (2^40+1, 2^40+1)")
    print("      device entry: out_capacity 0/99/100/200, hash_top_bits 48 and 32, d_build_vals + 8, d_out_keys + 4, d_out_vals + 4; out_count NULL for the multi-count forms")
    for entry in ("device", "host"):
        print(f"{entry} entry: {tot[entry, 'calls']} calls")
        for i, n in enumerate(names):
            print(f"  {n}: refused {tot[entry, i, 'refused']}, accepted {tot[entry, i, 'accepted']}")
        if a.against:
            print(f"  inputs refused by one library only: {tot[entry, 'refused set differs']}")
    if not a.against:
        print("digest of every (inputs -> rc, message):", hashlib.sha256("".join(digests).encode()).hexdigest())
        sys.exit(0)
    print(f"device entry: messages that differ: {tot['device', 'message differs']}")
    print(f"host entry: messages that differ (both refusals of the same call), by (old, new) with numbers masked: {sum(changed.values())} calls, {len(changed)} pairs")
    for (old, new), n in sorted(changed.items(), key=lambda kv: -kv[1]):
        print(f"{n:>9}  old: {old.decode()}\n           new: {new.decode()}")
    for b in bad[:10]:
        print("BAD", b)
    sys.exit(1 if bad else 0)
