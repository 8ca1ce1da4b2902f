"""All-copies outer joins (duplicates="all"; FJ_ALGO_ALL_COPIES with FJ_ALGO_LEFT_OUTER / FJ_ALGO_FULL_OUTER) whose build side holds
a key with thousands of copies (option "mm_heavy_outer", csrc/fj_many.hip fj_mm_tile_kernel<.., OUTER> and fj_mm_miss_sweep_kernel,
csrc/fj_joins.hip mm_tile_join): the option's contract without a GPU, and - on an MI355X - exact parity with the NumPy reference on
inputs that the default setting refuses: the inputs of tests/test_mm_heavy_keys.py, the hot key absent from the probe side, and a
crowded partition in which hundreds of probe keys match a non-hot build key or nothing at all (the cross-tile "no partner" verdict).

Reference (integers, compared exactly): oracle.np_inner_join for rows [0, P) as sorted pair multisets (oracle.canon_pairs),
pk[~np.isin(pk, bk)] for rows [P, P + u) and (bk, bv)[~np.isin(bk, pk)] for rows [P + u, P + u + r) as sorted arrays, the range
boundaries taken from (P, u, r).  Build values are row ids, so every build row is distinguishable."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import keymix
from conftest import ROOT, product_env

GOLDEN = np.uint64(0x9E3779B97F4A7C15)
LIMIT = 4096                      # build rows per final partition the one-table kernel takes
MAX_PAIRS = 20_000_000
TILED = 4096                      # FJ_LDS_RETRIES_MM_TILED
LEFT, ROW_IDS, FULL, ALL, RADIX = 0x20, 0x80, 0x100, 0x200, 2
HOT = 12345


# ---- inputs (NumPy only; built as in tests/test_mm_heavy_keys.py) ---------------------------------------------------------------
def refusal_input():
    bk = np.concatenate([np.full(6000, 12345, dtype=np.uint64), np.arange(100000, 100500, dtype=np.uint64)])
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = np.array([12345, 100001, 7], dtype=np.uint64)
    return bk, bv, pk


def hot_key_input(hot):
    rng = np.random.default_rng(2024)
    ids = rng.integers(10, 50_010, size=200_000, dtype=np.uint64)
    bk = np.concatenate([np.full(100_000, hot, dtype=np.uint64), ids * GOLDEN])
    rng.shuffle(bk)
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = np.concatenate([np.full(40, hot, dtype=np.uint64), rng.integers(10, 100_010, size=30_000, dtype=np.uint64) * GOLDEN])
    rng.shuffle(pk)
    return bk, bv, pk


def hot_key_absent_input():
    """hot_key_input with the hot key taken off the probe side: its 100 000 copies all belong in the third range of FULL."""
    bk, bv, pk = hot_key_input(HOT)
    return bk, bv, pk[pk != np.uint64(HOT)]


def colliding_input():
    rng = np.random.default_rng(7)
    cand = np.arange(1, 400_000, dtype=np.uint64)
    top = keymix.hash_w1(cand) >> np.uint32(20)
    group = cand[top == top[0]][:12]
    copies = rng.integers(1000, 3001, size=group.size)
    bk = np.concatenate([np.repeat(group, copies), np.arange(10**9, 10**9 + 100_000, dtype=np.uint64)])
    rng.shuffle(bk)
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = np.concatenate([np.repeat(group, 50), rng.integers(10**9 - 50_000, 10**9 + 150_000, size=40_000, dtype=np.uint64)])
    rng.shuffle(pk)
    return bk, bv, pk, group, copies


def zipf_input():
    rng = np.random.default_rng(99)
    n_dom = 1_000_000
    cdf = np.cumsum(1.0 / np.arange(1, n_dom + 1))
    cdf /= cdf[-1]
    draw = lambda n: (np.searchsorted(cdf, rng.random(n)) + 1).astype(np.uint64)
    bk = draw(1_000_000) * GOLDEN
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = draw(1500) * GOLDEN
    return bk, bv, pk


def crowded_input():
    """The hot key's partition, crowded: ids whose hash word 1 agrees with the hot key's in its top 12 bits (the same final partition
    under every plan of at most 12 radix bits) - about half of them on the build side with 1..8 copies each, shuffled among the
    100 000 hot copies and 200 000 background rows; the probe side holds every one of them three times, the hot key 40 times and
    30 000 background draws.  Returns (bk, bv, pk, group, on_build)."""
    rng = np.random.default_rng(31)
    hot = np.uint64(HOT)
    cand = np.arange(1, 3_000_000, dtype=np.uint64)
    top = keymix.hash_w1(cand) >> np.uint32(20)
    hot_top = keymix.hash_w1(np.array([hot], dtype=np.uint64))[0] >> np.uint32(20)
    group = cand[(top == hot_top) & (cand != hot)]
    on_build = group[::2]
    copies = rng.integers(1, 9, size=on_build.size)
    ids = rng.integers(10, 50_010, size=200_000, dtype=np.uint64)
    bk = np.concatenate([np.full(100_000, hot, dtype=np.uint64), np.repeat(on_build, copies), ids * GOLDEN])
    rng.shuffle(bk)
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = np.concatenate([np.full(40, hot, dtype=np.uint64), np.repeat(group, 3),
                         rng.integers(10, 100_010, size=30_000, dtype=np.uint64) * GOLDEN])
    rng.shuffle(pk)
    return bk, bv, pk, group, on_build


def max_multiplicity(bk):
    return int(np.unique(bk, return_counts=True)[1].max())


def np_ref(bk, bv, pk):
    """(P, pair keys, pair values, unmatched probe keys, unmatched build keys, their values) of the NumPy reference; P is bounded
    before anything runs on the GPU."""
    from oracle.oracle import np_inner_join
    P = np_inner_join(bk, bv, pk)
    assert 0 < P <= MAX_PAIRS, P
    P, k, v = np_inner_join(bk, bv, pk, return_arrays=True)
    rest = ~np.isin(bk, pk)
    return P, k, v, pk[~np.isin(pk, bk)], bk[rest], bv[rest]


def same_pairs(k1, v1, k2, v2):
    from oracle.oracle import canon_pairs
    a = canon_pairs(np.asarray(k1).view(np.uint64), np.asarray(v1).view(np.uint64))
    b = canon_pairs(np.asarray(k2).view(np.uint64), np.asarray(v2).view(np.uint64))
    return a[0].size == b[0].size and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def srt(a):
    return np.sort(np.asarray(a).reshape(-1).view(np.uint64))


def host(t):
    return (t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)).view(np.uint64)


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_the_option_defaults_to_zero_and_round_trips():
    from flash_hash_join_amd import api
    assert api.get_option("mm_heavy_outer") == 0
    try:
        for v in (1, 0, 1):
            api.set_option("mm_heavy_outer", v)
            assert api.get_option("mm_heavy_outer") == v
            assert api.get_option("mm_heavy_keys") == 0                         # independent
    finally:
        api.set_option("mm_heavy_outer", 0)
    assert api.get_option("mm_heavy_outer") == 0


@pytest.mark.parametrize("value", [-1, 2, 4096])
def test_a_value_outside_0_and_1_is_refused_with_a_message(value):
    from flash_hash_join_amd import api
    with pytest.raises(RuntimeError, match="mm_heavy_outer must be 0 or 1"):
        api.set_option("mm_heavy_outer", value)
    assert api.get_option("mm_heavy_outer") == 0
    api.set_option("mm_heavy_outer", 1)
    try:
        with pytest.raises(RuntimeError, match="mm_heavy_outer must be 0 or 1"):
            api.set_option("mm_heavy_outer", value)
        assert api.get_option("mm_heavy_outer") == 1                            # a refused value leaves what was there
    finally:
        api.set_option("mm_heavy_outer", 0)


def test_mm_heavy_keys_still_refuses_2():
    from flash_hash_join_amd import api
    with pytest.raises(RuntimeError, match="mm_heavy_keys must be 0 or 1"):
        api.set_option("mm_heavy_keys", 2)
    assert api.get_option("mm_heavy_keys") == 0 and api.get_option("mm_heavy_outer") == 0


def test_fj_options_in_the_environment_sets_it():
    code = ("from flash_hash_join_amd import api; "
            "print('opt', api.get_option('mm_heavy_outer'), api.get_option('mm_heavy_keys'))")
    for env_value, want in (("mm_heavy_outer=1", 1), ("mm_heavy_outer=0", 0), ("mm_heavy_outer=2", 0)):
        out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=ROOT,
                             env=product_env(FJ_OPTIONS=env_value))
        assert out.returncode == 0, out.stderr
        assert f"opt {want} 0" in out.stdout, (env_value, out.stdout, out.stderr)
        assert ("ignoring" in out.stderr) == (env_value == "mm_heavy_outer=2"), out.stderr


def test_the_documents_name_the_option_and_the_abi_version_stays():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    assert '"mm_heavy_outer"' in hdr and '"mm_heavy_keys"' in hdr
    assert int(re.search(r"#define FJ_LDS_RETRIES_MM_TILED (\d+)", hdr).group(1)) == TILED
    from flash_hash_join_amd import _lib, api
    assert _lib.load().fj_abi_version() == 8
    assert len(_lib.SYMBOLS) == 40
    for doc in ("README.md", "DESIGN.md", os.path.join("tools", "README.md"), os.path.join("flash_hash_join_amd", "csrc", "fj_host.h")):
        assert "mm_heavy_outer" in open(os.path.join(ROOT, doc)).read(), doc
    for fn in (api.set_option, api.left_join, api.full_join, api.join_indices):
        assert "mm_heavy_outer" in fn.__doc__, fn


CASE_COUNTS = {          # nb, np, P, u, r - computed with NumPy
    "refusal": (6500, 3, 6001, 1, 499),
    "hot_key": (300_000, 30_040, 4_059_389, 15_288, 148_880),
    "empty_marker": (300_000, 30_040, 4_059_389, 15_288, 148_880),
    "hot_key_absent": (300_000, 30_000, 59_389, 15_288, 248_880),
    "colliding": (126_159, 40_600, 1_328_020, 19_930, 81_826),
    "zipf": (1_000_000, 1500, 12_139_596, 248, 601_853),
}


def case_input(name):
    if name == "refusal":
        return refusal_input()
    if name == "hot_key":
        return hot_key_input(HOT)
    if name == "empty_marker":
        return hot_key_input(keymix.EMPTY_RAW)
    if name == "hot_key_absent":
        return hot_key_absent_input()
    if name == "colliding":
        return colliding_input()[:3]
    if name == "zipf":
        return zipf_input()
    if name == "crowded":
        return crowded_input()[:3]
    raise KeyError(name)


def heavy_group(bk):
    """The largest number of build rows that share the top 12 bits of hash word 1 (a final partition of every plan of <= 12 bits)."""
    return int(np.bincount((keymix.hash_w1(bk) >> np.uint32(20)).astype(np.int64)).max())


@pytest.mark.parametrize("name", list(CASE_COUNTS))
def test_the_inputs_are_heavy_and_their_counts_are_the_stated_ones(name):
    from oracle.oracle import np_inner_join
    bk, bv, pk = case_input(name)
    nb, n_p, P, u, r = CASE_COUNTS[name]
    assert (bk.size, pk.size) == (nb, n_p)
    assert max_multiplicity(bk) > LIMIT or heavy_group(bk) > LIMIT
    assert np_inner_join(bk, bv, pk) == P and 0 < P <= MAX_PAIRS
    assert int((~np.isin(pk, bk)).sum()) == u and int((~np.isin(bk, pk)).sum()) == r
    if name == "empty_marker":
        assert int(keymix.mix(np.array([keymix.EMPTY_RAW], dtype=np.uint64))[0]) == 2**64 - 1
    if name == "hot_key_absent":
        assert int((bk == np.uint64(HOT)).sum()) == 100_000 and not np.any(pk == np.uint64(HOT))


def check_crowded(bk, bv, pk, group, on_build):
    from oracle.oracle import np_inner_join
    hot = np.uint64(HOT)
    part = lambda a: keymix.hash_w1(a) >> np.uint32(20)
    hp = part(np.array([hot], dtype=np.uint64))[0]
    assert group.size >= 400 and np.all(part(group) == hp)
    in_part_b = bk[part(bk) == hp]
    assert in_part_b.size > 100_000 > LIMIT and max_multiplicity(bk) == 100_000
    probe_keys = np.unique(pk[part(pk) == hp])
    matching = probe_keys[np.isin(probe_keys, bk) & (probe_keys != hot)]
    missing = probe_keys[~np.isin(probe_keys, bk)]
    assert matching.size >= 100 and missing.size >= 100, (matching.size, missing.size)
    assert np.isin(on_build, bk).all() and hot in probe_keys
    assert 0 < np_inner_join(bk, bv, pk) <= MAX_PAIRS


def test_the_crowded_partition_is_crowded():
    check_crowded(*crowded_input())


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


@pytest.fixture
def heavy(fj):
    """mm_heavy_outer = 1 and mm_heavy_keys = 0 for the length of a test; both are 0 afterwards."""
    fj.set_option("mm_heavy_keys", 0)
    fj.set_option("mm_heavy_outer", 1)
    try:
        yield fj
    finally:
        fj.set_option("mm_heavy_outer", 0)
        fj.set_option("mm_heavy_keys", 0)


def to_device(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in arrays)


def check_row_ids(bk, pk, P, u, r, pi, bi, full):
    pi, bi = host(pi).view(np.int64), host(bi).view(np.int64)
    assert pi.size == P + u + r and bi.size == P + u + r
    assert np.all(pi[:P + u] >= 0) and np.all(pi[:P + u] < pk.size) and np.all(bi[:P] >= 0) and np.all(bi[:P] < bk.size)
    assert np.array_equal(pk[pi[:P]], bk[bi[:P]]), "a pair's keys differ"
    assert np.unique(pi[:P].astype(np.uint64) * np.uint64(bk.size) + bi[:P].astype(np.uint64)).size == P, "a (probe row, build row) pair appears twice"
    assert np.all(bi[P:P + u] == -1) and np.all(pi[P + u:] == -1)
    assert np.array_equal(np.sort(pi[P:P + u]), np.flatnonzero(~np.isin(pk, bk))), "second range: not every unmatched probe position exactly once"
    if full:
        assert np.array_equal(np.sort(bi[P + u:]), np.flatnonzero(~np.isin(bk, pk))), "third range: not every unmatched build position exactly once"


def calls(fj, args, fill=0):
    return (lambda: fj.left_join(*args, return_arrays=True, fill_value=fill, duplicates="all"),
            lambda: fj.full_join(*args, return_arrays=True, fill_value=fill, duplicates="all"),
            lambda: fj.join_indices(args[0], args[2], how="left", duplicates="all"),
            lambda: fj.join_indices(args[0], args[2], how="full", duplicates="all"))


def check_all_forms(fj, bk, bv, pk, device, counts=None, fill=0):
    """left / full, keys-values / row ids, against the reference with mm_heavy_outer = 1 (the caller set it); before anything runs:
    the input is heavy, 0 < P <= 20M, and the same calls at 0 are refused and leave the context usable."""
    assert max_multiplicity(bk) > LIMIT or heavy_group(bk) > LIMIT
    P_exp, ek, ev, anti_exp, rk_exp, rv_exp = np_ref(bk, bv, pk)
    u_exp, r_exp = anti_exp.size, rk_exp.size
    if counts is not None:
        assert (P_exp, u_exp, r_exp) == counts
    args = to_device(bk, bv, pk) if device else (bk, bv, pk)
    fj.set_option("mm_heavy_outer", 0)
    try:
        for call in calls(fj, args):
            with pytest.raises(RuntimeError, match="4096 build rows"):
                call()
        with pytest.raises(RuntimeError, match="4096 build rows"):           # (mm_heavy_keys is 0 too)
            fj.inner_join_count(*args)
        m = fj.left_join(*args)[0]                                              # an N:1 left join on the same context
        assert m == int(np.isin(pk, bk).sum())
    finally:
        fj.set_option("mm_heavy_outer", 1)
    left, full, left_ids, full_ids = calls(fj, args, fill)
    # ---- left, keys / values ----
    P, u, _, keys, vals = left()
    lt = fj.last_timings()
    keys, vals = host(keys), host(vals)
    print(f"left(all): P={P} ({P_exp}) u={u} ({u_exp}) rows={keys.size} lds_retries={lt['lds_retries']} join_ms={lt['join_ms']:.3f} emit_ms={lt['emit_ms']:.3f}")
    assert (P, u) == (P_exp, u_exp) and keys.size == P + u and vals.size == P + u
    assert lt["lds_retries"] == TILED and lt["fell_back"] == 0 and lt["path"] == 0, lt
    assert same_pairs(keys[:P], vals[:P], ek, ev), "left: rows [0, P) differ from np_inner_join"
    assert np.array_equal(srt(keys[P:]), srt(anti_exp)) and np.all(vals[P:] == np.uint64(fill))
    assert fj.left_join(*args, duplicates="all")[:2] == (P, u)
    # ---- full, keys / values ----
    P, u, r, _, keys, vals = full()
    lt = fj.last_timings()
    keys, vals = host(keys), host(vals)
    print(f"full(all): P={P} ({P_exp}) u={u} ({u_exp}) r={r} ({r_exp}) rows={keys.size} lds_retries={lt['lds_retries']} join_ms={lt['join_ms']:.3f} emit_ms={lt['emit_ms']:.3f}")
    assert (P, u, r) == (P_exp, u_exp, r_exp) and keys.size == P + u + r and vals.size == P + u + r
    assert lt["lds_retries"] == TILED
    assert same_pairs(keys[:P], vals[:P], ek, ev), "full: rows [0, P) differ from np_inner_join"
    assert np.array_equal(srt(keys[P:P + u]), srt(anti_exp)) and np.all(vals[P:P + u] == np.uint64(fill))
    third = np.lexsort((vals[P + u:], keys[P + u:]))
    ref3 = np.lexsort((rv_exp, rk_exp))
    assert np.array_equal(keys[P + u:][third], rk_exp[ref3]) and np.array_equal(vals[P + u:][third], rv_exp[ref3]), "full: third range differs"
    assert fj.full_join(*args, duplicates="all")[:3] == (P, u, r)
    # ---- row ids ----
    P, u, _, pi, bi = left_ids()
    assert (P, u) == (P_exp, u_exp) and fj.last_timings()["lds_retries"] == TILED
    check_row_ids(bk, pk, P, u, 0, pi, bi, full=False)
    assert same_pairs(pk[host(pi)[:P].astype(np.int64)], bv[host(bi)[:P].astype(np.int64)], ek, ev)      # (bv = row id)
    P, u, r, _, pi, bi = full_ids()
    assert (P, u, r) == (P_exp, u_exp, r_exp)
    check_row_ids(bk, pk, P, u, r, pi, bi, full=True)
    assert same_pairs(pk[host(pi)[:P].astype(np.int64)], bv[host(bi)[:P].astype(np.int64)], ek, ev)
    # ---- the context afterwards: an inner join (refused: mm_heavy_keys is 0) and an N:1 left join ----
    with pytest.raises(RuntimeError, match="4096 build rows"):
        fj.inner_join_count(*args)
    assert fj.left_join(*args)[0] == m


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("name", list(CASE_COUNTS))
def test_parity_with_the_numpy_reference(fj, heavy, name, device):
    bk, bv, pk = case_input(name)
    nb, n_p, P, u, r = CASE_COUNTS[name]
    assert (bk.size, pk.size) == (nb, n_p)
    check_all_forms(fj, bk, bv, pk, device, counts=(P, u, r), fill=0 if name != "hot_key" else 2**64 - 3)
    if name == "colliding":
        assert fj.last_timings()["radix_bits"] <= 12


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_a_crowded_partition_gets_its_verdicts_across_the_tiles(fj, heavy, device):
    bk, bv, pk, group, on_build = crowded_input()
    check_crowded(bk, bv, pk, group, on_build)
    check_all_forms(fj, bk, bv, pk, device)
    assert fj.last_timings()["radix_bits"] <= 12                                # (what "share a final partition" rests on)


@pytest.mark.gpu
def test_dlpack_inputs(fj, heavy):
    import torch

    class Capsule:                                                              # a DLPack exporter that is not a tensor
        def __init__(self, t):
            self.t = t

        def __dlpack__(self, stream=None):
            return self.t.__dlpack__() if stream is None else self.t.__dlpack__(stream=stream)

        def __dlpack_device__(self):
            return self.t.__dlpack_device__()

    bk, bv, pk = refusal_input()
    P_exp, ek, ev, anti_exp, rk_exp, rv_exp = np_ref(bk, bv, pk)
    args = tuple(Capsule(t) for t in to_device(bk, bv, pk))
    P, u, r, _, keys, vals = fj.full_join(*args, return_arrays=True, fill_value=9, duplicates="all")
    keys, vals = host(keys), host(vals)
    assert (P, u, r) == (6001, 1, 499) and keys.size == 6501
    assert same_pairs(keys[:P], vals[:P], ek, ev)
    assert np.array_equal(srt(keys[P:P + u]), srt(anti_exp)) and np.all(vals[P:P + u] == 9)
    assert same_pairs(keys[P + u:], vals[P + u:], rk_exp, rv_exp)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", [LEFT | ALL, FULL | ALL, FULL | ALL | ROW_IDS | RADIX], ids=["left", "full", "full_row_ids"])
def test_two_phase_form_of_the_c_abi(fj, heavy, algo):
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    bk, bv, pk = hot_key_input(HOT)
    assert max_multiplicity(bk) > LIMIT
    P_exp, ek, ev, anti_exp, rk_exp, rv_exp = np_ref(bk, bv, pk)
    u_exp, r_exp = anti_exp.size, (rk_exp.size if algo & FULL else 0)
    rows = P_exp + u_exp + r_exp
    dbk, dbv, dpk = to_device(bk, bv, pk)
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream

    def join(cnt, ok=None, ov=None, cap=0, t=None):
        return L.fj_join_device(ctx, algo, 0, 1, dbk.data_ptr(), dbv.data_ptr(), bk.size, dpk.data_ptr(), pk.size, stream, 64, cnt,
                                ok.data_ptr() if ok is not None else None, ov.data_ptr() if ov is not None else None, cap,
                                ctypes.byref(t) if t is not None else None)

    def check(k, v):
        k, v = host(k), host(v)
        if algo & ROW_IDS:
            check_row_ids(bk, pk, P_exp, u_exp, r_exp, k, v, full=bool(algo & FULL))
            return
        assert same_pairs(k[:P_exp], v[:P_exp], ek, ev)
        assert np.array_equal(srt(k[P_exp:P_exp + u_exp]), srt(anti_exp)) and np.all(v[P_exp:P_exp + u_exp] == 0)
        if algo & FULL:
            assert same_pairs(k[P_exp + u_exp:], v[P_exp + u_exp:], rk_exp, rv_exp)
        else:
            assert k.size == P_exp + u_exp

    cnt = (ctypes.c_uint64 * 3)(7, 7, 7)
    t = _lib.FjTimings()
    _lib.check(join(cnt, t=t))                                                  # counted, rows pending
    assert (int(cnt[0]), int(cnt[1]), int(cnt[2])) == (P_exp, r_exp, u_exp) and t.lds_retries == TILED
    ok = torch.full((rows + 1,), 12345, dtype=torch.int64, device="cuda")
    ov = torch.full((rows + 1,), 12345, dtype=torch.int64, device="cuda")
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows - 1, stream, None) != 0          # one row too few: refused ...
    assert "output capacity" in _lib.last_error()
    _lib.check(L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows, stream, ctypes.byref(t)))     # ... and still pending
    assert t.emit_ms > 0
    assert int(ok[rows]) == 12345 and int(ov[rows]) == 12345, "a row behind the result was written"
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows, stream, None) != 0
    assert "no counted materialising join is pending" in _lib.last_error()
    check(ok[:rows], ov[:rows])
    # one call, enough capacity
    ok2 = torch.full((rows + 5,), 12345, dtype=torch.int64, device="cuda")
    ov2 = torch.full((rows + 5,), 12345, dtype=torch.int64, device="cuda")
    cnt2 = (ctypes.c_uint64 * 3)(0, 0, 0)
    _lib.check(join(cnt2, ok2, ov2, rows + 5))
    assert list(cnt2) == list(cnt)
    assert bool((ok2[rows:] == 12345).all()) and bool((ov2[rows:] == 12345).all())
    check(ok2[:rows], ov2[:rows])
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows, stream, None) != 0               # nothing pending after it
    # one call, too little capacity: the counts are there, the rows stay pending for fj_emit_pairs
    cnt3 = (ctypes.c_uint64 * 3)(0, 0, 0)
    assert join(cnt3, ok2, ov2, rows - 1) != 0
    assert "output capacity" in _lib.last_error() and list(cnt3) == list(cnt)
    ok2.fill_(12345); ov2.fill_(12345)
    _lib.check(L.fj_emit_pairs(ctx, ok2.data_ptr(), ov2.data_ptr(), rows, stream, None))
    check(ok2[:rows], ov2[:rows])
    # the next call that starts work drops a pending result
    _lib.check(join(cnt3))
    assert fj.hash_join_count_radix(dbk, dbv, dpk)[0] == int(np.isin(pk, bk).sum())
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows, stream, None) != 0
    assert "no counted materialising join is pending" in _lib.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_lds_retries_reports_the_tiled_path_and_nothing_else_does(fj, heavy, device):
    bk, bv, pk = refusal_input()
    args = to_device(bk, bv, pk) if device else (bk, bv, pk)
    assert fj.left_join(*args, duplicates="all")[:2] == (6001, 1) and fj.last_timings()["lds_retries"] == TILED
    assert fj.full_join(*args, duplicates="all")[:3] == (6001, 1, 499) and fj.last_timings()["lds_retries"] == TILED
    # a many-to-many input no partition of which is beyond the table (the 60 000-row case of tests/test_gpu_parity.py): 0 at either
    # setting, and the same rows
    rng = np.random.default_rng(60007)
    bk = rng.integers(0, 9000, size=60000, dtype=np.uint64) * GOLDEN
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = rng.integers(0, 18001, size=300000, dtype=np.uint64) * GOLDEN
    assert max_multiplicity(bk) < 100
    P_exp, ek, ev, anti_exp, rk_exp, rv_exp = np_ref(bk, bv, pk)
    args = to_device(bk, bv, pk) if device else (bk, bv, pk)
    seen = []
    for setting in (0, 1, 0):
        fj.set_option("mm_heavy_outer", setting)
        P, u, r, _, keys, vals = fj.full_join(*args, return_arrays=True, duplicates="all")
        assert fj.last_timings()["lds_retries"] == 0
        keys, vals = host(keys), host(vals)
        assert (P, u, r) == (P_exp, anti_exp.size, rk_exp.size)
        assert same_pairs(keys[:P], vals[:P], ek, ev) and np.array_equal(srt(keys[P:P + u]), srt(anti_exp))
        assert same_pairs(keys[P + u:], vals[P + u:], rk_exp, rv_exp)
        P2, u2, _, k2, v2 = fj.left_join(*args, return_arrays=True, duplicates="all")
        assert (P2, u2) == (P, u) and fj.last_timings()["lds_retries"] == 0
        o1, o2, o3 = (np.lexsort((vals[a:b], keys[a:b])) for a, b in ((0, P), (P, P + u), (P + u, P + u + r)))
        seen.append((keys[:P][o1], vals[:P][o1], keys[P:P + u][o2], keys[P + u:][o3], vals[P + u:][o3]))
    for other in seen[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(seen[0], other))


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_the_two_options_are_independent(fj, heavy, device):
    bk, bv, pk = refusal_input()
    args = to_device(bk, bv, pk) if device else (bk, bv, pk)
    assert (fj.get_option("mm_heavy_outer"), fj.get_option("mm_heavy_keys")) == (1, 0)
    for call in (lambda: fj.inner_join_count(*args), lambda: fj.inner_join(*args, return_arrays=True),
                 lambda: fj.join_indices(args[0], args[2], how="inner", many_to_many=True)):
        with pytest.raises(RuntimeError, match="4096 build rows"):
            call()
    assert fj.full_join(*args, duplicates="all")[:3] == (6001, 1, 499)
    fj.set_option("mm_heavy_outer", 0)
    fj.set_option("mm_heavy_keys", 1)
    for call in calls(fj, args):
        with pytest.raises(RuntimeError, match="4096 build rows"):
            call()
    assert fj.inner_join_count(*args)[0] == 6001
    assert fj.left_join(*args)[0] == 2
