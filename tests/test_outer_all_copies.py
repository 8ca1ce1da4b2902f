"""Left and full outer joins that keep every copy of a duplicated build key (FJ_ALGO_ALL_COPIES, csrc/fj_many.hip;
duplicates="all" in Python): the C-ABI contract and argument checks that need no GPU, and - on an MI355X - exact parity with the
NumPy reference on zero-, one-, two-pass and deep plans, a build side far larger than the probe side, the row-id form, the N:1
joins on unique build keys, the counting joins, the two-phase form of the C ABI, the 4096-rows limit and empty sides.

Reference (integers, compared exactly as sorted multisets per range): oracle.np_inner_join for rows [0, P),
pk[~np.isin(pk, bk)] for rows [P, P + u), (bk, bv)[~np.isin(bk, pk)] for rows [P + u, P + u + r)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import keymix
from conftest import ROOT

U64_MAX = np.uint64(2**64 - 1)
MANY, LEFT, ANTI, ROW_IDS, FULL, ALL = 0x10, 0x20, 0x40, 0x80, 0x100, 0x200
GOLDEN = np.uint64(0x9E3779B97F4A7C15)


def _np_ref(bk, bv, pk):
    """(P, pair keys, pair values, unmatched probe keys, unmatched build keys, their values) of the NumPy reference."""
    from oracle.oracle import np_inner_join
    bk, bv, pk = (np.asarray(x, dtype=np.uint64) for x in (bk, bv, pk))
    P, k, v = np_inner_join(bk, bv, pk, return_arrays=True)
    rest = ~np.isin(bk, pk)
    return P, k, v, pk[~np.isin(pk, bk)], bk[rest], bv[rest]


def _same_pairs(k1, v1, k2, v2):
    from oracle.oracle import canon_pairs
    a = canon_pairs(np.asarray(k1).view(np.uint64), np.asarray(v1).view(np.uint64))
    b = canon_pairs(np.asarray(k2).view(np.uint64), np.asarray(v2).view(np.uint64))
    return a[0].size == b[0].size and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _sorted(a):
    return np.sort(np.asarray(a).reshape(-1).view(np.uint64))


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_header_flag_python_mirror_and_the_duplicates_parameter():
    hdr = open(os.path.join(ROOT, "include", "flashjoin.h")).read()
    assert int(re.search(r"#define FJ_ALGO_ALL_COPIES (0x[0-9a-fA-F]+)", hdr).group(1), 16) == 0x200
    assert int(re.search(r"#define FJ_ABI_VERSION (\d+)", hdr).group(1)) == 8
    from flash_hash_join_amd import api
    import flash_join
    assert api.ALGO_ALL_COPIES == 0x200
    for fn in (api.left_join, api.full_join, api.join_indices, flash_join.left_join, flash_join.full_join, flash_join.join_indices):
        assert inspect.signature(fn).parameters["duplicates"].default == "first", fn


DEVICE_REFUSALS = [   # id, algo, materialize, out_count given, misalignment, build values, needles
    ("bare_flag", ALL, 1, True, 0, 0x20000, ("unknown algo", "FJ_ALGO_LEFT_OUTER", "FJ_ALGO_MANY_TO_MANY")),
    ("bare_flag_radix", ALL | 2, 1, True, 0, 0x20000, ("unknown algo", "FJ_ALGO_FULL_OUTER")),
    ("bare_flag_row_ids", ALL | ROW_IDS, 1, True, 0, None, ("unknown algo",)),
    ("anti", ALL | ANTI, 1, True, 0, 0x20000, ("FJ_ALGO_ANTI", "no copies")),
    ("left_anti", ALL | LEFT | ANTI, 1, True, 0, 0x20000, ("FJ_ALGO_ANTI",)),
    ("left_many", ALL | LEFT | MANY, 1, True, 0, 0x20000, ("MANY_TO_MANY",)),
    ("full_many", ALL | FULL | MANY | 2, 1, True, 0, 0x20000, ("MANY_TO_MANY",)),
    ("left_full", ALL | LEFT | FULL, 1, True, 0, 0x20000, ("cannot be combined",)),
    ("left_count", ALL | LEFT, 0, True, 0, 0x20000, ("needs materialize = 1",)),
    ("full_count", ALL | FULL | 1, 0, True, 0, 0x20000, ("needs materialize = 1",)),
    ("left_rid_count", ALL | LEFT | ROW_IDS, 0, True, 0, None, ("needs materialize = 1",)),
    ("left_no_count", ALL | LEFT, 1, False, 0, 0x20000, ("out_count",)),
    ("full_no_count", ALL | FULL, 1, False, 0, 0x20000, ("out_count",)),
    ("left_misaligned", ALL | LEFT, 1, True, 4, 0x20000, ("8-byte aligned",)),
    ("full_misaligned", ALL | FULL | ROW_IDS, 1, True, 4, None, ("8-byte aligned",)),
    ("left_null_build_vals", ALL | LEFT, 1, True, 0, None, ("d_build_vals",)),
    ("full_null_build_vals", ALL | FULL | 2, 1, True, 0, None, ("d_build_vals",)),
    ("left_base_9", ALL | LEFT | 9, 1, True, 0, 0x20000, ("unknown algo",)),
]


@pytest.mark.parametrize("cid,algo,materialize,with_count,misalign,bv,needles", DEVICE_REFUSALS, ids=[r[0] for r in DEVICE_REFUSALS])
def test_invalid_combinations_are_refused_before_any_device_work(cid, algo, materialize, with_count, misalign, bv, needles):
    """A NULL context: the checks come before the context is touched (no GPU needed; the pointers are never dereferenced)."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    cnt = (ctypes.c_uint64 * 3)(0, 0, 0)
    rc = L.fj_join_device(None, algo, 0, materialize, 0x10000, bv, 100, 0x30000, 1000, None, 64, cnt if with_count else None,
                          0x40000 + misalign, 0x50000, 10**6, None)
    assert rc != 0
    err = _lib.last_error()
    assert "null context" not in err, err
    for needle in needles:
        assert needle in err, err


def test_what_is_refused_today_keeps_its_text():
    from flash_hash_join_amd import _lib
    L = _lib.load()
    cnt = (ctypes.c_uint64 * 3)(0, 0, 0)
    for algo, needle in ((LEFT | MANY, "FJ_ALGO_LEFT_OUTER cannot be combined with FJ_ALGO_MANY_TO_MANY"),
                         (ANTI | MANY, "FJ_ALGO_ANTI cannot be combined with FJ_ALGO_MANY_TO_MANY"),
                         (FULL | MANY, "FJ_ALGO_FULL_OUTER cannot be combined with FJ_ALGO_MANY_TO_MANY"),
                         (FULL | LEFT, "FJ_ALGO_FULL_OUTER cannot be combined with FJ_ALGO_LEFT_OUTER"),
                         (LEFT | ANTI, "FJ_ALGO_LEFT_OUTER and FJ_ALGO_ANTI cannot be combined"),
                         (0x400, "unknown algo 1024")):
        assert L.fj_join_device(None, algo, 0, 1, 0x10000, 0x20000, 100, 0x30000, 1000, None, 64, cnt, 0x40000, 0x50000, 1100, None) != 0
        assert needle in _lib.last_error(), _lib.last_error()


def test_valid_combinations_reach_the_context():
    """Also without output buffers (the counting half of the two-phase form) and, with row ids, without build values."""
    from flash_hash_join_amd import _lib
    L = _lib.load()
    cnt = (ctypes.c_uint64 * 3)(0, 0, 0)
    for algo, bv in ((LEFT | ALL, 0x20000), (FULL | ALL, 0x20000), (LEFT | ALL | ROW_IDS, 0x20000), (FULL | ALL | ROW_IDS, 0x20000),
                     (LEFT | ALL | ROW_IDS, None), (FULL | ALL | ROW_IDS, None), (LEFT | ALL | 1, 0x20000), (FULL | ALL | 2, 0x20000)):
        for ok, ov, cap in ((0x40000, 0x50000, 20), (None, None, 0)):
            assert L.fj_join_device(None, algo, 1, 1, 0x10000, bv, 10, 0x30000, 10, None, 64, cnt, ok, ov, cap, None) != 0
            assert "null context" in _lib.last_error(), (hex(algo), _lib.last_error())


@pytest.mark.parametrize("algo,materialize,bv,with_count,needles", [
    (ALL, 1, True, True, ("unknown algo", "FJ_ALGO_MANY_TO_MANY")),
    (ALL | ROW_IDS | 2, 1, True, True, ("unknown algo",)),
    (ALL | ANTI, 1, True, True, ("FJ_ALGO_ANTI",)),
    (ALL | LEFT | ANTI, 1, True, True, ("FJ_ALGO_ANTI",)),
    (ALL | LEFT | MANY, 1, True, True, ("MANY_TO_MANY",)),
    (ALL | FULL | MANY, 1, True, True, ("MANY_TO_MANY",)),
    (ALL | LEFT | FULL, 1, True, True, ("cannot be combined",)),
    (ALL | LEFT, 0, True, True, ("needs materialize = 1",)),
    (ALL | FULL, 0, True, True, ("needs materialize = 1",)),
    (ALL | LEFT, 1, False, True, ("build values",)),
    (ALL | FULL, 1, False, True, ("build values",)),
    (ALL | LEFT, 1, True, False, ("out_count",)),
    (ALL | FULL, 1, True, False, ("out_count",)),
    (ALL | LEFT | 9, 1, True, True, ("unknown algo",)),
], ids=["bare_flag", "bare_flag_row_ids", "anti", "left_anti", "left_many", "full_many", "left_full", "left_count", "full_count",
        "left_no_build_values", "full_no_build_values", "left_no_count", "full_no_count", "left_base_9"])
def test_host_entry_refusals(algo, materialize, bv, with_count, needles):
    from flash_hash_join_amd import _lib
    L = _lib.load()
    a = np.arange(16, dtype=np.uint64)
    cnt = (ctypes.c_uint64 * 3)(0, 0, 0)
    sec = ctypes.c_double(0)
    rc = L.fj_join_host(algo, 0, materialize, a.ctypes.data, a.ctypes.data if bv else None, a.size, a.ctypes.data, a.size,
                        cnt if with_count else None, ctypes.byref(sec), None, None)
    assert rc != 0
    for needle in needles:
        assert needle in _lib.last_error(), _lib.last_error()


def test_python_argument_errors():
    import flash_join
    a = np.arange(4, dtype=np.uint64)
    with pytest.raises(ValueError, match="duplicates"):
        flash_join.left_join(a, a, a, duplicates="bogus")
    with pytest.raises(ValueError, match="duplicates"):
        flash_join.full_join(a, a, a, return_arrays=True, duplicates="bogus")
    for how in ("inner", "left", "full", "semi", "anti"):
        with pytest.raises(ValueError, match="duplicates"):
            flash_join.join_indices(a, a, how=how, duplicates="bogus")
    for how in ("left", "full", "semi", "anti"):                   # pinned before this flag existed, with and without it
        for dup in ("first", "all"):
            with pytest.raises(ValueError, match="many_to_many"):
                flash_join.join_indices(a, a, how=how, many_to_many=True, duplicates=dup)


def test_numpy_reference_on_a_hand_written_case():
    # 7: duplicated and matched (by a repeated probe key); 8: duplicated and unmatched; 0 and 2**64 - 1 on both sides; 9 and 6: build only
    bk = np.array([5, 7, 7, 9, 2**64 - 1, 0, 8, 8, 6], dtype=np.uint64)
    bv = np.array([50, 70, 71, 90, 11, 1, 80, 81, 60], dtype=np.uint64)
    pk = np.array([7, 3, 5, 7, 2**64 - 1, 4, 0, 3], dtype=np.uint64)
    P, k, v, anti, rk, rv = _np_ref(bk, bv, pk)
    assert P == 7
    assert sorted(zip(k.tolist(), v.tolist())) == [(0, 1), (5, 50), (7, 70), (7, 70), (7, 71), (7, 71), (2**64 - 1, 11)]
    assert sorted(anti.tolist()) == [3, 3, 4]
    assert sorted(zip(rk.tolist(), rv.tolist())) == [(6, 60), (8, 80), (8, 81), (9, 90)]          # every copy of key 8
    # keys 0 and 2**64 - 1 on the build side only: they move to the third range
    P2, _, _, anti2, rk2, rv2 = _np_ref(bk, bv, pk[(pk != 0) & (pk != U64_MAX)])
    assert P2 == 5 and sorted(anti2.tolist()) == [3, 3, 4]
    assert {(0, 1), (2**64 - 1, 11)} <= set(zip(rk2.tolist(), rv2.tolist())) and rk2.size == 6


# ---- GPU -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    return flash_join


def _mm_case(nb, dom, npk):
    """The input family of test_many_to_many_extension_matches_the_numpy_oracle (tests/test_gpu_parity.py): duplicates on both
    sides, about half of the probe rows without a partner; raw 2^64 - 1 (the HBM table's empty marker, an ordinary key in the hash
    domain), 0, the LDS tables' empty marker (keymix.EMPTY_RAW) and the wide kernel's filler as duplicated keys."""
    rng = np.random.default_rng(nb + 7)
    ids = rng.integers(0, dom, size=nb, dtype=np.uint64)
    bk = ids * GOLDEN
    bk[ids == 1] = U64_MAX
    bk[ids == 2] = keymix.EMPTY_RAW
    bk[ids == 3] = keymix.FILLER_RAW
    bv = np.arange(nb, dtype=np.uint64) + np.uint64(5 * 10**12)               # value = row id: every row distinguishable
    pids = rng.integers(0, 2 * dom + 1, size=npk, dtype=np.uint64)
    pk = pids * GOLDEN
    pk[pids == 1] = U64_MAX
    pk[pids == 2] = keymix.EMPTY_RAW
    pk[pids == 3] = keymix.FILLER_RAW
    return bk, bv, pk


def _host(a):
    return a.cpu().numpy().view(np.uint64) if hasattr(a, "cpu") else np.asarray(a).view(np.uint64)


def _to_device(*arrays):
    import torch
    return tuple(torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda() for a in arrays)


def _check_row_ids(bk, pk, P, u, r, pi, bi, full=True):
    """The gather maps are usable and complete (full=False: a left join, no third range)."""
    pi, bi = _host(pi).view(np.int64), _host(bi).view(np.int64)
    assert pi.size == P + u + r and bi.size == P + u + r
    assert np.all(pi[:P + u] >= 0) and np.all(pi[:P + u] < max(pk.size, 1)) and np.all(bi[:P] >= 0) and np.all(bi[:P] < max(bk.size, 1))
    assert np.array_equal(pk[pi[:P]], bk[bi[:P]]), "a pair's keys differ"
    assert np.all(bi[P:P + u] == -1) and np.all(pi[P + u:] == -1)
    assert np.all(~np.isin(pk[pi[P:P + u]], bk)), "a probe row in the second range has a partner"
    sk = np.sort(bk)
    mult = np.searchsorted(sk, pk, side="right") - np.searchsorted(sk, pk, side="left")
    assert np.array_equal(np.bincount(pi[:P + u], minlength=pk.size), np.maximum(1, mult)), "a probe position does not appear max(1, multiplicity) times"
    if P:
        pairs = np.unique(np.stack([pi[:P], bi[:P]]), axis=1)
        assert pairs.shape[1] == P, "a (probe row, build row) pair appears twice"
    if full:
        assert np.array_equal(np.sort(bi[P + u:]), np.flatnonzero(~np.isin(bk, pk))), "third range: not every build position of an unmatched key exactly once"


def _check(fj, bk, bv, pk, device, fill=0):
    P_exp, ek, ev, anti_exp, rk_exp, rv_exp = _np_ref(bk, bv, pk)
    u_exp, r_exp = anti_exp.size, rk_exp.size
    args = _to_device(bk, bv, pk) if device else (bk, bv, pk)
    # ---- left, keys / values ----
    P, u, _, keys, vals = fj.left_join(*args, return_arrays=True, fill_value=fill, duplicates="all")
    keys, vals = _host(keys), _host(vals)
    print(f"left_join(all): P={P} (expected {P_exp}) u={u} (expected {u_exp}) rows={keys.size}")
    assert (P, u) == (P_exp, u_exp) and keys.size == P + u and vals.size == P + u
    assert _same_pairs(keys[:P], vals[:P], ek, ev), "left: rows [0, P) differ from np_inner_join"
    assert np.array_equal(_sorted(keys[P:]), _sorted(anti_exp)) and np.all(vals[P:] == np.uint64(fill))
    assert fj.left_join(*args, duplicates="all")[:2] == (P, u)
    # ---- full, keys / values ----
    P, u, r, _, keys, vals = fj.full_join(*args, return_arrays=True, fill_value=fill, duplicates="all")
    keys, vals = _host(keys), _host(vals)
    print(f"full_join(all): P={P} (expected {P_exp}) u={u} (expected {u_exp}) r={r} (expected {r_exp}) rows={keys.size}")
    assert (P, u, r) == (P_exp, u_exp, r_exp) and keys.size == P + u + r and vals.size == P + u + r
    assert _same_pairs(keys[:P], vals[:P], ek, ev), "full: rows [0, P) differ from np_inner_join"
    assert np.array_equal(_sorted(keys[P:P + u]), _sorted(anti_exp)) and np.all(vals[P:P + u] == np.uint64(fill))
    assert _same_pairs(keys[P + u:], vals[P + u:], rk_exp, rv_exp), "full: third range differs from (bk, bv)[~isin(bk, pk)]"
    assert fj.full_join(*args, duplicates="all")[:3] == (P, u, r)
    # ---- row ids ----
    P, u, _, pi, bi = fj.join_indices(args[0], args[2], how="left", duplicates="all")
    assert (P, u) == (P_exp, u_exp)
    _check_row_ids(bk, pk, P, u, 0, pi, bi, full=False)
    P, u, r, _, pi, bi = fj.join_indices(args[0], args[2], how="full", duplicates="all")
    assert (P, u, r) == (P_exp, u_exp, r_exp)
    _check_row_ids(bk, pk, P, u, r, pi, bi)


MM_CASES = [(1, 1, 1), (300, 40, 2000), (5000, 700, 60000), (60000, 9000, 300000), (1_000_000, 400_000, 3_000_000),
            (6_000_000, 3_000_000, 5_000_000)]


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("nb,dom,npk", MM_CASES)
def test_parity_with_the_numpy_reference(fj, oracle, nb, dom, npk, device):
    bk, bv, pk = _mm_case(nb, dom, npk)
    assert fj.inner_join_count(bk, bv, pk)[0] == oracle.np_inner_join(bk, bv, pk)       # (the 4096-rows limit is not what is tested)
    _check(fj, bk, bv, pk, device, fill=0 if nb != 60000 else 2**64 - 3)
    t = fj.last_timings()
    assert t["path"] == 0 and t["fell_back"] == 0
    if nb >= 1_000_000:
        assert t["passes"] >= (2 if nb > 4_000_000 else 1)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_parity_on_a_deep_plan(fj, device):
    bk, bv, pk = _mm_case(60000, 9000, 300000)
    fj.set_option("plan_target_keys", 32)
    try:
        _check(fj, bk, bv, pk, device)
        assert fj.last_timings()["path"] == 0 and fj.last_timings()["passes"] >= 2
    finally:
        fj.set_option("plan_target_keys", 4096)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_a_build_side_far_larger_than_the_probe_side(fj, device):
    """1M build rows in ~500 partitions, 1 000 probe rows: most partitions have no work item, and all their rows belong in the third range."""
    bk, bv, _ = _mm_case(1_000_000, 400_000, 1)
    rng = np.random.default_rng(3)
    pk = np.concatenate([rng.choice(bk, 600), rng.integers(0, 2**64, size=400, dtype=np.uint64)])
    r_exp = int((~np.isin(bk, pk)).sum())
    assert r_exp > 990_000
    _check(fj, bk, bv, pk, device)


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_unique_build_keys_equal_the_first_occurrence_joins(fj, device):
    rng = np.random.default_rng(5)
    bk = np.unique(rng.integers(0, 2**64, size=300_000, dtype=np.uint64))
    rng.shuffle(bk)
    bv = rng.integers(0, 2**64, size=bk.size, dtype=np.uint64)
    pk = np.concatenate([rng.choice(bk[:bk.size // 2], 600_000), rng.integers(0, 2**64, size=600_000, dtype=np.uint64)])
    n_p = pk.size
    args = _to_device(bk, bv, pk) if device else (bk, bv, pk)
    m, _, k1, v1 = fj.left_join(*args, return_arrays=True, fill_value=9)
    P, u, _, k2, v2 = fj.left_join(*args, return_arrays=True, fill_value=9, duplicates="all")
    k1, v1, k2, v2 = (_host(x) for x in (k1, v1, k2, v2))
    assert (P, u) == (m, n_p - m) and k2.size == n_p
    assert _same_pairs(k1[:m], v1[:m], k2[:P], v2[:P]) and _same_pairs(k1[m:], v1[m:], k2[P:], v2[P:])
    m, r1, _, k1, v1 = fj.full_join(*args, return_arrays=True)
    P, u, r, _, k2, v2 = fj.full_join(*args, return_arrays=True, duplicates="all")
    k1, v1, k2, v2 = (_host(x) for x in (k1, v1, k2, v2))
    assert (P, u, r) == (m, n_p - m, r1) and r > 0 and k2.size == n_p + r
    assert _same_pairs(k1[:m], v1[:m], k2[:P], v2[:P]) and _same_pairs(k1[m:n_p], v1[m:n_p], k2[P:n_p], v2[P:n_p])
    assert _same_pairs(k1[n_p:], v1[n_p:], k2[n_p:], v2[n_p:])


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_counts_equal_the_counting_joins(fj, device):
    bk, bv, pk = _mm_case(1_000_000, 400_000, 3_000_000)
    args = _to_device(bk, bv, pk) if device else (bk, bv, pk)
    P, u, r, _ = fj.full_join(*args, duplicates="all")
    assert P == fj.inner_join_count(*args)[0]
    assert u == fj.anti_join_count(args[0], args[2])[0]
    assert r == fj.anti_join_count(args[2], args[0])[0]                    # roles swapped: build ROWS, every copy
    assert fj.left_join(*args, duplicates="all")[:2] == (P, u)
    # semi / anti / inner accept the keyword: multiplicity does not matter to the first two, inner is the many-to-many join
    assert fj.join_indices(args[0], args[2], how="anti", duplicates="all")[0] == u
    assert fj.join_indices(args[0], args[2], how="semi", duplicates="all")[0] == pk.size - u
    assert fj.join_indices(args[0], args[2], how="inner", duplicates="all")[0] == P


def _u64p(t):
    return ctypes.c_void_p(t.data_ptr())


@pytest.mark.gpu
@pytest.mark.parametrize("algo", [LEFT | ALL, FULL | ALL, FULL | ALL | ROW_IDS | 2], ids=["left", "full", "full_row_ids"])
def test_two_phase_form_of_the_c_abi(fj, algo):
    import torch
    from flash_hash_join_amd import _lib, api
    L = _lib.load()
    bk, bv, pk = _mm_case(60000, 9000, 300000)
    P_exp, ek, ev, anti_exp, rk_exp, rv_exp = _np_ref(bk, bv, pk)
    u_exp, r_exp = anti_exp.size, (rk_exp.size if algo & FULL else 0)
    rows = P_exp + u_exp + r_exp
    dbk, dbv, dpk = _to_device(bk, bv, pk)
    ctx = api.context(0)
    stream = torch.cuda.current_stream(0).cuda_stream
    cnt = (ctypes.c_uint64 * 3)(7, 7, 7)
    t = _lib.FjTimings()
    _lib.check(L.fj_join_device(ctx, algo, 0, 1, dbk.data_ptr(), dbv.data_ptr(), bk.size, dpk.data_ptr(), pk.size, stream, 64,
                                cnt, None, None, 0, ctypes.byref(t)))                # counted, rows pending
    assert (int(cnt[0]), int(cnt[1]), int(cnt[2])) == (P_exp, r_exp, u_exp)
    ok = torch.full((rows + 1,), 12345, dtype=torch.int64, device="cuda")
    ov = torch.full((rows + 1,), 12345, dtype=torch.int64, device="cuda")
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows - 1, stream, None) != 0          # one row too few: refused ...
    assert "output capacity" in _lib.last_error()
    _lib.check(L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows, stream, ctypes.byref(t)))     # ... and still pending
    assert t.emit_ms > 0
    assert int(ok[rows]) == 12345 and int(ov[rows]) == 12345, "a row behind the result was written"
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows, stream, None) != 0
    assert "no counted materialising join is pending" in _lib.last_error()
    k, v = _host(ok[:rows]), _host(ov[:rows])
    if algo & ROW_IDS:
        _check_row_ids(bk, pk, P_exp, u_exp, r_exp, k, v, full=bool(algo & FULL))
    else:
        assert _same_pairs(k[:P_exp], v[:P_exp], ek, ev)
        assert np.array_equal(_sorted(k[P_exp:P_exp + u_exp]), _sorted(anti_exp)) and np.all(v[P_exp:P_exp + u_exp] == 0)
        if algo & FULL:
            assert _same_pairs(k[P_exp + u_exp:], v[P_exp + u_exp:], rk_exp, rv_exp)
    # one call, enough capacity
    ok2 = torch.full((rows + 5,), 12345, dtype=torch.int64, device="cuda")
    ov2 = torch.full((rows + 5,), 12345, dtype=torch.int64, device="cuda")
    cnt2 = (ctypes.c_uint64 * 3)(0, 0, 0)
    _lib.check(L.fj_join_device(ctx, algo, 0, 1, dbk.data_ptr(), dbv.data_ptr(), bk.size, dpk.data_ptr(), pk.size, stream, 64,
                                cnt2, ok2.data_ptr(), ov2.data_ptr(), rows + 5, None))
    assert list(cnt2) == list(cnt)
    assert bool((ok2[rows:] == 12345).all()) and bool((ov2[rows:] == 12345).all())
    assert _same_pairs(_host(ok2[:P_exp]), _host(ov2[:P_exp]), k[:P_exp], v[:P_exp])
    assert _same_pairs(_host(ok2[P_exp:rows]), _host(ov2[P_exp:rows]), k[P_exp:], v[P_exp:])
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows, stream, None) != 0               # nothing pending after it
    # one call, too little capacity: the counts are there, the rows stay pending for fj_emit_pairs
    cnt3 = (ctypes.c_uint64 * 3)(0, 0, 0)
    assert L.fj_join_device(ctx, algo, 0, 1, dbk.data_ptr(), dbv.data_ptr(), bk.size, dpk.data_ptr(), pk.size, stream, 64,
                            cnt3, ok2.data_ptr(), ov2.data_ptr(), rows - 1, None) != 0
    assert "output capacity" in _lib.last_error() and list(cnt3) == list(cnt)
    _lib.check(L.fj_emit_pairs(ctx, ok2.data_ptr(), ov2.data_ptr(), rows, stream, None))
    # the next call that starts work drops a pending result
    _lib.check(L.fj_join_device(ctx, algo, 0, 1, dbk.data_ptr(), dbv.data_ptr(), bk.size, dpk.data_ptr(), pk.size, stream, 64,
                                cnt3, None, None, 0, None))
    assert fj.hash_join_count_radix(dbk, dbv, dpk)[0] == int(np.isin(pk, bk).sum())
    assert L.fj_emit_pairs(ctx, ok.data_ptr(), ov.data_ptr(), rows, stream, None) != 0
    assert "no counted materialising join is pending" in _lib.last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
def test_fill_value_lands_in_the_second_range_only(fj, device):
    bk, bv, pk = _mm_case(60000, 9000, 20000)            # 20 000 draws from 18 001 ids: thousands of the 9 000 build ids are never probed
    fill = 2**64 - 3
    assert not np.any(bv == np.uint64(fill))
    args = _to_device(bk, bv, pk) if device else (bk, bv, pk)
    P, u, r, _, keys, vals = fj.full_join(*args, return_arrays=True, fill_value=fill, duplicates="all")
    vals = _host(vals)
    assert u > 0 and r > 0 and np.all(vals[P:P + u] == np.uint64(fill))
    assert not np.any(vals[:P] == np.uint64(fill)) and not np.any(vals[P + u:] == np.uint64(fill))
    P, u, _, keys, vals = fj.left_join(*args, return_arrays=True, fill_value=fill, duplicates="all")
    vals = _host(vals)
    assert np.all(vals[P:] == np.uint64(fill)) and not np.any(vals[:P] == np.uint64(fill)) and vals.size == P + u


@pytest.mark.gpu
def test_a_key_with_too_many_duplicates_is_refused_and_the_context_stays_usable(fj):
    bk = np.concatenate([np.full(6000, 12345, dtype=np.uint64), np.arange(100000, 100500, dtype=np.uint64)])
    bv = np.arange(bk.size, dtype=np.uint64)
    pk = np.array([12345, 100001, 7], dtype=np.uint64)
    for device in (False, True):
        args = _to_device(bk, bv, pk) if device else (bk, bv, pk)
        with pytest.raises(RuntimeError, match="4096 build rows"):
            fj.left_join(*args, duplicates="all")
        with pytest.raises(RuntimeError, match="4096 build rows"):
            fj.full_join(*args, return_arrays=True, duplicates="all")
        with pytest.raises(RuntimeError, match="4096 build rows"):
            fj.join_indices(args[0], args[2], how="full", duplicates="all")
        assert fj.hash_join_count_radix(*args)[0] == 2                    # an N:1 join on the same context
        assert fj.left_join(*args)[0] == 2


@pytest.mark.gpu
@pytest.mark.parametrize("device", [False, True], ids=["numpy", "device"])
@pytest.mark.parametrize("nb,n_p", [(0, 1000), (1000, 0), (0, 0)], ids=["nb0", "np0", "both0"])
def test_empty_sides(fj, nb, n_p, device):
    rng = np.random.default_rng(nb + n_p)
    bk = rng.integers(0, 50, size=nb, dtype=np.uint64)                     # (duplicates among them)
    bv = np.arange(nb, dtype=np.uint64) + np.uint64(100)
    pk = rng.integers(0, 50, size=n_p, dtype=np.uint64)
    args = _to_device(bk, bv, pk) if device else (bk, bv, pk)
    P, u, _, keys, vals = fj.left_join(*args, return_arrays=True, fill_value=4, duplicates="all")
    assert (P, u) == (0, n_p if nb == 0 else 0) and _host(keys).size == u
    assert np.array_equal(_sorted(_host(keys)), _sorted(pk[:u])) and np.all(_host(vals) == 4)
    P, u, r, _, keys, vals = fj.full_join(*args, return_arrays=True, fill_value=4, duplicates="all")
    assert (P, u, r) == (0, n_p if nb == 0 else 0, nb if n_p == 0 else 0)
    keys, vals = _host(keys), _host(vals)
    assert keys.size == u + r and np.array_equal(_sorted(keys[:u]), _sorted(pk[:u])) and np.all(vals[:u] == 4)
    assert _same_pairs(keys[u:], vals[u:], bk[:r], bv[:r])
    P, u, r, _, pi, bi = fj.join_indices(args[0], args[2], how="full", duplicates="all")
    assert (P, u, r) == (0, n_p if nb == 0 else 0, nb if n_p == 0 else 0)
    _check_row_ids(bk, pk, P, u, r, pi, bi)
    P, u, _, pi, bi = fj.join_indices(args[0], args[2], how="left", duplicates="all")
    _check_row_ids(bk, pk, P, u, 0, pi, bi, full=False)
    assert fj.full_join(*args, duplicates="all")[:3] == (0, n_p if nb == 0 else 0, nb if n_p == 0 else 0)
