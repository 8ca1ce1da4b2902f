"""How a caller hands work in, on an MI355X: device entry points on side streams, on tensor views, on a second device and from
independent contexts at once.  The rows, their inputs and their NumPy references are CASES of test_caller_context_cpu.py; nothing
is compared with the library itself.

A. Late inputs on a side stream.  The input buffers hold the poison of test_caller_context_cpu.py; on a non-blocking side stream a
   delay is enqueued, then the copies of the real data into the buffers, then the library call - while the delay is still running
   (`not ready.query()`, asserted: a delay that is too short FAILS the test).  A launch, memset or copy of the call that names another
   stream than the caller's reads the poison and returns the poison's result: a wrong count from valid data, never a fault.  The
   outputs are consumed by a torch op on the side stream with no synchronisation in between, then compared with the reference.
B. Tensor views: every tensor argument as base[1:] (address 8 mod 16), base[::2], a contiguous (r, 7) tensor, the .t() of a (7, r)
   one and torch.uint64, with guard words around and between the viewed elements; `out=` accumulators at an address 8 mod 16.
C. The same on cuda:1 while device 0 is current (skipped on a machine with one device: the only skip in this file).
D. Three threads with a side stream each: two Index objects and the module context at once.

Shapes (test_caller_context_cpu.SHAPES): 60 000 build rows over 9 000 keys and 200 003 probe rows - one radix pass at the default
options, two passes under plan_target_keys = 16 for the rows marked `deep` - and 300 x 2 000 rows (1 500 for the group-bys), which
take no pass at all.

The delay is a chain of in-place `add_` over one 1 GiB tensor, timed once per device with events at module set-up: measured
0.36 ms per repeat on an MI355X, so 418 repeats make the 150 ms aimed at (the 100 ms asked for and half as much again;
the number stands for nothing but "far beyond the host's enqueue latency", which is tens of microseconds per operation)."""
import math
import threading

import numpy as np
import pytest

import test_caller_context_cpu as CC

pytestmark = pytest.mark.gpu
DELAY_MS, AIM_MS = 100.0, 150.0
TARGET_DEFAULT, TARGET_DEEP = 4096, 16
VIEW_FORMS = ("offset8", "stride2", "2d", "2d_t", "uint64")
COLS = 7                                                  # columns of the 2-D forms: no input length is a multiple, so a tail is cut


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    for name, value in (("plan_target_keys", TARGET_DEFAULT), ("scalar_hbm_table", 0), ("radix_threshold", 0)):
        assert flash_join.get_option(name) == value, f"option {name} is not at its default"
    return flash_join


class plan_target:
    """plan_target_keys for the calls inside, restored in any case"""
    def __init__(self, fj, target):
        self.fj, self.target = fj, target

    def __enter__(self):
        if self.target:
            self.fj.set_option("plan_target_keys", self.target)

    def __exit__(self, *exc):
        if self.target:
            self.fj.set_option("plan_target_keys", TARGET_DEFAULT)
        return False


class Late:
    """a non-blocking side stream per device and a delay on it that lasts AIM_MS"""

    def __init__(self):
        self.per = {}

    def on(self, device):
        import torch
        device = torch.device(device)
        if device not in self.per:
            side = torch.cuda.Stream(device=device)
            big = torch.zeros(1 << 28, dtype=torch.int32, device=device)
            torch.cuda.synchronize(device)
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(side):
                for _ in range(4):
                    big.add_(1)
                start.record()
                for _ in range(32):
                    big.add_(1)
                stop.record()
            stop.synchronize()
            per_repeat = start.elapsed_time(stop) / 32
            repeats = max(1, math.ceil(AIM_MS / per_repeat))
            print(f"\n[caller context] {device}: delay primitive {per_repeat:.4f} ms per repeat, {repeats} repeats for {AIM_MS} ms")
            self.per[device] = (side, big, repeats, per_repeat)
        return self.per[device]

    def side(self, device):
        return self.on(device)[0]

    def delay(self, device):
        """enqueue the delay on the CURRENT stream"""
        _, big, repeats, _ = self.on(device)
        for _ in range(repeats):
            big.add_(1)


@pytest.fixture(scope="module")
def late(fj):
    import torch
    late = Late()
    side, big, repeats, per_repeat = late.on("cuda:0")
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        start.record()
        late.delay("cuda:0")
        stop.record()
    stop.synchronize()
    assert start.elapsed_time(stop) >= DELAY_MS, f"one delay lasts {start.elapsed_time(stop):.1f} ms: {repeats} repeats of {per_repeat:.4f} ms"
    return late


# ---- containers --------------------------------------------------------------------------------------------------------------------------
def to_device(a, device):
    """a NumPy array of words or float64 as a tensor on `device`: torch.int64 storage of the words, torch.float64"""
    import torch
    a = np.array(a, copy=True)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(device)


_REAL = {}


def real_tensors(shape, device):
    """the real inputs of a shape on a device: made once, on the default stream, never changed"""
    import torch
    key = (shape, str(device))
    if key not in _REAL:
        d = CC.data(shape)
        _REAL[key] = {n: to_device(getattr(d, n), device) for n in CC.KIND}
        torch.cuda.synchronize(device)
    return _REAL[key]


def tensors_of(x):
    if isinstance(x, (tuple, list)):
        return [t for item in x for t in tensors_of(item)]
    return [x] if hasattr(x, "is_cuda") else []


def to_numpy(x):
    if isinstance(x, (tuple, list)):
        return tuple(to_numpy(item) for item in x)
    return x.cpu().numpy() if hasattr(x, "is_cuda") else x


def consume(raw, device):
    """the outputs live on the inputs' device and compose with torch on the current stream at once: one reduction per output tensor,
    enqueued with no synchronisation beforehand; checked against the output itself afterwards"""
    import torch
    device = torch.device(device)
    outs = tensors_of(raw)
    for t in outs:
        assert t.is_cuda and t.device == device, f"an output lives on {t.device}, the inputs on {device}"
    sums = [t.sum() for t in outs]
    return [(t, s) for t, s in zip(outs, sums)]


def check_consumed(consumed):
    for t, s in consumed:
        whole = t.cpu().numpy()
        want = whole.sum(dtype=whole.dtype if whole.dtype.kind == "f" else np.int64)
        assert s.cpu().numpy() == want, f"a torch reduction right behind the call saw {s.item()}, the output sums to {want}"


def compare(r, got, a, exp, what):
    got = r.canon(got, a)
    assert got.keys() == exp.keys(), (what, sorted(got), sorted(exp))
    for k in exp:
        if not CC.same(got[k], exp[k]):
            g, e = got[k], exp[k]
            if isinstance(e, (int, np.integer)):
                detail = f"{g} != {e}"
            else:
                g, e = np.asarray(g), np.asarray(e)
                detail = f"shape {g.shape} {g.dtype} against {e.shape} {e.dtype}"
                if g.shape == e.shape:
                    bad = np.flatnonzero((g != e).reshape(-1))
                    detail += f", {bad.size} elements differ, the first at {bad[:1]}: {g.reshape(-1)[bad[:1]]} != {e.reshape(-1)[bad[:1]]}"
            raise AssertionError(f"{what}: output '{k}' is not the reference's: {detail}")


def check_plan(fj, r, shape, target):
    lt = fj.last_timings()
    want = 0 if shape == "zero_pass" else (2 if target else 1)
    assert lt["passes"] == want and lt["fell_back"] == 0, (r.id, shape, target, lt)


def late_call(fj, late, r, shape, device, ix):
    """steps 1 to 5 of section A on `device`; returns (result as NumPy, the real inputs as NumPy)"""
    import torch
    d, real = CC.data(shape), real_tensors(shape, device)
    bufs = {n: to_device(CC.poison(n, getattr(d, n).size), device) for n in r.args}
    torch.cuda.synchronize(device)
    side = late.side(device)
    with torch.cuda.stream(side):
        late.delay(device)
        for n in r.args:
            bufs[n].copy_(real[n])
        ready = torch.cuda.Event()
        ready.record()
        assert not ready.query(), "the delay was too short: the real data had arrived before the call was issued, the test proves nothing"
        raw = r.call(fj, bufs, ix)
        if r.after is None:
            consumed = consume(raw, device)
            check_consumed(consumed)
            got = to_numpy(raw)
        untouched = {n: bool(torch.equal(bufs[n], real[n])) for n in r.args if n not in r.accumulators()}
    if r.after is not None:                                # the second step: on the default stream, once the side stream is drained
        side.synchronize()
        raw = r.after(fj, raw, lambda n: real[n])
        check_consumed(consume(raw, device))
        got = to_numpy(raw)
    assert all(untouched.values()), f"inputs are read only, these changed: {[n for n, ok in untouched.items() if not ok]}"
    return got


A_PARAMS = ([pytest.param(r, shape, None, id=f"{r.id}-{shape}") for r in CC.CASES for shape in ("one_pass", "zero_pass")]
            + [pytest.param(CC.BY_ID[n], "one_pass", TARGET_DEEP, id=f"{n}-two_pass") for n in CC.DEEP])


# ---- A. late inputs on a side stream -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r,shape,target", A_PARAMS)
def test_late_inputs_on_a_side_stream(fj, late, r, shape, target):
    d, real = CC.data(shape), real_tensors(shape, "cuda:0")
    with plan_target(fj, target):
        ix = fj.build_index(real["bk"], real["bv"]) if r.index else None        # (on the default stream; probed late on the side stream)
        try:
            got = late_call(fj, late, r, shape, "cuda:0", ix)
            check_plan(fj, r, shape, target)
        finally:
            if ix is not None:
                ix.close()
    compare(r, got, r.real(d), CC.expected(r.id, shape), f"{r.id} with late inputs on a side stream")


NUMPY_ENTRY = [next(n for n in CC.REPRESENTATIVE if CC.BY_ID[n].family == f) for f in CC.FAMILIES]


@pytest.mark.parametrize("name", NUMPY_ENTRY)
def test_numpy_entry_inside_a_side_stream(fj, late, name):
    """NumPy inputs are staged through the null stream by the library itself: a busy side stream being current must not matter"""
    import torch
    r, d = CC.BY_ID[name], CC.data("one_pass")
    a = {n: np.array(v, copy=True) for n, v in r.real(d).items()}
    ix = fj.build_index(np.array(d.bk), np.array(d.bv)) if r.index else None
    try:
        with torch.cuda.stream(late.side("cuda:0")):
            late.delay("cuda:0")
            raw = r.call(fj, a, ix)
            if r.after is not None:
                raw = r.after(fj, raw, lambda n: np.array(getattr(d, n)))
    finally:
        if ix is not None:
            ix.close()
    assert not tensors_of(raw), "NumPy in, NumPy out"
    compare(r, raw, r.real(d), CC.expected(name, "one_pass"), f"{name} through the NumPy entry inside a side stream")
    assert all(np.array_equal(a[n], getattr(d, n)) for n in r.args if n not in r.accumulators())


# ---- B. tensor views --------------------------------------------------------------------------------------------------------------------------
def make_view(form, name, arr, device):
    """(base, view): `arr` (NumPy words or float64) behind a view of the given form; the base holds GUARD wherever the view does not look"""
    import torch
    words = to_device(np.ascontiguousarray(arr).view(np.uint64), device)
    n = words.numel()
    guard = int(CC.GUARD.view(np.int64))
    if CC.KIND[name] in ("acc", "facc"):                     # accumulators are combined into in place: never a copy, tested on their own
        base = view = words.clone()
    elif form == "offset8":
        base = torch.full((n + 1,), guard, dtype=torch.int64, device=device)
        view = base[1:]
        view.copy_(words)
        assert view.data_ptr() % 16 == 8
    elif form == "stride2":
        base = torch.full((2 * n,), guard, dtype=torch.int64, device=device)
        view = base[::2]
        view.copy_(words)
    else:
        m = n if form == "uint64" else (n // COLS) * COLS
        base = torch.full((m + 4,), guard, dtype=torch.int64, device=device)
        view = base[2:2 + m]
        view.copy_(words[:m])
        assert view.data_ptr() % 16 == 0
        if form == "2d":
            view = view.view(m // COLS, COLS)
        elif form == "2d_t":
            view = view.view(COLS, m // COLS).t()
            assert not view.is_contiguous()
    if CC.KIND[name] in ("fval", "facc"):
        view = view.view(torch.float64)
    elif form == "uint64" and CC.KIND[name] != "acc":
        view = view.view(torch.uint64)
    return base, view


def flat(view, name):
    """what the library must read: the view's elements in row-major order"""
    a = view.cpu().numpy().reshape(-1)
    return a if CC.KIND[name] in ("fval", "facc") else np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("shape", ["one_pass", "zero_pass"])
@pytest.mark.parametrize("form", VIEW_FORMS)
@pytest.mark.parametrize("r", CC.CASES, ids=lambda r: r.id)
def test_tensor_views(fj, r, form, shape):
    import torch
    d, real = CC.data(shape), real_tensors(shape, "cuda:0")
    made = {n: make_view(form, n, getattr(d, n), "cuda:0") for n in r.args}
    t = {n: v for n, (_, v) in made.items()}
    a = {n: flat(t[n], n) for n in r.args}
    before = {n: made[n][0].clone() for n in r.args if n not in r.accumulators()}
    ix = fj.build_index(real["bk"], real["bv"]) if r.index else None
    try:
        raw = r.call(fj, t, ix)
        if r.after is not None:
            raw = r.after(fj, raw, lambda n: real[n])
    finally:
        if ix is not None:
            ix.close()
    assert all(x.device == torch.device("cuda:0") for x in tensors_of(raw))
    as_given = all(np.array_equal(a[n], getattr(d, n)) for n in r.args)
    exp = CC.expected(r.id, shape) if as_given else r.ref(a, d)
    compare(r, to_numpy(raw), a, exp, f"{r.id} on {form} views")
    changed = [n for n in before if not torch.equal(made[n][0], before[n])]
    assert not changed, f"inputs and the guard words around them are read only, these changed: {changed}"


OUT_ROWS = [n for n in CC.BY_ID if n.startswith("Index.group_") and "out]" in n]


@pytest.mark.parametrize("shape", ["one_pass", "zero_pass"])
@pytest.mark.parametrize("name", OUT_ROWS)
def test_accumulators_at_an_address_8_mod_16_are_combined_into_in_place(fj, name, shape):
    import torch
    r, d, real = CC.BY_ID[name], CC.data(shape), real_tensors(shape, "cuda:0")
    nb, guard = d.bk.size, int(CC.GUARD.view(np.int64))
    t, bases = {n: real[n] for n in r.args}, {}
    for n in r.accumulators():
        bases[n] = torch.full((nb + 2,), guard, dtype=torch.int64, device="cuda:0")
        view = bases[n][1:1 + nb]
        view.copy_(real[n].view(torch.int64))
        assert view.is_contiguous() and view.data_ptr() % 16 == 8
        t[n] = view.view(torch.float64) if CC.KIND[n] == "facc" else view
    with fj.build_index(real["bk"], real["bv"]) as ix:
        raw = r.call(fj, t, ix)
    for out in tensors_of(raw):                                # what comes back IS the caller's storage
        assert out.data_ptr() in [t[n].data_ptr() for n in r.accumulators()]
    compare(r, to_numpy(raw), r.real(d), CC.expected(name, shape), f"{name} with accumulators at an address 8 mod 16")
    for n, base in bases.items():
        assert base[0].item() == guard and base[-1].item() == guard, f"a word next to {n} was written"


@pytest.mark.parametrize("name", OUT_ROWS)
def test_a_strided_accumulator_is_refused_before_any_native_call(fj, name, monkeypatch):
    import torch
    from flash_hash_join_amd import _lib
    r, d, real = CC.BY_ID[name], CC.data("zero_pass"), real_tensors("zero_pass", "cuda:0")
    nb = d.bk.size
    t = {n: real[n] for n in r.args}
    holder = {}
    for n in r.accumulators():
        holder[n] = torch.zeros(2 * nb, dtype=real[n].dtype, device="cuda:0")
        t[n] = holder[n][::2]
        assert t[n].numel() == nb and not t[n].is_contiguous()
    lookup = CC.BY_ID["Index.lookup"]
    with fj.build_index(real["bk"], real["bv"]) as ix:
        L = _lib.load()
        native = L.fj_join_device

        def no_native_call(*args):
            raise AssertionError("a native call was made with a strided accumulator")
        monkeypatch.setattr(L, "fj_join_device", no_native_call)
        try:
            with pytest.raises(ValueError, match="contiguous"):
                r.call(fj, t, ix)
        finally:
            monkeypatch.setattr(L, "fj_join_device", native)
        assert all(not bool(h.any()) for h in holder.values()), "the refused accumulator was written"
        got = to_numpy(lookup.call(fj, {"pk": real["pk"]}, ix))      # the index still answers
    compare(lookup, got, lookup.real(d), CC.expected("Index.lookup", "zero_pass"), "Index.lookup after a refused accumulator")


# ---- C. a second device -----------------------------------------------------------------------------------------------------------------------
def _two_devices():
    try:
        import torch
        return torch.cuda.device_count() >= 2
    except Exception:                                          # noqa: BLE001
        return False


second_device = pytest.mark.skipif(not _two_devices(), reason="needs a second ROCm device")


def _device0_still_answers(fj):
    r = CC.BY_ID["hash_join_count_radix"]
    got = to_numpy(r.call(fj, real_tensors("zero_pass", "cuda:0"), None))
    compare(r, got, None, CC.expected(r.id, "zero_pass"), "a call on cuda:0 after one on cuda:1")


def on_another_device(fj, name, device):
    """tensors on cuda:<device> while device 0 is current, no torch.cuda.device(...) around the call"""
    import torch
    where = f"cuda:{device}"
    r, d, real = CC.BY_ID[name], CC.data("one_pass"), real_tensors("one_pass", where)
    target = TARGET_DEEP if r.deep else None
    torch.cuda.set_device(0)
    with plan_target(fj, target):
        ix = fj.build_index(real["bk"], real["bv"]) if r.index else None
        try:
            raw = r.call(fj, {n: (real[n].clone() if n in r.accumulators() else real[n]) for n in r.args}, ix)
            if r.after is not None:
                raw = r.after(fj, raw, lambda n: real[n])
            check_plan(fj, r, "one_pass", target)
        finally:
            if ix is not None:
                ix.close()
    assert torch.cuda.current_device() == 0, "the call changed the current device"
    assert all(x.device == torch.device(where) for x in tensors_of(raw))
    compare(r, to_numpy(raw), r.real(d), CC.expected(name, "one_pass"), f"{name} on {where} with device 0 current")
    _device0_still_answers(fj)


def late_on_another_device(fj, late, name, device):
    """section A on a side stream of cuda:<device>, entered from device 0"""
    import torch
    where = f"cuda:{device}"
    r, d, real = CC.BY_ID[name], CC.data("one_pass"), real_tensors("one_pass", where)
    torch.cuda.set_device(0)
    ix = fj.build_index(real["bk"], real["bv"]) if r.index else None
    try:
        got = late_call(fj, late, r, "one_pass", where, ix)
    finally:
        if ix is not None:
            ix.close()
    assert torch.cuda.current_device() == 0, "the call changed the current device"
    compare(r, got, r.real(d), CC.expected(name, "one_pass"), f"{name} with late inputs on a side stream of {where}")
    _device0_still_answers(fj)


def numpy_built_index_on(fj, device):
    """build_index(numpy_keys, device=<device>), probed with tensors of that device and with NumPy"""
    import torch
    where = f"cuda:{device}"
    d, real = CC.data("one_pass"), real_tensors("one_pass", where)
    torch.cuda.set_device(0)
    with fj.build_index(np.array(d.bk), np.array(d.bv), device=device) as ix:
        assert ix.device == device
        for name in ("Index.lookup", "Index.isin", "Index.group_sum"):
            r = CC.BY_ID[name]
            raw = r.call(fj, {n: real[n] for n in r.args}, ix)
            assert all(x.device == torch.device(where) for x in tensors_of(raw))
            compare(r, to_numpy(raw), r.real(d), CC.expected(name, "one_pass"), f"{name}: a NumPy-built index on device {device}, {where} probes")
            raw = r.call(fj, {n: np.array(getattr(d, n)) for n in r.args}, ix)
            assert not tensors_of(raw)
            compare(r, raw, r.real(d), CC.expected(name, "one_pass"), f"{name}: a NumPy-built index on device {device}, NumPy probes")
    assert torch.cuda.current_device() == 0
    _device0_still_answers(fj)


@second_device
@pytest.mark.parametrize("name", CC.REPRESENTATIVE)
def test_tensors_on_device_1_while_device_0_is_current(fj, name):
    on_another_device(fj, name, 1)


@second_device
@pytest.mark.parametrize("name", CC.REPRESENTATIVE)
def test_late_inputs_on_a_side_stream_of_device_1(fj, late, name):
    late_on_another_device(fj, late, name, 1)


@second_device
def test_an_index_built_from_numpy_on_device_1(fj):
    numpy_built_index_on(fj, 1)


# ---- D. independent contexts at once ------------------------------------------------------------------------------------------------------------
def test_two_indexes_and_the_module_context_at_once(fj):
    """Three threads, a side stream each, six rounds each: two Index objects (a context and a lock of their own each) and the module
    context are driven at the same time - ctypes releases the GIL, nothing serialises the three against each other, the kernels may
    overlap on the GPU - and every result is checked against its reference inside the thread."""
    import torch
    shape = "one_pass"
    d, real = CC.data(shape), real_tensors(shape, "cuda:0")
    plans = {
        1: ["Index.lookup", "Index.group_sum[out]"],
        2: ["Index.isin", "Index.lookup_indices", "Index.group_min"],
        3: ["group_by_agg", "left_join", "GroupByAccumulator"],
    }
    for names in plans.values():
        for n in names:
            CC.expected(n, shape)                                  # computed once, before the threads start
    indexes = {1: fj.build_index(real["bk"], real["bv"]), 2: fj.build_index(real["bk"]), 3: None}
    streams = {tid: torch.cuda.Stream() for tid in plans}
    torch.cuda.synchronize()
    errors = []

    def work(tid):
        try:
            with torch.cuda.stream(streams[tid]):
                for rep in range(6):
                    for n in plans[tid]:
                        r = CC.BY_ID[n]
                        t = {a: (real[a].clone() if a in r.accumulators() else real[a]) for a in r.args}
                        raw = r.call(fj, t, indexes[tid])
                        consumed = consume(raw, "cuda:0")
                        check_consumed(consumed)
                        compare(r, to_numpy(raw), r.real(d), CC.expected(n, shape), f"thread {tid}, round {rep}, {n}")
        except BaseException as ex:                                 # noqa: BLE001
            errors.append((tid, repr(ex)))
    threads = [threading.Thread(target=work, args=(tid,), daemon=True) for tid in plans]
    try:
        for th in threads:
            th.start()
        for th in threads:
            th.join(timeout=60)
        alive = [th.name for th in threads if th.is_alive()]
        assert not alive, f"threads still running after 60 s: {alive}"
    finally:
        if not any(th.is_alive() for th in threads):
            for ix in indexes.values():
                if ix is not None:
                    ix.close()
    assert not errors, errors
