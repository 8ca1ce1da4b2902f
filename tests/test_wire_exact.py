"""What a rank sends its peers, on an MI355X, byte for byte: the build-broadcast regions decoded, range joins that run while the later
pieces are still missing, the exported per-partition filters, the in-place precheck key for key, and the sample - against the NumPy model
of tests/wire_model.py, equalities only.  Public API and LabEngine only.

The inputs, the two checks (check_region, check_precheck), what each input can tell apart (the seeded defects R-a .. R-h, F-a .. F-h)
and the pinned constants are tests/test_wire_exact_cpu.py; its docstring lists the key sets.

  A  test_regions_decoded, test_region_beyond_the_wide_scan
                                 LabEngine.bcast_pack into a buffer of 0xA5 with 4-KiB guards, for 1, 2, 3, 5, 7 and 16 pieces: offs, every
                                 partition's keys, every value, the piece bounds, fj_bcast_piece_span, every byte that must stay 0xA5
                                 (fj_dense_count, fj_dense_scan / _scan_wide, fj_dense_copy<2|4>, fj_dense_copy_vals)
  B  test_range_joins_see_only_what_has_arrived
                                 every rank of a world of 2, 3 and 8: its buffer holds 0xA5 but for its own region; piece q's spans of every
                                 peer are copied in, then range q is joined (fj_count_join_wide<DENSE>), counting and materialising
  C  test_exported_filters       shuffle_pack -> stream_append_chunks -> stream_export_part_filters, every owner of worlds 1, 3 and 8
                                 (fj_part_filter_export)
  D  test_precheck_key_for_key, test_every_workgroup_takes_a_second_batch, test_owners_join_the_prechecked_shares
                                 shuffle_pack(filters = the model's) (fj_part_filter_inplace<4>)
  E  test_the_sample             LabEngine.part_filter_sample (fj_part_filter_sample)
plan_target_keys is set through the `opts` fixture, which puts it back after every test; every `bits` is read back from the engine.

BEYOND 2^19 PARTITIONS: the case RAN.  bcast_plan accepts a nominal total of 16 << 20 rows under plan_target_keys = 16 (20 bits, three
passes), the chunk pools hold it, and test_region_beyond_the_wide_scan decodes 100 000 keys packed through the multi-sweep loop of
fj_dense_scan (64 sweeps).  Nothing is refused.

TIMES on an MI355X machine (pytest --durations=0, one run; 256 compute units): this file, 124 tests, 7.6 s in all, 1.6 s of that the
setup of the first test (loading the library).  The slowest calls: test_range_joins_see_only_what_has_arrived 0.3 - 0.4 s for the first
case of a world and width (it uploads the blocks and computes the reference), 0.03 - 0.10 s for the others;
test_every_workgroup_takes_a_second_batch (3 145 728 keys, twice) 0.41 s; test_exported_filters 0.01 - 0.12 s, the nine 512-MiB cases
0.01 - 0.10 s; test_precheck_key_for_key 0.01 - 0.12 s (random-17 and fa_twins-17, 512 MiB of filters: 0.12 and 0.07 s);
test_regions_decoded 0.01 - 0.11 s; test_region_beyond_the_wide_scan 0.11 s; test_the_sample (stride 4099: 410M keys of filler made on
the device) 0.01 s; test_owners_join_the_prechecked_shares 0.05 s.  Nothing had to be shrunk.  tests/test_wire_exact_cpu.py, which
builds every input and model once more, takes 20 s on one CPU core.

WOULD THEY FAIL?  Once, while this file was written, it ran against six scratch builds of the library with one seeded defect each (each
changes only which value or already-addressed element is written), and failed as it should; against the unmodified library all 124 pass.
  fj_dense_copy: `g0 + e >= vlo` -> `>`  53 fail: test_regions_decoded crafted and random at every width, with and without values (`one`
    in flush's low plane (R-a)            and `none` pass: the one partition starts at offset 0), test_region_beyond_the_wide_scan, and
                                          all 36 cases of test_range_joins_see_only_what_has_arrived (a lost key that is probed)
  fj_part_filter_export: `tid <` ->      25 fail: test_exported_filters random and crafted at every fan-out and world, and
    `tid + 1 <` the chunk's count (F-c)   test_owners_join_the_prechecked_shares (by its comparison of the owners' filters); the 12 `dups`
                                          cases pass - the dropped last key of a chunk has two more copies
  fj_part_filter_inplace: `== m[j]` ->   12 fail: test_precheck_key_for_key wherever a miss exists (no_hits, hits_1to1, hits_1to7, fa_twins,
    `!= 0` (F-a, all four positions)      holes, random; all_hits and b255 - b257 pass), test_every_workgroup_takes_a_second_batch and
                                          test_owners_join_the_prechecked_shares
  fj_bcast_piece_span: `L.mid_bytes` ->  13 fail: test_regions_decoded at 16 and 17 bits (crafted, random, one; the u32 widths and the
    `4` for part 2 (R-h)                  empty region pass) and test_region_beyond_the_wide_scan.  The range joins PASS: the doubled
                                          spans copy a superset of what each piece needs, from a staging buffer that holds the same bytes
  pf_bits: `(w >> 18)` -> `(w >> 19)`    55 fail: all 36 exports, all 14 cases of test_precheck_key_for_key, test_the_sample at every stride,
    (insert and test alike)               the big piece and the chain
  fj_dense_copy_vals: `cv[k]` ->         30 fail: every `vals` case of test_regions_decoded with keys (crafted, random, one) and the 18
    `cv[k ^ 1]` (R-f)                     materialising cases of the range joins; every keys-only case passes
"""
import functools

import numpy as np
import pytest

import keymix
import test_wire_exact_cpu as C
import wire_model as WM

pytestmark = pytest.mark.gpu
DEFAULTS = {"plan_target_keys": 4096}
GUARD, FILL = 4096, 0xA5
_U = np.uint64


@pytest.fixture(scope="module")
def fj():
    import flash_join
    from flash_hash_join_amd import _lib
    assert _lib.load().fj_device_count() >= 1, "no HIP device: the product path must not silently fall back"
    assert flash_join.initialize() is None
    for name, value in DEFAULTS.items():
        assert flash_join.get_option(name) == value, f"option {name} is not at its default"
    return flash_join


@pytest.fixture
def opts(fj):
    """set(name, value); plan_target_keys is back at its default after the test"""
    yield fj.set_option
    for name, value in DEFAULTS.items():
        fj.set_option(name, value)


@pytest.fixture(scope="module")
def eng(fj):
    from flash_hash_join_amd.lab import LabEngine
    return LabEngine("cuda:0")


@pytest.fixture(scope="module")
def G():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a):
    import torch
    a = np.array(a)                                               # (a writable copy: the inputs of the CPU file are read-only)
    if a.size == 0:
        return torch.empty(16, dtype=torch.int64, device="cuda:0")[:0]
    return torch.from_numpy(a.view(np.int64)).cuda()


def _bcast_bits(eng, opts, bits):
    """the nominal total build side whose broadcast plan has `bits` bits under plan_target_keys = 16, read back from the engine"""
    opts("plan_target_keys", C.TARGET)
    nbt = WM.nominal_rows(bits, C.TARGET)
    assert eng.bcast_plan(nbt) == (bits, 1 << bits, WM.region_layout(bits, 0)[1]), (bits, eng.bcast_plan(nbt))
    return nbt


def _shuffle_bits(eng, opts, bits, world):
    opts("plan_target_keys", C.TARGET)
    nbt = WM.nominal_rows(bits, C.TARGET)
    fl0 = WM.fan_logs(bits)[0]
    assert eng.shuffle_plan(nbt, world) == fl0 and eng.part_filter_range(nbt, world, 0)[2:] == (1 << bits, WM.PFILT_BYTES), (bits, eng.shuffle_plan(nbt, world))
    assert eng.shuffle_chunk_bytes(nbt, world) == (1792 if fl0 >= 8 else 2048)
    return nbt, fl0


def _end_step(eng, nbt):
    eng.bcast_probe(_dev(np.zeros(0, dtype=_U)), nbt)
    assert eng.bcast_finish() == 0


# ---- A. regions, decoded ------------------------------------------------------------------------------------------------------------------------
def _pack_and_check(eng, nbt, bits, keys, with_vals, pieces_list, what):
    import torch
    n = keys.size
    lay = WM.region_layout(bits, n, with_vals)
    assert eng.bcast_region_bytes(nbt, n, with_vals) == lay[5], f"{what}: bcast_region_bytes"
    buf = torch.empty(lay[5] + 2 * GUARD, dtype=torch.uint8, device="cuda:0")
    region = buf[GUARD: GUARD + lay[5]]
    assert region.data_ptr() % 16 == 0
    dk, dv = _dev(keys), (_dev(C.vals_of(keys)) if with_vals else None)
    for pieces in pieces_list:
        buf.fill_(FILL)
        eng.bcast_pack(dk, nbt, region, pieces, vals=dv)
        bounds = eng.bcast_pack_bounds(pieces)
        _end_step(eng, nbt)
        host = buf.cpu().numpy()
        tag = f"{what}, {pieces} pieces"
        if pieces in (pieces_list[0], pieces_list[-1]):          # the planes do not depend on the piece count: decoded for the first and the last
            offs = C.check_region(host[GUARD: GUARD + lay[5]], keys, bits, with_vals, tag)
        else:
            assert np.array_equal(host[GUARD: GUARD + 4 * lay[0] + 4].view(np.uint32), offs), f"{tag}: another offset table than with {pieces_list[0]} pieces"
        C.check_padding(host, GUARD, bits, n, with_vals, FILL, tag)
        assert bounds == WM.piece_bounds(offs, pieces), f"{tag}: bcast_pack_bounds {bounds}, offs[nparts * q // pieces] {WM.piece_bounds(offs, pieces)}"
        for q in range(pieces):
            for part in range(4):
                got, want = eng.bcast_piece_span(nbt, n, bounds[q], bounds[q + 1], part), WM.piece_span(bits, n, bounds[q], bounds[q + 1], part)
                assert got == want, f"{tag}: fj_bcast_piece_span of piece {q}, part {part}: {got}, the model {want}"


@pytest.mark.parametrize("with_vals", [False, True], ids=["keys", "vals"])
@pytest.mark.parametrize("bits", C.REGION_BITS)
@pytest.mark.parametrize("kind", C.REGION_KINDS)
def test_regions_decoded(fj, opts, eng, kind, bits, with_vals):
    """bits 12: the single-workgroup scan, u32 plane; 13: fj_dense_scan_wide with two workgroups; 16, 17: the u16 plane.  `none`: a rank
    without build rows yields an all-zero offs table and zero bounds"""
    nbt = _bcast_bits(eng, opts, bits)
    keys = C.region_keys(kind, bits)
    _pack_and_check(eng, nbt, bits, keys, with_vals, C.PIECES if kind in ("crafted", "random") else (1, 5), f"{kind}, {bits} bits, {'with' if with_vals else 'no'} values")
    import torch
    spare = torch.empty(eng.bcast_region_bytes(nbt, keys.size), dtype=torch.uint8, device="cuda:0")
    with pytest.raises(RuntimeError, match="pieces must be 1..16"):
        eng.bcast_pack(_dev(keys), nbt, spare, WM.MAX_PIECES + 1)


BEYOND_BITS = 20


def test_region_beyond_the_wide_scan(fj, opts, eng):
    """More than 2^19 partitions: a nominal total of 16 << 20 rows under plan_target_keys = 16 is a 20-bit, three-pass plan; bcast_plan and
    the chunk pools ACCEPT it (nothing is refused), and 100 000 keys run the multi-sweep loop of fj_dense_scan - 64 sweeps of 16384
    entries - which runs nowhere else in the suite.  Keys only: the values take the same path as at every other width."""
    nbt = _bcast_bits(eng, opts, BEYOND_BITS)
    assert (1 << BEYOND_BITS) > C.constants()["wide_scan"][1]
    keys = np.random.default_rng(20261108).integers(0, 2**64, 100_000, dtype=_U)
    _pack_and_check(eng, nbt, BEYOND_BITS, keys, False, (1, 7), f"100 000 keys under {BEYOND_BITS} bits")


# ---- B. range joins see only what has arrived ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _join_inputs(world, width):
    bks, bvs, pks = C.join_blocks(world, width)
    return [_dev(x) for x in bks], [_dev(x) for x in bvs], [_dev(x) for x in pks]


@pytest.mark.parametrize("pieces", C.JOIN_PIECES)
@pytest.mark.parametrize("mat", [False, True], ids=["count", "pairs"])
@pytest.mark.parametrize("width", list(C.JOIN_SHAPES))
@pytest.mark.parametrize("world", C.JOIN_WORLDS)
def test_range_joins_see_only_what_has_arrived(fj, opts, eng, world, width, mat, pieces):
    """As in the driver (the join of partition range q is queued behind piece q's arrival, pieces q + 1 .. still in flight): the receiver's
    buffer holds 0xA5 wherever nothing has arrived.  Per rank the count (and the pairs) of oracle.np_join over all ranks' build rows and the
    rank's probe rows (C.join_reference; the counts add up to np_join of the whole relations); no rung of the fallback
    ladder; at the end the receiver's buffer equals the senders' regions on every live byte - the spans cover them."""
    import torch
    opts("plan_target_keys", C.JOIN_SHAPES[width][2])
    bks, bvs, pks = _join_inputs(world, width)
    sizes = [int(b.numel()) for b in bks]
    nbt = sum(sizes)
    bits, nparts, mid_bytes = eng.bcast_plan(nbt)
    assert (bits, mid_bytes) == (C.join_bits(width), 2 if width == "u16" else 4)
    rbs = [eng.bcast_region_bytes(nbt, n, mat) for n in sizes]
    assert rbs == [WM.region_layout(bits, n, mat)[5] for n in sizes]
    offs = [sum(rbs[:r]) for r in range(world)]
    stage = torch.full((sum(rbs),), FILL, dtype=torch.uint8, device="cuda:0")
    bounds = []
    for r in range(world):                                        # what the peers hold, ready to send
        eng.bcast_pack(bks[r], nbt, stage[offs[r]: offs[r] + rbs[r]], pieces, vals=bvs[r] if mat else None)
        bounds.append(eng.bcast_pack_bounds(pieces))
        _end_step(eng, nbt)
    parts = (1, 2, 3) if mat else (1, 2)
    live = [torch.from_numpy(WM.live_mask(bits, n, mat)).cuda() for n in sizes]
    ref = C.join_reference(world, width)
    recv = torch.empty_like(stage)
    for r in range(world):
        recv.fill_(FILL)
        eng.bcast_pack(bks[r], nbt, recv[offs[r]: offs[r] + rbs[r]], pieces, vals=bvs[r] if mat else None)
        assert eng.bcast_pack_bounds(pieces) == bounds[r]
        eng.bcast_probe(pks[r], nbt)
        for q in range(pieces):
            for s in range(world):
                if s == r:
                    continue
                for part in ((0,) if q == 0 else ()) + parts:
                    o, nbytes = eng.bcast_piece_span(nbt, sizes[s], bounds[s][q], bounds[s][q + 1], part)
                    if nbytes:
                        recv[offs[s] + o: offs[s] + o + nbytes].copy_(stage[offs[s] + o: offs[s] + o + nbytes])
            eng.bcast_join(recv, offs, sizes, nparts * q // pieces, nparts * (q + 1) // pieces)
        n = eng.bcast_finish()
        assert eng.last_bcast_timings["fell_back"] == 0
        assert n == ref[r][0], f"rank {r} of {world}, {pieces} pieces: counted {n}, the reference {ref[r][0]}"
        if mat:
            k, v = eng.emit_pairs(n)
            k, v = k.cpu().numpy().view(_U), v.cpu().numpy().view(_U)
            o = np.lexsort((v, k))
            assert np.array_equal(k[o], ref[r][1]) and np.array_equal(v[o], ref[r][2]), f"rank {r} of {world}: the pairs differ from the reference's"
        for s in range(world):
            if s == r:
                continue
            a, b = recv[offs[s]: offs[s] + rbs[s]], stage[offs[s]: offs[s] + rbs[s]]
            assert torch.equal(a[live[s]], b[live[s]]), f"rank {r}: the spans of rank {s}'s pieces do not cover its region's live bytes"
            assert bool((a[~live[s]] == FILL).all())


# ---- C. exported partition filters, bit for bit --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def _filters(name, bits):
    """(the model's filters of a build side as a NumPy array, the same on the device as bytes)"""
    import torch
    f = C.model_filters(name, bits) if bits < 17 else WM.part_filters(C.filter_build(name, bits), bits)
    return f, _dev(f.reshape(-1)).view(torch.uint8)


def _assert_filters(got_u8, want_u8, what):
    import torch
    if torch.equal(got_u8, want_u8):
        return
    g, w = got_u8.view(torch.int64), want_u8.view(torch.int64)
    at = torch.nonzero(g != w).flatten()
    i = int(at[0])
    gi, wi = int(g[i]) & (2**64 - 1), int(w[i]) & (2**64 - 1)
    raise AssertionError(f"{what}: {at.numel()} blocks differ; the first: partition {i // WM.PF_BLOCKS}, block {i % WM.PF_BLOCKS}: got {gi:#018x}, the model {wi:#018x}, xor {gi ^ wi:#018x}")


def _export_all(eng, nbt, world, shares, out, fb):
    """every owner appends its share(s) of the build side and exports its filters where an all-gather would put them"""
    import torch
    for o in range(world):
        first, count, total, _ = eng.part_filter_range(nbt, world, o)
        nch = sum(int(d.numel()) for _, d in shares[o])
        eng.stream_open_shuffled(nbt, world, o, max(256, nch * 256), len(shares[o]), 1 << 20, 1)
        for ch, dw in shares[o]:
            eng.stream_append_chunks(0, ch.clone(), dw.clone())             # (directory words are rewritten in place)
        eng.stream_export_part_filters(out[first * fb: (first + count) * fb])
        torch.cuda.synchronize()
        eng.stream_abort()


@pytest.mark.parametrize("world", [1, 3, 8])
@pytest.mark.parametrize("name", C.FILTER_BUILDS)
@pytest.mark.parametrize("fan", list(C.FILTER_BITS))
def test_exported_filters(fj, opts, eng, world, fan, name):
    """First passes of 32, 64, 256 and 512 buckets (the last: 17 bits, 512 MiB of filters, model built on the host and compared on the
    device).  `crafted` in a world of 8 leaves owners without rows: they export zeros.  The owners' ranges are the model's (uneven at 3)."""
    import torch
    bits = C.FILTER_BITS[fan]
    nbt, fl0 = _shuffle_bits(eng, opts, bits, world)
    assert 1 << fl0 == fan
    build = C.filter_build(name, bits)
    _, want = _filters(name, bits)
    fb = WM.PFILT_BYTES
    for o in range(world):
        first, count, total, each = eng.part_filter_range(nbt, world, o)
        assert (first, count) == WM.filter_range(bits, fl0, world, o) and (total, each) == (1 << bits, fb)
    halves = np.array_split(build, 2) if name == "dups" else [build]        # two senders' shares per owner
    shares = [[] for _ in range(world)]
    rows = np.zeros(world, dtype=np.int64)
    for piece in halves:
        ch, dw, used = eng.shuffle_pack(_dev(piece), None, nbt, world)
        torch.cuda.synchronize()
        for o in range(world):
            shares[o].append((ch[o].clone(), dw[o].clone()))
            rows[o] += eng.chunk_rows(dw[o])
    assert np.array_equal(rows, np.bincount(WM.owner_of_bucket(C.l1_bucket(build, bits), fl0, world), minlength=world))
    if name == "crafted" and world == 8:
        assert (rows == 0).any(), "an owner without rows"
    out = torch.full((fb << bits,), FILL, dtype=torch.uint8, device="cuda:0")
    _export_all(eng, nbt, world, shares, out, fb)
    _assert_filters(out, want, f"the filters of `{name}` under {bits} bits, world {world}")
    del out


# ---- D. the in-place precheck, key for key -----------------------------------------------------------------------------------------------------------
def _wire(ch, dw, used, fl0, world):
    """every owner's share unpacked and concatenated: keys, bucket of every key, keys per chunk"""
    ks, bs, cs = [], [], []
    for r in range(world):
        assert dw[r].numel() == used[r]
        k, b, c = keymix.unpack_wire(ch[r].cpu().numpy(), dw[r].cpu().numpy(), fl0)
        assert np.all(WM.owner_of_bucket(b, fl0, world) == r), f"owner {r} receives a chunk of another owner's bucket"
        ks.append(k); bs.append(b); cs.append(c)
    return np.concatenate(ks), np.concatenate(bs), np.concatenate(cs)


def _precheck(eng, opts, probe, bname, bits, world, what, filters=None):
    import torch
    nbt, fl0 = _shuffle_bits(eng, opts, bits, world)
    f_np, f_dev = _filters(bname, bits) if filters is None else filters
    ok = WM.admits(f_np, probe, bits)
    ch, dw, used = eng.shuffle_pack(_dev(probe), None, nbt, world, filters=f_dev)
    torch.cuda.synchronize()
    wk, wb, wc = _wire(ch, dw, used, fl0, world)
    return ok, C.check_precheck(probe, ok, wk, wb, wc, eng.last_pack_kept, used, bits, what)


PRECHECK_CASES = [(n, b) for n in C.PROBE_CASES for b in C.probe_bits(n)]


@pytest.mark.parametrize("name,bits", PRECHECK_CASES, ids=[f"{n}-{b}" for n, b in PRECHECK_CASES])
def test_precheck_key_for_key(fj, opts, eng, name, bits):
    """kept == the model's count; per first-pass bucket the wire holds the admitted keys as an exact multiset, extras only for chunks that
    kept nothing.  holes: one XCD's bucket list empty, empties at the start, in the middle and at the end of others; random-17 and
    fa_twins-17: the 512-bucket plan, where lane 63 of every XCD's list holds a bucket"""
    bname, probe = C.probe_side(name, bits)
    if "F-a" in C.PROBE_DETECTS[name]:
        C.prove_fa(probe, C.filter_build(bname, bits), _filters(bname, bits)[0], bits, f"{name}-{bits}")
    _precheck(eng, opts, probe, bname, bits, 3, f"{name}, {bits} bits")


def test_every_workgroup_takes_a_second_batch(fj, opts, eng, G):
    """A piece of 12 x CUs x 1024 keys at 32 buckets: every XCD's list holds more than twice the chunks one round of batches covers
    (checked for THIS chip's workgroup count), hits in the first half of every bucket, misses in the second.  Then the same piece
    against all-zero filters: kept == 0 and every level-1 chunk travels with one key, its first.  How many level-1 chunks the first
    pass left is not visible through the API (`used` counts the DENSE wire chunks behind the squeeze), so "one key per chunk" is
    asserted as: per bucket at least ceil(n_b / 256) keys travel - a chunk holds at most 256 - and at most n_b // 256 + G + 1, the most
    chunks a first pass of G workgroups can leave (check_precheck); each of them a rejected input key, as often as it was sent at most."""
    import torch
    bits = 10
    bname, probe = C.big_piece(G, bits)
    per_round = (4 * G + 7) // 8 * 4
    n_b = np.bincount(C.l1_bucket(probe, bits), minlength=32)
    assert min(int((n_b[x::8] // C.CHUNK).sum()) for x in range(8)) > 2 * per_round, "an XCD's workgroups need no second batch: enlarge big_piece"
    ok, _ = _precheck(eng, opts, probe, bname, bits, 1, f"the big piece ({probe.size} keys)")
    assert ok[: probe.size // 2].all()
    zeros_np = np.zeros((1 << bits, WM.PF_BLOCKS), dtype=_U)
    zeros = torch.zeros(WM.PFILT_BYTES << bits, dtype=torch.uint8, device="cuda:0")
    ok, extras = _precheck(eng, opts, probe, bname, bits, 1, "the big piece against zero filters", filters=(zeros_np, zeros))
    assert not ok.any() and eng.last_pack_kept == 0
    assert np.all(extras >= -(-n_b // C.CHUNK)), "fewer keys travel than the bucket has chunks: a chunk without survivors vanished"

def test_owners_join_the_prechecked_shares(fj, opts, eng):
    """the whole chain at 64 buckets, world 3: the owners export their filters from the build shares, the probe side is prechecked against
    THEIR filters (equal to the model's), the owners join what is left: the reference's count"""
    import torch
    bits, world = 12, 3
    nbt, fl0 = _shuffle_bits(eng, opts, bits, world)
    bname, probe = C.probe_side("random", bits)
    build = C.filter_build(bname, bits)
    ch, dw, used = eng.shuffle_pack(_dev(build), None, nbt, world)
    torch.cuda.synchronize()
    bshare = [(ch[o].clone(), dw[o].clone()) for o in range(world)]
    fb = WM.PFILT_BYTES
    filters = torch.full((fb << bits,), FILL, dtype=torch.uint8, device="cuda:0")
    _export_all(eng, nbt, world, [[s] for s in bshare], filters, fb)
    f_np, f_dev = _filters(bname, bits)
    _assert_filters(filters, f_dev, "the owners' filters")
    ok, _ = _precheck(eng, opts, probe, bname, bits, world, "the probe side", filters=(f_np, filters))
    pch, pdw, pused = eng.shuffle_pack(_dev(probe), None, nbt, world, filters=filters)
    torch.cuda.synchronize()
    pshare = [(pch[o].clone(), pdw[o].clone()) for o in range(world)]
    total = 0
    for o in range(world):
        eng.stream_open_shuffled(nbt, world, o, max(256, used[o] * 256), 1, max(256, pused[o] * 256), 1)
        eng.stream_append_chunks(0, *bshare[o])
        eng.stream_append_chunks(1, *pshare[o])
        total += eng.stream_finish()
    assert total == int(np.isin(probe, build).sum())


# ---- E. the sample ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", C.SAMPLE_STRIDES)
def test_the_sample(fj, opts, eng, stride):
    """kept == the model's count over raw[::stride][:n]; what lies between the sampled keys is random (a kernel that ignored the stride
    would count about 1 / stride of it)"""
    import torch
    bits = 10
    nbt, _ = _shuffle_bits(eng, opts, bits, 1)
    bname, keys = C.sample_keys(bits)
    f_np, f_dev = _filters(bname, bits)
    ok = WM.admits(f_np, keys, bits)
    g = torch.Generator(device="cuda:0")
    g.manual_seed(20261109 + stride)
    raw = torch.randint(-2**62, 2**62, ((keys.size - 1) * stride + 1,), dtype=torch.int64, device="cuda:0", generator=g)
    raw[::stride] = _dev(keys)
    for n in C.SAMPLE_N:
        got = eng.part_filter_sample(raw, n, stride, f_dev, nbt, 1)
        assert got == int(ok[:n].sum()), f"stride {stride}, n {n}: kept {got}, the model {int(ok[:n].sum())}"
    del raw
