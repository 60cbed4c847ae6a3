"""The per-sample reductions and the L2 / L1 image updates of csrc/lnorm.hip on the MI355X: ``sumsq_stage1``,
``sumabs_stage1``, ``absmax_stage1/2``, ``sum_stage2`` and ``per_sample_kernel`` behind ``vqa_sumsq_per_sample``,
``vqa_sumabs_per_sample``, ``vqa_absmax_ties_per_sample``, ``vqa_l2_fgm``, ``vqa_l2_project``, ``vqa_l1_fgm`` and
``vqa_scale_per_sample``.

Rules of this file:

1. Reductions, exact integers.  Inputs are small integers stored as fp32 (t in [-4, 4] for the sum of squares, t and sub
   in [-2, 2] for the sum of squares of a difference, [-4, 4] for the sum of magnitudes), so every partial sum is an
   integer below 2^24 and exact in ANY order: the premise is asserted on the host in int64, the kernel's result must then
   EQUAL the int64 sum cast to fp32.  One dropped or double-counted element changes the sum by at least 1 unless it is a
   0, and a dropped 16-byte piece with four zeros is as likely as 9^-4.  Three chunk regimes are hit and asserted:
   1 < chunks < 512, chunks capped to 1 by a large batch, chunks capped at 512 by one large sample.  (At the 512-chunk
   size, 4 194 308 elements, the draws are narrowed to {-1, 1} and [-1, 1]: 16 * n_per would pass 2^24.)
2. One planted +-1 per sample of a zero tensor, at every 256-lane / 4096- / 8192-element tile edge and at the first and
   last element of every chunk: both sums, the maximum and the tie count must be exactly 1; an all-zero and an all-(-0.0)
   sample give sums 0, maximum +0.0 and n_per ties.
3. (max, count) merging across tiles and chunks on integer data: decoy below the maximum, a maximum spread over tiles and
   chunks, a maximum attained by negative values only, NaN and inf samples next to clean ones -- against
   ``t.abs().flatten(1).max(1)`` and the ``eq`` count, as ``oracle.cleverhans_cpu.optimize_linear`` forms them.
4. Elementwise updates: the statistic is read back from its own kernel (part 1 shows it deterministic), the chain is
   evaluated in numpy fp32 with one rounded operation at a time in the order of ``norm_apply`` -- the order of the
   reference's ``optimize_linear`` / ``clip_eta`` / ``_project``, with its NaN-propagating ``torch.max`` / ``torch.min``
   -- and the kernel's result must have the SAME BITS (``_assert_bits``; two NaNs count as equal whatever their payload).
   Parts 1 to 4 know no tolerance.
5. Real-valued data: the three sums against float64 at the project's bar ``NORM_RTOL`` of tests/test_hip_kernels.py, with
   the error of ``torch.sum`` in fp32 on the same device tensor printed next to the kernel's as a yardstick, and equal bits
   from two runs.
6. Entry points, straight through the C ABI: every refusal (shape, alignment, NULL, kind) and every zero extent leaves
   sentinel-filled outputs, workspace and flag word untouched.

``_place(t, misalign)`` puts a tensor on the device at a 16-byte aligned address or one float behind one;
``_chunks(batch, n_per)`` is the library's own answer (``vqa_reduce_ws_bytes // (8 * batch)``), so nothing here depends
on the number of compute units.  The largest tensors (134 MB: 4096 x 8200; 175 MB of zeros for the planted elements of
99 x 442 368, one sample per chunk edge) are built on the device.
"""
import functools

import numpy as np
import pytest
import torch

from tests.test_hip_kernels import NORM_RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
VQA_ERR_NULL, VQA_ERR_SHAPE, VQA_ERR_ALIGN = -1, -2, -3          # include/vqattack_hip.h
ALIGNED_OFFSET = pytest.mark.parametrize("misalign", [False, True], ids=["aligned", "offset"])


def _ops():
    from vqattack_amd import ops
    return ops


def _lib():
    from vqattack_amd import _hip
    return _hip.lib()


def _zeros(shape, misalign=False, dtype=torch.float32):
    """A zero-filled device tensor at a 16-byte aligned address, or one float (4 bytes) behind one."""
    numel = int(np.prod(shape))
    buf = torch.zeros(numel + 1, dtype=dtype, device=DEV)
    view = (buf[1:] if misalign else buf[:numel]).view(shape)
    assert view.data_ptr() % 16 == (4 if misalign else 0) and view.is_contiguous()
    return view


def _place(t, misalign=False):
    """Host array / tensor (or a device tensor) -> device tensor, 16-byte aligned or one float off (``buf[1:].view``)."""
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not misalign:
        d = t.contiguous().to(DEV)
        assert d.data_ptr() % 16 == 0
        return d
    view = _zeros(t.shape, True, t.dtype)
    view.copy_(t)
    return view


def _chunks(batch, n_per):
    """Partials per sample of a reduction of (batch, n_per), as the library itself sizes its workspace."""
    return _lib().vqa_reduce_ws_bytes(batch, n_per) // (8 * batch)


def _chunk_edges(n_per, chunks):
    """First and last element of every non-empty chunk.  The rule of chunk_bounds (csrc/lnorm.hip): a sample is cut into
    16-byte pieces, n4 = ceil(n_per / 4) of them; every chunk takes per = ceil(n4 / chunks) pieces, so chunk c holds the
    elements [4 * per * c, 4 * per * (c + 1)), both ends cut at n_per -- the last chunks may be empty."""
    n4 = -(-n_per // 4)
    per = -(-n4 // chunks)
    edges = []
    for c in range(chunks):
        lo, hi = min(4 * per * c, n_per), min(4 * per * (c + 1), n_per)
        if lo < hi:
            edges += [lo, hi - 1]
    return edges


def _assert_bits(got, want, what):
    """Equal bits everywhere (a NaN equals a NaN: the payload of a produced NaN is the processor's choice); reports the
    number of differing elements and the first of them."""
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype == F, what
    same = (got.view(np.int32) == want.view(np.int32)) | (np.isnan(got) & np.isnan(want))
    if not same.all():
        first = np.unravel_index(int(np.argmin(same)), same.shape)
        raise AssertionError("{}: {} of {} elements differ, first at {}: got {!r} want {!r}".format(
            what, int((~same).sum()), same.size, tuple(int(i) for i in first), got[first], want[first]))


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. exact integers
N_PER = [1, 2, 3, 4, 5, 7, 1023, 1024, 1025, 4095, 4096, 4097, 4100, 8191, 8192, 8196, 12289, 442368, 442371]
BATCHES = (1, 2, 3, 9)


@functools.lru_cache(maxsize=2)
def _int_data(n_per):
    """One draw of (9, n_per) per size, the smaller batches are its leading samples.  Returns the fp32 tensors and the
    int64 per-sample sums."""
    r = np.random.RandomState(n_per % 9973)
    t = r.randint(-4, 5, (9, n_per))
    a, b = r.randint(-2, 3, (9, n_per)), r.randint(-2, 3, (9, n_per))
    sums = ((t * t).sum(1), ((a - b) ** 2).sum(1), np.abs(t).sum(1), np.abs(t).max(1),
            (np.abs(t) == np.abs(t).max(1, keepdims=True)).sum(1))
    assert all(s.dtype == np.int64 for s in sums)
    return tuple(v.astype(F) for v in (t, a, b)), sums


def _as_f32(int_sums):
    return torch.from_numpy(np.asarray(int_sums).astype(F))


@ALIGNED_OFFSET
@pytest.mark.parametrize("n_per", N_PER)
def test_reductions_are_exact_on_small_integers(n_per, misalign):
    ops = _ops()
    (t, a, b), (sq, sqd, ab, top, ties) = _int_data(n_per)
    assert max(int(sq.max()), int(sqd.max()), int(ab.max())) < 2 ** 24          # the premise: exact in any order
    for batch in BATCHES:
        td, ad, bd = (_place(v[:batch], misalign) for v in (t, a, b))
        what = "n_per {} batch {} chunks {}".format(n_per, batch, _chunks(batch, n_per))
        assert torch.equal(ops.sumsq_per_sample(td).cpu(), _as_f32(sq[:batch])), what
        assert torch.equal(ops.sumabs_per_sample(td).cpu(), _as_f32(ab[:batch])), what
        assert torch.equal(ops.sumsq_per_sample(ad, sub=bd).cpu(), _as_f32(sqd[:batch])), what
        if misalign:                                     # ONE operand off its 16-byte boundary, either of the two
            assert torch.equal(ops.sumsq_per_sample(ad, sub=_place(b[:batch])).cpu(), _as_f32(sqd[:batch])), what
            assert torch.equal(ops.sumsq_per_sample(_place(a[:batch]), sub=bd).cpu(), _as_f32(sqd[:batch])), what
        amax, cnt = ops.absmax_ties_per_sample(td)
        assert torch.equal(amax.cpu(), _as_f32(top[:batch])) and torch.equal(cnt.cpu(), _as_f32(ties[:batch])), what


def _device_ints(shape, lo, hi, gen, misalign):
    """Integers in [lo, hi] as fp32, drawn on the device."""
    return _place(torch.randint(lo, hi + 1, shape, device=DEV, generator=gen, dtype=torch.int8).float(), misalign)


def _int_sums_on_host(t, sub=None):
    """int64 per-sample sums of squares and of magnitudes (the integers are formed on the device, the sums asserted and
    compared on the host)."""
    d = (t if sub is None else t - sub).to(torch.int32)
    sq, ab = (d * d).sum(1).cpu(), d.abs().sum(1).cpu()
    assert sq.dtype == torch.int64 and int(sq.max()) < 2 ** 24 and int(ab.max()) < 2 ** 24
    return sq.float(), ab.float()


@ALIGNED_OFFSET
def test_reductions_with_one_chunk_per_sample_because_the_batch_is_large(misalign):
    """chunks = min(ceil(n_per / 4096), 512, 2 * grid_cap / batch): the last term is 1 from batch = 2 * grid_cap on
    (4096 on 256 compute units, 134 MB at n_per = 8200); one workgroup then sweeps two whole tiles and a partial one."""
    ops = _ops()
    n_per, batch = 8200, 1
    while batch <= 16384 and _chunks(batch, n_per) != 1:
        batch *= 2
    if batch > 16384:
        pytest.skip("no power-of-two batch up to 16384 caps the reduction of 8200 elements to one chunk on this device")
    assert _chunks(batch, n_per) == 1 and _chunks(batch // 2, n_per) > 1
    assert 1 < _chunks(2, 442368) < 512                                     # the regime of the general shapes
    gen = torch.Generator(DEV).manual_seed(8200)
    t = _device_ints((batch, n_per), -4, 4, gen, misalign)
    sq, ab = _int_sums_on_host(t)
    assert torch.equal(ops.sumsq_per_sample(t).cpu(), sq)
    assert torch.equal(ops.sumabs_per_sample(t).cpu(), ab)
    del t
    a, b = _device_ints((batch, n_per), -2, 2, gen, misalign), _device_ints((batch, n_per), -2, 2, gen, False)
    sqd, _ = _int_sums_on_host(a, b)
    assert torch.equal(ops.sumsq_per_sample(a, sub=b).cpu(), sqd)


@ALIGNED_OFFSET
def test_reductions_with_the_chunk_count_capped_at_512(misalign):
    """One sample of 512 * 4096 * 2 + 4 elements: 512 chunks of 2049 pieces (the last one shorter).  16 * n_per is past
    2^24, so the draws are {-1, 1} (every element counts 1: n_per itself must come out) and [-1, 1]."""
    ops = _ops()
    n_per = 512 * 4096 * 2 + 4
    assert _chunks(1, n_per) == 512
    gen = torch.Generator(DEV).manual_seed(512)
    ones = _place(torch.randint(0, 2, (1, n_per), device=DEV, generator=gen, dtype=torch.int8).float() * 2 - 1, misalign)
    near = _place(ones + (torch.randint(0, 2, (1, n_per), device=DEV, generator=gen, dtype=torch.int8).float() * 2 - 1),
                  False)                                                    # in {-2, 0, 2}: ones - near is +-1
    sq, ab = _int_sums_on_host(ones)
    assert int(sq[0]) == n_per and int(ab[0]) == n_per
    assert torch.equal(ops.sumsq_per_sample(ones).cpu(), sq) and torch.equal(ops.sumabs_per_sample(ones).cpu(), ab)
    sqd, _ = _int_sums_on_host(ones, near)
    assert int(sqd[0]) == n_per and torch.equal(ops.sumsq_per_sample(ones, sub=near).cpu(), sqd)
    t = _device_ints((1, n_per), -1, 1, gen, misalign)
    sq, ab = _int_sums_on_host(t)
    assert torch.equal(ops.sumsq_per_sample(t).cpu(), sq) and torch.equal(ops.sumabs_per_sample(t).cpu(), ab)
    sqd, _ = _int_sums_on_host(t, ones)
    assert torch.equal(ops.sumsq_per_sample(t, sub=ones).cpu(), sqd)


# ------------------------------------------------------------------------------------------------ 2. planted elements
def _planted_positions(n_per):
    """One position per sample (+ the two zero samples = the batch).  The chunk edges depend on the batch through
    ``_chunks``; a larger batch never has more chunks, so growing the batch to the number of positions settles."""
    fixed = [0, 1, 3, 4] + list(range(n_per - 5, n_per)) + [1023, 1024, 4095, 4096, 8191, 8192]
    batch = len(fixed) + 2
    while True:
        pos = sorted(set(fixed + _chunk_edges(n_per, _chunks(batch, n_per))))
        if len(pos) + 2 <= batch:
            break
        batch = len(pos) + 2
    return [pos[i % len(pos)] for i in range(batch - 2)], _chunks(batch, n_per)


@ALIGNED_OFFSET
@pytest.mark.parametrize("n_per", [12289, 12292, 442368])
def test_one_planted_element_per_sample_is_counted_exactly_once(n_per, misalign):
    ops = _ops()
    pos, chunks = _planted_positions(n_per)
    planted = len(pos)
    assert chunks > 1 and all(0 <= p < n_per for p in pos)
    t = _zeros((planted + 2, n_per), misalign)
    rows = torch.arange(planted, device=DEV)
    t[rows, torch.tensor(pos, device=DEV)] = torch.where(rows % 2 == 0, 1.0, -1.0)
    t[planted + 1] = -0.0
    assert _chunks(planted + 2, n_per) == chunks
    want = torch.cat([torch.ones(planted), torch.zeros(2)])
    want_ties = torch.cat([torch.ones(planted), torch.full((2,), float(n_per))])
    amax, ties = ops.absmax_ties_per_sample(t)
    for name, got, exp in (("sumsq", ops.sumsq_per_sample(t), want), ("sumabs", ops.sumabs_per_sample(t), want),
                           ("amax", amax, want), ("ties", ties, want_ties)):
        got = got.cpu()
        wrong = [(i, pos[i] if i < planted else "zeros", float(got[i])) for i in torch.nonzero(got != exp).flatten().tolist()]
        assert not wrong, "{} with {} chunks: (sample, planted position, result) {}".format(name, chunks, wrong[:8])
    assert torch.equal(amax.cpu().view(torch.int32)[planted:], torch.zeros(2, dtype=torch.int32))     # +0.0, not -0.0


# ------------------------------------------------------------------------------------------------ 3. maximum and ties
TILE = 8192            # elements of one register-resident tile of absmax_stage1: 256 lanes x kTieU = 8 pieces x 4
KINDS = ("decoy", "spread", "negative", "inf", "clean", "nan", "clean")         # a NaN sample between two clean ones


def _tie_plants(kind, n_per, chunks):
    """{position: value} over a background of integers in [-3, 3]."""
    n4 = -(-n_per // 4)
    chunk = 4 * -(-n4 // chunks)                                                # elements per chunk (rule: _chunk_edges)
    if kind == "decoy":           # hundreds of 5s in the first tile, the one 9 in the last, partial, tile of the sample
        plants = {p: (5.0 if p % 6 else -5.0) for p in range(0, min(chunk, TILE, n_per - 8), 3)}
        plants[n_per - 2] = 9.0
    elif kind == "spread":        # first and last element of tile 0, last of tile 1, last of the sample ...
        plants = {0: 9.0, TILE - 1: 9.0, 2 * TILE - 1: -9.0, n_per - 1: 9.0}
        if chunks >= 4:           # ... the first element of three more chunks ...
            plants.update({(chunks * k // 4) * chunk: -9.0 for k in (1, 2, 3)})
        if chunk > TILE:          # ... and, where a chunk has several tiles, the end of one tile and the start of the last
            plants[chunk + TILE - 1] = 9.0
            plants[2 * chunk + (chunk - 1) // TILE * TILE] = 9.0
        plants = {p: v for p, v in plants.items() if p < n_per}                # the one-chunk size has no tile 1
        assert len(plants) >= 3
    elif kind == "negative":
        plants = {1: -7.0, TILE - 3: -7.0, n_per - 3: -7.0}
    elif kind == "inf":
        plants = {2: float("inf"), n_per // 2: float("inf"), n_per - 1: float("-inf")}
    elif kind == "nan":
        plants = {n_per - 1: float("nan")}
    else:
        plants = {}
    return plants


def _check_ties(n_per, batch, kinds, misalign, seed):
    """Samples 0 .. len(kinds) - 1 carry the plants, every further sample is background."""
    ops = _ops()
    chunks = _chunks(batch, n_per)
    t = _device_ints((batch, n_per), -3, 3, torch.Generator(DEV).manual_seed(seed), misalign)
    count = {}
    for row, kind in enumerate(kinds):
        plants = _tie_plants(kind, n_per, chunks)
        if plants:
            t[row, torch.tensor(sorted(plants), device=DEV)] = torch.tensor([plants[p] for p in sorted(plants)], device=DEV)
        count[row] = len(plants)
    mag = t.abs().flatten(1)
    want_max = mag.max(1).values                                               # torch.max propagates NaN ...
    want_ties = mag.eq(want_max[:, None]).sum(1).float()                       # ... and nothing equals it
    amax, ties = ops.absmax_ties_per_sample(t)
    amax, ties, want_max, want_ties = amax.cpu(), ties.cpu(), want_max.cpu(), want_ties.cpu()
    what = "n_per {} batch {} chunks {}".format(n_per, batch, chunks)
    for row, kind in enumerate(kinds):
        a, c = float(amax[row]), float(ties[row])
        if kind == "decoy":
            assert (a, c) == (9.0, 1.0), (what, kind, a, c)
        elif kind == "spread":
            assert (a, c) == (9.0, float(count[row])), (what, kind, a, c, count[row])
        elif kind == "negative":
            assert (a, c) == (7.0, 3.0), (what, kind, a, c)
        elif kind == "inf":
            assert (a, c) == (float("inf"), 3.0), (what, kind, a, c)
        elif kind == "nan":
            assert a != a and c == 0.0 and bool(torch.isnan(want_max[row])), (what, kind, a, c)
        else:
            assert a == 3.0 and c > 1.0, (what, kind, a, c)
    clean = ~torch.isnan(want_max)
    assert int((~clean).sum()) == sum(k == "nan" for k in kinds)
    assert torch.equal(amax[clean], want_max[clean]) and torch.equal(ties, want_ties), what
    return chunks


@ALIGNED_OFFSET
def test_maximum_and_tie_count_across_chunks(misalign):
    """n_per = 3 * 8192 + 4 at batch 7: seven chunks of 3512 elements, the merge of absmax_stage2."""
    assert 1 < _check_ties(3 * TILE + 4, len(KINDS), KINDS, misalign, 3) < 512


@ALIGNED_OFFSET
@pytest.mark.parametrize("kinds", [KINDS[:4], KINDS[4:]], ids=["decoy-spread-negative-inf", "clean-nan-clean"])
def test_maximum_and_tie_count_across_tiles_and_chunks(kinds, misalign):
    """512 chunks of 2 * 8192 + 4 elements: two whole tiles and a partial one per chunk, merged in absmax_stage1 (a larger
    maximum in a later tile resets the count, an equal one adds), then 512 partial pairs in absmax_stage2.  33.5 MB per
    sample, hence two launches."""
    assert _check_ties(512 * (2 * TILE + 4), len(kinds), kinds, misalign, 4) == 512


@ALIGNED_OFFSET
def test_maximum_and_tie_count_across_the_tiles_of_one_chunk(misalign):
    """8196 elements in ONE chunk (large batch): a whole tile and a partial one of a single piece, whose padding lanes are
    filled with -1 and must not tie.  The decoy's 9 sits in that last piece; the other samples are background."""
    n_per, batch = TILE + 4, 1
    while batch <= 16384 and _chunks(batch, n_per) != 1:
        batch *= 2
    if batch > 16384:
        pytest.skip("no power-of-two batch up to 16384 caps the reduction of 8196 elements to one chunk on this device")
    assert _check_ties(n_per, batch, KINDS, misalign, 5) == 1


# ------------------------------------------------------------------------------------------------ 4. elementwise chain
def _per(stat, like):
    return stat.astype(F).reshape((-1,) + (1,) * (like.ndim - 1))


def _length(stat):
    return np.sqrt(np.maximum(F(1e-12), stat))              # torch.max(tiny, sum) -> sqrt; a NaN sum stays NaN


def _factor(stat, eps):
    """torch.min(1, eps / length) with ONE correctly rounded division, as norm_apply and the C ABI state it.  (torch forms
    ``python_float / tensor`` as ``tensor.reciprocal() * python_float``, two roundings: the reference's factor can differ
    from this one in its last bit, inside the 5e-6 that tests/test_hip_kernels.py holds the L2 path to against the oracle.)"""
    return np.minimum(F(1), F(eps) / _length(stat))


def _clamp(v, clip):
    assert v.dtype == F
    return np.minimum(np.maximum(v, F(-1)), F(1)) if clip else v


def _sign(g):
    return (g > 0).astype(F) - (g < 0).astype(F)


def _hit(g, amax):
    return (np.abs(g) == _per(amax, g)).astype(F)


def chain_l2_fgm(x, g, sumsq, eps, clip):
    return _clamp(x + F(eps) * (g / _length(_per(sumsq, g))), clip)


def chain_l2_project(adv, x0, sumsq, eps, clip):
    return _clamp(x0 + (adv - x0) * _factor(_per(sumsq, adv), eps), clip)


def chain_l1_fgm(x, g, amax, ties, eps, clip):
    return _clamp(x + F(eps) * (_sign(g) * _hit(g, amax) / _per(ties, g)), clip)


def chain_scale(t, stat, stat2, eps, kind):
    if kind == 0:
        return t * _factor(_per(stat, t), eps)
    if kind == 1:
        return F(eps) * (t / _length(_per(stat, t)))
    return F(eps) * (_sign(t) * _hit(t, stat) / _per(stat2, t))


# (8, 1105924): launch_per_sample gives the vector kernel min(tiles, grid_cap / min(batch, 8)) workgroups per sample with
# grid_cap = 8 workgroups x 256 compute units = 2048 -> 256 at batch 8; a tile is 256 lanes x kRedU = 4 pieces = 4096
# elements, so one sweep of the grid covers 1 048 576 elements of a sample.  270 * 4096 + 4 elements are 270 whole tiles
# and one piece: workgroups 0 .. 14 run two tiles.  The scalar kernel's 256 workgroups sweep 65 536 elements: 17 rounds.
SHAPES = {"2x3x32x32": (2, 3, 32, 32), "3x3x5x7": (3, 3, 5, 7), "9x4100": (9, 4100), "11x1x1x3": (11, 1, 1, 3),
          "8x1105924": (8, 270 * 4096 + 4)}
EPS_FGM, EPS_BALL = 0.7, 0.3


@functools.lru_cache(maxsize=2)
def _data(name):
    """x0 in [-1, 1], x inside its 0.05-ball, a normal gradient, and adv = x0 + eta with |eta|_2 alternately half and
    three times the projection radius -- drawn once per shape and never changed."""
    shape = SHAPES[name]
    r = np.random.RandomState(len(name) + shape[-1] % 1000)
    x0 = r.uniform(-1, 1, shape).astype(F)
    x = np.clip(x0 + r.uniform(-0.05, 0.05, shape).astype(F), -1, 1).astype(F)
    g = r.standard_normal(shape).astype(F)
    u = r.standard_normal(shape)
    norm = np.sqrt((u.reshape(shape[0], -1) ** 2).sum(1)).reshape((-1,) + (1,) * (len(shape) - 1))
    radius = np.where(np.arange(shape[0]) % 2 == 0, 0.5, 3.0).reshape(norm.shape) * EPS_BALL
    adv = (x0 + (u / norm * radius).astype(F)).astype(F)
    return dict(x=x, x0=x0, g=g, adv=adv)


def _run_chain_case(host, align, mode):
    """Every operation once; ``align``: which operand sits one float off a 16-byte boundary (aligned / first / second /
    out); ``mode``: clip / noclip / inplace (with clip; out is x, adv or t)."""
    ops = _ops()
    clip = mode != "noclip"
    lo, hi = (-1.0, 1.0) if clip else (None, None)
    x, g, x0, adv = (host[k] for k in ("x", "g", "x0", "adv"))

    def first(a):
        return _place(a, align == "first")

    def out_for(t):
        return t if mode == "inplace" else _zeros(t.shape, align == "out")

    gd = _place(g, align == "second")
    ss = ops.sumsq_per_sample(gd).cpu().numpy()
    xd = first(x)
    got = ops.l2_fgm(xd, gd, EPS_FGM, lo, hi, out=out_for(xd))
    _assert_bits(got, chain_l2_fgm(x, g, ss, EPS_FGM, clip), "l2_fgm")

    advd, x0d = first(adv), _place(x0, align == "second")
    ss_eta = ops.sumsq_per_sample(advd, sub=x0d).cpu().numpy()
    got = ops.l2_project(advd, x0d, EPS_BALL, lo, hi, out=out_for(advd))
    _assert_bits(got, chain_l2_project(adv, x0, ss_eta, EPS_BALL, clip), "l2_project")

    amax, ties = ops.absmax_ties_per_sample(gd)
    xd = first(x)
    got = ops.l1_fgm(xd, gd, EPS_FGM, lo, hi, out=out_for(xd))
    _assert_bits(got, chain_l1_fgm(x, g, amax.cpu().numpy(), ties.cpu().numpy(), EPS_FGM, clip), "l1_fgm")

    for kind in (0, 1, 2):
        td = first(g)
        if kind < 2:
            stat, stat2 = ops.sumsq_per_sample(td), None
        else:
            stat, stat2 = ops.absmax_ties_per_sample(td)
        out = td if (mode == "inplace" and kind == 0) else _zeros(td.shape, align == "out")
        got = ops.scale_per_sample(td, stat, stat2, EPS_BALL, kind, out=out)
        assert got is out
        _assert_bits(got, chain_scale(g, stat.cpu().numpy(), None if stat2 is None else stat2.cpu().numpy(), EPS_BALL, kind),
                     "scale_per_sample kind {}".format(kind))


CHAIN_CASES = [(a, m) for m in ("clip", "noclip") for a in ("aligned", "first", "second", "out")] + \
              [("aligned", "inplace"), ("first", "inplace")]


@pytest.mark.parametrize("align,mode", CHAIN_CASES, ids=["-".join(c) for c in CHAIN_CASES])
@pytest.mark.parametrize("name", [n for n in SHAPES if n != "8x1105924"])
def test_updates_equal_the_numpy_fp32_chain_bitwise(name, align, mode):
    _run_chain_case(_data(name), align, mode)


@pytest.mark.parametrize("align,mode", [("aligned", "clip"), ("first", "noclip"), ("aligned", "inplace")],
                         ids=["aligned-clip", "first-noclip", "aligned-inplace"])
def test_updates_where_a_workgroup_runs_more_than_one_tile(align, mode):
    _run_chain_case(_data("8x1105924"), align, mode)


EDGE_SHAPES = {"6x4100": ((6, 4100), False), "6x4100-offset": ((6, 4100), True), "6x3x5x7": ((6, 3, 5, 7), False)}


@pytest.mark.parametrize("name", sorted(EDGE_SHAPES))
def test_l2_edge_samples(name):
    """Gradient samples: normal | zero (the 1e-12 floor) | sum of squares just under 1e-12 | just over | NaN in one element
    (the sum, and so the whole sample, is NaN -- torch.max(tiny, NaN) is NaN) | normal.  Projection samples: eta inside
    the ball (factor exactly 1) | far outside | inside | outside | NaN in one element | inside."""
    ops = _ops()
    shape, misalign = EDGE_SHAPES[name]
    r = np.random.RandomState(shape[-1])
    x0 = r.uniform(-1, 1, shape).astype(F)
    x = np.clip(x0 + r.uniform(-0.05, 0.05, shape).astype(F), -1, 1).astype(F)
    g = r.standard_normal(shape).astype(F)
    g[1] = 0.0
    for row, target in ((2, 0.999e-6), (3, 1.001e-6)):
        g[row] = (g[row] * (target / np.sqrt((g[row].astype(np.float64) ** 2).sum()))).astype(F)
    g[4].reshape(-1)[5] = np.nan
    eta = r.standard_normal(shape)
    eta /= np.sqrt((eta.reshape(6, -1) ** 2).sum(1)).reshape((6,) + (1,) * (len(shape) - 1))
    for row, radius in enumerate((0.5, 1000.0, 0.9, 1.1, 0.5, 0.01)):
        eta[row] *= radius * EPS_BALL
    adv = (x0 + eta.astype(F)).astype(F)
    adv[4].reshape(-1)[7] = np.nan
    xd, gd, x0d, advd = (_place(v, misalign) for v in (x, g, x0, adv))

    ss = ops.sumsq_per_sample(gd).cpu().numpy()
    assert ss[1] == 0 and 0 < ss[2] < F(1e-12) < ss[3] and np.isnan(ss[4])         # the regimes the samples are meant for
    with np.errstate(invalid="ignore"):
        for clip in (True, False):
            lo, hi = (-1.0, 1.0) if clip else (None, None)
            got = ops.l2_fgm(xd, gd, EPS_FGM, lo, hi)
            _assert_bits(got, chain_l2_fgm(x, g, ss, EPS_FGM, clip), "l2_fgm")
            got = got.cpu().numpy()
            assert np.array_equal(got[1], x[1]) and np.isnan(got[4]).all() and not np.isnan(got[[0, 1, 2, 3, 5]]).any()
        for kind in (0, 1):
            got = ops.scale_per_sample(gd, ops.sumsq_per_sample(gd), None, EPS_BALL, kind)
            _assert_bits(got, chain_scale(g, ss, None, EPS_BALL, kind), "kind {}".format(kind))
            assert np.isnan(got[4].cpu().numpy()).all()

        ss_eta = ops.sumsq_per_sample(advd, sub=x0d).cpu().numpy()
        radius = np.sqrt(ss_eta)
        assert (radius[[0, 2, 5]] < EPS_BALL).all() and (radius[[1, 3]] > EPS_BALL).all() and np.isnan(radius[4])
        for clip in (True, False):
            lo, hi = (-1.0, 1.0) if clip else (None, None)
            got = ops.l2_project(advd, x0d, EPS_BALL, lo, hi)
            _assert_bits(got, chain_l2_project(adv, x0, ss_eta, EPS_BALL, clip), "l2_project")
            got = got.cpu().numpy()
            for row in (0, 2, 5):                                                   # factor exactly 1
                assert np.array_equal(got[row], _clamp(x0[row] + (adv[row] - x0[row]), clip))
            far = np.sqrt(((got[1].astype(np.float64) - x0[1]) ** 2).sum())
            assert np.isnan(got[4]).all() and not np.isnan(got[[0, 1, 2, 3, 5]]).any() and (clip or far < EPS_BALL * 1.001)


@pytest.mark.parametrize("name", sorted(EDGE_SHAPES))
def test_l1_edge_samples(name):
    """normal | three-way tie with mixed signs | zero gradient | normal | NaN in one element | normal.  The reference
    (utils.py:88-99) gives the zero gradient ``sign * mask / n`` = 0 -- no perturbation, every element ties and its
    self-check fires -- and the NaN gradient ``0 / 0``: that sample, and only that one, is NaN."""
    ops = _ops()
    from vqattack_amd._hip import VQA_FLAG_DEGENERATE
    shape, misalign = EDGE_SHAPES[name]
    n = int(np.prod(shape[1:]))
    r = np.random.RandomState(shape[-1] + 1)
    x = r.uniform(-0.9, 0.9, shape).astype(F)
    g = r.standard_normal(shape).astype(F)
    g[1].reshape(-1)[[0, n // 2, n - 1]] = (8.0, -8.0, 8.0)
    g[2] = 0.0
    g[4].reshape(-1)[n - 2] = np.nan
    xd, gd = _place(x, misalign), _place(g, misalign)
    amax, ties = (v.cpu().numpy() for v in ops.absmax_ties_per_sample(gd))
    assert (amax[1], ties[1]) == (8.0, 3.0) and (amax[2], ties[2]) == (0.0, float(n)) and np.isnan(amax[4]) and ties[4] == 0
    with np.errstate(invalid="ignore", divide="ignore"):
        for clip in (True, False):
            lo, hi = (-1.0, 1.0) if clip else (None, None)
            flag = ops.new_flag(DEV)
            got = ops.l1_fgm(xd, gd, EPS_FGM, lo, hi, flag=flag)
            _assert_bits(got, chain_l1_fgm(x, g, amax, ties, EPS_FGM, clip), "l1_fgm")
            got = got.cpu().numpy()
            assert int(flag.item()) == VQA_FLAG_DEGENERATE
            assert np.array_equal(got[2], x[2]) and np.isnan(got[4]).all() and not np.isnan(got[[0, 1, 2, 3, 5]]).any()
            moved = np.flatnonzero(got[1].reshape(-1) != x[1].reshape(-1))
            assert moved.tolist() == [0, n // 2, n - 1]
        stat, stat2 = ops.absmax_ties_per_sample(gd)
        _assert_bits(ops.scale_per_sample(gd, stat, stat2, EPS_BALL, 2), chain_scale(g, amax, ties, EPS_BALL, 2), "kind 2")


def test_flags_degenerate_and_range_bits():
    ops = _ops()
    from vqattack_amd._hip import VQA_FLAG_DEGENERATE as DEG
    from vqattack_amd._hip import VQA_FLAG_RANGE as RANGE
    shape = (3, 4100)
    r = np.random.RandomState(11)
    x = r.uniform(-0.9, 0.9, shape).astype(F)
    g = r.standard_normal(shape).astype(F)

    def variant(a, row, where, value):
        a = a.copy()
        if where is None:
            a[row] = value
        else:
            a[row, where] = value
        return _place(a)

    xd, gd = _place(x), _place(g)
    x_out = variant(x, 2, 4099, 1.5)
    g_zero, g_nan, g_huge = variant(g, 1, None, 0.0), variant(g, 1, 17, np.nan), variant(g, 1, 17, 3e19)   # 9e38 > FLT_MAX

    def run(op, xt, gt, clip=True, **kw):
        flag = ops.new_flag(DEV)
        op(xt, gt, EPS_FGM, -1.0 if clip else None, 1.0 if clip else None, flag=flag, **kw)
        return int(flag.item())

    assert float(ops.sumsq_per_sample(g_huge)[1]) == float("inf")
    for op, degenerate in ((ops.l1_fgm, (g_zero, g_nan)), (ops.l2_fgm, (g_huge, g_nan))):
        assert run(op, xd, gd) == 0                                            # clean input: neither bit
        assert run(op, x_out, gd) == RANGE                                     # x outside the clip range: that bit alone
        assert run(op, x_out, gd, check_range=False) == 0
        assert run(op, x_out, gd, clip=False) == 0                             # no clip range: nothing to check
        for bad in degenerate:
            assert run(op, xd, bad) == DEG                                     # alone
            assert run(op, x_out, bad) == DEG | RANGE                          # both
            assert run(op, x_out, bad, check_range=False) == DEG
            assert run(op, xd, bad, clip=False) == DEG
    assert run(ops.l2_fgm, xd, g_zero) == 0              # an all-zero L2 gradient is the 1e-12 floor, not a failed self-check
    for kind, stats, bad_grads in ((1, lambda t: (ops.sumsq_per_sample(t), None), (g_huge, g_nan)),
                                   (2, ops.absmax_ties_per_sample, (g_zero, g_nan))):
        for t, want in [(gd, 0)] + [(b, DEG) for b in bad_grads]:
            flag = ops.new_flag(DEV)
            stat, stat2 = stats(t)
            ops.scale_per_sample(t, stat, stat2, EPS_BALL, kind, flag=flag)
            assert int(flag.item()) == want, (kind, want)


# ------------------------------------------------------------------------------------------------ 5. real-valued data
def test_real_valued_sums_meet_the_project_bar_against_float64():
    """Largest relative error over the samples against float64, kernel | ``torch.sum`` of the fp32 terms on the same
    device tensor (the yardstick), measured on an MI355X:
        normal (4, 3, 384, 384), vector path:      sumsq 5.0e-8 | 4.9e-8   sumsq(sub=) 7.4e-8 | 3.1e-8   sumabs 7.3e-8 | 7.3e-8
        gradient-like (9, 442371), scalar path:    sumsq 4.7e-8 | 6.3e-8   sumsq(sub=) 7.1e-8 | 4.7e-8   sumabs 8.8e-8 | 5.9e-8
    The bar stays the project's NORM_RTOL = 2e-6 (tests/test_hip_kernels.py); it is not taken from these numbers."""
    ops = _ops()
    gen = torch.Generator(DEV).manual_seed(55)
    scale = torch.logspace(-8, -2, 9, device=DEV)[:, None]
    cases = {"normal 4x3x384x384": (torch.randn(4, 3, 384, 384, device=DEV, generator=gen),
                                    torch.empty(4, 3, 384, 384, device=DEV).uniform_(-1, 1, generator=gen)),
             "gradient-like 9x442371": (torch.randn(9, 442371, device=DEV, generator=gen) * scale,
                                        torch.randn(9, 442371, device=DEV, generator=gen) * scale)}
    for name, (t, s) in cases.items():
        assert (t.data_ptr() % 16 == 0) and ((t[0].numel() % 4 != 0) == name.startswith("gradient"))   # vector | scalar
        dims = tuple(range(1, t.dim()))
        t64, s64 = t.double(), s.double()
        for what, got, terms, terms64 in (("sumsq", ops.sumsq_per_sample(t), t * t, t64 * t64),
                                          ("sumsq(sub=)", ops.sumsq_per_sample(t, sub=s), (t - s) * (t - s), (t64 - s64) ** 2),
                                          ("sumabs", ops.sumabs_per_sample(t), t.abs(), t64.abs())):
            want = terms64.sum(dims)
            err = float(((got.double() - want).abs() / want).max())
            yardstick = float(((terms.sum(dims).double() - want).abs() / want).max())
            print("{:24s} {:12s} kernel {:.3e} | torch.sum fp32 {:.3e}".format(name, what, err, yardstick))
            assert err <= NORM_RTOL, (name, what, err)
        assert _same_bits(ops.sumsq_per_sample(t), ops.sumsq_per_sample(t))
        assert _same_bits(ops.sumsq_per_sample(t, sub=s), ops.sumsq_per_sample(t, sub=s))
        assert _same_bits(ops.sumabs_per_sample(t), ops.sumabs_per_sample(t))


# ------------------------------------------------------------------------------------------------ 6. entry points
SENTINEL, FLAG_SENTINEL = -7.5, 0x5A5A
_MODE = 1 | 2                                  # VQA_CLIP | VQA_CHECK_RANGE: the flag word is then required
# symbol, arguments in ABI order: a name is a pointer of the world below ("?": optional), B / N the extents.  Arguments the
# entry point ignores (stat2 of kinds 0 and 1, the flag of kind 0) are passed as NULL, as ops.scale_per_sample does.
ENTRIES = {
    "sumsq": ("vqa_sumsq_per_sample", ("t", "?g", "out", "B", "N", "ws")),
    "sumabs": ("vqa_sumabs_per_sample", ("t", "out", "B", "N", "ws")),
    "absmax": ("vqa_absmax_ties_per_sample", ("t", "amax", "ties", "B", "N", "ws")),
    "l2_fgm": ("vqa_l2_fgm", ("t", "g", "stat", "img", "B", "N", 0.5, -1.0, 1.0, _MODE, "flag")),
    "l2_project": ("vqa_l2_project", ("t", "g", "stat", "img", "B", "N", 0.5, -1.0, 1.0, 1)),
    "l1_fgm": ("vqa_l1_fgm", ("t", "g", "stat", "stat2", "img", "B", "N", 0.5, -1.0, 1.0, _MODE, "flag")),
    "scale0": ("vqa_scale_per_sample", ("t", "stat", None, "img", "B", "N", 0.5, 0, None)),
    "scale1": ("vqa_scale_per_sample", ("t", "stat", None, "img", "B", "N", 0.5, 1, "?flag")),
    "scale2": ("vqa_scale_per_sample", ("t", "stat", "stat2", "img", "B", "N", 0.5, 2, "?flag")),
}
OUTPUTS = ("out", "amax", "ties", "ws", "img", "flag")


def _world(batch, n_per):
    """Every buffer an entry point may touch, outputs filled with a sentinel; each has four spare elements behind it."""
    def buf(numel, fill, dtype=torch.float32):
        return torch.full((numel + 4,), fill, dtype=dtype, device=DEV)[:numel]
    gen = torch.Generator(DEV).manual_seed(6)
    w = {"t": buf(batch * n_per, 0.0), "g": buf(batch * n_per, 0.0), "stat": buf(batch, 4.0), "stat2": buf(batch, 1.0),
         "out": buf(batch, SENTINEL), "amax": buf(batch, SENTINEL), "ties": buf(batch, SENTINEL),
         "ws": buf(_lib().vqa_reduce_ws_bytes(batch, n_per) // 4, SENTINEL), "img": buf(batch * n_per, SENTINEL),
         "flag": buf(1, FLAG_SENTINEL, torch.int32)}
    w["t"].uniform_(-0.5, 0.5, generator=gen)
    w["g"].normal_(generator=gen)
    return w


def _call(entry, world, batch, n_per, **override):
    """``override``: name -> pointer value (int) or None in place of that buffer's address."""
    from vqattack_amd import _hip
    symbol, spec = ENTRIES[entry]
    args = []
    for item in spec:
        if isinstance(item, str) and item in ("B", "N"):
            args.append(batch if item == "B" else n_per)
        elif isinstance(item, str):
            name = item.lstrip("?")
            args.append(override[name] if name in override else world[name].data_ptr())
        else:
            args.append(item)
    return getattr(_lib(), symbol)(*args, _hip.stream_for(world["t"]))


def _assert_untouched(world, what):
    torch.cuda.synchronize()
    for name in OUTPUTS:
        fill = FLAG_SENTINEL if name == "flag" else SENTINEL
        assert bool((world[name] == fill).all()), "{} wrote to {}".format(what, name)


@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_entry_point_refusals_and_zero_extents_write_nothing(entry):
    batch, n_per = 3, 8
    world = _world(batch, n_per)
    pointers = [item for item in ENTRIES[entry][1] if isinstance(item, str) and item not in ("B", "N")]
    for bad_batch in (65536, -1):
        assert _call(entry, world, bad_batch, n_per) == VQA_ERR_SHAPE, bad_batch
    for item in pointers:                                # two bytes off: every pointer, optional ones included
        name = item.lstrip("?")
        assert _call(entry, world, batch, n_per, **{name: world[name].data_ptr() + 2}) == VQA_ERR_ALIGN, name
    for item in pointers:
        if not item.startswith("?"):                     # required (the flag: because the mode asks for the range check)
            assert _call(entry, world, batch, n_per, **{item: None}) == VQA_ERR_NULL, item
    assert _call(entry, world, 0, n_per) == 0 and _call(entry, world, batch, 0) == 0 and _call(entry, world, 0, 0) == 0
    _assert_untouched(world, entry)
    assert _call(entry, world, batch, n_per) == 0        # and the same arguments, unmodified, are accepted
    torch.cuda.synchronize()
    written = {"sumsq": "out", "sumabs": "out", "absmax": "amax"}.get(entry, "img")
    assert not bool((world[written] == SENTINEL).any())


def test_scale_per_sample_refuses_an_unknown_kind():
    from vqattack_amd import _hip
    world = _world(3, 8)
    p = {k: v.data_ptr() for k, v in world.items()}
    for kind in (3, -1):
        assert _lib().vqa_scale_per_sample(p["t"], p["stat"], p["stat2"], p["img"], 3, 8, 0.5, kind, p["flag"],
                                           _hip.stream_for(world["t"])) == VQA_ERR_SHAPE
    _assert_untouched(world, "kind")


def test_sumabs_with_a_caller_workspace():
    ops = _ops()
    g = torch.randn(3, 12289, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    floats = _lib().vqa_reduce_ws_bytes(3, 12289) // 4
    with pytest.raises(ValueError):
        ops.sumabs_per_sample(g, ws=torch.empty(floats - 1, device=DEV))
    ws = ops.reduce_workspace(g)
    assert ws.numel() == floats
    assert _same_bits(ops.sumabs_per_sample(g, ws=ws), ops.sumabs_per_sample(g))
