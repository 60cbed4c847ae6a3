"""CPU checks that the trained-statistics inputs of ``tests/trained_stats.py`` do what they are for: the attention cases
drive the forward kernel's lazy-max rescale, mask whole key tiles and give the loop split a masked part and a part far
below the row max; the exact GEMM operands split into exactly the planes they were built from."""
import numpy as np
import pytest
import torch

from tests import trained_stats as ts
from tests.test_gemm_split import split

# the shapes the GPU tests run: packed self-attention (2, 12, 591) with key holes, cross-attention (1, 12, 25, 901),
# the loop split on (1, 12, 591)
SELF = dict(b=2, h=12, sq=591, sk=591, packed=True)
SELF_HOLES = [[6, 40], [40, 40]]
CROSS = dict(b=1, h=12, sq=25, sk=901)
SPLIT = dict(b=1, h=12, sq=591, sk=591, packed=True)


def _scores(kind, tau, shape, holes=None):
    case = ts.attn_case(kind, tau=tau, **shape)
    extra = ts.dense_hole(holes, shape["sk"]) if holes else None
    return ts.scores64(case, extra=extra)


def test_lazy_max_is_read_from_the_kernel_source():
    assert ts.lazy_max() == 8.0


@pytest.mark.parametrize("kind,tau,shape", [(k, 4.0, "self") for k in ts.RESCALE_KINDS if k != "split"] +
                         [(k, 4.0, "cross") for k in ("ramp", "sink", "lead_bert")] + [("split", 1.0, "split")])
def test_rescale_cases_rise_far_above_the_first_tile(kind, tau, shape):
    """At least half of the rows rise above the max of their first unmasked key tile by more than 2 * kLazyMax: the
    forward rescales its running max at least once in those rows, by a factor of 2^-23 or less."""
    s = _scores(kind, tau, dict(self=SELF, cross=CROSS, split=SPLIT)[shape], SELF_HOLES if shape == "self" else None)
    rise = ts.rise_over_first_tile(s)
    frac = float((rise > 2 * ts.lazy_max()).double().mean())
    assert frac >= 0.5, (kind, frac)


def test_the_suites_old_statistics_never_rescale():
    """The control: unit-variance q, k and a 0.5 * randn bias (the existing attention tests' data) stay within
    kLazyMax of the first tile in every row -- the branch above is reached only by the cases built for it."""
    s = _scores("plain", 1.0, SELF, SELF_HOLES)
    assert float(ts.rise_over_first_tile(s).max()) < ts.lazy_max()
    rev = _scores("ramp_rev", 4.0, SELF, SELF_HOLES)             # the max sits in the first tile: no rescale needed
    assert float((ts.rise_over_first_tile(rev) > ts.lazy_max()).double().mean()) < 0.05


@pytest.mark.parametrize("tau", [4.0, 8.0])
def test_hot_queries_fire_the_rescale_in_some_rows(tau):
    s = _scores("plain", tau, SELF, SELF_HOLES)
    assert float((ts.rise_over_first_tile(s) > ts.lazy_max()).double().mean()) >= 0.02


@pytest.mark.parametrize("kind", ["lead_inf", "lead_bert"])
def test_leading_key_mask_covers_whole_tiles(kind):
    case = ts.attn_case(kind, tau=4.0, **SELF)
    assert ts.LEAD % ts.TILE == 0 and ts.LEAD >= 2 * ts.TILE
    lead = case["bias"][..., :ts.LEAD]
    want = float("-inf") if kind == "lead_inf" else ts.BERT_MASK
    assert bool((lead == want).all())
    assert bool(torch.isfinite(case["bias"][..., ts.LEAD:]).all())
    assert bool((case["bias"][..., ts.LEAD:] > ts.BERT_MASK / 2).all())
    if kind == "lead_inf":
        tm = ts.tile_maxima(_scores(kind, 4.0, SELF, SELF_HOLES))
        assert bool(torch.isneginf(tm[..., :ts.LEAD // ts.TILE]).all())
        assert bool(torch.isfinite(tm[..., ts.LEAD // ts.TILE:]).all())


def test_sink_sits_in_the_last_partial_tile():
    for sk in (591, 901):
        assert sk % ts.TILE and ts.sink_key(sk) // ts.TILE == (sk - 1) // ts.TILE


@pytest.mark.parametrize("n", [3, 8])
def test_split_case_has_a_masked_part_and_a_part_far_below_the_row_max(n):
    s = _scores("split", 1.0, SPLIT)
    tm = ts.tile_maxima(s)
    bounds = ts.part_bounds(tm.shape[-1], n)
    part_max = torch.stack([tm[..., lo:hi].amax(-1) for lo, hi in zip(bounds[:-1], bounds[1:])], -1)
    row_max = tm.amax(-1, keepdim=True)
    masked = torch.isneginf(part_max).all(-2).all(-2).all(-2)         # a part masked in every row
    assert bool(masked.any()), bounds
    low = ((part_max - row_max) < -100) & torch.isfinite(part_max)
    assert bool(low.all(-2).all(-2).all(-2).any()), bounds          # a finite part > 100 below the max in every row
    assert bool(torch.isfinite(row_max).all())                      # no query row is fully masked


@pytest.mark.parametrize("kind", ts.LN_KINDS)
def test_layernorm_rows_have_the_intended_statistics(kind):
    x = ts.ln_rows(kind, 48, 768).double()
    mean, std = x.mean(-1), x.std(-1)
    if kind.startswith("offset"):
        off = 1e2 if kind == "offset1e2" else 1e3
        assert bool(((mean.abs() / std) > 0.9 * off).all())
    elif kind == "outliers":
        assert float(x.abs().amax(0).topk(2).values.min()) > 300.0
    elif kind == "constant":
        assert bool((x == x[:, :1]).all())
    else:
        assert bool((std / mean.abs() < 1e-4).all()) and bool((x != x[:, :1]).any(-1)[:2].all())      # 0.1 and -2.5 keep a spread


@pytest.mark.parametrize("pa,pb", ts.PRODUCTS)
def test_exact_gemm_operands_split_into_their_planes_and_sum_exactly(pa, pb):
    """The construction of the bit-exact GEMM test: the numpy restatement of the kernel's split returns exactly the
    planes the operands were built from (so only products (<= pa, <= pb) are nonzero, and none the kernel drops), and
    the fp64 product is exact in fp32 with every partial sum a multiple of 2^-20 below 2^3."""
    m, n, k = 300, 384, 256
    a, b, a_planes, b_planes = ts.exact_operands(pa, pb, m, n, k)
    for x, planes, top in ((a, a_planes, pa), (b, b_planes, pb)):
        got = split(x)
        for i in range(3):
            assert np.array_equal(got[i].astype(np.float64), planes[i]), i
            assert bool((planes[i] != 0).any()) == (i <= top)
    assert bool(((a != 0).sum(1) == ts.EXACT_NNZ).all())
    ref = a.astype(np.float64) @ b.astype(np.float64)
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    bound = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64)
    assert float(bound.max()) < 8.0
    q = 2.0 ** -20
    for i in range(3):
        for j in range(3):
            part = a_planes[i] @ b_planes[j]
            assert np.array_equal(np.round(part / q) * q, part)
    # a dropped product (a1b2, a2b1, a2b2) never contributes
    for i, j in ((1, 2), (2, 1), (2, 2)):
        assert not (a_planes[i] @ b_planes[j]).any()
