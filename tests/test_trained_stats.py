"""CPU checks that the trained-statistics inputs of ``tests/trained_stats.py`` do what they are for: the attention cases
drive the forward kernel's lazy-max rescale, mask whole key tiles and give the loop split a masked part and a part far
below the row max; the exact GEMM operands split into exactly the planes they were built from."""
import math

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


# ------------------------------------------------------------------------- loss / text-scoring inputs (fp64 only)
@pytest.mark.parametrize("kind", ts.PAIR_KINDS)
@pytest.mark.parametrize("delta", ts.DELTAS)
def test_feature_pairs_are_as_far_apart_as_they_claim(kind, delta):
    a, b = ts.feature_pair(kind, delta, 3, 40, 768)
    if delta == 0.0:
        assert torch.equal(a, b)
        return
    rel = (a.double() - b.double()).norm(dim=-1) / b.double().norm(dim=-1)
    assert float(rel.min()) >= delta / 2 and float(rel.max()) <= delta * 2, (float(rel.min()), float(rel.max()))
    if delta <= 1e-3:
        val, _ = ts.neg_cos64(a.double(), b.double())
        assert float((-val).min()) > 1.0 - 1e-5
    if kind != "plain":
        assert float(b[..., 7].abs().median() / b[..., 8].abs().median()) > 100.0
    if kind == "scaled":
        norms = b.double().norm(dim=-1) / (300.0 * 2 ** 0.5)
        assert float(norms.min()) < 1e-2 and float(norms.max()) > 1e2


def test_degenerate_rows_lie_on_the_intended_side_of_cos_eps():
    a, b = ts.feature_pair("degenerate", 1e-3, 3, 40, 768)
    na, nb = a.double().view(-1, 768).norm(dim=-1), b.double().view(-1, 768).norm(dim=-1)
    rows = ts.DEGENERATE_ROWS
    for r in rows["a_zero"] + rows["both_zero"]:
        assert float(na[r]) == 0.0
    for r in rows["b_zero"] + rows["both_zero"]:
        assert float(nb[r]) == 0.0
    for r in rows["a_tiny"]:
        assert 0.0 < float(na[r]) < 0.2 * ts.COS_EPS and float(nb[r]) > 1.0
    for r in rows["b_tiny"]:
        assert 0.0 < float(nb[r]) < 0.2 * ts.COS_EPS and float(na[r]) > 1.0
    for r in rows["a_above"]:
        assert ts.COS_EPS * 2 < float(na[r]) < ts.COS_EPS * 4
    for r in rows["b_above"]:
        assert ts.COS_EPS * 2 < float(nb[r]) < ts.COS_EPS * 4
    val, grad = ts.neg_cos64(a.double(), b.double())
    assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(grad).all())
    # the closed form is what autograd gives for torch's own float64 cosine on every row -- except 0 < |a| <= eps, where
    # torch clamps the norm outside autograd and lets a gradient through it (off by |a| / eps = 10 % here); the kernel
    # follows the header: nothing flows through a clamped norm
    x = a.double().clone().requires_grad_(True)
    c = torch.nn.CosineSimilarity(dim=-1, eps=ts.COS_EPS)(x, b.double())
    (gx,) = torch.autograd.grad((-c).sum(), x)
    scale = grad.abs().amax(-1).clamp_min(1e-300)
    rel = ((gx - grad).abs().amax(-1) / scale).view(-1)
    clamped = torch.zeros_like(rel, dtype=torch.bool)
    clamped[list(rows["a_tiny"])] = True
    assert float(rel[~clamped].max()) < 1e-9
    assert 0.05 < float(rel[clamped].min()) and float(rel[clamped].max()) < 0.2
    assert float((-c.detach() - val).abs().max()) < 1e-12


@pytest.mark.parametrize("kind", list(ts.MLM_KINDS))
@pytest.mark.parametrize("v,k", [(30522, 1), (30522, 3), (33334, 8)])
def test_mlm_rows_are_peaked_and_their_labels_sit_on_the_edge_lanes(kind, v, k):
    rows = 48
    x, labels, margin = ts.mlm_logits(kind, rows, v, k)
    live = ts.live_rows(rows)
    assert len(live) * 3 <= rows + 2 and bool((labels[:, [r for r in range(rows) if r not in live]] == ts.IGNORE).all())
    assert sorted(set(margin[live].tolist())) == list(range(len(ts.MARGINS)))
    row64, _ = ts.ce_rows_torch(x.double(), labels, 0)
    w0 = 1.0 / len(live)
    for r in live:
        t = int(labels[0, r])
        assert float(x[r, t]) == float(x[r].max()) and math.isfinite(float(x[r, t]))
        only0 = bool((labels[1:, r] == ts.IGNORE).all()) if k > 1 else True
        if ts.MARGINS[int(margin[r])] >= 15.0 and only0:
            assert 0.0 < float(row64[r]) / w0 < 1e-4, (r, float(row64[r]))
    if k > 1:
        r = live[1]
        assert int(labels[1, r]) == int(labels[0, r])
        assert any(int(labels[kk, q]) not in (ts.IGNORE, int(labels[0, q])) for kk in range(1, k) for q in live)
    # head / tail lanes of the register kernel (row_geom): at V = 30522 odd rows have a two-element head, even rows a
    # two-element tail; the forced positions land on them
    on_head = on_tail = body = 0
    for r in live:
        head, nquad, tail0 = ts.row_geom(r, v)
        assert head == (2 if r % 2 else 0) and v - tail0 == (0 if r % 2 else 2)
        t = int(labels[0, r])
        on_head += t < head
        on_tail += t >= tail0
        body += head <= t < tail0
    assert on_head >= 4 and on_tail >= 4 and body >= 4
    if kind == "masked":
        for r in live:
            # every lane's first element of the streaming fallback (256 lanes, pairs or single floats) is -inf, except
            # where a label sits; a third of the row is masked overall; no label is masked
            first = x[r, :2 * ts.CE_BLOCK]
            assert int(torch.isinf(first).sum()) >= 2 * ts.CE_BLOCK - 1
            assert bool(torch.isinf(x[r, :ts.MASKED_HEAD]).sum() >= ts.MASKED_HEAD - k)
            assert 0.25 < float(torch.isinf(x[r]).float().mean()) < 0.40
            for kk in range(k):
                if int(labels[kk, r]) != ts.IGNORE:
                    assert math.isfinite(float(x[r, int(labels[kk, r])]))
        assert bool(torch.isfinite(row64[live]).all())


@pytest.mark.parametrize("d", [768, 1024])
def test_text_tables_near_synonyms_and_the_pair_cap(d):
    """Near-synonym candidates move the embedding by < 10 % of its length, and at a gap of 1e-5 fewer than 2 % of the
    candidate pairs of a (sample, position) are too close to rank (float64 scores alone)."""
    tabs = ts.text_tables(d)
    ori, cand, syn = ts.text_candidates(tabs)
    assert cand.shape[0] == ts.TEXT_SAMPLES * ts.TEXT_POSITIONS * ts.TEXT_CANDS
    pos = torch.arange(ts.TEXT_LEN)[None].expand_as(ori)
    e_ori = ts.bert_embed(tabs, ori, pos, torch.float32)
    s64, rel = ts.dir_sim(tabs, e_ori, cand, torch.float64)
    assert int(syn.sum()) == ts.TEXT_SAMPLES * ts.TEXT_POSITIONS
    assert float(rel[syn].max()) < 0.1 and float(rel[~syn].min()) > 0.5
    assert float(tabs["gamma"].abs().max()) == 8.0
    gabs = tabs["grad"].abs()
    assert 1e-8 < float(gabs.median()) < 1e-6 and float(gabs.max()) > 50.0 * float(gabs.median())
    left, _ = ts.left_out_pairs(s64, 1e-5, ts.TEXT_CANDS)
    assert left <= 0.02, left


@pytest.mark.parametrize("e", [64, 512])
def test_greedy_cases_are_decidable_and_hold_a_close_call(e):
    case = ts.greedy_case(e)
    assert case["ori"].shape == (ts.GREEDY_B, ts.GREEDY_L)
    for thr in ts.GREEDY_THRESHOLDS:
        new_id, rank, smallest, risen = ts.greedy_accept64(case, thr)
        left = float((smallest <= ts.GREEDY_MARGIN).mean())
        assert left <= 0.05, (thr, left)
        # sample 0: accepted once, then a later candidate misses the risen threshold by 1e-5 .. 1e-3
        assert int((new_id[0] >= 0).sum()) >= 1
        assert risen[0] and ts.GREEDY_MARGIN < min(risen[0]) < 1e-3, risen[0]
        assert smallest[0] > ts.GREEDY_MARGIN
    # the exact-tie candidates are reached after an acceptance at the lower thresholds
    new_id, _, _, _ = ts.greedy_accept64(case, 0.5)
    assert sum(int((new_id[s] >= 0).sum()) >= 1 for s in range(1, 9)) >= 4
    assert float(np.mean([(new_id[s] >= 0).sum() for s in range(ts.GREEDY_B)])) >= 1.0


def test_image_gradients_are_small_and_heavy_tailed():
    g = ts.image_grads((4, 3, 96, 96))
    nz = g[g != 0].abs()
    assert 0.005 < float((g == 0).float().mean()) < 0.02
    assert 1e-7 < float(nz.median()) < 1e-6 and float(nz.max()) > 1e-5 and float(nz.min()) < 1e-8
    assert float(g.double().flatten(1).norm(dim=1).min()) > 1e-6
