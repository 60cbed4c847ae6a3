"""The loss kernels between two model calls -- ``vqa_neg_cos_rows`` / ``_multi`` (csrc/loss.hip), ``vqa_ce_rows``
(csrc/ce.hip), ``vqa_sumsq_per_sample`` and the L2 update -- against float64 in the regime an attack puts them in
(``tests/trained_stats.py``; ``test_trained_stats.py`` checks the inputs on the CPU).  The yardstick is torch fp32 on the
device on the same fp32 inputs; every case prints one ``FP64 ...: kernel/torch`` line.

Cosine loss: ``a = b + delta * noise`` (adversarial against clean features of one model), outlier channels, per-row scales,
rows at and below ``cos_eps``.  The gradient ``kb b + ka a`` is a difference of nearly equal vectors, so it is judged per
row in units of what one fp32 rounding of the operands moves it by:  e_row = |g - g64|_2 max(|a|_2, cos_eps) / 2^-24.

Cross entropy: rows whose label is predicted with p ~ 1 (loss 1e-2 .. 1e-7), a common offset of +-50 on the logits, labels
on the register kernel's head / tail lanes, shared labels, ``-inf`` (vocabulary-masked) logits, on the register-resident
kernel and on the streaming fallback.  Row losses are judged RELATIVELY per (margin, offset) cell.
"""
import ctypes

import pytest
import torch

from tests import trained_stats as ts

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
NORM_RTOL = 2e-6                     # the project's stated bar on per-sample norms (tests/test_hip_kernels.py)

# Absolute ceiling on max_row e(kernel), independent of torch: twice the largest max_row e that torch fp32 reached on the
# device over all cosine cases of this file (17.3, the full-size outlier maps), rounded up to a power of two.  Measured on
# an MI355X, max over D, shape, weights and delta, kernel / torch:
#   plain       11.7 / 9.26
#   outliers    21.4 / 17.3
#   scaled      18.6 / 16.8
#   degenerate  11.7 / 12.1    (yardstick: the header's formula in fp32)
COS_CEILING = 64.0


def _ops():
    from vqattack_amd import ops
    return ops


def _e_rows(g, g64, a64):
    return (g.double() - g64).norm(dim=-1) * a64.norm(dim=-1).clamp_min(ts.COS_EPS) / U


def _torch32_cos(a, b, w):
    x = a.clone().requires_grad_(True)
    val = -torch.nn.CosineSimilarity(dim=-1, eps=ts.COS_EPS)(x, b)
    if w is not None:
        val = val * w
    loss = val.sum()
    (grad,) = torch.autograd.grad(loss, x)
    return loss.detach(), grad


def _row_weights(rows0, rows1):
    """uint8 (rows0, rows1) weights in {0, 1, 2}; at least one of each."""
    r = torch.arange(rows0 * rows1).view(rows0, rows1)
    w = torch.ones(rows0, rows1, dtype=torch.uint8)
    w[r % 5 == 0] = 2
    w[r % 7 == 3] = 0
    return w


def _judge_cos(tag, got_grad, got_loss, a, b, w, formula_yardstick=False):
    """The rules of this file for one launch.  ``a`` may hold NaN in weight-0 rows.  Returns (max e kernel, max e torch)."""
    wf = None if w is None else w.to(a.dtype).expand(a.shape[:-1])
    dead = torch.zeros(a.shape[:-1], dtype=torch.bool, device=a.device) if wf is None else wf == 0
    assert bool(torch.isfinite(got_grad).all()) and bool(torch.isfinite(got_loss).all()), tag
    assert float(got_grad[dead].abs().max() if bool(dead.any()) else 0.0) == 0.0, tag   # weight-0 rows exactly zero
    clean = torch.where(dead.unsqueeze(-1), b, a)              # the references never see the NaN of a weight-0 row
    a64, b64 = clean.double(), b.double()
    val64, g64 = ts.neg_cos64(a64, b64, None if wf is None else wf.double())
    if formula_yardstick:                                       # rows at / below cos_eps: torch's autograd lets a
        val32, g32 = ts.neg_cos64(clean, b, wf)                 # gradient through the clamped norm, the header does not
        loss32 = val32.sum()
    else:
        loss32, g32 = _torch32_cos(clean, b, wf)
    live = ~dead
    ek, et = _e_rows(got_grad, g64, a64)[live], _e_rows(g32, g64, a64)[live]
    loss64 = float(val64.sum())
    lk, lt = abs(float(got_loss) - loss64), abs(float(loss32) - loss64)
    wsum = float(live.sum()) if wf is None else float(wf.sum())
    print("FP64 neg_cos {}: kernel/torch e_row max {:.3g}/{:.3g} median {:.3g}/{:.3g} loss err {:.3g}/{:.3g}".format(
        tag, float(ek.max()), float(et.max()), float(ek.median()), float(et.median()), lk, lt))
    assert float(ek.max()) <= 2.0 * float(et.max()) + 4.0, (tag, float(ek.max()), float(et.max()))
    assert float(ek.median()) <= 2.0 * float(et.median()) + 1.0, (tag, float(ek.median()), float(et.median()))
    assert float(ek.max()) <= COS_CEILING, (tag, float(ek.max()))
    assert lk <= 2.0 * lt + 4.0 * U * wsum, (tag, lk, lt, wsum)
    return float(ek.max()), float(et.max())


# ------------------------------------------------------------------------------------------------------ cosine loss
@pytest.mark.parametrize("shape", [(13, 617), (3, 40)], ids=str)
@pytest.mark.parametrize("d", [768, 1024, 260])
@pytest.mark.parametrize("kind", ts.PAIR_KINDS + ("degenerate",))
def test_neg_cos_rows_against_fp64(kind, d, shape):
    """Every delta, with and without row weights {0, 1, 2} (a weight-0 row holds NaN).  D = 768 / 1024 run on the
    whole-chunk kernel (on the general one where a weighted map has <= 128 rows per sample), D = 260 on the general one.
    delta = 0: the float64 gradient is 0 up to 1e-16, so e_row is the noise the kernel emits when the adversarial and the
    clean features coincide (text-only steps, FGM from the clean image).  ``degenerate``: rows of a and of b that are
    exactly zero, of norm 1e-7 (below cos_eps) and 3e-6 (just above), against the header's formula."""
    ops = _ops()
    rows0, rows1 = shape
    worst = [0.0, 0.0]
    for delta in ts.DELTAS:
        a_cpu, b_cpu = ts.feature_pair(kind, delta, rows0, rows1, d)
        for weighted in (False, True):
            a, b = a_cpu.to(DEV), b_cpu.to(DEV)
            w = None
            if weighted:
                w = _row_weights(rows0, rows1).to(DEV)
                if kind == "degenerate":
                    w.view(-1)[:13] = 1                         # the degenerate rows stay live
                nan_row = int(torch.nonzero(w.view(-1) == 0)[0])
                a.view(-1, d)[nan_row] = float("nan")
            slot = torch.full((1,), 7.0, device=DEV)
            g = ops.neg_cos_rows(a, b, slot, accumulate=False, row_weight=w, weight_period=rows0)
            ek, et = _judge_cos("{} delta={:g} D={} rows={}x{} w={}".format(kind, delta, d, rows0, rows1, int(weighted)),
                                g, slot[0], a, b, w, formula_yardstick=(kind == "degenerate"))
            worst = [max(worst[0], ek), max(worst[1], et)]
    print("FP64 neg_cos {} D={} rows={}x{}: kernel/torch e_row max over deltas and weights {:.3g}/{:.3g}".format(
        kind, d, rows0, rows1, *worst))


def test_neg_cos_rows_multi_and_strided_views_against_fp64():
    """13 maps in one launch (``neg_cos_rows_multi``), 13 of the 15 (kind, delta) combinations among them (delta = 1 only
    on plain rows), and ``[:, :feat_len, :]`` views."""
    ops = _ops()
    d, rows0, rows1, store = 768, 3, 160, 200
    cases = [(k, dl) for dl in ts.DELTAS for k in ts.PAIR_KINDS][:13]
    pairs = [ts.feature_pair(k, dl, rows0, store, d, seed=3 + i) for i, (k, dl) in enumerate(cases)]
    a_list = [p[0].to(DEV)[:, :rows1] for p in pairs]            # the reference's truncation views, never packed
    b_list = [p[1].to(DEV)[:, :rows1] for p in pairs]
    slot = torch.zeros(1, device=DEV)
    grads = ops.neg_cos_rows_multi(a_list, b_list, slot, accumulate=False)
    loss64 = loss32 = 0.0
    for (k, dl), a, b, g in zip(cases, a_list, b_list, grads):
        one = torch.zeros(1, device=DEV)
        g1 = ops.neg_cos_rows(a, b, one, accumulate=False)
        assert torch.equal(g, g1)                               # the multi launch is the per-map launch, bit for bit
        _judge_cos("multi/strided {} delta={:g}".format(k, dl), g, one[0], a.contiguous(), b.contiguous(), None)
        loss64 += float(ts.neg_cos64(a.double(), b.double())[0].sum())
        loss32 = loss32 + _torch32_cos(a.contiguous(), b.contiguous(), None)[0]
    lk, lt = abs(float(slot) - loss64), abs(float(loss32) - loss64)
    print("FP64 neg_cos multi 13 maps: kernel/torch loss err {:.3g}/{:.3g}".format(lk, lt))
    assert lk <= 2.0 * lt + 4.0 * U * 13 * rows0 * rows1


def test_neg_cos_rows_multi_full_size_loss_against_fp64():
    """13 maps of 64 x 617 x 768 (the attack's launch; loss ~ -5e5): the in-kernel fold of 513 k row values loses no
    more than the summation order explains, 4 * 2^-24 * rows on top of twice torch's own error.  Once, not per case."""
    ops = _ops()
    rows0, rows1, d = 64, 617, 768
    base = [ts.feature_pair("outliers", dl, rows0, rows1, d, seed=9) for dl in (1e-3, 1e-1)]
    base = [(a.to(DEV), b.to(DEV)) for a, b in base]
    a_list = [base[i % 2][0].roll(i, 0) for i in range(13)]
    b_list = [base[i % 2][1].roll(i, 0) for i in range(13)]
    w = torch.ones(1, rows1, dtype=torch.uint8)
    w[0, 0], w[0, -30:] = 2, 0                                  # VLMo: [CLS] twice, 30 padded tokens
    w = w.to(DEV)
    slot = torch.zeros(1, device=DEV)
    grads = ops.neg_cos_rows_multi(a_list, b_list, slot, accumulate=False, row_weight=w, weight_period=1)
    wf = w.float().expand(rows0, rows1)
    loss64, loss32 = 0.0, torch.zeros((), device=DEV)
    for i, (a, b) in enumerate(zip(a_list, b_list)):
        loss64 += float(ts.neg_cos64(a.double(), b.double(), wf.double())[0].sum())
        loss32 = loss32 + _torch32_cos(a, b, wf)[0]
    lk, lt = abs(float(slot) - loss64), abs(float(loss32) - loss64)
    print("FP64 neg_cos full size 13x64x617x768: loss64 {:.6f} kernel/torch loss err {:.3g}/{:.3g}".format(loss64, lk, lt))
    assert loss64 < -4e5
    assert lk <= 2.0 * lt + 4.0 * U * 13 * float(wf.sum())
    # the gradient of the first and the last map under the same rule as the small cases
    for i in (0, 12):
        a64 = a_list[i].double()
        _, g64 = ts.neg_cos64(a64, b_list[i].double(), wf.double())
        _, g32 = _torch32_cos(a_list[i], b_list[i], wf)
        live = wf != 0
        ek, et = _e_rows(grads[i], g64, a64)[live], _e_rows(g32, g64, a64)[live]
        print("FP64 neg_cos full size map {}: kernel/torch e_row max {:.3g}/{:.3g}".format(i, float(ek.max()), float(et.max())))
        assert float(ek.max()) <= 2.0 * float(et.max()) + 4.0 and float(ek.max()) <= COS_CEILING
        assert float(grads[i][~live].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- cross entropy
# Ceiling on the kernel's own relative row-loss error, independent of torch, for every cell whose loss is >= 1e-8.  With
# the element at the max counted apart, the loss of a peaked row is log1p(s), s = sum of exp(x - m) over the others, and
# inherits the relative error of those terms: x - m rounded at magnitude < 32 (0.5 ulp = 0.95e-6 absolute = relative in
# exp), its product with log2(e) inside the hardware exponential rounded at magnitude < 64 (1.9e-6 * ln 2 = 1.3e-6),
# v_exp_f32 itself (2 ulp = 0.24e-6): 2.5e-6 per term at worst, plus three roundings of 6e-8 for the sum, the division
# and log1p.  Rounded up to a power of two.  (A sum that carries the 1 of the max element misses it by 1e2 .. 1e5.)
CE_REL_CEILING = 2.0 ** -18
CE_REL_FLOOR_LOSS = 1e-8

CE_PATHS = {"register": (30522, 0), "fallback": (33334, 0), "row_stride": (30522, 6), "odd_v": (33335, 0)}


def _ce_kernel(logits, labels, rows_per_sample, pad=0, via_ops=False):
    """(row_loss, grad, loss_out) of one ``vqa_ce_rows`` launch through the C ABI; ``pad`` > 0: rows ``pad`` floats apart
    (NaN between them).  The gradient buffer starts as NaN: an element the launch does not write shows."""
    from vqattack_amd import _hip
    lib = _hip.lib()
    rows, v = logits.shape
    k = labels.shape[0]
    flat = logits
    if pad:
        store = torch.full((rows, v + pad), float("nan"), device=DEV)
        store[:, :v] = logits
        flat = store[:, :v]
    groups = 1 if rows_per_sample == 0 else -(-rows // rows_per_sample)
    scratch = torch.empty(max(int(lib.vqa_ce_scratch_floats(k, groups)), 1), device=DEV)
    grad = torch.full((rows, v), float("nan"), device=DEV)
    row_loss = torch.full((rows,), float("nan"), device=DEV)
    loss_out = torch.full((1,), 7.0, device=DEV)
    labels = labels.contiguous()
    _hip.check(lib.vqa_ce_rows(_hip.ptr(flat), flat.stride(0), ctypes.c_void_p(labels.data_ptr()), k, rows, v, ts.IGNORE,
                               rows_per_sample, _hip.ptr(scratch), _hip.ptr(grad), _hip.ptr(row_loss), 1.0,
                               _hip.ptr(loss_out), 0, None, None, _hip.stream_for(logits)), "vqa_ce_rows")
    if via_ops:                                                 # the wrapper is the same launch
        slot = torch.zeros(1, device=DEV)
        g2 = _ops().mlm_cross_entropy(logits, labels, slot, accumulate=False, rows_per_sample=rows_per_sample)
        assert torch.equal(g2, grad) and torch.equal(slot, loss_out)
    return row_loss, grad, loss_out[0]


def _judge_ce(tag, kind, x, labels, margin, rows_per_sample, pad=0, via_ops=False):
    """The rules for one launch; returns {(margin, kind): (rel kernel, rel torch, smallest l64)} of the judged cells and
    of the cells torch does not resolve (l64 < 1e-6)."""
    x, labels = x.to(DEV), labels.to(DEV)
    row_k, grad_k, loss_k = _ce_kernel(x, labels, rows_per_sample, pad, via_ops)
    row64, grad64 = ts.ce_rows_torch(x.double(), labels, rows_per_sample)
    row32, grad32 = ts.ce_rows_torch(x, labels, rows_per_sample)
    wsum = ts.ce_weights(labels, rows_per_sample, torch.float64).sum(0)
    live = wsum > 0
    assert bool(torch.isfinite(row_k).all()) and bool(torch.isfinite(grad_k).all()), tag
    assert float(row_k[~live].abs().max()) == 0.0 and float(grad_k[~live].abs().max()) == 0.0, tag
    if kind == "masked":
        assert float(grad_k[torch.isinf(x)].abs().max()) == 0.0, tag
    # per-row loss, relative, per (margin, offset) cell; rows that carry only label set 0 (the peaked ones)
    pure = live & (labels[1:] == ts.IGNORE).all(0) if labels.shape[0] > 1 else live
    cells, fails = {}, []
    for mi, mg in enumerate(ts.MARGINS):
        sel = pure & (margin.to(DEV) == mi)
        if not bool(sel.any()):
            continue
        l64 = row64[sel] / wsum[sel]                            # the row's own cross entropy
        rk = float(((row_k[sel].double() - row64[sel]).abs() / row64[sel]).max())
        rt = float(((row32[sel].double() - row64[sel]).abs() / row64[sel]).max())
        cells[(mg, kind)] = (rk, rt, float(l64.min()))
        if float(l64.min()) >= 1e-6 and not rk <= 2.0 * rt + 1e-6:
            fails.append((mg, rk, rt))
        if float(l64.min()) >= CE_REL_FLOOR_LOSS and not rk <= CE_REL_CEILING:
            fails.append((mg, rk, "ceiling"))
    # rows with several labels (one of them shares a label between two sets): the same relative rule on the row
    mixed = live & ~pure & (row64 / wsum.clamp_min(1e-300) >= 1e-6)
    if bool(mixed.any()):
        rk = float(((row_k[mixed].double() - row64[mixed]).abs() / row64[mixed]).max())
        rt = float(((row32[mixed].double() - row64[mixed]).abs() / row64[mixed]).max())
        cells[("mixed", kind)] = (rk, rt, float((row64[mixed] / wsum[mixed]).min()))
        if not rk <= 2.0 * rt + 1e-6:
            fails.append(("mixed", rk, rt))
    # gradient: per row, max |g - g64| <= 2 max |g32 - g64| + 4 * 2^-24 * wsum
    gk = (grad_k.double() - grad64).abs().amax(1)
    gt = (grad32.double() - grad64).abs().amax(1)
    bad = gk > 2.0 * gt + 4.0 * U * wsum
    # the scalar
    s64 = float(row64.sum())
    sk, st = abs(float(loss_k) - s64), abs(float(row32.sum()) - s64)
    print("FP64 ce {}: kernel/torch row loss rel {} | grad max err/wsum {:.3g}/{:.3g} | scalar err {:.3g}/{:.3g}".format(
        tag, " ".join("m{}={:.2g}/{:.2g}{}".format(c[0], v[0], v[1], "" if v[2] >= 1e-6 else "(l64<1e-6)")
                      for c, v in cells.items()),
        float((gk[live] / wsum[live]).max()), float((gt[live] / wsum[live]).max()), sk, st))
    assert not fails, (tag, fails)
    assert not bool(bad.any()), (tag, int(bad.sum()), float((gk / (2.0 * gt + 4.0 * U * wsum).clamp_min(1e-300)).max()))
    assert sk <= 2.0 * st + 4.0 * U * s64, (tag, sk, st, s64)
    return cells


@pytest.mark.parametrize("rows", [12, 192])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("path", list(CE_PATHS))
def test_ce_rows_against_fp64(path, k, rows):
    """Every kind (offset 0 / +50 / -50, masked) with rows_per_sample 0 and L on one path and one MAXK instantiation.
    Cells torch fp32 itself does not resolve (row loss below 1e-6: margins 20 and 30, where its error is 100 %) are
    printed and not judged.  Measured on an MI355X, row-loss relative error kernel / torch, K = 1, 192 rows, offset 0:
      before (lse = m + log(sum exp), one running sum that carries the 1 of the max element), register path:
          offset   0: margin 5: 1.9e-6 / 1.3e-6   10: 5.2e-4 / 9.8e-5   15: 0.20  / 0.030
          offset +50: margin 5: 2.8e-5 / 1.3e-6   10: 4.5e-3 / 1.1e-4   15: 0.31  / 0.010
          offset -50: margin 5: 4.9e-6 / 7.0e-7   10: 1.2e-3 / 2.0e-4   15: 0.085 / 0.0097
          (fallback: 0.14 / 0.034, 0.16 / 0.011, 0.17 / 0.011 at margin 15); margin 20 and 30: 1 / 1; the label's
          gradient entry off by up to 1.5e-6 * wsum; ``masked`` rows NaN on the streaming fallback.
      after (max elements counted apart from the sum of the rest, loss = log c + log1p(s / c) - (x[t] - m)):
          margin 5: 1.8e-7   10: 2.7e-7   15: 3.2e-7   20: 4.3e-7   30: 8.7e-5, at every offset and on both paths;
          gradient within 1.1e-7 * wsum; ``masked`` rows finite and inside the same rules.
    Every cell with a loss >= 1e-8 (margin 20 included, which torch does not resolve) is also held to CE_REL_CEILING on
    the kernel alone."""
    v, pad = CE_PATHS[path]
    for kind in ts.MLM_KINDS:
        for rps in (0, 4 if rows == 12 else 24):
            x, labels, margin = ts.mlm_logits(kind, rows, v, k, seed=k + (rps > 0))
            _judge_ce("{} {} K={} rows={} rps={}".format(path, kind, k, rows, rps), kind, x, labels, margin, rps, pad,
                      via_ops=(pad == 0))


def test_ce_rows_full_size_against_fp64():
    """2560 x 30522 logits (64 questions of 40 tokens), K = 3, per-sample normalisation: once, on the register path."""
    cells = {}
    for kind in ("off0", "off+50"):
        x, labels, margin = ts.mlm_logits(kind, 2560, 30522, 3, seed=1)
        cells.update(_judge_ce("register full size {} K=3 rows=2560 rps=40".format(kind), kind, x, labels, margin, 40))
    assert all((mg, "off+50") in cells for mg in ts.MARGINS)


@pytest.mark.parametrize("path", list(CE_PATHS))
def test_ce_row_of_only_minus_inf_is_nan_like_torch(path):
    """A row that is ENTIRELY -inf has no softmax: NaN in torch, NaN here; its neighbours are untouched."""
    v, pad = CE_PATHS[path]
    x, labels, _ = ts.mlm_logits("masked", 12, v, 1)
    x[4] = float("-inf")
    assert int(labels[0, 4]) != ts.IGNORE
    x, labels = x.to(DEV), labels.to(DEV)
    row_k, grad_k, loss_k = _ce_kernel(x, labels, 0, pad)
    row32, grad32 = ts.ce_rows_torch(x, labels, 0)
    assert bool(torch.isnan(row32[4])) and bool(torch.isnan(row_k[4])) and bool(torch.isnan(loss_k))
    assert bool(torch.isnan(grad_k[4]).all())
    others = [r for r in range(12) if r != 4]
    assert bool(torch.isfinite(row_k[others]).all()) and bool(torch.isfinite(grad_k[others]).all())


@pytest.mark.parametrize("kind", ["off0", "masked"])
@pytest.mark.parametrize("path", list(CE_PATHS))
def test_ce_nan_logit_poisons_its_row_like_torch(path, kind):
    """A NaN logit is never dropped: the row's loss, the scalar and the row's gradient are NaN, as in torch, on every
    path.  ``off0``: the NaN is a lane's FIRST element of the streaming fallback (position < 256) on an odd and on an even
    row.  ``masked``: it sits inside the all -inf head of the row -- beside a -inf, beside another NaN -- where the
    running max is still -inf and fmaxf would drop it."""
    v, pad = CE_PATHS[path]
    x, labels, _ = ts.mlm_logits(kind, 12, v, 1)
    nan = float("nan")
    if kind == "off0":
        x[1, 5], x[4, 200] = nan, nan
        poisoned = [1, 4]
    else:
        x[1, 300] = nan                                         # NaN / -inf pair
        x[4, 600], x[4, 601] = nan, nan                         # NaN / NaN pair
        x[7, 701] = nan                                         # -inf / NaN pair
        assert bool(torch.isinf(x[[1, 4, 7]][:, [301, 602, 700]]).all())
        poisoned = [1, 4, 7]
    assert all(int(labels[0, r]) not in (5, 200, 300, 600, 601, 701) for r in poisoned)
    x, labels = x.to(DEV), labels.to(DEV)
    row_k, grad_k, loss_k = _ce_kernel(x, labels, 0, pad)
    row32, grad32 = ts.ce_rows_torch(x, labels, 0)
    assert bool(torch.isnan(row32[poisoned]).all()) and bool(torch.isnan(grad32[poisoned]).all())
    assert bool(torch.isnan(row_k[poisoned]).all()), row_k[poisoned]
    assert bool(torch.isnan(loss_k))
    assert bool(torch.isnan(grad_k[poisoned]).all())
    others = [r for r in range(12) if r not in poisoned]
    assert bool(torch.isfinite(row_k[others]).all()) and bool(torch.isfinite(grad_k[others]).all())
    assert float(row_k[10]) > 0.0


# ------------------------------------------------------------------------------------------- norms and the L2 update
@pytest.mark.parametrize("shape", [(4, 3, 384, 384), (64, 3, 384, 384)], ids=str)
def test_l2_norms_and_update_on_image_gradients_against_fp64(shape):
    """Image gradients of the feature loss are 1e-5 .. 1e-8 and heavy-tailed: the squares are 1e-10 .. 1e-16 and their sum
    must neither lose the small ones nor land on the updates' ``max(1e-12, .)`` floor."""
    ops = _ops()
    g_cpu = ts.image_grads(shape)
    g_cpu[1] = (g_cpu[1].double() * (3e-6 / g_cpu[1].double().norm())).float()   # one sample just above the floor
    g = g_cpu.to(DEV)
    ss = ops.sumsq_per_sample(g).double()
    ss64 = (g.double() ** 2).flatten(1).sum(1)
    ss32 = (g ** 2).flatten(1).sum(1).double()
    rel_k, rel_t = float(((ss - ss64).abs() / ss64).max()), float(((ss32 - ss64).abs() / ss64).max())
    print("FP64 sumsq {}: kernel/torch max rel err {:.3g}/{:.3g}; smallest norm {:.3g}".format(
        shape, rel_k, rel_t, float(ss64.sqrt().min())))
    assert torch.allclose(ss, ss64, rtol=NORM_RTOL, atol=0)
    floored = (ss64.sqrt() > 1e-6) & (ss <= 1e-12)
    assert not bool(floored.any()), floored.nonzero().flatten().tolist()
    assert 2e-6 < float(ss64[1].sqrt()) < 4e-6                  # the sample that makes the line above bite
    # FGM update: x + eps_iter g / |g|, no clipping (the step is exactly the normalised gradient)
    gen = torch.Generator().manual_seed(3)
    x_cpu = torch.empty(shape).uniform_(-1, 1, generator=gen)
    x = x_cpu.to(DEV)
    eps_iter = 0.5
    out = ops.l2_fgm(x, g, eps_iter, None, None)
    want = x.double() + eps_iter * g.double() / ss64.sqrt().view(-1, 1, 1, 1)
    yard = x + eps_iter * (g / torch.sqrt(torch.clamp(ss32.float(), min=1e-12)).view(-1, 1, 1, 1))
    ek, et = float((out.double() - want).abs().max()), float((yard.double() - want).abs().max())
    # the step has unit L2 norm to NORM_RTOL
    step = ((out.double() - x.double()) / eps_iter).flatten(1).norm(dim=1)
    print("FP64 l2_fgm {}: kernel/torch max err {:.3g}/{:.3g}; |step| - 1 max {:.3g}".format(
        shape, ek, et, float((step - 1).abs().max())))
    assert ek <= 2.0 * et + 4.0 * U * 1.5                       # |x + step| <= 1.5
    # projection of x + 3 * eps-ball worth of those gradients back onto the ball
    eps = 2.0
    adv = (x.double() + 3.0 * eps * g.double() / ss64.sqrt().view(-1, 1, 1, 1)).float()
    proj = ops.l2_project(adv, x, eps, None, None)
    eta64 = adv.double() - x.double()
    n64 = eta64.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
    want = x.double() + eta64 * torch.clamp(eps / n64, max=1.0)
    eta32 = adv - x
    n32 = eta32.flatten(1).norm(dim=1).view(-1, 1, 1, 1)
    yard = x + eta32 * torch.clamp(eps / torch.clamp(n32, min=1e-6), max=1.0)
    ek, et = float((proj.double() - want).abs().max()), float((yard.double() - want).abs().max())
    pn = (proj.double() - x.double()).flatten(1).norm(dim=1)
    print("FP64 l2_project {}: kernel/torch max err {:.3g}/{:.3g}; projected norm / eps {:.6f} .. {:.6f}".format(
        shape, ek, et, float(pn.min() / eps), float(pn.max() / eps)))
    assert ek <= 2.0 * et + 4.0 * U * 3.0                       # |x + eta| <= 3
