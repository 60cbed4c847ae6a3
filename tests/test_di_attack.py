"""Input diversity (DI-FGSM) through the attack operators and the batched drivers, on the MI355X.

As in tests/test_ti_attack.py the comparison is a loop written here.  Per gradient evaluation it transforms the image with
the numpy chain of tests/test_di_kernels.py, takes the gradient from the SAME ``model_fn`` on the device at the
transformed image (through the operators' own loss code, which DI does not touch), applies the numpy adjoint, then --
where asked -- the numpy TI chain of tests/test_ti_kernels.py and the numpy momentum chain of
tests/test_momentum_kernels.py, and the L-inf update in numpy, and feeds the result back.  Identical inputs give identical
gradients, so the adversarial image (and the momentum) must be BIT-identical to the product's.  The rows come from
``ops.di_draw`` with a ``RandomState`` of the seed the operator gets (tests/test_di_host.py checks the draws themselves).
Toy white box on the device, batch 3, 32 x 32 images, 4 iterations, shrink 8 (new_h in 24..31); eps = 3 steps.
"""
import numpy as np
import pytest
import torch

from tests.test_di_kernels import di_adjoint, di_forward
from tests.test_momentum_attack import (BATCH, CLIP, DEV, EPS, EPS_ITER, IDS, ITERS, _assert_bits, _dev, _grad, _setup,
                                        _tiny)
from tests.test_momentum_kernels import _chain as _momentum_chain
from tests.test_ti_kernels import _chain as _ti_chain
from tests.test_ti_kernels import _sign

pytestmark = pytest.mark.gpu
DECAY, KERNLEN, SHRINK, SEED, SIZE = 0.9, 7, 8, 5, 32
F = np.float32


def _rows(n_evals, batch=BATCH, seed=SEED, prob=1.0):
    from vqattack_amd import ops
    return ops.di_draw(np.random.RandomState(seed), batch, n_evals, SIZE, SIZE, shrink=SHRINK, prob=prob)


def _di_kw(seed=SEED, prob=1.0):
    return dict(diversity_prob=prob, di_shrink=SHRINK, di_rng=np.random.RandomState(seed))


def _host_eval(x, m, rows, grad_at, x0, decay, taps, eps_iter=EPS_ITER):
    """One gradient evaluation and update in numpy fp32: transform, gradient at the transformed image (device), adjoint,
    (TI chain), (momentum chain), StepOp (x0 given) or FgmOp (x0 None) of csrc/common.hpp.  Returns (x, m)."""
    from vqattack_amd import ops
    d = di_adjoint(grad_at(_dev(di_forward(x, rows))).cpu().numpy(), rows)
    if taps is not None:
        d = _ti_chain(d, taps)
    if decay is not None:
        d = m = _momentum_chain(d, m, ops.sumabs_per_sample(_dev(d)).cpu().numpy(), decay)
    a = np.clip(x + F(eps_iter) * _sign(d), F(-1), F(1))
    if x0 is None:
        return a, m
    e = np.clip(a - x0, -F(EPS), F(EPS))
    out = np.clip(x0 + e, F(-1), F(1))
    assert out.dtype == np.float32
    return out, m


def _taps(ti):
    from vqattack_amd import ops
    return None if ti is None else ops.ti_gaussian_taps(ti)


def _host_loop(flavor, dual, decay=None, ti=None, vl=False, rows=None):
    taps = _taps(ti)
    _, x0, start, y, fns, emb = _setup(flavor)
    rows = _rows(ITERS * (2 if dual else 1)) if rows is None else rows
    x0h = x0.cpu().numpy()
    x = np.clip(start.cpu().numpy() + F(0), F(-1), F(1))
    m = np.zeros_like(x)
    for i in range(ITERS):
        if vl:
            x, m = _host_eval(x, m, rows[i], lambda d: _grad(fns["vl"], d, list(y["feat"]), 1, flavor, emb=emb), x0h, decay,
                              taps)
        elif not dual:
            x, m = _host_eval(x, m, rows[i], lambda d: _grad(fns["feat"], d, list(y["feat"]), 1, flavor), x0h, decay, taps)
        else:
            yd = y["dual"]
            if flavor == "albef":
                y_feat, y_mlm, extra = [yd[1], yd[2]], [yd[0]], dict(bkp=fns["feat"], bkp_y=[yd[1], yd[2]])
            else:
                y_feat, y_mlm, extra = list(yd), list(yd), {}
            x, m = _host_eval(x, m, rows[2 * i], lambda d: _grad(fns["feat"], d, y_feat, 1, flavor), None, decay, taps)
            x, m = _host_eval(x, m, rows[2 * i + 1], lambda d: _grad(fns["mlm"], d, y_mlm, 0, flavor, **extra), x0h, decay,
                              taps)
    return x, m


def _pgd_args(flavor, dual):
    _, x0, start, y, fns, _ = _setup(flavor)
    fn, yy, ls = ([fns["feat"], fns["mlm"]], list(y["dual"]), 0) if dual else (fns["feat"], list(y["feat"]), 1)
    return fn, start, dict(y=yy, ori_x=x0, time=None, ls=ls, flavor=flavor, **CLIP)


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("decay,ti", [(None, None), (None, KERNLEN), (DECAY, None), (DECAY, KERNLEN)],
                         ids=["di", "di_ti", "di_mi", "di_ti_mi"])
def test_pgd_with_di_equals_the_host_chain_bitwise(flavor, dual, decay, ti):
    import vqattack_amd
    want_x, want_m = _host_loop(flavor, dual, decay, ti)
    fn, start, kw = _pgd_args(flavor, dual)
    before = start.clone()
    m = torch.zeros_like(start)
    adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, ti_kernel=ti,
                                                          decay_factor=decay, momentum=m, **_di_kw(), **kw)
    assert len(losses) == ITERS * (2 if dual else 1) and torch.equal(start, before)
    _assert_bits(adv, want_x, "adv")
    if decay is not None:
        _assert_bits(m, want_m, "momentum")
    assert float((adv - kw["ori_x"]).abs().max()) <= EPS + 1e-6
    # the transform changes the trajectory: the loop without it ends elsewhere
    fn, start, kw = _pgd_args(flavor, dual)
    plain, _ = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, ti_kernel=ti,
                                                       decay_factor=decay, **kw)
    assert float((plain != adv).float().mean()) > 0.001


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_a_probability_in_between_transforms_some_samples_only(flavor):
    import vqattack_amd
    rows = _rows(ITERS, seed=9, prob=0.5)
    ident = (rows == [SIZE, SIZE, 0, 0]).all(axis=-1)
    assert ident.any() and not ident.all()
    want_x, _ = _host_loop(flavor, False, rows=rows)
    fn, start, kw = _pgd_args(flavor, False)
    adv, _ = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, **_di_kw(seed=9, prob=0.5),
                                                     **kw)
    _assert_bits(adv, want_x, "adv")


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("decay", [None, DECAY])
def test_pgd_vl_with_di_equals_the_host_chain_bitwise(flavor, decay):
    import vqattack_amd
    _, x0, start, y, fns, emb = _setup(flavor)
    want_x, want_m = _host_loop(flavor, False, decay, vl=True)
    m = torch.zeros_like(start)
    adv, text_grad = vqattack_amd.projected_gradient_descent_vl(fns["vl"], [start, emb.clone()], EPS, EPS_ITER, ITERS,
                                                                np.inf, y=list(y["feat"]), ori_x=x0, time=None, ls=1,
                                                                attack_mask=[0, 2], flavor=flavor, decay_factor=decay,
                                                                momentum=m, **_di_kw(), **CLIP)
    _assert_bits(adv, want_x, "adv")
    if decay is not None:
        _assert_bits(m, want_m, "momentum")
    assert text_grad.shape[1] == 2


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("ti", [None, 15])
def test_momentum_iterative_method_with_di(flavor, ti):
    """M-DI2-FGSM (and TI-DIM with a kernel): starts at x itself with the eps-ball around it, decay 1."""
    from vqattack_amd import dropin
    _, x0, _, y, fns, _ = _setup(flavor)
    rows, taps = _rows(ITERS), _taps(ti)
    x0h = x0.cpu().numpy()
    x, m = np.clip(x0h + F(0), F(-1), F(1)), np.zeros(x0.shape, np.float32)
    for i in range(ITERS):
        x, m = _host_eval(x, m, rows[i], lambda d: _grad(fns["feat"], d, list(y["feat"]), 1, flavor), x0h, 1.0, taps)
    m_dev = torch.zeros_like(x0)
    bound = dropin.load(flavor).momentum_iterative_method.momentum_iterative_method          # the drop-in binding
    adv, losses = bound(fns["feat"], x0, EPS, EPS_ITER, ITERS, np.inf, y=list(y["feat"]), momentum=m_dev, ti_kernel=ti,
                        **_di_kw(), **CLIP)
    assert len(losses) == ITERS
    _assert_bits(adv, x, "adv")
    _assert_bits(m_dev, m, "momentum")


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("ti", [None, KERNLEN])
def test_fast_gradient_method_and_vl_with_di(flavor, ti):
    import vqattack_amd
    _, x0, start, y, fns, emb = _setup(flavor)
    x = np.clip(start.cpu().numpy() + F(0), F(-1), F(1))
    rows = _rows(1)
    want, _ = _host_eval(x, None, rows[0], lambda d: _grad(fns["feat"], d, list(y["feat"]), 1, flavor), None, None,
                         _taps(ti), eps_iter=EPS)
    xin = _dev(x)
    adv, _ = vqattack_amd.fast_gradient_method(fns["feat"], xin, EPS, np.inf, x0, y=list(y["feat"]), ls=1, flavor=flavor,
                                               ti_kernel=ti, **_di_kw(), **CLIP)
    _assert_bits(adv, want, "adv")
    assert torch.equal(xin, _dev(x))
    plain, _ = vqattack_amd.fast_gradient_method(fns["feat"], xin, EPS, np.inf, x0, y=list(y["feat"]), ls=1,
                                                 flavor=flavor, ti_kernel=ti, **CLIP)
    assert not torch.equal(plain, adv)
    want, _ = _host_eval(x, None, rows[0], lambda d: _grad(fns["vl"], d, list(y["feat"]), 1, flavor, emb=emb), None, None,
                         _taps(ti), eps_iter=EPS)
    adv, text_grad = vqattack_amd.fast_gradient_method_vl(fns["vl"], [xin, emb.clone()], EPS, np.inf, x0,
                                                          y=list(y["feat"]), ls=1, text_emb_pick=[0, 2], flavor=flavor,
                                                          ti_kernel=ti, **_di_kw(), **CLIP)
    _assert_bits(adv, want, "adv (vl)")
    assert text_grad.shape[1] == 2


class _Cycle:
    """A generator that repeats the first ``n`` draws of a ``RandomState``: the table frozen at step 0."""

    def __init__(self, seed, n):
        self.rs, self.n, self.vals, self.i = np.random.RandomState(seed), n, [], 0

    def uniform(self, *a):
        if len(self.vals) < self.n:
            self.vals.append(self.rs.uniform(*a))
        self.i += 1
        return self.vals[(self.i - 1) % self.n]


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("decay,ti", [(None, None), (DECAY, KERNLEN)], ids=["di", "di_ti_mi"])
def test_graph_replay_with_di_equals_eager_bitwise_with_fresh_rows_per_replay(flavor, decay, ti):
    import vqattack_amd
    res = []
    for graph in (False, True):
        fn, start, kw = _pgd_args(flavor, False)
        m = torch.zeros_like(start)
        adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, graph=graph,
                                                              ti_kernel=ti, decay_factor=decay, momentum=m, **_di_kw(),
                                                              **kw)
        res.append((adv, m, losses))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    want_x, want_m = _host_loop(flavor, False, decay, ti)
    _assert_bits(res[1][0], want_x, "adv")
    if decay is not None:
        _assert_bits(res[1][1], want_m, "momentum")
    # a replay that kept the rows of the captured iteration would give the run with the table frozen at step 0
    fn, start, kw = _pgd_args(flavor, False)
    frozen_rng = _Cycle(SEED, 4 * BATCH)
    frozen, _ = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, graph=True, ti_kernel=ti,
                                                        decay_factor=decay, diversity_prob=1.0, di_shrink=SHRINK,
                                                        di_rng=frozen_rng, **kw)
    assert frozen_rng.i == 4 * BATCH * ITERS
    assert float((frozen != res[1][0]).float().mean()) > 0.001


@pytest.mark.parametrize("decay", [None, DECAY])
def test_l2_loop_with_di_equals_the_adjoint_in_front_of_the_existing_ops(decay):
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, _ = _setup("albef")
    eps, eps_iter = 1.0, 0.4
    table = ops.di_geometry(_rows(ITERS), SIZE, SIZE, DEV)
    x = ops.linf_init(start, None, float("inf"), -1, 1)
    m = torch.zeros_like(start)
    for i in range(ITERS):
        d = ops.di_transform(x, table[i])                                              # both checked bitwise in the
        g = ops.di_adjoint(_grad(fns["feat"], d, list(y["feat"]), 1, "albef"), table[i])   # kernel tests
        if decay is not None:
            g = ops.momentum_accumulate(g, m, decay)
        mid = ops.l2_fgm(x, g, eps_iter, -1, 1, check_range=False)
        x = ops.l2_project(mid, x0, eps, -1, 1)
    m_dev = torch.zeros_like(start)
    kw = dict(y=list(y["feat"]), ori_x=x0, time=None, ls=1, flavor="albef", decay_factor=decay, momentum=m_dev, **CLIP)
    adv, _ = vqattack_amd.projected_gradient_descent(fns["feat"], start, eps, eps_iter, ITERS, 2, **_di_kw(), **kw)
    assert torch.equal(adv, x) and torch.equal(m_dev, m)
    assert float((adv - x0).flatten(1).norm(dim=1).max()) <= eps * (1 + 1e-5)
    plain, _ = vqattack_amd.projected_gradient_descent(fns["feat"], start, eps, eps_iter, ITERS, 2, **kw)
    assert not torch.equal(plain, adv)


class _NoDraw:
    def uniform(self, *a):
        raise AssertionError("diversity_prob=None must not draw")


@pytest.mark.parametrize("dual", [False, True])
def test_without_a_diversity_prob_nothing_changes(dual):
    """``diversity_prob=None``: the call without the keys, which is today's chain from the existing kernels alone."""
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, _ = _setup("albef")
    fn, start, kw = _pgd_args("albef", dual)
    adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, diversity_prob=None,
                                                          di_shrink=SHRINK, di_rng=_NoDraw(), **kw)
    fn, start, kw = _pgd_args("albef", dual)
    again, losses2 = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, **kw)
    assert torch.equal(adv, again) and losses == losses2
    x = ops.linf_init(start, None, EPS, -1, 1)
    yd = y["dual"]
    for _ in range(ITERS):
        if dual:
            x = ops.linf_fgm(x, _grad(fns["feat"], x, [yd[1], yd[2]], 1, "albef"), EPS_ITER, -1, 1)
            x = ops.linf_step(x, _grad(fns["mlm"], x, [yd[0]], 0, "albef", bkp=fns["feat"], bkp_y=[yd[1], yd[2]]), x0,
                              EPS_ITER, EPS, -1, 1)
        else:
            x = ops.linf_step(x, _grad(fns["feat"], x, list(y["feat"]), 1, "albef"), x0, EPS_ITER, EPS, -1, 1)
    assert torch.equal(adv, x)


def test_probability_zero_gives_the_plain_trajectory_up_to_the_sign_of_zero():
    """Identity rows: T is the identity and its adjoint returns the gradient with -0 as +0, which sign() does not see."""
    import vqattack_amd
    fn, start, kw = _pgd_args("albef", False)
    zero, loss_zero = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf,
                                                              **_di_kw(prob=0.0), **kw)
    fn, start, kw = _pgd_args("albef", False)
    plain, loss_plain = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, **kw)
    assert torch.equal(zero, plain) and loss_zero == loss_plain


def test_image_must_have_planes():
    import vqattack_amd
    _, x0, start, y, fns, _ = _setup("albef")

    def never(_):
        raise AssertionError("refused before the white box runs")
    with pytest.raises(ValueError):
        vqattack_amd.projected_gradient_descent(never, start.flatten(1), EPS, EPS_ITER, 1, np.inf, y=list(y["feat"]),
                                                ori_x=x0.flatten(1), time=None, ls=1, flavor="albef", **_di_kw(), **CLIP)


# ------------------------------------------------------------------------------------------------ batched drivers
class _Record:
    def __init__(self, seed):
        self.rs, self.vals = np.random.RandomState(seed), []

    def uniform(self, *a):
        self.vals.append(self.rs.uniform(*a))
        return self.vals[-1]


class _Replay:
    def __init__(self, vals):
        self.vals, self.i = list(vals), 0

    def uniform(self, *a):
        self.i += 1
        return self.vals[self.i - 1]


@pytest.mark.parametrize("flavor", ["vlmo", "albef"])
def test_attack_batch_with_di_equals_the_per_sample_calls_with_the_same_rows(flavor):
    """An image-only batch of two through ``attack_batch`` with ``AttackConfig(diversity_prob=1)``, and each sample on its
    own with the draws the batch made for it (4 per gradient evaluation, sample-minor)."""
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    model, adapters_cls, cfg = _tiny(flavor)
    ids = IDS.to(DEV)
    masks = (ids != 0).long()
    g = torch.Generator().manual_seed(8)
    img = torch.empty(2, 3, cfg.image_size, cfg.image_size).uniform_(-1, 1, generator=g).to(DEV)
    eta = torch.empty(img.shape).uniform_(-0.125, 0.125, generator=g).to(DEV)
    none = torch.zeros_like(ids, dtype=torch.bool)
    conf = AttackConfig(budget=6, diversity_prob=1.0, di_shrink=SHRINK, di_seed=SEED)
    atk = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(), conf)
    seeded = atk.attack_batch(img, ids, masks, none, init_eta=eta)
    rec = _Record(SEED)
    atk.di_rng = rec
    both = atk.attack_batch(img, ids, masks, none, init_eta=eta)
    assert torch.equal(seeded.adv_images, both.adv_images)                   # di_seed is RandomState(di_seed)
    assert len(rec.vals) == 4 * 2 * 6
    off = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(), AttackConfig(budget=6))
    plain = off.attack_batch(img, ids, masks, none, init_eta=eta)
    assert float((plain.adv_images != both.adv_images).float().mean()) > 0.01
    draws = np.array(rec.vals).reshape(-1, 2, 4)
    for s in range(2):
        atk.di_rng = _Replay(draws[:, s].reshape(-1))
        one = atk.attack_batch(img[s:s + 1], ids[s:s + 1], masks[s:s + 1], none[s:s + 1], init_eta=eta[s:s + 1])
        ref = off.attack_batch(img[s:s + 1], ids[s:s + 1], masks[s:s + 1], none[s:s + 1], init_eta=eta[s:s + 1])
        same = (both.adv_images[s] == one.adv_images[0]).float().mean().item()
        same_plain = (plain.adv_images[s] == ref.adv_images[0]).float().mean().item()
        print("attack_batch vs per-sample, {} sample {}: {:.6f} of the pixels equal with DI, {:.6f} without".format(
            flavor, s, same, same_plain))
        assert torch.equal(both.adv_images[s], one.adv_images[0]), (flavor, s, same, same_plain)
        assert float((both.adv_images[s] - img[s]).abs().max()) <= np.float32(0.125) + 1e-6


@pytest.mark.parametrize("flavor", ["vlmo", "albef"])
@pytest.mark.parametrize("decay,ti", [(None, None), (1.0, 7)], ids=["di", "di_ti_mi"])
def test_attack_mixed_with_di_runs_the_step_loop_with_per_step_rows(flavor, decay, ti):
    """``attack_mixed``'s own step loop (one table per call, the active prefix per global step): reproducible from
    ``di_seed``, different for another seed and without DI, inside the eps-ball; with TI and momentum the adjoint goes
    through the call's scratch.  The kernels it launches are compared bitwise in the operator tests above."""
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    model, adapters_cls, cfg = _tiny(flavor)
    ids = IDS.to(DEV)
    masks = (ids != 0).long()
    g = torch.Generator().manual_seed(8)
    img = torch.empty(2, 3, cfg.image_size, cfg.image_size).uniform_(-1, 1, generator=g).to(DEV)
    eta = torch.empty(img.shape).uniform_(-0.125, 0.125, generator=g).to(DEV)
    none = torch.zeros_like(ids, dtype=torch.bool)
    conf = dict(budget=5, diversity_prob=1.0, di_shrink=SHRINK, di_seed=SEED, decay_factor=decay, ti_kernel=ti)
    atk = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(), AttackConfig(**conf))
    res = atk.attack_mixed(img, ids, masks, none, init_eta=eta)
    again = atk.attack_mixed(img, ids, masks, none, init_eta=eta)
    assert torch.equal(res.adv_images, again.adv_images)                     # a fresh RandomState(di_seed) per call
    off = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(),
                          AttackConfig(**dict(conf, diversity_prob=None)))
    plain = off.attack_mixed(img, ids, masks, none, init_eta=eta)
    assert float((plain.adv_images != res.adv_images).float().mean()) > 0.01
    assert float((res.adv_images - img).abs().max()) <= np.float32(0.125) + 1e-6
    other = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(),
                            AttackConfig(**dict(conf, di_seed=SEED + 1)))
    assert not torch.equal(other.attack_mixed(img, ids, masks, none, init_eta=eta).adv_images, res.adv_images)
