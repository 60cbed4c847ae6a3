"""TI (translation-invariant) gradient smoothing through the attack operators and the batched drivers, on the MI355X.

As in tests/test_momentum_attack.py the comparison is a loop written here: it takes every gradient from the SAME
``model_fn`` on the device (through the operators' own loss code, which TI does not touch), applies the numpy fp32
smoothing chain of tests/test_ti_kernels.py -- and, with a decay factor, the numpy momentum chain of
tests/test_momentum_kernels.py on the SMOOTHED gradient -- and the L-inf update in numpy on the host, and feeds the result
back.  Identical inputs give identical gradients, so the adversarial image (and the momentum) must be BIT-identical to the
product's.  Toy white box on the device, batch 3, 32 x 32 images, 4 iterations; eps = 3 steps, so the projection acts.
"""
import numpy as np
import pytest
import torch

from tests.test_momentum_attack import (BATCH, CLIP, DEV, EPS, EPS_ITER, IDS, ITERS, _assert_bits, _dev, _grad, _setup,
                                        _tiny)
from tests.test_momentum_kernels import _chain as _momentum_chain
from tests.test_ti_kernels import _chain as _ti_chain
from tests.test_ti_kernels import _sign

pytestmark = pytest.mark.gpu
DECAY, KERNLEN = 0.9, 7
F = np.float32


def _taps(kernlen=KERNLEN):
    from vqattack_amd import ops
    return ops.ti_gaussian_taps(kernlen)


def _host_update(x, m, g_dev, x0, decay, taps, eps_iter=EPS_ITER):
    """numpy fp32: smooth, then (decay given) the momentum chain on the smoothed gradient, then StepOp (x0 given) or FgmOp
    (x0 None) of csrc/common.hpp.  Returns (x, m)."""
    from vqattack_amd import ops
    d = _ti_chain(g_dev.cpu().numpy(), taps)
    if decay is not None:
        d = m = _momentum_chain(d, m, ops.sumabs_per_sample(_dev(d)).cpu().numpy(), decay)
    a = np.clip(x + F(eps_iter) * _sign(d), F(-1), F(1))
    if x0 is None:
        return a, m
    e = np.clip(a - x0, -F(EPS), F(EPS))
    out = np.clip(x0 + e, F(-1), F(1))
    assert out.dtype == np.float32
    return out, m


def _host_loop(flavor, dual, decay, vl=False, taps=None):
    taps = _taps() if taps is None else taps
    _, x0, start, y, fns, emb = _setup(flavor)
    x0h = x0.cpu().numpy()
    x = np.clip(start.cpu().numpy() + F(0), F(-1), F(1))
    m = np.zeros_like(x)
    for _ in range(ITERS):
        if vl:
            x, m = _host_update(x, m, _grad(fns["vl"], _dev(x), list(y["feat"]), 1, flavor, emb=emb), x0h, decay, taps)
        elif not dual:
            x, m = _host_update(x, m, _grad(fns["feat"], _dev(x), list(y["feat"]), 1, flavor), x0h, decay, taps)
        else:
            yd = y["dual"]
            if flavor == "albef":
                y_feat, y_mlm, extra = [yd[1], yd[2]], [yd[0]], dict(bkp=fns["feat"], bkp_y=[yd[1], yd[2]])
            else:
                y_feat, y_mlm, extra = list(yd), list(yd), {}
            x, m = _host_update(x, m, _grad(fns["feat"], _dev(x), y_feat, 1, flavor), None, decay, taps)   # no projection
            x, m = _host_update(x, m, _grad(fns["mlm"], _dev(x), y_mlm, 0, flavor, **extra), x0h, decay, taps)
    return x, m


def _pgd_args(flavor, dual):
    _, x0, start, y, fns, _ = _setup(flavor)
    fn, yy, ls = ([fns["feat"], fns["mlm"]], list(y["dual"]), 0) if dual else (fns["feat"], list(y["feat"]), 1)
    return fn, start, dict(y=yy, ori_x=x0, time=None, ls=ls, flavor=flavor, **CLIP)


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("decay", [None, DECAY])
def test_pgd_with_ti_equals_the_host_chain_bitwise(flavor, dual, decay):
    import vqattack_amd
    want_x, want_m = _host_loop(flavor, dual, decay)
    fn, start, kw = _pgd_args(flavor, dual)
    before = start.clone()
    m = torch.zeros_like(start)
    adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, ti_kernel=KERNLEN,
                                                          decay_factor=decay, momentum=m, **kw)
    assert len(losses) == ITERS * (2 if dual else 1) and torch.equal(start, before)
    _assert_bits(adv, want_x, "adv")
    if decay is not None:
        _assert_bits(m, want_m, "momentum")
    assert float((adv - kw["ori_x"]).abs().max()) <= EPS + 1e-6
    # smoothing changes the trajectory: the loop without it ends elsewhere
    fn, start, kw = _pgd_args(flavor, dual)
    plain, _ = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, decay_factor=decay, **kw)
    assert float((plain != adv).float().mean()) > 0.001


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_taps_given_as_a_sequence_are_used_as_they_are(flavor):
    import vqattack_amd
    taps = np.array([0.4, -0.1, 0.3, 0.25, 0.15], dtype=np.float32)          # asymmetric: a flipped kernel would show
    want_x, _ = _host_loop(flavor, False, None, taps=taps)
    fn, start, kw = _pgd_args(flavor, False)
    adv, _ = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, ti_kernel=taps.tolist(), **kw)
    _assert_bits(adv, want_x, "adv")


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("decay", [None, DECAY])
def test_pgd_vl_with_ti_equals_the_host_chain_bitwise(flavor, decay):
    import vqattack_amd
    _, x0, start, y, fns, emb = _setup(flavor)
    want_x, want_m = _host_loop(flavor, False, decay, vl=True)
    m = torch.zeros_like(start)
    adv, text_grad = vqattack_amd.projected_gradient_descent_vl(fns["vl"], [start, emb.clone()], EPS, EPS_ITER, ITERS,
                                                                np.inf, y=list(y["feat"]), ori_x=x0, time=None, ls=1,
                                                                attack_mask=[0, 2], flavor=flavor, ti_kernel=KERNLEN,
                                                                decay_factor=decay, momentum=m, **CLIP)
    _assert_bits(adv, want_x, "adv")
    if decay is not None:
        _assert_bits(m, want_m, "momentum")
    assert text_grad.shape[1] == 2


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_momentum_iterative_method_with_ti_is_ti_mi_fgsm(flavor):
    """Starts at x itself with the eps-ball around it, decay 1: smooth, normalise, accumulate, step."""
    import vqattack_amd
    from vqattack_amd import dropin
    _, x0, _, y, fns, _ = _setup(flavor)
    taps = _taps(15)
    x0h = x0.cpu().numpy()
    x, m = np.clip(x0h + F(0), F(-1), F(1)), np.zeros(x0.shape, np.float32)
    for _ in range(ITERS):
        x, m = _host_update(x, m, _grad(fns["feat"], _dev(x), list(y["feat"]), 1, flavor), x0h, 1.0, taps)
    m_dev = torch.zeros_like(x0)
    bound = dropin.load(flavor).momentum_iterative_method.momentum_iterative_method          # the drop-in binding
    adv, losses = bound(fns["feat"], x0, EPS, EPS_ITER, ITERS, np.inf, y=list(y["feat"]), momentum=m_dev, ti_kernel=15,
                        **CLIP)
    assert len(losses) == ITERS
    _assert_bits(adv, x, "adv")
    _assert_bits(m_dev, m, "momentum")


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_fast_gradient_method_with_ti(flavor):
    import vqattack_amd
    _, x0, start, y, fns, _ = _setup(flavor)
    x = np.clip(start.cpu().numpy() + F(0), F(-1), F(1))
    want, _ = _host_update(x, None, _grad(fns["feat"], _dev(x), list(y["feat"]), 1, flavor), None, None, _taps(),
                           eps_iter=EPS)
    xin = _dev(x)
    adv, _ = vqattack_amd.fast_gradient_method(fns["feat"], xin, EPS, np.inf, x0, y=list(y["feat"]), ls=1, flavor=flavor,
                                               ti_kernel=KERNLEN, **CLIP)
    _assert_bits(adv, want, "adv")
    plain, _ = vqattack_amd.fast_gradient_method(fns["feat"], xin, EPS, np.inf, x0, y=list(y["feat"]), ls=1,
                                                 flavor=flavor, **CLIP)
    assert not torch.equal(plain, adv)


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("decay", [None, DECAY])
def test_graph_replay_with_ti_equals_eager_bitwise(flavor, decay):
    import vqattack_amd
    res = []
    for graph in (False, True):
        fn, start, kw = _pgd_args(flavor, False)
        m = torch.zeros_like(start)
        adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, graph=graph,
                                                              ti_kernel=KERNLEN, decay_factor=decay, momentum=m, **kw)
        res.append((adv, m, losses))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    want_x, want_m = _host_loop(flavor, False, decay)
    _assert_bits(res[1][0], want_x, "adv")
    if decay is not None:
        _assert_bits(res[1][1], want_m, "momentum")


@pytest.mark.parametrize("decay", [None, DECAY])
def test_l2_loop_with_ti_equals_smoothing_in_front_of_the_existing_ops(decay):
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, _ = _setup("albef")
    eps, eps_iter = 1.0, 0.4
    taps = _taps()
    x = ops.linf_init(start, None, float("inf"), -1, 1)
    m = torch.zeros_like(start)
    for _ in range(ITERS):
        g = ops.ti_smooth(_grad(fns["feat"], x, list(y["feat"]), 1, "albef"), taps)     # checked bitwise in the kernel tests
        if decay is not None:
            g = ops.momentum_accumulate(g, m, decay)
        mid = ops.l2_fgm(x, g, eps_iter, -1, 1, check_range=False)
        x = ops.l2_project(mid, x0, eps, -1, 1)
    m_dev = torch.zeros_like(start)
    kw = dict(y=list(y["feat"]), ori_x=x0, time=None, ls=1, flavor="albef", decay_factor=decay, momentum=m_dev, **CLIP)
    adv, _ = vqattack_amd.projected_gradient_descent(fns["feat"], start, eps, eps_iter, ITERS, 2, ti_kernel=KERNLEN, **kw)
    assert torch.equal(adv, x) and torch.equal(m_dev, m)
    assert float((adv - x0).flatten(1).norm(dim=1).max()) <= eps * (1 + 1e-5)
    plain, _ = vqattack_amd.projected_gradient_descent(fns["feat"], start, eps, eps_iter, ITERS, 2, **kw)
    assert not torch.equal(plain, adv)


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("dual", [False, True])
def test_a_kernel_of_one_tap_gives_the_bits_of_the_call_without(flavor, dual):
    import vqattack_amd
    fn, start, kw = _pgd_args(flavor, dual)
    one, loss_one = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, ti_kernel=1, **kw)
    fn, start, kw = _pgd_args(flavor, dual)
    plain, loss_plain = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, **kw)
    assert torch.equal(one, plain) and loss_one == loss_plain


@pytest.mark.parametrize("dual", [False, True])
def test_without_a_ti_kernel_nothing_changes(dual):
    """``ti_kernel=None``: the call without the keyword, which is today's chain from the existing kernels alone."""
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, _ = _setup("albef")
    fn, start, kw = _pgd_args("albef", dual)
    adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, ti_kernel=None, **kw)
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


def test_image_must_have_planes():
    import vqattack_amd
    _, x0, start, y, fns, _ = _setup("albef")
    def never(_):
        raise AssertionError("refused before the white box runs")
    with pytest.raises(ValueError):
        vqattack_amd.projected_gradient_descent(never, start.flatten(1), EPS, EPS_ITER, 1, np.inf, y=list(y["feat"]),
                                                ori_x=x0.flatten(1), time=None, ls=1, flavor="albef", ti_kernel=KERNLEN,
                                                **CLIP)


# ------------------------------------------------------------------------------------------------ batched drivers
@pytest.mark.parametrize("flavor", ["vlmo", "albef"])
@pytest.mark.parametrize("decay", [None, 1.0])
def test_attack_mixed_with_ti_equals_the_per_sample_calls(flavor, decay):
    """One batch, three different schedules (0, 3 and 2 substitutable words), ``AttackConfig(ti_kernel=7)``: every sample
    must come out as from its own batch-1 ``attack_batch`` (identical token ids; >= 99 % of the pixels bit-identical, the
    tolerance of tests/test_attack_batched_parity.py for batch-size dependent rounding in the white box).  Sample 0
    finishes first: had a later global step touched it, the smoothed sign step would have moved nearly every pixel."""
    from vqattack_amd.attack import text_update
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    model, adapters_cls, cfg = _tiny(flavor, seed=3)
    g = torch.Generator().manual_seed(31)
    ids = torch.cat([IDS, torch.tensor([[101, 2003, 2009, 102, 0, 0, 0, 0]])])
    images = torch.empty(3, 3, cfg.image_size, cfg.image_size).uniform_(-1, 1, generator=g)
    eta = torch.empty_like(images).uniform_(-0.125, 0.125, generator=g)
    masks = (ids != 0).long()
    att = torch.zeros_like(ids, dtype=torch.bool)
    att[1, [1, 2, 4]] = True
    att[2, [1, 2]] = True
    sim = text_update.BagOfEmbeddingsSimilarity(seed=5)
    conf = dict(budget=10, sanity_checks=True, sim_threshold=0.3, ti_kernel=7, decay_factor=decay)
    attack = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(), AttackConfig(**conf), similarity_fn=sim)
    proposals = text_update.propose_candidates(attack.adapters.mlm_logits(ids.to(DEV), masks.to(DEV)), ids, att,
                                               threshold=0)
    res = attack.attack_mixed(images.to(DEV), ids.to(DEV), masks.to(DEV), att.to(DEV), init_eta=eta.to(DEV),
                              proposals=proposals)
    assert res.gradient_steps == 10 + 13 + 12
    plain = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(),
                            AttackConfig(**dict(conf, ti_kernel=None)), similarity_fn=sim)
    off = plain.attack_mixed(images.to(DEV), ids.to(DEV), masks.to(DEV), att.to(DEV), init_eta=eta.to(DEV),
                             proposals=proposals)
    assert float((off.adv_images != res.adv_images).float().mean()) > 0.01        # the smoothing acted
    for s in range(3):
        one = attack.attack_batch(images[s:s + 1].to(DEV), ids[s:s + 1].to(DEV), masks[s:s + 1].to(DEV),
                                  att[s:s + 1].to(DEV), init_eta=eta[s:s + 1].to(DEV),
                                  proposals=proposals[s:s + 1] if proposals[s] else None)
        same = (res.adv_images[s] == one.adv_images[0]).float().mean().item()
        assert same >= 0.99, (flavor, s, same)
        assert torch.equal(res.adv_text_ids[s], one.adv_text_ids[0]), (flavor, s)
        assert float((res.adv_images[s].cpu() - images[s]).abs().max()) <= np.float32(0.125) + 1e-7
