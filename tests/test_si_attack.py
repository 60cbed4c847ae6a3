"""SI-NI-FGSM (scale copies, Nesterov look-ahead) through the attack operators and the batched drivers, on the MI355X.

As in tests/test_di_attack.py the comparison is a loop written here.  Per gradient evaluation it makes the copies in
numpy (``s_i * (x [+ eps_iter * decay * m])``, one rounding per operation), takes one gradient per copy from the SAME
``model_fn`` on the device (through the operators' own loss code, which SI does not touch), combines them in numpy
(``w_0 g_0 + w_1 g_1 + ...`` ascending, ``w_i = s_i / n``), then -- where asked -- applies the numpy DI transform / adjoint
of tests/test_di_kernels.py (every copy of an evaluation with that evaluation's rows), the numpy TI chain of
tests/test_ti_kernels.py and the numpy momentum chain of tests/test_momentum_kernels.py, and the L-inf update in numpy, and
feeds the result back.  Identical inputs give identical gradients, so the adversarial image (and the momentum) must be
BIT-identical to the product's.  Toy white box on the device, batch 3, 32 x 32 images, 4 iterations; eps = 3 steps.
"""
import numpy as np
import pytest
import torch

from tests.pgd_reference import combine_np as _combine_np
from tests.pgd_reference import copies_np as _copies_np
from tests.test_di_attack import SHRINK, _di_kw, _rows
from tests.test_di_kernels import di_adjoint, di_forward
from tests.test_momentum_attack import (CLIP, DEV, EPS, EPS_ITER, IDS, ITERS, _assert_bits, _dev, _grad, _setup,
                                        _tiny)
from tests.test_momentum_kernels import _chain as _momentum_chain
from tests.test_ti_kernels import _chain as _ti_chain
from tests.test_ti_kernels import _sign

pytestmark = pytest.mark.gpu
DECAY, KERNLEN, SEED = 0.9, 7, 5
F = np.float32
# id -> (si_copies, nesterov, decay, ti_kernel, di)
COMBOS = {"si": (3, False, None, None, False), "ni": (None, True, DECAY, None, False),
          "si_ni": (3, True, DECAY, None, False), "si_ni_ti_di": (3, True, DECAY, KERNLEN, True)}


def _keys(combo, seed=SEED):
    n, nesterov, decay, ti, di = COMBOS[combo]
    kw = dict(si_copies=n, nesterov=nesterov, decay_factor=decay, ti_kernel=ti)
    if di:
        kw.update(_di_kw(seed))
    return kw


def _scales(n):
    from vqattack_amd import ops
    return ops.si_scales(1 if n is None else n)


def _step_np(x, d, x0, eps_iter, eps=EPS):
    """numpy fp32: StepOp (x0 given) or FgmOp (x0 None) of csrc/common.hpp."""
    a = np.clip(x + F(eps_iter) * _sign(d), F(-1), F(1))
    if x0 is None:
        return a
    out = np.clip(x0 + np.clip(a - x0, -F(eps), F(eps)), F(-1), F(1))
    assert out.dtype == np.float32
    return out


def _host_eval(x, m, combo, rows, grad_at, x0, eps_iter=EPS_ITER):
    """One gradient evaluation and update in numpy fp32.  ``grad_at(image, i)``: copy i's gradient from the device.
    Returns (x, m, copies as the model saw them)."""
    from vqattack_amd import ops
    n, nesterov, decay, ti, _ = COMBOS[combo] if isinstance(combo, str) else combo
    s = _scales(n)
    seen = _copies_np(x, s, m if nesterov else None, eps_iter * decay if nesterov else 0.0)
    if rows is not None:
        seen = [di_forward(c, rows) for c in seen]
    d = _combine_np([grad_at(_dev(c), i).cpu().numpy() for i, c in enumerate(seen)], ops.si_weights(s))
    if rows is not None:
        d = di_adjoint(d, rows)
    if ti is not None:
        d = _ti_chain(d, ops.ti_gaussian_taps(ti))
    if decay is not None:
        d = m = _momentum_chain(d, m, ops.sumabs_per_sample(_dev(d)).cpu().numpy(), decay)
    return _step_np(x, d, x0, eps_iter), m, seen


def _grad_vl(fn, x, y, flavor, emb, first):
    """(image gradient, text gradient or None): copy 0 carries the text leaf, the others see the text detached."""
    from vqattack_amd import attacks
    slot = attacks._LossSlot(torch.zeros(1, device=DEV), 0)
    leaf = x.detach().requires_grad_(True)
    if first:
        txt = emb.detach().requires_grad_(True)
        attacks._loss_and_grad(fn, [leaf, txt], [leaf, txt], y, 1, flavor, False, slot, vl=True)
        return leaf.grad.contiguous(), txt.grad.contiguous()
    attacks._loss_and_grad(fn, [leaf], [leaf, emb.detach()], y, 1, flavor, False, slot, vl=True)
    return leaf.grad.contiguous(), None


def _host_loop(flavor, dual, combo, vl=False, start=None):
    _, x0, start0, y, fns, emb = _setup(flavor)
    n, nesterov, decay, ti, di = COMBOS[combo]
    rows = _rows(ITERS * (2 if dual else 1)) if di else None
    x0h = x0.cpu().numpy()
    x = np.clip((start0 if start is None else start).cpu().numpy() + F(0), F(-1), F(1))
    m = np.zeros_like(x)
    text = [None]
    for i in range(ITERS):
        if vl:
            def grad_at(d, c):
                g, t = _grad_vl(fns["vl"], d, list(y["feat"]), flavor, emb, c == 0)
                if c == 0:
                    text[0] = t
                return g
            x, m, _ = _host_eval(x, m, combo, None if rows is None else rows[i], grad_at, x0h)
        elif not dual:
            x, m, _ = _host_eval(x, m, combo, None if rows is None else rows[i],
                                 lambda d, c: _grad(fns["feat"], d, list(y["feat"]), 1, flavor), x0h)
        else:
            yd = y["dual"]
            if flavor == "albef":
                y_feat, y_mlm, extra = [yd[1], yd[2]], [yd[0]], dict(bkp=fns["feat"], bkp_y=[yd[1], yd[2]])
            else:
                y_feat, y_mlm, extra = list(yd), list(yd), {}
            x, m, _ = _host_eval(x, m, combo, None if rows is None else rows[2 * i],
                                 lambda d, c: _grad(fns["feat"], d, y_feat, 1, flavor), None)     # no projection
            x, m, _ = _host_eval(x, m, combo, None if rows is None else rows[2 * i + 1],
                                 lambda d, c: _grad(fns["mlm"], d, y_mlm, 0, flavor, **extra), x0h)
    return x, m, text[0]


def _pgd_args(flavor, dual):
    _, x0, start, y, fns, _ = _setup(flavor)
    fn, yy, ls = ([fns["feat"], fns["mlm"]], list(y["dual"]), 0) if dual else (fns["feat"], list(y["feat"]), 1)
    return fn, start, dict(y=yy, ori_x=x0, time=None, ls=ls, flavor=flavor, **CLIP)


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_pgd_with_si_ni_equals_the_host_chain_bitwise(flavor, dual, combo):
    import vqattack_amd
    want_x, want_m, _ = _host_loop(flavor, dual, combo)
    fn, start, kw = _pgd_args(flavor, dual)
    before = start.clone()
    m = torch.zeros_like(start)
    adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, momentum=m,
                                                          **_keys(combo), **kw)
    assert len(losses) == ITERS * (2 if dual else 1) and torch.equal(start, before)
    _assert_bits(adv, want_x, "adv")
    if COMBOS[combo][2] is not None:
        _assert_bits(m, want_m, "momentum")
    assert float((adv - kw["ori_x"]).abs().max()) <= EPS + 1e-6
    # the copies / the look-ahead change the trajectory: the loop without them ends elsewhere
    fn, start, kw = _pgd_args(flavor, dual)
    keys = _keys(combo)
    keys.update(si_copies=None, nesterov=False)
    plain, _ = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, **keys, **kw)
    assert float((plain != adv).float().mean()) > 0.001


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("combo", ["si", "si_ni_ti_di"])
def test_pgd_vl_with_si_ni_equals_the_host_chain_bitwise_and_returns_copy_0s_text_gradient(flavor, combo):
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, emb = _setup(flavor)
    want_x, want_m, want_text = _host_loop(flavor, False, combo, vl=True)
    m = torch.zeros_like(start)
    adv, text_grad = vqattack_amd.projected_gradient_descent_vl(fns["vl"], [start, emb.clone()], EPS, EPS_ITER, ITERS,
                                                                np.inf, y=list(y["feat"]), ori_x=x0, time=None, ls=1,
                                                                attack_mask=[0, 2], flavor=flavor, momentum=m,
                                                                **_keys(combo), **CLIP)
    _assert_bits(adv, want_x, "adv")
    if COMBOS[combo][2] is not None:
        _assert_bits(m, want_m, "momentum")
    assert text_grad.shape[1] == 2
    assert torch.equal(text_grad, ops.gather_rows(want_text, [0, 2]))           # the last iteration's, from copy 0


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_momentum_iterative_method_with_si_ni(flavor):
    """SI-NI-FGSM as the paper runs it: starts at x itself with the eps-ball around it, decay 1."""
    from vqattack_amd import dropin
    _, x0, _, y, fns, _ = _setup(flavor)
    x0h = x0.cpu().numpy()
    x, m = np.clip(x0h + F(0), F(-1), F(1)), np.zeros(x0.shape, np.float32)
    for _ in range(ITERS):
        x, m, _ = _host_eval(x, m, (3, True, 1.0, None, False), None,
                             lambda d, c: _grad(fns["feat"], d, list(y["feat"]), 1, flavor), x0h)
    m_dev = torch.zeros_like(x0)
    bound = dropin.load(flavor).momentum_iterative_method.momentum_iterative_method          # the drop-in binding
    adv, losses = bound(fns["feat"], x0, EPS, EPS_ITER, ITERS, np.inf, y=list(y["feat"]), momentum=m_dev, si_copies=3,
                        nesterov=True, **CLIP)
    assert len(losses) == ITERS
    _assert_bits(adv, x, "adv")
    _assert_bits(m_dev, m, "momentum")


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("ti,di", [(None, False), (KERNLEN, True)], ids=["si", "si_ti_di"])
def test_fast_gradient_method_and_vl_with_si(flavor, ti, di):
    import vqattack_amd
    _, x0, start, y, fns, emb = _setup(flavor)
    x = np.clip(start.cpu().numpy() + F(0), F(-1), F(1))
    rows = _rows(1)[0] if di else None
    keys = dict(si_copies=3, ti_kernel=ti)
    combo = (3, False, None, ti, di)
    want, _, _ = _host_eval(x, None, combo, rows, lambda d, c: _grad(fns["feat"], d, list(y["feat"]), 1, flavor), None,
                            eps_iter=EPS)
    xin = _dev(x)
    adv, loss = vqattack_amd.fast_gradient_method(fns["feat"], xin, EPS, np.inf, x0, y=list(y["feat"]), ls=1,
                                                  flavor=flavor, **keys, **(_di_kw() if di else {}), **CLIP)
    _assert_bits(adv, want, "adv")
    assert torch.equal(xin, _dev(x))
    plain, loss_plain = vqattack_amd.fast_gradient_method(fns["feat"], xin, EPS, np.inf, x0, y=list(y["feat"]), ls=1,
                                                          flavor=flavor, ti_kernel=ti, **(_di_kw() if di else {}), **CLIP)
    assert not torch.equal(plain, adv)
    if not di:
        assert float(loss) == float(loss_plain)                                  # the reported loss is copy 0's (s = 1)
    want, _, seen = _host_eval(x, None, combo, rows,
                               lambda d, c: _grad_vl(fns["vl"], d, list(y["feat"]), flavor, emb, c == 0)[0], None,
                               eps_iter=EPS)
    xs = [xin, emb.clone()]
    adv, text_grad = vqattack_amd.fast_gradient_method_vl(fns["vl"], xs, EPS, np.inf, x0, y=list(y["feat"]), ls=1,
                                                          text_emb_pick=[0, 2], flavor=flavor, **keys,
                                                          **(_di_kw() if di else {}), **CLIP)
    _assert_bits(adv, want, "adv (vl)")
    assert text_grad.shape[1] == 2
    assert xs[0].requires_grad and xs[0].grad is not None                        # x[0] is copy 0's leaf
    _assert_bits(xs[0], seen[0], "x[0]")


@pytest.mark.parametrize("decay,nesterov", [(None, False), (DECAY, True)], ids=["si", "si_ni"])
def test_l2_loop_with_si_equals_the_combination_in_front_of_the_existing_ops(decay, nesterov):
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, _ = _setup("albef")
    eps, eps_iter = 1.0, 0.4
    s = ops.si_scales(3)
    w = ops.si_weights(s)
    x = ops.linf_init(start, None, float("inf"), -1, 1)
    m = torch.zeros_like(start)
    for _ in range(ITERS):
        seen = ops.si_copies(x, s, m=m if nesterov else None, lookahead=eps_iter * decay if nesterov else 0.0)
        g = ops.si_combine([_grad(fns["feat"], seen[i], list(y["feat"]), 1, "albef") for i in range(3)], w)
        if decay is not None:                                                   # (both checked bitwise in the kernel tests)
            g = ops.momentum_accumulate(g, m, decay)
        mid = ops.l2_fgm(x, g, eps_iter, -1, 1, check_range=False)
        x = ops.l2_project(mid, x0, eps, -1, 1)
    m_dev = torch.zeros_like(start)
    kw = dict(y=list(y["feat"]), ori_x=x0, time=None, ls=1, flavor="albef", decay_factor=decay, momentum=m_dev, **CLIP)
    adv, _ = vqattack_amd.projected_gradient_descent(fns["feat"], start, eps, eps_iter, ITERS, 2, si_copies=3,
                                                     nesterov=nesterov, **kw)
    assert torch.equal(adv, x) and torch.equal(m_dev, m)
    assert float((adv - x0).flatten(1).norm(dim=1).max()) <= eps * (1 + 1e-5)
    plain, _ = vqattack_amd.projected_gradient_descent(fns["feat"], start, eps, eps_iter, ITERS, 2, **kw)
    assert not torch.equal(plain, adv)


@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("decay", [None, DECAY])
def test_one_copy_without_the_look_ahead_is_the_plain_operator_bitwise(dual, decay):
    """si_copies=1: the copy is a bit copy, the weight is 1 and the combination the identity -- image, losses and momentum
    are the plain call's.  si_copies=3 ends elsewhere."""
    import vqattack_amd
    res = {}
    for n in (None, 1, 3):
        fn, start, kw = _pgd_args("albef", dual)
        m = torch.zeros_like(start)
        adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, si_copies=n,
                                                              decay_factor=decay, momentum=m, **kw)
        res[n] = (adv, losses, m)
    assert torch.equal(res[1][0], res[None][0]) and res[1][1] == res[None][1] and torch.equal(res[1][2], res[None][2])
    assert float((res[3][0] != res[None][0]).float().mean()) > 0.001
    assert res[3][1][0] == res[None][1][0]                                       # the first loss: copy 0 at the start point


@pytest.mark.parametrize("dual", [False, True])
def test_without_the_keys_nothing_changes(dual, monkeypatch):
    """``si_copies=None, nesterov=False``: the call without the keys, none of the new launches, and today's chain from
    the existing kernels alone."""
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, _ = _setup("albef")

    def never(*a, **k):
        raise AssertionError("the default path must not launch an SI kernel")
    for name in ("si_copies", "si_combine", "linf_si_step"):
        monkeypatch.setattr(ops, name, never)
    fn, start, kw = _pgd_args("albef", dual)
    adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, si_copies=None,
                                                          nesterov=False, **kw)
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


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("combo", ["si", "si_ni"])
def test_graph_replay_with_si_equals_eager_bitwise(flavor, combo):
    import vqattack_amd
    res = []
    for graph in (False, True):
        fn, start, kw = _pgd_args(flavor, False)
        m = torch.zeros_like(start)
        adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, graph=graph,
                                                              momentum=m, **_keys(combo), **kw)
        res.append((adv, m, losses))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    want_x, want_m, _ = _host_loop(flavor, False, combo)
    _assert_bits(res[1][0], want_x, "adv")
    if COMBOS[combo][2] is not None:
        _assert_bits(res[1][1], want_m, "momentum")


def test_a_closure_is_called_once_per_copy_in_ascending_order():
    """The model sees the copies one by one, largest scale first; a closure that draws draws once per call."""
    import vqattack_amd
    _, x0, start, y, fns, _ = _setup("albef")
    seen = []

    def spy(x):
        seen.append(x.detach().clone())
        return fns["feat"](x)
    vqattack_amd.projected_gradient_descent(spy, start, EPS, EPS_ITER, 2, np.inf, y=list(y["feat"]), ori_x=x0, time=None,
                                            ls=1, flavor="albef", si_copies=[1.0, 0.5, 0.25, 0.125], **CLIP)
    assert len(seen) == 2 * 4
    first = torch.clamp(start, -1, 1)
    for i in range(4):
        assert torch.equal(seen[i], first * 2.0 ** -i)


# ------------------------------------------------------------------------------------------------ batched drivers
def _driver_inputs(flavor):
    model, adapters_cls, cfg = _tiny(flavor)
    ids = IDS.to(DEV)
    masks = (ids != 0).long()
    g = torch.Generator().manual_seed(8)
    img = torch.empty(2, 3, cfg.image_size, cfg.image_size).uniform_(-1, 1, generator=g).to(DEV)
    eta = torch.empty(img.shape).uniform_(-0.125, 0.125, generator=g).to(DEV)
    return model, adapters_cls, cfg, ids, masks, img, eta


@pytest.mark.parametrize("flavor", ["vlmo", "albef"])
def test_attack_batch_with_the_keys_equals_the_operator_calls(flavor):
    """An image-only batch of two through ``attack_batch`` with ``AttackConfig(si_copies=3, nesterov=True)``: it is the
    operator call with the keys on the batch, and each sample on its own gives its rows of the batch."""
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    model, adapters_cls, cfg, ids, masks, img, eta = _driver_inputs(flavor)
    none = torch.zeros_like(ids, dtype=torch.bool)
    conf = AttackConfig(budget=5, si_copies=3, nesterov=True, decay_factor=1.0)
    atk = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(), conf)
    both = atk.attack_batch(img, ids, masks, none, init_eta=eta)
    off = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(), AttackConfig(budget=5, decay_factor=1.0))
    plain = off.attack_batch(img, ids, masks, none, init_eta=eta)
    assert float((plain.adv_images != both.adv_images).float().mean()) > 0.01
    assert float((both.adv_images - img).abs().max()) <= np.float32(0.125) + 1e-6
    # the operator itself, as _pgd_block calls it
    a = atk.adapters
    a.set_text(ids, masks)
    targets = a.gen_ori_feats(img)
    with torch.enable_grad():
        adv, losses = atk.pgd(a.pgd_attack, img, conf.eps, conf.eps_iter, 5, np.inf, y=atk._y_feature(targets), ls=1,
                              clip_min=conf.clip_min, clip_max=conf.clip_max, time=0, ori_x=img, sanity_checks=False,
                              init_eta=eta, decay_factor=1.0, si_copies=3, nesterov=True)
    assert torch.equal(adv, both.adv_images) and losses == both.loss_lists[0]
    for s in range(2):
        one = atk.attack_batch(img[s:s + 1], ids[s:s + 1], masks[s:s + 1], none[s:s + 1], init_eta=eta[s:s + 1])
        assert torch.equal(both.adv_images[s], one.adv_images[0]), (flavor, s)


@pytest.mark.parametrize("flavor", ["vlmo", "albef"])
@pytest.mark.parametrize("combo", ["si_ni", "si_ni_ti_di"])
def test_attack_mixed_with_si_ni_matches_a_host_restatement_of_its_step_rule(flavor, combo, monkeypatch):
    """``attack_mixed``'s own step loop.  Sample 0 has one substitutable word and so one step more than sample 1, which is
    finished at the last global step.  Every white-box call of the run is recorded (the image leaf it saw, the gradient it
    left); the restatement walks the steps in numpy: copies of the active prefix, looking ahead with the active prefix of
    the momentum -- checked against what the model saw, copy by copy --, the recorded gradients combined, DI adjoint / TI /
    momentum chains, StepOp on the prefix.  Image and momentum must come out bit-identical; the finished sample's rows of
    both stay as they were."""
    from vqattack_amd import attacks, ops
    from vqattack_amd.attack import text_update
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    n, nesterov, decay, ti, di = COMBOS[combo]
    model, adapters_cls, cfg, ids, masks, img, eta = _driver_inputs(flavor)
    att = torch.zeros_like(ids, dtype=torch.bool)
    att[0, 1] = True
    conf = AttackConfig(budget=4, si_copies=n, nesterov=nesterov, decay_factor=decay, ti_kernel=ti,
                        diversity_prob=1.0 if di else None, di_shrink=SHRINK, di_seed=SEED, sim_threshold=0.3)
    atk = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(), conf,
                          similarity_fn=text_update.BagOfEmbeddingsSimilarity(seed=5))
    proposals = text_update.propose_candidates(atk.adapters.mlm_logits(ids, masks), ids.cpu(), att.cpu(), threshold=0)
    calls, held = [], []
    for name in ("_loss_and_grad", "_mixed_loss_and_grad"):
        inner = getattr(attacks, name)

        def outer(fn, leaves, *a, _inner=inner, **k):
            out = _inner(fn, leaves, *a, **k)
            calls.append((leaves[0].detach().cpu().numpy().copy(), leaves[0].grad.detach().cpu().numpy().copy(),
                          len(leaves)))
            return out
        monkeypatch.setattr(attacks, name, outer)
    new_momentum = atk._new_momentum
    monkeypatch.setattr(atk, "_new_momentum", lambda images: held.append(new_momentum(images)) or held[-1])
    res = atk.attack_mixed(img, ids, masks, att, init_eta=eta, proposals=proposals)
    monkeypatch.undo()
    steps = res.global_steps
    assert len(calls) == n * steps and res.sample_steps == 2 * steps - 1          # sample 1 stops one step early
    assert [c[2] for c in calls] == [2, 1, 1] * steps                             # copy 0 carries the text leaf
    # ---- the restatement
    s = ops.si_scales(n)
    w = ops.si_weights(s)
    rows = ops.di_draw(np.random.RandomState(SEED), 2, steps, cfg.image_size, cfg.image_size, shrink=SHRINK) if di else None
    x0h = img.cpu().numpy()
    x = ops.linf_init(img, eta, conf.eps, -1, 1).cpu().numpy()                    # the existing start kernel
    m = np.zeros_like(x)
    before_last = None
    for t in range(steps):
        act = calls[n * t][0].shape[0]
        assert act == (2 if t < steps - 1 else 1)
        if t == steps - 1:
            before_last = (x.copy(), m.copy())
        seen = _copies_np(x[:act], s, m[:act], conf.eps_iter * decay)
        if di:
            seen = [di_forward(c, rows[t][:act]) for c in seen]
        for i in range(n):
            assert np.array_equal(seen[i].view(np.int32), calls[n * t + i][0].view(np.int32)), (t, i)
        d = _combine_np([calls[n * t + i][1] for i in range(n)], w)
        if di:
            d = di_adjoint(d, rows[t][:act])
        if ti is not None:
            d = _ti_chain(d, ops.ti_gaussian_taps(ti))
        d = _momentum_chain(d, m[:act], ops.sumabs_per_sample(_dev(d)).cpu().numpy(), decay)
        m[:act] = d
        x[:act] = _step_np(x[:act], d, x0h[:act], conf.eps_iter, eps=conf.eps)
    _assert_bits(res.adv_images, x, "adv")
    _assert_bits(held[0], m, "momentum")
    assert np.array_equal(x[1], before_last[0][1]) and np.array_equal(m[1], before_last[1][1])
    assert not np.array_equal(x[0], before_last[0][0])
    assert float((res.adv_images - img).abs().max()) <= np.float32(0.125) + 1e-6
