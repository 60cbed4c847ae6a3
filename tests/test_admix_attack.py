"""Admix (mixed-image copies) through the attack operators and the batched driver, on the MI355X.

As in tests/test_si_attack.py and tests/test_vt_attack.py the comparison is a loop written here, a host restatement of the
rule the operators document.  The partner table is drawn from an identically seeded ``RandomState`` through the stated
rule.  Per gradient evaluation ``G(t, src)`` makes, group by group, the mixed image ``v = t + eta * src[partner_j]`` and
its scale copies ``s_i * v`` in numpy (one rounding per operation), takes one gradient per copy from the SAME ``model_fn``
on the device (through the operators' own loss code, which Admix does not touch) and keeps the running sum ``gsum = w_0 *
g_00; gsum = gsum + w_i * g_ji`` in numpy, ``w_i = s_i / (m1 * m2)``; then -- where asked -- the numpy DI transform /
adjoint (every copy of an evaluation with that evaluation's rows), variance tuning with the numpy Philox neighbours (each
neighbour tensor mixed with its own samples), the numpy TI and momentum chains and the L-inf update in numpy, and feeds
the result back.  ``t`` is the image or the Nesterov look-ahead point, ``src`` always the image itself.  Identical inputs
give identical gradients, so the adversarial image (and the momentum) must be BIT-identical to the product's.
Toy white box on the device, batch 3, 32 x 32 images, 3 iterations, m2 = 3 (2 with variance tuning), eps = 3 steps.
"""
import numpy as np
import pytest
import torch

from tests.test_di_attack import _di_kw, _rows
from tests.test_di_kernels import di_adjoint, di_forward
from tests.test_momentum_attack import BATCH, CLIP, DEV, EPS, EPS_ITER, _assert_bits, _dev, _grad, _setup
from tests.test_momentum_kernels import _chain as _momentum_chain
from tests.test_si_attack import _driver_inputs, _grad_vl, _pgd_args, _step_np
from tests.test_ti_kernels import _chain as _ti_chain
from tests.test_vt_kernels import _noise_np

pytestmark = pytest.mark.gpu
DECAY, KERNLEN, DI_SEED, AX_SEED, VT_SEED, BETA, ITERS, ETA = 0.9, 7, 5, 23, 0xC0FFEE1234567, 1.5, 3, 0.2
F = np.float32
# id -> (si_copies, nesterov, decay, ti_kernel, di, vt_neighbors, admix_images)
COMBOS = {"admix": (None, False, None, None, False, None, 3), "admix_si": (2, False, None, None, False, None, 3),
          "admix_mi_ni": (None, True, DECAY, None, False, None, 3), "admix_di_ti_mi": (None, False, DECAY, KERNLEN, True, None, 3),
          "admix_vt": (None, False, None, None, False, 2, 2)}


def _keys(combo, eta=ETA):
    copies, nesterov, decay, ti, di, vt, images = COMBOS[combo] if isinstance(combo, str) else combo
    kw = dict(si_copies=copies, nesterov=nesterov, decay_factor=decay, ti_kernel=ti, admix_images=images, admix_eta=eta,
              admix_rng=np.random.RandomState(AX_SEED))
    if vt is not None:
        kw.update(vt_neighbors=vt, vt_beta=BETA, vt_seed=VT_SEED)
    if di:
        kw.update(_di_kw(DI_SEED))
    return kw


def _table(n_evals, images, batch=BATCH):
    """The partner table by the stated rule, from the generator the operator is given a twin of."""
    r = np.random.RandomState(AX_SEED)
    t = np.empty((n_evals, images, batch), dtype=np.int64)
    for e in range(n_evals):
        for j in range(images):
            for b in range(batch):
                t[e, j, b] = (b + 1 + min(int(r.uniform() * (batch - 1)), batch - 2)) % batch
    assert not np.any(t == np.arange(batch))
    return t


def _g_np(t, src, combo, prow, rows, grad_at, centre, eta=ETA, seen_out=None):
    """``G`` in numpy fp32: group by group the mixed copies, one device gradient per copy, the running sum; then the DI
    adjoint.  ``grad_at(image, first)``: ``first`` for the first copy of the first group of the centre."""
    from vqattack_amd import ops
    copies, images = combo[0], combo[6]
    s = ops.si_scales(1 if copies is None else copies)
    w = (s / F(s.size * images)).astype(F)
    gsum = None
    for j in range(images):
        u = F(eta) * src[prow[j]]
        v = t + u
        for i in range(s.size):
            seen = F(s[i]) * v
            assert seen.dtype == F
            if rows is not None:
                seen = di_forward(seen, rows)
            if seen_out is not None:
                seen_out.append(seen)
            term = F(w[i]) * grad_at(_dev(seen), centre and i == 0 and j == 0).cpu().numpy()
            gsum = term if gsum is None else gsum + term
    assert gsum.dtype == F
    return gsum if rows is None else di_adjoint(gsum, rows)


def _host_eval(x, m, v, combo, prow, rows, grad_at, x0, t_eval, eps=EPS, eps_iter=EPS_ITER, eta=ETA, seen_out=None):
    """One evaluation and update in numpy fp32.  Returns (x, m, v)."""
    from vqattack_amd import ops
    _, nesterov, decay, ti, _, vt, _ = combo
    p = x + F(eps_iter * decay) * m if nesterov else x
    d = _g_np(p, x, combo, prow, rows, grad_at, True, eta, seen_out)
    if vt is not None:
        bound, total = float(F(BETA * eps)), None
        for i in range(vt):
            q = p + _noise_np(x.shape, VT_SEED, t_eval, i, bound)
            gi = _g_np(q, q, combo, prow, rows, grad_at, False, eta)
            total = gi if total is None else total + gi
        g = d
        d = g + v
        v = (F(1.0) / F(vt)) * total - g
    if ti is not None:
        d = _ti_chain(d, ops.ti_gaussian_taps(ti))
    if decay is not None:
        d = m = _momentum_chain(d, m, ops.sumabs_per_sample(_dev(d)).cpu().numpy(), decay)
    return _step_np(x, d, x0, eps_iter, eps=eps), m, v


def _host_loop(flavor, dual, combo, vl=False, iters=ITERS, eta=ETA, start_at_x0=False):
    _, x0, start0, y, fns, emb = _setup(flavor)
    combo = COMBOS[combo] if isinstance(combo, str) else combo
    n_evals = iters * (2 if dual else 1)
    rows = _rows(n_evals, seed=DI_SEED) if combo[4] else None
    table = _table(n_evals, combo[6])
    x0h = x0.cpu().numpy()
    x = np.clip((x0 if start_at_x0 else start0).cpu().numpy() + F(0), F(-1), F(1))
    m, v, v_mlm = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    text = [None]
    for i in range(iters):
        if vl:
            def grad_at(d, first):
                g, t = _grad_vl(fns["vl"], d, list(y["feat"]), flavor, emb, first)
                if first:
                    text[0] = t
                return g
            x, m, v = _host_eval(x, m, v, combo, table[i], None if rows is None else rows[i], grad_at, x0h, i, eta=eta)
        elif not dual:
            x, m, v = _host_eval(x, m, v, combo, table[i], None if rows is None else rows[i],
                                 lambda d, first: _grad(fns["feat"], d, list(y["feat"]), 1, flavor), x0h, i, eta=eta)
        else:
            yd = y["dual"]
            if flavor == "albef":
                y_feat, y_mlm, extra = [yd[1], yd[2]], [yd[0]], dict(bkp=fns["feat"], bkp_y=[yd[1], yd[2]])
            else:
                y_feat, y_mlm, extra = list(yd), list(yd), {}
            x, m, v = _host_eval(x, m, v, combo, table[2 * i], None if rows is None else rows[2 * i],
                                 lambda d, first: _grad(fns["feat"], d, y_feat, 1, flavor), None, 2 * i, eta=eta)
            x, m, v_mlm = _host_eval(x, m, v_mlm, combo, table[2 * i + 1], None if rows is None else rows[2 * i + 1],
                                     lambda d, first: _grad(fns["mlm"], d, y_mlm, 0, flavor, **extra), x0h, 2 * i + 1,
                                     eta=eta)
    return x, m, text[0]


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("dual", [False, True])
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_pgd_with_admix_equals_the_host_restatement_bitwise(flavor, dual, combo):
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
    # mixing changes the trajectory: the loop without it ends elsewhere
    fn, start, kw = _pgd_args(flavor, dual)
    keys = _keys(combo)
    keys.update(admix_images=None)
    plain, _ = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, **keys, **kw)
    assert float((plain != adv).float().mean()) > 0.001


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("combo", sorted(COMBOS))
def test_pgd_vl_with_admix_equals_the_host_restatement_and_returns_the_first_mixed_copys_text_gradient(flavor, combo):
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
    assert torch.equal(text_grad, ops.gather_rows(want_text, [0, 2]))           # the last iteration's, from leaf (0, 0)


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_momentum_iterative_method_with_admix(flavor):
    """Admix-TI-DIM with momentum, the paper's own best line, through the drop-in binding: it starts at x itself."""
    from vqattack_amd import dropin
    _, x0, _, y, fns, _ = _setup(flavor)
    combo = (2, False, 1.0, KERNLEN, True, None, 3)
    want_x, want_m, _ = _host_loop(flavor, False, combo, start_at_x0=True)
    m_dev = torch.zeros_like(x0)
    bound = dropin.load(flavor).momentum_iterative_method.momentum_iterative_method
    keys = _keys(combo)
    del keys["decay_factor"], keys["nesterov"]
    adv, losses = bound(fns["feat"], x0, EPS, EPS_ITER, ITERS, np.inf, y=list(y["feat"]), momentum=m_dev, **keys, **CLIP)
    assert len(losses) == ITERS
    _assert_bits(adv, want_x, "adv")
    _assert_bits(m_dev, want_m, "momentum")


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("copies", [None, 2], ids=["admix", "admix_si"])
def test_fast_gradient_method_and_vl_with_admix(flavor, copies):
    import vqattack_amd
    _, x0, start, y, fns, emb = _setup(flavor)
    x = np.clip(start.cpu().numpy() + F(0), F(-1), F(1))
    combo = (copies, False, None, None, False, None, 3)
    keys = lambda: dict(si_copies=copies, admix_images=3, admix_eta=ETA, admix_rng=np.random.RandomState(AX_SEED))  # noqa: E731
    prow = _table(1, 3)[0]
    seen = []
    want, _, _ = _host_eval(x, None, None, combo, prow, None, lambda d, first: _grad(fns["feat"], d, list(y["feat"]), 1, flavor),
                            None, 0, eps_iter=EPS, seen_out=seen)
    xin = _dev(x)
    adv, loss = vqattack_amd.fast_gradient_method(fns["feat"], xin, EPS, np.inf, x0, y=list(y["feat"]), ls=1,
                                                  flavor=flavor, **keys(), **CLIP)
    _assert_bits(adv, want, "adv")
    assert torch.equal(xin, _dev(x))
    # the reported loss is that of the first mixed copy
    _, loss_first = vqattack_amd.fast_gradient_method(fns["feat"], _dev(seen[0]), EPS, np.inf, x0, y=list(y["feat"]), ls=1,
                                                      flavor=flavor, **CLIP)
    assert float(loss) == float(loss_first)
    want, _, _ = _host_eval(x, None, None, combo, prow, None,
                            lambda d, first: _grad_vl(fns["vl"], d, list(y["feat"]), flavor, emb, first)[0], None, 0,
                            eps_iter=EPS)
    xs = [xin, emb.clone()]
    adv, text_grad = vqattack_amd.fast_gradient_method_vl(fns["vl"], xs, EPS, np.inf, x0, y=list(y["feat"]), ls=1,
                                                          text_emb_pick=[0, 2], flavor=flavor, **keys(), **CLIP)
    _assert_bits(adv, want, "adv (vl)")
    assert text_grad.shape[1] == 2 and xs[0].requires_grad and xs[0].grad is not None


@pytest.mark.parametrize("decay,nesterov", [(None, False), (DECAY, True)], ids=["admix", "admix_mi_ni"])
def test_l2_loop_with_admix_equals_the_combination_in_front_of_the_existing_ops(decay, nesterov):
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, _ = _setup("albef")
    eps, eps_iter = 1.0, 0.4
    s = ops.si_scales(2)
    w = ops.admix_weights(s, 3)
    table = ops.admix_partners(_table(ITERS, 3), BATCH, DEV)
    x = ops.linf_init(start, None, float("inf"), -1, 1)
    m = torch.zeros_like(start)
    for it in range(ITERS):
        gsum = None
        for j in range(3):                                                      # (all checked bitwise in the kernel tests)
            seen = ops.admix_copies(x, table[it, j], s, ETA, m=m if nesterov else None,
                                    lookahead=eps_iter * decay if nesterov else 0.0)
            grads = [_grad(fns["feat"], seen[i], list(y["feat"]), 1, "albef") for i in range(2)]
            gsum = ops.si_combine(grads, w) if j == 0 else ops.admix_accumulate(grads, w, gsum)
        g = gsum
        if decay is not None:
            g = ops.momentum_accumulate(g, m, decay)
        mid = ops.l2_fgm(x, g, eps_iter, -1, 1, check_range=False)
        x = ops.l2_project(mid, x0, eps, -1, 1)
    m_dev = torch.zeros_like(start)
    kw = dict(y=list(y["feat"]), ori_x=x0, time=None, ls=1, flavor="albef", decay_factor=decay, momentum=m_dev, **CLIP)
    adv, _ = vqattack_amd.projected_gradient_descent(fns["feat"], start, eps, eps_iter, ITERS, 2, si_copies=2,
                                                     nesterov=nesterov, admix_images=3, admix_eta=ETA,
                                                     admix_rng=np.random.RandomState(AX_SEED), **kw)
    assert torch.equal(adv, x) and torch.equal(m_dev, m)
    assert float((adv - x0).flatten(1).norm(dim=1).max()) <= eps * (1 + 1e-5)
    plain, _ = vqattack_amd.projected_gradient_descent(fns["feat"], start, eps, eps_iter, ITERS, 2, si_copies=2,
                                                       nesterov=nesterov, **kw)
    assert not torch.equal(plain, adv)


@pytest.mark.parametrize("dual", [False, True])
def test_one_mixed_image_with_eta_zero_ends_where_plain_si_ends(dual):
    """``admix_images=1, admix_eta=0``: the copies differ from SI's only through ``t + 0 * x'``, which is ``t`` for finite
    data (a -0 would become +0); every launch behind the model is SI's."""
    import vqattack_amd
    res = {}
    for images in (None, 1):
        fn, start, kw = _pgd_args("albef", dual)
        m = torch.zeros_like(start)
        adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, si_copies=3,
                                                              decay_factor=DECAY, momentum=m, admix_images=images,
                                                              admix_eta=0.0, admix_rng=np.random.RandomState(1), **kw)
        res[images] = (adv, losses, m)
    assert torch.equal(res[1][0], res[None][0]) and res[1][1] == res[None][1] and torch.equal(res[1][2], res[None][2])


@pytest.mark.parametrize("dual", [False, True])
def test_without_the_keys_nothing_changes(dual, monkeypatch):
    """``admix_images=None``: the call without the keys, none of the new launches and no draw, and today's chain from the
    existing kernels alone."""
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, _ = _setup("albef")

    def never(*a, **k):
        raise AssertionError("the default path must not launch an Admix kernel or draw a partner")
    for name in ("admix_copies", "admix_accumulate", "linf_admix_step", "admix_draw", "admix_partners"):
        monkeypatch.setattr(ops, name, never)
    fn, start, kw = _pgd_args("albef", dual)
    adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, admix_images=None,
                                                          admix_eta=0.5, admix_rng=np.random.RandomState(0), **kw)
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
    # SI alone is today's too: weights and launches (tests/test_admix_host.py pins the launches against the recorded ones)
    fn, start, kw = _pgd_args("albef", dual)
    si, _ = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, si_copies=3, **kw)
    assert not torch.equal(si, adv)


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("combo", ["admix_si", "admix_mi_ni", "admix_di_ti_mi", "admix_vt"])
def test_graph_replay_with_admix_equals_eager_bitwise_with_a_fresh_partner_row_per_replay(flavor, combo):
    import vqattack_amd
    res = []
    for graph in (False, True):
        fn, start, kw = _pgd_args(flavor, False)
        m = torch.zeros_like(start)
        adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, graph=graph,
                                                              momentum=m, **_keys(combo), **kw)
        res.append((adv, m, losses))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    want_x, want_m, _ = _host_loop(flavor, False, combo)          # which walks a fresh row of the table per iteration
    _assert_bits(res[1][0], want_x, "adv")
    table = _table(ITERS, COMBOS[combo][6])
    assert len({table[i].tobytes() for i in range(ITERS)}) == ITERS


def test_a_closure_is_called_once_per_copy_in_group_major_ascending_order():
    import vqattack_amd
    _, x0, start, y, fns, _ = _setup("albef")
    seen = []

    def spy(x):
        seen.append(x.detach().clone())
        return fns["feat"](x)
    vqattack_amd.projected_gradient_descent(spy, start, EPS, EPS_ITER, 2, np.inf, y=list(y["feat"]), ori_x=x0, time=None,
                                            ls=1, flavor="albef", si_copies=[1.0, 0.5, 0.25], admix_images=2, admix_eta=ETA,
                                            admix_rng=np.random.RandomState(AX_SEED), **CLIP)
    assert len(seen) == 2 * 3 * 2                                               # m1 * m2 calls per evaluation
    first = torch.clamp(start, -1, 1)
    table = _table(2, 2)
    for j in range(2):
        mixed = first + ETA * first[torch.from_numpy(table[0, j]).to(DEV)]
        for i in range(3):
            assert torch.equal(seen[3 * j + i], mixed * 2.0 ** -i), (j, i)


def test_a_batch_of_one_is_refused_before_any_launch():
    import vqattack_amd
    _, x0, start, y, fns, _ = _setup("albef")

    def never(x):
        raise AssertionError("the model must not run")
    with pytest.raises(ValueError, match="admix_images needs a batch"):
        vqattack_amd.projected_gradient_descent(never, start[:1], EPS, EPS_ITER, 2, np.inf, y=list(y["feat"]),
                                                ori_x=x0[:1], time=None, ls=1, flavor="albef", admix_images=3, **CLIP)


# ------------------------------------------------------------------------------------------------ batched driver
@pytest.mark.parametrize("flavor", ["vlmo", "albef"])
def test_attack_batch_with_the_keys_equals_the_operator_calls(flavor):
    """An image-only batch of two through ``attack_batch`` with the Admix keys: it is the operator call with the keys and a
    ``RandomState(admix_seed)`` on the batch; two calls of one driver draw the same partners."""
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    model, adapters_cls, cfg, ids, masks, img, eta = _driver_inputs(flavor)
    none = torch.zeros_like(ids, dtype=torch.bool)
    conf = AttackConfig(budget=4, si_copies=2, decay_factor=1.0, admix_images=3, admix_eta=0.25, admix_seed=AX_SEED)
    atk = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(), conf)
    both = atk.attack_batch(img, ids, masks, none, init_eta=eta)
    again = atk.attack_batch(img, ids, masks, none, init_eta=eta)
    assert torch.equal(both.adv_images, again.adv_images)
    off = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(),
                          AttackConfig(budget=4, si_copies=2, decay_factor=1.0))
    plain = off.attack_batch(img, ids, masks, none, init_eta=eta)
    assert float((plain.adv_images != both.adv_images).float().mean()) > 0.01
    assert float((both.adv_images - img).abs().max()) <= np.float32(0.125) + 1e-6
    a = atk.adapters
    a.set_text(ids, masks)
    targets = a.gen_ori_feats(img)
    with torch.enable_grad():
        adv, losses = atk.pgd(a.pgd_attack, img, conf.eps, conf.eps_iter, 4, np.inf, y=atk._y_feature(targets), ls=1,
                              clip_min=conf.clip_min, clip_max=conf.clip_max, time=0, ori_x=img, sanity_checks=False,
                              init_eta=eta, decay_factor=1.0, si_copies=2, admix_images=3, admix_eta=0.25,
                              admix_rng=np.random.RandomState(AX_SEED))
    assert torch.equal(adv, both.adv_images) and losses == both.loss_lists[0]
    with pytest.raises(ValueError, match="admix_images needs a batch"):
        atk.attack_batch(img[:1], ids[:1], masks[:1], none[:1], init_eta=eta[:1])
