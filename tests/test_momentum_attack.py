"""Momentum (MI-FGSM) through the attack operators and the batched drivers, on the MI355X.

The comparison is a loop written here: it takes every gradient from the SAME ``model_fn`` on the device (through the
operators' own loss code, which momentum does not touch), applies the numpy fp32 chain of the issue on the host -- fed
``ops.sumabs_per_sample`` of that gradient -- and the L-inf update in numpy, and feeds the result back.  Identical inputs
give identical gradients, so the adversarial image and the final momentum must be BIT-identical to the product's.
Toy white box on the device, batch 3, 32 x 32 images, 4 iterations; eps = 3 steps, so the projection acts.
"""
import numpy as np
import pytest
import torch

from tests.golden.cases import _labels, attack_inputs
from tests.test_momentum_kernels import _chain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS, EPS_ITER, ITERS, DECAY, BATCH = 0.03, 0.01, 4, 0.9, 3
CLIP = dict(clip_min=-1, clip_max=1)
_cache = {}


def _setup(flavor):
    """(toy, clean images, start point inside the eps-ball, y lists, closures) -- built once per flavor, never changed."""
    if flavor not in _cache:
        toy, x0, start, feats = attack_inputs(dict(flavor=flavor, op="pgd", batch=BATCH, eps=EPS), DEV)
        lab = _labels("2d", BATCH, toy.text_len, DEV)
        if flavor == "albef":
            fns = dict(feat=toy.albef_feats, vl=toy.albef_feats_vl, mlm=toy.mlm_logits)
            y = dict(feat=[feats[0], feats[1], None, None, None], dual=[lab, feats[0], feats[1]])
        else:
            fns = dict(feat=toy.vlmo_feats, vl=toy.vlmo_feats_vl, mlm=toy.mlm_logits)
            y = dict(feat=[feats[0], feats[1], feats[2]], dual=[lab, feats[1], feats[2]])
        emb = toy.embed_text(toy.text_ids.expand(BATCH, -1)).clone()
        _cache[flavor] = (toy, x0, start, y, fns, emb)
    return _cache[flavor]


def _grad(fn, x, y, ls, flavor, emb=None, **extra):
    """d loss / d x from the same closure and the operators' own loss code, as the product's loop calls it."""
    from vqattack_amd import attacks
    slot = attacks._LossSlot(torch.zeros(1, device=DEV), 0)
    leaf = x.detach().requires_grad_(True)
    if emb is None:
        attacks._loss_and_grad(fn, [leaf], leaf, y, ls, flavor, False, slot, **extra)
    else:
        txt = emb.detach().requires_grad_(True)
        attacks._loss_and_grad(fn, [leaf, txt], [leaf, txt], y, ls, flavor, False, slot, vl=True)
    return leaf.grad.contiguous()


def _host_update(x, m, g_dev, x0, decay=DECAY):
    """numpy fp32: the momentum chain, then StepOp (x0 given) or FgmOp (x0 None) of csrc/common.hpp.  Returns (x, m)."""
    from vqattack_amd import ops
    f = np.float32
    m = _chain(g_dev.cpu().numpy(), m, ops.sumabs_per_sample(g_dev).cpu().numpy(), decay)
    a = np.clip(x + f(EPS_ITER) * np.sign(m), f(-1), f(1))
    if x0 is None:
        return a, m
    e = np.clip(a - x0, -f(EPS), f(EPS))
    out = np.clip(x0 + e, f(-1), f(1))
    assert out.dtype == np.float32 and m.dtype == np.float32
    return out, m


def _dev(a):
    return torch.from_numpy(a).to(DEV)


def _assert_bits(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    same = np.mean(got.view(np.int32) == want.view(np.int32))
    assert same == 1.0, (what, same, np.abs(got - want).max())


def _host_loop(flavor, dual, iters=ITERS, vl=False, start=None, m=None):
    _, x0, start0, y, fns, emb = _setup(flavor)
    x0h = x0.cpu().numpy()
    x = np.clip((start0 if start is None else start).cpu().numpy() + np.float32(0), np.float32(-1), np.float32(1))
    m = np.zeros_like(x) if m is None else m
    for _ in range(iters):
        if vl:
            x, m = _host_update(x, m, _grad(fns["vl"], _dev(x), list(y["feat"]), 1, flavor, emb=emb), x0h)
        elif not dual:
            x, m = _host_update(x, m, _grad(fns["feat"], _dev(x), list(y["feat"]), 1, flavor), x0h)
        else:
            yd = y["dual"]
            if flavor == "albef":
                y_feat, y_mlm, extra = [yd[1], yd[2]], [yd[0]], dict(bkp=fns["feat"], bkp_y=[yd[1], yd[2]])
            else:
                y_feat, y_mlm, extra = list(yd), list(yd), {}
            x, m = _host_update(x, m, _grad(fns["feat"], _dev(x), y_feat, 1, flavor), None)        # no projection
            x, m = _host_update(x, m, _grad(fns["mlm"], _dev(x), y_mlm, 0, flavor, **extra), x0h)
    return x, m


# ------------------------------------------------------------------------------------------------ operators
@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
@pytest.mark.parametrize("dual", [False, True])
def test_pgd_with_momentum_equals_the_host_chain_bitwise(flavor, dual):
    import vqattack_amd
    _, x0, start, y, fns, _ = _setup(flavor)
    want_x, want_m = _host_loop(flavor, dual)
    m = torch.zeros_like(start)
    before = start.clone()
    fn, yy, ls = ([fns["feat"], fns["mlm"]], list(y["dual"]), 0) if dual else (fns["feat"], list(y["feat"]), 1)
    adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, y=yy, ori_x=x0,
                                                          time=None, ls=ls, flavor=flavor, decay_factor=DECAY,
                                                          momentum=m, **CLIP)
    assert len(losses) == ITERS * (2 if dual else 1) and torch.equal(start, before)
    _assert_bits(adv, want_x, "adv")
    _assert_bits(m, want_m, "momentum")
    assert float((adv - x0).abs().max()) <= EPS + 1e-6
    # momentum changes the trajectory: the plain loop ends elsewhere
    plain, _ = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, y=yy, ori_x=x0, time=None,
                                                       ls=ls, flavor=flavor, **CLIP)
    assert float((plain != adv).float().mean()) > 0.001


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_pgd_vl_with_momentum_equals_the_host_chain_bitwise(flavor):
    import vqattack_amd
    _, x0, start, y, fns, emb = _setup(flavor)
    want_x, want_m = _host_loop(flavor, False, vl=True)
    m = torch.zeros_like(start)
    adv, text_grad = vqattack_amd.projected_gradient_descent_vl(fns["vl"], [start, emb.clone()], EPS, EPS_ITER, ITERS,
                                                                np.inf, y=list(y["feat"]), ori_x=x0, time=None, ls=1,
                                                                attack_mask=[0, 2], flavor=flavor, decay_factor=DECAY,
                                                                momentum=m, **CLIP)
    _assert_bits(adv, want_x, "adv")
    _assert_bits(m, want_m, "momentum")
    assert text_grad.shape[1] == 2


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_momentum_iterative_method_equals_the_host_chain_bitwise(flavor):
    """Starts at x itself with the eps-ball around it (no random start, ``ori_x`` defaults to ``x``), decay 1."""
    import vqattack_amd
    from vqattack_amd import dropin
    _, x0, _, y, fns, _ = _setup(flavor)
    x, m = np.clip(x0.cpu().numpy() + np.float32(0), np.float32(-1), np.float32(1)), np.zeros(x0.shape, np.float32)
    for _ in range(ITERS):
        x, m = _host_update(x, m, _grad(fns["feat"], _dev(x), list(y["feat"]), 1, flavor), x0.cpu().numpy(), decay=1.0)
    m_dev = torch.zeros_like(x0)
    adv, losses = vqattack_amd.momentum_iterative_method(fns["feat"], x0, EPS, EPS_ITER, ITERS, np.inf, y=list(y["feat"]),
                                                         flavor=flavor, momentum=m_dev, **CLIP)
    assert len(losses) == ITERS
    _assert_bits(adv, x, "adv")
    _assert_bits(m_dev, m, "momentum")
    bound = dropin.load(flavor).momentum_iterative_method.momentum_iterative_method          # the drop-in binding
    adv2, losses2 = bound(fns["feat"], x0, EPS, EPS_ITER, ITERS, np.inf, y=list(y["feat"]), **CLIP)
    assert torch.equal(adv, adv2) and losses == losses2                                       # momentum=None: zeros


def test_l2_loop_with_momentum_equals_the_composition_of_the_existing_ops():
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, _ = _setup("albef")
    eps, eps_iter = 1.0, 0.4
    x = ops.linf_init(start, None, float("inf"), -1, 1)
    m = torch.zeros_like(start)
    for _ in range(ITERS):
        g = _grad(fns["feat"], x, list(y["feat"]), 1, "albef")
        ops.momentum_accumulate(g, m, DECAY)                       # the new kernel, checked bitwise in the kernel tests
        mid = ops.l2_fgm(x, m, eps_iter, -1, 1, check_range=False)
        x = ops.l2_project(mid, x0, eps, -1, 1)
    m_dev = torch.zeros_like(start)
    adv, _ = vqattack_amd.projected_gradient_descent(fns["feat"], start, eps, eps_iter, ITERS, 2, y=list(y["feat"]),
                                                     ori_x=x0, time=None, ls=1, flavor="albef", decay_factor=DECAY,
                                                     momentum=m_dev, **CLIP)
    assert torch.equal(adv, x) and torch.equal(m_dev, m)
    assert float((adv - x0).flatten(1).norm(dim=1).max()) <= eps * (1 + 1e-5)
    plain, _ = vqattack_amd.projected_gradient_descent(fns["feat"], start, eps, eps_iter, ITERS, 2, y=list(y["feat"]),
                                                       ori_x=x0, time=None, ls=1, flavor="albef", **CLIP)
    assert not torch.equal(plain, adv)


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_graph_replay_with_momentum_equals_eager_bitwise(flavor):
    import vqattack_amd
    _, x0, start, y, fns, _ = _setup(flavor)
    res = []
    for graph in (False, True):
        m = torch.zeros_like(start)
        adv, losses = vqattack_amd.projected_gradient_descent(fns["feat"], start, EPS, EPS_ITER, ITERS, np.inf,
                                                              y=list(y["feat"]), ori_x=x0, time=None, ls=1, flavor=flavor,
                                                              graph=graph, decay_factor=DECAY, momentum=m, **CLIP)
        res.append((adv, m, losses))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]
    want_x, want_m = _host_loop(flavor, False)
    _assert_bits(res[1][0], want_x, "adv")
    _assert_bits(res[1][1], want_m, "momentum")


def test_two_calls_carrying_the_momentum_equal_one_call():
    import vqattack_amd
    _, x0, start, y, fns, _ = _setup("albef")
    kw = dict(y=list(y["feat"]), ori_x=x0, time=None, ls=1, flavor="albef", decay_factor=DECAY, **CLIP)
    m_one = torch.zeros_like(start)
    one, loss_one = vqattack_amd.projected_gradient_descent(fns["feat"], start, EPS, EPS_ITER, 4, np.inf, momentum=m_one,
                                                            **kw)
    m_two = torch.zeros_like(start)
    half, loss_a = vqattack_amd.projected_gradient_descent(fns["feat"], start, EPS, EPS_ITER, 2, np.inf, momentum=m_two,
                                                           **kw)
    two, loss_b = vqattack_amd.projected_gradient_descent(fns["feat"], half, EPS, EPS_ITER, 2, np.inf, momentum=m_two,
                                                          **kw)
    assert torch.equal(one, two) and torch.equal(m_one, m_two) and loss_one == loss_a + loss_b
    fresh, _ = vqattack_amd.projected_gradient_descent(fns["feat"], half, EPS, EPS_ITER, 2, np.inf, **kw)   # zeros again
    assert not torch.equal(fresh, two)


@pytest.mark.parametrize("dual", [False, True])
def test_without_a_decay_factor_nothing_changes(dual):
    """``decay_factor=None``: today's output, and a passed momentum tensor is left untouched."""
    import vqattack_amd
    from vqattack_amd import ops
    _, x0, start, y, fns, _ = _setup("albef")
    fn, yy, ls = ([fns["feat"], fns["mlm"]], list(y["dual"]), 0) if dual else (fns["feat"], list(y["feat"]), 1)
    kw = dict(y=yy, ori_x=x0, time=None, ls=ls, flavor="albef", **CLIP)
    m = torch.full_like(start, 0.25)
    adv, losses = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, decay_factor=None,
                                                          momentum=m, **kw)
    assert bool((m == 0.25).all())
    # today's chain, from the existing kernels alone
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
    again, losses2 = vqattack_amd.projected_gradient_descent(fn, start, EPS, EPS_ITER, ITERS, np.inf, **kw)
    assert torch.equal(adv, again) and losses == losses2


def test_momentum_argument_is_checked():
    import vqattack_amd
    _, x0, start, y, fns, _ = _setup("albef")
    kw = dict(y=list(y["feat"]), ori_x=x0, time=None, ls=1, flavor="albef", decay_factor=1.0, **CLIP)
    with pytest.raises(ValueError):
        vqattack_amd.projected_gradient_descent(fns["feat"], start, EPS, EPS_ITER, 1, np.inf,
                                                momentum=torch.zeros(BATCH, 3, 8, 8, device=DEV), **kw)
    with pytest.raises(TypeError):
        vqattack_amd.projected_gradient_descent(fns["feat"], start, EPS, EPS_ITER, 1, np.inf,
                                                momentum=torch.zeros_like(start, dtype=torch.float64), **kw)


# ------------------------------------------------------------------------------------------------ batched drivers
def _tiny(flavor, seed=6):
    if flavor == "vlmo":
        from vqattack_amd.whitebox.vlmo import FrozenVlmo, VlmoAttackAdapters, vlmo_tiny
        cfg = vlmo_tiny()
        return FrozenVlmo(cfg, seed=seed).to(DEV), VlmoAttackAdapters, cfg
    from vqattack_amd.whitebox.albef import AlbefAttackAdapters, FrozenAlbef, albef_tiny
    cfg = albef_tiny(mlm_probability=0.0)
    return FrozenAlbef(cfg, seed=seed).to(DEV), AlbefAttackAdapters, cfg


IDS = torch.tensor([[101, 2054, 3609, 2003, 102, 0, 0, 0], [101, 2129, 2116, 6077, 2024, 102, 0, 0]])


def test_runner_resets_the_momentum_per_attack_and_graph_replay_equals_eager():
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    model, adapters_cls, cfg = _tiny("vlmo")
    ids = IDS.to(DEV)
    masks = (ids != 0).long()
    g = torch.Generator().manual_seed(8)
    img = torch.empty(2, 3, cfg.image_size, cfg.image_size).uniform_(-1, 1, generator=g).to(DEV)
    eta = torch.empty(img.shape).uniform_(-0.125, 0.125, generator=g).to(DEV)
    none = torch.zeros_like(ids, dtype=torch.bool)
    outs = {}
    for key, kw in (("eager", dict(decay_factor=1.0)), ("graph", dict(decay_factor=1.0, use_graph=True)),
                    ("plain", dict())):
        atk = BatchedVQAttack(adapters_cls(model), "vlmo", model.embedding_tables(), AttackConfig(budget=9, **kw))
        outs[key] = atk.attack_batch(img, ids, masks, none, init_eta=eta)
        if key == "eager":
            second = atk.attack_batch(img, ids, masks, none, init_eta=eta)       # the buffer starts at zero again
            assert torch.equal(second.adv_images, outs[key].adv_images) and second.loss_lists == outs[key].loss_lists
    assert torch.equal(outs["eager"].adv_images, outs["graph"].adv_images)
    assert outs["eager"].loss_lists == outs["graph"].loss_lists
    assert float((outs["eager"].adv_images != outs["plain"].adv_images).float().mean()) > 0.01
    assert float((outs["eager"].adv_images - img).abs().max()) <= 0.125 + 1e-6


@pytest.mark.parametrize("flavor", ["vlmo", "albef"])
def test_attack_mixed_equals_attack_batch_with_momentum(flavor):
    """A same-schedule dual-loss batch through both drivers, as tests/test_attack_batched_parity.py compares them
    (identical token ids, >= 99.9 % of the pixels bit-identical); the momentum is carried through every PGD block and
    the probe step in one and through every global step in the other."""
    from vqattack_amd.attack import mlm_task, text_update
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    model, adapters_cls, cfg = _tiny(flavor, seed=3)
    g = torch.Generator().manual_seed(71)
    images = torch.empty(2, 3, cfg.image_size, cfg.image_size).uniform_(-1, 1, generator=g)
    eta = torch.empty_like(images).uniform_(-0.125, 0.125, generator=g)
    ids = IDS
    masks = (ids != 0).long()
    att = torch.zeros_like(ids, dtype=torch.bool)
    att[0, 1] = att[1, 2] = True                                   # one substitutable word each: blocks [4, 8] + 1 probe
    sim = text_update.BagOfEmbeddingsSimilarity(seed=5)
    max_len = cfg.max_text_len if flavor == "vlmo" else None
    tasks = []
    for s in range(2):
        body = [(int(t),) for t in ids[s].tolist() if t not in (0, 101, 102)]
        answer = (7301 + s,)
        correct = [[answer]] + ([[(7401,)]] if s else [])
        tasks.append(mlm_task.build_mlm_task([answer], correct, [True] + [False] * (len(correct) - 1),
                                             body[:2] + [answer], [], flavor, max_len=max_len))
    res = {}
    for decay in (1.0, None):
        attack = BatchedVQAttack(adapters_cls(model), flavor, model.embedding_tables(),
                                 AttackConfig(budget=12, sanity_checks=True, sim_threshold=0.3, decay_factor=decay),
                                 similarity_fn=sim)
        proposals = text_update.propose_candidates(attack.adapters.mlm_logits(ids.to(DEV), masks.to(DEV)), ids, att,
                                                   threshold=0)
        args = (images.to(DEV), ids.to(DEV), masks.to(DEV), att.to(DEV))
        mixed = attack.attack_mixed(*args, init_eta=eta.to(DEV), proposals=proposals, tasks=tasks)
        bucket = attack.attack_batch(*args, init_eta=eta.to(DEV), proposals=proposals, dual=True, tasks=tasks)
        assert mixed.gradient_steps == 2 * 13 and bucket.gradient_steps == 13
        assert torch.equal(mixed.adv_text_ids, bucket.adv_text_ids)
        assert (mixed.adv_images == bucket.adv_images).float().mean().item() >= 0.999
        res[decay] = bucket.adv_images
    assert float((res[1.0] != res[None]).float().mean()) > 0.01    # and the momentum acted
