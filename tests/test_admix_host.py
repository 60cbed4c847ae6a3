"""Admix (mixed-image copies): everything that needs no GPU -- validation, the partner draws, configuration, ABI, entry
points and, through the recorder of tests/golden/make_update_chain_golden.py, the launch sequences of a chain built with
``admix=``."""
import ctypes
import importlib.util
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import vqattack_amd
from tests.golden import make_update_chain_golden as gold
from vqattack_amd import _hip, attacks, dropin, ops
from vqattack_amd._hip import HipExtensionError
from vqattack_amd.attack import runner

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vqa_admix_copies", "vqa_admix_accumulate", "vqa_linf_admix_step")
ERR_NULL, ERR_SHAPE, ERR_ALIGN = -1, -2, -3
BAD = (dict(admix_images=0), dict(admix_images=9), dict(admix_images=True), dict(admix_images=2.0),
       dict(admix_images="3"), dict(admix_images=3, admix_eta=-0.1), dict(admix_images=3, admix_eta=float("nan")),
       dict(admix_images=3, admix_eta=float("inf")), dict(admix_images=3, admix_eta=True),
       dict(admix_images=3, admix_eta="0.2"))


# ------------------------------------------------------------------------------------------------ validation, host helpers
def test_validate_admix():
    assert attacks._validate_admix(None) is None
    assert attacks._validate_admix(None, -1.0, object()) is None          # off: the other two keys are ignored
    for n in range(1, 9):
        images, eta, rng = attacks._validate_admix(n)
        assert (images, eta) == (n, 0.2) and rng is np.random
    r = np.random.RandomState(3)
    assert attacks._validate_admix(np.int64(3), 0, r) == (3, 0.0, r)
    assert attacks._validate_admix(3, np.float32(0.5), np.random.default_rng(0))[1] == 0.5
    for bad in BAD:
        with pytest.raises(ValueError):
            attacks._validate_admix(**bad)
    for rng in (object(), 5, "np.random"):
        with pytest.raises(ValueError):
            attacks._validate_admix(3, 0.2, rng)
    assert ops.ADMIX_MAX_IMAGES == 8


def test_draw_follows_the_stated_rule_and_never_returns_the_sample_itself():
    t = ops.admix_draw(np.random.RandomState(11), 5, 2, 3)
    assert t.dtype == np.int32 and t.shape == (2, 3, 5)
    r = np.random.RandomState(11)                                        # the rule, restated: order evaluation, group, sample
    want = [[[(b + 1 + min(int(r.uniform() * 4), 3)) % 5 for b in range(5)] for _ in range(3)] for _ in range(2)]
    assert t.tolist() == want
    # RandomState(11): u = .180, .019, .463, .725, .420 -> k = 0, 0, 1, 2, 1 -> (b + 1 + k) mod 5
    assert t.tolist()[0][0] == [1, 2, 4, 1, 1]
    big = ops.admix_draw(np.random.RandomState(0), 4, 500, 1)            # 2000 draws at B = 4
    assert big.shape == (500, 1, 4)
    for b in range(4):
        assert set(big[:, 0, b].tolist()) == set(range(4)) - {b}

    class Top:                                                           # u at the top of [0, 1): k is clamped to B - 2
        def uniform(self):
            return float(np.nextafter(1.0, 0.0))
    assert ops.admix_draw(Top(), 3, 1, 1).tolist() == [[[2, 0, 1]]]
    assert ops.admix_draw(np.random.RandomState(0), 2, 3, 2).tolist() == [[[1, 0]] * 2] * 3
    assert ops.admix_draw(np.random.RandomState(0), 4, 0, 2).shape == (0, 2, 4)
    for bad in (lambda: ops.admix_draw(np.random, 1, 1, 1), lambda: ops.admix_draw(np.random, 0, 1, 1),
                lambda: ops.admix_draw(np.random, 4, -1, 1), lambda: ops.admix_draw(np.random, 4, 1, 0),
                lambda: ops.admix_draw(np.random, 4, 1, 9)):
        with pytest.raises(ValueError):
            bad()


def test_partners_rejects_entries_out_of_range_and_self_pointing():
    good = np.array([[[1, 2, 0], [2, 0, 1]]], dtype=np.int64)
    t = ops.admix_partners(good, 3, "cpu")
    assert t.dtype == torch.int32 and t.shape == (1, 2, 3) and t.is_contiguous() and t.tolist() == good.tolist()
    for i, j, v in ((0, 0, 3), (0, 1, -1), (0, 2, 2), (1, 0, 0), (1, 1, 1 << 40)):
        bad = good.copy()
        bad[0, i, j] = v
        with pytest.raises(ValueError):
            ops.admix_partners(bad, 3, "cpu")
    for bad in (good.astype(np.float32), good[..., :2], np.int32(1)):
        with pytest.raises(ValueError):
            ops.admix_partners(bad, 3, "cpu")


def test_weights_are_the_stated_float32_values():
    for n in range(1, 9):
        for images in (1, 3, 8):
            s = ops.si_scales(n)
            w = ops.admix_weights(s, images)
            assert w.dtype == np.float32 and w.shape == (n,)
            assert [float(v) for v in w] == [float(np.float32(s[i]) / np.float32(n * images)) for i in range(n)]
        assert np.array_equal(ops.admix_weights(s, 1), ops.si_weights(s))
    w = ops.admix_weights(ops.si_scales(5), 3)
    assert w[0] == np.float32(1) / np.float32(15) and w[4] == np.float32(0.0625) / np.float32(15)
    for bad in (0, 9, True, 2.0):
        with pytest.raises(ValueError):
            ops.admix_weights([1.0], bad)
    with pytest.raises(ValueError):
        ops.admix_weights([], 3)


def test_ops_refuse_cpu_tensors_and_bad_lists():
    g = torch.zeros(2, 3, 8, 8)
    row = torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(HipExtensionError):
        ops.admix_copies(g, row, [1.0, 0.5], 0.2)
    with pytest.raises(HipExtensionError):
        ops.admix_accumulate([g, g], [0.5, 0.25], g)
    with pytest.raises(HipExtensionError):
        ops.linf_admix_step(g, g, [g], g, [1.0], 0.01, 0.1, -1.0, 1.0)
    with pytest.raises(TypeError):
        ops.admix_accumulate(g, [1.0], g)
    with pytest.raises(ValueError):
        ops.admix_copies(g, row, [], 0.2)


# ------------------------------------------------------------------------------------------------ operators, drop-ins, driver
def _unreachable(_):
    raise AssertionError("model_fn must not run: the arguments are refused first")


def _run(call, x, norm=np.inf, **kw):
    y = [x, x]
    if call == "pgd":
        return vqattack_amd.projected_gradient_descent(_unreachable, x, 0.1, 0.01, 2, norm, y=y, ori_x=x, ls=1, **kw)
    if call == "pgd_vl":
        return vqattack_amd.projected_gradient_descent_vl(_unreachable, [x, x], 0.1, 0.01, 2, norm, y=y, ori_x=x, ls=1, **kw)
    if call == "mim":
        return vqattack_amd.momentum_iterative_method(_unreachable, x, 0.1, 0.01, 2, norm, y=y, **kw)
    if call == "fgm":
        return vqattack_amd.fast_gradient_method(_unreachable, x, 0.1, norm, x, y=y, ls=1, **kw)
    return vqattack_amd.fast_gradient_method_vl(_unreachable, [x, x], 0.1, norm, x, y=y, ls=1, **kw)


@pytest.mark.parametrize("call", ["pgd", "pgd_vl", "mim", "fgm", "fgm_vl"])
def test_operators_validate_the_admix_keys_and_the_batch_before_any_tensor(call):
    x = torch.zeros(2, 3, 4, 4)                                  # a CPU tensor: refused, but only after the arguments
    for bad in BAD + (dict(admix_images=3, admix_rng=object()),):
        with pytest.raises(ValueError):
            _run(call, x, **bad)
        with pytest.raises(ValueError):
            _run(call, x, norm=2, **bad)
    one = torch.zeros(1, 3, 4, 4)                                # nobody to mix with: refused before the CPU tensor is
    with pytest.raises(ValueError, match="admix_images needs a batch"):
        _run(call, one, admix_images=3)
    with pytest.raises(HipExtensionError):
        _run(call, one)                                          # without the key a batch of one is fine
    for kw in (dict(), dict(admix_images=None, admix_eta=-1.0), dict(admix_images=1), dict(admix_images=8, admix_eta=0),
               dict(admix_images=3, si_copies=5, admix_rng=np.random.RandomState(0)),
               dict(admix_images=3, ti_kernel=7, diversity_prob=0.5)):
        with pytest.raises(HipExtensionError):                   # fine: the CPU tensor is what is refused
            _run(call, x, **kw)


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_the_keywords_reach_the_dropin_bindings(flavor):
    ns = dropin.load(flavor)
    x = torch.zeros(2, 3, 4, 4)
    for bound in (ns.projected_gradient_descent.projected_gradient_descent,
                  ns.momentum_iterative_method.momentum_iterative_method):
        with pytest.raises(ValueError):
            bound(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x, ls=1, admix_images=9)
        with pytest.raises(HipExtensionError):
            bound(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x, ls=1, admix_images=3, admix_eta=0.3,
                  admix_rng=np.random.RandomState(1))
    with pytest.raises(ValueError):
        ns.projected_gradient_descent_vl.projected_gradient_descent(_unreachable, [x, x], 0.1, 0.01, 2, np.inf, y=[x, x],
                                                                    ori_x=x, ls=1, admix_images=0)
    with pytest.raises(ValueError):
        ns.fast_gradient_method.fast_gradient_method(_unreachable, x, 0.1, np.inf, x, y=[x, x], ls=1, admix_images=0)
    with pytest.raises(ValueError):
        ns.fast_gradient_method_vl.fast_gradient_method(_unreachable, [x, x], 0.1, np.inf, x, y=[x, x], ls=1,
                                                        admix_images=3, admix_eta=-1)


def test_attack_config_takes_the_fields_and_the_mixed_driver_refuses_them():
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    c = AttackConfig()
    assert c.admix_images is None and c.admix_eta == 0.2 and c.admix_seed is None
    c = AttackConfig(admix_images=3, admix_eta=0.3, admix_seed=11, si_copies=5, decay_factor=1.0, ti_kernel=7)
    assert (c.admix_images, c.admix_eta, c.admix_seed) == (3, 0.3, 11)
    kw = c.transfer_kwargs()
    assert kw["admix_images"] == 3 and kw["admix_eta"] == 0.3 and "admix_seed" not in kw and "di_seed" not in kw
    assert set(c.stage_kwargs()) == set(kw) - {"admix_images", "admix_eta"}
    for bad in BAD + (dict(admix_images=3, admix_seed=-1), dict(admix_images=3, admix_seed=1 << 32),
                      dict(admix_images=3, admix_seed=True), dict(admix_images=3, admix_seed=1.5)):
        with pytest.raises(ValueError):
            AttackConfig(**bad)
    with pytest.raises(ValueError, match="admix_images"):
        AttackConfig(admix_images=2, patch_layout=True)
    atk = object.__new__(BatchedVQAttack)                            # no model needed: the refusal comes first
    atk.cfg, atk.adapters = AttackConfig(admix_images=2), object()
    with pytest.raises(ValueError, match="admix_images"):
        atk.attack_mixed(None, None, None, None)
    # one RandomState per attack call, from the seed; a caller's generator instead when one is set
    atk.di_rng = atk.admix_rng = None
    atk.cfg = AttackConfig(admix_images=2, admix_seed=5)
    atk._start_di()
    assert atk._di_draws is None and atk._admix_draws.uniform() == np.random.RandomState(5).uniform()
    atk.admix_rng = mine = np.random.RandomState(1)
    atk._start_di()
    assert atk._admix_draws is mine
    atk.cfg = AttackConfig()
    atk._start_di()
    assert atk._admix_draws is None


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_and_library_exports_the_three_symbols():
    text = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    assert _hip.lib().vqa_abi_version() == 4                   # additive exports: the version stays
    assert _hip.lib().vqa_si_max_copies() == 8


def test_entry_points_validate_before_the_first_launch():
    """Every return code of the header's list, through the library on a machine without a GPU."""
    lib = _hip.lib()
    buf = (ctypes.c_float * 1024)()
    base = ctypes.cast(buf, ctypes.c_void_p).value
    at = lambda floats: ctypes.c_void_p(base + 4 * floats)      # noqa: E731
    x, m, x0, acc, out = at(0), at(16), at(32), at(48), at(512)  # batch 2 x per 8 = 16 floats each; out: 8 copies
    g = [at(64 + 16 * i) for i in range(9)]
    row = at(960)
    scales = (ctypes.c_float * 8)(*[1.0] * 8)
    off = ctypes.c_void_p(base + 4 * 900 + 2)                    # not 4-byte aligned, and apart from all the others
    null = None

    def ptrs(entries):
        return (ctypes.c_void_p * len(entries))(*[e if e is None else e.value for e in entries])

    def copies(x=x, m=null, row=row, out=out, batch=2, per=8, stride=16, sc=scales, c=3):
        return lib.vqa_admix_copies(x, m, row, out, batch, per, stride, sc, c, 0.2, 0.5, null)

    def accum(acc=acc, gl=g[:3], c=3, n=16, raw=False):
        return lib.vqa_admix_accumulate(acc, gl if raw else ptrs(gl), scales, c, n, null)

    def step(x=x, acc=acc, gl=g[:3], c=3, x0=x0, out=out, n=16, mode=1, flag=null):
        return lib.vqa_linf_admix_step(x, acc, ptrs(gl), scales, c, x0, out, n, 0.01, 0.1, -1.0, 1.0, mode, flag, null)

    for mm in (null, m):                                         # with and without the look-ahead
        assert copies(x=null, m=mm) == ERR_NULL and copies(out=null, m=mm) == ERR_NULL
        assert copies(row=null, m=mm) == ERR_NULL and copies(sc=null, m=mm) == ERR_NULL
        assert copies(c=0, m=mm) == ERR_SHAPE and copies(c=9, m=mm) == ERR_SHAPE
        assert copies(batch=-1, m=mm) == ERR_SHAPE and copies(batch=65536, per=0, stride=0, m=mm) == ERR_SHAPE
        assert copies(stride=15, m=mm) == ERR_SHAPE              # copy_stride < batch * per
        assert copies(out=x, m=mm) == ERR_SHAPE                  # out overlaps x
        assert copies(x=at(512 + 40), m=mm) == ERR_SHAPE         # x inside the third copy
        assert copies(row=at(512 + 20), m=mm) == ERR_SHAPE       # the partner row inside the second copy
        assert copies(x=off, m=mm) == ERR_ALIGN and copies(out=off, m=mm) == ERR_ALIGN and copies(row=off, m=mm) == ERR_ALIGN
        assert copies(per=0, stride=0, m=mm) == 0 and copies(batch=0, m=mm) == 0       # empty: no launch
    assert copies(m=at(512 + 16)) == ERR_SHAPE and copies(m=off) == ERR_ALIGN

    assert accum(acc=null) == ERR_NULL and accum(gl=null, raw=True) == ERR_NULL
    assert accum(gl=[g[0], null, g[2]]) == ERR_NULL              # a NULL entry of the pointer list
    assert accum(c=0) == ERR_SHAPE and accum(c=9, gl=g) == ERR_SHAPE
    assert accum(acc=g[1]) == ERR_SHAPE and accum(acc=at(64 + 16 * 2 + 8)) == ERR_SHAPE     # acc aliases / overlaps a gradient
    assert accum(gl=[g[0], off, g[2]]) == ERR_ALIGN and accum(acc=off) == ERR_ALIGN
    assert accum(n=0) == 0 and accum(c=8, gl=g[:8], n=0) == 0

    for z in (x0, null):                                         # both forms of the fused step
        assert step(x=null, x0=z) == ERR_NULL and step(out=null, x0=z) == ERR_NULL and step(acc=null, x0=z) == ERR_NULL
        assert step(gl=[g[0], null, g[2]], x0=z) == ERR_NULL
        assert step(mode=3, x0=z) == ERR_NULL                    # a range check needs a flag
        assert step(c=0, x0=z) == ERR_SHAPE and step(c=9, gl=g, x0=z) == ERR_SHAPE
        assert step(out=g[0], x0=z) == ERR_SHAPE and step(out=acc, x0=z) == ERR_SHAPE
        assert step(out=at(8), x0=z) == ERR_SHAPE                # out overlaps x without being x
        assert step(x=off, x0=z) == ERR_ALIGN and step(out=off, x0=z) == ERR_ALIGN and step(acc=off, x0=z) == ERR_ALIGN
        assert step(n=0, x0=z) == 0 and step(n=0, mode=3, flag=m, x0=z) == 0
        assert step(out=x, n=0, x0=z) == 0                       # out may alias x ...
    assert step(out=x0) == ERR_SHAPE                             # ... but not the centre of the eps-ball
    assert step(x0=off) == ERR_ALIGN


def test_kernel_source_table_knows_the_new_kernels():
    from vqattack_amd import build
    assert "admix.hip" in build.SOURCES and len(set(build.SOURCES)) == len(build.SOURCES)
    keys = [k for k, _ in build.KERNEL_SOURCES]
    for name in ("void vqa::admix_copies_vec_kernel<5, true, 2, 0>(float __vector(4) const*, float __vector(4) const*, "
                 "int const*, float __vector(4)*, int, unsigned long, unsigned long, vqa::Scales, float, float)",
                 "void vqa::admix_copies_scalar_kernel<1, false>(float const*, float const*, int const*, float*, int, "
                 "unsigned long, unsigned long, vqa::Scales, float, float)",
                 "void vqa::grad_fold_vec_kernel<true, 0, 5, 1, 0>(float __vector(4) const*, float __vector(4) const*, "
                 "float __vector(4) const*, vqa::GradList, float __vector(4)*, unsigned long, vqa::StepParams, int*)",
                 "void vqa::grad_fold_vec_kernel<true, 2, 8, 1, 4>(float __vector(4) const*, float __vector(4) const*, "
                 "float __vector(4) const*, vqa::GradList, float __vector(4)*, unsigned long, vqa::StepParams, int*)",
                 "void vqa::grad_fold_scalar_kernel<true, 1, 3>(float const*, float const*, float const*, vqa::GradList, "
                 "float*, unsigned long, vqa::StepParams, int*)"):
        first = next(f for k, f in build.KERNEL_SOURCES if k in name)          # the FIRST key that matches decides
        assert first == "admix.hip", (name, first)
        assert build.kernel_source_digest(name) not in (None, build.kernel_source_digest("vqa::si_copies_vec_kernel<1>"))
    assert len(set(keys)) == len(keys)
    for name in ("vqa::si_copies_vec_kernel<1>", "vqa::grad_fold_vec_kernel<false, 2, 8, 1, 0>"):   # SI's stay where they were
        assert next(f for k, f in build.KERNEL_SOURCES if k in name) == "si.hip"


def test_entry_points_accept_the_keys():
    entry = os.path.join(ROOT, "entry")
    sys.path.insert(0, entry)
    try:
        mods = {}
        for name in ("run", "VQA"):
            spec = importlib.util.spec_from_file_location("vqattack_entry_admix_" + name, os.path.join(entry, name + ".py"))
            mods[name] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[name])
    finally:
        sys.path.remove(entry)
    cfg = mods["run"].parse([])
    assert cfg["admix_images"] is None and cfg["admix_eta"] == 0.2 and cfg["admix_seed"] is None
    cfg = mods["run"].parse(["with", "tiny", "admix_images=3", "admix_eta=0.25", "admix_seed=7"])
    assert cfg["admix_images"] == 3 and isinstance(cfg["admix_images"], int)
    assert cfg["admix_eta"] == 0.25 and cfg["admix_seed"] == 7 and isinstance(cfg["admix_seed"], int)
    with pytest.raises(SystemExit):
        mods["run"].parse(["admix_image=3"])
    with pytest.raises(ValueError):
        mods["run"].parse(["admix_images=three"])
    args = mods["VQA"].parse([])[0]
    assert args.admix_images is None and args.admix_eta == 0.2 and args.admix_seed is None
    args = mods["VQA"].parse(["--admix_images", "3", "--admix_eta", "0.25", "--admix_seed", "7"])[0]
    assert (args.admix_images, args.admix_eta, args.admix_seed) == (3, 0.25, 7)
    with pytest.raises(SystemExit):
        mods["VQA"].parse(["--admix_images", "three"])
    for name in ("run.py", "VQA.py"):                             # ... and hand them to the attack's configuration,
        text = open(os.path.join(entry, name)).read()             # whose constructor validates them
        for key in ("admix_images", "admix_eta", "admix_seed"):
            assert re.search(r"AttackConfig\([^)]*" + key + "=", text, flags=re.S), (name, key)


# ------------------------------------------------------------------------------------------------ the chain's launches
HOST = ("admix_draw", "admix_check_table", "admix_partners", "admix_weights")     # host-side helpers: they run as they are


class _Recorder(gold.Recorder):
    def __getattr__(self, name):
        return getattr(self.real, name) if name in HOST else super().__getattr__(name)


with open(gold.OUT) as f:
    GOLDEN = json.load(f)["entries"]


def _chain(monkeypatch, subset, norm=np.inf, images=3):
    rec = _Recorder(attacks.ops)
    monkeypatch.setattr(attacks, "ops", rec)
    monkeypatch.setattr(runner, "ops", rec)
    monkeypatch.setattr(attacks, "dev_f32", lambda t, *a, **k: t)
    admix = None if images is None else (images, 0.2, np.random.RandomState(4))
    chain = attacks._Chain(gold.specs(subset), gold.image(), norm, gold.EPS, gold.EPS_ITER, gold.N_EVALS, admix=admix)
    states = {s: getattr(chain, s) for s in gold.STAGES}
    scratch = gold.finish_states(rec, states)
    rec.name_state("ax", chain.ax)
    return rec, chain, scratch


def _evaluate_and_update(rec, chain, norm_step=True):
    """One evaluation at ``x`` with a stand-in for the model call (it names the gradient it leaves ``g<k>``), then the
    update: the recorded launches and the ``first`` flags the calls got."""
    x, x0, out = (rec.name(n, gold.image()) for n in ("x", "x0", "out"))
    firsts = []

    def call(leaf, first):
        leaf.grad = rec.name("g{}".format(len(firsts)), torch.zeros_like(leaf))
        firsts.append(first)

    grad = chain.evaluate(x, call)
    chain.update(x, grad, x0, gold.EPS_ITER, gold.EPS, gold.CLIP[0], gold.CLIP[1], out=out)
    return [c[0] for c in rec.calls], [c[1] for c in rec.calls], firsts


def test_admix_alone_folds_group_by_group_and_fuses_the_last_group_into_the_step(monkeypatch):
    rec, chain, _ = _chain(monkeypatch, frozenset())
    assert chain.fused == "si" and chain.si.ghat is None and chain.ax.gsum is not None     # no scratch but the sum
    assert chain.si.scales.tolist() == [1.0] and chain.si.weights.tolist() == [float(np.float32(1) / np.float32(3))]
    assert chain.ax.table.shape == (gold.N_EVALS, 3, gold.BATCH) and chain.ax.row.shape == (3, gold.BATCH)
    assert chain.ax.table.tolist() == ops.admix_draw(np.random.RandomState(4), gold.BATCH, gold.N_EVALS, 3).tolist()
    names, args, firsts = _evaluate_and_update(rec, chain)
    assert names == ["admix_copies", "si_combine", "admix_copies", "admix_accumulate", "admix_copies", "linf_admix_step"]
    assert firsts == [True, False, False]
    w = chain.si.weights.tolist()
    assert all(a["partner_row"].startswith("ax.table") for n, a in zip(names, args) if n == "admix_copies")
    assert all(a["out"] == "si.images[0:1]" and a["eta"] == 0.2 and a["m"] is None and a["scales"] == [1.0]
               for n, a in zip(names, args) if n == "admix_copies")
    assert args[1] == dict(grads=["g0[0:5]"], weights=w, out="ax.gsum[0:5]")
    assert args[3] == dict(grads=["g1[0:5]"], weights=w, acc="ax.gsum[0:5]")
    assert args[5] == dict(x="x[0:5]", acc="ax.gsum[0:5]", grads=["g2[0:5]"], x0="x0[0:5]", weights=w, eps_iter=gold.EPS_ITER,
                           eps=gold.EPS, clip_min=gold.CLIP[0], clip_max=gold.CLIP[1], flag=None, out="out[0:5]")


def test_admix_with_scale_copies_calls_group_major_and_keeps_m1_gradients_live(monkeypatch):
    rec, chain, _ = _chain(monkeypatch, frozenset({"si"}))
    names, args, firsts = _evaluate_and_update(rec, chain)
    assert names == ["admix_copies", "si_combine", "admix_copies", "admix_accumulate", "admix_copies", "linf_admix_step"]
    assert firsts == [True] + [False] * 5
    assert [a["grads"] for a in (args[1], args[3], args[5])] == [["g0[0:5]", "g1[0:5]"], ["g2[0:5]", "g3[0:5]"],
                                                               ["g4[0:5]", "g5[0:5]"]]
    assert args[5]["weights"] == [float(np.float32(s) / np.float32(6)) for s in (1.0, 0.5)]


def test_admix_with_momentum(monkeypatch):
    rec, chain, _ = _chain(monkeypatch, frozenset({"mom"}))
    assert chain.fused == "mom"
    names, args, _ = _evaluate_and_update(rec, chain)
    assert names == ["admix_copies", "si_combine", "admix_copies", "admix_accumulate", "admix_copies", "admix_accumulate",
                     "sumabs_per_sample", "linf_momentum_step"]
    assert args[5]["acc"] == "ax.gsum[0:5]" and args[6]["g"] == "ax.gsum[0:5]" and args[7]["g"] == "ax.gsum[0:5]"


def test_admix_with_di_and_ti(monkeypatch):
    rec, chain, _ = _chain(monkeypatch, frozenset({"di", "ti"}))
    assert chain.fused == "ti"
    names, args, _ = _evaluate_and_update(rec, chain)
    assert names == ["admix_copies", "di_transform", "si_combine", "admix_copies", "di_transform", "admix_accumulate",
                     "admix_copies", "di_transform", "admix_accumulate", "di_adjoint", "linf_ti_step"]
    assert len({a["geom"] for n, a in zip(names, args) if n in ("di_transform", "di_adjoint")}) == 1     # one evaluation's rows
    assert args[9]["gd"] == "ax.gsum[0:5]" and args[9]["out"] == "di.grad[0:5]" and args[10]["g"] == "di.grad[0:5]"


def test_admix_with_variance_tuning(monkeypatch):
    rec, chain, _ = _chain(monkeypatch, frozenset({"vt"}))
    assert chain.fused is None
    names, args, firsts = _evaluate_and_update(rec, chain)
    group = ["admix_copies", "si_combine", "admix_copies", "admix_accumulate", "admix_copies", "admix_accumulate"]
    assert names == group + ["vt_neighbors"] + (group + ["vt_accumulate"]) * 2 + ["vt_tune", "linf_step"]
    assert firsts == [True] + [False] * 8
    # the centre's sum lives where G(p) is expected, the neighbours' in the state's own tensor
    assert [a.get("acc", a.get("out")) for n, a in zip(names, args) if n in ("si_combine", "admix_accumulate")] == \
        ["vt.ghat[0:5]"] * 3 + ["ax.gsum[0:5]"] * 6
    # a neighbour tensor is mixed with its own samples
    assert [a["x"].split("[")[0] for n, a in zip(names, args) if n == "admix_copies"] == ["x"] * 3 + ["vt.chunk"] * 6
    assert args[names.index("vt_tune")]["g"] == "vt.ghat[0:5]"


def test_admix_under_l2_sums_in_front_of_the_existing_update(monkeypatch):
    rec, chain, _ = _chain(monkeypatch, frozenset(), norm=2)
    assert chain.fused is None
    names, args, _ = _evaluate_and_update(rec, chain)
    assert names == ["admix_copies", "si_combine", "admix_copies", "admix_accumulate", "admix_copies", "admix_accumulate",
                     "l2_fgm", "l2_project"]
    assert args[6]["g"] == "ax.gsum[0:5]"


@pytest.mark.parametrize("subset", [frozenset({"si"}), frozenset({"si", "mom"}), frozenset({"si", "di", "ti"})],
                         ids=lambda s: "+".join(sorted(s)))
@pytest.mark.parametrize("norm", ["inf", "2"])
def test_one_mixed_image_launches_what_si_launches_behind_the_model(monkeypatch, subset, norm):
    rec, chain, scratch = _chain(monkeypatch, subset, gold.NORMS[norm], images=1)
    assert chain.ax.gsum is None
    x, grad, x0, out, flag = gold.inputs(rec, subset)
    chain.update(x, grad, x0, gold.EPS_ITER, gold.EPS, gold.CLIP[0], gold.CLIP[1], out=out, flag=flag)
    got = json.loads(json.dumps({"calls": rec.calls, "scratch": scratch}))
    assert got == GOLDEN[gold.key("step", norm, subset)]
    rec.calls.clear()
    list(chain.leaves(x))
    assert [c[0] for c in rec.calls if c[0] != "di_transform"] == ["admix_copies"]      # only the copies kernel differs


def test_a_chain_without_admix_allocates_nothing_new(monkeypatch):
    for subset in (frozenset(), frozenset({"si"}), frozenset({"mom", "ti", "di", "si", "vt"})):
        rec, chain, scratch = _chain(monkeypatch, subset, images=None)
        assert chain.ax is None
        assert scratch == GOLDEN[gold.key("step", "inf", subset)]["scratch"]
        if "si" in subset:
            assert np.array_equal(chain.si.weights, ops.si_weights(chain.si.scales))


def test_draw_order_is_di_then_vt_then_admix(monkeypatch):
    rec = _Recorder(attacks.ops)
    monkeypatch.setattr(attacks, "ops", rec)
    monkeypatch.setattr(attacks, "dev_f32", lambda t, *a, **k: t)
    specs = (None, None, (1.0, 1, np.random), None, (2, 1.5, None))
    like = torch.zeros(gold.BATCH, 1, 4, 4)
    np.random.seed(17)
    chain = attacks._Chain(specs, like, np.inf, gold.EPS, gold.EPS_ITER, 2, admix=(2, 0.2, np.random))
    np.random.seed(17)
    geom = ops.di_draw(np.random, gold.BATCH, 2, 4, 4, 1, 1.0)
    seed = (int(np.random.randint(0, 1 << 32)) << 32) | int(np.random.randint(0, 1 << 32))
    table = ops.admix_draw(np.random, gold.BATCH, 2, 2)
    assert chain.di.table.tolist() == geom.tolist() and chain.vt.seed == seed and chain.ax.table.tolist() == table.tolist()


def test_a_batch_of_one_is_refused_by_the_chain_before_it_allocates(monkeypatch):
    with pytest.raises(ValueError, match="admix_images needs a batch"):
        attacks._Chain((None,) * 5, torch.zeros(1, 1, 2, 2), np.inf, 0.1, 0.01, admix=(3, 0.2, np.random.RandomState(0)))
