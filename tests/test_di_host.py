"""Host side of the DI (input diversity) feature: the geometry draws, table and argument validation, C ABI return codes,
configuration keys.  Everything here runs without a GPU."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

import vqattack_amd
from vqattack_amd import _hip, attacks, dropin, ops
from vqattack_amd._hip import HipExtensionError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_NULL, ERR_SHAPE, ERR_ALIGN = -1, -2, -3
NAMES = ("vqa_di_transform", "vqa_di_adjoint", "vqa_linf_di_step")


def _reference_draws(rs, steps, batch, h, w, shrink=32):
    """The draw order of the reference's input_diversity (cleverhans/fgsm_copy.py:9-31) per step and sample, followed by
    the one draw that decides whether the sample is transformed at all."""
    rows, us = [], []
    for _ in range(steps * batch):
        newh = int(rs.uniform(h - shrink, h))
        neww = int((newh / h) * w)
        top = int(rs.uniform(0, h - newh))
        left = int(rs.uniform(0, w - neww))
        rows.append([newh, neww, top, left])
        us.append(rs.uniform())
    return np.array(rows, dtype=np.int32).reshape(steps, batch, 4), np.array(us).reshape(steps, batch)


def test_di_draw_follows_the_reference_draw_order():
    want, us = _reference_draws(np.random.RandomState(7), 5, 3, 384, 384)
    rs = np.random.RandomState(7)
    got = ops.di_draw(rs, 3, 5, 384, 384)
    assert isinstance(got, np.ndarray) and got.dtype == np.int32 and got.shape == (5, 3, 4)
    assert np.array_equal(got, want)
    assert (got[..., 0] >= 352).all() and (got[..., 0] < 384).all() and np.array_equal(got[..., 1], got[..., 0])
    assert len(np.unique(got[..., 0])) > 3
    tail = rs.uniform()                                          # ... and exactly 4 draws per row were taken
    rs2 = np.random.RandomState(7)
    _reference_draws(rs2, 5, 3, 384, 384)
    assert tail == rs2.uniform()
    # a probability in between keeps the rows whose fourth draw is below it
    half = ops.di_draw(np.random.RandomState(7), 3, 5, 384, 384, prob=0.5)
    keep = us < 0.5
    assert keep.any() and not keep.all()
    assert np.array_equal(half[keep], want[keep]) and (half[~keep] == [384, 384, 0, 0]).all()
    # a non-square plane and another shrink
    want, _ = _reference_draws(np.random.RandomState(11), 2, 4, 40, 72, shrink=9)
    got = ops.di_draw(np.random.RandomState(11), 4, 2, 40, 72, shrink=9)
    assert np.array_equal(got, want) and (got[..., 0] >= 31).all()
    ops.di_check_table(got, 40, 72)
    # the module and a Generator are generators too
    assert ops.di_draw(np.random, 2, 1, 64, 64).shape == (1, 2, 4)
    assert ops.di_draw(np.random.default_rng(3), 2, 1, 64, 64).shape == (1, 2, 4)


def test_probability_zero_gives_identity_rows_and_consumes_the_same_stream():
    rs = np.random.RandomState(7)
    got = ops.di_draw(rs, 3, 5, 384, 300, prob=0.0)
    assert (got == [384, 300, 0, 0]).all()
    rs2 = np.random.RandomState(7)
    ops.di_draw(rs2, 3, 5, 384, 300, prob=1.0)
    assert rs.uniform() == rs2.uniform()


def test_di_draw_refuses_a_shrink_that_leaves_no_row():
    for h, shrink in ((32, 32), (16, 32), (5, 5)):
        with pytest.raises(ValueError):
            ops.di_draw(np.random.RandomState(0), 1, 1, h, 64, shrink=shrink)
    assert ops.di_draw(np.random.RandomState(0), 1, 1, 33, 64, shrink=32).shape == (1, 1, 4)
    with pytest.raises(ValueError):                              # new_w = int(new_h / H * W) would be 0
        ops.di_draw(np.random.RandomState(0), 1, 1, 64, 1, shrink=32)


def test_di_geometry_refuses_every_range_violation():
    h, w = 40, 72
    good = [[40, 72, 0, 0], [1, 1, 39, 71], [33, 60, 7, 12], [33, 60, 0, 0]]
    t = ops.di_check_table(good, h, w)
    assert t.dtype == np.int32 and t.shape == (4, 4) and t.flags["C_CONTIGUOUS"]
    assert ops.di_check_table(np.array([good, good]), h, w).shape == (2, 4, 4)
    for bad in ([0, 72, 0, 0], [41, 72, 0, 0], [40, 0, 0, 0], [40, 73, 0, 0], [33, 60, -1, 0], [33, 60, 8, 0],
                [33, 60, 0, -1], [33, 60, 0, 13], [40, 72, 1, 0], [40, 72, 0, 1], [-5, -5, 0, 0]):
        with pytest.raises(ValueError):
            ops.di_check_table([good[2], bad], h, w)
        with pytest.raises(ValueError):                          # refused on the host, before the device is looked at
            ops.di_geometry([bad], h, w, "cuda:0")
    for bad in ([[1.0, 1.0, 0.0, 0.0]], [[1, 1, 0]], 5, [1, 1, 0, 0, 0]):
        with pytest.raises(ValueError):
            ops.di_check_table(bad, h, w)


def test_validate_di():
    assert attacks._validate_di(None) is None
    assert attacks._validate_di(None, di_shrink=-4, di_rng="ignored") is None      # off: the other keys are not looked at
    prob, shrink, rng = attacks._validate_di(0.5)
    assert prob == 0.5 and shrink == 32 and rng is np.random
    rs = np.random.RandomState(1)
    assert attacks._validate_di(1, 8, rs) == (1.0, 8, rs)
    assert attacks._validate_di(np.float32(0.0), np.int64(1), np.random.default_rng(0))[:2] == (0.0, 1)
    for bad in (-0.1, 1.5, float("nan"), float("inf"), True, "0.5", [0.5]):
        with pytest.raises(ValueError):
            attacks._validate_di(bad)
    for bad in (0, -1, 2.0, True, "32", None):
        with pytest.raises(ValueError):
            attacks._validate_di(0.5, bad)
    for bad in (7, "rng", object()):
        with pytest.raises(ValueError):
            attacks._validate_di(0.5, 32, bad)


def _unreachable(_):
    raise AssertionError("model_fn must not run: the arguments are refused first")


class _NoDraw:
    def uniform(self, *a, **k):
        raise AssertionError("no random number may be drawn before the tensors are checked")


@pytest.mark.parametrize("call", ["pgd", "pgd_vl", "mim", "fgm", "fgm_vl"])
def test_operators_validate_the_di_keys_before_any_tensor(call):
    x = torch.zeros(2, 3, 4, 4)                                  # a CPU tensor: refused, but only after the arguments
    y = [x, x]

    def run(norm=np.inf, **kw):
        if call == "pgd":
            return vqattack_amd.projected_gradient_descent(_unreachable, x, 0.1, 0.01, 2, norm, y=y, ori_x=x, ls=1, **kw)
        if call == "pgd_vl":
            return vqattack_amd.projected_gradient_descent_vl(_unreachable, [x, x], 0.1, 0.01, 2, norm, y=y, ori_x=x,
                                                              ls=1, **kw)
        if call == "mim":
            return vqattack_amd.momentum_iterative_method(_unreachable, x, 0.1, 0.01, 2, norm, y=y, **kw)
        if call == "fgm":
            return vqattack_amd.fast_gradient_method(_unreachable, x, 0.1, norm, x, y=y, ls=1, **kw)
        return vqattack_amd.fast_gradient_method_vl(_unreachable, [x, x], 0.1, norm, x, y=y, ls=1, **kw)

    for bad in (dict(diversity_prob=1.5), dict(diversity_prob=-1), dict(diversity_prob=True),
                dict(diversity_prob=0.5, di_shrink=0), dict(diversity_prob=0.5, di_shrink=1.5),
                dict(diversity_prob=0.5, di_rng=3)):
        with pytest.raises(ValueError):
            run(**bad)
        with pytest.raises(ValueError):
            run(norm=2, **bad)
    for good in (dict(), dict(diversity_prob=None), dict(diversity_prob=None, di_shrink=0),
                 dict(diversity_prob=0.5, di_rng=_NoDraw()), dict(diversity_prob=1.0, di_shrink=2, di_rng=_NoDraw()),
                 dict(diversity_prob=0.7, ti_kernel=7, di_rng=_NoDraw())):
        with pytest.raises(HipExtensionError):                   # fine: the CPU tensor is what is refused
            run(**good)


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_the_keywords_reach_the_dropin_bindings(flavor):
    ns = dropin.load(flavor)
    x = torch.zeros(2, 3, 4, 4)
    for bound in (ns.projected_gradient_descent.projected_gradient_descent,
                  ns.momentum_iterative_method.momentum_iterative_method):
        with pytest.raises(ValueError):
            bound(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x, ls=1, diversity_prob=2.0)
        with pytest.raises(HipExtensionError):
            bound(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x, ls=1, diversity_prob=0.5, di_shrink=2)
    with pytest.raises(ValueError):
        ns.projected_gradient_descent_vl.projected_gradient_descent(_unreachable, [x, x], 0.1, 0.01, 2, np.inf, y=[x, x],
                                                                    ori_x=x, ls=1, diversity_prob=2.0)
    with pytest.raises(ValueError):
        ns.fast_gradient_method.fast_gradient_method(_unreachable, x, 0.1, np.inf, x, y=[x, x], ls=1, diversity_prob=2.0)


def test_ops_refuse_cpu_tensors_and_bad_tables():
    g = torch.zeros(2, 3, 8, 8)
    geom = torch.zeros(2, 4, dtype=torch.int32)
    with pytest.raises(HipExtensionError):
        ops.di_transform(g, geom)
    with pytest.raises(HipExtensionError):
        ops.di_adjoint(g, geom)
    with pytest.raises(HipExtensionError):
        ops.linf_di_step(g, g, g, geom, 0.01, 0.1, -1.0, 1.0)
    with pytest.raises(TypeError):
        ops.di_transform([0.0, 1.0], geom)


def test_attack_config_takes_the_di_keys_and_refuses_them_with_patch_layout():
    from vqattack_amd.attack.runner import AttackConfig
    c = AttackConfig()
    assert c.diversity_prob is None and c.di_shrink == 32 and c.di_seed is None
    c = AttackConfig(diversity_prob=0.5, di_shrink=16, di_seed=3, ti_kernel=7, decay_factor=1.0)
    assert (c.diversity_prob, c.di_shrink, c.di_seed) == (0.5, 16, 3)
    assert AttackConfig(patch_layout=True).patch_layout                      # still fine on its own
    with pytest.raises(ValueError):
        AttackConfig(diversity_prob=0.5, patch_layout=True)
    for bad in (dict(diversity_prob=1.5), dict(diversity_prob=0.5, di_shrink=0), dict(diversity_prob=0.5, di_seed=-1),
                dict(di_seed=1.5), dict(diversity_prob="1")):
        with pytest.raises(ValueError):
            AttackConfig(**bad)


def test_header_declares_and_library_exports_the_three_entry_points():
    text = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    assert _hip.lib().vqa_abi_version() == 4                   # additive exports: the version stays


def test_entry_points_validate_before_the_first_launch():
    """Every return code of the header's list, through the library on a machine without a GPU."""
    lib = _hip.lib()
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 512)                           # a second buffer: the input must not be out
    off = ctypes.c_void_p(p.value + 2)                           # not 4-byte aligned
    tab = (ctypes.c_int * 16)()
    gm = ctypes.cast(tab, ctypes.c_void_p)
    gm_off = ctypes.c_void_p(gm.value + 2)
    null = None
    big = 2 ** 31 - 1

    def fwd(x=p, geom=gm, out=q, b=2, c=1, h=4, w=4):
        return lib.vqa_di_transform(x, geom, out, b, c, h, w, null)

    def adj(g=p, geom=gm, out=q, b=2, c=1, h=4, w=4):
        return lib.vqa_di_adjoint(g, geom, out, b, c, h, w, null)

    def step(x=p, g=p, x0=p, geom=gm, out=q, b=2, c=1, h=4, w=4, mode=1, flag=null):
        return lib.vqa_linf_di_step(x, g, x0, geom, out, b, c, h, w, 0.01, 0.1, -1.0, 1.0, mode, flag, null)

    for f in (fwd, adj):
        first = "x" if f is fwd else "g"
        assert f(**{first: null}) == ERR_NULL and f(geom=null) == ERR_NULL and f(out=null) == ERR_NULL
        assert f(b=-1) == ERR_SHAPE and f(c=-1) == ERR_SHAPE and f(h=-1) == ERR_SHAPE and f(w=-1) == ERR_SHAPE
        assert f(b=big, c=big, h=big, w=big) == ERR_SHAPE        # more tiles than one launch has workgroups
        assert f(b=big, c=1, h=big, w=big) == ERR_SHAPE
        assert f(out=p) == ERR_SHAPE                             # the input is out
        assert f(**{first: off}) == ERR_ALIGN and f(out=off) == ERR_ALIGN and f(geom=gm_off) == ERR_ALIGN
        assert f(b=0) == 0 and f(c=0) == 0 and f(h=0) == 0 and f(w=0) == 0          # empty: no launch
    for x0 in (p, null):                                         # both forms of the fused step
        assert step(x=null, x0=x0) == ERR_NULL and step(g=null, x0=x0) == ERR_NULL
        assert step(out=null, x0=x0) == ERR_NULL and step(geom=null, x0=x0) == ERR_NULL
        assert step(mode=3, x0=x0) == ERR_NULL                   # a range check needs a flag
        assert step(b=-1, x0=x0) == ERR_SHAPE and step(c=-1, x0=x0) == ERR_SHAPE
        assert step(h=-1, x0=x0) == ERR_SHAPE and step(w=-1, x0=x0) == ERR_SHAPE
        assert step(b=big, c=big, h=big, w=big, x0=x0) == ERR_SHAPE
        assert step(g=q, out=q, x0=x0) == ERR_SHAPE              # gD == out
        assert step(x=off, x0=x0) == ERR_ALIGN and step(g=off, x0=x0) == ERR_ALIGN and step(out=off, x0=x0) == ERR_ALIGN
        assert step(geom=gm_off, x0=x0) == ERR_ALIGN
        assert step(b=0, x0=x0) == 0 and step(c=0, x0=x0) == 0 and step(h=0, x0=x0) == 0 and step(w=0, x0=x0) == 0
        assert step(b=0, mode=3, flag=p, x0=x0) == 0
        assert step(x=q, out=q, b=0, x0=x0) == 0                 # out may alias x
    assert step(x0=off) == ERR_ALIGN


def test_kernel_source_table_knows_the_new_kernels():
    from vqattack_amd import build
    assert "di.hip" in build.SOURCES
    keys = [k for k, _ in build.KERNEL_SOURCES]
    for name in ("void vqa::di_adjoint_kernel<2>(float const*, float const*, float const*, int const*, float*, int)",
                 "vqa::di_forward_kernel(float const*, int const*, float*, int, int, int, int, int, int)"):
        first = next(f for k, f in build.KERNEL_SOURCES if k in name)          # the FIRST key that matches decides
        assert first == "di.hip", (name, first)
        assert build.kernel_source_digest(name) not in (None, build.kernel_source_digest("vqa::ti_kernel<32, 15, 2>"))
    assert len(set(keys)) == len(keys)


def test_entry_points_accept_the_keys():
    entry = os.path.join(ROOT, "entry")
    sys.path.insert(0, entry)
    try:
        mods = {}
        for name in ("run", "VQA"):
            spec = importlib.util.spec_from_file_location("vqattack_entry_di_" + name, os.path.join(entry, name + ".py"))
            mods[name] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[name])
    finally:
        sys.path.remove(entry)
    cfg = mods["run"].parse([])
    assert cfg["diversity_prob"] is None and cfg["di_shrink"] == 32 and cfg["di_seed"] is None
    cfg = mods["run"].parse(["with", "tiny", "diversity_prob=0.5", "di_shrink=8", "di_seed=3", "ti_kernel=15"])
    assert cfg["diversity_prob"] == 0.5 and isinstance(cfg["diversity_prob"], float)
    assert cfg["di_shrink"] == 8 and cfg["di_seed"] == 3 and isinstance(cfg["di_seed"], int) and cfg["ti_kernel"] == 15
    with pytest.raises(SystemExit):
        mods["run"].parse(["diversity_porb=0.5"])
    args = mods["VQA"].parse([])[0]
    assert args.diversity_prob is None and args.di_shrink == 32 and args.di_seed is None
    args = mods["VQA"].parse(["--diversity_prob", "0.7", "--di_shrink", "16", "--di_seed", "5"])[0]
    assert (args.diversity_prob, args.di_shrink, args.di_seed) == (0.7, 16, 5)
    for name in ("run.py", "VQA.py"):                             # ... and hand them to the attack's configuration
        text = open(os.path.join(entry, name)).read()
        for key in ("diversity_prob", "di_shrink", "di_seed"):
            assert re.search(r"AttackConfig\([^)]*" + key + "=", text, flags=re.S), (name, key)
