"""Host side of the TI (translation-invariant) smoothing feature: taps, argument validation, C ABI return codes,
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


def test_gaussian_taps_are_the_papers():
    x = np.linspace(-3.0, 3.0, 15)
    k = np.exp(-x * x / 2.0)
    want = (k / k.sum()).astype(np.float32)
    got = ops.ti_gaussian_taps(15)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (15,)
    assert np.array_equal(got, want) and np.array_equal(got, ops.ti_gaussian_taps(kernlen=15, nsig=3.0))
    assert abs(float(got.astype(np.float64).sum()) - 1.0) <= 2.0 ** -23
    assert np.array_equal(got, got[::-1]) and int(np.argmax(got)) == 7
    assert np.array_equal(ops.ti_gaussian_taps(1), np.ones(1, dtype=np.float32))
    assert not re.search(r"^\s*(import|from)\s+scipy", open(ops.__file__).read(), flags=re.M)


def test_validate_ti():
    assert attacks._validate_ti(None) is None
    assert np.array_equal(attacks._validate_ti(15), ops.ti_gaussian_taps(15, 3.0))
    assert np.array_equal(attacks._validate_ti(np.int64(7)), ops.ti_gaussian_taps(7))
    taps = attacks._validate_ti([0.25, 0.5, 0.25])
    assert taps.dtype == np.float32 and taps.tolist() == [0.25, 0.5, 0.25]
    assert attacks._validate_ti(np.ones(31)).shape == (31,)
    for bad in (14, 2, 33, 0, -3, True, [0.5, 0.5], [1.0] * 33, [], [0.2, float("nan"), 0.2], [0.2, float("inf"), 0.2],
                np.ones((3, 3)), "15", 15.0):
        with pytest.raises(ValueError):
            attacks._validate_ti(bad)


def _unreachable(_):
    raise AssertionError("model_fn must not run: the arguments are refused first")


@pytest.mark.parametrize("call", ["pgd", "pgd_vl", "mim", "fgm", "fgm_vl"])
def test_operators_validate_ti_kernel_before_any_tensor(call):
    x = torch.zeros(2, 3, 4, 4)                                  # a CPU tensor: refused, but only after the arguments
    y = [x, x]

    def run(ti, norm=np.inf):
        if call == "pgd":
            return vqattack_amd.projected_gradient_descent(_unreachable, x, 0.1, 0.01, 2, norm, y=y, ori_x=x, ls=1,
                                                           ti_kernel=ti)
        if call == "pgd_vl":
            return vqattack_amd.projected_gradient_descent_vl(_unreachable, [x, x], 0.1, 0.01, 2, norm, y=y, ori_x=x,
                                                              ls=1, ti_kernel=ti)
        if call == "mim":
            return vqattack_amd.momentum_iterative_method(_unreachable, x, 0.1, 0.01, 2, norm, y=y, ti_kernel=ti)
        if call == "fgm":
            return vqattack_amd.fast_gradient_method(_unreachable, x, 0.1, norm, x, y=y, ls=1, ti_kernel=ti)
        return vqattack_amd.fast_gradient_method_vl(_unreachable, [x, x], 0.1, norm, x, y=y, ls=1, ti_kernel=ti)

    for bad in (14, 33, 0, [0.5, 0.5], [0.2, float("nan"), 0.2], np.ones((3, 3))):
        with pytest.raises(ValueError):
            run(bad)
        with pytest.raises(ValueError):
            run(bad, norm=2)
    for good in (None, 1, 15, [0.25, 0.5, 0.25]):
        with pytest.raises(HipExtensionError):                   # fine: the CPU tensor is what is refused
            run(good)


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_the_keyword_reaches_the_dropin_bindings(flavor):
    ns = dropin.load(flavor)
    x = torch.zeros(2, 3, 4, 4)
    for bound in (ns.projected_gradient_descent.projected_gradient_descent,
                  ns.momentum_iterative_method.momentum_iterative_method):
        assert bound.keywords == {"flavor": flavor}
        with pytest.raises(ValueError):
            bound(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x, ls=1, ti_kernel=14)
        with pytest.raises(HipExtensionError):
            bound(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x, ls=1, ti_kernel=15)
    with pytest.raises(ValueError):
        ns.projected_gradient_descent_vl.projected_gradient_descent(_unreachable, [x, x], 0.1, 0.01, 2, np.inf, y=[x, x],
                                                                    ori_x=x, ls=1, ti_kernel=14)
    with pytest.raises(ValueError):
        ns.fast_gradient_method.fast_gradient_method(_unreachable, x, 0.1, np.inf, x, y=[x, x], ls=1, ti_kernel=14)


def test_ops_refuse_cpu_tensors_and_bad_taps():
    g = torch.zeros(2, 3, 8, 8)
    w = ops.ti_gaussian_taps(15)
    with pytest.raises(HipExtensionError):
        ops.ti_smooth(g, w)
    with pytest.raises(HipExtensionError):
        ops.linf_ti_step(g, g, g, w, 0.01, 0.1, -1.0, 1.0)
    with pytest.raises(TypeError):
        ops.ti_smooth([0.0, 1.0], w)


def test_attack_config_takes_a_ti_kernel_and_refuses_it_with_patch_layout():
    from vqattack_amd.attack.runner import AttackConfig
    assert AttackConfig().ti_kernel is None
    assert AttackConfig(ti_kernel=15).ti_kernel == 15
    assert AttackConfig(ti_kernel=7, decay_factor=1.0).decay_factor == 1.0
    assert AttackConfig(patch_layout=True).patch_layout                      # still fine on its own
    with pytest.raises(ValueError):
        AttackConfig(ti_kernel=15, patch_layout=True)
    for bad in (14, 33, 0, [0.5, 0.5]):
        with pytest.raises(ValueError):
            AttackConfig(ti_kernel=bad)


def test_header_declares_and_library_exports_the_two_entry_points():
    text = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in ("vqa_ti_smooth", "vqa_linf_ti_step"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    assert _hip.lib().vqa_abi_version() == 4                   # additive exports: the version stays


def test_entry_points_validate_before_the_first_launch():
    """Every return code of the header's list, through the library on a machine without a GPU."""
    lib = _hip.lib()
    buf = (ctypes.c_float * 256)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    q = ctypes.c_void_p(p.value + 512)                           # a second buffer: g must not be out
    off = ctypes.c_void_p(p.value + 2)                           # not 4-byte aligned
    taps = (ctypes.c_float * 31)(*([1.0 / 31] * 31))
    null = None
    big = 2 ** 31 - 1

    def smooth(g=p, out=q, planes=2, h=4, w=4, t=taps, k=15):
        return lib.vqa_ti_smooth(g, out, planes, h, w, t, k, null)

    def step(x=p, g=p, x0=p, out=q, planes=2, h=4, w=4, t=taps, k=15, mode=1, flag=null):
        return lib.vqa_linf_ti_step(x, g, x0, out, planes, h, w, t, k, 0.01, 0.1, -1.0, 1.0, mode, flag, null)

    assert smooth(g=null) == ERR_NULL and smooth(out=null) == ERR_NULL and smooth(t=null) == ERR_NULL
    for k in (0, 2, 14, 32, 33, -1):
        assert smooth(k=k) == ERR_SHAPE and step(k=k) == ERR_SHAPE and step(x0=null, k=k) == ERR_SHAPE
    assert smooth(planes=-1) == ERR_SHAPE and smooth(h=-1) == ERR_SHAPE and smooth(w=-1) == ERR_SHAPE
    assert smooth(planes=big, h=big, w=big) == ERR_SHAPE         # more tiles than one launch has workgroups
    assert smooth(out=p) == ERR_SHAPE                            # g == out
    assert smooth(g=off) == ERR_ALIGN and smooth(out=off) == ERR_ALIGN
    assert smooth(planes=0) == 0 and smooth(h=0) == 0 and smooth(w=0) == 0      # empty: no launch
    assert smooth(planes=0, k=1) == 0 and smooth(planes=0, k=31) == 0
    for x0 in (p, null):                                         # both forms of the fused step
        assert step(x=null, x0=x0) == ERR_NULL and step(g=null, x0=x0) == ERR_NULL
        assert step(out=null, x0=x0) == ERR_NULL and step(t=null, x0=x0) == ERR_NULL
        assert step(mode=3, x0=x0) == ERR_NULL                   # a range check needs a flag
        assert step(planes=-1, x0=x0) == ERR_SHAPE and step(h=-1, x0=x0) == ERR_SHAPE and step(w=-1, x0=x0) == ERR_SHAPE
        assert step(planes=big, h=big, w=big, x0=x0) == ERR_SHAPE
        assert step(g=q, out=q, x0=x0) == ERR_SHAPE              # g == out
        assert step(x=off, x0=x0) == ERR_ALIGN and step(g=off, x0=x0) == ERR_ALIGN and step(out=off, x0=x0) == ERR_ALIGN
        assert step(planes=0, x0=x0) == 0 and step(h=0, x0=x0) == 0 and step(w=0, x0=x0) == 0
        assert step(planes=0, mode=3, flag=p, x0=x0) == 0
        assert step(x=q, out=q, planes=0, x0=x0) == 0            # out may alias x
    assert step(x0=off) == ERR_ALIGN


def test_kernel_source_table_knows_the_new_kernels():
    from vqattack_amd import build
    assert "ti.hip" in build.SOURCES and ("ti_kernel", "ti.hip") in build.KERNEL_SOURCES
    digest = build.kernel_source_digest("void vqa::ti_kernel<32, 15, 2>(float const*, float const*)")
    assert digest is not None and digest != build.kernel_source_digest("vqa::momentum_scalar_kernel<0>")


def test_entry_points_accept_the_key():
    entry = os.path.join(ROOT, "entry")
    sys.path.insert(0, entry)
    try:
        mods = {}
        for name in ("run", "VQA"):
            spec = importlib.util.spec_from_file_location("vqattack_entry_ti_" + name, os.path.join(entry, name + ".py"))
            mods[name] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[name])
    finally:
        sys.path.remove(entry)
    assert mods["run"].parse([])["ti_kernel"] is None
    cfg = mods["run"].parse(["with", "tiny", "ti_kernel=15", "decay_factor=1.0"])
    assert cfg["ti_kernel"] == 15 and isinstance(cfg["ti_kernel"], int) and cfg["decay_factor"] == 1.0
    with pytest.raises(SystemExit):
        mods["run"].parse(["ti_kernle=15"])
    assert mods["VQA"].parse([])[0].ti_kernel is None
    assert mods["VQA"].parse(["--ti_kernel", "7"])[0].ti_kernel == 7
    for name in ("run.py", "VQA.py"):                             # ... and hand it to the attack's configuration
        assert re.search(r"AttackConfig\([^)]*ti_kernel=", open(os.path.join(entry, name)).read(), flags=re.S), name
