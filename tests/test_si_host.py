"""Host side of the SI-NI (scale copies, Nesterov look-ahead) feature: argument validation, scales and weights, C ABI
return codes, configuration keys.  Everything here runs without a GPU."""
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
NAMES = ("vqa_si_max_copies", "vqa_si_copies", "vqa_si_combine", "vqa_linf_si_step")


def test_validate_si():
    assert attacks._validate_si(None) is None
    assert attacks._validate_si(None, False, 0.9) is None
    for n in range(1, 9):
        scales, nesterov = attacks._validate_si(n)
        assert scales.dtype == np.float32 and nesterov is False
        assert np.array_equal(scales, np.float32(2.0) ** -np.arange(n, dtype=np.float32))
    scales, nesterov = attacks._validate_si(np.int64(3), True, 1.0)
    assert scales.tolist() == [1.0, 0.5, 0.25] and nesterov is True
    scales, nesterov = attacks._validate_si([1.0, 0.7, 0.3])             # a sequence is the scales themselves
    assert np.array_equal(scales, np.array([1.0, 0.7, 0.3], dtype=np.float32)) and not nesterov
    assert attacks._validate_si((2.0,))[0].tolist() == [2.0]
    assert attacks._validate_si(np.arange(1, 9, dtype=np.float64))[0].shape == (8,)
    scales, nesterov = attacks._validate_si(None, True, 0.5)             # look-ahead alone: one copy at scale 1
    assert scales.tolist() == [1.0] and nesterov is True
    for bad in (0, 9, -1, True, False, [], (), [1.0] * 9, [1.0, float("nan")], [float("inf")], [1.0, 0.0], [-0.5],
                [[1.0, 0.5]], "3", 2.5, object()):
        with pytest.raises(ValueError):
            attacks._validate_si(bad)
    with pytest.raises(ValueError):
        attacks._validate_si(3, True, None)                              # no momentum to look ahead along
    with pytest.raises(ValueError):
        attacks._validate_si(None, True)
    with pytest.raises(ValueError):
        attacks._validate_si(3, 1, 0.9)                                  # nesterov is a bool


def test_scales_and_weights_are_the_stated_float32_values():
    for n in range(1, 9):
        s = ops.si_scales(n)
        assert isinstance(s, np.ndarray) and s.dtype == np.float32 and s.shape == (n,)
        assert s.tolist() == [2.0 ** -i for i in range(n)]
        w = ops.si_weights(s)
        assert w.dtype == np.float32 and w.shape == (n,)
        for i in range(n):
            assert w[i] == np.float32(s[i]) / np.float32(n)
    assert ops.si_weights([1.0]).tolist() == [1.0]
    w = ops.si_weights([1.0, 0.7, 0.3])
    assert w[1] == np.float32(0.7) / np.float32(3)
    for bad in (0, 9, -2):
        with pytest.raises(ValueError):
            ops.si_scales(bad)
    for bad in ([], [1.0] * 9, [[1.0]]):
        with pytest.raises(ValueError):
            ops.si_weights(bad)
    assert ops.SI_MAX_COPIES == 8 == _hip.lib().vqa_si_max_copies()


def _unreachable(_):
    raise AssertionError("model_fn must not run: the arguments are refused first")


@pytest.mark.parametrize("call", ["pgd", "pgd_vl", "mim", "fgm", "fgm_vl"])
def test_operators_validate_the_si_keys_before_any_tensor(call):
    x = torch.zeros(2, 3, 4, 4)                                  # a CPU tensor: refused, but only after the arguments
    y = [x, x]
    loop = call in ("pgd", "pgd_vl", "mim")

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

    for bad in (dict(si_copies=0), dict(si_copies=9), dict(si_copies=True), dict(si_copies=[]),
                dict(si_copies=[1.0, -1.0]), dict(si_copies=[float("nan")])):
        with pytest.raises(ValueError):
            run(**bad)
        with pytest.raises(ValueError):
            run(norm=2, **bad)
    good = [dict(), dict(si_copies=None), dict(si_copies=1), dict(si_copies=8), dict(si_copies=[1.0, 0.5]),
            dict(si_copies=3, ti_kernel=7)]
    if loop:
        if call != "mim":                                        # (its decay factor defaults to 1)
            with pytest.raises(ValueError):
                run(nesterov=True)
            with pytest.raises(ValueError):
                run(si_copies=3, nesterov=True)
        good += [dict(nesterov=True, decay_factor=0.9), dict(si_copies=3, nesterov=True, decay_factor=1.0),
                 dict(nesterov=False)]
    else:
        with pytest.raises(TypeError):                           # one step has no momentum to look ahead along
            run(nesterov=True)
    for kw in good:
        with pytest.raises(HipExtensionError):                   # fine: the CPU tensor is what is refused
            run(**kw)


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_the_keywords_reach_the_dropin_bindings(flavor):
    ns = dropin.load(flavor)
    x = torch.zeros(2, 3, 4, 4)
    for bound in (ns.projected_gradient_descent.projected_gradient_descent,
                  ns.momentum_iterative_method.momentum_iterative_method):
        with pytest.raises(ValueError):
            bound(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x, ls=1, si_copies=9)
        with pytest.raises(HipExtensionError):
            bound(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x, ls=1, si_copies=3, nesterov=True,
                  decay_factor=0.9)
    with pytest.raises(ValueError):
        ns.projected_gradient_descent.projected_gradient_descent(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x,
                                                                 ls=1, nesterov=True)
    with pytest.raises(ValueError):
        ns.projected_gradient_descent_vl.projected_gradient_descent(_unreachable, [x, x], 0.1, 0.01, 2, np.inf, y=[x, x],
                                                                    ori_x=x, ls=1, si_copies=0)
    with pytest.raises(ValueError):
        ns.fast_gradient_method.fast_gradient_method(_unreachable, x, 0.1, np.inf, x, y=[x, x], ls=1, si_copies=0)
    with pytest.raises(ValueError):
        ns.fast_gradient_method_vl.fast_gradient_method(_unreachable, [x, x], 0.1, np.inf, x, y=[x, x], ls=1, si_copies=9)


def test_ops_refuse_cpu_tensors_and_bad_lists():
    g = torch.zeros(2, 3, 8, 8)
    with pytest.raises(HipExtensionError):
        ops.si_copies(g, [1.0, 0.5])
    with pytest.raises(HipExtensionError):
        ops.si_combine([g, g], [0.5, 0.25])
    with pytest.raises(HipExtensionError):
        ops.linf_si_step(g, [g, g], g, [0.5, 0.25], 0.01, 0.1, -1.0, 1.0)
    with pytest.raises(TypeError):
        ops.si_combine(g, [1.0])                                 # a stack is not a list of gradients
    with pytest.raises(TypeError):
        ops.si_combine([[0.0, 1.0]], [1.0])
    with pytest.raises(ValueError):
        ops.si_combine([], [])
    with pytest.raises(ValueError):
        ops.si_combine([g] * 9, [1.0] * 9)                       # more than vqa_si_max_copies()
    with pytest.raises(ValueError):
        ops.si_copies(g, [1.0] * 9)
    with pytest.raises(ValueError):
        ops.si_copies(g, [])


def test_attack_config_takes_the_si_keys_and_performs_its_refusals():
    from vqattack_amd.attack.runner import AttackConfig
    c = AttackConfig()
    assert c.si_copies is None and c.nesterov is False
    c = AttackConfig(si_copies=5, nesterov=True, decay_factor=1.0, ti_kernel=7, diversity_prob=0.5)
    assert (c.si_copies, c.nesterov) == (5, True)
    assert AttackConfig(si_copies=[1.0, 0.5]).si_copies == [1.0, 0.5]
    assert AttackConfig(patch_layout=True).patch_layout                      # still fine on its own
    with pytest.raises(ValueError):
        AttackConfig(si_copies=3, patch_layout=True)
    with pytest.raises(ValueError):
        AttackConfig(nesterov=True)                                          # no decay factor
    with pytest.raises(ValueError):
        AttackConfig(si_copies=3, nesterov=True)
    for bad in (dict(si_copies=0), dict(si_copies=9), dict(si_copies=True), dict(si_copies=[0.0]), dict(si_copies="3")):
        with pytest.raises(ValueError):
            AttackConfig(**bad)


def test_header_declares_and_library_exports_the_four_symbols():
    text = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    assert re.search(r"#define\s+VQA_SI_MAX_COPIES\s+8\b", text)
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
    x, m, x0, out = at(0), at(16), at(32), at(512)              # n = 16 floats each; out has room for 8 copies of 16
    g = [at(64 + 16 * i) for i in range(9)]
    off = ctypes.c_void_p(base + 4 * 900 + 2)                    # not 4-byte aligned, and apart from all the others
    null = None
    scales = (ctypes.c_float * 9)(*[2.0 ** -i for i in range(9)])
    weights = (ctypes.c_float * 9)(*[0.125] * 9)

    def ptrs(entries):
        return (ctypes.c_void_p * len(entries))(*[e if e is None else e.value for e in entries])

    def copies(x=x, m=null, out=out, n=16, stride=16, sc=scales, c=3):
        return lib.vqa_si_copies(x, m, out, n, stride, sc, c, 0.5, null)

    def combine(gl=g[:3], w=weights, c=3, out=out, n=16, raw=False):
        return lib.vqa_si_combine(gl if raw else ptrs(gl), w, c, out, n, null)

    def step(x=x, gl=g[:3], w=weights, c=3, x0=x0, out=out, n=16, mode=1, flag=null, raw=False):
        return lib.vqa_linf_si_step(x, gl if raw else ptrs(gl), w, c, x0, out, n, 0.01, 0.1, -1.0, 1.0, mode, flag, null)

    for mm in (null, m):                                         # with and without the look-ahead
        assert copies(x=null, m=mm) == ERR_NULL and copies(out=null, m=mm) == ERR_NULL and copies(sc=null, m=mm) == ERR_NULL
        assert copies(c=0, m=mm) == ERR_SHAPE and copies(c=9, m=mm) == ERR_SHAPE and copies(c=-1, m=mm) == ERR_SHAPE
        assert copies(stride=15, m=mm) == ERR_SHAPE              # copy_stride < n
        assert copies(out=x, m=mm) == ERR_SHAPE                  # out overlaps x
        assert copies(x=at(512 + 40), m=mm) == ERR_SHAPE         # x inside the third copy
        assert copies(x=off, m=mm) == ERR_ALIGN and copies(out=off, m=mm) == ERR_ALIGN
        assert copies(n=0, stride=0, m=mm) == 0 and copies(n=0, m=mm) == 0           # empty: no launch
    assert copies(m=at(512 + 16)) == ERR_SHAPE                   # m inside the second copy
    assert copies(m=off) == ERR_ALIGN
    assert copies(c=1, out=at(16), n=0) == 0

    assert combine(gl=null, raw=True) == ERR_NULL and combine(w=null) == ERR_NULL and combine(out=null) == ERR_NULL
    assert combine(gl=[g[0], null, g[2]]) == ERR_NULL            # a NULL entry of the pointer list
    assert combine(c=0) == ERR_SHAPE and combine(c=9, gl=g) == ERR_SHAPE
    assert combine(out=g[1]) == ERR_SHAPE                        # out aliases a gradient
    assert combine(out=at(64 + 16 * 2 + 8)) == ERR_SHAPE         # ... or overlaps one
    assert combine(gl=[g[0], off, g[2]]) == ERR_ALIGN and combine(out=off) == ERR_ALIGN
    assert combine(n=0) == 0 and combine(n=0, out=g[1]) == 0
    assert combine(c=1, gl=g[:1], n=0) == 0 and combine(c=8, gl=g[:8], n=0) == 0

    for z in (x0, null):                                         # both forms of the fused step
        assert step(x=null, x0=z) == ERR_NULL and step(out=null, x0=z) == ERR_NULL and step(w=null, x0=z) == ERR_NULL
        assert step(gl=null, raw=True, x0=z) == ERR_NULL and step(gl=[null, g[1], g[2]], x0=z) == ERR_NULL
        assert step(mode=3, x0=z) == ERR_NULL                    # a range check needs a flag
        assert step(c=0, x0=z) == ERR_SHAPE and step(c=9, gl=g, x0=z) == ERR_SHAPE
        assert step(out=g[2], x0=z) == ERR_SHAPE                 # out aliases a gradient
        assert step(out=at(8), x0=z) == ERR_SHAPE                # out overlaps x without being x
        assert step(x=off, x0=z) == ERR_ALIGN and step(out=off, x0=z) == ERR_ALIGN
        assert step(gl=[g[0], g[1], off], x0=z) == ERR_ALIGN
        assert step(n=0, x0=z) == 0 and step(n=0, mode=3, flag=m, x0=z) == 0
        assert step(out=x, n=0, x0=z) == 0                       # out may alias x ...
    assert step(out=x0) == ERR_SHAPE                             # ... but not the centre of the eps-ball
    assert step(x0=off) == ERR_ALIGN


def test_kernel_source_table_knows_the_new_kernels():
    from vqattack_amd import build
    assert "si.hip" in build.SOURCES and len(set(build.SOURCES)) == len(build.SOURCES)
    keys = [k for k, _ in build.KERNEL_SOURCES]
    for name in ("void vqa::grad_fold_vec_kernel<false, 2, 5, 1, 4>(float __vector(4) const*, float __vector(4) const*, "
                 "float __vector(4) const*, vqa::GradList, float __vector(4)*, unsigned long, vqa::StepParams, int*)",
                 "void vqa::grad_fold_scalar_kernel<false, 0, 3>(float const*, float const*, float const*, vqa::GradList, "
                 "float*, unsigned long, vqa::StepParams, int*)",
                 "void vqa::si_copies_vec_kernel<5, true, 2, 0>(float __vector(4) const*, float __vector(4) const*, "
                 "float __vector(4)*, unsigned long, unsigned long, vqa::Scales, float)",
                 "void vqa::si_copies_scalar_kernel<1, false>(float const*, float const*, float*, unsigned long, "
                 "unsigned long, vqa::Scales, float)"):
        first = next(f for k, f in build.KERNEL_SOURCES if k in name)          # the FIRST key that matches decides
        assert first == "si.hip", (name, first)
        assert build.kernel_source_digest(name) not in (None, build.kernel_source_digest("vqa::ti_kernel<32, 15, 2>"))
    assert len(set(keys)) == len(keys)


def test_entry_points_accept_the_keys():
    entry = os.path.join(ROOT, "entry")
    sys.path.insert(0, entry)
    try:
        mods = {}
        for name in ("run", "VQA"):
            spec = importlib.util.spec_from_file_location("vqattack_entry_si_" + name, os.path.join(entry, name + ".py"))
            mods[name] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[name])
    finally:
        sys.path.remove(entry)
    cfg = mods["run"].parse([])
    assert cfg["si_copies"] is None and cfg["nesterov"] is False
    cfg = mods["run"].parse(["with", "tiny", "si_copies=5", "nesterov=true", "decay_factor=1.0"])
    assert cfg["si_copies"] == 5 and isinstance(cfg["si_copies"], int) and cfg["nesterov"] is True
    assert mods["run"].parse(["nesterov=false"])["nesterov"] is False
    with pytest.raises(SystemExit):
        mods["run"].parse(["si_copeis=5"])
    args = mods["VQA"].parse([])[0]
    assert args.si_copies is None and args.nesterov is False
    args = mods["VQA"].parse(["--si_copies", "3", "--nesterov", "--decay_factor", "0.9"])[0]
    assert (args.si_copies, args.nesterov) == (3, True)
    for name in ("run.py", "VQA.py"):                             # ... and hand them to the attack's configuration
        text = open(os.path.join(entry, name)).read()
        for key in ("si_copies", "nesterov"):
            assert re.search(r"AttackConfig\([^)]*" + key + "=", text, flags=re.S), (name, key)
