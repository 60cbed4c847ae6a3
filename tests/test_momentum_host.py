"""Host side of the momentum (MI-FGSM) feature: C ABI, drop-in modules, argument validation, configuration keys.
Everything here runs without a GPU."""
import ctypes
import importlib
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

import vqattack_amd
from vqattack_amd import _hip, dropin
from vqattack_amd._hip import HipExtensionError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("vqa_sumabs_per_sample", "vqa_momentum_accumulate", "vqa_linf_momentum_step")


def test_header_declares_and_library_exports_the_three_entry_points():
    text = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    assert _hip.lib().vqa_abi_version() == 4                   # additive exports: the version stays


def test_entry_points_validate_before_the_first_launch():
    lib = _hip.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    off = ctypes.c_void_p(p.value + 2)                           # not 4-byte aligned
    null = None
    ERR_NULL, ERR_SHAPE, ERR_ALIGN = -1, -2, -3
    # sumabs(g, out, batch, n_per, ws, stream)
    assert lib.vqa_sumabs_per_sample(null, p, 2, 8, p, null) == ERR_NULL
    assert lib.vqa_sumabs_per_sample(p, null, 2, 8, p, null) == ERR_NULL
    assert lib.vqa_sumabs_per_sample(p, p, 2, 8, null, null) == ERR_NULL           # workspace missing
    assert lib.vqa_sumabs_per_sample(p, p, 70000, 4, p, null) == ERR_SHAPE         # batch > 65535
    assert lib.vqa_sumabs_per_sample(p, p, -1, 4, p, null) == ERR_SHAPE
    assert lib.vqa_sumabs_per_sample(off, p, 2, 8, p, null) == ERR_ALIGN
    assert lib.vqa_sumabs_per_sample(p, p, 0, 8, p, null) == 0                     # empty: no launch
    # accumulate(g, sumabs, m, batch, n_per, decay, stream)
    assert lib.vqa_momentum_accumulate(null, p, p, 2, 8, 1.0, null) == ERR_NULL
    assert lib.vqa_momentum_accumulate(p, null, p, 2, 8, 1.0, null) == ERR_NULL
    assert lib.vqa_momentum_accumulate(p, p, null, 2, 8, 1.0, null) == ERR_NULL
    assert lib.vqa_momentum_accumulate(p, p, p, 65536, 8, 1.0, null) == ERR_SHAPE
    assert lib.vqa_momentum_accumulate(p, p, off, 2, 8, 1.0, null) == ERR_ALIGN
    assert lib.vqa_momentum_accumulate(p, p, p, 2, 0, 1.0, null) == 0
    # step(x, g, sumabs, x0, m, out, batch, n_per, decay, eps_iter, eps, cmin, cmax, mode, flag, stream)
    tail = (2, 8, 1.0, 0.01, 0.1, -1.0, 1.0)
    assert lib.vqa_linf_momentum_step(null, p, p, p, p, p, *tail, 1, null, null) == ERR_NULL
    assert lib.vqa_linf_momentum_step(p, null, p, p, p, p, *tail, 1, null, null) == ERR_NULL
    assert lib.vqa_linf_momentum_step(p, p, null, p, p, p, *tail, 1, null, null) == ERR_NULL
    assert lib.vqa_linf_momentum_step(p, p, p, p, null, p, *tail, 1, null, null) == ERR_NULL
    assert lib.vqa_linf_momentum_step(p, p, p, p, p, null, *tail, 1, null, null) == ERR_NULL
    assert lib.vqa_linf_momentum_step(p, p, p, p, p, p, *tail, 3, null, null) == ERR_NULL      # range check needs a flag
    assert lib.vqa_linf_momentum_step(p, p, p, null, p, p, *tail, 3, null, null) == ERR_NULL   # also without x0
    assert lib.vqa_linf_momentum_step(p, p, p, p, p, p, 70000, 8, 1.0, 0.01, 0.1, -1.0, 1.0, 1, null, null) == ERR_SHAPE
    assert lib.vqa_linf_momentum_step(p, p, p, off, p, p, *tail, 1, null, null) == ERR_ALIGN
    assert lib.vqa_linf_momentum_step(off, p, p, null, p, p, *tail, 1, null, null) == ERR_ALIGN
    assert lib.vqa_linf_momentum_step(p, p, p, null, p, p, 0, 8, 1.0, 0.01, 0.1, -1.0, 1.0, 1, null, null) == 0
    assert lib.vqa_linf_momentum_step(p, p, p, p, p, p, 2, 0, 1.0, 0.01, 0.1, -1.0, 1.0, 1, null, null) == 0


def test_kernel_source_table_knows_the_new_kernels():
    from vqattack_amd import build
    assert ("sumabs", "lnorm.hip") in build.KERNEL_SOURCES and ("momentum", "lnorm.hip") in build.KERNEL_SOURCES
    for kernel in ("vqa::sumabs_stage1<true>", "vqa::momentum_vec_kernel<2, 4, 4>", "vqa::momentum_scalar_kernel<0>"):
        assert build.kernel_source_digest(kernel) == build.kernel_source_digest("vqa::sumsq_stage1<true, false>")


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_dropin_module_path_binds_the_flavor(flavor):
    root = os.path.join(ROOT, "vqattack_amd", "dropin", flavor)

    def forget():
        for name in [m for m in sys.modules if m == "cleverhans" or m.startswith("cleverhans.")]:
            del sys.modules[name]
    forget()
    sys.path.insert(0, root)
    try:
        mim = importlib.import_module("cleverhans.torch.attacks.momentum_iterative_method")
        assert mim.momentum_iterative_method.keywords == {"flavor": flavor}
        assert mim.momentum_iterative_method.func is vqattack_amd.momentum_iterative_method
    finally:
        sys.path.remove(root)
        forget()
    bound = dropin.load(flavor).momentum_iterative_method.momentum_iterative_method
    assert bound.keywords == {"flavor": flavor} and bound.func is vqattack_amd.attacks.momentum_iterative_method


def _unreachable(_):
    raise AssertionError("model_fn must not run: the arguments are refused first")


@pytest.mark.parametrize("call", ["pgd", "pgd_vl", "mim"])
def test_validation_order(call):
    x = torch.zeros(2, 3, 4, 4)                                  # a CPU tensor: refused, but only after the arguments
    y = [x, x]

    def run(norm, decay, **kw):
        if call == "pgd":
            return vqattack_amd.projected_gradient_descent(_unreachable, x, 0.1, 0.01, 2, norm, y=y, ori_x=x, ls=1,
                                                           decay_factor=decay, **kw)
        if call == "pgd_vl":
            return vqattack_amd.projected_gradient_descent_vl(_unreachable, [x, x], 0.1, 0.01, 2, norm, y=y, ori_x=x,
                                                              ls=1, decay_factor=decay, **kw)
        return vqattack_amd.momentum_iterative_method(_unreachable, x, 0.1, 0.01, 2, norm, y=y, decay_factor=decay, **kw)

    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        with pytest.raises(NotImplementedError):                 # norm 1 stays the first check
            run(1, bad)
        with pytest.raises(ValueError):                          # before the CPU-tensor refusal
            run(np.inf, bad)
        with pytest.raises(ValueError):
            run(2, bad)
    with pytest.raises(NotImplementedError):
        run(1, 1.0)
    for good in (0.0, 1.0, 0.9):
        with pytest.raises(HipExtensionError):                   # a fine decay factor: the CPU tensor is what is refused
            run(np.inf, good)
    if call != "mim":
        with pytest.raises(HipExtensionError):                   # momentum off: today's behaviour
            run(np.inf, None, momentum=x)
    else:
        with pytest.raises(ValueError):                          # the method IS the momentum: None is not a decay factor
            run(np.inf, None)


def test_ops_refuse_cpu_tensors():
    from vqattack_amd import ops
    g = torch.zeros(2, 8)
    with pytest.raises(HipExtensionError):
        ops.sumabs_per_sample(g)
    with pytest.raises(HipExtensionError):
        ops.momentum_accumulate(g, g.clone(), 1.0)
    with pytest.raises(HipExtensionError):
        ops.linf_momentum_step(g, g, g, g.clone(), 1.0, 0.01, 0.1, -1.0, 1.0)
    with pytest.raises(TypeError):
        ops.sumabs_per_sample([0.0, 1.0])


def test_attack_config_takes_a_decay_factor_and_refuses_it_with_patch_layout():
    from vqattack_amd.attack.runner import AttackConfig
    assert AttackConfig().decay_factor is None
    assert AttackConfig(decay_factor=1.0).decay_factor == 1.0
    assert AttackConfig(patch_layout=True).patch_layout                      # still fine on its own
    with pytest.raises(ValueError):
        AttackConfig(decay_factor=1.0, patch_layout=True)
    with pytest.raises(ValueError):
        AttackConfig(decay_factor=-1.0)


def test_entry_points_accept_the_key():
    entry = os.path.join(ROOT, "entry")
    sys.path.insert(0, entry)
    try:
        mods = {}
        for name in ("run", "VQA"):
            spec = importlib.util.spec_from_file_location("vqattack_entry_" + name, os.path.join(entry, name + ".py"))
            mods[name] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[name])
    finally:
        sys.path.remove(entry)
    assert mods["run"].parse([])["decay_factor"] is None
    assert mods["run"].parse(["with", "tiny", "decay_factor=0.9"])["decay_factor"] == 0.9
    with pytest.raises(SystemExit):
        mods["run"].parse(["decay_factro=1"])
    assert mods["VQA"].parse([])[0].decay_factor is None
    assert mods["VQA"].parse(["--decay_factor", "0.9"])[0].decay_factor == 0.9
    for name in ("run.py", "VQA.py"):                             # ... and hand it to the attack's configuration
        assert re.search(r"AttackConfig\([^)]*decay_factor=", open(os.path.join(entry, name)).read(), flags=re.S), name
