"""Variance tuning (VMI / VNI-FGSM): everything that needs no GPU -- validation, configuration, ABI, entry points and
the numpy Philox4x32-10 restatement the GPU tests compare the kernels with (against the known answers)."""
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
NAMES = ("vqa_vt_max_chunk", "vqa_vt_neighbors", "vqa_vt_accumulate", "vqa_vt_tune", "vqa_linf_vt_step")
BAD = (dict(vt_neighbors=0), dict(vt_neighbors=65), dict(vt_neighbors=True), dict(vt_neighbors=2.0),
       dict(vt_neighbors="3"), dict(vt_neighbors=2, vt_beta=0.0), dict(vt_neighbors=2, vt_beta=-1.0),
       dict(vt_neighbors=2, vt_beta=float("nan")), dict(vt_neighbors=2, vt_beta=float("inf")),
       dict(vt_neighbors=2, vt_beta="1.5"), dict(vt_neighbors=2, vt_seed=-1), dict(vt_neighbors=2, vt_seed=1 << 64),
       dict(vt_neighbors=2, vt_seed=1.0), dict(vt_neighbors=2, vt_seed=True))
GOOD = (dict(), dict(vt_neighbors=None), dict(vt_neighbors=1), dict(vt_neighbors=64), dict(vt_neighbors=20, vt_beta=1.5),
        dict(vt_neighbors=np.int64(3), vt_beta=np.float32(0.5), vt_seed=(1 << 64) - 1), dict(vt_neighbors=2, vt_seed=0),
        dict(vt_beta=-1.0), dict(vt_seed=-5), dict(vt_neighbors=None, vt_beta="x", vt_seed="y"))     # harmless when off


def test_validate_vt():
    assert attacks._validate_vt(None) is None and attacks._validate_vt(None, -1.0, "x") is None
    assert attacks._validate_vt(20) == (20, 1.5, None)
    assert attacks._validate_vt(np.int32(3), 2, 7) == (3, 2.0, 7)
    assert attacks._validate_vt(1, 0.25, (1 << 64) - 1) == (1, 0.25, (1 << 64) - 1)
    for bad in BAD:
        with pytest.raises(ValueError):
            attacks._validate_vt(**bad)


def _unreachable(_):
    raise AssertionError("model_fn must not run: the arguments are refused first")


@pytest.mark.parametrize("call", ["pgd", "pgd_vl", "mim"])
def test_operators_validate_the_vt_keys_before_any_tensor(call):
    x = torch.zeros(2, 3, 4, 4)                                  # a CPU tensor: refused, but only after the arguments
    y = [x, x]

    def run(norm=np.inf, **kw):
        if call == "pgd":
            return vqattack_amd.projected_gradient_descent(_unreachable, x, 0.1, 0.01, 2, norm, y=y, ori_x=x, ls=1, **kw)
        if call == "pgd_vl":
            return vqattack_amd.projected_gradient_descent_vl(_unreachable, [x, x], 0.1, 0.01, 2, norm, y=y, ori_x=x,
                                                              ls=1, **kw)
        return vqattack_amd.momentum_iterative_method(_unreachable, x, 0.1, 0.01, 2, norm, y=y, **kw)

    for bad in BAD:
        with pytest.raises(ValueError):
            run(**bad)
        with pytest.raises(ValueError):
            run(norm=2, **bad)
    for kw in GOOD:
        with pytest.raises(HipExtensionError):                   # fine: the CPU tensor is what is refused
            run(**kw)


def test_one_step_operators_do_not_take_the_keys():
    """With one step and v = 0 variance tuning would be a no-op."""
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(TypeError):
        vqattack_amd.fast_gradient_method(_unreachable, x, 0.1, np.inf, x, y=[x, x], ls=1, vt_neighbors=2)
    with pytest.raises(TypeError):
        vqattack_amd.fast_gradient_method_vl(_unreachable, [x, x], 0.1, np.inf, x, y=[x, x], ls=1, vt_neighbors=2)


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_the_keywords_reach_the_dropin_bindings(flavor):
    ns = dropin.load(flavor)
    x = torch.zeros(2, 3, 4, 4)
    for bound in (ns.projected_gradient_descent.projected_gradient_descent,
                  ns.momentum_iterative_method.momentum_iterative_method):
        with pytest.raises(ValueError):
            bound(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x, ls=1, vt_neighbors=65)
        with pytest.raises(HipExtensionError):
            bound(_unreachable, x, 0.1, 0.01, 2, np.inf, y=[x, x], ori_x=x, ls=1, vt_neighbors=20, vt_beta=1.5, vt_seed=3)
    with pytest.raises(ValueError):
        ns.projected_gradient_descent_vl.projected_gradient_descent(_unreachable, [x, x], 0.1, 0.01, 2, np.inf, y=[x, x],
                                                                    ori_x=x, ls=1, vt_neighbors=0)


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    g = torch.zeros(2, 3, 4, 4)
    key = torch.zeros(3, dtype=torch.uint32)
    for cpu in (lambda: ops.vt_neighbors(g, key, 2, 0.1), lambda: ops.vt_accumulate([g], g.clone(), True),
                lambda: ops.vt_tune(g, g.clone(), g.clone(), 0.5),
                lambda: ops.linf_vt_step(g, g.clone(), g.clone(), g.clone(), g.clone(), 0.5, 0.01, 0.1, -1.0, 1.0)):
        with pytest.raises(HipExtensionError):
            cpu()
    for bad in (lambda: ops.vt_neighbors(g, key, 0, 0.1), lambda: ops.vt_neighbors(g, key, 9, 0.1),
                lambda: ops.vt_accumulate([], g, True), lambda: ops.vt_accumulate([g] * 9, g, True),
                lambda: ops.vt_key_table(-1, 2, "cpu"), lambda: ops.vt_key_table(1 << 64, 2, "cpu")):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.vt_accumulate(g, g, True)
    table = ops.vt_key_table((7 << 32) | 5, 3, "cpu")                    # the table itself is plain data
    assert table.dtype == torch.uint32 and table.shape == (3, 3)
    assert table.numpy().astype(np.int64).tolist() == [[5, 7, 0], [5, 7, 1], [5, 7, 2]]
    assert ops.VT_MAX_CHUNK == 8 == _hip.lib().vqa_vt_max_chunk() and ops.VT_MAX_NEIGHBORS == 64


def test_attack_config_takes_the_fields_and_the_mixed_driver_refuses_them():
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    c = AttackConfig()
    assert c.vt_neighbors is None and c.vt_beta == 1.5 and c.vt_seed is None
    c = AttackConfig(vt_neighbors=20, vt_beta=2.0, vt_seed=11, nesterov=True, decay_factor=1.0, si_copies=5)
    assert (c.vt_neighbors, c.vt_beta, c.vt_seed) == (20, 2.0, 11)
    for bad in BAD:
        with pytest.raises(ValueError):
            AttackConfig(**bad)
    with pytest.raises(ValueError, match="vt_neighbors"):
        AttackConfig(vt_neighbors=2, patch_layout=True)
    atk = object.__new__(BatchedVQAttack)                            # no model needed: the refusal comes first
    atk.cfg, atk.adapters = AttackConfig(vt_neighbors=2), object()
    with pytest.raises(ValueError, match="vt_neighbors"):
        atk.attack_mixed(None, None, None, None)


def test_header_declares_and_library_exports_the_five_symbols():
    text = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    assert re.search(r"#define\s+VQA_VT_MAX_CHUNK\s+8\b", text)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = ctypes.CDLL(_hip.LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", text), name
        assert name in _hip.SIGNATURES and hasattr(lib, name), name
    assert _hip.lib().vqa_abi_version() == 4                   # additive exports: the version stays
    assert _hip.lib().vqa_vt_max_chunk() == 8


def test_entry_points_validate_before_the_first_launch():
    """Every return code of the header's list, through the library on a machine without a GPU."""
    lib = _hip.lib()
    buf = (ctypes.c_float * 1024)()
    base = ctypes.cast(buf, ctypes.c_void_p).value
    at = lambda floats: ctypes.c_void_p(base + 4 * floats)      # noqa: E731
    x, m, x0, v, vsum, out = at(0), at(16), at(32), at(48), at(240), at(512)   # n = 16 floats each; out: 8 neighbours
    g = [at(64 + 16 * i) for i in range(9)]
    key = at(960)
    off = ctypes.c_void_p(base + 4 * 900 + 2)                    # not 4-byte aligned, and apart from all the others
    null = None

    def ptrs(entries):
        return (ctypes.c_void_p * len(entries))(*[e if e is None else e.value for e in entries])

    def near(x=x, m=null, out=out, n=16, stride=16, c=3, first=0, key=key):
        return lib.vqa_vt_neighbors(x, m, out, n, stride, c, first, 0, 0.1, 0.5, key, null)

    def acc(gl=g[:3], c=3, out=vsum, n=16, init=1, raw=False):
        return lib.vqa_vt_accumulate(gl if raw else ptrs(gl), c, out, n, init, null)

    def tune(g=g[0], vsum=vsum, v=v, out=out, n=16):
        return lib.vqa_vt_tune(g, vsum, v, out, n, 0.5, null)

    def step(x=x, g=g[0], vsum=vsum, v=v, x0=x0, out=out, n=16, mode=1, flag=null):
        return lib.vqa_linf_vt_step(x, g, vsum, v, x0, out, n, 0.5, 0.01, 0.1, -1.0, 1.0, mode, flag, null)

    for mm in (null, m):                                         # with and without the look-ahead
        assert near(x=null, m=mm) == ERR_NULL and near(out=null, m=mm) == ERR_NULL and near(key=null, m=mm) == ERR_NULL
        assert near(c=0, m=mm) == ERR_SHAPE and near(c=9, m=mm) == ERR_SHAPE and near(first=-1, m=mm) == ERR_SHAPE
        assert near(stride=15, m=mm) == ERR_SHAPE                # copy_stride < n
        assert near(out=x, m=mm) == ERR_SHAPE                    # out overlaps x
        assert near(x=at(512 + 40), m=mm) == ERR_SHAPE           # x inside the third neighbour
        assert near(key=at(512 + 20), m=mm) == ERR_SHAPE         # the key row inside the second neighbour
        assert near(x=off, m=mm) == ERR_ALIGN and near(out=off, m=mm) == ERR_ALIGN and near(key=off, m=mm) == ERR_ALIGN
        assert near(n=0, stride=0, m=mm) == 0 and near(n=0, m=mm) == 0               # empty: no launch
    assert near(m=at(512 + 16)) == ERR_SHAPE and near(m=off) == ERR_ALIGN

    assert acc(gl=null, raw=True) == ERR_NULL and acc(out=null) == ERR_NULL
    assert acc(gl=[g[0], null, g[2]]) == ERR_NULL                # a NULL entry of the pointer list
    assert acc(c=0) == ERR_SHAPE and acc(c=9, gl=g) == ERR_SHAPE
    assert acc(out=g[1]) == ERR_SHAPE and acc(out=at(64 + 16 * 2 + 8), init=0) == ERR_SHAPE   # sum aliases / overlaps a gradient
    assert acc(gl=[g[0], off, g[2]]) == ERR_ALIGN and acc(out=off) == ERR_ALIGN
    assert acc(n=0) == 0 and acc(c=8, gl=g[:8], n=0, init=0) == 0

    assert tune(g=null) == ERR_NULL and tune(vsum=null) == ERR_NULL and tune(v=null) == ERR_NULL and tune(out=null) == ERR_NULL
    assert tune(v=g[0]) == ERR_SHAPE and tune(v=vsum) == ERR_SHAPE and tune(out=v) == ERR_SHAPE and tune(out=vsum) == ERR_SHAPE
    assert tune(out=at(64 + 8)) == ERR_SHAPE                     # ghat overlaps g without being g
    assert tune(g=off) == ERR_ALIGN and tune(out=off) == ERR_ALIGN
    assert tune(n=0) == 0 and tune(out=g[0], n=0) == 0           # ghat may be g

    for z in (x0, null):                                         # both forms of the fused step
        assert step(x=null, x0=z) == ERR_NULL and step(out=null, x0=z) == ERR_NULL and step(v=null, x0=z) == ERR_NULL
        assert step(g=null, x0=z) == ERR_NULL and step(vsum=null, x0=z) == ERR_NULL
        assert step(mode=3, x0=z) == ERR_NULL                    # a range check needs a flag
        assert step(out=g[0], x0=z) == ERR_SHAPE and step(out=v, x0=z) == ERR_SHAPE and step(out=vsum, x0=z) == ERR_SHAPE
        assert step(out=at(8), x0=z) == ERR_SHAPE                # out overlaps x without being x
        assert step(v=x, x0=z) == ERR_SHAPE
        assert step(x=off, x0=z) == ERR_ALIGN and step(out=off, x0=z) == ERR_ALIGN and step(v=off, x0=z) == ERR_ALIGN
        assert step(n=0, x0=z) == 0 and step(n=0, mode=3, flag=m, x0=z) == 0
        assert step(out=x, n=0, x0=z) == 0                       # out may alias x ...
    assert step(out=x0) == ERR_SHAPE                             # ... but not the centre of the eps-ball
    assert step(x0=off) == ERR_ALIGN


def test_kernel_source_table_knows_the_new_kernels():
    from vqattack_amd import build
    assert "vt.hip" in build.SOURCES and len(set(build.SOURCES)) == len(build.SOURCES)
    keys = [k for k, _ in build.KERNEL_SOURCES]
    for name in ("void vqa::vt_neighbors_vec_kernel<8, true, 2, 0>(float __vector(4) const*, float __vector(4) const*, "
                 "float __vector(4)*, unsigned long, unsigned long, unsigned int, unsigned long, float, float, unsigned int const*)",
                 "void vqa::vt_neighbors_scalar_kernel<1, false>(float const*, float const*, float*, unsigned long, "
                 "unsigned long, unsigned int, unsigned long, float, float, unsigned int const*)",
                 "void vqa::vt_accumulate_vec_kernel<8, false, 1, 0>(vqa::VtGrads, float __vector(4)*, unsigned long)",
                 "void vqa::vt_accumulate_scalar_kernel<3, true>(vqa::VtGrads, float*, unsigned long)",
                 "void vqa::vt_tune_vec_kernel<2, 1, 4>(float __vector(4) const*, float __vector(4) const*, "
                 "float __vector(4) const*, float __vector(4)*, float __vector(4) const*, float __vector(4)*, unsigned long, "
                 "float, vqa::StepParams, int*)",
                 "void vqa::vt_tune_scalar_kernel<0>(float const*, float const*, float const*, float*, float const*, float*, "
                 "unsigned long, float, vqa::StepParams, int*)"):
        first = next(f for k, f in build.KERNEL_SOURCES if k in name)          # the FIRST key that matches decides
        assert first == "vt.hip", (name, first)
        assert build.kernel_source_digest(name) not in (None, build.kernel_source_digest("vqa::si_copies_vec_kernel<1>"))
    assert len(set(keys)) == len(keys)


def test_entry_points_accept_the_keys():
    entry = os.path.join(ROOT, "entry")
    sys.path.insert(0, entry)
    try:
        mods = {}
        for name in ("run", "VQA"):
            spec = importlib.util.spec_from_file_location("vqattack_entry_vt_" + name, os.path.join(entry, name + ".py"))
            mods[name] = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mods[name])
    finally:
        sys.path.remove(entry)
    cfg = mods["run"].parse([])
    assert cfg["vt_neighbors"] is None and cfg["vt_beta"] == 1.5 and cfg["vt_seed"] is None
    cfg = mods["run"].parse(["with", "tiny", "vt_neighbors=20", "vt_beta=2.5", "vt_seed=7"])
    assert cfg["vt_neighbors"] == 20 and isinstance(cfg["vt_neighbors"], int)
    assert cfg["vt_beta"] == 2.5 and cfg["vt_seed"] == 7 and isinstance(cfg["vt_seed"], int)
    with pytest.raises(SystemExit):
        mods["run"].parse(["vt_neighbours=5"])
    args = mods["VQA"].parse([])[0]
    assert args.vt_neighbors is None and args.vt_beta == 1.5 and args.vt_seed is None
    args = mods["VQA"].parse(["--vt_neighbors", "20", "--vt_beta", "2.5", "--vt_seed", "7"])[0]
    assert (args.vt_neighbors, args.vt_beta, args.vt_seed) == (20, 2.5, 7)
    for name in ("run.py", "VQA.py"):                             # ... and hand them to the attack's configuration
        text = open(os.path.join(entry, name)).read()
        for key in ("vt_neighbors", "vt_beta", "vt_seed"):
            assert re.search(r"AttackConfig\([^)]*" + key + "=", text, flags=re.S), (name, key)


# ------------------------------------------------------------------------------------------------ the yardstick
def test_numpy_philox_reproduces_the_known_answers():
    """The restatement the GPU tests compare the kernels with, against the three known answers of Philox4x32-10 (counter
    | key | output), independently of the product."""
    from tests.test_vt_kernels import _noise_np, philox4x32_10
    cases = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
              (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))
    for counter, key, want in cases:
        assert tuple(int(w) for w in philox4x32_10(counter, key)) == want
    # vectorised over the counter as the tests use it: three blocks at once equal three single calls
    got = philox4x32_10((np.array([0, 0xffffffff, 0x243f6a88], dtype=np.uint64), np.array([0, 0xffffffff, 0x85a308d3],
                        dtype=np.uint64), np.array([0, 0xffffffff, 0x13198a2e], dtype=np.uint64),
                         np.array([0, 0xffffffff, 0x03707344], dtype=np.uint64)),
                        (np.array([0, 0xffffffff, 0xa4093822], dtype=np.uint64),
                         np.array([0, 0xffffffff, 0x299f31d0], dtype=np.uint64)))
    assert [tuple(int(w[i]) for w in got) for i in range(3)] == [c[2] for c in cases]
    # word -> value: word e % 4 of block e // 4 belongs to element e; zero key, t = i = 0: the first known answer
    r = _noise_np((5,), 0, 0, 0, 0.25)
    u = [np.float32(w >> 8) * np.float32(2.0 ** -24) for w in cases[0][2]]
    assert r.dtype == np.float32 and [float(v) for v in r[:4]] == [float((v * 2 - 1) * np.float32(0.25)) for v in u]
    assert np.all(_noise_np((4099,), 12345, 3, 1, 0.045) >= -np.float32(0.045))
    assert np.all(_noise_np((4099,), 12345, 3, 1, 0.045) < np.float32(0.045))
