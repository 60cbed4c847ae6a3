"""The three momentum (MI-FGSM) kernels on the MI355X.

Arithmetic under test, per sample b of n elements (include/vqattack_hip.h):
    den_b = max(1e-12f, sumabs[b] / (float)n);   m <- decay * m + g / den_b        (fp32, one rounding per operation)
and then vqa_linf_step / vqa_linf_fgm with m in place of g.  The sum is compared with fp64 at the project's bar for
per-sample norms; everything behind the sum is compared BITWISE -- with the numpy fp32 chain for the accumulate, with the
two-launch form (accumulate, then the existing L-inf kernel) for the fused step.

Shapes: (3,3,5,7) n % 4 != 0: scalar path, sample boundaries inside 16-byte groups; (2,3,64,64) three reduction chunks and
three whole tiles; (2,4100) vector path with one whole and one partial tile; "offset" the same from a view one float off
16-byte alignment: scalar path; (3100,8200) more samples than the grid has workgroups: ONE workgroup per sample walks two
whole tiles and the partial one; (64,3,592,592) 269 MB per tensor: the non-temporal stores of a result larger than the
Infinity Cache.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NORM_RTOL = 2e-6          # the project's bar on per-sample norms vs fp64; the two-stage fp32 sum emulated on the CPU for
#                           1..108 chunks is off by at most 3.1e-7 at 3 * 384 * 384 normal draws (about 6x room)
SMALL = ["3x3x5x7", "2x3x64x64", "2x4100", "offset"]
PARTIAL = SMALL + ["2x11276"]          # 2819 16-byte pieces per row: a partial tile with whole slots and 3 lanes
_SHAPES = {"3x3x5x7": (3, 3, 5, 7), "2x3x64x64": (2, 3, 64, 64), "2x4100": (2, 4100), "offset": (2, 4100),
           "2x11276": (2, 11276)}
_cache = {}


def _place(a, name):
    """Host array -> device tensor; the ``offset`` case lives one float behind a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if name != "offset":
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def _data(name):
    """x0 in [-1, 1], x inside its 0.05-ball, normal-draw gradient and momentum -- computed once per shape, never changed."""
    if name not in _cache:
        shape = _SHAPES[name]
        r = np.random.RandomState(len(name) + shape[-1])
        x0 = r.uniform(-1, 1, shape).astype(np.float32)
        x = np.clip(x0 + r.uniform(-0.05, 0.05, shape).astype(np.float32), -1, 1).astype(np.float32)
        g = (r.standard_normal(shape) * 1e-3).astype(np.float32)
        m = r.standard_normal(shape).astype(np.float32)
        host = dict(x=x, x0=x0, g=g, m=m)
        _cache[name] = (host, {k: _place(v, name) for k, v in host.items()})
    return _cache[name]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------------------------------------ sum of |g|
@pytest.mark.parametrize("name", SMALL)
def test_sumabs_matches_fp64_and_is_reproducible(name):
    from vqattack_amd import ops
    host, dev = _data(name)
    got = ops.sumabs_per_sample(dev["g"])
    want = np.abs(host["g"].astype(np.float64)).reshape(host["g"].shape[0], -1).sum(axis=1)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want) / want
    print("sumabs", name, "relative error vs fp64:", err)
    assert got.shape == (host["g"].shape[0],) and got.dtype == torch.float32
    assert np.all(err <= NORM_RTOL), err
    assert _same_bits(got, ops.sumabs_per_sample(dev["g"]))                  # no atomics: the same bits every run
    out = torch.full_like(got, -1.0)
    ws = ops.reduce_workspace(dev["g"])
    assert ops.sumabs_per_sample(dev["g"], out=out, ws=ws) is out and _same_bits(out, got)   # caller's buffers, as is


@pytest.mark.parametrize("name", SMALL)
def test_sumabs_is_exact_on_small_integers(name):
    from vqattack_amd import ops
    shape = _SHAPES[name]
    ints = np.random.RandomState(5).randint(-8, 9, shape).astype(np.float32)  # every partial sum < 2^24: exact in fp32
    got = ops.sumabs_per_sample(_place(ints, name)).cpu().numpy()
    assert np.array_equal(got, np.abs(ints).reshape(shape[0], -1).sum(axis=1).astype(np.float32))


def test_sumabs_of_an_empty_batch_and_a_full_size_image_batch():
    from vqattack_amd import ops
    assert ops.sumabs_per_sample(torch.empty(0, 8, device=DEV)).shape == (0,)
    g = torch.randn(2, 3, 384, 384, device=DEV, generator=torch.Generator(DEV).manual_seed(1))   # 108 chunks per sample
    want = g.double().abs().sum(dim=(1, 2, 3))
    err = ((ops.sumabs_per_sample(g).double() - want).abs() / want).cpu().numpy()
    print("sumabs 2x3x384x384 relative error vs fp64:", err)
    assert np.all(err <= NORM_RTOL), err


# ------------------------------------------------------------------------------------------------ accumulate
def _chain(g, m, sumabs, decay):
    """The numpy fp32 chain of the issue: one rounding per operation, fed the device's own sum."""
    n = np.float32(g[0].size)
    den = np.maximum(np.float32(1e-12), sumabs.astype(np.float32) / n).astype(np.float32)
    den = den.reshape((-1,) + (1,) * (g.ndim - 1))
    out = np.float32(decay) * m + g / den
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("decay", [1.0, 0.9, 0.0])
@pytest.mark.parametrize("name", PARTIAL)
def test_accumulate_equals_the_numpy_fp32_chain_bitwise(name, decay):
    from vqattack_amd import ops
    host, dev = _data(name)
    sums = ops.sumabs_per_sample(dev["g"])
    m = _place(host["m"], name)
    assert ops.momentum_accumulate(dev["g"], m, decay, sumabs=sums) is m          # in place
    want = _chain(host["g"], host["m"], sums.cpu().numpy(), decay)
    assert np.array_equal(m.cpu().numpy().view(np.int32), want.view(np.int32))
    m2 = _place(host["m"], name)
    ops.momentum_accumulate(dev["g"], m2, decay)                                  # the sum computed by the wrapper
    assert _same_bits(m, m2)


@pytest.mark.parametrize("name", SMALL)
def test_a_zero_gradient_sample_only_decays(name):
    from vqattack_amd import ops
    host, dev = _data(name)
    g = host["g"].copy()
    g[1] = 0.0
    m = _place(host["m"], name)
    ops.momentum_accumulate(_place(g, name), m, 0.75)
    assert np.array_equal(m[1].cpu().numpy(), np.float32(0.75) * host["m"][1])
    assert not np.array_equal(m[0].cpu().numpy(), np.float32(0.75) * host["m"][0])


# ------------------------------------------------------------------------------------------------ fused step
def _two_launches(ops, t, m, decay, sums, with_x0, clip, out=None, flag=None):
    lo, hi = (-1.0, 1.0) if clip else (None, None)
    ops.momentum_accumulate(t["g"], m, decay, sumabs=sums)
    if with_x0:
        return ops.linf_step(t["x"] if out is None else out, m, t["x0"], 0.01, 0.05, lo, hi, flag=flag, out=out)
    return ops.linf_fgm(t["x"] if out is None else out, m, 0.01, lo, hi, flag=flag, out=out)


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("with_x0", [True, False])
@pytest.mark.parametrize("name", PARTIAL)
def test_fused_step_equals_accumulate_then_linf_kernel_bitwise(name, with_x0, clip, in_place):
    from vqattack_amd import ops
    host, dev = _data(name)
    lo, hi = (-1.0, 1.0) if clip else (None, None)
    sums = ops.sumabs_per_sample(dev["g"])
    m_ref, m_fused = _place(host["m"], name), _place(host["m"], name)
    x_ref = _place(host["x"], name) if in_place else None
    want = _two_launches(ops, dev, m_ref, 0.9, sums, with_x0, clip, out=x_ref)
    x_fused = _place(host["x"], name) if in_place else dev["x"]
    got = ops.linf_momentum_step(x_fused, dev["g"], dev["x0"] if with_x0 else None, m_fused, 0.9, 0.01, 0.05, lo, hi,
                                 out=x_fused if in_place else None, sumabs=sums)
    assert (got is x_fused) == in_place
    assert _same_bits(m_fused, m_ref) and _same_bits(got, want)
    assert not _same_bits(m_fused, dev["m"])                                     # the momentum really moved
    assert np.array_equal(dev["x"].cpu().numpy(), host["x"])                     # the shared inputs are never written
    if with_x0:
        assert float((got - dev["x0"]).abs().max()) <= 0.05 + 1e-6
        assert float((got - dev["x0"]).abs().max()) > 0.05 - 1e-6                # the projection acted
    assert float((got - dev["x"]).abs().max()) > 0


@pytest.mark.parametrize("with_x0", [True, False])
@pytest.mark.parametrize("name", SMALL)
def test_decay_zero_is_the_plain_linf_kernel(name, with_x0):
    """decay = 0 with any finite momentum: m becomes g / den, whose sign is g's -- the step without momentum, bit for bit."""
    from vqattack_amd import ops
    host, dev = _data(name)
    m = _place(host["m"], name)
    got = ops.linf_momentum_step(dev["x"], dev["g"], dev["x0"] if with_x0 else None, m, 0.0, 0.01, 0.05, -1.0, 1.0)
    want = ops.linf_step(dev["x"], dev["g"], dev["x0"], 0.01, 0.05, -1.0, 1.0) if with_x0 else \
        ops.linf_fgm(dev["x"], dev["g"], 0.01, -1.0, 1.0)
    assert _same_bits(got, want)


@pytest.mark.parametrize("with_x0", [True, False])
@pytest.mark.parametrize("name", SMALL)
def test_range_flag_is_set_exactly_when_an_input_is_outside_the_clip_range(name, with_x0):
    from vqattack_amd import ops
    from vqattack_amd._hip import VQA_FLAG_RANGE
    host, dev = _data(name)
    x0 = dev["x0"] if with_x0 else None
    flag = ops.new_flag(DEV)
    ops.linf_momentum_step(dev["x"], dev["g"], x0, _place(host["m"], name), 1.0, 0.01, 0.05, -1.0, 1.0, flag=flag)
    assert int(flag.item()) == 0
    for where, value in ((0, 1.5), (-1, -1.0000001), (host["x"].size // 2, float("nan"))):
        x = host["x"].copy()
        x.reshape(-1)[where] = value                                             # ONE element outside, first / last / middle
        flag = ops.new_flag(DEV)
        ops.linf_momentum_step(_place(x, name), dev["g"], x0, _place(host["m"], name), 1.0, 0.01, 0.05, -1.0, 1.0,
                               flag=flag)
        assert int(flag.item()) == VQA_FLAG_RANGE, (where, value)
    flag = ops.new_flag(DEV)                                                     # no clip range: nothing to check
    x = host["x"].copy()
    x.reshape(-1)[0] = 7.0
    ops.linf_momentum_step(_place(x, name), dev["g"], x0, _place(host["m"], name), 1.0, 0.01, 0.05, None, None, flag=flag)
    assert int(flag.item()) == 0


@pytest.mark.parametrize("shape", [(3100, 8200), (64, 3, 592, 592)], ids=["3100x8200", "64x3x592x592"])
@pytest.mark.parametrize("in_place", [False, True])
def test_fused_step_on_the_large_shapes(shape, in_place):
    """(3100, 8200): the grid has one workgroup per sample, which walks two whole tiles and the partial one.
    (64, 3, 592, 592): 269 MB per tensor, past the Infinity-Cache size at which the result is stored non-temporally."""
    from vqattack_amd import ops
    gen = torch.Generator(DEV).manual_seed(shape[0])
    x0 = torch.empty(shape, device=DEV).uniform_(-1, 1, generator=gen)
    x = (x0 + torch.empty(shape, device=DEV).uniform_(-0.05, 0.05, generator=gen)).clamp_(-1, 1)
    g = torch.randn(shape, device=DEV, generator=gen) * 1e-3
    m = torch.randn(shape, device=DEV, generator=gen)
    sums = ops.sumabs_per_sample(g)
    want64 = g.double().abs().sum(dim=tuple(range(1, g.dim())))
    assert float(((sums.double() - want64).abs() / want64).max()) <= NORM_RTOL
    m_ref, m_fused = m.clone(), m.clone()
    x_ref, x_fused = (x.clone(), x.clone()) if in_place else (None, x)
    want = _two_launches(ops, dict(x=x, g=g, x0=x0), m_ref, 0.9, sums, True, True, out=x_ref)
    got = ops.linf_momentum_step(x_fused, g, x0, m_fused, 0.9, 0.01, 0.05, -1.0, 1.0, out=x_fused if in_place else None,
                                 sumabs=sums)
    assert _same_bits(m_fused, m_ref) and _same_bits(got, want)
    assert not torch.equal(m_fused, m)


def test_wrappers_check_shapes_and_empty_tensors():
    from vqattack_amd import ops
    g = torch.zeros(2, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.momentum_accumulate(g, torch.zeros(2, 4, device=DEV), 1.0)
    with pytest.raises(ValueError):
        ops.linf_momentum_step(g, g, torch.zeros(2, 4, device=DEV), g.clone(), 1.0, 0.01, 0.1, -1.0, 1.0)
    with pytest.raises(ValueError):
        ops.linf_momentum_step(g, g, None, g.clone(), 1.0, 0.01, 0.1, -1.0, 1.0, sumabs=torch.zeros(3, device=DEV))
    with pytest.raises(ValueError):
        ops.sumabs_per_sample(g, out=torch.zeros(5, device=DEV))
    empty = torch.empty(0, 8, device=DEV)
    assert ops.momentum_accumulate(empty, empty.clone(), 1.0).shape == (0, 8)
    assert ops.linf_momentum_step(empty, empty, None, empty.clone(), 1.0, 0.01, 0.1, -1.0, 1.0).shape == (0, 8)
