"""The TI (translation-invariant) smoothing kernels on the MI355X: ``vqa_ti_smooth`` and both forms of ``vqa_linf_ti_step``.

The reference is a numpy fp32 chain written here (``_chain``): zero-padded shifts, one float32 multiply and one float32 add
per tap, taps in ascending order, rows then columns -- the contract of ``include/vqattack_hip.h``, independent of the
product and of torch's convolution.  It is followed by the numpy ``StepOp`` / ``FgmOp`` of ``csrc/common.hpp``.  The
kernels must give its bits.  The output tile is 64 wide and 32 high: the shapes below include exactly one tile, one
row / column more, several tiles in both directions, a plane smaller than the halo, widths that are no multiple of 4, and
tap counts of the unrolled (7, 15) and of the run-time (1, 3, 5, 31) loops.  References are computed once per case.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
EPS, EPS_ITER, LO, HI = 0.03, 0.01, -1.0, 1.0
_ASYM7 = np.array([0.31, -0.12, 0.05, 0.44, 0.02, 0.2, -0.07], dtype=np.float32)      # flipped kernel / swapped passes show
_ASYM5 = np.array([0.5, 0.1, -0.3, 0.25, 0.4], dtype=np.float32)

CASES = {
    "halo_only_k15": ((1, 3, 5, 9), 15),
    "odd_width_k15": ((2, 3, 37, 70), 15),
    "one_tile_k15": ((3, 1, 32, 64), 15),
    "tile_plus_one_k15": ((1, 1, 33, 65), 15),
    "k31": ((2, 3, 33, 65), 31),
    "k3": ((1, 2, 16, 16), 3),
    "k1": ((1, 2, 16, 16), 1),
    "asym_k7": ((2, 3, 96, 96), _ASYM7),
    "asym_k5": ((2, 3, 37, 70), _ASYM5),
}
_refs = {}


def _taps(k):
    from vqattack_amd import ops
    return ops.ti_gaussian_taps(k) if isinstance(k, int) else k


def _pass(a, w, axis):
    k, r, n = len(w), len(w) // 2, a.shape[axis]
    pad = [(0, 0)] * a.ndim
    pad[axis] = (r, r)
    ap = np.pad(a, pad)                                   # zeros outside the plane
    acc = np.zeros_like(a)                                # +0.0f
    for j in range(k):
        sl = [slice(None)] * a.ndim
        sl[axis] = slice(j, j + n)
        acc = acc + F(w[j]) * ap[tuple(sl)]               # one fp32 multiply, one fp32 add
    assert acc.dtype == np.float32
    return acc


def _chain(g, w):
    """(B, C, H, W) float32 -> smoothed gradient, float32: rows, then columns."""
    with np.errstate(all="ignore"):
        return _pass(_pass(g, w, 3), w, 2)


def _sign(g):
    return (g > 0).astype(np.float32) - (g < 0).astype(np.float32)      # torch.sign: sign(NaN) = 0


def _host_update(x, ghat, x0):
    """numpy fp32: StepOp (x0 given) or FgmOp (x0 None) of csrc/common.hpp."""
    a = np.clip(x + F(EPS_ITER) * _sign(ghat), F(LO), F(HI))
    if x0 is None:
        return a
    e = np.clip(a - x0, -F(EPS), F(EPS))
    out = np.clip(x0 + e, F(LO), F(HI))
    assert out.dtype == np.float32
    return out


def _inputs(shape, seed):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(shape) * np.exp(rng.standard_normal(shape) * 2.0)).astype(np.float32)   # log-normal scales
    x0 = rng.uniform(-1, 1, shape).astype(np.float32)
    x = np.clip(x0 + rng.uniform(-EPS, EPS, shape).astype(np.float32), F(LO), F(HI))
    return g, x, x0


def _case(name):
    """(taps, g, x, x0, ghat, step, fgm): inputs and the host references of a case, built once and never changed."""
    if name not in _refs:
        shape, k = CASES[name]
        w = _taps(k)
        g, x, x0 = _inputs(shape, sum(map(ord, name)))
        ghat = _chain(g, w)
        _refs[name] = (w, g, x, x0, ghat, _host_update(x, ghat, x0), _host_update(x, ghat, None))
    return _refs[name]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _assert_bits(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    same = np.mean(got.view(np.int32) == want.view(np.int32))
    assert same == 1.0, (what, same, np.nanmax(np.abs(got - want)))


# ------------------------------------------------------------------------------------------------ bitwise
@pytest.mark.parametrize("name", sorted(CASES))
def test_smooth_and_both_fused_steps_equal_the_host_chain_bitwise(name):
    from vqattack_amd import ops
    w, g, x, x0, ghat, step, fgm = _case(name)
    gd, xd, x0d = _dev(g), _dev(x), _dev(x0)
    _assert_bits(ops.ti_smooth(gd, w), ghat, "ti_smooth")
    _assert_bits(ops.linf_ti_step(xd, gd, x0d, w, EPS_ITER, EPS, LO, HI), step, "linf_ti_step")
    _assert_bits(ops.linf_ti_step(xd, gd, None, w, EPS_ITER, EPS, LO, HI), fgm, "linf_ti_step without x0")
    # ... and the fused step is the two-launch form
    two = ops.linf_step(xd, ops.ti_smooth(gd, w), x0d, EPS_ITER, EPS, LO, HI)
    assert torch.equal(two, ops.linf_ti_step(xd, gd, x0d, w, EPS_ITER, EPS, LO, HI))
    assert np.abs(step - x0).max() <= EPS + 1e-6 and not np.array_equal(step, fgm)


def test_one_tap_of_one_is_the_plain_step():
    from vqattack_amd import ops
    w, g, x, x0, ghat, step, fgm = _case("k1")
    assert np.array_equal(ghat, g + F(0))                        # the identity, -0 as +0
    gd, xd, x0d = _dev(g), _dev(x), _dev(x0)
    assert torch.equal(ops.linf_ti_step(xd, gd, x0d, w, EPS_ITER, EPS, LO, HI),
                       ops.linf_step(xd, gd, x0d, EPS_ITER, EPS, LO, HI))
    assert torch.equal(ops.linf_ti_step(xd, gd, None, w, EPS_ITER, EPS, LO, HI), ops.linf_fgm(xd, gd, EPS_ITER, LO, HI))
    neg0 = torch.full((1, 1, 4, 4), -0.0, device=DEV)
    assert not bool(torch.signbit(ops.ti_smooth(neg0, w)).any())


# ------------------------------------------------------------------------------------------------ containment
def _guarded(a, offset, fill):
    """``a`` as the interior ``big[1:-1]`` of a larger tensor whose outer samples (and the ``offset`` floats in front of
    it) hold ``fill``.  Returns (view, whole flat buffer)."""
    b = a.shape[0]
    n = a[0].size
    flat = torch.full((offset + (b + 2) * n,), fill, dtype=torch.float32, device=DEV)
    big = flat[offset:].view((b + 2,) + a.shape[1:])
    big[1:-1].copy_(torch.from_numpy(a))
    return big[1:-1], flat


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("name", ["odd_width_k15", "one_tile_k15", "k31"])
def test_no_access_outside_the_planes(name, offset):
    """NaN all around the inputs, a sentinel all around the output: a read outside a plane or the tensor would bring a NaN
    into the result, a write outside would change a sentinel."""
    from vqattack_amd import ops
    w, g, x, x0, ghat, step, fgm = _case(name)
    nan = float("nan")
    (gd, _), (xd, _), (x0d, _) = _guarded(g, offset, nan), _guarded(x, offset, nan), _guarded(x0, offset, nan)
    n = g[0].size
    for want, run in ((ghat, lambda o: ops.ti_smooth(gd, w, out=o)),
                      (step, lambda o: ops.linf_ti_step(xd, gd, x0d, w, EPS_ITER, EPS, LO, HI, out=o)),
                      (fgm, lambda o: ops.linf_ti_step(xd, gd, None, w, EPS_ITER, EPS, LO, HI, out=o))):
        od, oflat = _guarded(np.zeros_like(g), offset, 777.0)
        assert run(od) is od
        assert not bool(torch.isnan(od).any())
        _assert_bits(od, want, name)
        assert bool((oflat[:offset + n] == 777.0).all()) and bool((oflat[-n:] == 777.0).all())


@pytest.mark.parametrize("name", ["one_tile_k15", "asym_k7"])
def test_base_pointers_offset_by_one_float(name):
    """Widths that are multiples of 4 with every base pointer 4- but not 16-byte aligned."""
    from vqattack_amd import ops
    w, g, x, x0, ghat, step, fgm = _case(name)

    def shifted(a):
        flat = torch.zeros(a.size + 1, device=DEV)
        view = flat[1:].view(a.shape)
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 == 4
        return view
    gd, xd, x0d = shifted(g), shifted(x), shifted(x0)
    _assert_bits(ops.ti_smooth(gd, w, out=shifted(np.zeros_like(g))), ghat, "ti_smooth")
    _assert_bits(ops.linf_ti_step(xd, gd, x0d, w, EPS_ITER, EPS, LO, HI, out=shifted(np.zeros_like(g))), step, "step")
    _assert_bits(ops.linf_ti_step(xd, gd, None, w, EPS_ITER, EPS, LO, HI, out=shifted(np.zeros_like(g))), fgm, "fgm")
    # one misaligned pointer is enough to leave the 16-byte path
    _assert_bits(ops.linf_ti_step(_dev(x), _dev(g), x0d, w, EPS_ITER, EPS, LO, HI), step, "x0 alone")


# ------------------------------------------------------------------------------------------------ planes, non-finite
def test_a_plane_never_sees_its_neighbour():
    from vqattack_amd import ops
    w = _taps(15)
    rng = np.random.default_rng(3)
    g = (rng.standard_normal((1, 3, 40, 70)) * 1e-3).astype(np.float32)
    g[0, 1] = F(1e30)
    got = ops.ti_smooth(_dev(g), w).cpu().numpy()
    for c in (0, 2):
        alone = ops.ti_smooth(_dev(g[:, c:c + 1]), w).cpu().numpy()
        assert np.array_equal(got[:, c:c + 1].view(np.int32), alone.view(np.int32))
        assert np.abs(got[0, c]).max() < 1.0
    _assert_bits(torch.from_numpy(got), _chain(g, w), "whole tensor")


@pytest.mark.parametrize("k,pos", [(15, (20, 33)), (7, (1, 68)), (31, (36, 0))])
def test_one_nan_spreads_over_its_k_by_k_neighbourhood_only(k, pos):
    from vqattack_amd import ops
    w = _taps(k)
    g, x, x0 = _inputs((1, 2, 37, 70), 11)
    g[0, 1, pos[0], pos[1]] = np.nan
    r = k // 2
    want_nan = np.zeros(g.shape, dtype=bool)
    want_nan[0, 1, max(pos[0] - r, 0):pos[0] + r + 1, max(pos[1] - r, 0):pos[1] + r + 1] = True
    ref = _chain(g, w)
    assert np.array_equal(np.isnan(ref), want_nan)
    got = ops.ti_smooth(_dev(g), w).cpu().numpy()
    assert np.array_equal(np.isnan(got), want_nan)
    assert np.array_equal(got[~want_nan].view(np.int32), ref[~want_nan].view(np.int32))
    # the fused step takes sign(NaN) = 0 there, like sign_torch
    _assert_bits(ops.linf_ti_step(_dev(x), _dev(g), _dev(x0), w, EPS_ITER, EPS, LO, HI), _host_update(x, ref, x0), "step")
    _assert_bits(ops.linf_ti_step(_dev(x), _dev(g), None, w, EPS_ITER, EPS, LO, HI), _host_update(x, ref, None), "fgm")


# ------------------------------------------------------------------------------------------------ in place, flag, repeat
@pytest.mark.parametrize("name", ["odd_width_k15", "asym_k7"])
def test_in_place_update(name):
    from vqattack_amd import ops
    w, g, x, x0, ghat, step, fgm = _case(name)
    for want, x0d in ((step, _dev(x0)), (fgm, None)):
        xd = _dev(x)
        assert ops.linf_ti_step(xd, _dev(g), x0d, w, EPS_ITER, EPS, LO, HI, out=xd) is xd
        _assert_bits(xd, want, name)


@pytest.mark.parametrize("with_x0", [True, False])
def test_range_flag(with_x0):
    from vqattack_amd import _hip, ops
    w, g, x, x0, ghat, step, fgm = _case("odd_width_k15")
    gd, x0d = _dev(g), (_dev(x0) if with_x0 else None)
    flag = ops.new_flag(DEV)
    out = ops.linf_ti_step(_dev(x), gd, x0d, w, EPS_ITER, EPS, LO, HI, flag=flag)
    assert int(flag.item()) == 0
    _assert_bits(out, step if with_x0 else fgm, "with a flag")
    for bad_value in (1.5, float("nan")):
        bad = x.copy()
        bad[1, 2, 36, 69] = bad_value                            # the last element of a partial group of a partial tile
        flag = ops.new_flag(DEV)
        ops.linf_ti_step(_dev(bad), gd, x0d, w, EPS_ITER, EPS, LO, HI, flag=flag)
        assert int(flag.item()) == _hip.VQA_FLAG_RANGE
    flag = ops.new_flag(DEV)
    ops.linf_ti_step(_dev(x), gd, x0d, w, EPS_ITER, EPS, None, None, flag=flag)      # no clipping: no range to check
    assert int(flag.item()) == 0


def test_two_launches_give_the_same_bits():
    from vqattack_amd import ops
    w = _taps(15)
    g, x, x0 = _inputs((4, 3, 96, 130), 5)
    gd, xd, x0d = _dev(g), _dev(x), _dev(x0)
    assert torch.equal(ops.ti_smooth(gd, w), ops.ti_smooth(gd, w))
    a = ops.linf_ti_step(xd, gd, x0d, w, EPS_ITER, EPS, LO, HI)
    assert torch.equal(a, ops.linf_ti_step(xd, gd, x0d, w, EPS_ITER, EPS, LO, HI))


def test_wrappers_refuse_what_the_kernel_cannot_take():
    from vqattack_amd import ops
    w = _taps(15)
    g = torch.zeros(2, 3, 8, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.ti_smooth(g.view(6, 8, 8), w)                        # not 4-d
    with pytest.raises(ValueError):
        ops.ti_smooth(g.permute(0, 1, 3, 2), w)                  # not contiguous
    with pytest.raises(ValueError):
        ops.ti_smooth(g, w[:14])
    with pytest.raises(ValueError):
        ops.linf_ti_step(g[:1], g, None, w, EPS_ITER, EPS, LO, HI)
    with pytest.raises(Exception):
        ops.ti_smooth(g, w, out=g)                               # g == out: VQA_ERR_SHAPE
    assert ops.ti_smooth(g[:0], w).shape == (0, 3, 8, 8)


# ------------------------------------------------------------------------------------------------ the paper's operator
@pytest.mark.parametrize("k", [3, 7, 15, 31])
def test_faithful_to_the_2d_gaussian_convolution_in_float64(k):
    """|ghat - ref| <= (2K + 8) * 2^-24 * (W * |g|) elementwise, ref and the right side the float64 2-D convolution with
    ``outer(k, k) / sum`` on the CPU: the running-error bound of K products and K adds per pass, two passes, plus the taps'
    rounding -- derived, not measured."""
    import torch.nn.functional as Fn
    from vqattack_amd import ops
    g, _, _ = _inputs((2, 3, 45, 70), 20 + k)
    x = np.linspace(-3.0, 3.0, k)
    k1 = np.exp(-0.5 * x * x)
    k2 = np.outer(k1, k1)
    k2 = torch.from_numpy(k2 / k2.sum()).expand(3, 1, k, k).contiguous()
    g64 = torch.from_numpy(g.astype(np.float64))
    ref = Fn.conv2d(g64, k2, padding=k // 2, groups=3).numpy()
    bound = (2 * k + 8) * 2.0 ** -24 * Fn.conv2d(g64.abs(), k2, padding=k // 2, groups=3).numpy()
    got = ops.ti_smooth(_dev(g), ops.ti_gaussian_taps(k)).cpu().numpy().astype(np.float64)
    ratio = np.abs(got - ref) / bound
    print("K = {}: max |err| / bound = {:.3f}".format(k, ratio.max()))
    assert np.all(np.abs(got - ref) <= bound)
