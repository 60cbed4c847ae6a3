"""The three SI-NI (scale copies, Nesterov look-ahead) kernels on the MI355X.

Arithmetic under test (include/vqattack_hip.h), fp32 with one rounding per operation:
    copies:   out[i] = s_i * x                    or   s_i * (x + lookahead * m)
    combine:  acc = w_0 * g_0;  acc = acc + w_i * g_i  (i ascending);  out = acc
    step:     vqa_linf_step / vqa_linf_fgm on the combination, which never reaches memory
Everything is compared BITWISE with the numpy fp32 chain written here, the fused step also with the two-launch form; the
combination additionally with float64 inside the bound derived below.

Shapes: (3,3,5,7) n % 4 != 0: scalar path; (2,3,64,64) whole tiles only (6144 16-byte pieces: 12 tiles of 512, 24 of 256);
(2,4100) one whole tile of 512 pieces (or 8 of 256) and a partial one; "offset" the same from views one float off 16-byte
alignment: scalar path; "one_off" the same with only ONE gradient of the list misaligned; "flat" more tiles than the grid
has workgroups (256 CUs x 12), so the grid-stride loop goes round, and a partial tile; (64,3,592,592) 269 MB per tensor: the
non-temporal stores of a result larger than the Infinity Cache.
"""
import numpy as np
import pytest
import torch

from tests.pgd_reference import accumulate_np as _accumulate_np
from tests.pgd_reference import assert_bits as _assert_bits
from tests.pgd_reference import combine_np as _combine_np
from tests.pgd_reference import copies_np as _copies_np
from tests.pgd_reference import place as _place
from tests.pgd_reference import same_bits as _same_bits
from tests.pgd_reference import update_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
EPS_ITER, EPS, LO, HI = 0.01, 0.05, -1.0, 1.0
LOOKAHEAD = 0.009
SMALL = ["3x3x5x7", "2x3x64x64", "2x4100", "offset", "one_off"]
PARTIAL = SMALL + ["2x11276"]          # 2819 16-byte pieces per row: a partial tile with whole slots and 3 lanes
COPIES = [1, 2, 5, 8]
FLAT = 256 * 12 * 2048 + 5 * 2048 + 1036          # > grid x the larger tile (2 x 256 pieces of 4 floats), partial tile
_SHAPES = {"3x3x5x7": (3, 3, 5, 7), "2x3x64x64": (2, 3, 64, 64), "2x4100": (2, 4100), "offset": (2, 4100),
           "one_off": (2, 4100), "flat": (FLAT,), "2x11276": (2, 11276)}
_cache = {}


def _data(name):
    """x0 in [-1, 1], x inside its ball, 8 gradients drawn as 1e-3 * N(0, 1), a normal-draw momentum: built once per
    shape and never changed."""
    if name not in _cache:
        shape = _SHAPES[name]
        r = np.random.RandomState(len(name) + shape[-1] % 1000)
        x0 = r.uniform(-1, 1, shape).astype(F)
        x = np.clip(x0 + r.uniform(-EPS, EPS, shape).astype(F), LO, HI).astype(F)
        m = r.standard_normal(shape).astype(F)
        n_g = 8 if name != "flat" else 5
        g = [(r.standard_normal(shape) * 1e-3).astype(F) for _ in range(n_g)]
        host = dict(x=x, x0=x0, m=m, g=g)
        off = name == "offset"
        dev = dict(x=_place(x, off), x0=_place(x0, off), m=_place(m, off),
                   g=[_place(a, off or (name == "one_off" and i == 1)) for i, a in enumerate(g)])
        _cache[name] = (host, dev)
    return _cache[name]


def _update_np(x, ghat, x0, clip=True):
    return update_np(x, ghat, x0, EPS_ITER, EPS, LO, HI, clip)


def _weights(copies):
    from vqattack_amd import ops
    return ops.si_weights(ops.si_scales(copies))


# ------------------------------------------------------------------------------------------------ copies
@pytest.mark.parametrize("copies", COPIES)
@pytest.mark.parametrize("name", SMALL)
def test_copies_equal_the_numpy_fp32_chain_bitwise(name, copies):
    from vqattack_amd import ops
    host, dev = _data(name)
    s = ops.si_scales(copies)
    got = ops.si_copies(dev["x"], s)
    assert got.shape == (copies,) + host["x"].shape and got.is_contiguous()
    _assert_bits(got, _copies_np(host["x"], s), "si_copies")
    got_ni = ops.si_copies(dev["x"], s, m=dev["m"], lookahead=LOOKAHEAD)
    _assert_bits(got_ni, _copies_np(host["x"], s, host["m"], LOOKAHEAD), "si_copies with look-ahead")
    assert not _same_bits(got, got_ni)
    odd = np.array([1.0, 0.7, 1.3, 0.3, 2.0, 0.11, 0.9, 0.5], dtype=F)[:copies]      # scales that do round
    _assert_bits(ops.si_copies(dev["x"], odd, m=dev["m"], lookahead=LOOKAHEAD),
                 _copies_np(host["x"], odd, host["m"], LOOKAHEAD), "si_copies, free scales")
    out = torch.full((copies,) + host["x"].shape, 7.0, device=DEV)
    assert ops.si_copies(dev["x"], s, out=out) is out and _same_bits(out, got)        # caller's buffer, same bits again
    assert np.array_equal(dev["x"].cpu().numpy(), host["x"]) and np.array_equal(dev["m"].cpu().numpy(), host["m"])


@pytest.mark.parametrize("name", SMALL)
def test_scale_one_without_momentum_is_a_bit_copy(name):
    from vqattack_amd import ops
    host, _ = _data(name)
    x = host["x"].copy()
    flat = x.reshape(-1)
    flat[0], flat[1], flat[-1], flat[5] = -0.0, np.nan, np.inf, F(1e-30)
    got = ops.si_copies(_place(x, name == "offset"), [1.0])
    _assert_bits(got, x[None], "s = 1")
    got = ops.si_copies(_place(x, name == "offset"), [1.0, 1.0, 1.0])
    _assert_bits(got, np.stack([x] * 3), "three copies at s = 1")


def test_copies_into_the_prefix_of_a_larger_buffer():
    """copy_stride > n: the copies of a batch prefix land in the prefix of each copy's slot; the rest stays untouched."""
    from vqattack_amd import ops
    host, dev = _data("2x3x64x64")
    s = ops.si_scales(3)
    big = torch.full((3, 5, 3, 64, 64), 7.0, device=DEV)
    got = ops.si_copies(dev["x"], s, m=dev["m"], lookahead=LOOKAHEAD, out=big[:, :2])
    assert got.data_ptr() == big.data_ptr()
    _assert_bits(big[:, :2], _copies_np(host["x"], s, host["m"], LOOKAHEAD), "prefix")
    assert bool((big[:, 2:] == 7.0).all())
    with pytest.raises(ValueError):
        ops.si_copies(dev["x"], s, out=torch.zeros(3, 2, 3, 64, 128, device=DEV)[..., :64])   # out[i] is not contiguous


# ------------------------------------------------------------------------------------------------ combine
@pytest.mark.parametrize("copies", COPIES)
@pytest.mark.parametrize("name", PARTIAL)
def test_combine_equals_the_numpy_fp32_chain_bitwise_and_stays_inside_the_fp64_bound(name, copies):
    """Against float64: the fp32 chain makes one rounding per product and one per add, `copies` products and
    `copies - 1` adds; every intermediate is at most S = sum_i |w_i * g_i| (1 + O(2^-24)) in magnitude, so each rounding
    errs by at most 2^-24 * S and a product's by 2^-24 * |w_i g_i|: in all at most (1 + copies - 1) * 2^-24 * S to first
    order, and (copies + 1) * 2^-24 * S leaves a whole term for the higher orders.  Gradients are 1e-3 * N(0, 1):
    nothing is subnormal."""
    from vqattack_amd import ops
    host, dev = _data(name)
    w = _weights(copies)
    got = ops.si_combine(dev["g"][:copies], w)
    want = _combine_np(host["g"][:copies], w)
    _assert_bits(got, want, "si_combine")
    assert _same_bits(got, ops.si_combine(dev["g"][:copies], w))                      # the same bits every run
    out = torch.full_like(got, 7.0)
    assert ops.si_combine(dev["g"][:copies], w, out=out) is out and _same_bits(out, got)
    terms = [np.float64(w[i]) * host["g"][i].astype(np.float64) for i in range(copies)]
    exact, mag = sum(terms), sum(np.abs(t) for t in terms)
    ratio = np.abs(got.cpu().numpy().astype(np.float64) - exact) / ((copies + 1) * 2.0 ** -24 * mag)
    print("si_combine", name, "copies", copies, "worst |err| / bound vs fp64: %.4f" % ratio.max())
    assert ratio.max() <= 1.0, ratio.max()
    for i in range(copies):
        assert np.array_equal(dev["g"][i].cpu().numpy(), host["g"][i])                # the inputs are never written


@pytest.mark.parametrize("name", SMALL)
def test_one_copy_of_weight_one_is_the_identity(name):
    from vqattack_amd import ops
    host, dev = _data(name)
    g = host["g"][0].copy()
    flat = g.reshape(-1)
    flat[0], flat[1], flat[-1], flat[7] = -0.0, np.nan, -np.inf, 0.0
    gd = _place(g, name == "offset")
    _assert_bits(ops.si_combine([gd], [1.0]), g, "identity")
    # ... and so the fused step with it is the plain kernel
    assert _same_bits(ops.linf_si_step(dev["x"], [gd], dev["x0"], [1.0], EPS_ITER, EPS, LO, HI),
                      ops.linf_step(dev["x"], gd, dev["x0"], EPS_ITER, EPS, LO, HI))
    assert _same_bits(ops.linf_si_step(dev["x"], [gd], None, [1.0], EPS_ITER, EPS, LO, HI),
                      ops.linf_fgm(dev["x"], gd, EPS_ITER, LO, HI))


@pytest.mark.parametrize("shape", [(3, 3, 5, 7), (2, 4100)], ids=["3x3x5x7", "2x4100"])
def test_the_unseeded_fold_keeps_minus_zero_and_the_seeded_one_adds_it_to_its_seed(shape):
    """The one place where the two starts of the shared fold kernel differ: 1 * -0 is -0, +0 + 1 * -0 is +0."""
    from vqattack_amd import ops
    g = np.full(shape, -0.0, dtype=F)
    gd = _place(g, False)
    combined = ops.si_combine([gd], [1.0])
    assert np.all(combined.cpu().numpy().view(np.int32) == np.int32(-2 ** 31)), "si_combine: not the bits of -0.0"
    _assert_bits(combined, _combine_np([g], [1.0]), "si_combine")
    acc = torch.zeros(shape, dtype=torch.float32, device=DEV)
    summed = ops.admix_accumulate([gd], [1.0], acc)
    assert np.all(summed.cpu().numpy().view(np.int32) == 0), "admix_accumulate: not the bits of +0.0"
    _assert_bits(summed, _accumulate_np(np.zeros(shape, dtype=F), [g], [1.0]), "admix_accumulate")


# ------------------------------------------------------------------------------------------------ fused step
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("with_x0", [True, False])
@pytest.mark.parametrize("copies", COPIES)
@pytest.mark.parametrize("name", PARTIAL)
def test_fused_step_equals_the_numpy_chain_and_the_two_launches_bitwise(name, copies, with_x0, in_place):
    from vqattack_amd import ops
    host, dev = _data(name)
    w = _weights(copies)
    off = name == "offset"
    grads = dev["g"][:copies]
    x0 = dev["x0"] if with_x0 else None
    x_fused = _place(host["x"], off) if in_place else dev["x"]
    got = ops.linf_si_step(x_fused, grads, x0, w, EPS_ITER, EPS, LO, HI, out=x_fused if in_place else None)
    assert (got is x_fused) == in_place
    want = _update_np(host["x"], _combine_np(host["g"][:copies], w), host["x0"] if with_x0 else None)
    _assert_bits(got, want, "linf_si_step")
    ghat = ops.si_combine(grads, w)
    two = ops.linf_step(dev["x"], ghat, x0, EPS_ITER, EPS, LO, HI) if with_x0 else \
        ops.linf_fgm(dev["x"], ghat, EPS_ITER, LO, HI)
    assert _same_bits(got, two)
    assert np.array_equal(dev["x"].cpu().numpy(), host["x"])                          # the shared inputs are never written
    if with_x0:
        assert float((got - dev["x0"]).abs().max()) <= EPS + 1e-6
    assert float((got - dev["x"]).abs().max()) > 0


@pytest.mark.parametrize("with_x0", [True, False])
def test_fused_step_without_a_clip_range(with_x0):
    from vqattack_amd import ops
    host, dev = _data("2x4100")
    w = _weights(5)
    got = ops.linf_si_step(dev["x"], dev["g"][:5], dev["x0"] if with_x0 else None, w, EPS_ITER, EPS, None, None)
    want = _update_np(host["x"], _combine_np(host["g"][:5], w), host["x0"] if with_x0 else None, clip=False)
    _assert_bits(got, want, "no clip")


@pytest.mark.parametrize("with_x0", [True, False])
@pytest.mark.parametrize("name", SMALL)
def test_range_flag_is_set_exactly_when_an_input_is_outside_the_clip_range(name, with_x0):
    from vqattack_amd import ops
    from vqattack_amd._hip import VQA_FLAG_RANGE
    host, dev = _data(name)
    off = name == "offset"
    x0 = dev["x0"] if with_x0 else None
    w = _weights(3)
    flag = ops.new_flag(DEV)
    ops.linf_si_step(dev["x"], dev["g"][:3], x0, w, EPS_ITER, EPS, LO, HI, flag=flag)
    assert int(flag.item()) == 0
    for where, value in ((0, 1.5), (-1, -1.0000001), (host["x"].size // 2, float("nan"))):
        x = host["x"].copy()
        x.reshape(-1)[where] = value                                             # ONE element outside, first / last / middle
        flag = ops.new_flag(DEV)
        ops.linf_si_step(_place(x, off), dev["g"][:3], x0, w, EPS_ITER, EPS, LO, HI, flag=flag)
        assert int(flag.item()) == VQA_FLAG_RANGE, (where, value)
    flag = ops.new_flag(DEV)                                                     # no clip range: nothing to check
    x = host["x"].copy()
    x.reshape(-1)[0] = 7.0
    ops.linf_si_step(_place(x, off), dev["g"][:3], x0, w, EPS_ITER, EPS, None, None, flag=flag)
    assert int(flag.item()) == 0


# ------------------------------------------------------------------------------------------------ more tiles than workgroups
@pytest.mark.parametrize("copies", [2, 5])
def test_flat_tensor_with_more_tiles_than_the_grid_has_workgroups(copies):
    """copies = 2 runs two tiles of 256 pieces in flight, copies = 5 one: both grids go round at this size."""
    from vqattack_amd import ops
    host, dev = _data("flat")
    w = _weights(copies)
    ghat = _combine_np(host["g"][:copies], w)
    _assert_bits(ops.si_combine(dev["g"][:copies], w), ghat, "si_combine")
    _assert_bits(ops.linf_si_step(dev["x"], dev["g"][:copies], dev["x0"], w, EPS_ITER, EPS, LO, HI),
                 _update_np(host["x"], ghat, host["x0"]), "linf_si_step")
    x = dev["x"].clone()
    ops.linf_si_step(x, dev["g"][:copies], None, w, EPS_ITER, EPS, LO, HI, out=x)
    _assert_bits(x, _update_np(host["x"], ghat, None), "linf_si_step without x0, in place")
    s = ops.si_scales(copies)
    _assert_bits(ops.si_copies(dev["x"], s, m=dev["m"], lookahead=LOOKAHEAD),
                 _copies_np(host["x"], s, host["m"], LOOKAHEAD), "si_copies")


# ------------------------------------------------------------------------------------------------ past the Infinity Cache
def test_large_result_takes_the_non_temporal_stores():
    """(64, 3, 592, 592): 269 MB per tensor.  The references are eager torch ops, one rounding each (mul, then add)."""
    from vqattack_amd import ops
    shape = (64, 3, 592, 592)
    gen = torch.Generator(DEV).manual_seed(64)
    x0 = torch.empty(shape, device=DEV).uniform_(-1, 1, generator=gen)
    x = (x0 + torch.empty(shape, device=DEV).uniform_(-EPS, EPS, generator=gen)).clamp_(-1, 1)
    g = [torch.randn(shape, device=DEV, generator=gen) * 1e-3 for _ in range(2)]
    w = _weights(2)
    want = g[0] * float(w[0])
    want = want + g[1] * float(w[1])
    ghat = ops.si_combine(g, w)
    assert _same_bits(ghat, want)
    del want
    got = ops.linf_si_step(x, g, x0, w, EPS_ITER, EPS, LO, HI)
    assert _same_bits(got, ops.linf_step(x, ghat, x0, EPS_ITER, EPS, LO, HI))
    xi = x.clone()
    ops.linf_si_step(xi, g, x0, w, EPS_ITER, EPS, LO, HI, out=xi)
    assert _same_bits(xi, got)
    del xi, got, ghat
    m = g[1]                                                                         # any tensor will do as a momentum
    s = ops.si_scales(2)
    c = ops.si_copies(x, s, m=m, lookahead=LOOKAHEAD)
    base = x + m * LOOKAHEAD
    assert _same_bits(c[0], base * float(s[0])) and _same_bits(c[1], base * float(s[1]))
    c = ops.si_copies(x, s, out=c)
    assert _same_bits(c[0], x) and _same_bits(c[1], x * 0.5)


def test_wrappers_check_shapes_and_empty_tensors():
    from vqattack_amd import ops
    g = torch.zeros(2, 8, device=DEV)
    h = torch.zeros(2, 4, device=DEV)
    with pytest.raises(ValueError):
        ops.si_combine([g, h], [0.5, 0.5])                                           # mixed shapes
    with pytest.raises(ValueError):
        ops.si_combine([g, g.clone()], [0.5])                                        # one weight short
    with pytest.raises(TypeError):
        ops.si_combine([g, g.double()], [0.5, 0.5])
    with pytest.raises(ValueError):
        ops.si_combine([g, torch.zeros(8, 2, device=DEV).t()], [0.5, 0.5])           # not contiguous
    with pytest.raises(ValueError):
        ops.linf_si_step(h, [g, g.clone()], None, [0.5, 0.5], 0.01, 0.1, -1.0, 1.0)
    with pytest.raises(ValueError):
        ops.si_copies(g, [1.0, 0.5], m=h)
    with pytest.raises(ValueError):
        ops.si_copies(g, [1.0, 0.5], out=torch.zeros(3, 2, 8, device=DEV))
    from vqattack_amd._hip import HipExtensionError
    with pytest.raises(HipExtensionError):
        ops.si_combine([g, g.clone()], [0.5, 0.5], out=g)                            # out aliases a gradient
    empty = torch.empty(0, 8, device=DEV)
    assert ops.si_copies(empty, [1.0, 0.5]).shape == (2, 0, 8)
    assert ops.si_combine([empty, empty], [0.5, 0.5]).shape == (0, 8)
    assert ops.linf_si_step(empty, [empty], None, [1.0], 0.01, 0.1, -1.0, 1.0).shape == (0, 8)
