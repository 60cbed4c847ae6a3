"""The DI (input diversity) kernels on the MI355X: ``vqa_di_transform``, ``vqa_di_adjoint`` and both forms of
``vqa_linf_di_step``.

The reference is a numpy fp32 chain written here from the contract of ``include/vqattack_hip.h`` (``di_forward`` /
``di_adjoint``), independent of the product and of torch: per axis ``src = scale * (d + 0.5) - 0.5`` in fp32, the
bilinear blend with one multiply per product and one add per sum, and the adjoint as a gather whose two contributors per
source coordinate are added in ascending destination order to ``+0``.  It is followed by the numpy ``StepOp`` / ``FgmOp``
of ``csrc/common.hpp``.  The kernels must give its bits.

Every kernel works on tiles of 64 columns x 32 rows of one plane, a lane on 4 consecutive pixels.  The shapes follow from
that: a plane smaller than a tile, exactly one tile, one row and one column more, several tiles both ways (so that a
tile's destination window starts in the middle of the table), a width that is no multiple of 4, rows that differ per
sample (identity, a 1 x 1 window, a window in the bottom-left and in the top-right corner), one axis identity and the
other not, and tensors sliced at a 4-byte-but-not-16-byte offset (the per-element path).  References are computed once.

Adjointness bound.  Both chains use the same fp32 weights, so in exact arithmetic ``<T x, g> == <x, T^T g>``.  A forward
pixel is ``ly0 * (lx0 * a + lx1 * b) + ly1 * (...)``: a term passes through 4 roundings (multiply, add, multiply, add); an
adjoint pixel is two nested sums of at most two products each, started at +0 (exact): again at most 4 roundings per term
(multiply, add, multiply, add).  With u = 2^-24 each side is therefore within ``4.1 u S`` of the exact bilinear form,
``S = <T|x|, |g|>`` (float64, every term taken by absolute value), the two float64 accumulations add ``~N 2^-53 S``, far
below that: ``|<T x, g> - <x, T^T g>| <= 8.2 * 2^-24 * S + 1e-12 * S``.

Bound against torch (CPU, ``F.interpolate(bilinear, align_corners=False, antialias=False)`` + ``F.pad`` and autograd).
Torch forms the source coordinate with its own rounding.  Either side computes it with at most 3 rounded operations on
values below ``full``, so the two coordinates differ by at most ``delta = 6 * full * 2^-24`` per axis.  The bilinear
interpolant is continuous and piecewise linear in the coordinate with slope = the neighbour difference, also across a
pixel boundary (where the two sides may pick different ``i0``), so the forward differs by at most
``delta_x * Dx + delta_y * Dy`` (``Dx`` / ``Dy``: the largest neighbour difference of the sample along x / y) plus the
blend's own rounding on both sides, ``<= 12 * 2^-24 * max|x|``.  For the adjoint every weight moves by at most ``delta``;
a source coordinate has at most 2 contributors (3 where a boundary case moves one over) whose weights sum to at most 2,
so the 2-D weights of a source pixel move by at most ``3 delta_y * 2 + 2 * 3 delta_x`` in total: the adjoint differs by
at most ``(6 (delta_x + delta_y) + 16 * 2^-24) * max|gD|``.  Measured worst cases: ``profiles/r21/README.md``.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
U = 2.0 ** -24
EPS, EPS_ITER, LO, HI = 0.03, 0.01, -1.0, 1.0

# name -> (shape, rows [new_h, new_w, top, left] per sample)
CASES = {
    "sub_tile": ((1, 3, 5, 9), [[3, 5, 1, 2]]),
    "one_tile": ((2, 1, 32, 64), [[25, 50, 3, 7], [31, 63, 1, 0]]),
    "tile_plus_one": ((1, 2, 33, 65), [[29, 57, 2, 5]]),
    "multi_tile": ((2, 3, 96, 160), [[71, 118, 11, 23], [95, 159, 0, 1]]),
    "odd_width": ((2, 3, 37, 70), [[30, 57, 4, 6], [19, 35, 18, 35]]),
    "mixed_rows": ((4, 2, 40, 72), [[40, 72, 0, 0], [1, 1, 17, 30], [33, 60, 7, 0], [33, 60, 0, 12]]),
    "axis_identity": ((2, 1, 33, 68), [[33, 50, 0, 9], [20, 68, 5, 0]]),
}
_refs = {}


# ------------------------------------------------------------------------------------------------ the numpy chain
def di_axis(full, new):
    """Destination d = 0 .. new-1 of one axis -> (i0, l0, l1), fp32 as in the header; (arange, None, None) for the
    identity axis."""
    if new == full:
        return np.arange(new), None, None
    d = np.arange(new, dtype=np.float32)
    scale = F(full) / F(new)
    src = scale * (d + F(0.5)) - F(0.5)
    f = np.floor(src)
    l1 = src - f
    l0 = F(1) - l1
    i0 = f.astype(np.int64)
    assert src.dtype == l0.dtype == l1.dtype == np.float32
    assert i0[0] >= 0 and i0[-1] + 1 <= full - 1 and np.all(np.diff(i0) > 0)      # no clamp, strictly increasing
    return i0, l0, l1


def _blend(a, i0, l0, l1):
    """Last axis of ``a`` (full) -> new, in a's dtype: l0 * a[i0] + l1 * a[i0 + 1], or a[i0] on the identity axis."""
    if l0 is None:
        return a[..., i0]
    return l0.astype(a.dtype) * a[..., i0] + l1.astype(a.dtype) * a[..., i0 + 1]


def _spread(a, full, i0, l0, l1):
    """The transpose of ``_blend``: last axis of ``a`` (new) -> full; per source coordinate the contributor that names
    it as i1 (the smaller destination) first, then the one that names it as i0, added to +0."""
    acc = np.zeros(a.shape[:-1] + (full,), dtype=a.dtype)
    if l0 is None:
        acc[..., i0] = acc[..., i0] + a.dtype.type(1) * a
        return acc
    acc[..., i0 + 1] = acc[..., i0 + 1] + l1.astype(a.dtype) * a
    acc[..., i0] = acc[..., i0] + l0.astype(a.dtype) * a
    return acc


def di_forward(x, rows):
    """(B, C, H, W), rows (B, 4) -> T(x) in x's dtype (float32: the contract's bits)."""
    b, _, h, w = x.shape
    out = np.zeros_like(x)
    with np.errstate(all="ignore"):
        for s in range(b):
            nh, nw, top, left = (int(v) for v in rows[s])
            ax, ay = di_axis(w, nw), di_axis(h, nh)
            inner = _blend(x[s], *ax)                                         # (C, H, nw)
            out[s, :, top:top + nh, left:left + nw] = np.swapaxes(_blend(np.swapaxes(inner, 1, 2), *ay), 1, 2)
    return out


def di_adjoint(gd, rows):
    """(B, C, H, W), rows (B, 4) -> T^T(gD) in gD's dtype: the row pass over x first, then the column pass."""
    b, _, h, w = gd.shape
    out = np.zeros_like(gd)
    with np.errstate(all="ignore"):
        for s in range(b):
            nh, nw, top, left = (int(v) for v in rows[s])
            win = gd[s, :, top:top + nh, left:left + nw]
            t = _spread(win, w, *di_axis(w, nw))                              # (C, nh, W)
            out[s] = np.swapaxes(_spread(np.swapaxes(t, 1, 2), h, *di_axis(h, nh)), 1, 2)
    return out


def referenced(shape, rows):
    """bool (B, 1, H, W): the source pixels some destination reads."""
    b, _, h, w = shape
    m = np.zeros((b, 1, h, w), dtype=bool)
    for s in range(b):
        nh, nw, _, _ = (int(v) for v in rows[s])
        (yi, yl, _), (xi, xl, _) = di_axis(h, nh), di_axis(w, nw)
        ys = yi if yl is None else np.concatenate([yi, yi + 1])
        xs = xi if xl is None else np.concatenate([xi, xi + 1])
        m[s, 0][np.ix_(ys, xs)] = True
    return m


def window(shape, rows):
    b, _, h, w = shape
    m = np.zeros((b, 1, h, w), dtype=bool)
    for s in range(b):
        nh, nw, top, left = (int(v) for v in rows[s])
        m[s, 0, top:top + nh, left:left + nw] = True
    return m


def sign(g):
    return (g > 0).astype(np.float32) - (g < 0).astype(np.float32)      # torch.sign: sign(NaN) = 0


def host_update(x, g, x0, eps_iter=EPS_ITER, eps=EPS, lo=LO, hi=HI):
    """numpy fp32: StepOp (x0 given) or FgmOp (x0 None) of csrc/common.hpp."""
    a = np.clip(x + F(eps_iter) * sign(g), F(lo), F(hi))
    if x0 is None:
        return a
    e = np.clip(a - x0, -F(eps), F(eps))
    out = np.clip(x0 + e, F(lo), F(hi))
    assert out.dtype == np.float32
    return out


def _inputs(shape, seed):
    rng = np.random.default_rng(seed)
    g = (rng.standard_normal(shape) * np.exp(rng.standard_normal(shape) * 2.0)).astype(np.float32)   # log-normal scales
    x0 = rng.uniform(-1, 1, shape).astype(np.float32)
    x = np.clip(x0 + rng.uniform(-EPS, EPS, shape).astype(np.float32), F(LO), F(HI))
    return g, x, x0


def _case(name):
    """(rows, g, x, x0, T(x), T^T(g), step, fgm): inputs and the host references of a case, built once, never changed."""
    if name not in _refs:
        shape, rows = CASES[name]
        rows = np.asarray(rows, dtype=np.int32)
        g, x, x0 = _inputs(shape, sum(map(ord, name)))
        adj = di_adjoint(g, rows)
        _refs[name] = (rows, g, x, x0, di_forward(x, rows), adj, host_update(x, adj, x0), host_update(x, adj, None))
    return _refs[name]


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _geom(rows, shape):
    from vqattack_amd import ops
    return ops.di_geometry(rows, shape[2], shape[3], DEV)


def _assert_bits(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    same = np.mean(got.view(np.int32) == want.view(np.int32))
    assert same == 1.0, (what, same, np.nanmax(np.abs(got - want)))


# ------------------------------------------------------------------------------------------------ bitwise
@pytest.mark.parametrize("name", sorted(CASES))
def test_transform_adjoint_and_both_fused_steps_equal_the_host_chain_bitwise(name):
    from vqattack_amd import ops
    rows, g, x, x0, fwd, adj, step, fgm = _case(name)
    geom = _geom(rows, x.shape)
    gd, xd, x0d = _dev(g), _dev(x), _dev(x0)
    _assert_bits(ops.di_transform(xd, geom), fwd, "di_transform")
    _assert_bits(ops.di_adjoint(gd, geom), adj, "di_adjoint")
    _assert_bits(ops.linf_di_step(xd, gd, x0d, geom, EPS_ITER, EPS, LO, HI), step, "linf_di_step")
    _assert_bits(ops.linf_di_step(xd, gd, None, geom, EPS_ITER, EPS, LO, HI), fgm, "linf_di_step without x0")
    # ... and the fused step is the two-launch form, through the product
    two = ops.linf_step(xd, ops.di_adjoint(gd, geom), x0d, EPS_ITER, EPS, LO, HI)
    assert torch.equal(two, ops.linf_di_step(xd, gd, x0d, geom, EPS_ITER, EPS, LO, HI))
    two = ops.linf_fgm(xd, ops.di_adjoint(gd, geom), EPS_ITER, LO, HI)
    assert torch.equal(two, ops.linf_di_step(xd, gd, None, geom, EPS_ITER, EPS, LO, HI))
    assert np.abs(step - x0).max() <= EPS + 1e-6 and not np.array_equal(step, fgm)
    # in place
    xi = xd.clone()
    assert ops.linf_di_step(xi, gd, x0d, geom, EPS_ITER, EPS, LO, HI, out=xi) is xi
    _assert_bits(xi, step, "linf_di_step in place")
    xi = xd.clone()
    ops.linf_di_step(xi, gd, None, geom, EPS_ITER, EPS, LO, HI, out=xi)
    _assert_bits(xi, fgm, "linf_di_step without x0 in place")


def test_identity_row_copies_forward_and_drops_only_the_sign_of_zero_backward():
    from vqattack_amd import ops
    rows, g, x, _, fwd, adj, _, _ = _case("mixed_rows")
    assert np.array_equal(fwd[0].view(np.int32), x[0].view(np.int32)) and np.array_equal(adj[0], g[0] + F(0))
    neg0 = torch.full((1, 1, 4, 8), -0.0, device=DEV)
    ident = _geom([[4, 8, 0, 0]], neg0.shape)
    assert bool(torch.signbit(ops.di_transform(neg0, ident)).all())
    assert not bool(torch.signbit(ops.di_adjoint(neg0, ident)).any())


def test_a_row_outside_its_ranges_is_the_identity_row_in_the_kernel():
    """The wrappers refuse such tables (tests/test_di_host.py); a table written on the device can still hold one."""
    from vqattack_amd import ops
    rows, g, x, x0, _, _, _, _ = _case("odd_width")
    h, w = x.shape[2:]
    ident = np.array([[h, w, 0, 0]] * 2, dtype=np.int32)
    bad = torch.tensor([[h, w, 1, 0], [-3, 2 ** 30, -(2 ** 31), 2 ** 31 - 1]], dtype=torch.int32, device=DEV)
    gd, xd, x0d = _dev(g), _dev(x), _dev(x0)
    _assert_bits(ops.di_transform(xd, bad), di_forward(x, ident), "di_transform")
    _assert_bits(ops.di_adjoint(gd, bad), di_adjoint(g, ident), "di_adjoint")
    _assert_bits(ops.linf_di_step(xd, gd, x0d, bad, EPS_ITER, EPS, LO, HI),
                 host_update(x, di_adjoint(g, ident), x0), "linf_di_step")


@pytest.mark.parametrize("name", ["one_tile", "odd_width"])
def test_unaligned_views_take_the_per_element_path(name):
    from vqattack_amd import ops
    rows, g, x, x0, fwd, adj, step, fgm = _case(name)
    geom = _geom(rows, x.shape)

    def off(a):      # 4-byte aligned, not 16-byte aligned
        flat = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
        v = flat[1:].view(a.shape)
        v.copy_(_dev(a))
        assert v.data_ptr() % 16 == 4
        return v
    gd, xd, x0d = off(g), off(x), off(x0)
    out = off(np.zeros_like(x))
    _assert_bits(ops.di_transform(xd, geom, out=out), fwd, "di_transform")
    _assert_bits(ops.di_adjoint(gd, geom, out=out), adj, "di_adjoint")
    _assert_bits(ops.linf_di_step(xd, gd, x0d, geom, EPS_ITER, EPS, LO, HI, out=out), step, "linf_di_step")
    _assert_bits(ops.linf_di_step(xd, gd, None, geom, EPS_ITER, EPS, LO, HI, out=out), fgm, "linf_di_step without x0")
    # only one operand off the 16-byte grid is enough
    _assert_bits(ops.linf_di_step(_dev(x), _dev(g), x0d, geom, EPS_ITER, EPS, LO, HI), step, "x0 unaligned")
    geom_off = torch.empty(geom.numel() + 1, dtype=torch.int32, device=DEV)[1:].view(geom.shape).copy_(geom)
    _assert_bits(ops.di_adjoint(_dev(g), geom_off), adj, "geom at a 4-byte offset")


# ------------------------------------------------------------------------------------------------ the window
@pytest.mark.parametrize("name", ["sub_tile", "multi_tile", "mixed_rows", "axis_identity"])
def test_nothing_outside_the_window_or_unreferenced_reaches_the_result(name):
    from vqattack_amd import ops
    rows, g, x, x0, fwd, adj, step, _ = _case(name)
    geom = _geom(rows, x.shape)
    win = np.broadcast_to(window(g.shape, rows), g.shape)
    for junk in (np.nan, np.inf, -np.inf):
        gj = np.where(win, g, F(junk))
        _assert_bits(ops.di_adjoint(_dev(gj), geom), adj, "di_adjoint, {} outside the window".format(junk))
        _assert_bits(ops.linf_di_step(_dev(x), _dev(gj), _dev(x0), geom, EPS_ITER, EPS, LO, HI), step,
                     "linf_di_step, {} outside the window".format(junk))
    ref = np.broadcast_to(referenced(x.shape, rows), x.shape)
    xj = np.where(ref, x, F(np.nan))
    got = ops.di_transform(_dev(xj), geom)
    _assert_bits(got, fwd, "di_transform, NaN at unreferenced pixels")
    if name == "mixed_rows":          # a shrink below 2 references every source pixel; the 1 x 1 window leaves most out
        assert ref[0].all() and ref[1].sum() == 4 * x.shape[1]


# ------------------------------------------------------------------------------------------------ adjointness
@pytest.mark.parametrize("name", sorted(CASES))
def test_adjointness_in_float64(name):
    from vqattack_amd import ops
    rows, g, x, _, _, _, _, _ = _case(name)
    geom = _geom(rows, x.shape)
    tx = ops.di_transform(_dev(x), geom).cpu().numpy().astype(np.float64)
    tg = ops.di_adjoint(_dev(g), geom).cpu().numpy().astype(np.float64)
    lhs, rhs = float(np.sum(tx * g.astype(np.float64))), float(np.sum(x.astype(np.float64) * tg))
    s = float(np.sum(di_forward(np.abs(x).astype(np.float64), rows) * np.abs(g).astype(np.float64)))
    bound = 8.2 * U * s + 1e-12 * s
    print("adjointness {}: |lhs - rhs| = {:.3e}, bound {:.3e}, S = {:.3e}".format(name, abs(lhs - rhs), bound, s))
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)
    assert abs(lhs) > 0


# ------------------------------------------------------------------------------------------------ torch on the CPU
def _torch_reference(x, g, rows):
    import torch.nn.functional as tf
    b, _, h, w = x.shape
    fwd, adj = np.zeros_like(x), np.zeros_like(x)
    for s in range(b):
        nh, nw, top, left = (int(v) for v in rows[s])
        leaf = torch.from_numpy(x[s:s + 1].copy()).requires_grad_(True)
        d = tf.pad(tf.interpolate(leaf, size=(nh, nw), mode="bilinear", align_corners=False, antialias=False),
                   (left, w - nw - left, top, h - nh - top))
        d.backward(torch.from_numpy(g[s:s + 1].copy()))
        fwd[s], adj[s] = d.detach().numpy()[0], leaf.grad.numpy()[0]
    return fwd, adj


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_torch_interpolate_and_pad_on_the_cpu(name):
    from vqattack_amd import ops
    rows, g, x, _, _, _, _, _ = _case(name)
    geom = _geom(rows, x.shape)
    b, _, h, w = x.shape
    fwd_t, adj_t = _torch_reference(x, g, rows)
    fwd = ops.di_transform(_dev(x), geom).cpu().numpy()
    adj = ops.di_adjoint(_dev(g), geom).cpu().numpy()
    win = np.broadcast_to(window(g.shape, rows), g.shape)
    for s in range(b):
        dx_, dy_ = 6 * w * U, 6 * h * U
        nx = np.abs(np.diff(x[s], axis=2)).max() if w > 1 else 0.0
        ny = np.abs(np.diff(x[s], axis=1)).max() if h > 1 else 0.0
        bound_f = dx_ * nx + dy_ * ny + 12 * U * np.abs(x[s]).max()
        bound_a = (6 * (dx_ + dy_) + 16 * U) * np.abs(np.where(win[s], g[s], 0)).max()
        err_f, err_a = np.abs(fwd[s] - fwd_t[s]).max(), np.abs(adj[s] - adj_t[s]).max()
        print("torch {} sample {}: forward {:.3e} (bound {:.3e}), adjoint {:.3e} (bound {:.3e})".format(
            name, s, err_f, bound_f, err_a, bound_a))
        assert err_f <= bound_f and err_a <= bound_a


# ------------------------------------------------------------------------------------------------ the range flag
def test_range_flag_is_set_by_x_only_and_not_by_the_rest_of_a_partial_tile():
    from vqattack_amd import ops
    rows, g, x, x0, _, _, _, _ = _case("odd_width")          # 37 x 70: partial tiles both ways, per-element path
    geom = _geom(rows, x.shape)
    for x0d in (_dev(x0), None):
        flag = ops.new_flag(DEV)
        ops.linf_di_step(_dev(x), _dev(g), x0d, geom, EPS_ITER, EPS, LO, HI, flag=flag)
        assert int(flag.item()) == 0
        bad = x.copy()
        bad[1, 2, 36, 69] = 1.5
        ops.linf_di_step(_dev(bad), _dev(g), x0d, geom, EPS_ITER, EPS, LO, HI, flag=flag)
        assert int(flag.item()) & 1
    rows, g, x, x0, _, _, _, _ = _case("multi_tile")         # the 16-byte path
    geom = _geom(rows, x.shape)
    flag = ops.new_flag(DEV)
    ops.linf_di_step(_dev(x), _dev(g), _dev(x0), geom, EPS_ITER, EPS, LO, HI, flag=flag)
    assert int(flag.item()) == 0
    bad = x.copy()
    bad[0, 0, 0, 0] = np.nan
    ops.linf_di_step(_dev(bad), _dev(g), _dev(x0), geom, EPS_ITER, EPS, LO, HI, flag=flag)
    assert int(flag.item()) & 1
