"""The three Admix kernels (mixed-image copies, running sum, fused L-inf step) on the MI355X.

Arithmetic under test (include/vqattack_hip.h), fp32 with one rounding per operation:
    copies:      t = x[b] (or x[b] + lookahead * m[b]);  u = eta * x[partner[b]];  v = t + u;  out[i][b] = s_i * v
    accumulate:  a = acc;  a = a + w_i * g_i  (i ascending);  acc = a
    step:        vqa_linf_step / vqa_linf_fgm on that sum, which never reaches memory (and acc stays as it is)
Everything is compared BITWISE with the numpy fp32 chain written here, the fused step also with the two-launch form, the
sum additionally with float64 inside the bound derived at its test.

Copies shapes (batch first): (3,3,5,7) per = 105, odd: scalar path; (4,3,64,64) whole tiles only; (3,4100) one whole tile
and a partial one; (3,11276) 2819 16-byte pieces per sample: a partial tile with whole slots and 3 lanes in the last;
"offset" (3,4100) one float behind a 16-byte boundary: scalar path; "round" B = 2 with more tiles per sample than the
grid has workgroups per sample (stream_grid: CUs x 12 / 2 workgroups, 1536 on 256 CUs, each tile 2 x 256 pieces of 4
floats: about 3.2 M floats per sample), so the tile loop goes round, and a partial tile.
Sum shapes: (3,3,5,7) scalar path; (2,3,64,64) whole tiles; (2,4100) a partial tile; "offset"; "one_off": only ONE gradient
of the list misaligned.
"""
import numpy as np
import pytest
import torch

from tests.pgd_reference import accumulate_np as _accumulate_np
from tests.pgd_reference import assert_bits as _assert_bits
from tests.pgd_reference import combine_np as _combine_np
from tests.pgd_reference import place as _place
from tests.pgd_reference import same_bits as _same_bits
from tests.pgd_reference import update_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
EPS_ITER, EPS, LO, HI = 0.01, 0.05, -1.0, 1.0
LOOKAHEAD, ETA = 0.009, 0.2
COPIES = [1, 2, 5, 8]
_COPY_SHAPES = {"3x3x5x7": (3, 3, 5, 7), "4x3x64x64": (4, 3, 64, 64), "3x4100": (3, 4100), "3x11276": (3, 11276),
                "offset": (3, 4100)}
COPY_SMALL = ["3x3x5x7", "4x3x64x64", "3x4100", "3x11276", "offset"]
_SUM_SHAPES = {"3x3x5x7": (3, 3, 5, 7), "2x3x64x64": (2, 3, 64, 64), "2x4100": (2, 4100), "offset": (2, 4100),
               "one_off": (2, 4100)}
SUM_NAMES = list(_SUM_SHAPES)
_cache = {}


def _update_np(x, ghat, x0, clip=True):
    return update_np(x, ghat, x0, EPS_ITER, EPS, LO, HI, clip)


def _round_per():
    """Floats per sample of the "round" shape at B = 2, from stream_grid(per / 4, U = 2, share = 2): grid.x = CUs * 12 / 2
    workgroups per sample, each tile 2 x 256 pieces of 4 floats; three tiles and a partial one more than one round."""
    grid_x = torch.cuda.get_device_properties(0).multi_processor_count * 12 // 2
    return grid_x * 2048 + 3 * 2048 + 1036


def _copy_data(name):
    """x in [-1, 1] and a normal-draw momentum: built once per shape and never changed."""
    key = ("copies", name)
    if key not in _cache:
        shape = _COPY_SHAPES[name] if name != "round" else (2, _round_per())
        r = np.random.RandomState(len(name) + shape[-1] % 1000)
        x = r.uniform(-1, 1, shape).astype(F)
        m = r.standard_normal(shape).astype(F)
        off = name == "offset"
        _cache[key] = (dict(x=x, m=m), dict(x=_place(x, off), m=_place(m, off)))
    return _cache[key]


def _sum_data(name):
    """x0 in [-1, 1], x inside its ball, a running sum and 8 gradients drawn as 1e-3 * N(0, 1): built once per shape."""
    key = ("sum", name)
    if key not in _cache:
        shape = _SUM_SHAPES[name]
        r = np.random.RandomState(100 + len(name) + shape[-1] % 1000)
        x0 = r.uniform(-1, 1, shape).astype(F)
        x = np.clip(x0 + r.uniform(-EPS, EPS, shape).astype(F), LO, HI).astype(F)
        acc = (r.standard_normal(shape) * 1e-3).astype(F)
        g = [(r.standard_normal(shape) * 1e-3).astype(F) for _ in range(8)]
        off = name == "offset"
        dev = dict(x=_place(x, off), x0=_place(x0, off), acc=_place(acc, off),
                   g=[_place(a, off or (name == "one_off" and i == 1)) for i, a in enumerate(g)])
        _cache[key] = (dict(x=x, x0=x0, acc=acc, g=g), dev)
    return _cache[key]


def _rows(batch):
    """Partner rows: constant (all to sample 0, sample 0 to 1), a cyclic shift, and the shift the other way round."""
    const = np.zeros(batch, dtype=np.int32)
    const[0] = 1
    ar = np.arange(batch, dtype=np.int32)
    return {"constant": const, "shift": (ar + 1) % batch, "back": (ar + batch - 1) % batch}


def _row_dev(row):
    return torch.from_numpy(np.ascontiguousarray(row, dtype=np.int32)).to(DEV)


def _copies_np(x, row, s, eta, m=None, lookahead=0.0):
    with np.errstate(all="ignore"):
        t = x if m is None else x + F(lookahead) * m
        u = F(eta) * x[row]
        v = t + u
        out = np.stack([F(si) * v for si in s])
    assert out.dtype == F
    return out


# ------------------------------------------------------------------------------------------------ copies
@pytest.mark.parametrize("copies", COPIES)
@pytest.mark.parametrize("name", COPY_SMALL)
def test_copies_equal_the_numpy_fp32_chain_bitwise(name, copies):
    from vqattack_amd import ops
    host, dev = _copy_data(name)
    s = ops.si_scales(copies)
    odd = np.array([1.0, 0.7, 1.3, 0.3, 2.0, 0.11, 0.9, 0.5], dtype=F)[:copies]      # scales that do round
    for which, row in _rows(host["x"].shape[0]).items():
        rd = _row_dev(row)
        got = ops.admix_copies(dev["x"], rd, s, ETA)
        assert got.shape == (copies,) + host["x"].shape and got.is_contiguous()
        _assert_bits(got, _copies_np(host["x"], row, s, ETA), "admix_copies, " + which)
        got_ni = ops.admix_copies(dev["x"], rd, s, ETA, m=dev["m"], lookahead=LOOKAHEAD)
        _assert_bits(got_ni, _copies_np(host["x"], row, s, ETA, host["m"], LOOKAHEAD), "admix_copies with look-ahead, " + which)
        assert not _same_bits(got, got_ni)
        _assert_bits(ops.admix_copies(dev["x"], rd, odd, 0.37, m=dev["m"], lookahead=LOOKAHEAD),
                     _copies_np(host["x"], row, odd, 0.37, host["m"], LOOKAHEAD), "admix_copies, free scales, " + which)
    out = torch.full((copies,) + host["x"].shape, 7.0, device=DEV)
    assert ops.admix_copies(dev["x"], rd, s, ETA, out=out) is out and _same_bits(out, got)   # caller's buffer, same bits
    assert np.array_equal(dev["x"].cpu().numpy(), host["x"]) and np.array_equal(dev["m"].cpu().numpy(), host["m"])


@pytest.mark.parametrize("with_m", [False, True])
def test_copies_when_the_tile_loop_goes_round(with_m):
    """More tiles per sample than the grid has workgroups per sample; compared on the device with the same chain in
    torch's own fp32 operations (one rounding each), which the small shapes pin against numpy."""
    from vqattack_amd import ops
    host, dev = _copy_data("round")
    per, grid_x = _round_per(), torch.cuda.get_device_properties(0).multi_processor_count * 12 // 2
    assert per // 4 > grid_x * 512 and per % 4 == 0 and host["x"].shape == (2, per)
    s = ops.si_scales(2)
    row = np.array([1, 0], dtype=np.int32)
    got = ops.admix_copies(dev["x"], _row_dev(row), s, ETA, m=dev["m"] if with_m else None,
                           lookahead=LOOKAHEAD if with_m else 0.0)
    x = dev["x"]
    t = x + LOOKAHEAD * dev["m"] if with_m else x
    v = t + ETA * x[[1, 0]]
    for i in range(2):
        assert _same_bits(got[i], float(s[i]) * v), i
    # and a stretch around the wrap and the partial tile against numpy itself
    for lo in (0, grid_x * 2048 - 64, per - 1100):
        sl = slice(lo, lo + 1100)
        want = _copies_np(host["x"][:, sl], row, s, ETA, host["m"][:, sl] if with_m else None, LOOKAHEAD)
        _assert_bits(got[:, :, sl], want, "stretch at {}".format(lo))


def test_copies_into_the_batch_prefix_of_a_larger_buffer():
    from vqattack_amd import ops
    host, dev = _copy_data("3x4100")
    s = ops.si_scales(5)
    row = _rows(3)["shift"]
    big = torch.full((5, 6, 4100), 7.0, device=DEV)
    got = ops.admix_copies(dev["x"], _row_dev(row), s, ETA, out=big[:, :3])
    assert got.data_ptr() == big.data_ptr()
    _assert_bits(big[:, :3], _copies_np(host["x"], row, s, ETA), "prefix")
    assert bool((big[:, 3:] == 7.0).all())                                  # nothing behind the prefix is touched


def test_an_index_outside_the_batch_stands_for_the_sample_itself():
    """The kernel's own guard (``admix_partners`` refuses such a table before it gets there): no memory outside x is read."""
    from vqattack_amd import ops
    host, dev = _copy_data("3x4100")
    s = ops.si_scales(2)
    row = np.array([3, -1, 1 << 30], dtype=np.int32)
    got = ops.admix_copies(dev["x"], _row_dev(row), s, ETA)
    _assert_bits(got, _copies_np(host["x"], np.arange(3), s, ETA), "own sample")


def test_copies_wrapper_checks():
    from vqattack_amd import ops
    _, dev = _copy_data("3x4100")
    x, rd = dev["x"], _row_dev(_rows(3)["shift"])
    s = ops.si_scales(2)
    for bad in (lambda: ops.admix_copies(x, rd.to(torch.int64), s, ETA), lambda: ops.admix_copies(x, rd[:2], s, ETA),
                lambda: ops.admix_copies(x, rd.cpu(), s, ETA), lambda: ops.admix_copies(x, rd, [], ETA),
                lambda: ops.admix_copies(x, rd, [1.0] * 9, ETA), lambda: ops.admix_copies(x, rd, s, ETA, m=dev["m"][:2]),
                lambda: ops.admix_copies(x, rd, s, ETA, out=torch.empty((2, 3, 4099), device=DEV))):
        with pytest.raises(ValueError):
            bad()
    empty = torch.empty((3, 0), device=DEV)
    assert ops.admix_copies(empty, rd, s, ETA).shape == (2, 3, 0)
    from vqattack_amd._hip import HipExtensionError
    with pytest.raises(HipExtensionError):                                   # out overlaps x: refused by the library
        both = torch.zeros((2, 3, 4100), device=DEV)
        ops.admix_copies(both[0], rd, s, ETA, out=both)


# ------------------------------------------------------------------------------------------------ running sum, fused step
@pytest.mark.parametrize("copies", COPIES)
@pytest.mark.parametrize("name", SUM_NAMES)
def test_accumulate_equals_the_numpy_fp32_chain_bitwise_and_float64_within_the_bound(name, copies):
    """Bound: recursive summation of copies + 1 terms, each product rounded once -- the computed sum differs from the
    exact one by at most (copies + 2) * 2^-24 * (|acc| + sum_c |w_c * g_c|) to first order (Higham, Accuracy and
    Stability of Numerical Algorithms, eq. 4.4, with one more rounding for the products)."""
    from vqattack_amd import ops
    host, dev = _sum_data(name)
    w = ops.admix_weights(ops.si_scales(copies), 3)
    acc = dev["acc"].clone() if name != "offset" else _place(host["acc"], True)
    got = ops.admix_accumulate(dev["g"][:copies], w, acc)
    assert got is acc
    want = _accumulate_np(host["acc"], host["g"], w)
    _assert_bits(acc, want, "admix_accumulate")
    exact = host["acc"].astype(np.float64) + sum(np.float64(w[c]) * host["g"][c].astype(np.float64) for c in range(copies))
    mag = np.abs(host["acc"]).astype(np.float64) + sum(np.abs(np.float64(w[c]) * host["g"][c]) for c in range(copies))
    err = np.abs(acc.cpu().numpy().astype(np.float64) - exact)
    print("copies", copies, "max err / bound", float(np.max(err / ((copies + 2) * 2.0 ** -24 * mag))))
    assert np.all(err <= (copies + 2) * 2.0 ** -24 * mag)
    for c in range(copies):
        assert np.array_equal(dev["g"][c].cpu().numpy(), host["g"][c])


@pytest.mark.parametrize("copies", COPIES)
@pytest.mark.parametrize("name", SUM_NAMES)
def test_fused_step_equals_the_chain_and_the_two_launch_form_bitwise(name, copies):
    from vqattack_amd import ops
    host, dev = _sum_data(name)
    w = ops.admix_weights(ops.si_scales(copies), 3)
    grads = dev["g"][:copies]
    gsum_np = _accumulate_np(host["acc"], host["g"], w)
    two = ops.admix_accumulate(grads, w, dev["acc"].clone())
    for x0_key in ("x0", None):                                  # step form / FGM form
        x0_np, x0 = (host["x0"], dev["x0"]) if x0_key else (None, None)
        for clip in (True, False):                               # with and without a clip range
            lo, hi = (LO, HI) if clip else (None, None)
            got = ops.linf_admix_step(dev["x"], dev["acc"], grads, x0, w, EPS_ITER, EPS, lo, hi)
            _assert_bits(got, _update_np(host["x"], gsum_np, x0_np, clip), "linf_admix_step {} {}".format(x0_key, clip))
            ref = ops.linf_step(dev["x"], two, x0, EPS_ITER, EPS, lo, hi) if x0_key else \
                ops.linf_fgm(dev["x"], two, EPS_ITER, lo, hi)
            assert _same_bits(got, ref)
            xin = dev["x"].clone() if name != "offset" else _place(host["x"], True)
            assert ops.linf_admix_step(xin, dev["acc"], grads, x0, w, EPS_ITER, EPS, lo, hi, out=xin) is xin     # in place
            assert _same_bits(xin, got)
    assert np.array_equal(dev["acc"].cpu().numpy(), host["acc"])               # the fused form writes neither sum nor acc
    assert np.array_equal(dev["x"].cpu().numpy(), host["x"])


@pytest.mark.parametrize("form", ["step", "fgm"])
def test_range_flag_is_set_exactly_when_an_input_lies_outside_the_clip_range(form):
    from vqattack_amd import ops
    from vqattack_amd._hip import VQA_FLAG_RANGE
    host, dev = _sum_data("2x4100")
    w = ops.admix_weights(ops.si_scales(5), 3)
    x0 = dev["x0"] if form == "step" else None
    flag = ops.new_flag(DEV)
    ops.linf_admix_step(dev["x"], dev["acc"], dev["g"][:5], x0, w, EPS_ITER, EPS, LO, HI, flag=flag)
    assert int(flag.item()) == 0
    for idx, val in ((0, 1.5), (8199, -1.25), (4100, float("nan"))):
        x = dev["x"].clone()
        x.view(-1)[idx] = val
        flag = ops.new_flag(DEV)
        ops.linf_admix_step(x, dev["acc"], dev["g"][:5], x0, w, EPS_ITER, EPS, LO, HI, flag=flag)
        assert int(flag.item()) == VQA_FLAG_RANGE, (idx, val)
        flag = ops.new_flag(DEV)
        ops.linf_admix_step(x, dev["acc"], dev["g"][:5], x0, w, EPS_ITER, EPS, None, None, flag=flag)     # no range: no check
        assert int(flag.item()) == 0


@pytest.mark.parametrize("name", ["3x3x5x7", "2x4100"])
def test_si_combine_then_accumulate_is_the_fifteen_term_chain(name):
    """m1 = 5, m2 = 3: group 0 through si_combine, groups 1 and 2 through admix_accumulate (8 gradients are reused as 15)."""
    from vqattack_amd import ops
    host, dev = _sum_data(name)
    w = ops.admix_weights(ops.si_scales(5), 3)
    assert [float(v) for v in w] == [float(F(2.0 ** -i) / F(15)) for i in range(5)]
    order = [[0, 1, 2, 3, 4], [5, 6, 7, 0, 2], [4, 6, 1, 3, 5]]
    with np.errstate(all="ignore"):
        a = None
        for j in range(3):
            for i in range(5):
                term = F(w[i]) * host["g"][order[j][i]]
                a = term if a is None else a + term
    gsum = ops.si_combine([dev["g"][k] for k in order[0]], w)
    _assert_bits(gsum, _combine_np([host["g"][k] for k in order[0]], w), "group 0")
    for j in (1, 2):
        ops.admix_accumulate([dev["g"][k] for k in order[j]], w, gsum)
    _assert_bits(gsum, a, "15 terms")
    # and the fused end: groups 0 and 1 in the sum, group 2 in the step's own launch
    part = ops.admix_accumulate([dev["g"][k] for k in order[1]], w, ops.si_combine([dev["g"][k] for k in order[0]], w))
    got = ops.linf_admix_step(dev["x"], part, [dev["g"][k] for k in order[2]], dev["x0"], w, EPS_ITER, EPS, LO, HI)
    _assert_bits(got, _update_np(host["x"], a, host["x0"]), "fused end")


def test_sum_wrapper_checks():
    from vqattack_amd import ops
    from vqattack_amd._hip import HipExtensionError
    _, dev = _sum_data("2x4100")
    g, acc, x, x0 = dev["g"], dev["acc"].clone(), dev["x"], dev["x0"]
    w = ops.admix_weights(ops.si_scales(2), 3)
    with pytest.raises(TypeError):
        ops.admix_accumulate(g[0], w, acc)
    for bad in (lambda: ops.admix_accumulate([], w, acc), lambda: ops.admix_accumulate(g[:3], w, acc),
                lambda: ops.admix_accumulate(g[:2], w, acc[:1]), lambda: ops.admix_accumulate(g * 2, list(w) * 8, acc),
                lambda: ops.linf_admix_step(x, acc[:1], g[:2], x0, w, EPS_ITER, EPS, LO, HI),
                lambda: ops.linf_admix_step(x[:1], acc, g[:2], x0, w, EPS_ITER, EPS, LO, HI),
                lambda: ops.linf_admix_step(x, acc, g[:2], x0[:1], w, EPS_ITER, EPS, LO, HI)):
        with pytest.raises(ValueError):
            bad()
    for bad in (lambda: ops.admix_accumulate([g[0], acc], w, acc),                       # acc aliases a gradient
                lambda: ops.linf_admix_step(x, acc, g[:2], x0, w, EPS_ITER, EPS, LO, HI, out=acc),
                lambda: ops.linf_admix_step(x, acc, g[:2], x0, w, EPS_ITER, EPS, LO, HI, out=g[1]),
                lambda: ops.linf_admix_step(x, acc, g[:2], x0, w, EPS_ITER, EPS, LO, HI, out=x0)):
        with pytest.raises(HipExtensionError):
            bad()
    e = torch.empty((0, 4), device=DEV)
    assert ops.admix_accumulate([e, e], w, e) is e
    assert ops.linf_admix_step(e, e, [e, e], e, w, EPS_ITER, EPS, LO, HI).shape == (0, 4)
