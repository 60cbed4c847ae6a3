"""The variance-tuning (VMI / VNI-FGSM) kernels on the MI355X.

Arithmetic under test (include/vqattack_hip.h), fp32 with one rounding per operation:
    neighbours:  out[c] = base + r_{first + c},  base = x  or  x + lookahead * m,
                 r = (float(word >> 8) * 2^-24 * 2 - 1) * bound,  word e % 4 of Philox4x32-10 at counter
                 (j & 0xffffffff, j >> 32, first + c, t), j = block_offset + e // 4, key (seed_lo, seed_hi)
    accumulate:  acc = g_0 (init) or sum + g_0;  acc = acc + g_i  (i ascending);  sum = acc
    tune:        ghat = g + v;  v = w * vsum - g
    step:        vqa_linf_step / vqa_linf_fgm on ghat, which never reaches memory
Everything is compared BITWISE with the numpy fp32 chain written here (the Philox restatement is the one
tests/test_vt_host.py checks against the known answers), the fused step also with the two-launch form; the variance
additionally with float64 inside the bound derived below.

Shapes and placements as in tests/test_si_kernels.py: (3,3,5,7) n % 4 != 0: scalar path; (2,3,64,64) whole tiles only;
(2,4100) whole tiles and a partial one; "offset" the same from views one float off 16-byte alignment: scalar path;
"one_off" the same with only ONE gradient of the list misaligned; "flat" more tiles than the grid has workgroups
(256 CUs x 12), so the grid-stride loop goes round, and a partial tile; (64,3,592,592) 269 MB per tensor: the non-temporal
stores of a result larger than the Infinity Cache.
"""
import numpy as np
import pytest
import torch

from tests.pgd_reference import assert_bits as _assert_bits
from tests.pgd_reference import place as _place
from tests.pgd_reference import same_bits as _same_bits
from tests.pgd_reference import update_np

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
EPS_ITER, EPS, LO, HI = 0.01, 0.05, -1.0, 1.0
LOOKAHEAD = 0.009
BOUND = float(F(1.5 * EPS))
SEED = 0x9E3779B97F4A7C15
SMALL = ["3x3x5x7", "2x3x64x64", "2x4100", "offset", "one_off"]
PARTIAL = SMALL + ["2x11276"]          # 2819 16-byte pieces per row: a partial tile with whole slots and 3 lanes
COUNTS = [1, 3, 8]
FLAT = 256 * 12 * 2048 + 5 * 2048 + 1036          # > grid x the larger tile (2 x 256 pieces of 4 floats), partial tile
_SHAPES = {"3x3x5x7": (3, 3, 5, 7), "2x3x64x64": (2, 3, 64, 64), "2x4100": (2, 4100), "offset": (2, 4100),
           "one_off": (2, 4100), "flat": (FLAT,), "2x11276": (2, 11276)}
_cache = {}
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """numpy restatement: ``counter`` four and ``key`` two uint64 arrays (or ints) holding 32-bit values -> four words."""
    c = [np.asarray(v, dtype=np.uint64) for v in counter]
    k = [np.asarray(v, dtype=np.uint64) for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return [v.astype(np.uint32) for v in c]


def _noise_np(shape, seed, t, i, bound, block_offset=0):
    n = int(np.prod(shape))
    blocks = (n + 3) // 4
    j = (np.arange(blocks, dtype=np.uint64) + np.uint64(block_offset & 0xFFFFFFFFFFFFFFFF))       # wraps mod 2^64
    words = philox4x32_10((j & MASK, j >> np.uint64(32), i, t), (seed & 0xFFFFFFFF, seed >> 32))
    words = np.stack(words, axis=1).reshape(-1)[:n]
    u = (words >> np.uint32(8)).astype(F) * F(2.0 ** -24)
    r = (u * F(2.0) - F(1.0)) * F(bound)
    assert r.dtype == F
    return r.reshape(shape)


def _neighbors_np(x, seed, t, first, count, bound, m=None, lookahead=0.0, block_offset=0):
    base = x if m is None else x + F(lookahead) * m
    out = np.stack([base + _noise_np(x.shape, seed, t, first + c, bound, block_offset) for c in range(count)])
    assert out.dtype == F
    return out


def _data(name):
    """x0 in [-1, 1], x inside its ball, 9 gradients drawn as 1e-3 * N(0, 1) (the last one plays the centre's), a
    normal-draw momentum, a variance of the gradients' size: built once per shape and never changed."""
    if name not in _cache:
        shape = _SHAPES[name]
        r = np.random.RandomState(len(name) + shape[-1] % 1000)
        x0 = r.uniform(-1, 1, shape).astype(F)
        x = np.clip(x0 + r.uniform(-EPS, EPS, shape).astype(F), LO, HI).astype(F)
        m = r.standard_normal(shape).astype(F)
        n_g = 9 if name != "flat" else 4
        g = [(r.standard_normal(shape) * 1e-3).astype(F) for _ in range(n_g)]
        v = (r.standard_normal(shape) * 1e-3).astype(F)
        host = dict(x=x, x0=x0, m=m, g=g, v=v)
        off = name == "offset"
        dev = dict(x=_place(x, off), x0=_place(x0, off), m=_place(m, off), v=_place(v, off),
                   g=[_place(a, off or (name == "one_off" and i == 1)) for i, a in enumerate(g)])
        _cache[name] = (host, dev)
    return _cache[name]


def _update_np(x, ghat, x0, clip=True):
    return update_np(x, ghat, x0, EPS_ITER, EPS, LO, HI, clip)


def _key(t, seed=SEED):
    from vqattack_amd import ops
    return ops.vt_key_table(seed, t + 1, DEV)[t]


def _sum_np(g, start=None):
    with np.errstate(all="ignore"):
        acc = g[0] if start is None else start + g[0]
        for a in g[1:]:
            acc = acc + a
    assert acc.dtype == F
    return acc


def _tune_np(g, vsum, v, w):
    ghat = g + v
    nv = F(w) * vsum - g
    assert ghat.dtype == F and nv.dtype == F
    return ghat, nv


# ------------------------------------------------------------------------------------------------ neighbours
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", SMALL)
def test_neighbors_equal_the_numpy_chain_bitwise(name, count):
    from vqattack_amd import ops
    host, dev = _data(name)
    got = ops.vt_neighbors(dev["x"], _key(2), count, BOUND)
    assert got.shape == (count,) + host["x"].shape and got.is_contiguous()
    _assert_bits(got, _neighbors_np(host["x"], SEED, 2, 0, count, BOUND), "vt_neighbors")
    r = got.cpu().numpy() - host["x"]                      # every value inside [-bound, bound) up to the sum's rounding
    noise = np.stack([_noise_np(host["x"].shape, SEED, 2, c, BOUND) for c in range(count)])
    assert noise.min() >= -F(BOUND) and noise.max() < F(BOUND) and np.abs(r).max() <= BOUND * (1 + 2.0 ** -20)
    got_ni = ops.vt_neighbors(dev["x"], _key(2), count, BOUND, first=5, m=dev["m"], lookahead=LOOKAHEAD)
    _assert_bits(got_ni, _neighbors_np(host["x"], SEED, 2, 5, count, BOUND, host["m"], LOOKAHEAD),
                 "vt_neighbors with look-ahead, first = 5")
    out = torch.full((count,) + host["x"].shape, 7.0, device=DEV)
    assert ops.vt_neighbors(dev["x"], _key(2), count, BOUND, out=out) is out and _same_bits(out, got)
    assert np.array_equal(dev["x"].cpu().numpy(), host["x"]) and np.array_equal(dev["m"].cpu().numpy(), host["m"])


@pytest.mark.parametrize("name", SMALL)
def test_the_key_row_is_read_from_device_memory_at_every_launch(name):
    """Overwriting the row changes the output of the same launch arguments: what a replayed graph relies on."""
    from vqattack_amd import ops
    host, dev = _data(name)
    table = ops.vt_key_table(SEED, 8, DEV)
    row = torch.empty(3, dtype=torch.uint32, device=DEV)
    out = torch.empty((3,) + host["x"].shape, device=DEV)
    row.copy_(table[3])
    ops.vt_neighbors(dev["x"], row, 3, BOUND, out=out)
    first = out.clone()
    _assert_bits(first, _neighbors_np(host["x"], SEED, 3, 0, 3, BOUND), "t = 3")
    row.copy_(table[7])
    ops.vt_neighbors(dev["x"], row, 3, BOUND, out=out)
    _assert_bits(out, _neighbors_np(host["x"], SEED, 7, 0, 3, BOUND), "t = 7")
    assert not _same_bits(first, out)
    other = ops.vt_neighbors(dev["x"], ops.vt_key_table(SEED + 1, 8, DEV)[7], 3, BOUND)       # another seed, too
    _assert_bits(other, _neighbors_np(host["x"], SEED + 1, 7, 0, 3, BOUND), "seed + 1")
    assert not _same_bits(other, out)


@pytest.mark.parametrize("name", ["2x4100", "offset"])
def test_block_offset_carries_into_the_high_counter_word(name):
    from vqattack_amd import ops
    host, dev = _data(name)
    off = 2 ** 32 - 2
    got = ops.vt_neighbors(dev["x"], _key(1), 3, BOUND, block_offset=off)
    _assert_bits(got, _neighbors_np(host["x"], SEED, 1, 0, 3, BOUND, block_offset=off), "block_offset = 2^32 - 2")
    assert not _same_bits(got, ops.vt_neighbors(dev["x"], _key(1), 3, BOUND))
    # the values of an element depend on its block alone: the second row of the tensor, drawn on its own
    tail = ops.vt_neighbors(dev["x"][1:].contiguous(), _key(1), 3, BOUND, block_offset=off + 4100 // 4)
    assert _same_bits(tail[:, 0], got[:, 1])


@pytest.mark.parametrize("name", SMALL)
def test_a_chunk_of_eight_equals_eight_chunks_of_one(name):
    from vqattack_amd import ops
    host, dev = _data(name)
    whole = ops.vt_neighbors(dev["x"], _key(0), 8, BOUND, m=dev["m"], lookahead=LOOKAHEAD)
    for c in range(8):
        one = ops.vt_neighbors(dev["x"], _key(0), 1, BOUND, first=c, m=dev["m"], lookahead=LOOKAHEAD)
        assert _same_bits(one[0], whole[c]), c
    split = torch.cat([ops.vt_neighbors(dev["x"], _key(0), 3, BOUND, first=0, m=dev["m"], lookahead=LOOKAHEAD),
                       ops.vt_neighbors(dev["x"], _key(0), 5, BOUND, first=3, m=dev["m"], lookahead=LOOKAHEAD)])
    assert _same_bits(split, whole)


def test_neighbors_into_the_prefix_of_a_larger_buffer():
    """copy_stride > n: the neighbours of a batch prefix land in the prefix of each slot; the rest stays untouched."""
    from vqattack_amd import ops
    host, dev = _data("2x3x64x64")
    big = torch.full((3, 5, 3, 64, 64), 7.0, device=DEV)
    got = ops.vt_neighbors(dev["x"], _key(4), 3, BOUND, m=dev["m"], lookahead=LOOKAHEAD, out=big[:, :2])
    assert got.data_ptr() == big.data_ptr()
    _assert_bits(big[:, :2], _neighbors_np(host["x"], SEED, 4, 0, 3, BOUND, host["m"], LOOKAHEAD), "prefix")
    assert bool((big[:, 2:] == 7.0).all())
    with pytest.raises(ValueError):
        ops.vt_neighbors(dev["x"], _key(4), 3, BOUND, out=torch.zeros(3, 2, 3, 64, 128, device=DEV)[..., :64])


# ------------------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("init", [True, False])
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("name", PARTIAL)
def test_accumulate_equals_the_numpy_chain_bitwise_however_grouped(name, count, init):
    from vqattack_amd import ops
    host, dev = _data(name)
    off = name == "offset"
    start = host["v"]
    acc = _place(np.full_like(start, 7.0) if init else start, off)
    assert ops.vt_accumulate(dev["g"][:count], acc, init) is acc
    want = _sum_np(host["g"][:count], None if init else start)
    _assert_bits(acc, want, "vt_accumulate")
    one = _place(np.full_like(start, 7.0) if init else start, off)                    # one at a time: the same bits
    for c in range(count):
        ops.vt_accumulate([dev["g"][c]], one, init and c == 0)
    assert _same_bits(one, acc)
    for i in range(count):
        assert np.array_equal(dev["g"][i].cpu().numpy(), host["g"][i])                # the inputs are never written


# ------------------------------------------------------------------------------------------------ tune and fused step
@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("name", SMALL)
def test_tune_equals_the_numpy_chain_bitwise_and_the_variance_stays_inside_the_fp64_bound(name, in_place):
    """Against float64, with N = 8 neighbour gradients G_i, the centre's g and w = fp32(1) / fp32(N) taken as it is:
    the running sum S makes N - 1 roundings, so S = sum_i G_i (1 + a_i) with |a_i| <= gamma_{N-1}, gamma_k = k u /
    (1 - k u), u = 2^-24; the product w * S and the subtraction of g round once each, so
        v - (w sum_i G_i - g) = w sum_i G_i ((1 + a_i)(1 + d_1)(1 + d_2) - 1) - g d_2,   |d| <= u,
    which is at most gamma_{N+1} * w * sum_i |G_i| + u * |g| in magnitude.  Gradients are 1e-3 * N(0, 1): nothing is
    subnormal."""
    from vqattack_amd import ops
    host, dev = _data(name)
    off = name == "offset"
    n = 8
    w = float(F(1.0) / F(n))
    vsum = _place(np.zeros_like(host["v"]), off)
    ops.vt_accumulate(dev["g"][:n], vsum, True)
    g_host, g = host["g"][8], _place(host["g"][8], off)
    v = _place(host["v"], off)
    ghat = ops.vt_tune(g, vsum, v, w, out=g if in_place else None)
    assert (ghat is g) == in_place
    want_ghat, want_v = _tune_np(g_host, _sum_np(host["g"][:n]), host["v"], w)
    _assert_bits(ghat, want_ghat, "ghat")
    _assert_bits(v, want_v, "v")
    g64 = [a.astype(np.float64) for a in host["g"][:n]]
    exact = np.float64(F(w)) * sum(g64) - g_host.astype(np.float64)
    u = 2.0 ** -24
    bound = (n + 1) * u / (1 - (n + 1) * u) * np.float64(F(w)) * sum(np.abs(a) for a in g64) + u * np.abs(g_host.astype(np.float64))
    ratio = np.abs(v.cpu().numpy().astype(np.float64) - exact) / bound
    print("vt_tune", name, "worst |err| / bound vs fp64: %.4f" % ratio.max())
    assert ratio.max() <= 1.0, ratio.max()


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("with_x0", [True, False])
@pytest.mark.parametrize("name", PARTIAL)
def test_fused_step_equals_the_numpy_chain_and_the_two_launches_bitwise(name, with_x0, in_place):
    from vqattack_amd import ops
    host, dev = _data(name)
    off = name == "offset"
    w = float(F(1.0) / F(3))
    vsum_host = _sum_np(host["g"][:3])
    vsum = _place(vsum_host, off)
    g_host, g = host["g"][8], dev["g"][8]
    x0 = dev["x0"] if with_x0 else None
    v = _place(host["v"], off)
    x_fused = _place(host["x"], off) if in_place else dev["x"]
    got = ops.linf_vt_step(x_fused, g, vsum, v, x0, w, EPS_ITER, EPS, LO, HI, out=x_fused if in_place else None)
    assert (got is x_fused) == in_place
    want_ghat, want_v = _tune_np(g_host, vsum_host, host["v"], w)
    _assert_bits(got, _update_np(host["x"], want_ghat, host["x0"] if with_x0 else None), "linf_vt_step")
    _assert_bits(v, want_v, "v of the fused step")
    v2 = _place(host["v"], off)
    ghat = ops.vt_tune(g, vsum, v2, w)
    two = ops.linf_step(dev["x"], ghat, x0, EPS_ITER, EPS, LO, HI) if with_x0 else \
        ops.linf_fgm(dev["x"], ghat, EPS_ITER, LO, HI)
    assert _same_bits(got, two) and _same_bits(v, v2)
    assert np.array_equal(dev["x"].cpu().numpy(), host["x"]) and np.array_equal(g.cpu().numpy(), g_host)
    if with_x0:
        assert float((got - dev["x0"]).abs().max()) <= EPS + 1e-6
    assert float((got - dev["x"]).abs().max()) > 0


@pytest.mark.parametrize("with_x0", [True, False])
def test_fused_step_without_a_clip_range(with_x0):
    from vqattack_amd import ops
    host, dev = _data("2x4100")
    w = float(F(1.0) / F(3))
    vsum_host = _sum_np(host["g"][:3])
    v = _place(host["v"], False)
    got = ops.linf_vt_step(dev["x"], dev["g"][8], _place(vsum_host, False), v, dev["x0"] if with_x0 else None, w,
                           EPS_ITER, EPS, None, None)
    ghat, nv = _tune_np(host["g"][8], vsum_host, host["v"], w)
    _assert_bits(got, _update_np(host["x"], ghat, host["x0"] if with_x0 else None, clip=False), "no clip")
    _assert_bits(v, nv, "v")


@pytest.mark.parametrize("with_x0", [True, False])
@pytest.mark.parametrize("name", SMALL)
def test_range_flag_is_set_exactly_when_an_input_is_outside_the_clip_range(name, with_x0):
    from vqattack_amd import ops
    from vqattack_amd._hip import VQA_FLAG_RANGE
    host, dev = _data(name)
    off = name == "offset"
    x0 = dev["x0"] if with_x0 else None
    vsum = _place(host["g"][0], off)

    def run(x, lo=LO, hi=HI):
        flag = ops.new_flag(DEV)
        ops.linf_vt_step(x, dev["g"][8], vsum, _place(host["v"], off), x0, 0.5, EPS_ITER, EPS, lo, hi, flag=flag)
        return int(flag.item())

    assert run(dev["x"]) == 0
    for where, value in ((0, 1.5), (-1, -1.0000001), (host["x"].size // 2, float("nan"))):
        x = host["x"].copy()
        x.reshape(-1)[where] = value                                             # ONE element outside, first / last / middle
        assert run(_place(x, off)) == VQA_FLAG_RANGE, (where, value)
    x = host["x"].copy()                                                         # no clip range: nothing to check
    x.reshape(-1)[0] = 7.0
    assert run(_place(x, off), None, None) == 0


# ------------------------------------------------------------------------------------------------ more tiles than workgroups
def test_flat_tensor_with_more_tiles_than_the_grid_has_workgroups():
    from vqattack_amd import ops
    host, dev = _data("flat")
    _assert_bits(ops.vt_neighbors(dev["x"], _key(1), 2, BOUND, first=1, m=dev["m"], lookahead=LOOKAHEAD),
                 _neighbors_np(host["x"], SEED, 1, 1, 2, BOUND, host["m"], LOOKAHEAD), "vt_neighbors")
    vsum = torch.empty_like(dev["x"])
    ops.vt_accumulate(dev["g"][:3], vsum, True)
    vsum_host = _sum_np(host["g"][:3])
    _assert_bits(vsum, vsum_host, "vt_accumulate")
    ops.vt_accumulate(dev["g"][:1], vsum, False)
    vsum_host = _sum_np(host["g"][:1], vsum_host)
    _assert_bits(vsum, vsum_host, "vt_accumulate, not init")
    w = 0.25
    ghat_host, v_host = _tune_np(host["g"][3], vsum_host, host["v"], w)
    v = dev["v"].clone()
    _assert_bits(ops.vt_tune(dev["g"][3], vsum, v, w), ghat_host, "vt_tune")
    _assert_bits(v, v_host, "v")
    v = dev["v"].clone()
    _assert_bits(ops.linf_vt_step(dev["x"], dev["g"][3], vsum, v, dev["x0"], w, EPS_ITER, EPS, LO, HI),
                 _update_np(host["x"], ghat_host, host["x0"]), "linf_vt_step")
    _assert_bits(v, v_host, "v of the fused step")
    x, v = dev["x"].clone(), dev["v"].clone()
    ops.linf_vt_step(x, dev["g"][3], vsum, v, None, w, EPS_ITER, EPS, LO, HI, out=x)
    _assert_bits(x, _update_np(host["x"], ghat_host, None), "linf_vt_step without x0, in place")


# ------------------------------------------------------------------------------------------------ past the Infinity Cache
def test_large_result_takes_the_non_temporal_stores():
    """(64, 3, 592, 592): 269 MB per tensor, so every result is stored non-temporally.  The reference is the same entry
    point on the two halves of the batch (134 MB: the plain stores, compared with numpy above); for the neighbours the
    second half is drawn with the block offset of its first element."""
    from vqattack_amd import ops
    shape = (64, 3, 592, 592)
    half = 32 * 3 * 592 * 592
    gen = torch.Generator(DEV).manual_seed(64)
    x0 = torch.empty(shape, device=DEV).uniform_(-1, 1, generator=gen)
    x = (x0 + torch.empty(shape, device=DEV).uniform_(-EPS, EPS, generator=gen)).clamp_(-1, 1)
    g = [torch.randn(shape, device=DEV, generator=gen) * 1e-3 for _ in range(3)]
    key = _key(3)
    nb = ops.vt_neighbors(x, key, 1, BOUND, m=g[0], lookahead=LOOKAHEAD)
    assert _same_bits(nb[0, :32], ops.vt_neighbors(x[:32], key, 1, BOUND, m=g[0][:32], lookahead=LOOKAHEAD)[0])
    assert _same_bits(nb[0, 32:], ops.vt_neighbors(x[32:], key, 1, BOUND, m=g[0][32:], lookahead=LOOKAHEAD,
                                                   block_offset=half // 4)[0])
    del nb
    vsum, parts = torch.empty(shape, device=DEV), torch.empty(shape, device=DEV)
    ops.vt_accumulate(g[:2], vsum, True)
    ops.vt_accumulate(g[2:], vsum, False)
    for s in (slice(0, 32), slice(32, 64)):
        ops.vt_accumulate([a[s] for a in g[:2]], parts[s], True)
        ops.vt_accumulate([g[2][s]], parts[s], False)
    assert _same_bits(vsum, parts)
    v0 = g[1] * 0.5
    v, vh = v0.clone(), v0.clone()
    ghat = ops.vt_tune(g[0], vsum, v, 0.5)
    for s in (slice(0, 32), slice(32, 64)):
        ops.vt_tune(g[0][s], vsum[s], vh[s], 0.5, out=parts[s])
    assert _same_bits(ghat, parts) and _same_bits(v, vh)
    vf = v0.clone()
    got = ops.linf_vt_step(x, g[0], vsum, vf, x0, 0.5, EPS_ITER, EPS, LO, HI)
    assert _same_bits(got, ops.linf_step(x, ghat, x0, EPS_ITER, EPS, LO, HI)) and _same_bits(vf, v)
    vf = v0.clone()
    xi = x.clone()
    ops.linf_vt_step(xi, g[0], vsum, vf, None, 0.5, EPS_ITER, EPS, LO, HI, out=xi)
    assert _same_bits(xi, ops.linf_fgm(x, ghat, EPS_ITER, LO, HI)) and _same_bits(vf, v)


# ------------------------------------------------------------------------------------------------ wrappers
def test_wrappers_check_shapes_empty_tensors_aliases_and_cpu_tensors():
    from vqattack_amd import ops
    from vqattack_amd._hip import HipExtensionError
    host, dev = _data("2x4100")
    x, g, v = dev["x"], dev["g"], dev["v"].clone()
    key = _key(0)
    vsum = torch.zeros_like(x)
    wrong = torch.zeros(2, 4096, device=DEV)
    for bad in (lambda: ops.vt_neighbors(x, key, 0, BOUND), lambda: ops.vt_neighbors(x, key, 9, BOUND),
                lambda: ops.vt_neighbors(x, key, 2, BOUND, first=-1), lambda: ops.vt_neighbors(x, key, 2, BOUND, m=wrong),
                lambda: ops.vt_neighbors(x, key, 2, BOUND, out=torch.zeros(3, 2, 4100, device=DEV)),
                lambda: ops.vt_neighbors(x, torch.zeros(4, dtype=torch.uint32, device=DEV), 2, BOUND),
                lambda: ops.vt_neighbors(x, torch.zeros(3, dtype=torch.int32, device=DEV), 2, BOUND),
                lambda: ops.vt_accumulate([], vsum, True), lambda: ops.vt_accumulate(g[:9], vsum, True),
                lambda: ops.vt_accumulate([wrong], vsum, True), lambda: ops.vt_tune(g[0], wrong, v, 0.5),
                lambda: ops.vt_tune(g[0], vsum, wrong, 0.5), lambda: ops.vt_tune(g[0], vsum, v, 0.5, out=wrong),
                lambda: ops.linf_vt_step(x, wrong, vsum, v, dev["x0"], 0.5, EPS_ITER, EPS, LO, HI),
                lambda: ops.linf_vt_step(x, g[0], vsum, v, wrong, 0.5, EPS_ITER, EPS, LO, HI)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.vt_accumulate(g[0], vsum, True)
    for cpu in (lambda: ops.vt_neighbors(x.cpu(), key, 2, BOUND), lambda: ops.vt_neighbors(x, key.cpu(), 2, BOUND),
                lambda: ops.vt_accumulate([g[0].cpu()], vsum, True), lambda: ops.vt_tune(g[0].cpu(), vsum, v, 0.5),
                lambda: ops.linf_vt_step(x.cpu(), g[0], vsum, v, None, 0.5, EPS_ITER, EPS, LO, HI)):
        with pytest.raises(HipExtensionError):
            cpu()
    # aliases the entry points refuse (VQA_ERR_SHAPE): a sum that is one of its gradients, a variance that is the
    # gradient or the sum, a fused step written over the gradient, neighbours written over their source
    for alias in (lambda: ops.vt_accumulate([g[0], g[1]], g[1], False), lambda: ops.vt_tune(g[0], vsum, g[0], 0.5),
                  lambda: ops.vt_tune(g[0], vsum, vsum, 0.5), lambda: ops.vt_tune(g[0], vsum, v, 0.5, out=v),
                  lambda: ops.linf_vt_step(x, g[0], vsum, v, dev["x0"], 0.5, EPS_ITER, EPS, LO, HI, out=g[0]),
                  lambda: ops.linf_vt_step(x, g[0], vsum, v, dev["x0"], 0.5, EPS_ITER, EPS, LO, HI, out=dev["x0"]),
                  lambda: ops.vt_neighbors(x, key, 1, BOUND, out=x.view(1, 2, 4100))):
        with pytest.raises(HipExtensionError):
            alias()
    assert np.array_equal(g[0].cpu().numpy(), host["g"][0]) and np.array_equal(x.cpu().numpy(), host["x"])
    empty = torch.empty(0, 3, 8, 8, device=DEV)
    assert ops.vt_neighbors(empty, key, 2, BOUND).shape == (2, 0, 3, 8, 8)
    assert ops.vt_accumulate([empty], torch.empty_like(empty), True).numel() == 0
    assert ops.vt_tune(empty, empty.clone(), empty.clone(), 0.5).numel() == 0
    assert ops.linf_vt_step(empty, empty.clone(), empty.clone(), empty.clone(), None, 0.5, EPS_ITER, EPS, LO, HI).numel() == 0
    assert ops.VT_MAX_CHUNK == 8 and tuple(ops.vt_key_table(5 << 32 | 9, 3, DEV).cpu().numpy().astype(np.int64)[2]) == (9, 5, 2)
