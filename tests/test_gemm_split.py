"""The bf16x6 encoder GEMM (``csrc/gemm.hip``): the exact three-way bf16 split, the packed weight layout, and the kernel
against the library fp32 GEMM and an fp64 product.

CPU: a numpy restatement of the split (a0 = bf16(a), a1 = bf16(a - a0), a2 = bf16(a - a0 - a1), correction terms zero
when a0 is not finite) and of the packed layout documented in ``include/vqattack_hip.h``.  GPU: the device packer
against that restatement, the kernel's error against fp64 (at most 2x the library fp32 GEMM's, max and RMS) over the
benchmark shapes with row tails, bias and strided rows, run-to-run bit equality, inf / NaN propagation, and the fused
encoder on the kernel against the same encoder on the library path.
"""
import numpy as np
import pytest

F32_MAX_BF16_FINITE = np.array([0x7F7F7FFF], dtype=np.uint32).view(np.float32)[0]   # largest fp32 with a finite bf16


def bf16_rne(x):
    """fp32 -> the fp32 value of its round-to-nearest-even bf16 (NaN stays NaN, overflow goes to inf)."""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)
    out = r.view(np.float32).copy()
    out[np.isnan(x)] = np.nan
    return out


def split(a):
    a = np.asarray(a, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        a0 = bf16_rne(a)
        r = (a - a0).astype(np.float32)
        r = np.where(np.isfinite(r), r, np.float32(0)).astype(np.float32)
        a1 = bf16_rne(r)
        a2 = bf16_rne((r - a1).astype(np.float32))
    return a0, a1, a2


def bits16(x):
    """bf16 bit patterns of fp32 values that are exactly bf16 (NaN -> the canonical quiet NaN)."""
    u = (np.asarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)
    u[np.isnan(x)] = 0x7FC0
    return u


def pack_numpy(b):
    """B [K, N] fp32 -> packed bf16 bits [K/32][N/16][3][64][8]: element (k, n) at lane (n % 16) + 16 * ((k % 32) / 8),
    slot k % 8 of plane tile (k / 32, n / 16)."""
    K, N = b.shape
    planes = np.stack([bits16(p) for p in split(b)])                       # [3, K, N]
    t = planes.reshape(3, K // 32, 4, 8, N // 16, 16)                      # p, kt, kg, j, nt, c
    return np.ascontiguousarray(t.transpose(1, 4, 0, 2, 5, 3)).reshape(K // 32, N // 16, 3, 64, 8)


def unpack_numpy(packed, K, N):
    p = packed.reshape(K // 32, N // 16, 3, 4, 16, 8).transpose(2, 0, 3, 5, 1, 4).reshape(3, K, N)
    return [(p[i].astype(np.uint32) << 16).view(np.float32) for i in range(3)]


def _edge_values():
    tiny = np.float32(np.finfo(np.float32).tiny)
    return np.array([0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, tiny, tiny * 0.5, -tiny * 0.25, 1e-38, 3e38, -3e38,
                     F32_MAX_BF16_FINITE, -F32_MAX_BF16_FINITE, np.finfo(np.float32).max, np.inf, -np.inf, np.nan,
                     1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 65504.0, 0.1, 1.0 / 3.0, 2.0 ** -100, 2.0 ** 100],
                    dtype=np.float32)


def test_split_is_exact_on_random_and_edge_values():
    rng = np.random.default_rng(0)
    bits = rng.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    a = np.concatenate([bits.view(np.float32), rng.standard_normal(100000).astype(np.float32),
                        (rng.standard_normal(10000) * 1e-30).astype(np.float32), _edge_values()])
    a0, a1, a2 = split(a)
    for p in (a0, a1, a2):                                   # every piece is a bf16 value
        fin = np.isfinite(p)
        assert not (p[fin].view(np.uint32) & 0xFFFF).any()
    fin = np.isfinite(a) & (np.abs(a) <= F32_MAX_BF16_FINITE)
    total = a0[fin].astype(np.float64) + a1[fin].astype(np.float64) + a2[fin].astype(np.float64)
    # exact wherever the pieces stay above bf16's subnormal step 2^-133; below it at most that step is lost
    big = np.abs(a[fin]) >= 2.0 ** -100
    assert np.array_equal(total[big], a[fin][big].astype(np.float64))
    assert np.all(np.abs(total[~big] - a[fin][~big]) <= 2.0 ** -133)
    assert np.all(np.abs(a1[fin]) <= np.abs(a[fin]) * 2.0 ** -8) and np.all(np.abs(a2[fin]) <= np.abs(a[fin]) * 2.0 ** -16)
    # +-0 keep their sign in a0, and non-finite a (or a0 rounding to inf) carries no correction terms
    z = split(np.array([0.0, -0.0], dtype=np.float32))[0]
    assert np.array_equal(np.signbit(z), [False, True])
    nf = ~fin
    assert np.all(a1[nf] == 0) and np.all(a2[nf] == 0)
    assert np.array_equal(np.isnan(a0[nf]), np.isnan(a[nf]))
    assert np.all(np.isinf(a0[nf & ~np.isnan(a)]))


def test_packing_round_trip():
    rng = np.random.default_rng(1)
    K, N = 96, 48
    b = rng.standard_normal((K, N)).astype(np.float32)
    b.flat[:len(_edge_values())] = _edge_values()
    packed = pack_numpy(b)
    assert packed.shape == (K // 32, N // 16, 3, 64, 8)
    p0, p1, p2 = unpack_numpy(packed, K, N)
    s0, s1, s2 = split(b)
    for got, want in ((p0, s0), (p1, s1), (p2, s2)):
        assert np.array_equal(got, want, equal_nan=True)
    # spot-check the documented address of one element
    k, n = 37, 21
    lane, slot = (n % 16) + 16 * ((k % 32) // 8), k % 8
    assert packed[k // 32, n // 16, 0, lane, slot] == bits16(s0[k:k + 1, n])[0]


# ---------------------------------------------------------------------------------------------------------- GPU
def _torch():
    import torch
    return torch, torch.device("cuda", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("trans", [True, False])
def test_device_packer_matches_the_numpy_layout(trans):
    torch, dev = _torch()
    from vqattack_amd import ops
    rng = np.random.default_rng(2)
    out_f, in_f = 256, 128                                   # a Linear weight [out, in]
    w = (rng.standard_normal((out_f, in_f)) * 0.02).astype(np.float32)
    edge = np.array([0.0, -0.0, 1.0, 3e38, -3e38, np.inf, -np.inf, np.nan, 1e-30, 65504.0], dtype=np.float32)
    w.flat[:len(edge)] = edge
    packed = ops.gemm_pack(torch.from_numpy(w).to(dev), trans=trans)
    b = w.T if trans else w
    want = pack_numpy(np.ascontiguousarray(b))
    got = packed.data.cpu().numpy().view(np.uint16).reshape(want.shape)
    nan = (want & 0x7FFF) > 0x7F80
    assert np.array_equal((got & 0x7FFF) > 0x7F80, nan)
    assert np.array_equal(got[~nan], want[~nan])


# (M, N, K, bias, lda pad): the benchmark's GEMMs (VLMO-base rows 64 x 591, experts 64 x 40 / 64 x 551), ALBEF-base and
# VLMO-large widths, and row tails of 1, 17 and 591 rows
SHAPES = [(1, 768, 768, True, 0), (17, 2304, 768, True, 4), (591, 768, 3072, False, 0), (591, 3072, 768, True, 8),
          (2560, 3072, 768, True, 0), (2560, 768, 3072, False, 0), (37824, 2304, 768, True, 0),
          (37824, 768, 2304, False, 0), (37824, 768, 768, True, 12), (35264, 3072, 768, True, 0),
          (35264, 768, 3072, False, 0), (1000, 4096, 1024, True, 0), (1000, 1024, 4096, False, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,has_bias,pad", SHAPES)
def test_gemm_error_within_twice_the_library(M, N, K, has_bias, pad):
    torch, dev = _torch()
    from vqattack_amd import ops
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    # the library's error is taken on at least 4096 rows of the same data: at a few rows it runs a GEMV-style solution
    # with another summation order than at the workload's row counts, and a max over a few hundred outputs is noise
    full = max(M, 4096)
    a_store = torch.randn(full, K + pad, device=dev, generator=g)
    a = a_store[:M, :K]
    w = torch.randn(N, K, device=dev, generator=g) * 0.02
    bias = torch.randn(N, device=dev, generator=g) * 0.02 if has_bias else None
    packed = ops.gemm_pack(w, trans=True)
    buf = torch.full((M + 1, N), 7.0, device=dev)               # a sentinel row after the output
    out = ops.gemm(a, packed, bias, out=buf[:M])
    a_full = a_store[:, :K]
    lib = torch.addmm(bias, a_full, w.t()) if has_bias else torch.mm(a_full, w.t())
    ref = a_full.double() @ w.t().double()
    if has_bias:
        ref += bias.double()
    ek, el = (out.double() - ref[:M]).abs(), (lib.double() - ref).abs()
    assert float(ek.max()) <= 2.0 * float(el.max()), (float(ek.max()), float(el.max()))
    assert float(ek.pow(2).mean().sqrt()) <= 2.0 * float(el.pow(2).mean().sqrt())
    assert bool((buf[M] == 7.0).all()), "a row past M was written"
    again = ops.gemm(a, packed, bias)
    assert torch.equal(again, out), "not bitwise reproducible"
    # the input-gradient operand (trans=False) on the same weight: dA = dC @ W
    if N <= 2304 and M <= 2560:
        packed_b = ops.gemm_pack(w, trans=False)
        dc = torch.randn(full, N, device=dev, generator=g)
        got = ops.gemm(dc, packed_b)
        ref_b = dc.double() @ w.double()
        err_b, err_l = float((got.double() - ref_b).abs().max()), float((torch.mm(dc, w).double() - ref_b).abs().max())
        assert err_b <= 2.0 * err_l, (err_b, err_l)


@pytest.mark.gpu
def test_gemm_keeps_inf_and_nan_non_finite():
    """NaN in A gives NaN where fp32 does; inf gives a non-finite output wherever fp32 gives inf (it may be NaN instead:
    inf times a zero correction plane of an exactly-bf16 weight).  Finite outputs stay finite and accurate."""
    torch, dev = _torch()
    from vqattack_amd import ops
    g = torch.Generator(device=dev).manual_seed(9)
    M, N, K = 300, 256, 256
    a = torch.randn(M, K, device=dev, generator=g)
    a[3, 5], a[10, 7], a[20, 100], a[299, 0] = float("inf"), float("-inf"), float("nan"), 3.3e38
    w = torch.randn(N, K, device=dev, generator=g) * 0.02 + 0.001
    got = ops.gemm(a, ops.gemm_pack(w, trans=True))
    want = torch.mm(a, w.t())
    assert bool(torch.isnan(got)[torch.isnan(want)].all())
    assert torch.equal(torch.isfinite(got), torch.isfinite(want))
    fin = torch.isfinite(want) & (torch.arange(M, device=dev) != 299)[:, None]
    assert float((got - want)[fin].abs().max()) < 1e-4


@pytest.mark.gpu
def test_gemm_refuses_unsupported_operands():
    torch, dev = _torch()
    from vqattack_amd import _hip, ops
    w = torch.randn(256, 128, device=dev)
    with pytest.raises(ValueError):
        ops.gemm_pack(torch.randn(100, 128, device=dev), trans=True)            # N % 128
    packed = ops.gemm_pack(w, trans=True)
    with pytest.raises(ValueError):
        ops.gemm(torch.randn(4, 64, device=dev), packed)                         # K mismatch
    with pytest.raises(_hip.HipExtensionError):
        ops.gemm(torch.randn(4, 132, device=dev)[:, 1:129], packed)              # 4-byte offset: not 16-byte aligned


@pytest.mark.gpu
def test_fused_encoder_on_the_kernel_matches_the_library_path(monkeypatch):
    """VLMO-base widths, batch 2: every encoder GEMM on the bf16x6 kernel (grid threshold lowered) against VQA_GEMM=library;
    features and the input gradient within the whole-encoder tolerances of test_fused_blocks.py."""
    torch, dev = _torch()
    from vqattack_amd.whitebox import _fused
    from vqattack_amd.whitebox.vlmo import FrozenVlmo, vlmo_base
    model = FrozenVlmo(vlmo_base(384), seed=0).to(dev)
    model.fused_blocks = True
    ids = torch.zeros(2, 40, dtype=torch.long, device=dev)
    ids[0, :6] = torch.tensor([101, 11, 12, 13, 14, 102], device=dev)
    ids[1, :10] = torch.tensor([101, 21, 22, 23, 24, 25, 26, 27, 28, 102], device=dev)
    masks = (ids != 0).long()
    g = torch.Generator(device=dev).manual_seed(3)
    image = torch.empty(2, 3, 384, 384, device=dev).uniform_(-1, 1, generator=g)
    emb = model.text_embeddings(ids)[:, :10]
    calls = []
    real_gemm = _fused.ops.gemm

    def counting(*args, **kw):
        calls.append(1)
        return real_gemm(*args, **kw)

    def run(library):
        monkeypatch.setenv("VQA_GEMM", "library" if library else "kernel")
        img = image.clone().requires_grad_(True)
        feats, states = model.encode(img, emb, masks[:, :10])
        outs = feats[1:] + [states]
        gg = torch.Generator(device=dev).manual_seed(5)
        torch.autograd.backward(outs, [torch.randn(o.shape, device=dev, generator=gg) for o in outs], inputs=[img])
        return [o.detach() for o in outs], img.grad

    monkeypatch.setattr(_fused, "MIN_WORKGROUPS", 1)
    monkeypatch.setattr(_fused.ops, "gemm", counting)
    outs_k, grad_k = run(False)
    assert len(calls) > 0, "the kernel path was not taken"
    n_kernel = len(calls)
    outs_l, grad_l = run(True)
    assert len(calls) == n_kernel, "VQA_GEMM=library still ran the kernel"
    for k, (a, b) in enumerate(zip(outs_k, outs_l)):
        assert float((a - b).abs().max()) <= 5e-5 * max(1.0, float(b.abs().max())), k
    assert float((grad_k - grad_l).abs().max()) <= 5e-4 * float(grad_l.abs().max())


@pytest.mark.gpu
def test_packed_weights_follow_weight_updates(monkeypatch):
    """The packed planes live on the cached spec: an in-place weight update re-packs them (weights_key), and so does
    invalidate_fused() after a write through .data."""
    torch, dev = _torch()
    from vqattack_amd.whitebox import _fused
    from vqattack_amd.whitebox.vlmo import FrozenVlmo, VlmoConfig
    monkeypatch.setattr(_fused, "MIN_WORKGROUPS", 1)
    monkeypatch.setenv("VQA_GEMM", "kernel")
    cfg = VlmoConfig(dim=128, depth=3, heads=2, vlffn_start=2, image_size=32, patch=8, max_text_len=8, n_answers=7)
    model, donor = FrozenVlmo(cfg, seed=4).to(dev), FrozenVlmo(cfg, seed=9).to(dev)
    ids = torch.tensor([[101, 5, 6, 7, 102, 0, 0, 0], [101, 8, 9, 102, 0, 0, 0, 0]], device=dev)
    g = torch.Generator(device=dev).manual_seed(5)
    image = torch.empty(2, 3, 32, 32, device=dev).uniform_(-1, 1, generator=g)

    def fwd(m, fused):
        m.fused_blocks = fused
        with torch.no_grad():
            return m.encode(image, m.text_embeddings(ids), (ids != 0).long())[1]

    before = fwd(model, True)
    packed0 = model._fused_spec[1].layers[0].packed["qkv"][0].data.clone()
    with torch.no_grad():
        for p, q in zip(model.parameters(), donor.parameters()):
            p.copy_(q)
    after = fwd(model, True)
    assert not torch.equal(model._fused_spec[1].layers[0].packed["qkv"][0].data, packed0), "not re-packed"
    eager = fwd(model, False)
    assert float((after - before).abs().max()) > 1e-2
    assert float((after - eager).abs().max()) <= 2e-5 * float(eager.abs().max())
    with torch.no_grad():
        for p, q in zip(model.parameters(), donor.parameters()):
            p.data.mul_(0.5).add_(q.data * 0.5)
    model.invalidate_fused()
    assert float((fwd(model, True) - fwd(model, False)).abs().max()) <= 2e-5 * float(eager.abs().max())
