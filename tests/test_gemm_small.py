"""The small-tile bf16x6 GEMM with deterministic split-K (``csrc/gemm.hip``: ``vqa_gemm_bf16x6_small``,
``ops.gemm_small`` / ``ops.gemm_small_plan``) and its dispatch in ``whitebox/_fused.py``.

GPU: ``ksplit == 1`` has the bits of the big kernel (same packed operand, same product and k-step order); ``ksplit > 1``
is, bit for bit, the ordered fp32 sum of the parts' products as the big kernel computes them on the K slices; error
against fp64 within twice the library's at the reference's batch-1 shapes; non-finite inputs; argument checking through
the raw ABI; graph replay; the fused encoder at batch 1 on the small kernel against the library path.
CPU: the planner and the dispatch rules under every ``VQA_GEMM`` value, with the GEMMs stubbed.
"""
import ctypes

import pytest


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _parts(nk, ksplit):
    return [(p * nk // ksplit, (p + 1) * nk // ksplit) for p in range(ksplit)]


# ---------------------------------------------------------------------------------------------------------- CPU
def test_plan_is_a_valid_split_for_a_grid_of_shapes():
    from vqattack_amd import ops
    for M in (1, 40, 63, 64, 65, 551, 577, 591, 1182, 2560, 4096, 37824):
        for N in (128, 768, 2304, 3072, 4096):
            for K in (32, 64, 96, 224, 768, 1024, 3072, 4096):
                k = ops.gemm_small_plan(M, N, K)
                assert isinstance(k, int) and 1 <= k <= min(K // 32, 8), (M, N, K, k)
                assert k == ops.gemm_small_plan(M, N, K)
                # every part keeps at least one k-step
                assert all(k1 > k0 for k0, k1 in _parts(K // 32, k))


def test_plan_does_not_split_a_grid_that_covers_the_device():
    from vqattack_amd import ops
    for N, K in ((768, 768), (2304, 768), (768, 3072), (3072, 768)):
        assert ops.gemm_small_plan(37824, N, K) == 1
    assert ops.gemm_small_plan(4096, 3072, 768) == 1               # 64 x 24 tiles
    assert ops.gemm_small_plan(591, 768, 3072) > 1                 # 60 tiles, 96 k-steps
    assert ops.gemm_small_plan(591, 768, 32) == 1                  # nothing to split


class _Packed:
    def __init__(self, K, N):
        self.K, self.N, self.data = K, N, None


def _dispatch_table(monkeypatch, mode):
    """Which GEMM ``_linear`` / ``_linear_grad`` pick for a table of shapes, with every GEMM stubbed."""
    import torch
    from vqattack_amd.whitebox import _fused
    if mode is None:
        monkeypatch.delenv("VQA_GEMM", raising=False)
    else:
        monkeypatch.setenv("VQA_GEMM", mode)
    picked = []
    monkeypatch.setattr(_fused.ops, "gemm", lambda a, pk, bias=None, out=None: picked.append("large"))
    monkeypatch.setattr(_fused.ops, "gemm_small",
                        lambda a, pk, bias=None, out=None, ksplit=1: picked.append(("small", ksplit)))
    monkeypatch.setattr(_fused.torch, "addmm", lambda *a, **k: picked.append("library"))
    monkeypatch.setattr(_fused.torch, "mm", lambda *a, **k: picked.append("library"))
    rows_nk = [(1, 768, 768), (591, 768, 768), (591, 2304, 768), (591, 768, 3072), (591, 3072, 768), (2560, 768, 768),
               (2560, 3072, 768), (8191, 768, 3072), (8192, 768, 768), (37824, 768, 768), (37824, 2304, 768)]
    table = []
    for M, N, K in rows_nk:
        a, w = torch.empty(M, K, device="meta"), torch.empty(N, K, device="meta")
        bias = torch.empty(N, device="meta")
        _fused._linear(a, w, bias, (_Packed(K, N), _Packed(N, K)))
        _fused._linear_grad(torch.empty(M, N, device="meta"), w, (_Packed(K, N), _Packed(N, K)))
        table.append(((M, N, K), picked[-2], picked[-1]))
    assert len(picked) == 2 * len(rows_nk)
    return table


def test_dispatch_large_is_the_big_kernel_from_the_threshold_up_and_the_library_below(monkeypatch):
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    assert _fused.MIN_WORKGROUPS == 192
    for (M, N, K), fwd, bwd in _dispatch_table(monkeypatch, "large"):
        assert fwd == ("large" if ops.gemm_workgroups(M, N) >= 192 else "library"), (M, N, K)
        assert bwd == ("large" if ops.gemm_workgroups(M, K) >= 192 else "library"), (M, N, K)
    # both sides of the threshold are in the table: 8192 x 768 is exactly 32 x 6 = 192 tiles, 2560 x 768 is 60
    assert ops.gemm_workgroups(8192, 768) == 192 and ops.gemm_workgroups(2560, 768) == 60


def test_dispatch_library_calls_neither_kernel(monkeypatch):
    for _shape, fwd, bwd in _dispatch_table(monkeypatch, "library"):
        assert fwd == "library" and bwd == "library"


def test_dispatch_small_takes_every_covered_shape_below_the_threshold(monkeypatch):
    from vqattack_amd import ops
    for (M, N, K), fwd, bwd in _dispatch_table(monkeypatch, "small"):
        assert fwd == ("large" if ops.gemm_workgroups(M, N) >= 192 else ("small", ops.gemm_small_plan(M, N, K))), (M, N, K)
        assert bwd == ("large" if ops.gemm_workgroups(M, K) >= 192 else ("small", ops.gemm_small_plan(M, K, N))), (M, N, K)


def test_dispatch_default_keeps_the_threshold_rule_and_follows_the_recorded_policy(monkeypatch):
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    for (M, N, K), fwd, bwd in _dispatch_table(monkeypatch, None):
        for rows, n, k, got in ((M, N, K, fwd), (M, K, N, bwd)):
            lo, hi = _fused.SMALL_POLICY.get((n, k), (1, 0))
            if ops.gemm_workgroups(rows, n) >= 192:
                assert got == "large"
            elif lo <= rows <= hi:
                assert got == ("small", ops.gemm_small_plan(rows, n, k))
            else:
                assert got == "library"


# ---------------------------------------------------------------------------------------------------------- GPU
def _operands(M, N, K, has_bias, pad, seed):
    torch, dev = _torch()
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(M, K + pad, device=dev, generator=g)[:, :K]
    w = torch.randn(N, K, device=dev, generator=g) * 0.02
    bias = torch.randn(N, device=dev, generator=g) * 0.02 if has_bias else None
    return a, w, bias


# row tails on either side of the 64-row tile, a single k-step, one and several column tiles, a strided A
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,has_bias,pad", [(1, 128, 32, True, 0), (63, 128, 64, False, 4), (65, 256, 96, True, 0),
                                                (130, 384, 3072, False, 0), (591, 768, 768, True, 8)])
def test_unsplit_small_kernel_has_the_bits_of_the_big_kernel(M, N, K, has_bias, pad):
    torch, dev = _torch()
    from vqattack_amd import ops
    a, w, bias = _operands(M, N, K, has_bias, pad, M + N + K)
    packed = ops.gemm_pack(w, trans=True)
    want = ops.gemm(a, packed, bias)
    buf = torch.full((M + 1, N), 7.0, device=dev)               # a sentinel row after the output
    got = ops.gemm_small(a, packed, bias, out=buf[:M])
    assert torch.equal(got, want)
    assert bool((buf[M] == 7.0).all()), "a row past M was written"
    assert torch.equal(ops.gemm_small(a, packed, bias), got), "not bitwise reproducible"


# K = 224 is 7 k-steps: 4 parts are uneven (boundaries 0, 1, 3, 5, 7) and 7 parts are one k-step each
@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,ksplit", [(65, 256, 224, 2), (65, 256, 224, 3), (65, 256, 224, 4), (65, 256, 224, 7),
                                          (591, 768, 3072, 2), (591, 768, 3072, 4), (591, 768, 3072, 8)])
def test_split_k_is_the_ordered_sum_of_its_parts(M, N, K, ksplit):
    torch, dev = _torch()
    from vqattack_amd import ops
    assert _parts(7, 4) == [(0, 1), (1, 3), (3, 5), (5, 7)]
    a, w, bias = _operands(M, N, K, True, 0, M + N + K + ksplit)
    want = None
    for k0, k1 in _parts(K // 32, ksplit):
        part = ops.gemm(a[:, 32 * k0:32 * k1], ops.gemm_pack(w[:, 32 * k0:32 * k1].contiguous(), trans=True))
        want = part if want is None else want + part
    want = want + bias
    buf = torch.full((M + 1, N), 7.0, device=dev)
    got = ops.gemm_small(a, ops.gemm_pack(w, trans=True), bias, out=buf[:M], ksplit=ksplit)
    assert torch.equal(got, want)
    assert bool((buf[M] == 7.0).all()), "a row past M was written"
    assert torch.equal(ops.gemm_small(a, ops.gemm_pack(w, trans=True), bias, ksplit=ksplit), got), "not reproducible"


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,trans", [(591, 768, 3072, True), (591, 3072, 768, True), (2560, 768, 768, True),
                                         (591, 768, 3072, False)])
def test_small_gemm_error_within_twice_the_library(M, N, K, trans):
    """The rule of test_gemm_split.py::test_gemm_error_within_twice_the_library: max and RMS error against an fp64
    product at most twice the library fp32 GEMM's, the library's taken on >= 4096 rows of the same data."""
    torch, dev = _torch()
    from vqattack_amd import ops
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    full = max(M, 4096)
    a_full = torch.randn(full, K, device=dev, generator=g)
    a = a_full[:M]
    # trans=True: a Linear weight [N, K] and its forward operand w.t(); trans=False: a weight [K, N] used as it is
    w = torch.randn((N, K) if trans else (K, N), device=dev, generator=g) * 0.02
    b = w.t() if trans else w
    bias = torch.randn(N, device=dev, generator=g) * 0.02 if trans else None
    ksplit = ops.gemm_small_plan(M, N, K)
    got = ops.gemm_small(a, ops.gemm_pack(w, trans=trans), bias, ksplit=ksplit)
    lib = torch.addmm(bias, a_full, b) if bias is not None else torch.mm(a_full, b)
    ref = a_full.double() @ b.double()
    if bias is not None:
        ref += bias.double()
    ek, el = (got.double() - ref[:M]).abs(), (lib.double() - ref).abs()
    print("small gemm {}x{}x{} ksplit {}: kernel/library max {:.3g}/{:.3g} rms {:.3g}/{:.3g}".format(
        M, N, K, ksplit, float(ek.max()), float(el.max()), float(ek.pow(2).mean().sqrt()), float(el.pow(2).mean().sqrt())))
    assert float(ek.max()) <= 2.0 * float(el.max()), (float(ek.max()), float(el.max()))
    assert float(ek.pow(2).mean().sqrt()) <= 2.0 * float(el.pow(2).mean().sqrt())


@pytest.mark.gpu
def test_small_gemm_keeps_inf_and_nan_non_finite():
    """The operands of test_gemm_split.py::test_gemm_keeps_inf_and_nan_non_finite."""
    torch, dev = _torch()
    from vqattack_amd import ops
    g = torch.Generator(device=dev).manual_seed(9)
    M, N, K = 300, 256, 256
    a = torch.randn(M, K, device=dev, generator=g)
    a[3, 5], a[10, 7], a[20, 100], a[299, 0] = float("inf"), float("-inf"), float("nan"), 3.3e38
    w = torch.randn(N, K, device=dev, generator=g) * 0.02 + 0.001
    packed = ops.gemm_pack(w, trans=True)
    big, one = ops.gemm(a, packed), ops.gemm_small(a, packed, ksplit=1)
    assert torch.equal(torch.isnan(one), torch.isnan(big))
    assert torch.equal(one[~torch.isnan(big)], big[~torch.isnan(big)])
    two = ops.gemm_small(a, packed, ksplit=2)
    assert torch.equal(torch.isfinite(two), torch.isfinite(torch.mm(a, w.t())))


@pytest.mark.gpu
def test_small_gemm_refuses_bad_arguments():
    torch, dev = _torch()
    from vqattack_amd import _hip, ops
    M, N, K = 70, 128, 96
    a, w, _ = _operands(M, N, K, False, 0, 1)
    packed = ops.gemm_pack(w, trans=True)
    for bad in (0, K // 32 + 1):
        with pytest.raises(ValueError):
            ops.gemm_small(a, packed, ksplit=bad)
    with pytest.raises(ValueError):
        ops.gemm_small(torch.randn(4, 64, device=dev), packed)                   # K mismatch
    with pytest.raises(_hip.HipExtensionError):
        ops.gemm_small(torch.randn(4, 100, device=dev)[:, 1:97], packed)         # 4-byte offset: not 16-byte aligned
    empty = ops.gemm_small(torch.empty(0, K, device=dev), packed, ksplit=2)
    assert tuple(empty.shape) == (0, N)

    lib = _hip.lib()
    assert lib.vqa_gemm_small_ws_bytes(M, N, 1) == 0
    assert lib.vqa_gemm_small_ws_bytes(M, N, 3) == 3 * M * N * 4
    assert lib.vqa_gemm_small_ws_bytes(M, 100, 2) == 0 and lib.vqa_gemm_small_ws_bytes(M, N, 17) == 0
    out = torch.full((M, N), 7.0, device=dev)
    ws = torch.empty(3 * M * N * 4 + 16, dtype=torch.uint8, device=dev)

    def raw(ksplit, ws_ptr, rows=M):
        return lib.vqa_gemm_bf16x6_small(_hip.ptr(a), a.stride(0), _hip.ptr(packed.data), None, _hip.ptr(out), N, rows, N,
                                         K, ksplit, ws_ptr, _hip.stream_for(a))
    assert raw(0, _hip.ptr(ws)) == -2 and raw(K // 32 + 1, _hip.ptr(ws)) == -2      # VQA_ERR_SHAPE
    assert raw(2, None) == -1                                                       # VQA_ERR_NULL
    assert raw(2, ctypes.c_void_p(ws.data_ptr() + 4)) == -3                         # VQA_ERR_ALIGN
    assert raw(2, None, rows=0) == -1 and raw(2, _hip.ptr(ws), rows=0) == 0         # same checks at M == 0, then VQA_OK
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    assert raw(3, _hip.ptr(ws)) == 0 and raw(1, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, ops.gemm(a, packed))


@pytest.mark.gpu
def test_split_k_replays_from_a_captured_graph():
    torch, dev = _torch()
    from vqattack_amd import ops
    M, N, K, ksplit = 591, 768, 3072, 4
    a, w, bias = _operands(M, N, K, True, 0, 11)
    packed = ops.gemm_pack(w, trans=True)
    out = torch.empty(M, N, device=dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                               # warm up off the capture
        ops.gemm_small(a, packed, bias, out=out, ksplit=ksplit)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                               # one stream, no parallel branches
        ops.gemm_small(a, packed, bias, out=out, ksplit=ksplit)
    g = torch.Generator(device=dev).manual_seed(12)
    for _ in range(2):
        a.copy_(torch.randn(M, K, device=dev, generator=g))
        out.fill_(7.0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.gemm_small(a, packed, bias, ksplit=ksplit))


def _encoder_small_against_library(monkeypatch, model, run):
    torch, dev = _torch()
    from vqattack_amd.whitebox import _fused
    model.fused_blocks = True
    calls = []
    real_small = _fused.ops.gemm_small

    def counting(*args, **kw):
        calls.append(kw.get("ksplit", 1))
        return real_small(*args, **kw)

    monkeypatch.setattr(_fused.ops, "gemm_small", counting)
    monkeypatch.setenv("VQA_GEMM", "small")
    outs_k, grad_k = run()
    assert len(calls) > 0, "the small kernel path was not taken"
    assert max(calls) > 1, "no GEMM of the encoder was split over K"
    n_small = len(calls)
    monkeypatch.setenv("VQA_GEMM", "library")
    outs_l, grad_l = run()
    assert len(calls) == n_small, "VQA_GEMM=library still ran the kernel"
    for k, (a, b) in enumerate(zip(outs_k, outs_l)):
        assert float((a - b).abs().max()) <= 5e-5 * max(1.0, float(b.abs().max())), k
    assert float((grad_k - grad_l).abs().max()) <= 5e-4 * float(grad_l.abs().max())


@pytest.mark.gpu
def test_vlmo_encoder_at_batch_one_on_the_small_kernel_matches_the_library_path(monkeypatch):
    """VLMO-base widths, batch 1, 384 x 384: the tolerances of
    test_gemm_split.py::test_fused_encoder_on_the_kernel_matches_the_library_path."""
    torch, dev = _torch()
    from vqattack_amd.whitebox.vlmo import FrozenVlmo, vlmo_base
    model = FrozenVlmo(vlmo_base(384), seed=0).to(dev)
    ids = torch.zeros(1, 40, dtype=torch.long, device=dev)
    ids[0, :10] = torch.tensor([101, 21, 22, 23, 24, 25, 26, 27, 28, 102], device=dev)
    masks = (ids != 0).long()
    g = torch.Generator(device=dev).manual_seed(3)
    image = torch.empty(1, 3, 384, 384, device=dev).uniform_(-1, 1, generator=g)
    emb = model.text_embeddings(ids)[:, :10]

    def run():
        img = image.clone().requires_grad_(True)
        feats, states = model.encode(img, emb, masks[:, :10])
        outs = feats[1:] + [states]
        gg = torch.Generator(device=dev).manual_seed(5)
        torch.autograd.backward(outs, [torch.randn(o.shape, device=dev, generator=gg) for o in outs], inputs=[img])
        return [o.detach() for o in outs], img.grad

    _encoder_small_against_library(monkeypatch, model, run)


@pytest.mark.gpu
def test_albef_vit_at_batch_one_on_the_small_kernel_matches_the_library_path(monkeypatch):
    """ALBEF's ViT at base width and depth (577 rows), batch 1; the text side is cut down, it is not run."""
    torch, dev = _torch()
    from vqattack_amd.whitebox.albef import FrozenAlbef, albef_base
    cfg = albef_base(384, bert_depth=2, fusion_layer=1, decoder_depth=1, vocab=1000, n_answers=5, k_test=3)
    model = FrozenAlbef(cfg, seed=0).to(dev)
    g = torch.Generator(device=dev).manual_seed(4)
    image = torch.empty(1, 3, 384, 384, device=dev).uniform_(-1, 1, generator=g)

    def run():
        img = image.clone().requires_grad_(True)
        states, feats = model.visual_encoder(img)
        outs = feats[1:] + [states]
        gg = torch.Generator(device=dev).manual_seed(6)
        torch.autograd.backward(outs, [torch.randn(o.shape, device=dev, generator=gg) for o in outs], inputs=[img])
        return [o.detach() for o in outs], img.grad

    _encoder_small_against_library(monkeypatch, model, run)
