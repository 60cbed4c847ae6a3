"""The 128 x 256 tile of the bf16x6 GEMM (``csrc/gemm.hip``: ``gemm_bf16x6_wide_kernel`` behind ``vqa_gemm_bf16x6_tile``,
``ops.gemm(..., tile="wide")``) and its dispatch in ``whitebox/_fused.py``.

GPU: the bits of the small kernel at ``ksplit == 1`` (code the wide tile shares nothing but the split and the packed
operand with) over row tails on both sides of the 128-row tile, a single k-step, one and several column tiles, a strided A
and the row clamp at M = 1; the fallback to the 256 x 128 tile where N % 256 != 0; non-finite inputs; error against fp64
within twice the library's.
CPU: the tile policy under every ``VQA_GEMM`` value with the GEMMs stubbed, and the instruction budget and the
placement of the global loads in the wide kernel's loop, read from the compiler's assembly.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------- CPU
class _Packed:
    def __init__(self, K, N):
        self.K, self.N, self.data = K, N, None


def _picked(monkeypatch, mode, policy, rows_nk):
    """What ``_linear`` / ``_linear_grad`` run for each (M, N, K), with every GEMM stubbed below ``ops.gemm``'s tile choice."""
    import torch
    from vqattack_amd.whitebox import _fused
    if mode is None:
        monkeypatch.delenv("VQA_GEMM", raising=False)
    else:
        monkeypatch.setenv("VQA_GEMM", mode)
    monkeypatch.setattr(_fused, "WIDE_POLICY", policy)
    picked = []
    monkeypatch.setattr(_fused.ops, "_gemm_tiled", lambda a, pk, bias, out, tile: picked.append(tile))
    monkeypatch.setattr(_fused.ops, "gemm_small", lambda a, pk, bias=None, out=None, ksplit=1: picked.append("small"))
    monkeypatch.setattr(_fused.torch, "addmm", lambda *a, **k: picked.append("library"))
    monkeypatch.setattr(_fused.torch, "mm", lambda *a, **k: picked.append("library"))
    table = {}
    for M, N, K in rows_nk:
        a, w = torch.empty(M, K, device="meta"), torch.empty(N, K, device="meta")
        _fused._linear(a, w, torch.empty(N, device="meta"), (_Packed(K, N), _Packed(N, K)))
        _fused._linear_grad(torch.empty(M, N, device="meta"), w, (_Packed(K, N), _Packed(N, K)))
        table[(M, N, K)] = (picked[-2], picked[-1])
    assert len(picked) == 2 * len(rows_nk)
    return table


# the benchmark's qkv projection and image-expert fc1 (forward / input gradient), and a shape below the grid threshold
_ROWS_NK = [(37824, 2304, 768), (35264, 3072, 768), (37824, 768, 768), (8192, 2304, 768), (591, 2304, 768)]
_POLICY = {(2304, 768): (30000, 40000), (768, 3072): (30000, 40000)}


def test_policy_sends_a_listed_shape_to_the_wide_tile_and_every_other_to_the_existing_kernel(monkeypatch):
    got = _picked(monkeypatch, None, _POLICY, _ROWS_NK)
    assert got[(37824, 2304, 768)] == ("wide", "large")       # forward listed; its gradient (N, K) = (768, 2304) is not
    assert got[(35264, 3072, 768)] == ("large", "wide")       # the gradient's (N, K) = (768, 3072) is listed
    assert got[(37824, 768, 768)] == ("large", "large")       # unlisted (N, K)
    assert got[(8192, 2304, 768)] == ("large", "large")       # listed (N, K), rows outside the recorded range
    assert got[(591, 2304, 768)] == ("library", "library")    # below the grid threshold: no tile at all
    assert all(v == ("large", "large") or k[0] == 591 for k, v in _picked(monkeypatch, None, {}, _ROWS_NK).items())


def test_forced_modes_ignore_the_policy(monkeypatch):
    for key, got in _picked(monkeypatch, "wide", {}, _ROWS_NK).items():
        assert got == (("library", "library") if key[0] == 591 else ("wide", "wide")), key
    for mode in ("large", "small"):
        below = ("small", "small") if mode == "small" else ("library", "library")
        for key, got in _picked(monkeypatch, mode, _POLICY, _ROWS_NK).items():
            assert got == (below if key[0] == 591 else ("large", "large")), (mode, key)
    for _key, got in _picked(monkeypatch, "library", _POLICY, _ROWS_NK).items():
        assert got == ("library", "library")


def test_shipped_policy_lists_only_shapes_the_wide_tile_covers(monkeypatch):
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    monkeypatch.delenv("VQA_GEMM", raising=False)
    for (n, k), (lo, hi) in _fused.WIDE_POLICY.items():
        assert n % 256 == 0 and k % 32 == 0 and 1 <= lo <= hi, (n, k, lo, hi)
        assert ops.gemm_workgroups(lo, n) >= _fused.MIN_WORKGROUPS
        assert _fused.gemm_tile(lo, n, k) == "wide" and _fused.gemm_tile(hi + 1, n, k) == "large"
    assert _fused.gemm_tile(37824, 640, 768) == "large"
    with pytest.raises(ValueError):
        ops.gemm(None, _Packed(32, 256), tile="tall")


def test_wide_loop_keeps_its_instruction_budget():
    """From the compiler's assembly (tools/isa_loop_mix.py): 96 MFMAs per k-step, no scratch, two waves per SIMD, and at
    most two thirds of the 256 x 128 kernel's other vector instructions (the split of A is halved; 69 against 121 when
    this was written)."""
    spec = importlib.util.spec_from_file_location("isa_loop_mix", os.path.join(ROOT, "tools", "isa_loop_mix.py"))
    mix = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mix)
    found = {}
    for name, meta, body in mix.kernels(mix.assembly("gemm.hip")):
        ins = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and l.split() and not l.strip().startswith(";")]
        mfma = sum(x.startswith("v_mfma") for x in ins)
        found[name.split("::")[-1]] = (meta, mfma, sum(x.startswith("v_") for x in ins) - mfma)
    meta, mfma, valu = found["gemm_bf16x6_wide_kernel"]
    _meta_big, mfma_big, valu_big = found["gemm_bf16x6_kernel"]
    print("wide: mfma {} valu {} {} | 256 x 128: mfma {} valu {}".format(mfma, valu, meta, mfma_big, valu_big))
    assert mfma == 96 and mfma_big == 96
    assert meta["ScratchSize"] == "0" and meta["Occupancy"] == "2", meta
    assert 3 * valu <= 2 * valu_big, (valu, valu_big)


def test_wide_loop_spaces_its_global_loads_among_the_mfmas():
    """The load placement is asked for with scheduling hints the compiler may drop: check the assembly.  At most two
    global loads ahead of the loop's first MFMA, never more than two without an MFMA between them, and all eight issued
    within the first half of the step's 96 MFMAs."""
    spec = importlib.util.spec_from_file_location("isa_loop_mix", os.path.join(ROOT, "tools", "isa_loop_mix.py"))
    mix = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mix)
    body = next(b for name, _meta, b in mix.kernels(mix.assembly("gemm.hip")) if name.endswith("gemm_bf16x6_wide_kernel"))
    ops_ = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and l.split()]
    seq = "".join("M" if o.startswith("v_mfma") else "G" for o in ops_ if o.startswith(("v_mfma", "global_load")))
    print(seq)
    assert seq.count("G") == 8 and seq.count("M") == 96
    assert seq.index("M") <= 2, "more than two global loads ahead of the first MFMA"
    assert "GGG" not in seq, "three global loads with no MFMA between them"
    assert seq[:seq.rindex("G")].count("M") <= 48, "a load of the next step issued in the second half of the step"


# ---------------------------------------------------------------------------------------------------------- GPU
def _operands(M, N, K, has_bias, pad, seed):
    torch, dev = _torch()
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(M, K + pad, device=dev, generator=g)[:, :K]
    w = torch.randn(N, K, device=dev, generator=g) * 0.02
    bias = torch.randn(N, device=dev, generator=g) * 0.02 if has_bias else None
    return a, w, bias


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 96, 768])
@pytest.mark.parametrize("N", [256, 512, 768])
@pytest.mark.parametrize("M", [1, 127, 129, 300])
def test_wide_tile_has_the_bits_of_the_small_kernel(M, N, K):
    torch, dev = _torch()
    from vqattack_amd import ops
    for has_bias, pad in ((True, 0), (False, 0), (True, 4), (False, 4)):
        a, w, bias = _operands(M, N, K, has_bias, pad, M + N + K + pad)
        assert a.stride(0) == K + pad
        packed = ops.gemm_pack(w, trans=True)
        want = ops.gemm_small(a, packed, bias, ksplit=1)
        buf = torch.full((M + 1, N), 7.0, device=dev)               # a sentinel row after the output
        got = ops.gemm(a, packed, bias, out=buf[:M], tile="wide")
        assert torch.equal(got, want), (has_bias, pad)
        assert bool((buf[M] == 7.0).all()), "a row past M was written"
        assert torch.equal(ops.gemm(a, packed, bias, tile="wide"), got), "not bitwise reproducible"


@pytest.mark.gpu
def test_forced_wide_tile_falls_back_to_the_existing_kernel_where_n_is_no_multiple_of_256(monkeypatch):
    torch, dev = _torch()
    from vqattack_amd import ops
    M, N, K = 300, 384, 96
    a, w, bias = _operands(M, N, K, True, 0, 5)
    packed = ops.gemm_pack(w, trans=True)
    want = ops.gemm(a, packed, bias, tile="large")
    assert torch.equal(want, ops.gemm_small(a, packed, bias, ksplit=1))
    buf = torch.full((M + 1, N), 7.0, device=dev)
    assert torch.equal(ops.gemm(a, packed, bias, out=buf[:M], tile="wide"), want)
    assert bool((buf[M] == 7.0).all()), "a row past M was written"
    monkeypatch.setenv("VQA_GEMM", "wide")
    assert torch.equal(ops.gemm(a, packed, bias), want)


@pytest.mark.gpu
def test_wide_tile_keeps_inf_and_nan_non_finite():
    """The operands and assertions of test_gemm_split.py::test_gemm_keeps_inf_and_nan_non_finite."""
    torch, dev = _torch()
    from vqattack_amd import ops
    g = torch.Generator(device=dev).manual_seed(9)
    M, N, K = 300, 256, 256
    a = torch.randn(M, K, device=dev, generator=g)
    a[3, 5], a[10, 7], a[20, 100], a[299, 0] = float("inf"), float("-inf"), float("nan"), 3.3e38
    w = torch.randn(N, K, device=dev, generator=g) * 0.02 + 0.001
    got = ops.gemm(a, ops.gemm_pack(w, trans=True), tile="wide")
    want = torch.mm(a, w.t())
    assert bool(torch.isnan(got)[torch.isnan(want)].all())
    assert torch.equal(torch.isfinite(got), torch.isfinite(want))
    fin = torch.isfinite(want) & (torch.arange(M, device=dev) != 299)[:, None]
    assert float((got - want)[fin].abs().max()) < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("M,N,K,has_bias", [(2560, 3072, 768, True), (4096, 768, 3072, False)])
def test_wide_tile_error_within_twice_the_library(M, N, K, has_bias):
    """The rule of test_gemm_split.py::test_gemm_error_within_twice_the_library: max and RMS error against an fp64
    product at most twice the library fp32 GEMM's, the library's taken on >= 4096 rows of the same data."""
    torch, dev = _torch()
    from vqattack_amd import ops
    g = torch.Generator(device=dev).manual_seed(M + N + K)
    a_full = torch.randn(max(M, 4096), K, device=dev, generator=g)
    a = a_full[:M]
    w = torch.randn(N, K, device=dev, generator=g) * 0.02
    bias = torch.randn(N, device=dev, generator=g) * 0.02 if has_bias else None
    got = ops.gemm(a, ops.gemm_pack(w, trans=True), bias, tile="wide")
    lib = torch.addmm(bias, a_full, w.t()) if has_bias else torch.mm(a_full, w.t())
    ref = a_full.double() @ w.t().double()
    if has_bias:
        ref += bias.double()
    ek, el = (got.double() - ref[:M]).abs(), (lib.double() - ref).abs()
    print("wide gemm {}x{}x{}: kernel/library max {:.3g}/{:.3g} rms {:.3g}/{:.3g}".format(
        M, N, K, float(ek.max()), float(el.max()), float(ek.pow(2).mean().sqrt()), float(el.pow(2).mean().sqrt())))
    assert float(ek.max()) <= 2.0 * float(el.max()), (float(ek.max()), float(el.max()))
    assert float(ek.pow(2).mean().sqrt()) <= 2.0 * float(el.pow(2).mean().sqrt())
