"""The 128 x 128 tile of the bf16x6 GEMM (``csrc/gemm.hip``: ``gemm_bf16x6_half_kernel`` behind ``vqa_gemm_bf16x6_half``)
and the launch that hands the rows behind a large tile's last full round to it (``vqa_gemm_bf16x6_tail``,
``ops.gemm_tail_plan``, ``_fused.gemm_tail_split`` / ``TAIL_POLICY``).

CPU: the planner's values (worked out by hand below) and its invariants over a sweep; what the policy and its switches
send to the tail entry point, with the C calls stubbed; the new kernel's loop from the compiler's assembly
(tools/isa_loop_mix.py): 48 MFMAs per k-step, packed B straight into LDS, no scratch.
GPU: the bits of ``ops.gemm(tile="large")`` and of the register-staged small kernel at ``ksplit == 1`` for the half tile
alone and for every cut of a product, guard rows untouched; return codes; the fused encoder with every plain GEMM cut
against the same encoder with none.
"""
import ctypes
import functools
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = "gemm_bf16x6_half_kernel"


# ---------------------------------------------------------------------------------------------------------- CPU: plan
# (M, N, tile, cus) -> m_split.  256 CUs: 37824 x 768 is 148 x 6 = 888 large (296 x 3 wide) tiles, 3 full rounds = 768
# tiles = 32768 rows, the other 5056 rows are 40 x 6 = 240 half tiles; 35264 rows leave 2496 = 20 x 6 = 120; N = 2304:
# 148 x 18 = 2664 tiles, 2560 in full rounds, 2560 // 18 = 142 row blocks = 36352 rows, 1472 rows = 12 x 18 = 216 half
# tiles; N = 3072: 3552 tiles, 3328 // 24 = 138 row blocks, 2496 rows = 20 x 24 = 480 half tiles > 256: no cut.
PLAN = [
    (37824, 768, "large", 256, 32768), (37824, 768, "wide", 256, 32768), (35264, 768, "large", 256, 32768),
    (37824, 2304, "large", 256, 36352), (37824, 3072, "large", 256, 37824),
    (1024, 768, "large", 256, 1024), (1024, 768, "wide", 256, 1024),              # 24 tiles: below one round
    (65536, 128, "large", 256, 65536), (65536, 128, "wide", 256, 65536),          # 256 tiles: one round exactly
    (1600, 128, "large", 6, 1536),                                                # 7 tiles, 64 rows = 1 half tile
    (1600, 128, "large", 4, 1600),                                                # 4 of 7: 576 rows = 5 half tiles > 4
]


@pytest.mark.parametrize("M,N,tile,cus,want", PLAN)
def test_plan_values(M, N, tile, cus, want):
    from vqattack_amd import ops
    assert ops.gemm_tail_plan(M, N, tile, cus) == want


def test_plan_treats_the_wide_tile_at_an_n_it_does_not_cover_as_large():
    from vqattack_amd import ops
    for M in (1, 700, 1600, 5000, 37824):
        for cus in (1, 4, 6, 256):
            assert ops.gemm_tail_plan(M, 384, "wide", cus) == ops.gemm_tail_plan(M, 384, "large", cus)
    with pytest.raises(ValueError):
        ops.gemm_tail_plan(1600, 128, "tall", 6)


def test_plan_invariants_over_a_sweep():
    from vqattack_amd import ops
    cuts = 0
    for tile in ("large", "wide"):
        for N in (128, 256, 384, 768, 2304, 3072):
            bm, bn = (128, 256) if tile == "wide" and N % 256 == 0 else (256, 128)
            ntb = N // bn
            for cus in (1, 4, 6, 8, 64, 256, 304):
                for M in list(range(1, 2400, 37)) + [35264, 36000, 37824, 147712]:
                    s = ops.gemm_tail_plan(M, N, tile, cus)
                    assert 0 <= s <= M
                    if s == M:
                        continue
                    cuts += 1
                    assert s % bm == 0 and 0 < s
                    main = -(-s // bm) * ntb
                    nwg = -(-M // bm) * ntb
                    assert main <= (nwg // cus) * cus, "the main launch runs into a partial round"
                    assert -(-(M - s) // 128) * (N // 128) <= cus, "the half tiles do not fit one round"
    assert cuts > 100


# ---------------------------------------------------------------------------------------------------------- CPU: policy
class _Packed:
    def __init__(self, K, N):
        self.K, self.N, self.data = K, N, None


class _FakeLib:
    """Records which GEMM entry point ``ops._gemm_tiled`` calls, and the cut."""
    def __init__(self):
        self.calls = []

    def vqa_gemm_bf16x6_tile(self, *args):
        self.calls.append(("tile", args[6]))
        return 0

    def vqa_gemm_bf16x6_tail(self, *args):
        self.calls.append(("tail", args[10]))
        return 0

    def vqa_gemm_bf16x6_half(self, *args):
        self.calls.append(("half", 0))
        return 0


def _stub(monkeypatch, policy, tail=None, cus=None):
    """``ops._gemm_tiled`` on meta tensors with its C calls recorded; touching ``torch.cuda`` fails the test."""
    import torch
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    for name, value in (("VQA_GEMM_TAIL", tail), ("VQA_GEMM_TAIL_CUS", cus)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    monkeypatch.delenv("VQA_GEMM", raising=False)
    monkeypatch.setattr(_fused, "TAIL_POLICY", policy)
    fake = _FakeLib()
    monkeypatch.setattr(ops, "lib", lambda: fake)
    monkeypatch.setattr(ops, "dev_f32", lambda t, name, contiguous=True: t)
    monkeypatch.setattr(ops, "_p", lambda t: None)
    monkeypatch.setattr(ops, "ptr", lambda t: None)
    monkeypatch.setattr(ops, "stream_for", lambda t: None)

    def no_cuda(*a, **k):
        raise AssertionError("torch.cuda was touched")
    monkeypatch.setattr(torch.cuda, "get_device_properties", no_cuda)
    monkeypatch.setattr(torch.cuda, "current_device", no_cuda)

    def run(M, N, K, tile="large"):
        a = torch.empty(M, K, device="meta")
        out = ops._gemm_tiled(a, _Packed(K, N), None, None, tile)
        assert tuple(out.shape) == (M, N)
        return fake.calls[-1]
    return run


def test_empty_policy_never_calls_the_tail_entry_point(monkeypatch):
    run = _stub(monkeypatch, {})
    for M, N, K in ((1600, 128, 128), (37824, 768, 768), (35264, 768, 3072), (37824, 2304, 768)):
        for tile in ("large", "wide"):
            assert run(M, N, K, tile) == ("tile", M)


def test_switch_cuts_every_shape_the_plan_cuts(monkeypatch):
    run = _stub(monkeypatch, {}, tail="1", cus="6")
    assert run(1600, 128, 128) == ("tail", 1536)
    assert run(1600, 384, 128, "wide") == ("tail", 1536)          # 21 tiles, 18 in full rounds, 3 half tiles
    assert run(1024, 128, 128) == ("tile", 1024)                  # 4 tiles: below one round
    run = _stub(monkeypatch, {}, tail="1", cus="256")
    assert run(37824, 768, 768, "wide") == ("tail", 32768)
    assert run(37824, 3072, 768) == ("tile", 37824)


def test_listed_shape_is_cut_and_the_switch_overrides_it(monkeypatch):
    policy = {(768, 3072): (35264, 37824)}
    run = _stub(monkeypatch, policy, cus="256")
    assert run(35264, 768, 3072) == ("tail", 32768)
    assert run(37824, 768, 3072, "wide") == ("tail", 32768)
    assert run(37825, 768, 3072) == ("tile", 37825)               # rows outside the recorded range
    assert run(37824, 768, 768) == ("tile", 37824)                # unlisted (N, K)
    run = _stub(monkeypatch, policy, tail="0", cus="256")
    assert run(35264, 768, 3072) == ("tile", 35264)


def test_every_shipped_entry_is_a_shape_the_plan_cuts(monkeypatch):
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    for (n, k), (lo, hi) in _fused.TAIL_POLICY.items():
        assert n % 128 == 0 and k % 32 == 0 and 1 <= lo <= hi, (n, k, lo, hi)
        for rows in (lo, hi):
            assert ops.gemm_workgroups(rows, n) >= _fused.MIN_WORKGROUPS
            assert ops.gemm_tail_plan(rows, n, _fused.gemm_tile(rows, n, k), 256) < rows, (n, k, rows)


def test_explicit_cut_is_checked_by_the_wrapper():
    from vqattack_amd import ops
    import torch
    a = torch.empty(700, 64, device="meta")
    for bad in (-1, 701, 1.5, True):
        with pytest.raises(ValueError):
            ops.gemm(a, _Packed(64, 128), tile="large", m_split=bad)
    with pytest.raises(ValueError):
        ops.gemm(a, _Packed(64, 128), tile="large", epilogue="gelu", m_split=256)


def test_header_and_bindings_name_the_two_entry_points():
    from vqattack_amd import _hip
    header = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    for name, nargs in (("vqa_gemm_bf16x6_half", 10), ("vqa_gemm_bf16x6_tail", 12)):
        assert "int {}(".format(name) in header
        assert len(_hip.SIGNATURES[name][1]) == nargs
    assert _hip.ABI_VERSION == 4


# ---------------------------------------------------------------------------------------------------------- CPU: assembly
@functools.lru_cache(maxsize=None)
def _mix():
    spec = importlib.util.spec_from_file_location("isa_loop_mix", os.path.join(ROOT, "tools", "isa_loop_mix.py"))
    mix = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mix)
    return mix


@functools.lru_cache(maxsize=None)
def _half_kernel():
    mix = _mix()
    found = {name.split("::")[-1]: (meta, body) for name, meta, body in mix.kernels(mix.assembly("gemm.hip"))}
    return found[HALF]


def _loop_lines(body):
    return [(l.split()[0], l) for l in body.split("\n") if l.startswith("\t") and l.split() and not l.strip().startswith(";")]


def test_half_loop_stages_b_without_registers_and_keeps_its_budget():
    """Per k-step 6 products x 2 x 4 tiles = 48 MFMAs, 3 direct-to-LDS pieces of B, the three planes of one piece of A as
    the only LDS writes, 18 fragment reads; no scratch; 512 threads = two waves per SIMD."""
    meta, body = _half_kernel()
    ops_ = [o for o, _l in _loop_lines(body)]
    direct = sum(o == "global_load_lds_dwordx4" for o in ops_)
    writes = sum(o == "ds_write_b128" for o in ops_)
    reads = sum(o == "ds_read_b128" for o in ops_)
    mfma = sum(o.startswith("v_mfma") for o in ops_)
    print(HALF, meta, "direct", direct, "ds_write_b128", writes, "ds_read_b128", reads, "mfma", mfma)
    assert mfma == 48
    assert direct == 3 and sum(o.startswith("global_load_lds") for o in ops_) == 3
    assert writes == 3 and sum(o.startswith("ds_write") for o in ops_) == 3, "B is written to LDS from registers"
    assert reads == 18 and sum(o.startswith("ds_read") for o in ops_) == 18
    assert sum(o == "global_load_dwordx4" for o in ops_) == 2
    assert meta["ScratchSize"] == "0" and meta["Occupancy"] == "2", meta


def test_half_loop_waits_for_every_direct_load_ahead_of_the_steps_barrier():
    _meta, body = _half_kernel()
    seq = _mix().memory_sequence(body)
    print(HALF, " ".join(seq))
    assert seq.count("|") == 1 and seq.count("L") == 5
    pending = seen = 0
    for op, line in _loop_lines(body):
        if op.startswith("global_load_lds"):
            pending, seen = pending + 1, seen + 1
        elif op == "s_waitcnt" and "vmcnt(0)" in line:
            pending = 0
        elif op == "s_barrier":
            assert pending == 0, "{} direct loads outstanding at the barrier".format(pending)
    assert seen == 3 and pending == 0


def test_half_loop_issues_its_global_loads_in_the_first_half_of_the_step():
    _meta, body = _half_kernel()
    seq = "".join("M" if o.startswith("v_mfma") else "G" for o, _l in _loop_lines(body) if o.startswith(("v_mfma", "global_load")))
    print(seq)
    assert seq.count("G") == 5 and seq.count("M") == 48
    assert seq.index("M") <= 2, "more than two global loads ahead of the first MFMA"
    assert "GGG" not in seq, "three global loads with no MFMA between them"
    assert seq[:seq.rindex("G")].count("M") <= 24, "a load of the next step issued in the second half of the step"


# ---------------------------------------------------------------------------------------------------------- GPU
def _torch():
    import torch
    return torch, torch.device("cuda", 0)


def _operands(M, N, K, has_bias, pad, seed):
    torch, dev = _torch()
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(M, K + pad, device=dev, generator=g)[:, :K]
    w = torch.randn(N, K, device=dev, generator=g) * 0.02
    bias = torch.randn(N, device=dev, generator=g) * 0.02 if has_bias else None
    return a, w, bias


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 64, 96, 128])
@pytest.mark.parametrize("N", [128, 256, 384])
def test_half_tile_has_the_bits_of_the_large_tile_and_of_the_small_kernel(N, K):
    torch, dev = _torch()
    from vqattack_amd import ops
    for M in (1, 127, 128, 129, 257, 513):
        for has_bias, pad in ((True, 0), (False, 0), (True, 4), (False, 4)):
            a, w, bias = _operands(M, N, K, has_bias, pad, 7 * M + N + K + pad)
            assert a.stride(0) == K + pad
            packed = ops.gemm_pack(w, trans=True)
            want = ops.gemm_small(a, packed, bias, ksplit=1)
            assert torch.equal(ops.gemm(a, packed, bias, tile="large"), want)
            buf = torch.full((M + 1, N), 7.0, device=dev)               # a sentinel row after the output
            got = ops.gemm_half(a, packed, bias, out=buf[:M])
            assert torch.equal(got, want), (M, has_bias, pad)
            assert bool((buf[M] == 7.0).all()), "a row past M was written"
            assert torch.equal(ops.gemm_half(a, packed, bias), got), "not bitwise reproducible"


def _c_call(name, a, packed, bias, c_ptr, ldc, M, *rest):
    from vqattack_amd import _hip
    return getattr(_hip.lib(), name)(ctypes.c_void_p(a.data_ptr()), a.stride(0), ctypes.c_void_p(packed.data.data_ptr()),
                                     ctypes.c_void_p(bias.data_ptr()) if bias is not None else None,
                                     ctypes.c_void_p(c_ptr), ldc, M, packed.N, packed.K, *rest, _hip.stream_for(a))


@pytest.mark.gpu
@pytest.mark.parametrize("ldc_pad,c_off,b_off", [(1, 0, 0), (0, 1, 0), (0, 0, 1), (2, 3, 1)])
def test_scalar_path_of_the_half_tile_through_the_c_entry(ldc_pad, c_off, b_off):
    """A misaligned C or bias, or a row stride that is no multiple of 4 floats: the same lane map with dword accesses.
    Through vqa_gemm_bf16x6_half and through vqa_gemm_bf16x6_tail (whose second part starts at C + m_split * ldc)."""
    torch, dev = _torch()
    from vqattack_amd import ops
    M, N, K = 300, 256, 96
    a, w, bias_al = _operands(M, N, K, True, 0, 3)
    packed = ops.gemm_pack(w, trans=True)
    bias = torch.zeros(N + 4, device=dev)
    bias[b_off:b_off + N] = bias_al
    bias = bias[b_off:b_off + N]
    want = ops.gemm_small(a, packed, bias_al, ksplit=1)
    ldc = N + ldc_pad
    for entry, rest in (("vqa_gemm_bf16x6_half", ()), ("vqa_gemm_bf16x6_tail", (0, 256)), ("vqa_gemm_bf16x6_tail", (1, 128))):
        store = torch.full((c_off + (M + 1) * ldc,), 7.0, device=dev)
        assert _c_call(entry, a, packed, bias, store.data_ptr() + 4 * c_off, ldc, M, *rest) == 0
        torch.cuda.synchronize()
        view = store[c_off:].view(M + 1, ldc)
        assert torch.equal(view[:M, :N], want), (entry, rest)
        assert bool((view[:M, N:] == 7.0).all()) and bool((view[M] == 7.0).all()) and bool((store[:c_off] == 7.0).all())


@pytest.mark.gpu
def test_non_finite_rows_propagate_as_in_the_other_kernels():
    torch, dev = _torch()
    from vqattack_amd import ops
    M, N, K = 257, 256, 64
    a, w, bias = _operands(M, N, K, True, 0, 5)
    a = a.contiguous()
    a[3, 5], a[3, 40], a[130, 0], a[256, 63] = float("inf"), float("nan"), float("-inf"), 3.0e38
    packed = ops.gemm_pack(w, trans=True)
    want = ops.gemm_small(a, packed, bias, ksplit=1)
    got = ops.gemm_half(a, packed, bias)
    assert not bool(torch.isfinite(want[3]).any()) and bool(torch.isfinite(want[4]).all())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "NaN / inf bits differ"
    assert torch.equal(ops.gemm(a, packed, bias, tile="wide", m_split=128).view(torch.int32), want.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["large", "wide"])
@pytest.mark.parametrize("N", [128, 256])
def test_every_cut_has_the_bits_of_the_uncut_product(N, tile):
    torch, dev = _torch()
    from vqattack_amd import ops
    M, K, guard = 700, 96, 3
    for has_bias, pad in ((True, 0), (False, 4)):
        a, w, bias = _operands(M, N, K, has_bias, pad, N + pad)
        packed = ops.gemm_pack(w, trans=True)
        want = ops.gemm(a, packed, bias, tile=tile)
        assert torch.equal(want, ops.gemm_small(a, packed, bias, ksplit=1))
        for s in (0, 128, 256, 512, 700):
            buf = torch.full((M + guard, N), 7.0, device=dev)
            before = ops.TAIL_CALLS[0]
            got = ops.gemm(a, packed, bias, out=buf[:M], tile=tile, m_split=s)
            assert ops.TAIL_CALLS[0] == before + 1
            assert torch.equal(got, want), (s, has_bias, pad)
            assert bool((buf[M:] == 7.0).all()), "a row past M was written"


@pytest.mark.gpu
def test_return_codes():
    torch, dev = _torch()
    from vqattack_amd import ops
    M, N, K = 300, 128, 64
    a, w, bias = _operands(M, N, K, True, 0, 9)
    packed = ops.gemm_pack(w, trans=True)
    out = torch.full((M, N), 7.0, device=dev)
    codes = {}
    for label, m, rest in (("below", M, (0, -1)), ("above", M, (0, M + 1)), ("tile", M, (2, 128)), ("empty", 0, (0, 0)),
                           ("empty_wide", 0, (1, 0))):
        codes[label] = _c_call("vqa_gemm_bf16x6_tail", a, packed, bias, out.data_ptr(), N, m, *rest)
    codes["half_empty"] = _c_call("vqa_gemm_bf16x6_half", a, packed, bias, out.data_ptr(), N, 0)
    codes["half_ldc"] = _c_call("vqa_gemm_bf16x6_half", a, packed, bias, out.data_ptr(), N - 1, M)
    torch.cuda.synchronize()
    shape = -2                                                     # VQA_ERR_SHAPE of include/vqattack_hip.h
    assert _c_call("vqa_gemm_bf16x6_tile", a, packed, bias, out.data_ptr(), N, M, 2) == shape
    assert codes["below"] == codes["above"] == codes["tile"] == codes["half_ldc"] == shape, codes
    assert codes["empty"] == codes["empty_wide"] == codes["half_empty"] == 0, codes
    assert bool((out == 7.0).all()), "a refused or empty call wrote to C"


@pytest.mark.gpu
def test_encoder_with_every_gemm_cut_has_the_bits_of_the_encoder_with_none(monkeypatch):
    """64 samples x (8 text + 17 image tokens) = 1600 rows at width 128, head size 64.  With 6 CUs planned for, the
    attention projections (7, 21 tiles), the image expert's fc1 / fc2 gradient (20 tiles) and the VL-FFN are cut."""
    torch, dev = _torch()
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    from vqattack_amd.whitebox.vlmo import FrozenVlmo, VlmoConfig
    monkeypatch.delenv("VQA_GEMM", raising=False)
    monkeypatch.setattr(_fused, "MIN_WORKGROUPS", 1)
    monkeypatch.setenv("VQA_GEMM_TAIL_CUS", "6")
    cfg = VlmoConfig(dim=128, depth=2, heads=2, vlffn_start=1, image_size=32, patch=8, max_text_len=8, n_answers=7)
    model = FrozenVlmo(cfg, seed=3).to(dev)
    g = torch.Generator(device=dev).manual_seed(4)
    ids = torch.randint(3, 90, (64, 8), device=dev, generator=g)
    ids[:, 0] = 101
    ids[::2, 6:] = 0
    masks = (ids != 0).long()
    image = torch.empty(64, 3, 32, 32, device=dev).uniform_(-1, 1, generator=g)
    emb = model.text_embeddings(ids).detach()
    n_text = emb.shape[1]
    with torch.no_grad():
        x0 = torch.cat([emb + model.token_type_embeddings.weight[0],
                        model.visual_embed(image) + model.token_type_embeddings.weight[1]], dim=1)
    assert x0.shape[0] * x0.shape[1] == 1600
    bias = model.attention_bias(masks)
    spec = _fused.vlmo_spec(model)
    grads = None
    results = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("VQA_GEMM_TAIL", switch)
        before = ops.TAIL_CALLS[0]
        x = x0.clone().requires_grad_(True)
        feats, states = _fused.encode(x, spec, bias, n_text)
        outs = list(feats[1:]) + [states]
        if grads is None:
            grads = [torch.randn(o.shape, device=dev, generator=g) for o in outs]
        torch.autograd.backward(outs, grads, inputs=[x])
        results[switch] = ([o.detach() for o in outs], x.grad, ops.TAIL_CALLS[0] - before)
    assert results["0"][2] == 0, "VQA_GEMM_TAIL=0 reached the tail entry point"
    assert results["1"][2] >= 8, "the tail entry point did not run: {} calls".format(results["1"][2])
    for o0, o1 in zip(results["0"][0], results["1"][0]):
        assert torch.equal(o0, o1)
    assert float(results["0"][1].abs().max()) > 0 and torch.equal(results["0"][1], results["1"][1])
