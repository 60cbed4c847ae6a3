"""Packed B of the bf16x6 GEMM goes from global memory straight into LDS (``csrc/gemm.hip``: ``stage_b16`` in
``gemm_bf16x6_kernel``, ``gemm_bf16x6_wide_kernel`` and their ``_epi`` copies); only A still passes through registers.

CPU, from the compiler's assembly (tools/isa_loop_mix.py): per k-step the six kernels issue 3 (256 x 128) or 6 (128 x 256)
``global_load_lds_dwordx4`` and write only the planes of A to LDS, keep 96 MFMAs, no scratch and two waves per SIMD; every
direct load is waited for (``vmcnt(0)``) ahead of the barrier that ends the step; the 256 x 128 loop spaces its seven loads
as the wide loop does.
GPU: the bits of the register-staged small kernel at ``ksplit == 1`` on both tiles, at the K where a direct load first
targets the idle buffer only (32), both buffers (64), a buffer again (96), and 128; at N whose later column blocks start
inside packed B; at M on both sides of both tiles' row counts and with several row blocks; with and without bias, a
strided A, a sentinel row behind the output, twice.  Both epilogues against GEMM + GELU kernel at an FFN shape.
"""
import functools
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LARGE = ("gemm_bf16x6_kernel", "gemm_bf16x6_epi_kernel<1>", "gemm_bf16x6_epi_kernel<2>")
WIDE = ("gemm_bf16x6_wide_kernel", "gemm_bf16x6_wide_epi_kernel<1>", "gemm_bf16x6_wide_epi_kernel<2>")
B_PIECES = dict([(k, 3) for k in LARGE] + [(k, 6) for k in WIDE])        # 16 B of packed B per thread and k-step
A_WRITES = dict([(k, 6) for k in LARGE] + [(k, 3) for k in WIDE])        # (row, 8-k) pieces of A x 3 planes


# ---------------------------------------------------------------------------------------------------------- CPU
@functools.lru_cache(maxsize=None)
def _mix():
    spec = importlib.util.spec_from_file_location("isa_loop_mix", os.path.join(ROOT, "tools", "isa_loop_mix.py"))
    mix = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mix)
    return mix


@functools.lru_cache(maxsize=None)
def _gemm_kernels():
    """name -> (meta, loop body) of every kernel of gemm.hip, from the compiler's assembly."""
    mix = _mix()
    return {name.split("::")[-1]: (meta, body) for name, meta, body in mix.kernels(mix.assembly("gemm.hip"))}


def _loop_lines(body):
    """(mnemonic, line) of the loop's instructions in layout order."""
    return [(l.split()[0], l) for l in body.split("\n") if l.startswith("\t") and l.split() and not l.strip().startswith(";")]


@pytest.mark.parametrize("name", LARGE + WIDE)
def test_loop_stages_b_without_registers_and_keeps_its_budget(name):
    meta, body = _gemm_kernels()[name]
    ops_ = [o for o, _l in _loop_lines(body)]
    direct = sum(o == "global_load_lds_dwordx4" for o in ops_)
    writes = sum(o == "ds_write_b128" for o in ops_)
    mfma = sum(o.startswith("v_mfma") for o in ops_)
    print(name, meta, "direct", direct, "ds_write_b128", writes, "mfma", mfma)
    assert direct == B_PIECES[name]
    assert sum(o.startswith("global_load_lds") for o in ops_) == direct, "a direct load of another width"
    assert writes == A_WRITES[name] and sum(o.startswith("ds_write") for o in ops_) == writes
    assert mfma == 96
    assert meta["ScratchSize"] == "0" and meta["Occupancy"] == "2", meta


@pytest.mark.parametrize("name", LARGE + WIDE)
def test_every_direct_load_is_waited_for_ahead_of_the_steps_barrier(name):
    """A direct-to-LDS load is a pending LDS write on the vector-memory counter: in layout order each one must be
    followed by an ``s_waitcnt`` that brings ``vmcnt`` to 0 before the loop's ``s_barrier``, and none is left pending
    where the loop ends."""
    _meta, body = _gemm_kernels()[name]
    seq = _mix().memory_sequence(body)
    print(name, " ".join(seq))
    assert seq.count("|") == 1, "the k-loop has one barrier per step"
    assert seq.count("L") == B_PIECES[name] + (4 if name in LARGE else 2)
    pending = seen = 0
    for op, line in _loop_lines(body):
        if op.startswith("global_load_lds"):
            pending, seen = pending + 1, seen + 1
        elif op == "s_waitcnt" and "vmcnt(0)" in line:
            pending = 0
        elif op == "s_barrier":
            assert pending == 0, "{} direct loads outstanding at the barrier".format(pending)
    assert seen == B_PIECES[name] and pending == 0


@pytest.mark.parametrize("name", LARGE)
def test_large_loop_spaces_its_global_loads_among_the_mfmas(name):
    """The conditions of test_gemm_wide.py::test_wide_loop_spaces_its_global_loads_among_the_mfmas for the 256 x 128
    tile's seven loads (four of A, three direct ones of B): at most two ahead of the first MFMA, never three in a row, all
    within the first half of the step's 96 MFMAs."""
    _meta, body = _gemm_kernels()[name]
    seq = "".join("M" if o.startswith("v_mfma") else "G" for o, _l in _loop_lines(body) if o.startswith(("v_mfma", "global_load")))
    print(seq)
    assert seq.count("G") == 7 and seq.count("M") == 96
    assert seq.index("M") <= 2, "more than two global loads ahead of the first MFMA"
    assert "GGG" not in seq, "three global loads with no MFMA between them"
    assert seq[:seq.rindex("G")].count("M") <= 48, "a load of the next step issued in the second half of the step"


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


_CASES = [("wide", n) for n in (256, 768)] + [("large", n) for n in (128, 384, 768)]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 64, 96, 128])
@pytest.mark.parametrize("M", [1, 255, 257, 513])
@pytest.mark.parametrize("tile,N", _CASES)
def test_direct_staged_tiles_have_the_bits_of_the_small_kernel(tile, N, M, K):
    torch, dev = _torch()
    from vqattack_amd import ops
    for has_bias, pad in ((True, 0), (False, 0), (True, 4), (False, 4)):
        a, w, bias = _operands(M, N, K, has_bias, pad, 7 * M + N + K + pad)
        assert a.stride(0) == K + pad
        packed = ops.gemm_pack(w, trans=True)
        want = ops.gemm_small(a, packed, bias, ksplit=1)
        buf = torch.full((M + 1, N), 7.0, device=dev)               # a sentinel row after the output
        got = ops.gemm(a, packed, bias, out=buf[:M], tile=tile)
        assert torch.equal(got, want), (has_bias, pad)
        assert bool((buf[M] == 7.0).all()), "a row past M was written"
        assert torch.equal(ops.gemm(a, packed, bias, tile=tile), got), "not bitwise reproducible"


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["wide", "large"])
def test_direct_staged_epilogues_have_the_bits_of_gemm_and_gelu_kernel(tile):
    """An FFN's shape at N = 768: fc1 forward and fc2 input gradient both have K = N / 4."""
    torch, dev = _torch()
    from vqattack_amd import ops
    M, N, K = 257, 768, 192
    g = torch.Generator(device=dev).manual_seed(11)
    for has_bias in (True, False):
        a = torch.randn(M, K + 4, device=dev, generator=g)[:, :K]
        w = torch.randn(N, K, device=dev, generator=g) * (2.0 / K ** 0.5)     # h spreads over both branches of erf2
        bias = torch.randn(N, device=dev, generator=g) if has_bias else None
        pk = ops.gemm_pack(w, trans=True)
        h_want = ops.gemm_small(a, pk, bias, ksplit=1)
        assert torch.equal(ops.gemm(a, pk, bias, tile=tile), h_want)
        act_want = ops.gelu_fwd(h_want)
        buf = torch.full((M + 1, N), 7.0, device=dev)
        aux = torch.empty(M, N, device=dev)
        got = ops.gemm(a, pk, bias, out=buf[:M], tile=tile, epilogue="gelu", aux=aux)
        assert torch.equal(aux, h_want) and torch.equal(got, act_want), ("gelu", has_bias)
        assert bool((buf[M] == 7.0).all()), "a row past M was written"
        h = torch.randn(M, N, device=dev, generator=g) * 2.0
        dh_want = ops.gelu_bwd(h, h_want.clone())
        buf2 = torch.full((M + 1, N), 7.0, device=dev)
        got2 = ops.gemm(a, pk, bias, out=buf2[:M], tile=tile, epilogue="gelu_grad", aux=h)
        assert torch.equal(got2, dh_want), ("gelu_grad", has_bias)
        assert bool((buf2[M] == 7.0).all()), "a row past M was written"
        assert torch.equal(ops.gemm(a, pk, bias, tile=tile, epilogue="gelu_grad", aux=h), got2), "not bitwise reproducible"
