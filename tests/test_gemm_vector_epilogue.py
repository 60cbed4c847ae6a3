"""The vector epilogues of the six large-tile bf16x6 GEMM kernels (``csrc/gemm.hip``): the MFMA operands are swapped so
that a lane holds four consecutive columns of a row, stored (and, for GELU', loaded) as one 16-byte access where ``C``,
``bias`` and ``aux`` are 16-byte aligned and ``ldc``, ``ldaux`` are multiples of 4, and as four dwords on the same lane map
where they are not.

Everything is compared BITWISE (``torch.equal``) against ``ops.gemm_small`` (unsplit), whose kernel keeps the
instruction's own operand order and its dword stores, and for the fused kernels against that GEMM followed by
``ops.gelu_fwd`` / ``ops.gelu_bwd``: no tolerance appears here.  The kernels are called through the C ABI, which takes
what ``ops.gemm`` does not: a stride that is no multiple of 4, pointers 1, 2 and 3 floats past a 16-byte boundary.
GPU: every combination of tile (N of one and three column tiles), M in {1, 15, 17, 255, 257} (a lone row, a ragged
16-row lane group, one row past a tile of either height), K of one and three k-steps, with and without bias, on both
paths of every kernel, with a sentinel around every view; NaN around (and in the rows >= M of) the h that GELU' reads;
one inf and one NaN in A.
CPU: the whole text of each kernel in the compiler's assembly -- 16-byte stores, no more dword stores than the scalar
path needs, 16-byte loads of h outside the loop, occupancy and scratch.
"""
import functools
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN_KERNELS = ["gemm_bf16x6_kernel", "gemm_bf16x6_wide_kernel"]
EPI_KERNELS = ["gemm_bf16x6_epi_kernel<1>", "gemm_bf16x6_epi_kernel<2>",
               "gemm_bf16x6_wide_epi_kernel<1>", "gemm_bf16x6_wide_epi_kernel<2>"]


# ---------------------------------------------------------------------------------------------------------- CPU
@functools.lru_cache(maxsize=None)
def _kernel_texts():
    """name -> (meta, every instruction of the kernel, the instructions of its loop), from the compiler's assembly."""
    spec = importlib.util.spec_from_file_location("isa_loop_mix", os.path.join(ROOT, "tools", "isa_loop_mix.py"))
    mix = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mix)
    path = mix.assembly("gemm.hip")
    loops = {name.split("::")[-1]: (meta, body) for name, meta, body in mix.kernels(path)}
    out = {}
    # the same split into kernels as tools/isa_loop_mix.py, keeping the whole text; the order of the two is the file's
    chunks = [k for k in re.split(r"\n(?=_ZN3vqa[^\n]*:\s+; @)", open(path).read()) if k.startswith("_ZN3vqa")]
    assert len(chunks) == len(loops)
    for (name, (meta, body)), chunk in zip(loops.items(), chunks):
        code = chunk.split(".section")[0]                      # the instructions end where the kernel's descriptor begins

        def ops(text):
            return [l.split()[0] for l in text.split("\n") if l.startswith("\t") and l.split() and not l.strip().startswith(";")]
        out[name] = (meta, ops(code), ops(body))
    return out


def _count(ops, name):
    return sum(o == name for o in ops)


@pytest.mark.parametrize("name", PLAIN_KERNELS + EPI_KERNELS)
def test_every_large_tile_kernel_stores_16_bytes_at_occupancy_two_without_scratch(name):
    meta, ops, loop = _kernel_texts()[name]
    print(name, meta, "dwordx4 stores", _count(ops, "global_store_dwordx4"), "dword stores", _count(ops, "global_store_dword"))
    assert _count(ops, "global_store_dwordx4") >= 16, "a lane's 16 tiles are not stored as 16-byte rows"
    assert not any(o.startswith("global_store") for o in loop), "a store inside the k-loop: the epilogue is not unrolled"
    assert meta["Occupancy"] == "2" and meta["ScratchSize"] == "0", meta


@pytest.mark.parametrize("name", PLAIN_KERNELS)
def test_plain_kernels_have_no_more_dword_stores_than_the_scalar_path(name):
    """16 tiles per lane: one 16-byte store each on the vector path, at most four dwords each on the scalar path (the
    compiler may merge those as well: a 16-byte store of 4-byte alignment is legal on this target).  Three copies of the
    epilogue -- vector unguarded, vector guarded, scalar guarded -- of 64 values per lane: 192 stored dwords in the
    kernel's text, and nothing narrower than a dword or odd in between."""
    _meta, ops, _loop = _kernel_texts()[name]
    x4, x1 = _count(ops, "global_store_dwordx4"), _count(ops, "global_store_dword")
    print(name, "dwordx4", x4, "dword", x1)
    assert x4 >= 32 and x1 <= 64
    assert not any(o.startswith("global_store") and o not in ("global_store_dword", "global_store_dwordx4") for o in ops)
    assert 4 * x4 + x1 == 192


@pytest.mark.parametrize("name", [EPI_KERNELS[1], EPI_KERNELS[3]])
def test_gelu_grad_kernels_load_h_16_bytes_at_a_time_outside_the_loop(name):
    """The loop's 16-byte loads are those of A (2 or 4), which the prologue issues once more; a lane's 16 tiles of h come
    on top of that, outside the loop."""
    _meta, ops, loop = _kernel_texts()[name]
    inside = _count(loop, "global_load_dwordx4")
    outside = _count(ops, "global_load_dwordx4") - inside
    print(name, "global_load_dwordx4 inside", inside, "outside", outside)
    assert inside in (2, 4)
    assert outside >= inside + 16


# ---------------------------------------------------------------------------------------------------------- GPU
SENTINEL = 7.0
TILES = {"large": 0, "wide": 1}
# (ldc - N, floats C starts past a 16-byte boundary, floats bias starts past one, ldaux - N, floats aux starts past one)
LAYOUTS = [
    (0, 0, 0, 0, 0), (4, 0, 0, 4, 0), (4, 0, 0, 0, 0), (0, 0, 0, 4, 0),                       # vector path
    (1, 0, 0, 0, 0), (2, 0, 0, 0, 0), (0, 1, 0, 0, 0), (0, 2, 0, 0, 0), (0, 3, 0, 0, 0),      # scalar: C or ldc
    (0, 0, 1, 0, 0),                                                                          # scalar: bias[1:]
    (0, 0, 0, 1, 0), (0, 0, 0, 2, 0), (0, 0, 0, 0, 1), (0, 0, 0, 0, 2), (0, 0, 0, 0, 3),      # scalar: aux or ldaux
    (1, 3, 1, 2, 1),
]


def _is_vector(layout, has_bias, has_aux):
    ldc, c_off, b_off, ldaux, aux_off = layout
    return ldc % 4 == 0 and c_off == 0 and (not has_bias or b_off == 0) and (not has_aux or (ldaux % 4 == 0 and aux_off == 0))


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


class _View:
    """An (M, N) view with row stride N + pad that starts ``off`` floats into a 16-byte-aligned buffer filled with
    ``fill``; the buffer ends one row and 8 floats behind the view."""

    def __init__(self, M, N, pad, off, fill=SENTINEL):
        torch, dev = _torch()
        self.ld = N + pad
        self.buf = torch.full((off + (M + 1) * self.ld + 8,), fill, device=dev)
        assert self.buf.data_ptr() % 16 == 0
        self.view = torch.as_strided(self.buf, (M, N), (self.ld, 1), off)
        assert self.view.data_ptr() % 16 == 4 * off
        inside = torch.zeros(self.buf.shape, dtype=torch.bool, device=dev)
        torch.as_strided(inside, (M, N), (self.ld, 1), off).fill_(True)
        self.outside = ~inside

    def untouched_outside(self, fill=SENTINEL):
        return bool((self.buf[self.outside] == fill).all())


def _call(tile, epilogue, a, pk, bias, out, aux=None):
    """The C entry points themselves: ``ops.gemm`` passes ldc = N to the plain kernels and refuses nothing else here."""
    from vqattack_amd import _hip
    lib, p = _hip.lib(), _hip.ptr
    M, K = a.shape
    N = pk.N
    if epilogue == 0:
        rc = lib.vqa_gemm_bf16x6_tile(p(a), a.stride(0), p(pk.data), p(bias), p(out.view), out.ld, M, N, K, TILES[tile],
                                      _hip.stream_for(a))
    else:
        rc = lib.vqa_gemm_bf16x6_epi(p(a), a.stride(0), p(pk.data), p(bias), p(out.view), out.ld, M, N, K, TILES[tile], epilogue,
                                     p(aux.view) if aux is not None else None, aux.ld if aux is not None else 0,
                                     _hip.stream_for(a))
    assert rc == 0, rc


@functools.lru_cache(maxsize=None)
def _case(M, N, K, has_bias):
    """Operands and the small kernel's results, computed once: (a, packed, a longer bias vector, h, gelu(h), the
    pre-activation GELU' reads, gemm * gelu'(that))."""
    torch, dev = _torch()
    from vqattack_amd import ops
    g = torch.Generator(device=dev).manual_seed(100000 * has_bias + 1000 * M + N + K)
    a = torch.randn(M, K, device=dev, generator=g)
    w = torch.randn(N, K, device=dev, generator=g) * 0.02
    bias_long = torch.randn(N + 4, device=dev, generator=g) * 0.02 if has_bias else None
    pk = ops.gemm_pack(w, trans=True)
    wants = {}
    for b_off in (0, 1) if has_bias else (0,):
        bias = bias_long[b_off:b_off + N].clone() if has_bias else None     # the small kernel gets an aligned copy
        h = ops.gemm_small(a, pk, bias)
        pre = torch.randn(M, N, device=dev, generator=torch.Generator(device=dev).manual_seed(M + N))
        wants[b_off] = (h, ops.gelu_fwd(h), pre, ops.gelu_bwd(pre, h.clone()))
    return a, pk, bias_long, wants


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 96])
@pytest.mark.parametrize("M", [1, 15, 17, 255, 257])
@pytest.mark.parametrize("tile,N", [("wide", 256), ("wide", 768), ("large", 128), ("large", 384)])
def test_both_paths_of_every_kernel_have_the_bits_of_the_small_kernel(tile, N, M, K):
    torch, dev = _torch()
    nan = float("nan")
    for has_bias in (True, False):
        a, pk, bias_long, wants = _case(M, N, K, has_bias)
        seen = set()
        for layout in LAYOUTS:
            ldc, c_off, b_off, ldaux, aux_off = layout
            if not has_bias:
                b_off = 0
            bias = bias_long[b_off:b_off + N] if has_bias else None
            assert bias is None or bias.data_ptr() % 16 == 4 * b_off
            h_want, act_want, pre, dh_want = wants[b_off]
            tag = (layout, has_bias)
            # plain
            if (ldc, c_off, b_off) not in seen:
                seen.add((ldc, c_off, b_off))
                out = _View(M, N, ldc, c_off)
                _call(tile, 0, a, pk, bias, out)
                assert torch.equal(out.view, h_want), ("plain", tag)
                assert out.untouched_outside(), ("plain wrote outside its view", tag)
            # GELU, h stored
            out, aux = _View(M, N, ldc, c_off), _View(M, N, ldaux, aux_off)
            _call(tile, 1, a, pk, bias, out, aux)
            assert torch.equal(aux.view, h_want), ("h", tag)
            assert torch.equal(out.view, act_want), ("gelu", tag)
            assert out.untouched_outside() and aux.untouched_outside(), ("gelu wrote outside a view", tag)
            # GELU, h not stored
            if (ldc, c_off, b_off, "nosave") not in seen:
                seen.add((ldc, c_off, b_off, "nosave"))
                out = _View(M, N, ldc, c_off)
                _call(tile, 1, a, pk, bias, out)
                assert torch.equal(out.view, act_want), ("gelu without aux", tag)
                assert out.untouched_outside(), ("gelu without aux wrote outside its view", tag)
            # GELU': NaN in the pad columns and the rows >= M of h
            out, aux = _View(M, N, ldc, c_off), _View(M, N, ldaux, aux_off, fill=nan)
            aux.view.copy_(pre)
            before = aux.buf.clone()
            _call(tile, 2, a, pk, bias, out, aux)
            assert torch.equal(out.view, dh_want), ("gelu_grad", tag)
            assert out.untouched_outside(), ("gelu_grad wrote outside its view", tag)
            assert torch.equal(aux.buf.view(torch.int32), before.view(torch.int32)), ("aux is read only", tag)
    # both paths were taken
    paths = {_is_vector(l, True, True) for l in LAYOUTS}
    assert paths == {True, False}


@pytest.mark.gpu
@pytest.mark.parametrize("tile,N", [("wide", 256), ("large", 128)])
def test_inf_and_nan_in_a_come_out_where_the_small_kernel_puts_them(tile, N):
    torch, dev = _torch()
    from vqattack_amd import ops
    M, K = 257, 96
    g = torch.Generator(device=dev).manual_seed(5)
    a = torch.randn(M, K, device=dev, generator=g)
    a[3, 40] = float("inf")
    a[200, 7] = float("nan")
    w = torch.randn(N, K, device=dev, generator=g) * 0.02
    bias = torch.randn(N, device=dev, generator=g) * 0.02
    pk = ops.gemm_pack(w, trans=True)
    want = ops.gemm_small(a, pk, bias)
    bad = ~torch.isfinite(want)
    assert bool(bad[3].all()) and bool(bad[200].all()) and int(bad.sum()) == 2 * N, "the small kernel's own rows"
    for pad in (0, 1):                                                   # vector path, scalar path
        out = _View(M, N, pad, 0)
        _call(tile, 0, a, pk, bias, out)
        assert torch.equal(~torch.isfinite(out.view), bad), (tile, pad)
        assert torch.equal(torch.isnan(out.view), torch.isnan(want)), (tile, pad)
        assert torch.equal(out.view[~bad], want[~bad]), (tile, pad)
        assert out.untouched_outside()
        for epi in (1, 2):
            res, aux = _View(M, N, pad, 0), _View(M, N, pad, 0)
            aux.view.copy_(torch.randn(M, N, device=dev, generator=g))
            _call(tile, epi, a, pk, bias, res, aux)
            assert torch.equal(~torch.isfinite(res.view), bad), (tile, pad, epi)
