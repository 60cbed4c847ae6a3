"""The grouped launch of the bf16x6 GEMM (``csrc/gemm.hip``: ``gemm_bf16x6_grouped_kernel<EPI>`` behind
``vqa_gemm_bf16x6_grouped``, ``ops.gemm_grouped`` / ``ops.gemm_grouped_blocks``) and its dispatch for the two expert FFNs
of a multiway layer (``_fused._ffn_forward`` / ``_ffn_backward``, ``GROUPED_POLICY``, ``VQA_GEMM_GROUPED``).

CPU: the tile list's arithmetic (values worked out by hand below, invariants over a sweep); the entry point's return codes
(every check precedes the first HIP call); what the dispatch calls with the C-level wrappers stubbed, on meta tensors; the
new kernel's loop from the compiler's assembly (tools/isa_loop_mix.py).
GPU: per group the bits of ``ops.gemm(tile="wide")`` and of the register-staged small kernel at ``ksplit == 1``, over row
lists that put a group boundary inside and at a tile edge, empty groups, a tile count with an XCD remainder and four
groups, on the vector and the dword epilogue, sentinels around every output; both GELU epilogues against
``ops.gemm(..., epilogue=)``; a refused call writes nothing; the wrapper's fallback; a two-expert encoder with every pair
grouped against the same encoder with none; one call captured in a graph and replayed.
"""
import ctypes
import functools
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPED = ("gemm_bf16x6_grouped_kernel<0>", "gemm_bf16x6_grouped_kernel<1>", "gemm_bf16x6_grouped_kernel<2>")
ERR_NULL, ERR_SHAPE, ERR_ALIGN = -1, -2, -3

ROW_LISTS = [(1,), (128,), (129, 1), (0, 5), (200, 0, 77), (700, 45), (128, 128, 128, 128), (300, 7, 130, 64)]


# ---------------------------------------------------------------------------------------------------------- CPU: tile list
# 128-row blocks per group, cumulative, and starts[-1] * (N / 256) workgroups:
#   (700, 45) at N = 512: 6 and 1 blocks -> (0, 6, 7), 7 x 2 = 14;  (200, 0, 77) at 256: 2, 0, 1 -> (0, 2, 2, 3), 3;
#   (128, 128, 128, 128) at 256: one block each -> (0, 1, 2, 3, 4), 4;  (129, 1) at 768: 2 and 1 -> (0, 2, 3), 9;
#   (0, 5) at 256: (0, 0, 1), 1;  the benchmark's experts (36928, 896) at 3072: 289 and 7 -> (0, 289, 296), 296 x 12 = 3552.
BLOCKS = [
    ((700, 45), 512, (0, 6, 7), 14), ((200, 0, 77), 256, (0, 2, 2, 3), 3), ((128, 128, 128, 128), 256, (0, 1, 2, 3, 4), 4),
    ((129, 1), 768, (0, 2, 3), 9), ((0, 5), 256, (0, 0, 1), 1), ((36928, 896), 3072, (0, 289, 296), 3552),
    ((0, 0), 256, (0, 0, 0), 0), ((1,), 256, (0, 1), 1),
]


@pytest.mark.parametrize("Ms,N,starts,grid", BLOCKS)
def test_blocks_values(Ms, N, starts, grid):
    from vqattack_amd import ops
    assert ops.gemm_grouped_blocks(Ms, N) == (starts, grid)


def test_blocks_invariants_over_a_sweep():
    from vqattack_amd import ops
    seen = 0
    for N in (256, 512, 768, 3072):
        for a in (0, 1, 127, 128, 129, 700):
            for b in (0, 1, 45, 128, 300):
                for c in (None, 0, 77):
                    Ms = (a, b) if c is None else (a, c, b)
                    starts, grid = ops.gemm_grouped_blocks(Ms, N)
                    seen += 1
                    assert len(starts) == len(Ms) + 1 and starts[0] == 0
                    assert all(lo <= hi for lo, hi in zip(starts, starts[1:])), "the starts are not monotone"
                    for i, m in enumerate(Ms):
                        assert (starts[i + 1] == starts[i]) == (m == 0), "a group without rows has tiles"
                    # the grid of the wide kernel alone is ceil(M / 128) * (N / 256)
                    assert grid == sum(-(-m // 128) * (N // 256) for m in Ms)
                    assert ops.gemm_grouped_blocks([m for m in Ms if m], N)[1] == grid
    assert seen > 300
    for bad_n in (0, 128, 384):
        with pytest.raises(ValueError):
            ops.gemm_grouped_blocks((5,), bad_n)
    with pytest.raises(ValueError):
        ops.gemm_grouped_blocks((5, -1), 256)


# ---------------------------------------------------------------------------------------------------------- CPU: return codes
@functools.lru_cache(maxsize=None)
def _host_buffer():
    """ONE buffer for every table of this module, so that an address taken from one table means the same in another."""
    buf = (ctypes.c_char * 4096)()
    return buf, (ctypes.addressof(buf) + 63) & ~63


def _tables(n, **over):
    """Host tables of a well-formed call on n groups of 4 rows (host addresses: no launch is ever reached with a bad
    argument, and the good ones below have no rows), with entries replaced by ``over[name] = {group: value}``."""
    buf, base = _host_buffer()
    ptrs, longs = ctypes.c_void_p * max(n, 1), ctypes.c_long * max(n, 1)
    cols = dict(A=[base] * n, lda=[64] * n, packed=[base + 1024] * n, bias=[base + 2048] * n, C=[base + 3072] * n,
                ldc=[256] * n, aux=[base + 2560] * n, ldaux=[256] * n, M=[4] * n)
    for name, changes in over.items():
        for i, v in changes.items():
            cols[name][i] = v
    out = {k: (longs if k in ("lda", "ldc", "ldaux", "M") else ptrs)(*v) for k, v in cols.items()}
    out["_keep"] = buf
    return out, base


def _call(t, n, N=256, K=64, epilogue=0, aux=True):
    from vqattack_amd import _hip
    return _hip.lib().vqa_gemm_bf16x6_grouped(t["A"], t["lda"], t["packed"], t["bias"], t["C"], t["ldc"],
                                              t["aux"] if aux else None, t["ldaux"] if aux else None, t["M"], n, N, K,
                                              epilogue, None)


def test_argument_validation_returns_error_codes_without_touching_a_gpu():
    t, base = _tables(2)
    assert _call(t, 0) == ERR_SHAPE and _call(_tables(5)[0], 5) == ERR_SHAPE
    assert _call(t, 2, N=384) == ERR_SHAPE and _call(t, 2, N=128) == ERR_SHAPE and _call(t, 2, K=48) == ERR_SHAPE
    assert _call(t, 2, epilogue=3) == ERR_SHAPE and _call(t, 2, epilogue=-1) == ERR_SHAPE
    assert _call(_tables(2, M={1: -1})[0], 2) == ERR_SHAPE
    assert _call(_tables(2, M={0: 0, 1: -1})[0], 2) == ERR_SHAPE
    assert _call(_tables(2, A={1: None})[0], 2) == ERR_NULL
    assert _call(_tables(2, C={0: None})[0], 2) == ERR_NULL
    assert _call(_tables(2, packed={1: None})[0], 2) == ERR_NULL
    assert _call(t, 2, epilogue=2, aux=False) == ERR_NULL                       # GELU' without any aux
    assert _call(_tables(2, aux={1: None})[0], 2, epilogue=2) == ERR_NULL       # ... and without one group's
    assert _call(_tables(2, A={1: base + 4})[0], 2) == ERR_ALIGN                # A on a 4-byte boundary only
    assert _call(_tables(2, C={1: base + 3074})[0], 2) == ERR_ALIGN
    assert _call(_tables(2, lda={1: 66})[0], 2) == ERR_SHAPE and _call(_tables(2, lda={0: 32})[0], 2) == ERR_SHAPE
    assert _call(_tables(2, ldc={1: 255})[0], 2) == ERR_SHAPE
    assert _call(_tables(2, ldaux={1: 255})[0], 2, epilogue=1) == ERR_SHAPE
    assert _call(_tables(2, aux={0: base + 3072})[0], 2, epilogue=1) == ERR_SHAPE      # aux == C
    assert _call(_tables(2, aux={1: base})[0], 2, epilogue=2) == ERR_SHAPE             # aux == A
    assert _call(_tables(2, M={0: 1 << 40, 1: 1 << 40})[0], 2) == ERR_SHAPE            # more than 2^31 - 1 tiles
    # groups without rows are not looked at; all of them empty: VQA_OK and no launch
    empty = _tables(3, M={0: 0, 1: 0, 2: 0}, A={0: None, 1: base + 2}, C={2: None}, lda={1: 3})[0]
    assert _call(empty, 3) == 0 and _call(empty, 3, epilogue=2, aux=False) == 0
    assert _call(_tables(2, M={0: 0}, A={0: None}, C={1: None})[0], 2) == ERR_NULL     # ... but the others are


def test_header_and_binding_name_the_entry_point():
    from vqattack_amd import _hip, ops
    header = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    assert "int vqa_gemm_bf16x6_grouped(" in header and "#define VQA_GEMM_MAX_GROUPS 4" in header
    assert len(_hip.SIGNATURES["vqa_gemm_bf16x6_grouped"][1]) == 14
    assert ops.GEMM_MAX_GROUPS == 4 and _hip.ABI_VERSION == 4


# ---------------------------------------------------------------------------------------------------------- CPU: dispatch
class _Packed:
    def __init__(self, K, N):
        self.K, self.N, self.data = K, N, None


class _Layer:
    """The FFN part of a two-expert ``LayerSpec`` at width d on meta tensors."""
    def __init__(self, d, packed=True):
        import torch
        w1, b1 = torch.empty(4 * d, d, device="meta"), torch.empty(4 * d, device="meta")
        w2, b2 = torch.empty(d, 4 * d, device="meta"), torch.empty(d, device="meta")
        self.mlp = [(w1, b1, w2, b2), (w1, b1, w2, b2)]
        pair = lambda w: (_Packed(w.shape[1], w.shape[0]), _Packed(w.shape[0], w.shape[1])) if packed else (None, None)
        self.packed = {"fc1_0": pair(w1), "fc1_1": pair(w1), "fc2_0": pair(w2), "fc2_1": pair(w2)}


def _stub(monkeypatch, grouped=None, gemm=None, epilogue=None, policy=None):
    """``_ffn_forward`` + ``_ffn_backward`` of one layer with every GEMM wrapper recorded: returns run(rows, d) -> calls,
    each call (entry, rows per group in launch order, N, K, epilogue)."""
    import torch
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    for name, value in (("VQA_GEMM_GROUPED", grouped), ("VQA_GEMM", gemm), ("VQA_GEMM_EPILOGUE", epilogue)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)
    if policy is not None:
        monkeypatch.setattr(_fused, "GROUPED_POLICY", policy)
    calls = []

    def out(rows, n):
        return torch.empty(rows, n, device="meta")

    def gemm_grouped(a_list, packed_list, bias_list=None, out_list=None, epilogue=None, aux_list=None):
        assert len({(p.K, p.N) for p in packed_list}) == 1 and out_list is None
        if epilogue == "gelu_grad":
            assert [tuple(x.shape) for x in aux_list] == [(a.shape[0], packed_list[0].N) for a in a_list]
        calls.append(("grouped", tuple(a.shape[0] for a in a_list), packed_list[0].N, packed_list[0].K, epilogue))
        return [out(a.shape[0], p.N) for a, p in zip(a_list, packed_list)]

    def gemm_one(a, packed, bias=None, out_=None, tile=None, epilogue=None, aux=None, m_split=None):
        calls.append(("gemm", (a.shape[0],), packed.N, packed.K, epilogue))
        return out(a.shape[0], packed.N)

    def library(name):
        def run(*args):
            a, w = args[-2], args[-1]
            calls.append(("library", (a.shape[0],), w.shape[1], a.shape[1], None))
            return out(a.shape[0], w.shape[1])
        return run
    monkeypatch.setattr(ops, "gemm_grouped", gemm_grouped)
    monkeypatch.setattr(ops, "gemm", gemm_one)
    monkeypatch.setattr(ops, "gelu_fwd", lambda h, out=None: torch.empty_like(h))
    monkeypatch.setattr(ops, "gelu_bwd", lambda h, da, out=None: da)
    monkeypatch.setattr(torch, "addmm", library("addmm"))
    monkeypatch.setattr(torch, "mm", library("mm"))

    def run(rows, d, packed=True, save=True):
        del calls[:]
        lay = _Layer(d, packed)
        ys = [torch.empty(r, d, device="meta") for r in rows]
        hs, ms = _fused._ffn_forward(ys, lay, save)
        assert [tuple(m.shape) for m in ms] == [(r, d) for r in rows]
        assert [None if h is None else tuple(h.shape) for h in hs] == [(r, 4 * d) if save else None for r in rows]
        n_fwd = len(calls)
        if save:
            dys = _fused._ffn_backward([torch.empty(r, d, device="meta") for r in rows], hs, lay)
            assert [tuple(g.shape) for g in dys] == [(r, d) for r in rows]
        return calls[:n_fwd], calls[n_fwd:]
    return run


# VLMO-base at batch 64: 896 text rows (below MIN_WORKGROUPS at every FFN shape: library) and 36928 image rows
_TODAY_FWD = [("library", (896,), 3072, 768, None), ("library", (896,), 768, 3072, None),
              ("gemm", (36928,), 3072, 768, None), ("gemm", (36928,), 768, 3072, None)]
_TODAY_BWD = [("library", (896,), 3072, 768, None), ("library", (896,), 768, 3072, None),
              ("gemm", (36928,), 3072, 768, "gelu_grad"), ("gemm", (36928,), 768, 3072, None)]


def test_unset_switch_and_empty_policy_call_what_is_called_today(monkeypatch):
    from vqattack_amd.whitebox import _fused
    assert _fused.GROUPED_POLICY == {}, "the shipped policy groups something"
    run = _stub(monkeypatch)
    assert run((896, 36928), 768) == (_TODAY_FWD, _TODAY_BWD)
    assert run((896, 36928), 768, save=False)[0] == _TODAY_FWD


def test_switch_groups_every_ffn_gemm_larger_group_first(monkeypatch):
    run = _stub(monkeypatch, grouped="1")
    fwd, bwd = run((896, 36928), 768)
    # the shipped EPILOGUE_POLICY for the larger group's (rows, N, K): no fused GELU forward, fused GELU' backward
    assert fwd == [("grouped", (36928, 896), 3072, 768, None), ("grouped", (36928, 896), 768, 3072, None)]
    assert bwd == [("grouped", (36928, 896), 3072, 768, "gelu_grad"), ("grouped", (36928, 896), 768, 3072, None)]
    fwd, bwd = run((36928, 896), 768)                     # the larger group already first
    assert [c[1] for c in fwd + bwd] == [(36928, 896)] * 4
    run = _stub(monkeypatch, grouped="1", epilogue="1")
    fwd, bwd = run((896, 36928), 768)
    assert [c[4] for c in fwd] == ["gelu", None] and [c[4] for c in bwd] == ["gelu_grad", None]
    assert all(c[0] == "grouped" for c in fwd + bwd)
    run = _stub(monkeypatch, grouped="1", epilogue="0")
    fwd, bwd = run((896, 36928), 768)
    assert [c[4] for c in fwd + bwd] == [None] * 4 and all(c[0] == "grouped" for c in fwd + bwd)


def test_listed_class_is_grouped_and_the_switch_overrides_it(monkeypatch):
    policy = {(3072, 768): (35264, 37824)}                 # fc1 forward and fc2 gradient only
    run = _stub(monkeypatch, policy=policy)
    fwd, bwd = run((896, 36928), 768)
    assert fwd == [("grouped", (36928, 896), 3072, 768, None), ("library", (896,), 768, 3072, None),
                   ("gemm", (36928,), 768, 3072, None)]
    assert bwd == [("grouped", (36928, 896), 3072, 768, "gelu_grad"), ("library", (896,), 768, 3072, None),
                   ("gemm", (36928,), 768, 3072, None)]
    assert all(c[0] != "grouped" for c in sum(run((896, 40000), 768), []))      # rows outside the listed range
    run = _stub(monkeypatch, grouped="0", policy=policy)
    assert run((896, 36928), 768) == (_TODAY_FWD, _TODAY_BWD)


def test_switch_off_library_mode_and_small_pairs_group_nothing(monkeypatch):
    run = _stub(monkeypatch, grouped="0")
    assert run((896, 36928), 768) == (_TODAY_FWD, _TODAY_BWD)
    run = _stub(monkeypatch, grouped="1", gemm="library")
    assert all(c[0] == "library" for c in sum(run((896, 36928), 768), []))
    run = _stub(monkeypatch, grouped="1")
    # the larger side below MIN_WORKGROUPS (2560 x 768: 60 workgroups) is not grouped; at N = 3072 (240) it is
    fwd, bwd = run((896, 2560), 768)
    assert [c[0] for c in fwd] == ["grouped", "library", "library"] and fwd[0][1:4] == ((2560, 896), 3072, 768)
    assert [c[0] for c in bwd] == ["grouped", "library", "library"]
    fwd, bwd = run((100, 600), 768)
    assert all(c[0] == "library" for c in fwd + bwd)
    # an expert without rows, unpacked weights, and a width whose fc2 has N % 256 != 0
    assert all(c[0] != "grouped" for c in sum(run((0, 36928), 768), []))
    assert all(c[0] == "library" for c in sum(run((896, 36928), 768, packed=False), []))
    fwd, bwd = run((7000, 300000), 128)
    assert [c[0] for c in fwd] == ["grouped", "library", "gemm"] and [c[0] for c in bwd] == ["grouped", "library", "gemm"]


def test_wrapper_checks_its_lists():
    import torch
    from vqattack_amd import ops
    a = torch.empty(5, 64, device="meta")
    with pytest.raises(ValueError):
        ops.gemm_grouped([a, a], [_Packed(64, 256), _Packed(64, 512)])
    with pytest.raises(ValueError):
        ops.gemm_grouped([a, a], [_Packed(64, 256), _Packed(32, 256)])
    with pytest.raises(ValueError):
        ops.gemm_grouped([a, a], [_Packed(64, 256)])
    with pytest.raises(ValueError):
        ops.gemm_grouped([], [])
    with pytest.raises(ValueError):
        ops.gemm_grouped([a], [_Packed(64, 256)], epilogue="relu")
    with pytest.raises(ValueError):
        ops.gemm_grouped([a], [_Packed(64, 256)], epilogue="gelu_grad")
    with pytest.raises(ValueError):
        ops.gemm_grouped([a], [_Packed(64, 256)], aux_list=[torch.empty(5, 256, device="meta")])
    with pytest.raises(ValueError):
        ops.gemm_grouped([a, a], [_Packed(64, 256)] * 2, bias_list=[None])


# ---------------------------------------------------------------------------------------------------------- CPU: assembly
@functools.lru_cache(maxsize=None)
def _mix():
    spec = importlib.util.spec_from_file_location("isa_loop_mix", os.path.join(ROOT, "tools", "isa_loop_mix.py"))
    mix = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mix)
    return mix


@functools.lru_cache(maxsize=None)
def _gemm_kernels():
    mix = _mix()
    return {name.split("::")[-1]: (meta, body) for name, meta, body in mix.kernels(mix.assembly("gemm.hip"))}


def _loop_lines(body):
    return [(l.split()[0], l) for l in body.split("\n") if l.startswith("\t") and l.split() and not l.strip().startswith(";")]


@pytest.mark.parametrize("name", GROUPED)
def test_grouped_loop_is_the_wide_loop(name):
    """Per k-step 96 MFMAs, the six pieces of packed B as direct-to-LDS loads, the three planes of one piece of A as the
    only LDS writes, 24 fragment reads, two loads of A; no scratch; a register count that keeps two waves per SIMD (512
    threads: at most 256 registers).  The same counts as the wide kernel of the same epilogue."""
    kernels = _gemm_kernels()
    meta, body = kernels[name]
    wide = {"<0>": "gemm_bf16x6_wide_kernel", "<1>": "gemm_bf16x6_wide_epi_kernel<1>", "<2>": "gemm_bf16x6_wide_epi_kernel<2>"}
    ref = [o for o, _l in _loop_lines(kernels[wide[name[-3:]]][1])]
    ops_ = [o for o, _l in _loop_lines(body)]
    count = lambda seq, pre: sum(o.startswith(pre) for o in seq)
    print(name, meta, {pre: count(ops_, pre) for pre in ("v_mfma", "global_load_lds_dwordx4", "ds_write", "ds_read", "global_load")})
    assert count(ops_, "v_mfma") == 96
    assert sum(o == "global_load_lds_dwordx4" for o in ops_) == 6 and count(ops_, "global_load_lds") == 6
    assert sum(o == "ds_write_b128" for o in ops_) == 3 and count(ops_, "ds_write") == 3, "B is written to LDS from registers"
    assert sum(o == "ds_read_b128" for o in ops_) == 24 and count(ops_, "ds_read") == 24
    assert sum(o == "global_load_dwordx4" for o in ops_) == 2 and count(ops_, "global_load") == 8
    assert count(ops_, "scratch_") == 0 and count(ops_, "buffer_") == 0
    assert meta["ScratchSize"] == "0" and meta["Occupancy"] == "2" and int(meta["NumVgprs"]) <= 256, meta
    for pre in ("v_mfma", "global_load", "ds_write", "ds_read", "s_barrier"):
        assert count(ops_, pre) == count(ref, pre), pre
    valu = lambda seq: sum(o.startswith("v_") and not o.startswith("v_mfma") for o in seq)
    assert valu(ops_) <= valu(ref) + 4, (valu(ops_), valu(ref))


@pytest.mark.parametrize("name", GROUPED)
def test_grouped_loop_waits_for_its_direct_loads_and_spaces_its_global_loads(name):
    _meta, body = _gemm_kernels()[name]
    seq = _mix().memory_sequence(body)
    print(name, " ".join(seq))
    assert seq.count("|") == 1 and seq.count("L") == 8
    pending = seen = 0
    for op, line in _loop_lines(body):
        if op.startswith("global_load_lds"):
            pending, seen = pending + 1, seen + 1
        elif op == "s_waitcnt" and "vmcnt(0)" in line:
            pending = 0
        elif op == "s_barrier":
            assert pending == 0, "{} direct loads outstanding at the barrier".format(pending)
    assert seen == 6 and pending == 0
    order = "".join("M" if o.startswith("v_mfma") else "G" for o, _l in _loop_lines(body) if o.startswith(("v_mfma", "global_load")))
    assert order.index("M") <= 2, "more than two global loads ahead of the first MFMA"
    assert "GGG" not in order, "three global loads with no MFMA between them"
    assert order[:order.rindex("G")].count("M") <= 48, "a load of the next step issued in the second half of the step"


# ---------------------------------------------------------------------------------------------------------- GPU
def _torch():
    import torch
    return torch, torch.device("cuda", 0)


SENTINEL = 7.0


def _group(M, N, K, has_bias, pad, seed):
    torch, dev = _torch()
    from vqattack_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(M, K + pad, device=dev, generator=g)[:, :K]
    w = torch.randn(N, K, device=dev, generator=g) * 0.05
    bias = torch.randn(N, device=dev, generator=g) * 0.05 if has_bias else None
    return a, ops.gemm_pack(w, trans=True), bias


def _guarded(M, N, ldc, c_off, guard=2):
    """An (M, N) output view with row stride ldc, ``c_off`` floats into its buffer, every other float a sentinel."""
    torch, dev = _torch()
    store = torch.full((c_off + (M + guard) * ldc,), SENTINEL, device=dev)
    view = store[c_off:].view(M + guard, ldc)
    return store, view, view[:M, :N]


def _untouched(store, view, M, N, c_off):
    return bool((view[:M, N:] == SENTINEL).all()) and bool((view[M:] == SENTINEL).all()) and \
        bool((store[:c_off] == SENTINEL).all())


# (ldc - N, floats C is offset by, lda - K): the 16-byte epilogue on a padded C; the dword epilogue for an odd row stride
# and for a C one float off its 16-byte boundary
LAYOUTS = [(4, 0, 4), (1, 0, 0), (4, 1, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 64, 96, 128])
@pytest.mark.parametrize("N", [256, 512])
def test_every_group_has_the_bits_of_the_wide_tile_and_of_the_small_kernel(N, K):
    torch, dev = _torch()
    from vqattack_amd import ops
    for li, Ms in enumerate(ROW_LISTS):
        for vi, (ldc_pad, c_off, lda_pad) in enumerate(LAYOUTS):
            # a group with a bias beside one without; a lone group has one in the first layout only
            groups = [_group(M, N, K, (i + vi) % 2 == 0, lda_pad, 1000 * li + 10 * i + N + K) for i, M in enumerate(Ms)]
            want = []
            for a, packed, bias in groups:
                assert a.shape[0] <= 1 or a.stride(0) == K + lda_pad
                ref = ops.gemm(a, packed, bias, tile="wide")
                assert torch.equal(ref, ops.gemm_small(a, packed, bias, ksplit=1))
                want.append(ref)
            bufs = [_guarded(M, N, N + ldc_pad, c_off) for M in Ms]
            got = ops.gemm_grouped([g[0] for g in groups], [g[1] for g in groups], [g[2] for g in groups],
                                   out_list=[b[2] for b in bufs])
            assert len(got) == len(Ms)
            for i, (M, w, o, (store, view, _o)) in enumerate(zip(Ms, want, got, bufs)):
                assert torch.equal(o, w), (Ms, i, ldc_pad, c_off)
                assert _untouched(store, view, M, N, c_off), (Ms, i, "a float outside the output was written")
        fresh = ops.gemm_grouped([g[0] for g in groups], [g[1] for g in groups], [g[2] for g in groups])
        assert all(torch.equal(f, w) and f.is_contiguous() for f, w in zip(fresh, want)), "outputs of the wrapper's own"


@pytest.mark.gpu
@pytest.mark.parametrize("epilogue,with_aux", [("gelu", True), ("gelu", False), ("gelu_grad", True)])
@pytest.mark.parametrize("N,K", [(256, 64), (512, 96)])
def test_epilogues_have_the_bits_of_the_ungrouped_epilogue(N, K, epilogue, with_aux):
    torch, dev = _torch()
    from vqattack_amd import ops
    gen = torch.Generator(device=dev).manual_seed(N + K)
    for li, Ms in enumerate([(129, 1), (200, 0, 77), (300, 7, 130, 64)]):
        for vi, (ldc_pad, c_off, lda_pad) in enumerate(LAYOUTS):
            groups = [_group(M, N, K, (i + vi) % 2 == 0, lda_pad, 77 * li + 10 * i + N + K) for i, M in enumerate(Ms)]
            hs = [torch.randn(M, N, device=dev, generator=gen) for M in Ms]
            want, want_aux = [], []
            for (a, packed, bias), h in zip(groups, hs):
                if a.shape[0] == 0:                      # nothing to compare (and ops.gemm takes no empty aux)
                    want.append(torch.empty(0, N, device=dev)), want_aux.append(torch.empty(0, N, device=dev))
                elif epilogue == "gelu":
                    aux = torch.full_like(h, SENTINEL) if with_aux else None
                    want.append(ops.gemm(a, packed, bias, tile="wide", epilogue="gelu", aux=aux))
                    want_aux.append(aux)
                    if with_aux:                         # the two-step form: the plain product, then the GELU kernel
                        plain = ops.gemm_small(a, packed, bias, ksplit=1)
                        assert torch.equal(aux, plain) and torch.equal(want[-1], ops.gelu_fwd(plain))
                else:
                    want.append(ops.gemm(a, packed, bias, tile="wide", epilogue="gelu_grad", aux=h))
            bufs = [_guarded(M, N, N + ldc_pad, c_off) for M in Ms]
            if epilogue == "gelu":
                auxb = [_guarded(M, N, N + ldc_pad, c_off) for M in Ms] if with_aux else None
                aux_list = [b[2] for b in auxb] if with_aux else None
            else:
                auxb, aux_list = None, hs
            keep = [h.clone() for h in hs]
            got = ops.gemm_grouped([g[0] for g in groups], [g[1] for g in groups], [g[2] for g in groups],
                                   out_list=[b[2] for b in bufs], epilogue=epilogue, aux_list=aux_list)
            for i, (M, w, o, (store, view, _o)) in enumerate(zip(Ms, want, got, bufs)):
                assert torch.equal(o, w), (Ms, i, ldc_pad, c_off)
                assert _untouched(store, view, M, N, c_off)
                if auxb is not None:
                    assert torch.equal(auxb[i][2], want_aux[i]) and _untouched(auxb[i][0], auxb[i][1], M, N, c_off)
            assert all(torch.equal(h, k) for h, k in zip(hs, keep)), "the GELU' epilogue wrote to aux"


def _c_grouped(groups, outs, ldcs, Ms, N, K, epilogue=0, lda=None, n=None):
    from vqattack_amd import _hip
    k = len(groups)
    ptrs, longs = ctypes.c_void_p * k, ctypes.c_long * k
    return _hip.lib().vqa_gemm_bf16x6_grouped(
        ptrs(*[g[0].data_ptr() for g in groups]), longs(*(lda or [g[0].stride(0) for g in groups])),
        ptrs(*[g[1].data.data_ptr() for g in groups]), ptrs(*[g[2].data_ptr() if g[2] is not None else None for g in groups]),
        ptrs(*outs), longs(*ldcs), None, None, longs(*Ms), k if n is None else n, N, K, epilogue,
        _hip.stream_for(groups[0][0]))


@pytest.mark.gpu
def test_a_refused_call_leaves_every_output_at_its_sentinel():
    torch, dev = _torch()
    N, K, Ms = 256, 64, (200, 77, 130)
    groups = [_group(M, N, K, True, 0, 31 + i) for i, M in enumerate(Ms)]
    outs = [torch.full((M, N), SENTINEL, device=dev) for M in Ms]
    p = [o.data_ptr() for o in outs]
    a_off = torch.randn(Ms[2], K + 4, device=dev)[:, 1:K + 1]                        # one float off its 16-byte boundary
    codes = {
        "ldc": _c_grouped(groups, p, [N, N, N - 1], Ms, N, K),                       # the LAST group is the bad one
        "lda": _c_grouped(groups, p, [N] * 3, Ms, N, K, lda=[K, K, K + 2]),
        "rows": _c_grouped(groups, p, [N] * 3, (200, 77, -1), N, K),
        "c_align": _c_grouped(groups, [p[0], p[1], p[2] + 2], [N] * 3, Ms, N, K),
        "a_align": _c_grouped([groups[0], groups[1], (a_off, groups[2][1], None)], p, [N] * 3, Ms, N, K),
        "null": _c_grouped(groups, [p[0], p[1], None], [N] * 3, Ms, N, K),
        "grad_without_aux": _c_grouped(groups, p, [N] * 3, Ms, N, K, epilogue=2),
        "epilogue": _c_grouped(groups, p, [N] * 3, Ms, N, K, epilogue=3),
        "groups": _c_grouped(groups, p, [N] * 3, Ms, N, K, n=0),
        "k": _c_grouped(groups, p, [N] * 3, Ms, N, K + 16),
        "empty": _c_grouped(groups, p, [N] * 3, (0, 0, 0), N, K),
    }
    torch.cuda.synchronize()
    assert codes["ldc"] == codes["lda"] == codes["rows"] == codes["epilogue"] == codes["groups"] == codes["k"] == ERR_SHAPE, codes
    assert codes["c_align"] == codes["a_align"] == ERR_ALIGN and codes["null"] == codes["grad_without_aux"] == ERR_NULL and codes["empty"] == 0, codes
    assert all(bool((o == SENTINEL).all()) for o in outs), "a refused or empty call wrote to C"
    assert _c_grouped(groups, p, [N] * 3, Ms, N, K) == 0                             # and the same tables, intact, run
    torch.cuda.synchronize()
    from vqattack_amd import ops
    for (a, packed, bias), o in zip(groups, outs):
        assert torch.equal(o, ops.gemm_small(a, packed, bias, ksplit=1))


@pytest.mark.gpu
def test_fallback_for_an_n_or_a_group_count_the_launch_does_not_take():
    torch, dev = _torch()
    from vqattack_amd import ops
    for N, Ms in ((384, (129, 1, 77)), (256, (40, 129, 0, 7, 200))):
        groups = [_group(M, N, 64, i % 2 == 0, 0, 5 + i + N) for i, M in enumerate(Ms)]
        got = ops.gemm_grouped([g[0] for g in groups], [g[1] for g in groups], [g[2] for g in groups])
        assert len(got) == len(Ms)
        for (a, packed, bias), o in zip(groups, got):
            assert torch.equal(o, ops.gemm_small(a, packed, bias, ksplit=1))
        hs = [torch.randn(M, N, device=dev) for M in Ms]
        got = ops.gemm_grouped([g[0] for g in groups], [g[1] for g in groups], [g[2] for g in groups],
                               epilogue="gelu_grad", aux_list=hs)
        for (a, packed, bias), h, o in zip(groups, hs, got):
            assert tuple(o.shape) == (a.shape[0], N)
            if a.shape[0]:
                assert torch.equal(o, ops.gemm(a, packed, bias, tile="wide", epilogue="gelu_grad", aux=h))


def _two_expert_spec(d, heads, depth, seed):
    """A VLMo-shaped encoder whose layers all have a text and an image FFN (4 d wide), from random frozen weights."""
    torch, dev = _torch()
    from vqattack_amd.whitebox import _fused
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *shape, s=0.05: torch.randn(*shape, device=dev, generator=g) * s
    ln = lambda: (1.0 + rnd(d, s=0.1), rnd(d, s=0.1))
    mlp = lambda: (rnd(4 * d, d), rnd(4 * d), rnd(d, 4 * d), rnd(d))
    layers = [_fused.LayerSpec(ln(), rnd(3 * d, d), rnd(3 * d), rnd(d, d), rnd(d), 0.5 + rnd(d, s=0.1), [ln(), ln()],
                               [mlp(), mlp()], 0.5 + rnd(d, s=0.1), 1e-6) for _ in range(depth)]
    return _fused.EncoderSpec(layers, ln(), 1e-6, heads)


@pytest.mark.gpu
@pytest.mark.parametrize("epilogue", [None, "1"])
def test_encoder_with_every_expert_pair_grouped_has_the_bits_of_the_encoder_with_none(epilogue, monkeypatch):
    """3 samples x (5 text + 20 image tokens) at width 256 (4 heads of 64, FFN 1024), two experts in both layers: 15 text
    and 60 image rows.  With MIN_WORKGROUPS at 1 both settings run the bf16x6 kernels, whose tiles all give the same
    bits, so grouping must not change a bit of the feature maps, the final states or the input gradient."""
    torch, dev = _torch()
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    monkeypatch.delenv("VQA_GEMM", raising=False)
    monkeypatch.delenv("VQA_GEMM_TAIL", raising=False)
    if epilogue is None:
        monkeypatch.delenv("VQA_GEMM_EPILOGUE", raising=False)
    else:
        monkeypatch.setenv("VQA_GEMM_EPILOGUE", epilogue)
    monkeypatch.setattr(_fused, "MIN_WORKGROUPS", 1)
    spec = _two_expert_spec(256, 4, 2, 11)
    g = torch.Generator(device=dev).manual_seed(12)
    x0 = torch.randn(3, 25, 256, device=dev, generator=g)
    seen = []
    real = ops.gemm_grouped

    def counted(a_list, packed_list, *args, **kw):
        seen.append((tuple(a.shape[0] for a in a_list), kw.get("epilogue"), kw.get("aux_list") is not None))
        return real(a_list, packed_list, *args, **kw)
    monkeypatch.setattr(ops, "gemm_grouped", counted)
    results, grads = {}, None
    for switch in ("0", "1"):
        monkeypatch.setenv("VQA_GEMM_GROUPED", switch)
        del seen[:]
        x = x0.clone().requires_grad_(True)
        feats, states = _fused.encode(x, spec, None, 5)
        outs = list(feats[1:]) + [states]
        if grads is None:
            grads = [torch.randn(o.shape, device=dev, generator=g) for o in outs]
        torch.autograd.backward(outs, grads, inputs=[x])
        with torch.no_grad():
            feats_ng, states_ng = _fused.encode(x0, spec, None, 5)
        results[switch] = ([o.detach() for o in outs], x.grad, [f for f in feats_ng[1:]] + [states_ng], list(seen))
    assert results["0"][3] == [], "VQA_GEMM_GROUPED=0 reached the grouped entry point"
    calls = results["1"][3]
    assert len(calls) == 2 * 4 + 2 * 2, calls            # per layer: 4 with a gradient, 2 under no_grad
    assert all(c[0] == (60, 15) for c in calls), "the larger group does not come first"
    if epilogue == "1":
        assert [c[1:] for c in calls].count(("gelu", True)) == 2 and [c[1:] for c in calls].count(("gelu", False)) == 2
        assert [c[1] for c in calls].count("gelu_grad") == 2
    else:
        assert all(c[1] is None for c in calls)
    for o0, o1 in zip(results["0"][0] + results["0"][2], results["1"][0] + results["1"][2]):
        assert bool(torch.isfinite(o0).all()) and torch.equal(o0, o1)
    for with_grad, without in zip(results["1"][0], results["1"][2]):
        assert torch.equal(with_grad, without)
    assert float(results["0"][1].abs().max()) > 0 and torch.equal(results["0"][1], results["1"][1])


@pytest.mark.gpu
def test_a_captured_grouped_call_replays_on_fresh_inputs():
    """The groups travel in the kernel arguments: a captured launch keeps them, and reads its operands anew."""
    torch, dev = _torch()
    from vqattack_amd import ops
    N, K, Ms = 256, 96, (200, 0, 77)
    groups = [_group(M, N, K, i != 1, 0, 50 + i) for i, M in enumerate(Ms)]
    a_list, packed_list, bias_list = [g[0].contiguous() for g in groups], [g[1] for g in groups], [g[2] for g in groups]
    hs = [torch.randn(M, N, device=dev) for M in Ms]
    outs = [torch.zeros(M, N, device=dev) for M in Ms]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # load the library and warm the allocator outside the capture
        ops.gemm_grouped(a_list, packed_list, bias_list, out_list=outs, epilogue="gelu_grad", aux_list=hs)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gemm_grouped(a_list, packed_list, bias_list, out_list=outs, epilogue="gelu_grad", aux_list=hs)
    gen = torch.Generator(device=dev).manual_seed(99)
    for _round in range(2):
        for t in a_list + hs:
            t.copy_(torch.randn(t.shape, device=dev, generator=gen))
        for o in outs:
            o.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        replayed = [o.clone() for o in outs]
        eager = ops.gemm_grouped(a_list, packed_list, bias_list, epilogue="gelu_grad", aux_list=hs)
        assert all(torch.equal(r, e) for r, e in zip(replayed, eager))
        for r, a, packed, bias, h in zip(replayed, a_list, packed_list, bias_list, hs):
            if a.shape[0]:
                assert torch.equal(r, ops.gemm(a, packed, bias, tile="wide", epilogue="gelu_grad", aux=h))
