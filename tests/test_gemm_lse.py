"""vqa_gemm_bf16x6_lse / ops.gemm_lse: an LM head's per-row cross entropy from the GEMM's epilogue, without the logits.

CPU part: the declaration, the error codes and the loop budget of the two new kernel instantiations.  GPU part: the
target logit has the bits of ops.gemm, lse and row_loss stand against fp64 of those fp32 logits at 1e-4 * max(1, |value|)
(the parity vqa_ce_rows states for the hardware exponential), both tiles and two runs give the same bits, the mask is
n_valid and not the pad weights, and chosen values (overflow, -inf blocks, NaN rows, bad and ignored targets).
"""
import ctypes
import functools
import importlib.util
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LSE_KERNELS = ["gemm_bf16x6_epi_kernel<3>", "gemm_bf16x6_wide_epi_kernel<3>"]
IGNORE = -100
TOL = 1e-4


# ---------------------------------------------------------------------------------------------------------- CPU
def test_header_declares_the_entry_points_and_the_binding_matches():
    from vqattack_amd import _hip
    text = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    assert "model_vqa.py:149-203" in text and "xbert.py:1265-1271" in text, "the header says what the entry point replaces"
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+vqa_gemm_bf16x6_lse\s*\(([^)]*)\)\s*;", code)
    assert decl, "vqa_gemm_bf16x6_lse is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const float* A", "long lda", "const void* packed", "const float* bias", "long M", "int N", "int K",
                      "int n_valid", "const int64_t* targets", "long ignore_index", "float* ws", "float* row_loss",
                      "float* lse", "int* flag", "int tile", "vqa_stream_t stream"]
    ctype = {"long": ctypes.c_long, "int": ctypes.c_int}
    want = [ctypes.c_void_p if ("*" in p or p.startswith("vqa_stream_t")) else ctype[p.split()[0]] for p in params]
    assert _hip.SIGNATURES["vqa_gemm_bf16x6_lse"] == (ctypes.c_int, want)
    assert re.search(r"\blong\s+vqa_gemm_lse_ws_floats\s*\(\s*long M,\s*int N\s*\)\s*;", code)
    assert _hip.SIGNATURES["vqa_gemm_lse_ws_floats"] == (ctypes.c_long, [ctypes.c_long, ctypes.c_int])
    assert _hip.ABI_VERSION == 4


def test_error_codes_come_before_the_first_hip_call():
    from vqattack_amd import _hip
    lib = _hip.lib()
    OK, ERR_NULL, ERR_SHAPE, ERR_ALIGN = 0, -1, -2, -3
    buf = (ctypes.c_float * 256)()
    base = ctypes.cast(buf, ctypes.c_void_p).value
    base += -base % 16
    p = ctypes.c_void_p(base)

    def call(A=p, lda=32, packed=p, bias=None, M=4, N=128, K=32, n_valid=100, targets=p, ws=p, row_loss=p, lse=None,
             flag=None, tile=0):
        return lib.vqa_gemm_bf16x6_lse(A, lda, packed, bias, M, N, K, n_valid, targets, IGNORE, ws, row_loss, lse, flag,
                                       tile, None)
    for name in ("A", "packed", "targets", "ws", "row_loss"):
        assert call(**{name: None}) == ERR_NULL, name
    assert call(N=192) == ERR_SHAPE and call(N=64) == ERR_SHAPE and call(N=0) == ERR_SHAPE        # N % 128
    assert call(K=48, lda=48) == ERR_SHAPE and call(K=0) == ERR_SHAPE                              # K % 32
    assert call(n_valid=0) == ERR_SHAPE and call(n_valid=129) == ERR_SHAPE and call(n_valid=-3) == ERR_SHAPE
    assert call(lda=31) == ERR_SHAPE and call(lda=34) == ERR_SHAPE                                 # lda < K, lda % 4
    assert call(tile=2) == ERR_SHAPE and call(M=-1) == ERR_SHAPE
    assert call(ws=ctypes.c_void_p(base + 8)) == ERR_ALIGN and call(ws=ctypes.c_void_p(base + 4)) == ERR_ALIGN
    assert call(A=ctypes.c_void_p(base + 4)) == ERR_ALIGN
    assert call(targets=ctypes.c_void_p(base + 4)) == ERR_ALIGN
    assert call(bias=ctypes.c_void_p(base + 2)) == ERR_ALIGN
    assert call(M=0) == OK                                                                         # empty: no launch
    assert lib.vqa_gemm_lse_ws_floats(300, 768) == (768 // 64 * 2 + 1) * 300
    assert lib.vqa_gemm_lse_ws_floats(300, 100) == 0 and lib.vqa_gemm_lse_ws_floats(0, 128) == 0


@functools.lru_cache(maxsize=None)
def _gemm_kernels():
    """name -> (meta, loop body) of every kernel of gemm.hip, from the compiler's assembly (tools/isa_loop_mix.py)."""
    spec = importlib.util.spec_from_file_location("isa_loop_mix", os.path.join(ROOT, "tools", "isa_loop_mix.py"))
    mix = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mix)
    return {name.split("::")[-1]: (meta, body) for name, meta, body in mix.kernels(mix.assembly("gemm.hip"))}


def _loop_ops(body):
    return [l.split()[0] for l in body.split("\n") if l.startswith("\t") and l.split() and not l.strip().startswith(";")]


@pytest.mark.parametrize("name", LSE_KERNELS)
def test_lse_kernels_keep_the_loop_budget(name):
    """No scratch, two waves per SIMD, 96 MFMAs per k-step -- the budget of the kernels they copy the loop of."""
    meta, body = _gemm_kernels()[name]
    mfma = sum(o.startswith("v_mfma") for o in _loop_ops(body))
    print(name, meta, "mfma", mfma)
    assert meta["ScratchSize"] == "0" and meta["Occupancy"] == "2", meta
    assert mfma == 96


def test_wide_lse_kernel_spaces_its_global_loads_among_the_mfmas():
    """The conditions of test_gemm_wide.py::test_wide_loop_spaces_its_global_loads_among_the_mfmas."""
    _meta, body = _gemm_kernels()[LSE_KERNELS[1]]
    seq = "".join("M" if o.startswith("v_mfma") else "G" for o in _loop_ops(body) if o.startswith(("v_mfma", "global_load")))
    assert seq.count("G") == 8 and seq.count("M") == 96
    assert seq.index("M") <= 2 and "GGG" not in seq and seq[:seq.rindex("G")].count("M") <= 48


# ---------------------------------------------------------------------------------------------------------- GPU
def _torch():
    import torch
    return torch, torch.device("cuda")


def _padded_n(V):
    return -(-V // 256) * 256


def _targets(torch, gen, M, V, dev):
    """Random targets, the forced columns at block and tile edges (those below V), and some ignore_index rows."""
    t = torch.randint(0, V, (M,), device=dev, generator=gen)
    forced = [c for c in (0, V - 1, 63, 64, 127, 128, 255, 256) if c < V]
    rows = torch.randperm(M, device=dev, generator=gen)[:len(forced)]
    t[rows] = torch.tensor(forced[:len(rows)], device=dev)
    if M > 4:
        t[torch.randperm(M, device=dev, generator=gen)[:max(1, M // 10)]] = IGNORE
        if M >= len(forced) + 2:                 # the forced columns survive where the rows allow
            t[rows] = torch.tensor(forced[:len(rows)], device=dev)
    return t


def _reference(torch, logits, targets, V):
    """(lse, row_loss) in fp64 of fp32 logits over [:V]."""
    x = logits[:, :V].double()
    lse = torch.logsumexp(x, dim=1)
    live = targets != IGNORE
    tl = x.gather(1, targets.clamp(min=0).unsqueeze(1)).squeeze(1)
    return lse, torch.where(live, lse - tl, torch.zeros_like(lse))


def _rel(got, want):
    return float(((got.double() - want).abs() / want.abs().clamp(min=1.0)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 96, 768])
@pytest.mark.parametrize("V", [100, 256, 257, 700])
def test_grid_against_the_unfused_gemm_and_fp64(V, K):
    """M x lda x tile x bias at one (V, K): tgt bitwise ops.gemm's, lse / row_loss at 1e-4 * max(1, |value|) of fp64,
    the two tiles bitwise equal.  Prints the maxima and, beside them, the error of fp32 logits + F.cross_entropy."""
    torch, dev = _torch()
    import torch.nn.functional as F
    from vqattack_amd import ops
    gen = torch.Generator(device=dev).manual_seed(1000 * V + K)
    N = _padded_n(V)
    w = torch.randn(V, K, device=dev, generator=gen) * (3.0 / math.sqrt(K))
    packed = ops.gemm_pack_vocab(w)
    assert (packed.N, packed.K, packed.n_valid) == (N, K, V)
    bias_v = torch.randn(V, device=dev, generator=gen)
    bias_n = torch.cat([bias_v, bias_v.new_zeros(N - V)])
    worst = {"lse": 0.0, "row_loss": 0.0, "two_step": 0.0}
    for M in (1, 127, 129, 300):
        targets = _targets(torch, gen, M, V, dev)
        live = targets != IGNORE
        for lda in (K, K + 4):
            a = torch.randn(M, lda, device=dev, generator=gen)[:, :K]
            for bias in (None, bias_v):
                logits = ops.gemm(a, packed, None if bias is None else bias_n, tile="large")
                want_lse, want_loss = _reference(torch, logits, targets, V)
                want_tgt = logits.gather(1, targets.clamp(min=0).unsqueeze(1)).squeeze(1)
                two_step = F.cross_entropy(logits[:, :V], targets, ignore_index=IGNORE, reduction="none")
                worst["two_step"] = max(worst["two_step"], _rel(two_step, want_loss))
                got = {}
                for tile in ("large", "wide"):
                    loss, lse, tgt = ops.gemm_lse(a, packed, bias, targets, ignore_index=IGNORE, tile=tile, want_lse=True,
                                                  want_target_logit=True)
                    got[tile] = (loss, lse)
                    assert torch.equal(tgt[live], want_tgt[live]), (M, lda, tile, bias is None)
                    worst["lse"] = max(worst["lse"], _rel(lse, want_lse))
                    worst["row_loss"] = max(worst["row_loss"], _rel(loss, want_loss))
                    assert bool((loss[~live] == 0).all())
                assert torch.equal(got["large"][0], got["wide"][0]) and torch.equal(got["large"][1], got["wide"][1])
    print("V={} K={} max rel err: lse {:.3e} row_loss {:.3e} | fp32 logits + F.cross_entropy {:.3e}".format(
        V, K, worst["lse"], worst["row_loss"], worst["two_step"]))
    assert worst["lse"] <= TOL and worst["row_loss"] <= TOL, worst


@pytest.mark.gpu
def test_two_runs_give_equal_bits_and_the_default_tile_is_one_of_them():
    torch, dev = _torch()
    from vqattack_amd import ops
    gen = torch.Generator(device=dev).manual_seed(5)
    M, V, K = 300, 700, 96
    a = torch.randn(M, K, device=dev, generator=gen)
    packed = ops.gemm_pack_vocab(torch.randn(V, K, device=dev, generator=gen))
    bias = torch.randn(V, device=dev, generator=gen)
    targets = _targets(torch, gen, M, V, dev)
    first = ops.gemm_lse(a, packed, bias, targets, tile="wide", want_lse=True)
    for tile in ("wide", "large", None):
        again = ops.gemm_lse(a, packed, bias, targets, tile=tile, want_lse=True)
        assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert torch.equal(ops.gemm_lse(a, packed, bias, targets), first[0])          # without lse: a tensor, same bits


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["large", "wide"])
def test_the_mask_is_n_valid_not_the_pad_weights(tile):
    """Non-zero pad rows in the packed weight and +50 on the pad columns of the bias: the bits of the zero-padded one."""
    torch, dev = _torch()
    from vqattack_amd import ops
    gen = torch.Generator(device=dev).manual_seed(6)
    M, V, K = 129, 257, 96
    N = _padded_n(V)
    a = torch.randn(M, K, device=dev, generator=gen)
    w = torch.randn(V, K, device=dev, generator=gen)
    bias = torch.randn(V, device=dev, generator=gen)
    targets = _targets(torch, gen, M, V, dev)
    clean = ops.gemm_lse(a, ops.gemm_pack_vocab(w), bias, targets, tile=tile, want_lse=True)
    dirty_w = torch.cat([w, 5.0 * torch.randn(N - V, K, device=dev, generator=gen)])
    dirty_p = ops.gemm_pack(dirty_w, trans=True)
    dirty = ops.gemm_lse(a, ops.PackedWeight(dirty_p.data, K, N, V), torch.cat([bias, bias.new_full((N - V,), 50.0)]),
                         targets, tile=tile, want_lse=True)
    assert torch.equal(clean[0], dirty[0]) and torch.equal(clean[1], dirty[1])


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["large", "wide"])
def test_chosen_values(tile):
    torch, dev = _torch()
    from vqattack_amd import ops
    gen = torch.Generator(device=dev).manual_seed(7)
    M, V, K = 129, 700, 96
    N = _padded_n(V)                                                            # 768: block 11 = columns 704 .. 767 is pad only
    inf = float("inf")
    a = torch.randn(M, K, device=dev, generator=gen)
    w = torch.randn(V, K, device=dev, generator=gen) * (1.0 / math.sqrt(K))
    packed = ops.gemm_pack_vocab(w)
    targets = torch.randint(0, V, (M,), device=dev, generator=gen)

    def run(bias, a_=a, targets_=targets, flag=None):
        return ops.gemm_lse(a_, packed, bias, targets_, tile=tile, want_lse=True, flag=flag)

    def ref(bias, a_=a, targets_=targets):
        return _reference(torch, ops.gemm(a_, packed, bias, tile="large"), targets_, V)

    def close(got, want):
        assert bool(torch.isfinite(got[0]).all()) and bool(torch.isfinite(got[1]).all())
        assert _rel(got[1], want[0]) <= TOL and _rel(got[0], want[1]) <= TOL

    # a column with bias +200 does not overflow
    bias = torch.zeros(N, device=dev)
    bias[77] = 200.0
    got = run(bias)
    close(got, ref(bias))
    assert bool((got[1] > 150).all())
    # a row of equal logits: lse = x + log V  (zero activations: every logit is the bias)
    bias = torch.full((N,), 3.25, device=dev)
    got = run(bias, a_=torch.zeros(M, K, device=dev))
    assert _rel(got[1], torch.full((M,), 3.25 + math.log(V), dtype=torch.float64, device=dev)) <= TOL
    assert _rel(got[0], torch.full((M,), math.log(V), dtype=torch.float64, device=dev)) <= TOL
    # -inf bias on scattered valid columns contributes 0; on one whole 64-column block and on all columns of the
    # pad-only block: finite, no NaN
    bias = torch.randn(N, device=dev, generator=gen)
    bias[torch.tensor([0, 5, 63, 64, 300, 699], device=dev)] = -inf
    bias[128:192] = -inf
    bias[704:] = -inf
    safe = torch.where(torch.isinf(bias[:V][targets]), (targets + 1) % V, targets)      # a target at a live column
    safe = torch.where(torch.isinf(bias[:V][safe]), torch.full_like(safe, 200), safe)
    assert not bool(torch.isinf(bias[:V][safe]).any())
    close(run(bias, targets_=safe), ref(bias, targets_=safe))
    # every valid column -inf: lse = -inf like torch.logsumexp, and still no NaN in lse
    got = run(torch.full((N,), -inf, device=dev))
    assert bool((got[1] == -inf).all())
    # a NaN in one row of a: that row NaN, its neighbours untouched
    bias = torch.randn(N, device=dev, generator=gen)
    base = run(bias)
    a_nan = a.clone()
    a_nan[64, 3] = float("nan")
    got = run(bias, a_=a_nan)
    others = torch.arange(M, device=dev) != 64
    assert bool(torch.isnan(got[0][64])) and bool(torch.isnan(got[1][64]))
    assert torch.equal(got[0][others], base[0][others]) and torch.equal(got[1][others], base[1][others])
    # an out-of-range target: NaN and the flag bit; an ignore_index row: exactly 0; the lse of both rows is untouched
    bad = targets.clone()
    bad[3], bad[70], bad[9], bad[100] = V, -1, IGNORE, N + 5
    flag = ops.new_flag(dev)
    got = run(bias, targets_=bad, flag=flag)
    assert int(flag.item()) == 2                                                # VQA_FLAG_BAD_LABEL
    assert bool(torch.isnan(got[0][torch.tensor([3, 70, 100], device=dev)]).all())
    assert float(got[0][9]) == 0.0 and math.copysign(1.0, float(got[0][9])) == 1.0
    keep = torch.ones(M, dtype=torch.bool, device=dev)
    keep[torch.tensor([3, 70, 9, 100], device=dev)] = False
    assert torch.equal(got[0][keep], base[0][keep]) and torch.equal(got[1], base[1])
    clean_flag = ops.new_flag(dev)
    run(bias, flag=clean_flag)
    assert int(clean_flag.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["large", "wide"])
def test_graph_replay_equals_eager_launch(tile):
    torch, dev = _torch()
    from vqattack_amd import ops
    gen = torch.Generator(device=dev).manual_seed(8)
    M, V, K = 300, 700, 96
    a = torch.randn(M, K, device=dev, generator=gen)
    packed = ops.gemm_pack_vocab(torch.randn(V, K, device=dev, generator=gen))
    bias = torch.randn(V, device=dev, generator=gen)
    targets = _targets(torch, gen, M, V, dev)
    eager = ops.gemm_lse(a, packed, bias, targets, tile=tile, want_lse=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = ops.gemm_lse(a, packed, bias, targets, tile=tile, want_lse=True)
    for _ in range(2):
        for t in static:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(static[0], eager[0]) and torch.equal(static[1], eager[1])
