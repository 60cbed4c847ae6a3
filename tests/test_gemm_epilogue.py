"""GELU and its derivative in the epilogue of the bf16x6 GEMM (``csrc/gemm.hip``: ``gemm_bf16x6_epi_kernel<EPI>`` /
``gemm_bf16x6_wide_epi_kernel<EPI>`` behind ``vqa_gemm_bf16x6_epi``, ``ops.gemm(..., epilogue=, aux=)``) and its dispatch
in ``whitebox/_fused.py`` (``EPILOGUE_POLICY``, ``VQA_GEMM_EPILOGUE``, ``_linear_gelu`` / ``_linear_grad_gelu``).

The fused call is pinned BITWISE to the unfused pair (GEMM, then ``vqa_gelu_fwd`` / ``vqa_gelu_bwd``), which the existing
GEMM and GELU tests hold against fp64: no tolerance appears here.
GPU: partial tiles of both tile heights, one and several column tiles, padded strides of every operand with sentinels
around ``out`` and ``aux``, chosen values around erf's branch point and at the ends of the range, the C ABI's return codes,
whole encoders with the switch on against off, graph replay.
CPU: the wrapper's checks, the dispatch with every GEMM stubbed, header against binding, and the new kernels' loop budget
and load placement read from the compiler's assembly.
"""
import ctypes
import functools
import importlib.util
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPI_KERNELS = ["gemm_bf16x6_epi_kernel<1>", "gemm_bf16x6_epi_kernel<2>",
               "gemm_bf16x6_wide_epi_kernel<1>", "gemm_bf16x6_wide_epi_kernel<2>"]


def _torch():
    import torch
    return torch, torch.device("cuda", 0)


# ---------------------------------------------------------------------------------------------------------- CPU
class _Packed:
    def __init__(self, K, N):
        self.K, self.N, self.data = K, N, None


def test_wrapper_refuses_bad_epilogue_arguments_before_any_launch():
    import torch
    from vqattack_amd import ops
    a, pk = torch.empty(5, 32, device="meta"), _Packed(32, 256)
    h = torch.empty(5, 256, device="meta")
    with pytest.raises(ValueError, match="epilogue"):
        ops.gemm(a, pk, epilogue="relu")
    with pytest.raises(ValueError, match="aux"):
        ops.gemm(a, pk, epilogue="gelu_grad")
    for bad in (torch.empty(4, 256, device="meta"), torch.empty(5, 128, device="meta"), torch.empty(5 * 256, device="meta"),
                torch.empty(256, 5, device="meta").t()):
        with pytest.raises(ValueError, match="aux"):
            ops.gemm(a, pk, epilogue="gelu", aux=bad)
        with pytest.raises(ValueError, match="aux"):
            ops.gemm(a, pk, epilogue="gelu_grad", aux=bad)
    with pytest.raises(ValueError, match="aux"):
        ops.gemm(a, pk, out=h, epilogue="gelu", aux=h)
    with pytest.raises(ValueError, match="aux"):
        ops.gemm(a, pk, aux=h)                                   # aux without an epilogue


def _picked(monkeypatch, mode, switch, policy, rows):
    """What ``_linear_gelu`` / ``_linear_grad_gelu`` run for an FFN of width 768 -> 3072 at each row count, with every
    GEMM and GELU stubbed below ``ops.gemm``'s checks: per row count (forward calls, backward calls)."""
    import torch
    from vqattack_amd.whitebox import _fused
    for name, val in (("VQA_GEMM", mode), ("VQA_GEMM_EPILOGUE", switch)):
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)
    monkeypatch.setattr(_fused, "EPILOGUE_POLICY", policy)
    picked = []
    monkeypatch.setattr(_fused.ops, "_gemm_tiled", lambda a, pk, bias, out, tile: picked.append(tile))
    monkeypatch.setattr(_fused.ops, "_gemm_epilogue",
                        lambda a, pk, bias, out, tile, epilogue, aux: picked.append((epilogue, tile, aux is not None)))
    monkeypatch.setattr(_fused.ops, "gemm_small", lambda a, pk, bias=None, out=None, ksplit=1: picked.append("small"))
    monkeypatch.setattr(_fused.ops, "gelu_fwd", lambda h, out=None: picked.append("gelu_fwd"))
    monkeypatch.setattr(_fused.ops, "gelu_bwd", lambda h, da, out=None: picked.append("gelu_bwd"))
    monkeypatch.setattr(_fused.torch, "addmm", lambda *a, **k: picked.append("library"))
    monkeypatch.setattr(_fused.torch, "mm", lambda *a, **k: picked.append("library"))
    table = {}
    for M, D, F in rows:
        w1, w2 = torch.empty(F, D, device="meta"), torch.empty(D, F, device="meta")
        for save in (True, False):
            del picked[:]
            h, _act = _fused._linear_gelu(torch.empty(M, D, device="meta"), w1, torch.empty(F, device="meta"),
                                          (_Packed(D, F), _Packed(F, D)), save)
            fwd = list(picked)
            if fwd[0][0] == "gelu":
                assert fwd[0][2] == save and (h is not None) == save, "h is allocated and written only when saved"
            table[(M, D, F, save)] = fwd
        del picked[:]
        _fused._linear_grad_gelu(torch.empty(M, D, device="meta"), w2, (_Packed(F, D), _Packed(D, F)),
                                 torch.empty(M, F, device="meta"))
        table[(M, D, F)] = (table[(M, D, F, True)], list(picked))
    return table


# the benchmark's image-expert FFN, another width, and a row count whose grid is below MIN_WORKGROUPS
_FFNS = [(37824, 768, 3072), (37824, 1024, 4096), (591, 768, 3072)]
_ROWS = {(3072, 768): (30000, 40000)}
_POLICY = {"gelu": _ROWS, "gelu_grad": _ROWS}
_NONE = {"gelu": {}, "gelu_grad": {}}
_FUSED = ([("gelu", "large", True)], [("gelu_grad", "large", True)])
_TWO_STEP = (["large", "gelu_fwd"], ["large", "gelu_bwd"])
_LIBRARY = (["library", "gelu_fwd"], ["library", "gelu_bwd"])


def test_policy_fuses_a_listed_shape_and_no_other(monkeypatch):
    got = _picked(monkeypatch, "large", None, _POLICY, _FFNS)
    assert got[(37824, 768, 3072)] == _FUSED
    assert got[(37824, 768, 3072, False)] == [("gelu", "large", False)]       # no_grad: h is not stored
    assert got[(37824, 1024, 4096)] == _TWO_STEP                              # unlisted (N, K)
    assert got[(591, 768, 3072)] == _LIBRARY                                  # below the grid threshold
    short = {(3072, 768): (30000, 37000)}
    got = _picked(monkeypatch, "large", None, {"gelu": short, "gelu_grad": short}, _FFNS)
    assert got[(37824, 768, 3072)] == _TWO_STEP                               # rows outside the recorded range
    # the two epilogues are listed separately
    got = _picked(monkeypatch, "large", None, {"gelu": {}, "gelu_grad": _ROWS}, _FFNS)
    assert got[(37824, 768, 3072)] == (_TWO_STEP[0], _FUSED[1])
    got = _picked(monkeypatch, "large", None, {"gelu": _ROWS, "gelu_grad": {}}, _FFNS)
    assert got[(37824, 768, 3072)] == (_FUSED[0], _TWO_STEP[1])
    for key, val in _picked(monkeypatch, "library", None, _POLICY, _FFNS).items():
        assert len(key) == 4 or val == _LIBRARY, key
    # the tile is ops.gemm's choice as for every other GEMM
    wide = _picked(monkeypatch, "wide", None, _POLICY, _FFNS)
    assert wide[(37824, 768, 3072)] == ([("gelu", "wide", True)], [("gelu_grad", "wide", True)])
    # VQA_GEMM=small runs the 256 x 128 kernel from MIN_WORKGROUPS up (fused if listed) and the small kernel below
    small = _picked(monkeypatch, "small", None, _POLICY, _FFNS)
    assert small[(37824, 768, 3072)] == _FUSED
    assert small[(591, 768, 3072)] == (["small", "gelu_fwd"], ["small", "gelu_bwd"])
    for key, val in _picked(monkeypatch, "large", None, _NONE, _FFNS).items():
        assert len(key) == 4 or val == (_LIBRARY if key[0] == 591 else _TWO_STEP), key


def test_switch_overrides_the_policy(monkeypatch):
    for key, val in _picked(monkeypatch, "large", "0", _POLICY, _FFNS).items():
        assert len(key) == 4 or val == (_LIBRARY if key[0] == 591 else _TWO_STEP), key
    for key, val in _picked(monkeypatch, "large", "1", _NONE, _FFNS).items():
        assert len(key) == 4 or val == (_LIBRARY if key[0] == 591 else _FUSED), key
    for key, val in _picked(monkeypatch, "library", "1", _POLICY, _FFNS).items():
        assert len(key) == 4 or val == _LIBRARY, key


def test_shipped_policy_lists_only_shapes_the_fused_kernels_cover(monkeypatch):
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    monkeypatch.delenv("VQA_GEMM", raising=False)
    monkeypatch.delenv("VQA_GEMM_EPILOGUE", raising=False)
    assert sorted(_fused.EPILOGUE_POLICY) == ["gelu", "gelu_grad"]
    for epi, table in _fused.EPILOGUE_POLICY.items():
        for (n, k), (lo, hi) in table.items():
            assert n % 128 == 0 and k % 32 == 0 and 1 <= lo <= hi, (epi, n, k, lo, hi)
            assert ops.gemm_workgroups(lo, n) >= _fused.MIN_WORKGROUPS
            assert _fused.gelu_epilogue(lo, n, k, epi) and _fused.gelu_epilogue(hi, n, k, epi)
            assert not _fused.gelu_epilogue(hi + 1, n, k, epi)
    assert not _fused.gelu_epilogue(37824, 640, 768) and not _fused.gelu_epilogue(37824, 640, 768, "gelu_grad")


def test_header_declares_the_entry_point_and_the_binding_matches():
    from vqattack_amd import _hip, ops
    text = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+vqa_gemm_bf16x6_epi\s*\(([^)]*)\)\s*;", code)
    assert decl, "vqa_gemm_bf16x6_epi is not declared"
    params = [" ".join(p.split()) for p in decl.group(1).split(",")]
    assert params == ["const float* A", "long lda", "const void* packed", "const float* bias", "float* C", "long ldc",
                      "long M", "int N", "int K", "int tile", "int epilogue", "float* aux", "long ldaux",
                      "vqa_stream_t stream"]
    ctype = {"long": ctypes.c_long, "int": ctypes.c_int}
    want = [ctypes.c_void_p if ("*" in p or p.startswith("vqa_stream_t")) else ctype[p.split()[0]] for p in params]
    assert _hip.SIGNATURES["vqa_gemm_bf16x6_epi"] == (ctypes.c_int, want)
    consts = dict(re.findall(r"#define\s+(VQA_GEMM_EPI_[A-Z_]+)\s+(\d+)", code))
    assert consts == {"VQA_GEMM_EPI_NONE": "0", "VQA_GEMM_EPI_GELU": "1", "VQA_GEMM_EPI_GELU_GRAD": "2"}
    assert ops.GEMM_EPILOGUES == {"gelu": 1, "gelu_grad": 2}
    assert _hip.ABI_VERSION == 4


@functools.lru_cache(maxsize=None)
def _gemm_kernels():
    """name -> (meta, loop body) of every kernel of gemm.hip, from the compiler's assembly (tools/isa_loop_mix.py)."""
    spec = importlib.util.spec_from_file_location("isa_loop_mix", os.path.join(ROOT, "tools", "isa_loop_mix.py"))
    mix = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mix)
    return {name.split("::")[-1]: (meta, body) for name, meta, body in mix.kernels(mix.assembly("gemm.hip"))}


def _loop_ops(body):
    return [l.split()[0] for l in body.split("\n") if l.startswith("\t") and l.split() and not l.strip().startswith(";")]


@pytest.mark.parametrize("name", EPI_KERNELS)
def test_fused_kernels_keep_the_loop_budget(name):
    """No scratch, two waves per SIMD, 96 MFMAs per k-step -- the budget of the kernels they copy the loop of."""
    meta, body = _gemm_kernels()[name]
    mfma = sum(o.startswith("v_mfma") for o in _loop_ops(body))
    print(name, meta, "mfma", mfma)
    assert meta["ScratchSize"] == "0" and meta["Occupancy"] == "2", meta
    assert mfma == 96


@pytest.mark.parametrize("name", EPI_KERNELS[2:])
def test_wide_fused_kernels_space_their_global_loads_among_the_mfmas(name):
    """The conditions of test_gemm_wide.py::test_wide_loop_spaces_its_global_loads_among_the_mfmas."""
    _meta, body = _gemm_kernels()[name]
    seq = "".join("M" if o.startswith("v_mfma") else "G" for o in _loop_ops(body) if o.startswith(("v_mfma", "global_load")))
    print(seq)
    assert seq.count("G") == 8 and seq.count("M") == 96
    assert seq.index("M") <= 2, "more than two global loads ahead of the first MFMA"
    assert "GGG" not in seq, "three global loads with no MFMA between them"
    assert seq[:seq.rindex("G")].count("M") <= 48, "a load of the next step issued in the second half of the step"


def test_unfused_kernels_keep_their_names():
    kernels = _gemm_kernels()
    assert "gemm_bf16x6_kernel" in kernels and "gemm_bf16x6_wide_kernel" in kernels


# ---------------------------------------------------------------------------------------------------------- GPU
SENTINEL = 7.0


def _padded(M, N, fill=SENTINEL):
    """An (M, N) view with row stride N + 4 inside a buffer of M + 1 rows filled with the sentinel."""
    torch, dev = _torch()
    buf = torch.full((M + 1, N + 4), fill, device=dev)
    return buf, buf[:M, :N]


def _only_view_written(buf, M, N):
    return bool((buf[:, N:] == SENTINEL).all()) and bool((buf[M] == SENTINEL).all())


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 96])
@pytest.mark.parametrize("N", [128, 256, 512])
@pytest.mark.parametrize("M", [1, 127, 129, 300])
@pytest.mark.parametrize("tile", ["large", "wide"])
def test_fused_epilogues_have_the_bits_of_the_unfused_pair(tile, M, N, K):
    torch, dev = _torch()
    from vqattack_amd import ops
    g = torch.Generator(device=dev).manual_seed(1000 * M + N + K)
    for has_bias in (True, False):
        a = torch.randn(M, K + 4, device=dev, generator=g)[:, :K]
        w = torch.randn(N, K, device=dev, generator=g) * (2.0 / math.sqrt(K))
        bias = torch.randn(N, device=dev, generator=g) if has_bias else None
        assert a.stride(0) == K + 4
        pk = ops.gemm_pack(w, trans=True)
        # forward: h = a @ w.t() (+ bias) has a spread of about 2: both branches of erf2 and its tail
        h_want = ops.gemm(a, pk, bias, tile=tile)
        act_want = ops.gelu_fwd(h_want)
        obuf, out = _padded(M, N)
        xbuf, aux = _padded(M, N)
        got = ops.gemm(a, pk, bias, out=out, tile=tile, epilogue="gelu", aux=aux)
        assert got is out
        assert torch.equal(aux, h_want), ("h", has_bias)
        assert torch.equal(out, act_want), ("gelu", has_bias)
        assert _only_view_written(obuf, M, N) and _only_view_written(xbuf, M, N), "a pad column or a row past M was written"
        assert torch.equal(ops.gemm(a, pk, bias, tile=tile, epilogue="gelu"), act_want), "without aux"
        obuf2, out2 = _padded(M, N)
        xbuf2, aux2 = _padded(M, N)
        ops.gemm(a, pk, bias, out=out2, tile=tile, epilogue="gelu", aux=aux2)
        assert torch.equal(obuf2, obuf) and torch.equal(xbuf2, xbuf), "not bitwise reproducible"
        # backward: a plays the gradient, h is random with the spread of the forward's
        hbuf, h = _padded(M, N)
        h.copy_(torch.randn(M, N, device=dev, generator=g) * 2.0)
        h_before = hbuf.clone()
        dh_want = ops.gelu_bwd(h.contiguous(), ops.gemm(a, pk, bias, tile=tile))
        dbuf, dh = _padded(M, N)
        ops.gemm(a, pk, bias, out=dh, tile=tile, epilogue="gelu_grad", aux=h)
        assert torch.equal(dh, dh_want), ("gelu_grad", has_bias)
        assert _only_view_written(dbuf, M, N), "a pad column or a row past M was written"
        assert torch.equal(hbuf, h_before), "aux is read only"
        dbuf2, dh2 = _padded(M, N)
        ops.gemm(a, pk, bias, out=dh2, tile=tile, epilogue="gelu_grad", aux=h)
        assert torch.equal(dbuf2, dbuf), "not bitwise reproducible"


def _chosen_values():
    torch, dev = _torch()
    branch = torch.tensor(1.3120374, dtype=torch.float32)           # 0.927734375 * sqrt(2): erf2's branch point in h
    near = [branch, torch.nextafter(branch, torch.tensor(2.0)), torch.nextafter(branch, torch.tensor(0.0))]
    vals = [0.0, -0.0] + [s * float(v) for v in near for s in (1.0, -1.0)]
    vals += [s * v for v in (6.0, 12.0, 40.0, float("inf")) for s in (1.0, -1.0)] + [float("nan")]
    return torch.tensor(vals, dtype=torch.float32, device=dev)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["large", "wide"])
def test_chosen_values_through_both_epilogues(tile):
    """+-0, erf2's branch point and its fp32 neighbours, the tail, +-inf and NaN: compared as bit patterns."""
    torch, dev = _torch()
    from vqattack_amd import ops
    vals = _chosen_values()
    M, N, K = vals.numel(), 256, 32
    i32 = torch.int32
    # forward: row m of a is vals[m] at k = 0, every column of the operand has its single 1.0 there: h[m, :] = vals[m]
    a = torch.zeros(M, K, device=dev)
    a[:, 0] = vals
    w = torch.zeros(N, K, device=dev)
    w[:, 0] = 1.0
    pk = ops.gemm_pack(w, trans=True)
    h_want = ops.gemm(a, pk, tile=tile)
    finite = torch.isfinite(vals)
    assert torch.equal(h_want[finite], vals[finite][:, None].expand(-1, N)), "the chosen values do not reach the epilogue"
    aux = torch.empty(M, N, device=dev)
    got = ops.gemm(a, pk, tile=tile, epilogue="gelu", aux=aux)
    assert torch.equal(aux.view(i32), h_want.view(i32))
    assert torch.equal(got.view(i32), ops.gelu_fwd(h_want).view(i32))
    # the non-finite ones reach h through the bias (inf times the operand's zero correction planes is NaN): column n
    # carries vals[n % len(vals)]
    bias = vals.repeat(N // M + 1)[:N].contiguous()
    a0 = torch.zeros(M, K, device=dev)
    hb_want = ops.gemm(a0, pk, bias, tile=tile)
    assert torch.equal(torch.isnan(hb_want[0]), torch.isnan(bias)) and \
        torch.equal(torch.nan_to_num(hb_want[0]), torch.nan_to_num(bias)), "the chosen values do not reach the epilogue"
    got = ops.gemm(a0, pk, bias, tile=tile, epilogue="gelu", aux=aux)
    assert torch.equal(aux.view(i32), hb_want.view(i32))
    assert torch.equal(got.view(i32), ops.gelu_fwd(hb_want).view(i32))
    # backward: the values are the pre-activation itself
    h = vals[:, None].expand(-1, N).contiguous()
    gen = torch.Generator(device=dev).manual_seed(3)
    grad = torch.randn(M, K, device=dev, generator=gen)
    wr = torch.randn(N, K, device=dev, generator=gen) * (2.0 / math.sqrt(K))
    pkr = ops.gemm_pack(wr, trans=True)
    want = ops.gelu_bwd(h, ops.gemm(grad, pkr, tile=tile))
    got = ops.gemm(grad, pkr, tile=tile, epilogue="gelu_grad", aux=h)
    assert torch.equal(got.view(i32), want.view(i32))


@pytest.mark.gpu
def test_c_abi_return_codes():
    torch, dev = _torch()
    from vqattack_amd import _hip, ops
    OK, ERR_NULL, ERR_SHAPE, ERR_ALIGN = 0, -1, -2, -3
    M, N, K = 4, 128, 32
    a, c, aux = torch.zeros(M, K, device=dev), torch.zeros(M, N, device=dev), torch.zeros(M + 1, N, device=dev)
    pk = ops.gemm_pack(torch.zeros(N, K, device=dev), trans=True)
    lib, st = _hip.lib(), _hip.stream_for(a)
    p = _hip.ptr

    def call(epilogue, aux_ptr, ldaux, rows=M, tile=0):
        return lib.vqa_gemm_bf16x6_epi(p(a), K, p(pk.data), None, p(c), N, rows, N, K, tile, epilogue, aux_ptr, ldaux, st)
    assert call(3, p(aux), N) == ERR_SHAPE and call(-1, p(aux), N) == ERR_SHAPE      # unknown epilogue
    assert call(2, None, N) == ERR_NULL                                              # GELU_GRAD reads aux
    assert call(1, p(aux), N - 1) == ERR_SHAPE and call(2, p(aux), N - 1) == ERR_SHAPE
    assert call(1, ctypes.c_void_p(aux.data_ptr() + 2), N) == ERR_ALIGN
    assert call(1, p(aux), N, rows=0) == OK and call(2, p(aux), N, rows=0) == OK and call(1, None, 0, rows=0) == OK
    assert call(1, p(aux), N, tile=2) == ERR_SHAPE                                   # the checks of vqa_gemm_bf16x6_tile
    assert call(0, None, 0, tile=2) == ERR_SHAPE
    assert call(1, p(c), N) == ERR_SHAPE                                             # aux == C
    torch.cuda.synchronize()
    assert bool((c == 0).all()) and bool((aux == 0).all()), "a refused call wrote"
    assert call(0, None, 0) == OK and call(1, None, 0) == OK and call(1, p(aux), N) == OK and call(2, p(aux), N) == OK
    torch.cuda.synchronize()


def _encoder_case(name, monkeypatch):
    """(run(grad) -> (outputs, input gradients)) of a smallest model with 64-wide heads: width 128, 2 heads, FFN 512,
    batch 2, 8 text tokens, a 4 x 4 patch grid."""
    torch, dev = _torch()
    gen = torch.Generator(device=dev).manual_seed(11)
    image = torch.empty(2, 3, 32, 32, device=dev).uniform_(-1, 1, generator=gen)
    ids = torch.tensor([[101, 5, 6, 7, 102, 0, 0, 0], [101, 8, 9, 3, 4, 2, 7, 102]], device=dev)
    masks = (ids != 0).long()
    if name == "vlmo":
        from vqattack_amd.whitebox.vlmo import FrozenVlmo, VlmoConfig
        cfg = VlmoConfig(dim=128, depth=2, heads=2, vlffn_start=1, image_size=32, patch=8, max_text_len=8, n_answers=7)
        model = FrozenVlmo(cfg, seed=4).to(dev)
        model.fused_blocks = True
        emb = model.text_embeddings(ids).detach()

        def forward(leaf_img, leaf_txt):
            feats, states = model.encode(leaf_img, leaf_txt, masks)
            return feats[1:] + [states]
        leaves = (image, emb)
    else:
        from vqattack_amd.whitebox.albef import AlbefConfig, FrozenAlbef
        monkeypatch.setenv("VQA_FUSED_TEXT", "1")
        cfg = AlbefConfig(dim=128, vit_depth=2, bert_depth=2, fusion_layer=1, heads=2, patch=8, image_size=32, n_answers=5,
                          decoder_depth=1, k_test=3, mlm_probability=0.0)
        model = FrozenAlbef(cfg, seed=4).to(dev)
        assert model.fused_blocks and model.fused_text
        emb = model.text_embeddings(ids).detach()
        if name == "albef_vit":
            def forward(leaf_img, _leaf_txt):
                states, feats = model.visual_encoder(leaf_img)
                return feats[1:] + [states]
            leaves = (image, None)
        else:
            with torch.no_grad():
                image_states = model.visual_encoder(image)[0].clone()

            def forward(leaf_img, leaf_txt):
                states, feats = model.text_encoder(leaf_txt, masks, leaf_img)
                return feats[1:] + [states]
            leaves = (image_states, emb)

    def run(grad):
        if not grad:
            with torch.no_grad():
                return [o.clone() for o in forward(*leaves)], []
        ins = [None if t is None else t.clone().requires_grad_(True) for t in leaves]
        outs = forward(*ins)
        gg = torch.Generator(device=dev).manual_seed(5)
        live = [t for t in ins if t is not None]
        torch.autograd.backward(outs, [torch.randn(o.shape, device=dev, generator=gg) for o in outs], inputs=live)
        return [o.detach().clone() for o in outs], [t.grad for t in live]
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["large", "wide"])
@pytest.mark.parametrize("name", ["vlmo", "albef_vit", "albef_fusion"])
def test_encoders_with_the_epilogue_on_equal_the_two_step_form_bitwise(name, mode, monkeypatch):
    torch, dev = _torch()
    from vqattack_amd.whitebox import _fused
    monkeypatch.setattr(_fused, "MIN_WORKGROUPS", 1)
    monkeypatch.setenv("VQA_GEMM", mode)
    run = _encoder_case(name, monkeypatch)
    fused_calls = []
    real = _fused.ops._gemm_epilogue

    def counting(a, pk, bias, out, tile, epilogue, aux):
        fused_calls.append((epilogue, aux is not None))
        return real(a, pk, bias, out, tile, epilogue, aux)
    monkeypatch.setattr(_fused.ops, "_gemm_epilogue", counting)
    results = {}
    for switch in ("0", "1"):
        monkeypatch.setenv("VQA_GEMM_EPILOGUE", switch)
        n0 = len(fused_calls)
        results[switch] = (run(True), run(False))
        if switch == "0":
            assert len(fused_calls) == n0, "VQA_GEMM_EPILOGUE=0 still fused"
    kinds = set(fused_calls)
    assert ("gelu", True) in kinds and ("gelu_grad", True) in kinds, "the fused path was not taken"
    assert ("gelu", False) in kinds, "the no_grad forward stored h"
    (outs0, grads0), (plain0, _) = results["0"]
    (outs1, grads1), (plain1, _) = results["1"]
    assert len(outs0) == len(outs1) and len(grads0) == len(grads1) >= 1
    for k, (x, y) in enumerate(zip(outs0 + grads0 + plain0, outs1 + grads1 + plain1)):
        assert torch.equal(x, y), (name, mode, k)
    assert all(float(gr.abs().max()) > 0 for gr in grads0)


@pytest.mark.gpu
@pytest.mark.parametrize("tile", ["large", "wide"])
def test_graph_replay_of_the_fused_calls_equals_eager_launch(tile):
    """One fused forward and one fused backward call captured on a single stream, replayed twice."""
    torch, dev = _torch()
    from vqattack_amd import ops
    gen = torch.Generator(device=dev).manual_seed(8)
    M, D, F = 300, 128, 256
    a = torch.randn(M, D, device=dev, generator=gen)
    w1 = torch.randn(F, D, device=dev, generator=gen) * (2.0 / math.sqrt(D))
    b1 = torch.randn(F, device=dev, generator=gen)
    w2 = torch.randn(D, F, device=dev, generator=gen) * (2.0 / math.sqrt(D))
    grad = torch.randn(M, D, device=dev, generator=gen)
    pk1, pk2 = ops.gemm_pack(w1, trans=True), ops.gemm_pack(w2, trans=False)

    def step(h, act, dh):
        ops.gemm(a, pk1, b1, out=act, tile=tile, epilogue="gelu", aux=h)
        ops.gemm(grad, pk2, out=dh, tile=tile, epilogue="gelu_grad", aux=h)
    eager = [torch.empty(M, F, device=dev) for _ in range(3)]
    step(*eager)
    static = [torch.zeros(M, F, device=dev) for _ in range(3)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(*static)
    for _ in range(2):
        for t in static:
            t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(static, eager):
            assert torch.equal(got, want)
