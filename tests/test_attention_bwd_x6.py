"""The bf16x6 attention backward (``vqa_attn_bwd_x6``: the dK / dV kernel's three products as six exact bf16 plane
products each) on the MI355X.

1. Operand maps with exact integers: scores in {0, -inf} with lse = 0 make P exactly 0 or 1, and integer q, k, v, go, o
   with scale 1/8 make delta, dP, dS (up to a few thousand: all three planes carry bits), dV, dK and dQ exact fp32
   numbers, so dq, dk, dv and the dS^T workspace must equal the fp32 grade's and the float64 result BITWISE (a wrong
   query permutation in either transposed image fails on almost every element).
2. All three planes: random fp32 at trained-model statistics against float64 by the rule of ``test_attention_fp64.py``
   (``err <= 2 err_sdpa + 1e-6 max|ref|``) and ``err <= 2 err_f32kernel + 1e-6 max|ref|``.  No fixed ceiling.
3. Dispatch: the loop-split, no-scores and no-workspace calls run fp32 whatever the switch says, and the entry point
   refuses them without launching anything.
4. Reproducibility: two calls give the same bits; ``KeyHoleBias`` and its dense form give the same gradients.
"""
import pytest
import torch

from tests import trained_stats as ts
from tests.test_attention_fp64 import _forms
from tests.test_attention_x6 import CASES, HOLE, _case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _grade(monkeypatch, grade):
    from vqattack_amd import attention
    monkeypatch.setenv("VQA_ATTN_BWD", grade)
    monkeypatch.setenv("VQA_ATTN_SPLIT", "1")
    monkeypatch.delenv("VQA_ATTN_FWD", raising=False)
    assert attention.backward_grade(1, True, True) == grade


def _pack(dense, fill):
    """Dense (B, H, R, C) -> the blocked slab of ``vqa_attn_scores_floats``: the inverse of the view / permute in
    ``test_attention_x6._fwd``.  Rows and columns up to the next multiple of 128 hold ``fill``."""
    b, h, rows, cols = dense.shape
    tr, tc = (rows + 127) // 128 * 4, (cols + 127) // 128 * 4
    full = torch.full((b, h, tr * 32, tc * 32), fill, dtype=dense.dtype, device=dense.device)
    full[:, :, :rows, :cols] = dense
    return full.view(b, h, tr, 32, tc, 4, 2, 4).permute(0, 1, 2, 4, 5, 6, 3, 7).contiguous().view(-1)


def _unpack(slab, b, h, rows, cols):
    """The blocked slab -> dense (B, H, rows, cols) (scores: rows = queries; dS^T: rows = keys)."""
    tr, tc = (rows + 127) // 128 * 4, (cols + 127) // 128 * 4
    s = slab.view(b, h, tr, tc, 4, 2, 32, 4).permute(0, 1, 2, 6, 3, 4, 5, 7).reshape(b, h, tr * 32, tc * 32)
    return s[:, :, :rows, :cols]


def _int_case(shape, strided):
    b, h, sq, sk = shape
    g = torch.Generator().manual_seed(sq * 1000 + sk)
    rnd = lambda lo, hi, *size: torch.randint(lo, hi + 1, size, generator=g).float()
    q, go, o = (rnd(-4, 4, b, sq, h, 64).to(DEV) for _ in range(3))
    if strided:                                            # K and V stacked in one projection output
        kv = torch.cat([rnd(-4, 4, b, sk, 1, h, 64), rnd(-8, 8, b, sk, 1, h, 64)], 2).to(DEV)
        k, v = kv[:, :, 0], kv[:, :, 1]
    else:
        k, v = rnd(-4, 4, b, sk, h, 64).to(DEV), rnd(-8, 8, b, sk, h, 64).to(DEV)
    live = torch.randint(0, 2, (b, h, sq, sk), generator=g).bool()
    live.scatter_(3, torch.randint(0, sk, (b, h, sq, 1), generator=g), True)      # at least one live key per query
    scores = torch.zeros(b, h, sq, sk).masked_fill(~live, float("-inf")).to(DEV)
    return q, k, v, go, o, scores


def _int_ref(q, k, v, go, o, scores):
    """float64 (dq, dk, dv, dS^T) at lse = 0, scale 1/8; every value is an integer or an eighth: exact in fp32."""
    q, k, v, go, o = (t.double() for t in (q, k, v, go, o))
    p = (scores == 0).double()
    delta = (go * o).sum(-1).permute(0, 2, 1)                                       # (B, H, Sq)
    ds = p * (torch.einsum("bqhd,bkhd->bhqk", go, v) - delta[..., None])
    return dict(dq=0.125 * torch.einsum("bhqk,bkhd->bqhd", ds, k), dk=0.125 * torch.einsum("bhqk,bqhd->bkhd", ds, q),
                dv=torch.einsum("bhqk,bqhd->bkhd", p, go), ds=ds.transpose(2, 3))


def _int_backward(monkeypatch, grade, q, k, v, go, o, scores, fill):
    from vqattack_amd import attention
    _grade(monkeypatch, grade)
    b, sq, h, _ = q.shape
    sk = k.shape[1]
    lse = torch.zeros(b, h, sq, device=DEV)
    dq, dk, dv = (torch.full((b, s, h, 64), 7.0, device=DEV) for s in (sq, sk, sk))
    ws = attention._backward(q, k, v, None, None, o, lse, go, dq, dk, dv, 0.125, scores=_pack(scores, fill))
    return dict(dq=dq, dk=dk, dv=dv, ds=_unpack(ws, b, h, sk, sq).clone())


INT_SHAPES = [((1, 2, 5, 5), False), ((1, 1, 32, 32), False), ((1, 1, 33, 33), False), ((2, 2, 129, 70), False),
              ((2, 1, 70, 129), False), ((1, 2, 25, 97), True)]


def _assert_int_case(monkeypatch, shape, strided, fill):
    case = _int_case(shape, strided)
    ref = _int_ref(*case)
    x6 = _int_backward(monkeypatch, "x6", *case, fill)
    f32 = _int_backward(monkeypatch, "f32", *case, fill)
    for name in ("dk", "dv", "dq", "ds"):
        assert float(ref[name].abs().max()) < 2 ** 24                              # the premise: exact in fp32
        want = ref[name].float()
        print("x6 backward integers {} {}: max |value| {:g}, x6 / f32 kernel elements off {} / {}".format(
            shape, name, float(want.abs().max()), int((x6[name] != want).sum()), int((f32[name] != want).sum())))
        assert torch.equal(x6[name], f32[name]), (name, int((x6[name] != f32[name]).sum()))
        assert torch.equal(x6[name], want), (name, int((x6[name] != want).sum()))
    assert float(ref["ds"].abs().max()) >= 256                                     # dS needs more than plane 0's 8 bits


@pytest.mark.parametrize("shape,strided", INT_SHAPES)
def test_operand_maps_with_exact_integers(shape, strided, monkeypatch):
    _assert_int_case(monkeypatch, shape, strided, 0.0)


def test_slab_padding_is_not_read_into_results(monkeypatch):
    _assert_int_case(monkeypatch, (2, 2, 129, 70), False, 7.0)


# ---------------------------------------------------------------------------------------------- all three planes
def _through(monkeypatch, grade, c, bias):
    from vqattack_amd import attention
    _grade(monkeypatch, grade)
    x = c["qkv"].clone().requires_grad_(True)
    o = attention.self_attention_packed(x, bias)
    o.backward(c["go"])
    _, lse = attention.attention_forward(c["qkv"][:, :, 0], c["qkv"][:, :, 1], c["qkv"][:, :, 2], bias)
    return dict(o=o.detach(), lse=lse, dq=x.grad[:, :, 0], dk=x.grad[:, :, 1], dv=x.grad[:, :, 2])


@pytest.mark.parametrize("kind,tau", CASES)
def test_backward_against_fp64(kind, tau, monkeypatch):
    _forms(monkeypatch, "saved_scores")
    c, khb, ref, yard = _case(kind, tau)
    got = _through(monkeypatch, "x6", c, khb)
    f32 = _through(monkeypatch, "f32", c, khb)
    for name in ("o", "lse", "dq", "dk", "dv"):
        scale = float(ref[name].abs().max())
        ex, ef, ey = (float((t[name].double() - ref[name]).abs().max()) for t in (got, f32, yard))
        print("x6 backward fp64 {} tau={:g} {}: x6 / f32 kernel / sdpa max err {:.3g} / {:.3g} / {:.3g} (max|ref| {:.3g})"
              .format(kind, tau, name, ex, ef, ey, scale))
        assert ex <= 2.0 * ey + 1e-6 * scale, (name, ex, ey, scale)
        assert ex <= 2.0 * ef + 1e-6 * scale, (name, ex, ef, scale)
    grad = got["dk"].abs() + got["dv"].abs()
    assert float(grad[0, HOLE[0]:HOLE[1]].max()) == 0.0                            # the hole's keys: dK = dV = 0 exactly
    if kind == "lead_inf":
        assert float(grad[:, :ts.LEAD].max()) == 0.0                               # -inf keys: dK = dV = 0 exactly


# ------------------------------------------------------------------------------------------------------- dispatch
@pytest.mark.parametrize("switch", ["x6", "f32", None])
def test_calls_without_an_x6_form_run_fp32(switch, monkeypatch):
    from vqattack_amd import attention
    if switch is None:
        monkeypatch.delenv("VQA_ATTN_BWD", raising=False)
    else:
        monkeypatch.setenv("VQA_ATTN_BWD", switch)
    assert attention.backward_grade(1, True, True) == (switch or attention.BACKWARD_DEFAULT)
    assert attention.backward_grade(2, True, True) == "f32"                        # loop-split
    assert attention.backward_grade(1, False, True) == "f32"                       # form ds_workspace: no saved scores
    assert attention.backward_grade(1, False, False) == "f32"                      # form recompute: no workspace
    assert attention.backward_grade(1, True, False) == "f32"


@pytest.mark.parametrize("form", ["ds_workspace", "recompute"])
def test_forms_without_saved_scores_ignore_the_switch(form, monkeypatch):
    """With the switch at x6 these forms give the bits they give with it at f32."""
    _forms(monkeypatch, form)
    c, khb, _, _ = _case("plain", 1.0)
    a = _through_switch(monkeypatch, "x6", c, khb)
    b = _through_switch(monkeypatch, "f32", c, khb)
    for name in ("dq", "dk", "dv"):
        assert torch.equal(a[name], b[name]), name


def _through_switch(monkeypatch, switch, c, bias):
    from vqattack_amd import attention
    monkeypatch.setenv("VQA_ATTN_BWD", switch)
    monkeypatch.setenv("VQA_ATTN_SPLIT", "1")
    x = c["qkv"].clone().requires_grad_(True)
    attention.self_attention_packed(x, bias).backward(c["go"])
    return dict(dq=x.grad[:, :, 0], dk=x.grad[:, :, 1], dv=x.grad[:, :, 2])


def test_entry_point_refuses_other_forms_and_launches_nothing():
    from vqattack_amd import _hip, attention
    lib = _hip.lib()
    b, h, s = 1, 2, 40
    q, go = torch.randn(b, s, h, 64, device=DEV), torch.randn(b, s, h, 64, device=DEV)
    o, lse, scores = (t for t in attention._forward(q, q, q, None, None, 0.125, save_scores=True))
    assert scores is not None
    dq, dk, dv = (torch.full_like(q, 7.0) for _ in range(3))
    delta = torch.full((b, h, s), 7.0, device=DEV)
    ds_ws = torch.empty(lib.vqa_attn_bwd_ws_floats(b, h, s, s), device=DEV)
    split_ws = torch.empty(lib.vqa_attn_split_ws_floats(b, h, s, s, 2), device=DEV)
    strides = attention._longs([q.stride(0), q.stride(1), q.stride(2)] * 4)
    p = _hip.ptr

    def call(scores_, ds_, nsplit):
        return lib.vqa_attn_bwd_x6(p(q), p(q), p(q), None, p(o), p(go), p(lse), p(scores_), p(delta), p(dq), p(dk), p(dv),
                                   p(ds_), b, h, s, s, strides, None, strides, 0.125, nsplit,
                                   p(split_ws) if nsplit > 1 else None, None)

    for args in ((scores, ds_ws, 2), (None, ds_ws, 1), (scores, None, 1)):
        assert call(*args) == -2                                                   # VQA_ERR_SHAPE
    torch.cuda.synchronize()
    for t in (dq, dk, dv, delta):
        assert float(t.min()) == 7.0 == float(t.max())
    assert call(scores, ds_ws, 1) == 0
    torch.cuda.synchronize()
    for t in (dq, dk, dv):
        assert float((t - 7.0).abs().min()) > 0.0


# ------------------------------------------------------------------------------------------------ reproducibility
def test_two_calls_give_the_same_bits(monkeypatch):
    c, khb, _, _ = _case("plain", 8.0)
    a = _through(monkeypatch, "x6", c, khb)
    b = _through(monkeypatch, "x6", c, khb)
    for name in ("dq", "dk", "dv"):
        assert torch.equal(a[name], b[name]), name


def test_key_hole_bias_and_its_dense_form_give_the_same_bits(monkeypatch):
    c, khb, _, _ = _case("lead_inf", 4.0)
    a = _through(monkeypatch, "x6", c, khb)
    b = _through(monkeypatch, "x6", c, khb.dense())
    for name in ("dq", "dk", "dv"):
        assert torch.equal(a[name], b[name]), name
