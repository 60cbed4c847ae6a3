"""The bf16x6 attention forward (``vqa_attn_fwd_x6``: both products as six exact bf16 plane products) on the MI355X.

1. Operand maps with exact integers: q, k in [-4, 4], v in [-8, 8], scale 1/8 and biases in eighths make every product and
   sum exact in bf16 plane 0 and in fp32, so the saved scores must equal the fp32 kernel's and the float64 product BITWISE
   (a wrong k permutation of either chain fails on almost every element), and with a 0 / -inf bias that leaves one live
   key per query, at a score whose exponential is exactly 1, ``o`` is that key's V row, bitwise.
2. All three planes: random fp32 at trained-model statistics against float64 by the rule of ``test_attention_fp64.py``
   (``err <= 2 err_sdpa + 1e-6 max|ref|``), and additionally ``err <= 2 err_f32kernel + 1e-6 max|ref|`` with the fp32
   kernel on the same inputs: both are fp32-grade and differ by rounding order, hence the margin of 2.  No fixed ceiling.
3. ``self_attention_packed`` with x6 on and its backward (fp32 kernels, all three forms), by the same rule.
4. The score-storing and the plain variant give bitwise equal o and lse.
5. ``nsplit != 1`` is an error and launches nothing.

The two backward forms that do not read saved scores (``ds_workspace``, ``recompute``) recompute q k^T in fp32 MFMA, and
that chain's rounding cancels in P = exp(s - lse) only against the lse of the fp32 forward: with the x6 forward paired to
them, dq of ``plain`` at tau = 8 read 1.71e-05 / 1.66e-05 against the fp32 forward's 5.69e-06 / 5.80e-06 (bounds 1.42e-05 /
1.45e-05).  ``attention.forward_grade`` therefore runs the fp32 forward for a differentiated call that cannot save its
scores, switch or no switch; test 3 holds the product to the rule in all three forms and checks which kernel each ran.
"""
import pytest
import torch

from tests import trained_stats as ts
from tests.test_attention_fp64 import _forms, _ref64, _sdpa32

pytestmark = pytest.mark.gpu
DEV = "cuda"
HOLE = (30, 40)                    # straddles the boundary of key tiles 0 and 1


def _grade(monkeypatch, grade):
    from vqattack_amd import attention
    monkeypatch.setenv("VQA_ATTN_FWD", grade)
    monkeypatch.setenv("VQA_ATTN_SPLIT", "1")
    assert attention.forward_grade(1) == grade


def _fwd(monkeypatch, grade, q, k, v, bias, save):
    """(o, lse, scores (B, H, Sq, Sk) or None) of one forward launch of the given grade."""
    from vqattack_amd import attention
    _grade(monkeypatch, grade)
    qq, kk, vv, bt, bstr, scale, hole = attention._prepare(q, k, v, bias, 0.125, need_grad=save)
    o, lse, scores = attention._forward(qq, kk, vv, bt, bstr, scale, save_scores=save, key_hole=hole)
    assert (scores is not None) == save
    if save:
        b, sq, h, _ = q.shape
        sk = k.shape[1]
        tr, tc = (sq + 127) // 128 * 4, (sk + 127) // 128 * 4
        # a tile is the producing wave's registers: chunk g of lane (r, hh) = query r, keys 8 g + 4 hh .. + 3
        s = scores.view(b, h, tr, tc, 4, 2, 32, 4).permute(0, 1, 2, 6, 3, 4, 5, 7).reshape(b, h, tr * 32, tc * 32)
        scores = s[:, :, :sq, :sk]
    return o, lse, scores


def _int_case(shape, mode, strided):
    from vqattack_amd import attention
    b, h, sq, sk = shape
    g = torch.Generator().manual_seed(sq * 1000 + sk)
    q = torch.randint(-4, 5, (b, sq, h, 64), generator=g).float().to(DEV)
    if strided:                                            # K and V stacked in one projection output
        kv = torch.cat([torch.randint(-4, 5, (b, sk, 1, h, 64), generator=g),
                        torch.randint(-8, 9, (b, sk, 1, h, 64), generator=g)], 2).float().to(DEV)
        k, v = kv[:, :, 0], kv[:, :, 1]
    else:
        k = torch.randint(-4, 5, (b, sk, h, 64), generator=g).float().to(DEV)
        v = torch.randint(-8, 9, (b, sk, h, 64), generator=g).float().to(DEV)
    bias = dense = live = None
    if mode == "one_live_key":
        # P of the live key is exp2(fma(s, log2 e, -round(s log2 e))): exactly 1 -- and o exactly the V row -- only when
        # s log2 e is an fp32 number, i.e. s is 0 or a power of two.  One nonzero element of +-1, 2 or 4 per query row
        # (at a random dimension, so every k slot of the S chain still carries one) and keys without +-3 make it so.
        pow2 = torch.tensor([-4.0, -2.0, -1.0, 0.0, 1.0, 2.0, 4.0])
        dim = torch.randint(0, 64, (b, sq, h, 1), generator=g)
        val = pow2[torch.randint(0, 7, (b, sq, h, 1), generator=g)]
        q = torch.zeros(b, sq, h, 64).scatter_(3, dim, val).to(DEV)
        k.copy_(pow2[torch.randint(0, 7, tuple(k.shape), generator=g)].to(DEV))
    if mode == "bias":                                     # eighths in [-2, 2] + a key hole in sample 0
        dense = (torch.randint(-16, 17, (1, h, sq, sk), generator=g).float() / 8).to(DEV).expand(b, -1, -1, -1)
        bias = dense
        if sk > HOLE[0]:
            hole = torch.tensor([[HOLE[0], min(HOLE[1], sk)]] + [[0, 0]] * (b - 1), dtype=torch.int32, device=DEV)
            bias = attention.KeyHoleBias(dense, hole)
            dense = bias.dense()
    elif mode == "one_live_key":
        live = (7 * torch.arange(sq)[None, None, :] + 3 * torch.arange(h)[None, :, None] +
                torch.arange(b)[:, None, None]) % sk                                          # (B, H, Sq)
        dense = torch.full((b, h, sq, sk), float("-inf")).scatter_(3, live[..., None], 0.0).to(DEV)
        bias, live = dense, live.to(DEV)
    return q, k, v, bias, dense, live


INT_SHAPES = [((1, 2, 5, 5), False), ((1, 1, 32, 32), False), ((1, 1, 33, 33), False), ((2, 2, 129, 70), False),
              ((1, 2, 25, 97), True)]


@pytest.mark.parametrize("mode", ["no_bias", "bias", "one_live_key"])
@pytest.mark.parametrize("shape,strided", INT_SHAPES)
def test_operand_maps_with_exact_integers(shape, strided, mode, monkeypatch):
    q, k, v, bias, dense, live = _int_case(shape, mode, strided)
    s64 = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) * 0.125
    if dense is not None:
        s64 = s64 + dense.double()
    o64 = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s64, -1), v.double())
    lse64 = torch.logsumexp(s64, -1)
    ox, lx, sx = _fwd(monkeypatch, "x6", q, k, v, bias, True)
    of, lf, sf = _fwd(monkeypatch, "f32", q, k, v, bias, True)
    assert torch.equal(sx, sf), int((sx != sf).sum())
    assert torch.equal(sx, s64.float()), int((sx != s64.float()).sum())
    if mode == "one_live_key":                             # P is 1 for one key and exactly 0 for the others
        b, h, sq, _ = shape
        rows = v[torch.arange(b, device=DEV)[:, None, None], live.permute(0, 2, 1),
                 torch.arange(h, device=DEV)[None, None, :]]                                   # (B, Sq, H, 64)
        assert torch.equal(ox, rows), int((ox != rows).sum())
    for name, got, f32, ref in (("o", ox, of, o64), ("lse", lx, lf, lse64)):
        ex, ef = float((got.double() - ref).abs().max()), float((f32.double() - ref).abs().max())
        print("x6 integers {} {} {}: x6 / f32 kernel max err {:.3g} / {:.3g}".format(shape, mode, name, ex, ef))
        assert ex <= 2.0 * ef + 1e-6 * float(ref.abs().max()), (name, ex, ef)
    o2, l2, _ = _fwd(monkeypatch, "x6", q, k, v, bias, False)                                  # the variant that stores no scores
    assert torch.equal(o2, ox) and torch.equal(l2, lx)


# ---------------------------------------------------------------------------------- all three planes, and the backward
CASES = [("plain", 1.0), ("plain", 8.0), ("ramp", 4.0), ("sink", 4.0), ("lead_inf", 4.0)]
HOLES = [[HOLE[0], HOLE[1]], [40, 40]]
_REF = {}


def _case(kind, tau):
    """(case, bias with holes, float64 reference, fp32 library yardstick) at (2, 2, 97, 97), computed once per case."""
    if (kind, tau) not in _REF:
        from vqattack_amd import attention
        c = {n: t.to(DEV) for n, t in ts.attn_case(kind, 2, 2, 97, 97, tau=tau, packed=True).items()}
        khb = attention.KeyHoleBias(c["bias"].expand(2, -1, -1, -1), torch.tensor(HOLES, dtype=torch.int32, device=DEV))
        q, k, v = c["qkv"][:, :, 0], c["qkv"][:, :, 1], c["qkv"][:, :, 2]
        _REF[kind, tau] = (c, khb, _ref64(q, k, v, khb.dense(), c["go"]), _sdpa32(q, k, v, khb.dense(), c["go"]))
    return _REF[kind, tau]


def _through(monkeypatch, grade, c, khb):
    from vqattack_amd import attention
    _grade(monkeypatch, grade)
    x = c["qkv"].clone().requires_grad_(True)
    o = attention.self_attention_packed(x, khb)
    o.backward(c["go"])
    o2, lse = attention.attention_forward(c["qkv"][:, :, 0], c["qkv"][:, :, 1], c["qkv"][:, :, 2], khb)
    return dict(o=o.detach(), lse=lse, dq=x.grad[:, :, 0], dk=x.grad[:, :, 1], dv=x.grad[:, :, 2]), o2


@pytest.mark.parametrize("form", ["saved_scores", "ds_workspace", "recompute"])
@pytest.mark.parametrize("kind,tau", CASES)
def test_forward_and_backward_through_it_against_fp64(kind, tau, form, monkeypatch):
    from vqattack_amd import attention
    _forms(monkeypatch, form)
    c, khb, ref, yard = _case(kind, tau)
    got, o_plain = _through(monkeypatch, "x6", c, khb)
    # the x6 forward pairs with the backward that starts from its saved scores only (see the module's notes)
    assert attention.forward_grade(1, recomputing_backward=form != "saved_scores") == ("x6" if form == "saved_scores" else "f32")
    f32, _ = _through(monkeypatch, "f32", c, khb)
    if form == "saved_scores":
        assert torch.equal(o_plain, got["o"])                                  # score-storing and plain variant: the same bits
    for name in ("o", "lse", "dq", "dk", "dv"):
        scale = float(ref[name].abs().max())
        ex, ef, ey = (float((t[name].double() - ref[name]).abs().max()) for t in (got, f32, yard))
        print("x6 fp64 {} tau={:g} {} {}: x6 / f32 kernel / sdpa max err {:.3g} / {:.3g} / {:.3g} (max|ref| {:.3g})".format(
            kind, tau, form, name, ex, ef, ey, scale))
        assert ex <= 2.0 * ey + 1e-6 * scale, (name, ex, ey, scale)
        assert ex <= 2.0 * ef + 1e-6 * scale, (name, ex, ef, scale)
    grad = got["dk"].abs() + got["dv"].abs()
    assert float(grad[0, HOLE[0]:HOLE[1]].max()) == 0.0                        # the hole's keys: dK = dV = 0 exactly
    if kind == "lead_inf":
        assert float(grad[:, :ts.LEAD].max()) == 0.0                           # -inf keys: dK = dV = 0 exactly


@pytest.mark.parametrize("kind,tau", CASES)
def test_score_storing_and_plain_variant_agree_bitwise(kind, tau, monkeypatch):
    c, khb, _, _ = _case(kind, tau)
    q, k, v = c["qkv"][:, :, 0], c["qkv"][:, :, 1], c["qkv"][:, :, 2]
    for bias in (khb, None):
        o1, l1, _ = _fwd(monkeypatch, "x6", q, k, v, bias, True)
        o2, l2, _ = _fwd(monkeypatch, "x6", q, k, v, bias, False)
        assert torch.equal(o1, o2) and torch.equal(l1, l2)


def test_loop_split_is_refused_and_launches_nothing(monkeypatch):
    from vqattack_amd import _hip, attention
    lib = _hip.lib()
    q = torch.randn(1, 40, 2, 64, device=DEV)
    o, lse = torch.full_like(q, 7.0), torch.full((1, 2, 40), 7.0, device=DEV)
    strides = attention._longs([q.stride(0), q.stride(1), q.stride(2)] * 4)
    ws = torch.empty(lib.vqa_attn_split_ws_floats(1, 2, 40, 40, 2), device=DEV)
    args = (_hip.ptr(q), _hip.ptr(q), _hip.ptr(q), None, _hip.ptr(o), _hip.ptr(lse), None, 1, 2, 40, 40, strides, None, 0.125, None)
    for nsplit in (2, 0):
        assert lib.vqa_attn_fwd_x6(*args, nsplit, _hip.ptr(ws), None) == -2    # VQA_ERR_SHAPE
    torch.cuda.synchronize()
    assert float(o.min()) == 7.0 == float(o.max()) and float(lse.min()) == 7.0 == float(lse.max())
    assert lib.vqa_attn_fwd_x6(*args, 1, None, None) == 0
    torch.cuda.synchronize()
    assert float((o - 7.0).abs().min()) > 0.0
    _grade(monkeypatch, "x6")
    assert attention.forward_grade(2) == "f32"                                 # the dispatch never sends a split call there
