"""fp32 MFMA attention (csrc/attn.hip) against float64 at trained-model statistics (``tests/trained_stats.py``).

Reference: the same fp32 inputs promoted to float64 on the device, ``softmax(scale q k^T + bias) v`` written out, its
logsumexp, and the gradients by float64 autograd.  Yardstick: ``F.scaled_dot_product_attention`` in fp32 (and
``torch.logsumexp`` of the fp32 scores) against the same reference.  Rule for each of o, lse, dq, dk, dv:
``err_kernel <= 2 err_sdpa + 1e-6 max|ref|``, and a fixed ceiling ``CEIL[name] * max|ref|`` set from the yardstick's
own largest error over these cases, so that a degraded yardstick cannot carry a degraded kernel.  The cases rescale the
forward's running max (key ramps, a sink key, masked leading tiles), hand the loop split's combine a fully masked part
and a part whose weight underflows, and run every backward form.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import trained_stats as ts

pytestmark = pytest.mark.gpu
DEV = "cuda"
SCALE = ts.HEAD ** -0.5
# about 4x the yardstick's largest max error / max|ref| over these cases on the MI355X (o 3.1e-6, lse 3.5e-7, dq 1.7e-5,
# dk 1.5e-5, dv 2.2e-5); the yardstick itself must stay within CEIL / 4
CEIL = {"o": 1.6e-5, "lse": 1.6e-6, "dq": 8e-5, "dk": 8e-5, "dv": 1e-4}
SELF_HOLES = [[6, 40], [40, 40]]


def _ref64(q, k, v, bias, go):
    """float64 (o, lse, dq, dk, dv) of fp32 device tensors; ``bias`` dense, broadcastable to (B, H, Sq, Sk)."""
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    s = torch.einsum("bqhd,bkhd->bhqk", q64, k64) * SCALE + bias.double()
    o = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v64)
    dq, dk, dv = torch.autograd.grad(o, (q64, k64, v64), go.double())
    return dict(o=o.detach(), lse=torch.logsumexp(s.detach(), -1), dq=dq, dk=dk, dv=dv)


def _sdpa32(q, k, v, bias, go):
    qs, ks, vs = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    o = F.scaled_dot_product_attention(qs.transpose(1, 2), ks.transpose(1, 2), vs.transpose(1, 2), attn_mask=bias,
                                       scale=SCALE).transpose(1, 2)
    dq, dk, dv = torch.autograd.grad(o, (qs, ks, vs), go)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * SCALE + bias
    return dict(o=o.detach(), lse=torch.logsumexp(s, -1), dq=dq, dk=dk, dv=dv)


def _check(tag, got, ref, yard):
    rows = []
    for name in ("o", "lse", "dq", "dk", "dv"):
        scale = float(ref[name].abs().max())
        ek = float((got[name].double() - ref[name]).abs().max())
        ey = float((yard[name].double() - ref[name]).abs().max())
        rows.append((name, ek, ey, scale))
    print("FP64 attention {}: kernel/sdpa max err {}".format(
        tag, " ".join("{}={:.3g}/{:.3g} (rel {:.3g}/{:.3g})".format(n, ek, ey, ek / s, ey / s) for n, ek, ey, s in rows)))
    for name, ek, ey, scale in rows:
        assert ek <= 2.0 * ey + 1e-6 * scale, (tag, name, ek, ey, scale)
        assert ek <= CEIL[name] * scale, (tag, name, ek, scale)
        assert ey <= CEIL[name] * scale / 4, ("yardstick", tag, name, ey, scale)


def _device(case):
    return {k: v.to(DEV) for k, v in case.items()}


def _forms(monkeypatch, form):
    from vqattack_amd import attention
    if form != "saved_scores":
        monkeypatch.setattr(attention, "SCORES_LIMIT", 0)
    if form == "recompute":
        monkeypatch.setattr(attention, "DS_WORKSPACE_LIMIT", 0)


_REF = {}


def _self_ref(kind, tau):
    """Packed self-attention (2, 12, 591) with a shared bias slab and per-sample key holes; reference and yardstick are
    computed once per case and shared by the backward forms."""
    key = ("self", kind, tau)
    if key not in _REF:
        from vqattack_amd import attention
        c = _device(ts.attn_case(kind, 2, 12, 591, 591, tau=tau, packed=True))
        hole = torch.tensor(SELF_HOLES, dtype=torch.int32, device=DEV)
        khb = attention.KeyHoleBias(c["bias"].expand(2, -1, -1, -1), hole)
        dense = khb.dense()
        q, k, v = c["qkv"][:, :, 0], c["qkv"][:, :, 1], c["qkv"][:, :, 2]
        _REF[key] = (c, khb, _ref64(q, k, v, dense, c["go"]), _sdpa32(q, k, v, dense, c["go"]))
    return _REF[key]


# (kind, q temperature): the controls run the saved-scores backward only, the others every backward form
CONTROLS = [("plain", 1.0), ("plain", 4.0), ("ramp_rev", 4.0)]
HOT = [("plain", 8.0), ("ramp", 4.0), ("sink", 4.0), ("lead_inf", 4.0), ("lead_bert", 4.0)]
SELF_PARAMS = [(k, t, "saved_scores") for k, t in CONTROLS] + [(k, t, f) for k, t in HOT
                                                                 for f in ("saved_scores", "ds_workspace", "recompute")]


@pytest.mark.parametrize("kind,tau,form", SELF_PARAMS)
def test_packed_self_attention_against_fp64(kind, tau, form, monkeypatch):
    from vqattack_amd import attention
    _forms(monkeypatch, form)
    monkeypatch.setenv("VQA_ATTN_SPLIT", "1")
    c, khb, ref, yard = _self_ref(kind, tau)
    x = c["qkv"].clone().requires_grad_(True)
    o = attention.self_attention_packed(x, khb)
    o.backward(c["go"])
    _, lse = attention.attention_forward(c["qkv"][:, :, 0], c["qkv"][:, :, 1], c["qkv"][:, :, 2], khb)
    got = dict(o=o.detach(), lse=lse, dq=x.grad[:, :, 0], dk=x.grad[:, :, 1], dv=x.grad[:, :, 2])
    _check("self {} tau={:g} {}".format(kind, tau, form), got, ref, yard)
    assert float(x.grad[0, 6:40, 1:].abs().max()) == 0.0                       # the hole's keys: dK = dV = 0 exactly
    if kind == "lead_inf":
        assert float(x.grad[:, :ts.LEAD, 1:].abs().max()) == 0.0               # -inf keys: dK = dV = 0 exactly


@pytest.mark.parametrize("form", ["saved_scores", "recompute"])
@pytest.mark.parametrize("kind,tau", HOT)
def test_cross_attention_25_queries_901_keys_against_fp64(kind, tau, form, monkeypatch):
    """ALBEF's fusion cross-attention at batch 1; its forward runs loop-split by the default heuristic."""
    from vqattack_amd import attention
    _forms(monkeypatch, form)
    monkeypatch.delenv("VQA_ATTN_SPLIT", raising=False)
    c = _device(ts.attn_case(kind, 1, 12, 25, 901, tau=tau))
    assert attention.loop_split(1, 12, 25, 901, DEV, backward=False) > 1
    q, k, v = (c[n].clone().requires_grad_(True) for n in "qkv")
    o = attention.attention(q, k, v, c["bias"])
    o.backward(c["go"])
    _, lse = attention.attention_forward(c["q"], c["k"], c["v"], c["bias"])
    got = dict(o=o.detach(), lse=lse, dq=q.grad, dk=k.grad, dv=v.grad)
    _check("cross {} tau={:g} {}".format(kind, tau, form), got, _ref64(c["q"], c["k"], c["v"], c["bias"], c["go"]),
           _sdpa32(c["q"], c["k"], c["v"], c["bias"], c["go"]))
    if kind == "lead_inf":
        assert float(k.grad[:, :ts.LEAD].abs().max()) == 0.0 and float(v.grad[:, :ts.LEAD].abs().max()) == 0.0


@pytest.mark.parametrize("n", [3, 8])
def test_loop_split_combine_against_fp64(n, monkeypatch):
    """The forward's parts include one whose keys are all masked (partial max -inf, weight 0) and one whose weight
    underflows to 0 against the row max; the backward's split parts sum partial dK / dV / dQ."""
    from vqattack_amd import attention
    monkeypatch.setenv("VQA_ATTN_SPLIT", str(n))
    c = _device(ts.attn_case("split", 1, 12, 591, 591, tau=1.0, packed=True))
    assert attention.loop_split(1, 12, 591, 591, DEV) == n
    q, k, v = c["qkv"][:, :, 0], c["qkv"][:, :, 1], c["qkv"][:, :, 2]
    x = c["qkv"].clone().requires_grad_(True)
    o = attention.self_attention_packed(x, c["bias"])
    o.backward(c["go"])
    _, lse = attention.attention_forward(q, k, v, c["bias"])
    got = dict(o=o.detach(), lse=lse, dq=x.grad[:, :, 0], dk=x.grad[:, :, 1], dv=x.grad[:, :, 2])
    _check("split n={}".format(n), got, _ref64(q, k, v, c["bias"], c["go"]), _sdpa32(q, k, v, c["bias"], c["go"]))
    assert float(x.grad[:, :ts.SPLIT_MASKED, 1:].abs().max()) == 0.0          # masked keys: dK = dV = 0 exactly
