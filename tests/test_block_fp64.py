"""LayerNorm, GELU and the bf16x6 GEMM against float64 at trained-model statistics (``tests/trained_stats.py``).

LayerNorm (``vqa_ln_fwd`` / ``vqa_ln_bwd``, and the text side's ``vqa_embed_tokens``) on offset, outlier, constant and
near-constant rows at the products' two epsilons: y, mean, rstd and dx within 2x torch fp32 on the device + a floor of
a few fp32 steps.  GELU: every one of the 2^32 fp32 inputs through both kernels, bounded per element against float64 by
a bound that torch's own fp32 GELU meets too.  GEMM: operands whose result is exact in fp32 must give the fp64 product bit
for bit (plane placement, k order, product selection); trained-statistics operands at two benchmark shapes stay within
2x the library GEMM and within the elementwise fp32 dot-product bound.
"""
import pytest
import torch
import torch.nn.functional as F

from tests import trained_stats as ts

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24                       # fp32 unit roundoff


def _cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


def _err(a, ref):
    return float((a.double() - ref).abs().max())


def _rule(tag, got, yard, ref, floor_ulps=4, ceil_ulps=32):
    """err_kernel <= 2 err_torch + floor_ulps * U * max|ref| for every named output, and a fixed ceiling of ceil_ulps *
    U * max|ref| that does not lean on torch (whose fp32 LayerNorm on the device is far off on near-constant rows:
    errors of 1e2 in y at eps = 1e-12); prints both errors."""
    rows = []
    for name in got:
        scale = float(ref[name].abs().max())
        rows.append((name, _err(got[name], ref[name]), _err(yard[name], ref[name]), scale))
    print("FP64 {}: kernel/torch max err {}".format(tag, " ".join(
        "{}={:.3g}/{:.3g}".format(n, ek, ey) for n, ek, ey, _ in rows)))
    for name, ek, ey, scale in rows:
        assert ek <= 2.0 * ey + floor_ulps * U * scale, (tag, name, ek, ey, scale)
        assert ek <= ceil_ulps * U * scale, (tag, name, ek, scale)


# ------------------------------------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize("mode", ["plain", "residual"])
@pytest.mark.parametrize("eps", [1e-6, 1e-12])
@pytest.mark.parametrize("d", [768, 1024, 200])
@pytest.mark.parametrize("kind", ts.LN_KINDS)
def test_layernorm_against_fp64(kind, d, eps, mode):
    from vqattack_amd import ops
    rows = 48
    g = _cpu_gen(d + 7 * ts.LN_KINDS.index(kind))
    target = ts.ln_rows(kind, rows, d)
    gamma, beta = 1.0 + 0.3 * torch.randn(d, generator=g), 0.3 * torch.randn(d, generator=g)
    dy = torch.randn(rows, d, generator=g)
    r = torch.randn(rows, d, generator=g) * 0.5
    target, gamma, beta, dy, r = (t.to(DEV) for t in (target, gamma, beta, dy, r))
    y, mean, rstd = torch.empty(rows, d, device=DEV), torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    if mode == "residual":                                    # x_out = x + r lands on the case's rows (fp32-rounded)
        x_in = target - r
        x_out = torch.empty_like(x_in)
        ops.ln_fwd(x_in, gamma, beta, y, mean, rstd, eps, r0=r, x_out=x_out)
        x = x_in + r
        assert torch.equal(x_out, x)
    else:
        x = target
        ops.ln_fwd(x, gamma, beta, y, mean, rstd, eps)
    dx = torch.empty_like(x)
    ops.ln_bwd(dy, x, mean, rstd, gamma, dx)

    def ln(t, gm, bt):
        t = t.clone().requires_grad_(True)
        out, m, rs = torch.ops.aten.native_layer_norm(t, [d], gm, bt, eps)
        (gx,) = torch.autograd.grad(out, t, dy.to(t.dtype))
        return dict(y=out.detach(), mean=m.view(-1), rstd=rs.view(-1), dx=gx)

    ref = ln(x.double(), gamma.double(), beta.double())
    yard = ln(x, gamma, beta)
    _rule("layernorm {} D={} eps={:g} {}".format(kind, d, eps, mode), dict(y=y, mean=mean, rstd=rstd, dx=dx), yard, ref)


def test_embed_tokens_near_constant_rows_against_fp64():
    """BERT embeddings at eps = 1e-12 with word + type + position near-constant for a third of the tokens."""
    from vqattack_amd import ops
    v, length, d, b = 40, 12, 768, 3
    g = _cpu_gen(12)
    word = torch.randn(v, d, generator=g) * 0.05
    word[5:10] = 0.3 + 1e-7 * torch.randn(5, d, generator=g).double().float()        # near-constant words
    word[10] = 0.7                                                                      # an exactly constant word
    pos = torch.randn(length, d, generator=g) * 0.02
    pos[:4] = 0.02                                                                      # constant positions
    type_emb = torch.full((2, d), 0.01)
    gamma, beta = 1.0 + 0.3 * torch.randn(d, generator=g), 0.3 * torch.randn(d, generator=g)
    ids = torch.randint(11, v, (b, length), generator=g)
    ids[:, :4] = torch.tensor([[5, 6, 7, 10], [8, 9, 10, 5], [10, 10, 6, 7]])
    tables = {k: t.to(DEV) for k, t in dict(word=word, pos=pos, type_emb=type_emb, gamma=gamma, beta=beta).items()}
    tables["ln_eps"] = 1e-12
    got = ops.embed_tokens(tables, ids.to(DEV))
    e = (tables["word"][ids.to(DEV)] + tables["type_emb"][0]) + tables["pos"][None]       # the kernel's fp32 sum
    ref = F.layer_norm(e.double(), (d,), tables["gamma"].double(), tables["beta"].double(), 1e-12)
    yard = F.layer_norm(e, (d,), tables["gamma"], tables["beta"], 1e-12)
    _rule("embed_tokens eps=1e-12", dict(y=got), dict(y=yard), dict(y=ref))


# ------------------------------------------------------------------------------------------------------------ GELU
CHUNK = 1 << 28
GELU_ULPS, GELU_TAIL = 4.0, 2.0      # |err| <= GELU_ULPS ulp(ref) + GELU_TAIL |x| 2^-24


def _ulp32(ref):
    """fp32 ulp at each float64 value (subnormal step below 2^-126)."""
    e = torch.frexp(ref).exponent
    return torch.ldexp(torch.ones_like(ref), (e - 24).clamp(min=-149))


def _gelu_grad64(x):
    return torch.ops.aten.gelu_backward(torch.ones_like(x), x)


@pytest.mark.parametrize("which", ["fwd", "bwd"])
def test_gelu_on_every_fp32_input(which):
    """All 2^32 bit patterns.  Non-finite results in the same class (NaN / +inf / -inf) as torch fp32; finite results
    within GELU_ULPS ulp of the float64 value plus GELU_TAIL |x| 2^-24 -- the cancellation of 1 + erf(x / sqrt 2) in the
    left tail, which torch's fp32 GELU meets on every input too."""
    from vqattack_amd import ops
    worst = {"kernel": 0.0, "torch": 0.0}
    worst_ulp = {"kernel": 0.0, "torch": 0.0}
    for lo in range(-(1 << 31), 1 << 31, CHUNK):
        x = torch.arange(lo, lo + CHUNK, dtype=torch.int32, device=DEV).view(torch.float32)
        if which == "fwd":
            got = ops.gelu_fwd(x)
            yard = F.gelu(x)
        else:
            got = ops.gelu_bwd(x, torch.ones_like(x))
            yard = torch.ops.aten.gelu_backward(torch.ones_like(x), x)
        for name, t in (("kernel", got), ("torch", yard)):
            assert torch.equal(torch.isnan(t), torch.isnan(yard)), (which, name, lo)
            assert torch.equal(torch.isposinf(t), torch.isposinf(yard)), (which, name, lo)
            assert torch.equal(torch.isneginf(t), torch.isneginf(yard)), (which, name, lo)
        fin = torch.isfinite(yard)
        xf = x[fin].double()
        ref = F.gelu(xf) if which == "fwd" else _gelu_grad64(xf)
        ulp = _ulp32(ref)
        bound = GELU_ULPS * ulp + GELU_TAIL * xf.abs() * U
        outside_tail = xf >= -1.0
        for name, t in (("kernel", got), ("torch", yard)):
            err = (t[fin].double() - ref).abs()
            worst[name] = max(worst[name], float((err / bound).max()))
            if bool(outside_tail.any()):
                worst_ulp[name] = max(worst_ulp[name], float((err / ulp)[outside_tail].max()))
        del x, got, yard, fin, xf, ref, ulp, bound, outside_tail, err
    print("FP64 gelu {}: max err / bound kernel {:.3g} torch {:.3g}; max ulp for x >= -1 kernel {:.3g} torch {:.3g}".format(
        which, worst["kernel"], worst["torch"], worst_ulp["kernel"], worst_ulp["torch"]))
    assert worst["torch"] <= 1.0, worst                       # the bound is a property of fp32 GELU ...
    assert worst["kernel"] <= 1.0, worst                      # ... and the kernel meets it on every input


# ------------------------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("trans", [True, False])
@pytest.mark.parametrize("pa,pb", ts.PRODUCTS)
def test_gemm_exact_operands_bit_for_bit(pa, pb, trans):
    """Operands whose every product and partial sum is exact in fp32 (checked on the CPU in test_trained_stats.py): the
    kernel's result equals the float64 product exactly, whatever its summation order.  A wrong plane, k position or
    product selection changes it."""
    from vqattack_amd import ops
    m, n, k = 300, 384, 256                                   # ragged M (two row tiles), 3 N tiles, 8 k-steps
    a, b, _, _ = ts.exact_operands(pa, pb, m, n, k)
    a, b = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    w = b.t().contiguous() if trans else b                    # trans=True packs w^T of a Linear weight w [N, K]
    out = ops.gemm(a, ops.gemm_pack(w, trans=trans))
    ref = a.double() @ b.double()
    assert torch.equal(out.double(), ref), float((out.double() - ref).abs().max())


def _rows(make, m, k, seed, distinct=4096):
    """(m, k) rows: ``distinct`` CPU-generated rows repeated (the shapes' row counts are ~37 k)."""
    block = make(distinct, k, _cpu_gen(seed)).to(DEV)
    return block.repeat(-(-m // distinct), 1)[:m].contiguous()


@pytest.mark.parametrize("trans", [True, False])
@pytest.mark.parametrize("m,n_out,k_in", [(37824, 2304, 768), (37824, 768, 3072)])
def test_gemm_trained_statistics_against_fp64(m, n_out, k_in, trans):
    """The forward operand (trans=True: LN output x W^T for the QKV projection, GELU output x W^T for FC2) and the
    input-gradient operand (trans=False: dC x W) of the same trained-statistics weight W [n_out, k_in]."""
    from vqattack_amd import ops
    w = ts.trained_weight(n_out, k_in, _cpu_gen(n_out + k_in)).to(DEV)
    if trans:
        a = _rows(ts.post_ln if k_in == 768 else ts.post_gelu, m, k_in, 1)
        wb = w.t()
    else:
        a = _rows(ts.post_ln, m, n_out, 2) * 1e-3                # an output gradient: LN-like spread and outliers
        wb = w
    out = torch.full((m, wb.shape[1]), float("nan"), device=DEV)
    ops.gemm(a, ops.gemm_pack(w, trans=trans), out=out)
    assert bool(torch.isfinite(out).all()), "an output element was not written"
    lib = torch.mm(a, wb)
    ref = a.double() @ wb.double()
    ek, el = (out.double() - ref).abs(), (lib.double() - ref).abs()
    print("FP64 gemm {}x{}x{} trans={}: kernel/library max {:.3g}/{:.3g} rms {:.3g}/{:.3g}".format(
        m, wb.shape[1], a.shape[1], trans, float(ek.max()), float(el.max()), float(ek.pow(2).mean().sqrt()),
        float(el.pow(2).mean().sqrt())))
    assert float(ek.max()) <= 2.0 * float(el.max())
    assert float(ek.pow(2).mean().sqrt()) <= 2.0 * float(el.pow(2).mean().sqrt())
    bound = (a.shape[1] * U + 4 * U) * (a.double().abs() @ wb.double().abs())
    assert bool((ek <= bound).all()), float((ek / bound).max())
