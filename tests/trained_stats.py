"""Seeded inputs with the statistics of trained ALBEF / VLMo checkpoints, for the fp64-referenced kernel tests.

The encoders' unit tests feed their kernels unit-variance Gaussians.  Trained weights make peaked attention (hot queries,
position ramps, "sink" keys), masked leading key blocks, LayerNorm rows with large offsets or almost no spread, outlier
channels, and heavy-tailed GEMM operands.  Every tensor here is drawn on the CPU from a ``torch.Generator`` and only then
moved to a device, so a case is the same bits on every machine; ``tests/test_trained_stats.py`` checks on the CPU that the
cases reach the kernel branches they are meant for, ``test_attention_fp64.py`` / ``test_block_fp64.py`` run them.
"""
import math
import os
import re

import numpy as np
import torch

HEAD = 64
TILE = 32                                          # key tile of csrc/attn.hip: the forward's max walks tile by tile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lazy_max():
    """``kLazyMax`` of csrc/attn.hip: the forward rescales its running max only when a tile's max exceeds it by more."""
    with open(os.path.join(ROOT, "vqattack_amd", "csrc", "attn.hip")) as fh:
        m = re.search(r"constexpr\s+float\s+kLazyMax\s*=\s*([0-9.]+)f?\s*;", fh.read())
    return float(m.group(1))


def part_bounds(tiles, n):
    """Key-tile boundaries of the forward's loop split: part p owns tiles [p * tiles / n, (p + 1) * tiles / n)."""
    return [p * tiles // n for p in range(n + 1)]


# ------------------------------------------------------------------------------------------------------- attention
RAMP = 40.0            # total rise of a key ramp over the sequence (position-biased heads)
SINK = 30.0            # extra logit of one key in the last, partial key tile
LEAD = 64              # masked leading keys: two whole key tiles
BERT_MASK = -10000.0   # BERT's finite additive padding mask
SPLIT_MASKED = 192     # split case: keys [0, 192) masked, [192, 384) pushed far below the row max
SPLIT_LOW = -150.0

# kinds whose rows must rise far above their first tile's max (the lazy rescale fires), and the controls
RESCALE_KINDS = ("ramp", "sink", "lead_inf", "lead_bert", "split")
KINDS = ("plain", "ramp", "ramp_rev", "sink", "lead_inf", "lead_bert", "split")


def sink_key(sk):
    """A key inside the last key tile, which is partial at the suite's lengths (591, 901)."""
    return sk - 3


def attn_bias(kind, h, sq, sk, g):
    """Additive bias (1, H, Sq, Sk) of a case, rows padded to whole key tiles in storage (the kernels' contract: from
    every row start ceil32(Sk) floats are readable), on the CPU."""
    pad = (sk + TILE - 1) // TILE * TILE
    store = torch.zeros(1, h, sq, pad)
    bias = store[..., :sk]
    bias += torch.randn(1, h, sq, sk, generator=g) * 0.5
    head_gain = torch.linspace(0.9, 1.1, h).view(1, h, 1, 1)
    ramp = torch.linspace(0.0, RAMP, sk).view(1, 1, 1, sk) * head_gain
    if kind in ("ramp", "lead_inf", "lead_bert", "split"):
        bias += ramp
    elif kind == "ramp_rev":
        bias += ramp.flip(-1)
    elif kind == "sink":
        bias[..., sink_key(sk)] += SINK
    elif kind != "plain":
        raise ValueError(kind)
    if kind == "lead_inf":
        bias[..., :LEAD] = float("-inf")
    elif kind == "lead_bert":
        bias[..., :LEAD] = BERT_MASK
    elif kind == "split":
        bias[..., :SPLIT_MASKED] = float("-inf")
        bias[..., SPLIT_MASKED:2 * SPLIT_MASKED] = SPLIT_LOW
    return bias


def attn_case(kind, b, h, sq, sk, tau=1.0, seed=0, packed=False):
    """CPU tensors of one attention case: dict(q, k, v (B, S, H, 64), bias (1, H, Sq, Sk), go, qkv when ``packed``).
    ``tau`` multiplies q (a trained query projection's temperature); ``packed``: q, k, v are the slices of ONE
    (B, S, 3, H, 64) projection output, as in the encoders' self-attention."""
    g = torch.Generator().manual_seed(seed * 1000 + KINDS.index(kind) * 10 + int(tau))
    out = {}
    if packed:
        assert sq == sk
        qkv = torch.randn(b, sq, 3, h, HEAD, generator=g)
        qkv[:, :, 0] *= tau
        out["qkv"] = qkv
        q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    else:
        q = torch.randn(b, sq, h, HEAD, generator=g) * tau
        k = torch.randn(b, sk, h, HEAD, generator=g)
        v = torch.randn(b, sk, h, HEAD, generator=g)
    out.update(q=q, k=k, v=v, bias=attn_bias(kind, h, sq, sk, g), go=torch.randn(b, sq, h, HEAD, generator=g))
    return out


def dense_hole(hole, sk):
    """(B, 1, 1, Sk) additive -inf mask of ``KeyHoleBias`` holes [lo, hi) (int (B, 2)), on the CPU."""
    keys = torch.arange(sk)
    hole = torch.as_tensor(hole)
    masked = (keys[None, :] >= hole[:, :1]) & (keys[None, :] < hole[:, 1:2])
    return torch.zeros(hole.shape[0], 1, 1, sk).masked_fill(masked[:, None, None, :], float("-inf"))


def scores64(case, scale=HEAD ** -0.5, extra=None):
    """scale * q k^T + bias in float64 on the CPU, (B, H, Sq, Sk); ``extra``: a further additive mask (e.g. a hole)."""
    s = torch.einsum("bqhd,bkhd->bhqk", case["q"].double(), case["k"].double()) * scale + case["bias"].double()
    return s if extra is None else s + extra.double()


def tile_maxima(s):
    """Per row, the max of every 32-key tile: (..., Sq, tiles), -inf for a tile whose keys are all masked."""
    sk = s.shape[-1]
    tiles = (sk + TILE - 1) // TILE
    padded = torch.full(s.shape[:-1] + (tiles * TILE,), float("-inf"), dtype=s.dtype)
    padded[..., :sk] = s
    return padded.view(s.shape[:-1] + (tiles, TILE)).amax(-1)


def rise_over_first_tile(s):
    """Per row: how far the row max lies above the max of the first key tile that holds an unmasked key -- where the
    kernel's tile walk fixes its first running max."""
    tm = tile_maxima(s)
    finite = torch.isfinite(tm)
    first = finite.float().argmax(-1, keepdim=True)
    return tm.amax(-1) - tm.gather(-1, first).squeeze(-1)


# ------------------------------------------------------------------------------------------------------- LayerNorm
LN_KINDS = ("offset1e2", "offset1e3", "outliers", "constant", "near_constant")
CONSTANTS = (0.1, -2.5, 1000.3, 3.0e-3, 7.0, -0.37)


def ln_rows(kind, rows, d, seed=0):
    """(rows, D) fp32 LayerNorm inputs on the CPU.  ``offset1e2`` / ``offset1e3``: a per-row offset of 1e2 / 1e3 times
    the row's spread (unit std); ``outliers``: two channels at x300 (trained residual streams' massive activations);
    ``constant``: every row one value; ``near_constant``: c + 1e-7 * randn (a handful of fp32 steps of spread)."""
    g = torch.Generator().manual_seed(seed * 100 + LN_KINDS.index(kind) + d)
    x = torch.randn(rows, d, generator=g)
    sign = torch.where(torch.rand(rows, 1, generator=g) < 0.5, -1.0, 1.0)
    c = torch.tensor(CONSTANTS).repeat(rows // len(CONSTANTS) + 1)[:rows].view(rows, 1)
    if kind == "offset1e2":
        return x + 1e2 * sign
    if kind == "offset1e3":
        return x + 1e3 * sign
    if kind == "outliers":
        x[:, [7, d // 2 + 3]] *= 300.0
        return x
    if kind == "constant":
        return c.expand(rows, d).contiguous()
    if kind == "near_constant":
        return (c.double() + 1e-7 * x.double()).float()
    raise ValueError(kind)


# ------------------------------------------------------------------------------------------------------------ GEMM
def post_gelu(m, k, g):
    """Activations after GELU: mostly positive, a floor at -0.17, heavy right tail (a few x30 entries)."""
    x = torch.randn(m, k, generator=g) * 1.5
    x = 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    hot = torch.rand(m, k, generator=g) < 1e-3
    return torch.where(hot, x.abs() * 30.0 + 5.0, x)


def post_ln(m, k, g):
    """LayerNorm outputs: unit spread around a beta offset of about 0.3, two channels at x50."""
    x = torch.randn(m, k, generator=g) * (1.0 + 0.2 * torch.randn(k, generator=g)) + 0.3
    x[:, [11, k // 3]] *= 50.0
    return x


def trained_weight(out_f, in_f, g):
    """A Linear weight [out, in]: 0.02 spread with a few entries 100x larger."""
    w = torch.randn(out_f, in_f, generator=g) * 0.02
    hot = torch.rand(out_f, in_f, generator=g) < 2e-4
    return torch.where(hot, w * 100.0, w)


# Exact-arithmetic GEMM operands: one variant per (A-plane, B-plane) product of the bf16x6 kernel.  A value with planes
# {0 .. p} is  sum_i s_i 1.5 2^(-9 i)  with random signs s_i: each piece is a bf16 value below half a bf16 step of the
# piece before it, so the split returns exactly these pieces.  A row of A holds NNZ = 3 nonzeros at random k.  Every
# product of two pieces is a multiple of 2^-20, and the sum of the magnitudes of a row's products is below
# 3 * 1.5^2 * (1 + 2^-8)^2 < 2^3: every product, every partial sum and the result are exact in fp32 in any summation
# order, so the kernel's result must equal the fp64 product bit for bit.
PRODUCTS = ((0, 0), (1, 0), (0, 1), (2, 0), (1, 1), (0, 2))      # the six products the kernel sums
EXACT_NNZ = 3


def _planes_value(shape, top, rng):
    """float64 values with nonzero planes 0 .. top (top = -1: zeros), and the planes themselves (3, *shape)."""
    planes = np.zeros((3,) + tuple(shape))
    for i in range(top + 1):
        planes[i] = rng.choice([-1.5, 1.5], size=shape) * 2.0 ** (-9 * i)
    return planes.sum(0), planes


def exact_operands(pa, pb, m, n, k, seed=0):
    """(a (M, K), b (K, N), a planes, b planes) numpy float32 / float64 for product (pa, pb): A carries planes
    0 .. pa, B planes 0 .. pb (so every product the kernel drops, a1b2 / a2b1 / a2b2, is zero)."""
    rng = np.random.default_rng(seed * 10 + 3 * pa + pb)
    a_val, a_planes = _planes_value((m, k), pa, rng)
    keep = np.zeros((m, k), dtype=bool)
    for r in range(m):
        keep[r, rng.choice(k, size=EXACT_NNZ, replace=False)] = True
    a_val = np.where(keep, a_val, 0.0)
    a_planes = np.where(keep[None], a_planes, 0.0)
    b_val, b_planes = _planes_value((k, n), pb, rng)
    return a_val.astype(np.float32), b_val.astype(np.float32), a_planes, b_planes
