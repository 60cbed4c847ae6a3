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


# ------------------------------------------------------------------------------------------------ feature-loss pairs
# Inside an attack the two operands of the cosine loss are the adversarial and the clean feature map of ONE model:
# a = b + small.  The gradient  kb b + ka a  is then the difference of two nearly equal vectors.
COS_EPS = 1e-6                                     # nn.CosineSimilarity(eps=1e-6), ops._COS_EPS
PAIR_KINDS = ("plain", "outliers", "scaled")
DELTAS = (0.0, 1e-5, 1e-3, 1e-1, 1.0)
TINY_NORM, ABOVE_NORM = 1e-7, 3e-6                 # row norms below / just above COS_EPS
# flat row indices of the ``degenerate`` kind (needs >= 13 rows)
DEGENERATE_ROWS = dict(a_zero=(0, 1), b_zero=(2, 3), both_zero=(4,), a_tiny=(5, 6), b_tiny=(7, 8), a_above=(9, 10),
                       b_above=(11, 12))


def feature_pair(kind, delta, rows0, rows1, d, seed=0):
    """(a, b) fp32 (rows0, rows1, D) on the CPU.  ``b``: unit Gaussian; ``outliers``: two channels at x300 (massive
    activations); ``scaled``: the outlier rows times a per-row scale drawn log-uniformly from 1e-3 .. 1e3.
    ``a = fp32(b64 + delta * n)`` with n Gaussian of the row's own rms, so |a - b| / |b| ~ delta; delta = 0: a is b, bit
    for bit.  ``degenerate``: plain rows, the first 13 replaced per DEGENERATE_ROWS (exact zeros, norms 1e-7 and 3e-6)."""
    g = torch.Generator().manual_seed(seed * 1000 + d)
    b = torch.randn(rows0, rows1, d, generator=g)
    n = torch.randn(rows0, rows1, d, generator=g)
    scale = torch.exp(torch.empty(rows0, rows1, 1).uniform_(math.log(1e-3), math.log(1e3), generator=g))
    if kind in ("outliers", "scaled"):
        b[..., [7, d // 2 + 3]] *= 300.0
    if kind == "scaled":
        b = b * scale
    elif kind not in ("plain", "outliers", "degenerate"):
        raise ValueError(kind)
    b64 = b.double()
    if delta == 0.0:
        a = b.clone()
    else:
        rms = b64.norm(dim=-1, keepdim=True) / math.sqrt(d)
        a = (b64 + delta * rms * n.double()).float()
    if kind == "degenerate":
        af, bf = a.view(-1, d), b.view(-1, d)
        for name, rows in DEGENERATE_ROWS.items():
            for r in rows:
                for t, tag in ((af, "a"), (bf, "b")):
                    if name.startswith(tag) or name == "both_zero":
                        if name.endswith("zero"):
                            t[r] = 0.0
                        else:
                            want = TINY_NORM if name.endswith("tiny") else ABOVE_NORM
                            t[r] = (t[r].double() * (want / t[r].double().norm())).float()
    return a, b


def neg_cos64(a, b, w=None, eps=COS_EPS):
    """The header's formula in the dtype of ``a`` (pass float64): per-row -c = -(a / max(|a|, eps)) . (b / max(|b|, eps))
    and d(-c)/da = -( b / (dna dnb) - [|a| > eps] c a / |a|^2 ) (nothing flows through a clamped norm), times the row
    weight ``w``.  Returns (row values, gradient)."""
    na, nb = a.norm(dim=-1, keepdim=True), b.norm(dim=-1, keepdim=True)
    inv = 1.0 / (na.clamp_min(eps) * nb.clamp_min(eps))
    c = (a * b).sum(-1, keepdim=True) * inv
    ka = torch.where(na > eps, c / (na * na).clamp_min(1e-300), torch.zeros_like(c))
    grad = -(b * inv - ka * a)
    val = -c.squeeze(-1)
    if w is not None:
        val, grad = val * w, grad * w.unsqueeze(-1)
    return val, grad


# ---------------------------------------------------------------------------------------------------- MLM logits
# A trained MLM head predicts the masked answer piece with p ~ 1: the row's loss is 1e-2 .. 1e-7.
MARGINS = (0.0, 5.0, 10.0, 15.0, 20.0, 30.0)
MLM_KINDS = {"off0": 0.0, "off+50": 50.0, "off-50": -50.0, "masked": 0.0}
IGNORE = -100
MASKED_HEAD = 1024                                 # leading entries of a ``masked`` row that are all -inf
CE_BLOCK = 256                                     # threads of the streaming fallback (csrc/ce.hip, kBlock)


def live_rows(rows):
    """Every third row is live (>= 2/3 dead); consecutive live rows alternate parity."""
    return list(range(1, rows, 3))


def forced_position(j, v):
    """Label position of the j-th live row: 0 / 1 on odd rows and V-1 / V-2 on even rows (the register kernel's head and
    tail lanes at V = 30522), the row's argmax (None), a random one (-1)."""
    return (0, v - 1, 1, v - 2, None, -1)[j % 6]


def margin_index(j, seed):
    return (j + j // 6 + seed) % len(MARGINS)


def row_geom(r, v):
    """``row_geom`` of csrc/ce.hip: (head, nquad, tail0); lanes t < head own x[t], lanes 8 + t own x[tail0 + t]."""
    head = (4 - (r * v) % 4) % 4
    nquad = (v - head) // 4
    return head, nquad, head + 4 * nquad


def mlm_logits(kind, rows, v, k, seed=0):
    """(logits fp32 (rows, V), labels int64 (K, rows), margin index per row (-1 dead)) on the CPU.  ``2 randn + offset``;
    label set 0 of the j-th live row sits at ``forced_position`` and is lifted to row max + MARGINS[margin_index];
    sets 1 .. K-1 are live on every fourth live row at random positions, and on the second live row set 1 repeats set 0's
    label.  ``masked``: a random 30 % of each row and its first MASKED_HEAD entries are -inf, the labels are not."""
    g = torch.Generator().manual_seed(seed * 7919 + v + 31 * k + list(MLM_KINDS).index(kind))
    x = 2.0 * torch.randn(rows, v, generator=g) + MLM_KINDS[kind]
    labels = torch.full((k, rows), IGNORE, dtype=torch.int64)
    margin = torch.full((rows,), -1, dtype=torch.int64)
    if kind == "masked":
        x[torch.rand(rows, v, generator=g) < 0.3] = float("-inf")
        x[:, :MASKED_HEAD] = float("-inf")
    for j, r in enumerate(live_rows(rows)):
        pos = forced_position(j, v)
        if pos is None:
            pos = int(x[r].argmax())
        elif pos < 0:
            pos = int(torch.randint(2, v - 2, (1,), generator=g))
        margin[r] = margin_index(j, seed)
        x[r, pos] = float(x[r].max()) + MARGINS[int(margin[r])]
        labels[0, r] = pos
        for kk in range(1, k):
            if (j + kk) % 4 == 0:
                other = int(torch.randint(MASKED_HEAD, v, (1,), generator=g))
                if kind == "masked" and not math.isfinite(float(x[r, other])):
                    x[r, other] = MLM_KINDS[kind]
                labels[kk, r] = other
    if k > 1 and len(live_rows(rows)) > 1:
        r = live_rows(rows)[1]
        labels[1, r] = labels[0, r]
    return x, labels, margin


def ce_weights(labels, rows_per_sample, dtype):
    """w[k, r] = 1 / #{valid labels of set k in r's group} on live entries, 0 elsewhere (``vqa_ce_rows``'s mean)."""
    k, rows = labels.shape
    rpg = rows if rows_per_sample in (0, None) else rows_per_sample
    groups = -(-rows // rpg)
    valid = (labels != IGNORE)
    pad = groups * rpg - rows
    vp = torch.nn.functional.pad(valid, (0, pad)).view(k, groups, rpg)
    count = vp.sum(-1, keepdim=True).expand(k, groups, rpg).reshape(k, groups * rpg)[:, :rows].to(dtype)
    return torch.where(valid, 1.0 / count.clamp_min(1.0), torch.zeros((), dtype=dtype, device=labels.device))


def ce_rows_torch(logits, labels, rows_per_sample):
    """(row losses, gradient) of sum_k mean-CE in the dtype of ``logits`` through torch's own cross_entropy + autograd."""
    x = logits.clone().requires_grad_(True)
    w = ce_weights(labels, rows_per_sample, logits.dtype)
    per = torch.stack([torch.nn.functional.cross_entropy(x, lab, ignore_index=IGNORE, reduction="none") for lab in labels])
    row = (per * w).sum(0)
    (grad,) = torch.autograd.grad(row.sum(), x)
    return row.detach(), grad


# --------------------------------------------------------------------------------------------------- text tables
SYN_STEP = 1e-3                                    # near-synonym: word[j] = word[i] + SYN_STEP * randn
TEXT_SAMPLES, TEXT_POSITIONS, TEXT_CANDS = 3, 4, 48
TEXT_LEN = 12


def text_tables(d, v=600, seed=0):
    """BERT-like embedding tables on the CPU: word rows 0.05 randn with two channels at x20, ids [v/2, v) near-synonyms of
    ids [0, v/2) (word[i + v/2] = word[i] + 1e-3 randn), gamma with one x8 entry; ``grad`` rows (TEXT_SAMPLES, TEXT_LEN, D)
    at 1e-7 with a heavy tail."""
    g = torch.Generator().manual_seed(seed * 13 + d)
    half = v // 2
    word = torch.randn(v, d, generator=g) * 0.05
    word[:, [5, d // 3]] *= 20.0
    word[half:] = (word[:half].double() + SYN_STEP * torch.randn(half, d, generator=g).double()).float()
    pos = torch.randn(TEXT_LEN, d, generator=g) * 0.02
    type_emb = torch.randn(2, d, generator=g) * 0.01
    gamma = 1.0 + 0.3 * torch.randn(d, generator=g)
    gamma[11] = 8.0
    beta = 0.3 * torch.randn(d, generator=g)
    grad = 1e-7 * torch.randn(TEXT_SAMPLES, TEXT_LEN, d, generator=g) * torch.exp(
        torch.randn(TEXT_SAMPLES, TEXT_LEN, d, generator=g))
    return dict(word=word, pos=pos, type_emb=type_emb, gamma=gamma, beta=beta, ln_eps=1e-12, grad=grad)


def text_candidates(tabs, seed=0):
    """(ori ids (S, L) int64, cand int32 (n, 4), synonym flag (n,)): TEXT_POSITIONS positions per sample with TEXT_CANDS
    candidates each; the first is a near-synonym of the original word, the next two of each other.  Every other candidate
    reads a gradient row that is NOT its position (the kernel takes both from the row: columns 1 and 2)."""
    v = tabs["word"].shape[0]
    half = v // 2
    g = torch.Generator().manual_seed(seed + 77)
    ori = torch.randint(1, half, (TEXT_SAMPLES, TEXT_LEN), generator=g)
    rows, syn = [], []
    for s in range(TEXT_SAMPLES):
        for p in (1, 3, 6, 10)[:TEXT_POSITIONS]:
            o = int(ori[s, p])
            other = int(torch.randint(1, half, (1,), generator=g))
            ids = [o + half, other, other + half] + [int(t) for t in torch.randperm(v - 1, generator=g)[:TEXT_CANDS] + 1]
            ids = [t for i, t in enumerate(ids) if t != o and t not in ids[:i]][:TEXT_CANDS]
            for i, t in enumerate(ids):
                rows.append((s, p, (p + 1 + i % 3) % TEXT_LEN if i % 2 else p, t))
                syn.append(i == 0)
    return ori, torch.tensor(rows, dtype=torch.int32), torch.tensor(syn)


def bert_embed(tabs, ids, positions, dtype):
    """LayerNorm(word[id] + type[0] + pos[p]) in ``dtype`` (tables may live on any device)."""
    e = (tabs["word"][ids].to(dtype) + tabs["type_emb"][0].to(dtype)) + tabs["pos"][positions].to(dtype)
    return torch.nn.functional.layer_norm(e, e.shape[-1:], tabs["gamma"].to(dtype), tabs["beta"].to(dtype),
                                          tabs["ln_eps"])


def dir_sim(tabs, e_ori, cand, dtype):
    """The header's formula of ``vqa_cand_dir_sim`` in ``dtype`` with the GIVEN fp32 ``e_ori``: scores (n,) and |d| / |e|."""
    s, p, k, v = (cand[:, i].long() for i in range(4))
    e = bert_embed(tabs, v, p, dtype)
    dvec = e - e_ori[s, p].to(dtype)
    gvec = tabs["grad"][s, k].to(dtype)
    nd, ng = dvec.norm(dim=-1, keepdim=True), gvec.norm(dim=-1, keepdim=True)
    u, w = dvec / nd.clamp_min(1e-12), gvec / ng.clamp_min(1e-12)
    score = (u * w).sum(-1) / (u.norm(dim=-1).clamp_min(1e-6) * w.norm(dim=-1).clamp_min(1e-6))
    return score, (nd.squeeze(-1) / e.norm(dim=-1))


def left_out_pairs(s64, gap, per_group):
    """Share of candidate pairs (within each group of ``per_group`` consecutive scores) closer than ``gap``, and the mask
    (groups, n, n) of the pairs that remain."""
    sc = s64.view(-1, per_group)
    diff = (sc[:, :, None] - sc[:, None, :]).abs()
    upper = torch.triu(torch.ones(per_group, per_group, dtype=torch.bool, device=s64.device), 1)[None]
    decided = (diff > gap) & upper
    return 1.0 - float(decided.sum()) / float(upper.sum() * sc.shape[0]), decided


# ------------------------------------------------------------------------------------------------ greedy acceptance
GREEDY_B, GREEDY_L, GREEDY_V = 64, 24, 2000
GREEDY_THRESHOLDS = (0.95, 0.8, 0.5)
GREEDY_MARGIN = 1e-5
CLOSE_STEP = 0.1                                   # sample 0: candidates are table rows 0.1 randn away from the original


def greedy_case(e, seed=0):
    """dict(table (V, E) fp32, ori (B, L) int64 with padding, cand int32 (n, 4), scores fp32 (n,)) on the CPU.  Five
    positions x three candidates per sample.  Sample 0's candidates are near-synonyms (CLOSE_STEP) of its own words: the
    first one is accepted, the threshold rises to ~1 - 1e-4, and the later ones miss it by 1e-5 .. 1e-3.  Samples 1 .. 8
    carry a candidate that proposes the word already there, visited after an acceptance: an exact tie with the risen
    threshold, which `>` rejects."""
    g = torch.Generator().manual_seed(seed * 17 + e)
    table = torch.randn(GREEDY_V, e, generator=g)
    ori = torch.randint(1, GREEDY_V // 2, (GREEDY_B, GREEDY_L), generator=g)
    for s in range(GREEDY_B):
        ori[s, 10 + s % 14:] = 0                                 # 10 .. 23 tokens, padded with id 0
    rows, scores = [], []
    for s in range(GREEDY_B):
        n_tok = 10 + s % 14
        positions = torch.randperm(n_tok, generator=g)[:5].tolist()
        for i, p in enumerate(positions):
            for c in range(3):
                rows.append((s, p, p, int(torch.randint(GREEDY_V // 2, GREEDY_V, (1,), generator=g))))
                scores.append(float(torch.rand(1, generator=g)) * 0.5)
        if 1 <= s <= 8:                                           # the no-op candidate: lowest score, visited last
            free = [p for p in range(n_tok) if p not in positions][0]
            rows.append((s, free, free, int(ori[s, free])))
            scores.append(-1.0)
    # sample 0: five near-synonym candidates, best score first
    rows0 = [i for i, r in enumerate(rows) if r[0] == 0]
    for n, i in enumerate(rows0):
        p = rows[i][1]
        syn = GREEDY_V - 1 - n
        table[syn] = (table[int(ori[0, p])].double() + CLOSE_STEP * torch.randn(e, generator=g).double()).float()
        rows[i] = (0, p, p, syn)
        scores[i] = 1.0 - 0.01 * n
    return dict(table=table, ori=ori, cand=torch.tensor(rows, dtype=torch.int32), scores=torch.tensor(scores))


def greedy_accept64(case, threshold):
    """The loop of ``attack/text_update.py::greedy_accept`` with the bag-of-embeddings similarity in float64.  Returns
    (new_id (B, L), rank (B, L), smallest |sim - threshold at that moment| per sample, per sample the margins of the
    comparisons made AFTER the threshold had risen).  A candidate that proposes the word already in place after an
    acceptance reproduces the risen threshold by construction (same ids, same arithmetic): an exact tie, rejected by
    `>`, which no rounding can move -- it records no margin."""
    table = case["table"].double().numpy()
    ori_all, cand, scores = case["ori"].numpy(), case["cand"].numpy(), case["scores"].numpy()
    b, length = ori_all.shape
    new_id = np.full((b, length), -1, dtype=np.int64)
    rank = np.full((b, length), -1, dtype=np.int64)
    smallest = np.full(b, np.inf)
    risen = [[] for _ in range(b)]

    def mean(ids):
        return table[[t for t in ids if t != 0]].mean(0)

    for s in range(b):
        mine = np.nonzero(cand[:, 0] == s)[0]
        order = sorted(mine, key=lambda i: scores[i], reverse=True)
        cur = ori_all[s].copy()
        mo = mean(ori_all[s])
        thr, taken = threshold, set()
        for i in order:
            p, v = int(cand[i, 1]), int(cand[i, 3])
            if p in taken:
                continue
            if v == cur[p] and taken:
                continue                                          # exact tie with the risen threshold
            trial = cur.copy()
            trial[p] = v
            mt = mean(trial)
            sim = float(mo @ mt / (np.linalg.norm(mo) * np.linalg.norm(mt) + 1e-12))
            smallest[s] = min(smallest[s], abs(sim - thr))
            if taken:
                risen[s].append(abs(sim - thr))
            if sim > thr:
                thr = sim
                new_id[s, p], rank[s, p] = v, len(taken)
                taken.add(p)
                cur = trial
    return new_id, rank, smallest, risen


# --------------------------------------------------------------------------------------------------- image gradients
def image_grads(shape, seed=0):
    """Image gradients of the feature loss: ``1e-6 randn exp(randn)`` (heavy-tailed, 1e-5 .. 1e-8) with 1 % exact zeros."""
    g = torch.Generator().manual_seed(seed + 5)
    x = 1e-6 * torch.randn(shape, generator=g) * torch.exp(torch.randn(shape, generator=g))
    x[torch.rand(shape, generator=g) < 0.01] = 0.0
    return x
