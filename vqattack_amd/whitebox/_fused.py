"""Transformer encoders of the frozen white boxes (pre-LN: VLMo, ALBEF's ViT; post-LN: ALBEF's BERT fusion encoder, second
half of this file) WITHOUT an autograd graph inside: library GEMMs, the hand-written
attention (``csrc/attn.hip``) and the fused block glue of ``csrc/block.hip`` -- forward and input-gradient backward written
out stage by stage.

Reference computation: ``Block.forward`` of ``VLMO_VQAttack/vlmo/modules/multiway_transformer.py:184-201`` (shared
attention, modality-expert FFNs split at the text length, layer scale ``gamma_1`` / ``gamma_2``) and ALBEF's ViT block
(``ALBEF_attack/models/vit.py``; no layer scale, one FFN).  Weights are frozen, so the backward produces the INPUT gradient
only: two GEMMs per linear layer disappear against a training backward, and nothing but the layer inputs, the packed
``qkv``, the attention statistics and the pre-GELU activations is kept from the forward.

Why not autograd: eager execution runs every residual add, layer-scale multiply, LayerNorm, slice, ``cat`` and
gradient-accumulation add as its own full pass over the (B, S, D) residual stream (10.8 % of the attack's device time in
round 3).  Here a stage boundary is ONE kernel: ``vqa_ln_fwd`` = residual add of the previous branch + LayerNorm (+ the
text / image split the expert GEMMs need), ``vqa_ln_bwd`` = LayerNorm backward + the gradient of the residual path + the
loss kernel's gradient of that feature map (+ the layer-scaled branch gradient).  The whole encoder is one
``torch.autograd.Function`` whose outputs are the per-layer feature maps and the final normalised states, so callers
(the ``model_fn`` closures, the loss kernels' ``torch.autograd.backward(outputs, grads)``) see ordinary tensors.
"""
import os

import torch

from .. import attention as _attn
from .. import ops

# Encoder GEMMs run on the bf16x6 kernel (csrc/gemm.hip: fp32-grade products on the bf16 matrix pipe) where it covers
# the shape and its grid has at least MIN_WORKGROUPS workgroups (one 256 x 128 output tile each, one per CU at a time);
# below that it cannot fill the 256 CUs and the library fp32 GEMM is faster.  Measured per shape (tools/gemm_bench.py,
# VLMO-base): 1.21-1.41x at 888-2664 workgroups and at the text expert's 240 (2560 x 3072), 0.45x at its 60
# (2560 x 768).  VQA_GEMM=library restores the library everywhere.
MIN_WORKGROUPS = 192

# Below MIN_WORKGROUPS the small-tile kernel (64 x 128 tiles, deterministic split-K: ops.gemm_small with the split of
# ops.gemm_small_plan) takes the shape classes it was MEASURED to win: (N, K) -> (fewest rows, most rows), both
# inclusive.  An entry is there only where the small kernel's median time beat the library's by more than the
# round-to-round spread of either variant in the same record, at every measured row count of the range
# (profiles/r08/README.md, tools/gemm_bench.py --batch); everything else stays on the library.
# Recorded: at 551-591 rows (batch 1) every shape loses (0.77-0.92x of the library, call times of 20-35 us); the text
# expert's 2560 x 768 x 3072 passes the margin in one of its two records only (1.10x).  At 1102-1182 rows (VLMO-base,
# batch 2) the N = 3072, K = 768 GEMMs win 1.34-1.49x unsplit, but the end-to-end comparison with that entry was not
# taken, so it is not dispatched: the policy is empty and the unset VQA_GEMM behaves as "large".
SMALL_POLICY = {}

# From MIN_WORKGROUPS up, ops.gemm runs one of two output tiles with the same bits: 256 x 128, or 128 x 256 ("wide":
# half the in-loop split work per product, N % 256 == 0).  A shape class (N, K) -> (fewest rows, most rows), both
# inclusive, is listed here only by the rule of SMALL_POLICY: the wide tile's median in tools/gemm_bench.py beat the
# 256 x 128 tile's by more than the round-to-round spread of either in the same record (profiles/r10/README.md), and
# the benchmark with the entries in place beat the one without.  VQA_GEMM=large / VQA_GEMM=wide force one tile everywhere.
# Recorded at 35264 and 37824 rows (VLMO-base, batch 64; (768, 768) at 37824 only): 1.07-1.10x.  The range spans the two
# measured row counts; the benchmark's own row counts (text trimmed to its longest question) lie between them.  Not
# listed: the qkv classes (2304, 768) and (768, 2304) -- 1.08-1.10x at the median in both gemm_bench records, but the
# 256 x 128 kernel's own max - min (0.07-0.09 ms) exceeds the margin (0.06-0.07 ms), so they fail the rule; the text
# expert's 2560 x 3072 x 768 (240 workgroups; one of its two shapes fails the margin); ALBEF-base's 147712 rows (not
# measured).  Re-taken with packed B staged straight into LDS in both tiles (profiles/r12/README.md, two records):
# the listed classes 1.07-1.12x, margins 1.4-4.3 times the larger spread; (768, 2304) fails again in both records
# (margin 0.05-0.06 ms against the 256 x 128 kernel's max - min of 0.07-0.08 ms) and (2304, 768) passes by 0.0001 ms
# in one of them, so the qkv classes stay unlisted (the benchmark with both listed read 16.51-16.54 examples/s against
# 16.32-16.34 without).
_WIDE_ROWS = (35264, 37824)
WIDE_POLICY = {(768, 768): _WIDE_ROWS, (3072, 768): _WIDE_ROWS, (768, 3072): _WIDE_ROWS}

# The FFN's GELU (forward) and the product with its derivative (backward) can run in the epilogue of the GEMM that
# produces their input (ops.gemm(..., epilogue=): vqa_gemm_bf16x6_epi, the bits of the two-step form), which saves one
# pass over the (rows, 4D) pre-activation per direction.  Whether that is faster is a measurement, not a given: the tiles
# run one workgroup per CU, so the epilogue's erf arithmetic is not hidden behind another workgroup's MFMAs.  Per
# epilogue, a shape class (N, K) -> (fewest rows, most rows), both inclusive, is listed only by the rule of WIDE_POLICY:
# the fused call's median in tools/gemm_bench.py beat the median of GEMM + GELU kernel by more than the round-to-round
# spread of either in BOTH records of the shape (profiles/r11/README.md), and the benchmark with the entries in place
# beat the one without.  Listed shapes are fused wherever the 256 x 128 or 128 x 256 kernel runs the GEMM (from
# MIN_WORKGROUPS up, VQA_GEMM != library).  VQA_GEMM_EPILOGUE=1 fuses every such GEMM + GELU pair, =0 none.
# Recorded per shape at 35264 and 37824 rows (VLMO-base, batch 64; profiles/r11/README.md): "gelu_grad" is 1.18-1.22x of
# the pair, its margin 3-12 times the larger spread in every record, and the benchmark with its entry in place read
# 15.68-15.71 examples/s against the previous commit's 15.45-15.48 in three alternating rounds (1.015x, outputs bitwise
# equal): listed, on the row range of WIDE_POLICY.  "gelu" with h stored is 1.06-1.10x, but its margin (0.06-0.10 ms) is
# of the size of the spreads and falls below the fused call's own max - min in one of four records at 35264 rows: not
# listed (without the store of h, as under no_grad, it is 1.14-1.17x and passes).  Passing per shape but not listed,
# the table holding one row range per class and no end-to-end run taken with them: "gelu_grad" at the text expert's
# 2560 rows (1.25-1.29x) and at ALBEF-base's 147712 rows (1.21-1.22x).
EPILOGUE_POLICY = {"gelu": {}, "gelu_grad": {(3072, 768): _WIDE_ROWS}}

# The two large tiles run one workgroup per CU, so a launch proceeds in rounds of one tile per CU, and its last round,
# however few tiles it holds, costs most of a full one: the N = 768 GEMMs at 35264-37824 rows are 828-888 tiles =
# 3.23-3.47 rounds on 256 CUs.
# ops.gemm_tail_plan cuts such a launch behind its last full round and vqa_gemm_bf16x6_tail runs the rows behind the cut
# on a 128 x 128 tile (twice as many workgroups of half the length, the same bits).  A shape class (N, K) -> (fewest
# rows, most rows), both inclusive, is listed only by the rule of WIDE_POLICY: the split call's median in
# tools/gemm_bench.py beat the unsplit call's by more than the larger round-to-round spread of the two in BOTH records of
# the shape, and the benchmark with the entries in place beat the one without (profiles/r15/README.md).  A listed class
# must be one the plan cuts at 256 CUs.  VQA_GEMM_TAIL=1 cuts every shape the plan cuts, =0 none; VQA_GEMM_TAIL_CUS=n
# pins the CU count the plan is made for (experiments and tests).  Plain ops.gemm calls only: the GELU and LSE epilogues
# have no half tile.
# Recorded (profiles/r15/README.md, VLMO-base, batch 64, 256 CUs, two records): a last round that is 23-47 % full costs
# 0.56-0.78 of a full one and a round of half tiles 0.59-0.66 of a round of full ones, so the cut gains 1.03-1.04x per call
# on (768, 768) at 37824 rows and on (768, 3072) at 35264 rows (passing in both records), 1.01x at 37824 rows of
# (768, 3072) (fails three of four), fails one record of (768, 2304) and loses on (2304, 768).  With the two passing
# classes listed the benchmark read 16.43-16.44 examples/s against the previous commit's 16.41-16.46 in three alternating
# rounds: no difference ((768, 3072) at 35264 rows is a row count of tools/gemm_bench.py that the benchmark's image expert,
# at 64 x 577 rows, never runs, and the projections alone are 0.2 % of a step).  So nothing is listed and the unset
# switch runs what the previous commit ran.  VQA_GEMM_TAIL=1 read 1.008x of VQA_GEMM_TAIL=0 in one tree (two rounds).
TAIL_POLICY = {}

# A multiway layer sends its text rows and its image rows through two FFNs: four GEMMs per layer (fc1 / fc2, forward and
# input gradient) run twice, once per expert.  At the benchmark's shape the text expert's are 24-96 workgroups -- below
# MIN_WORKGROUPS, so they are library calls -- while the image expert's 128 x 256 tiles end in a round that is partly
# empty.  ops.gemm_grouped (vqa_gemm_bf16x6_grouped) runs both experts' tiles in ONE launch, larger group first, with the
# bits of ops.gemm on each expert's rows; the GELU epilogue of the launch is what gelu_epilogue decides for the larger
# group.  A pair is grouped only where both experts are packed, N % 256 == 0, both have rows and the larger one alone
# would run a bf16x6 large tile (from MIN_WORKGROUPS up, VQA_GEMM != library).  A shape class (N, K) -> (fewest rows, most
# rows) OF THE LARGER GROUP, both inclusive, is to be listed only by the rule of WIDE_POLICY (tools/gemm_bench.py
# --grouped: the grouped call's median against the median of the two calls it replaces) plus the benchmark.
# VQA_GEMM_GROUPED=1 groups every eligible pair, =0 none.
# Grouping moves the smaller expert's rows from the library's fp32 GEMM to the bf16x6 kernel, which changes their bits
# (fp32-grade either way); the larger expert's outputs keep theirs.  Nothing is listed: the unset switch launches what
# the previous commit launched, and listing a class is a change of its own that weighs that.  See profiles/r16/README.md
# for what was measured.
GROUPED_POLICY = {}

# The two large tiles run one workgroup per CU, so nothing covers what a tile pays once: while a workgroup waits for
# its first operands the CU's matrix pipe is idle.  ops.gemm_persistent (vqa_gemm_bf16x6_persistent) launches one
# workgroup per CU that walks a list of 128 x 256 tiles and stages a tile's first k-step in the last k-step of the tile
# before it, with the bits of ops.gemm.  A shape class (N, K) -> (fewest rows, most rows), both inclusive, is listed only
# by the rule of WIDE_POLICY: the persistent call's median in tools/gemm_bench.py beat the median of what this module
# dispatches for the class without the entry (the qkv classes: the 256 x 128 kernel) by more than the larger
# round-to-round spread of the two in BOTH records of the shape, and the benchmark with the entries in place beat the one
# without (profiles/r17/README.md).  VQA_GEMM_PERSISTENT=1 runs every plain large-tile GEMM with N % 256 == 0 that
# names no tile of its own as the persistent launch, =0 none; a VQA_GEMM that forces a kernel overrides both.  Plain ops.gemm calls only: the GELU, GELU' and LSE
# epilogues, the tail cut and the grouped launch have no persistent form; a product that gemm_tail_split cuts stays cut.
# Recorded at the benchmark's row counts (VLMO-base, batch 64; profiles/r17/README.md, two records): the fixed cost of a
# tile is 5-8 us, of which the wait for the first operands -- all this launch removes -- is 0.9-1.1 us and the epilogue's
# stores the rest.  Listed: the qkv classes (2304, 768) and (768, 2304) from 37312 to 39488 rows -- batch 64 with 6 to
# 40 text tokens beside 577 image tokens; recorded at 37312, 37760, 37824, 37888, 38848 and 39488 rows, two records each,
# all passing -- 1.08-1.10x of the 256 x 128 kernel they ran before, margins 2.6-18 times the larger spread (most of it is the 128 x 256 tile, which failed WIDE_POLICY's
# rule on the 256 x 128 kernel's spread; the persistent launch is 1.03-1.04x and 1.00-1.01x of the wide kernel).  Not
# listed: (3072, 768), 1.025-1.034x of the wide kernel in all eight records but inside the wide kernel's own max - min
# in one of the two at 36928 rows; (768, 768), 1.02-1.04x, passing in one record of two; (768, 3072), no difference at
# 36928 rows and 0.98x at 35264 (96 k-steps per tile: the wait is 0.5 % of a tile).  With the two entries the benchmark
# read 16.36-16.38 examples/s against the previous commit's 16.11-16.15 in three alternating rounds (1.015x, outputs
# bitwise equal).  ALBEF-base was not measured.
_QKV_ROWS = (37312, 39488)
PERSISTENT_POLICY = {(2304, 768): _QKV_ROWS, (768, 2304): _QKV_ROWS}

_CUS = {}


def _mode():
    """VQA_GEMM: "library" = the library everywhere, "large" = the 256 x 128 kernel from MIN_WORKGROUPS up and the library
    below, "wide" = as "large" on the 128 x 256 tile (where N % 256 == 0), "small" = as "large" plus the small kernel for
    every covered shape below, anything else = the measured policies."""
    mode = os.environ.get("VQA_GEMM", "")
    return mode if mode in ("library", "large", "wide", "small") else ""


def gemm_tile(rows, n, k):
    """The output tile ops.gemm runs (rows, n, k) with where the caller names none: "wide" or "large"."""
    mode = _mode()
    if mode == "wide":
        return "wide"
    lo, hi = WIDE_POLICY.get((n, k), (1, 0))
    return "wide" if mode == "" and lo <= rows <= hi else "large"


def gemm_persistent(rows, n, k):
    """Whether ops.gemm runs (rows, n, k), where the caller names no tile, as the persistent launch of 128 x 256 tiles."""
    if n % 256 or _mode() != "":          # VQA_GEMM=large / wide / small force a kernel: the switch and the table stand back
        return False
    switch = os.environ.get("VQA_GEMM_PERSISTENT", "")
    if switch in ("0", "1"):
        return switch == "1"
    lo, hi = PERSISTENT_POLICY.get((n, k), (1, 0))
    return lo <= rows <= hi


def _kernel_gemms():
    return _mode() != "library"


def device_cus(device):
    """Compute units of ``device``, asked for once per device (the tail plan and the persistent launch's grid)."""
    dev = torch.device(device).index or 0
    if dev not in _CUS:
        _CUS[dev] = torch.cuda.get_device_properties(dev).multi_processor_count
    return _CUS[dev]


def gemm_tail_split(rows, n, k, tile, device):
    """The row from which ops._gemm_tiled hands (rows, n, k) on ``tile`` to the 128 x 128 tile; ``rows`` = nowhere.  The
    device is asked for its CU count (once) only where a cut is wanted at all and VQA_GEMM_TAIL_CUS does not pin it."""
    switch = os.environ.get("VQA_GEMM_TAIL", "")
    if switch == "0":
        return rows
    if switch != "1":
        lo, hi = TAIL_POLICY.get((n, k), (1, 0))
        if switch != "" or not lo <= rows <= hi:
            return rows
    pinned = os.environ.get("VQA_GEMM_TAIL_CUS")
    return ops.gemm_tail_plan(rows, n, tile, int(pinned) if pinned else device_cus(device))


def _small_gemm(rows, n, k):
    mode = _mode()
    if mode == "small":
        return True
    lo, hi = SMALL_POLICY.get((n, k), (1, 0))
    return mode == "" and lo <= rows <= hi


def gelu_epilogue(rows, n, k, epilogue="gelu"):
    """Whether a GEMM (rows, n, k) that feeds a GELU ("gelu"), or the derivative's product ("gelu_grad"), takes the
    fused epilogue."""
    if not _kernel_gemms() or ops.gemm_workgroups(rows, n) < MIN_WORKGROUPS:
        return False
    switch = os.environ.get("VQA_GEMM_EPILOGUE", "")
    if switch in ("0", "1"):
        return switch == "1"
    lo, hi = EPILOGUE_POLICY[epilogue].get((n, k), (1, 0))
    return lo <= rows <= hi


def _pack(w):
    """(forward operand w.t(), input-gradient operand w) of a Linear weight w [out, in], packed once for both kernels;
    None where they do not cover the shape or VQA_GEMM=library."""
    if not _kernel_gemms() or not (ops.gemm_shape_ok(w.shape[0], w.shape[1]) and ops.gemm_shape_ok(w.shape[1], w.shape[0])):
        return (None, None)
    return (ops.gemm_pack(w, trans=True), ops.gemm_pack(w, trans=False))


def _linear(a, w, bias, packed):
    """a @ w.t() + bias (a Linear layer's forward)."""
    pk = packed[0]
    if pk is not None and _kernel_gemms():
        if ops.gemm_workgroups(a.shape[0], pk.N) >= MIN_WORKGROUPS:
            return ops.gemm(a, pk, bias)
        if a.shape[0] and _small_gemm(a.shape[0], pk.N, pk.K):
            return ops.gemm_small(a, pk, bias, ksplit=ops.gemm_small_plan(a.shape[0], pk.N, pk.K))
    return torch.addmm(bias, a, w.t())


def _linear_grad(g, w, packed):
    """g @ w (the input gradient of a Linear layer)."""
    pk = packed[1]
    if pk is not None and _kernel_gemms():
        if ops.gemm_workgroups(g.shape[0], pk.N) >= MIN_WORKGROUPS:
            return ops.gemm(g, pk)
        if g.shape[0] and _small_gemm(g.shape[0], pk.N, pk.K):
            return ops.gemm_small(g, pk, ksplit=ops.gemm_small_plan(g.shape[0], pk.N, pk.K))
    return torch.mm(g, w)


def _linear_gelu(a, w, bias, packed, save):
    """(h or None, gelu(h)) with h = a @ w.t() + bias: an FFN's first layer and its activation.  ``h`` is returned for
    the backward only if ``save``; the fused form then neither allocates nor writes it."""
    pk = packed[0]
    if pk is not None and gelu_epilogue(a.shape[0], pk.N, pk.K):
        h = torch.empty(a.shape[0], pk.N, dtype=torch.float32, device=a.device) if save else None
        return h, ops.gemm(a, pk, bias, epilogue="gelu", aux=h)
    h = _linear(a, w, bias, packed)
    return (h if save else None), ops.gelu_fwd(h)


def _linear_grad_gelu(g, w, packed, h):
    """(g @ w) * gelu'(h): the gradient of the pre-activation ``h`` from the gradient of the FFN's second layer's output."""
    pk = packed[1]
    if pk is not None and gelu_epilogue(g.shape[0], pk.N, pk.K, "gelu_grad"):
        return ops.gemm(g, pk, epilogue="gelu_grad", aux=h)
    return ops.gelu_bwd(h, _linear_grad(g, w, packed))                  # in place on the GEMM's output


def gemm_grouped_pair(rows, n, k):
    """Whether the two experts' GEMMs (rows[0] and rows[1] rows, one (n, k)) run as one grouped launch."""
    big = max(rows)
    if not _kernel_gemms() or n % 256 or min(rows) <= 0 or ops.gemm_workgroups(big, n) < MIN_WORKGROUPS:
        return False
    switch = os.environ.get("VQA_GEMM_GROUPED", "")
    if switch in ("0", "1"):
        return switch == "1"
    lo, hi = GROUPED_POLICY.get((n, k), (1, 0))
    return lo <= big <= hi


def _pair_order(rows, pks):
    """The order -- larger group first -- in which a two-expert layer's GEMMs on ``pks`` go into ONE ops.gemm_grouped
    launch, or None where they run as the two calls of ``_linear`` / ``_linear_grad``."""
    if len(pks) != 2 or pks[0] is None or pks[1] is None or (pks[0].N, pks[0].K) != (pks[1].N, pks[1].K):
        return None
    if not gemm_grouped_pair(rows, pks[0].N, pks[0].K):
        return None
    return (0, 1) if rows[0] >= rows[1] else (1, 0)


def _pair_call(order, xs, pks, biases=None, epilogue=None, aux=None):
    """One grouped launch over the experts in ``order``; the outputs come back in expert order."""
    def pick(ts):
        return None if ts is None else [ts[e] for e in order]
    outs = ops.gemm_grouped(pick(xs), pick(pks), pick(biases), epilogue=epilogue, aux_list=pick(aux))
    back = [None] * len(order)
    for e, o in zip(order, outs):
        back[e] = o
    return back


def _pair_linear_gelu(order, ys, lay, save):
    """``_linear_gelu`` of both experts' fc1 as one launch: ([h or None per expert], [gelu(h) per expert])."""
    pks = [lay.packed["fc1_%d" % e][0] for e in range(2)]
    b1s = [m[1] for m in lay.mlp]
    big = order[0]
    if gelu_epilogue(ys[big].shape[0], pks[big].N, pks[big].K):
        hs = [torch.empty(y.shape[0], pks[big].N, dtype=torch.float32, device=y.device) for y in ys] if save else None
        return (hs if save else [None, None]), _pair_call(order, ys, pks, b1s, epilogue="gelu", aux=hs)
    hs = _pair_call(order, ys, pks, b1s)
    return (hs if save else [None, None]), [ops.gelu_fwd(h) for h in hs]


def _pair_linear_grad_gelu(order, dm, lay, hs):
    """``_linear_grad_gelu`` of both experts' fc2 as one launch."""
    pks = [lay.packed["fc2_%d" % e][1] for e in range(2)]
    big = order[0]
    if gelu_epilogue(dm[big].shape[0], pks[big].N, pks[big].K, "gelu_grad"):
        return _pair_call(order, dm, pks, epilogue="gelu_grad", aux=hs)
    return [ops.gelu_bwd(h, da) for h, da in zip(hs, _pair_call(order, dm, pks))]     # in place on the GEMM's output


def _ffn_forward(ys, lay, save):
    """The FFN of every expert of a layer on its rows ``ys[e]``: ([h or None per expert], [fc2 output per expert]).  A
    two-expert layer runs a stage of both experts as one grouped launch where ``_pair_order`` allows it, and exactly the
    per-expert calls where it allows neither stage."""
    erows = [ye.shape[0] for ye in ys]
    o1 = _pair_order(erows, [lay.packed["fc1_%d" % e][0] for e in range(len(ys))])
    o2 = _pair_order(erows, [lay.packed["fc2_%d" % e][0] for e in range(len(ys))])
    if o1 is None and o2 is None:
        hs, ms = [], []
        for e, (ye, (w1, b1, w2, b2)) in enumerate(zip(ys, lay.mlp)):
            h, a = _linear_gelu(ye, w1, b1, lay.packed["fc1_%d" % e], save)
            ms.append(_linear(a, w2, b2, lay.packed["fc2_%d" % e]))
            hs.append(h)
            del a
    else:                         # both experts stage by stage: each stage one grouped launch where it is eligible
        if o1 is not None:
            hs, acts = _pair_linear_gelu(o1, ys, lay, save)
        else:
            hs, acts = map(list, zip(*[_linear_gelu(ye, m[0], m[1], lay.packed["fc1_%d" % e], save)
                                       for e, (ye, m) in enumerate(zip(ys, lay.mlp))]))
        if o2 is not None:
            ms = _pair_call(o2, acts, [lay.packed["fc2_%d" % e][0] for e in range(2)], [m[3] for m in lay.mlp])
        else:
            ms = [_linear(a, m[2], m[3], lay.packed["fc2_%d" % e]) for e, (a, m) in enumerate(zip(acts, lay.mlp))]
        del acts
    return hs, ms


def _ffn_backward(dm, hs, lay):
    """The input gradient of every expert's FFN from the gradients ``dm[e]`` of its output and the saved ``hs[e]``."""
    erows = [dme.shape[0] for dme in dm]
    o2 = _pair_order(erows, [lay.packed["fc2_%d" % e][1] for e in range(len(dm))])
    o1 = _pair_order(erows, [lay.packed["fc1_%d" % e][1] for e in range(len(dm))])
    if o1 is None and o2 is None:
        dys = []
        for e, (dme, h, (w1, _b1, w2, _b2)) in enumerate(zip(dm, hs, lay.mlp)):
            da = _linear_grad_gelu(dme, w2, lay.packed["fc2_%d" % e], h)      # (rows_e, 4D): dh
            dys.append(_linear_grad(da, w1, lay.packed["fc1_%d" % e]))
            del da
    else:                         # stage by stage, as in _forward
        if o2 is not None:
            das = _pair_linear_grad_gelu(o2, dm, lay, hs)
        else:
            das = [_linear_grad_gelu(dme, m[2], lay.packed["fc2_%d" % e], h)
                   for e, (dme, h, m) in enumerate(zip(dm, hs, lay.mlp))]
        if o1 is not None:
            dys = _pair_call(o1, das, [lay.packed["fc1_%d" % e][1] for e in range(2)])
        else:
            dys = [_linear_grad(da, m[0], lay.packed["fc1_%d" % e]) for e, (da, m) in enumerate(zip(das, lay.mlp))]
        del das
    return dys


class LayerSpec:
    """Frozen parameters of one block, in the form the stages consume (plain fp32 device tensors), and every weight
    packed for the GEMM kernel: ``packed[name] = (forward operand, input-gradient operand)`` for "qkv", "proj" and
    "fc1_e" / "fc2_e" of expert e (``_pack``; 12 bytes per parameter)."""
    __slots__ = ("ln1", "wqkv", "bqkv", "wproj", "bproj", "gamma1", "ln2", "mlp", "gamma2", "eps", "packed")

    def __init__(self, ln1, wqkv, bqkv, wproj, bproj, gamma1, ln2, mlp, gamma2, eps):
        self.ln1, self.wqkv, self.bqkv, self.wproj, self.bproj = ln1, wqkv, bqkv, wproj, bproj
        self.gamma1, self.ln2, self.mlp, self.gamma2, self.eps = gamma1, ln2, mlp, gamma2, eps
        self.packed = dict(qkv=_pack(wqkv), proj=_pack(wproj))
        for e, (w1, _b1, w2, _b2) in enumerate(mlp):
            self.packed["fc1_%d" % e], self.packed["fc2_%d" % e] = _pack(w1), _pack(w2)


class EncoderSpec:
    def __init__(self, layers, final_ln, final_eps, heads):
        self.layers, self.final_ln, self.final_eps, self.heads = layers, final_ln, final_eps, heads


def supported(dim, heads):
    """The hand-written stages cover the head size of every BASELINE configuration (64) and D <= 1024."""
    return dim % heads == 0 and dim // heads == _attn.HEAD_DIM and dim % 4 == 0 and dim <= 1024


def weights_key(module):
    """Fingerprint of the frozen weights a spec was built from: storage address and in-place version counter of every
    parameter.  Detected: ``load_state_dict`` (copying or ``assign=True``), ``.to()``, ``p.copy_()`` / any in-place op ON
    THE PARAMETER.  NOT detected: writes through ``p.data`` (``p.data.copy_(w)``, ``p.data.add_(1)``) -- ``.data`` is a
    detached alias with its own version counter, so the key stays equal and a cached spec that holds COPIES (ALBEF's
    packed q / k / v, contiguous copies of strided parameters) would keep the old values.  Code that updates weights
    that way calls ``invalidate_fused()`` on the model (``FrozenVlmo`` / ``FrozenAlbef``); the reference-checkpoint
    loaders do.  ~0.1 us per parameter, once per encoder pass."""
    return tuple((p.data_ptr(), p._version) for p in module.parameters())


def _c(t):
    t = t.detach()
    return t if t.is_contiguous() else t.contiguous()


def _ln(mod):
    return (_c(mod.weight), _c(mod.bias))


def _mlp(mod):
    return (_c(mod.fc1.weight), _c(mod.fc1.bias), _c(mod.fc2.weight), _c(mod.fc2.bias))


def vlmo_spec(model):
    """``FrozenVlmo`` -> EncoderSpec.  Expert layers carry two LayerNorm / MLP sets (text, image), VL-FFN layers one."""
    layers = []
    for blk in model.blocks:
        if blk.mlp_vl is None:
            ln2, mlp = [_ln(blk.norm2_text), _ln(blk.norm2_imag)], [_mlp(blk.mlp_text), _mlp(blk.mlp_imag)]
        else:
            ln2, mlp = [_ln(blk.norm2_vl)], [_mlp(blk.mlp_vl)]
        layers.append(LayerSpec(_ln(blk.norm1), _c(blk.attn.qkv.weight), _c(blk.attn.qkv.bias), _c(blk.attn.proj.weight),
                                _c(blk.attn.proj.bias), _c(blk.gamma_1), ln2, mlp, _c(blk.gamma_2), blk.norm1.eps))
    return EncoderSpec(layers, _ln(model.norm), model.norm.eps, model.cfg.heads)


def vit_spec(blocks, final_norm, heads):
    """ALBEF's ViT blocks (separate q / k / v projections packed into one GEMM once -- the weights are frozen)."""
    layers = []
    for blk in blocks:
        a = blk.attn
        wqkv = torch.cat([a.q.weight.detach(), a.k.weight.detach(), a.v.weight.detach()], dim=0).contiguous()
        bqkv = torch.cat([a.q.bias.detach(), a.k.bias.detach(), a.v.bias.detach()], dim=0).contiguous()
        layers.append(LayerSpec(_ln(blk.norm1), wqkv, bqkv, _c(a.o.weight), _c(a.o.bias), None, [_ln(blk.norm2)],
                                [_mlp(blk.mlp)], None, blk.norm1.eps))
    return EncoderSpec(layers, _ln(final_norm), final_norm.eps, heads)


class _Call:
    """Per-call context: the attention masks of the text batch and the token layout."""

    def __init__(self, spec, biases, n_text):
        self.spec, self.biases, self.n_text = spec, biases, n_text


def _attention_inputs(qkv5, bias, need_grad):
    q, k, v = qkv5[:, :, 0], qkv5[:, :, 1], qkv5[:, :, 2]
    b, s, h, _ = q.shape
    hole = None
    if isinstance(bias, _attn.KeyHoleBias):
        if need_grad and not _attn.scores_fit(b, h, s, s):
            bias = bias.dense()
        else:
            bias, hole = bias.slab, bias.hole
    bias_t, bstr = _attn._bias_view(None if bias is None else bias.detach(), b, h, s, s)
    return q, k, v, bias_t, bstr, hole


def _forward(x0, call, save):
    spec = call.spec
    b, s, d = x0.shape
    rows, t = b * s, call.n_text
    dev, f32 = x0.device, torch.float32
    scale = _attn.HEAD_DIM ** -0.5
    x = x0 if x0.is_contiguous() else x0.contiguous()
    pend = None                       # (m0, m1, gamma2) of the previous layer: its residual add happens in the next LN
    feats, saved = [], []
    for li, lay in enumerate(spec.layers):
        y = torch.empty(rows, d, dtype=f32, device=dev)
        mean1, rstd1 = torch.empty(rows, dtype=f32, device=dev), torch.empty(rows, dtype=f32, device=dev)
        if pend is None:
            x_l = x
            ops.ln_fwd(x, lay.ln1[0], lay.ln1[1], y, mean1, rstd1, lay.eps)
        else:
            x_l = torch.empty(b, s, d, dtype=f32, device=dev)
            ops.ln_fwd(x, lay.ln1[0], lay.ln1[1], y, mean1, rstd1, lay.eps, r0=pend[0], r1=pend[1], rscale=pend[2],
                       x_out=x_l, period=s if pend[1] is not None else 0, split=t if pend[1] is not None else 0)
            feats.append(x_l)
        qkv = _linear(y, lay.wqkv, lay.bqkv, lay.packed["qkv"])
        del y
        qkv5 = qkv.view(b, s, 3, spec.heads, _attn.HEAD_DIM)
        q, k, v, bias_t, bstr, hole = _attention_inputs(qkv5, None if call.biases is None else call.biases[li], save)
        o, lse, scores = _attn._forward(q, k, v, bias_t, bstr, scale, save_scores=save, key_hole=hole)
        p = _linear(o.view(rows, d), lay.wproj, lay.bproj, lay.packed["proj"])
        x1 = torch.empty(b, s, d, dtype=f32, device=dev)
        mean2, rstd2 = torch.empty(rows, dtype=f32, device=dev), torch.empty(rows, dtype=f32, device=dev)
        two = len(lay.mlp) == 2
        if two:
            ys = [torch.empty(b * t, d, dtype=f32, device=dev), torch.empty(b * (s - t), d, dtype=f32, device=dev)]
            ops.ln_fwd(x_l, lay.ln2[0][0], lay.ln2[0][1], ys[0], mean2, rstd2, lay.eps, r0=p, rscale=lay.gamma1, x_out=x1,
                       gamma1=lay.ln2[1][0], beta1=lay.ln2[1][1], y1=ys[1], period=s, split=t)
        else:
            ys = [torch.empty(rows, d, dtype=f32, device=dev)]
            ops.ln_fwd(x_l, lay.ln2[0][0], lay.ln2[0][1], ys[0], mean2, rstd2, lay.eps, r0=p, rscale=lay.gamma1, x_out=x1)
        del p
        hs, ms = _ffn_forward(ys, lay, save)
        del ys
        if save:
            saved.append(dict(x_l=x_l, mean1=mean1, rstd1=rstd1, qkv=qkv, o=o, lse=lse, scores=scores, bias=bias_t,
                              bstr=bstr, x1=x1, mean2=mean2, rstd2=rstd2, hs=hs))
        x, pend = x1, (ms[0], ms[1] if two else None, lay.gamma2)
    x_last = torch.empty(b, s, d, dtype=f32, device=dev)
    states = torch.empty(b, s, d, dtype=f32, device=dev)
    mean_f, rstd_f = torch.empty(rows, dtype=f32, device=dev), torch.empty(rows, dtype=f32, device=dev)
    ops.ln_fwd(x, spec.final_ln[0], spec.final_ln[1], states, mean_f, rstd_f, spec.final_eps, r0=pend[0], r1=pend[1],
               rscale=pend[2], x_out=x_last, period=s if pend[1] is not None else 0, split=t if pend[1] is not None else 0)
    feats.append(x_last)
    if save:
        saved.append(dict(x_l=x_last, mean1=mean_f, rstd1=rstd_f))
    return feats, states, saved


def _dense(g, like):
    """A gradient autograd hands over, as the kernels read it: fp32, contiguous, or None."""
    if g is None:
        return None
    return g if g.is_contiguous() else g.contiguous()


def _branch_buffers(two, b, s, t, d, dev):
    if two:
        return [torch.empty(b * t, d, dtype=torch.float32, device=dev),
                torch.empty(b * (s - t), d, dtype=torch.float32, device=dev)]
    return [torch.empty(b * s, d, dtype=torch.float32, device=dev)]


def _backward(saved, call, g_feats, g_states, shape):
    """``g_feats[l]``: gradient of feature map l + 1 (the output of block l; None = no loss on it); ``g_states``: gradient
    of the final normalised states.  Returns the gradient of the encoder's input."""
    spec = call.spec
    b, s, d = shape
    rows, t = b * s, call.n_text
    dev = saved[-1]["x_l"].device
    scale = _attn.HEAD_DIM ** -0.5
    n = len(spec.layers)
    fin = saved[n]
    if g_states is None:
        g_states = torch.zeros(b, s, d, dtype=torch.float32, device=dev)
    last = spec.layers[n - 1]
    two = len(last.mlp) == 2
    dx = torch.empty(rows, d, dtype=torch.float32, device=dev)
    dm = _branch_buffers(two, b, s, t, d, dev) if (two or last.gamma2 is not None) else [dx]
    ops.ln_bwd(_dense(g_states, dx), fin["x_l"], fin["mean1"], fin["rstd1"], spec.final_ln[0], dx,
               g_inj=_dense(g_feats[n - 1], dx), rscale=last.gamma2, dr0=dm[0] if dm[0] is not dx else None,
               dr1=dm[1] if two else None, period=s if two else 0, split=t if two else 0)
    g = dx                                        # gradient w.r.t. the last layer's x1 (residual path)
    for li in range(n - 1, -1, -1):
        lay, sv = spec.layers[li], saved[li]
        two = len(lay.mlp) == 2
        dys = _ffn_backward(dm, sv["hs"], lay)
        del dm
        dx1 = torch.empty(rows, d, dtype=torch.float32, device=dev)
        dp = torch.empty(rows, d, dtype=torch.float32, device=dev) if lay.gamma1 is not None else dx1
        ops.ln_bwd(dys[0], sv["x1"], sv["mean2"], sv["rstd2"], lay.ln2[0][0], dx1, dy1=dys[1] if two else None,
                   gamma1=lay.ln2[1][0] if two else None, g_a=g, rscale=lay.gamma1,
                   dr0=dp if lay.gamma1 is not None else None, period=s if two else 0, split=t if two else 0)
        del dys, g
        do = _linear_grad(dp, lay.wproj, lay.packed["proj"])
        dqkv = torch.empty_like(sv["qkv"])
        qkv5, dqkv5 = sv["qkv"].view(b, s, 3, spec.heads, _attn.HEAD_DIM), dqkv.view(b, s, 3, spec.heads, _attn.HEAD_DIM)
        _attn._backward(qkv5[:, :, 0], qkv5[:, :, 1], qkv5[:, :, 2], sv["bias"], sv["bstr"], sv["o"], sv["lse"],
                        do.view(b, s, spec.heads, _attn.HEAD_DIM), dqkv5[:, :, 0], dqkv5[:, :, 1], dqkv5[:, :, 2], scale,
                        scores=sv["scores"])
        del do, dp
        dy1 = _linear_grad(dqkv.view(rows, -1), lay.wqkv, lay.packed["qkv"])
        del dqkv
        dx_l = torch.empty(rows, d, dtype=torch.float32, device=dev)
        if li > 0:
            prev = spec.layers[li - 1]
            ptwo = len(prev.mlp) == 2
            dm = _branch_buffers(ptwo, b, s, t, d, dev) if (ptwo or prev.gamma2 is not None) else [dx_l]
            ops.ln_bwd(dy1, sv["x_l"], sv["mean1"], sv["rstd1"], lay.ln1[0], dx_l, g_a=dx1,
                       g_inj=_dense(g_feats[li - 1], dx_l), rscale=prev.gamma2, dr0=dm[0] if dm[0] is not dx_l else None,
                       dr1=dm[1] if ptwo else None, period=s if ptwo else 0, split=t if ptwo else 0)
        else:
            ops.ln_bwd(dy1, sv["x_l"], sv["mean1"], sv["rstd1"], lay.ln1[0], dx_l, g_a=dx1)
        del dy1, dx1
        saved[li] = None                          # this layer's activations are dead
        g = dx_l
    return g.view(b, s, d)


class _Encoder(torch.autograd.Function):
    """(x0 (B, S, D), call) -> (feature map 1, ..., feature map L, final normalised states)."""

    @staticmethod
    def forward(ctx, x0, call):
        # an output the loss does not touch (every feature map during an MLM step of the dual loss) must reach backward
        # as None, not as a materialised zero tensor: 12 x (fill + read) of (B, S, D) per step otherwise
        ctx.set_materialize_grads(False)
        save = ctx.needs_input_grad[0]
        feats, states, saved = _forward(x0.detach(), call, save)
        if save:
            # the layer inputs x_l are the Function's own input / outputs: they must go through save_for_backward (an
            # output kept in a ctx attribute is a reference cycle through the C++ graph that no collector sees)
            layer_inputs = [sv.pop("x_l") for sv in saved]
            ctx.save_for_backward(*layer_inputs)
        ctx.call, ctx.saved, ctx.shape = call, saved, tuple(x0.shape)
        return tuple(feats) + (states,)

    @staticmethod
    def backward(ctx, *grads):
        saved, ctx.saved = ctx.saved, None
        if saved is None:
            raise RuntimeError("the fused encoder's backward ran twice (its activations are freed by the first run)")
        for sv, x_l in zip(saved, ctx.saved_tensors):
            sv["x_l"] = x_l
        return _backward(saved, ctx.call, grads[:-1], grads[-1], ctx.shape), None


def encode(x0, spec, biases, n_text):
    """Run the encoder on the residual stream ``x0`` (B, S, D) (token embeddings + type embeddings).  ``biases``: one
    additive attention mask per layer (or None), ``n_text``: text tokens at the front of the sequence (0 = one
    modality).  Returns ``([x0, feature maps 1..L], states)`` like the eager block loop."""
    if not x0.is_cuda or x0.dtype != torch.float32:
        raise ops._hip.HipExtensionError("the fused encoder runs on fp32 HIP tensors")
    outs = _Encoder.apply(x0, _Call(spec, biases, n_text))
    return [x0] + list(outs[:-1]), outs[-1]


# ------------------------------------------------------------------------------------ post-LN BERT fusion encoder (ALBEF)
# Reference computation: ``BertLayer.forward`` of ``ALBEF_attack/models/xbert.py`` -- self-attention, ``BertSelfOutput``
# (LayerNorm(dense(o) + x)), from ``fusion_layer`` up the same pair with the image states as keys / values, then
# ``BertIntermediate`` (GELU) and ``BertOutput`` (LayerNorm(dense(a) + x)); restated by ``whitebox/albef.py _BertLayer``.
# A post-LN stage is ``y = LN(s)``, ``s = x + f(x)``: forward ONE ``vqa_ln_fwd`` (r0 = f(x), x_out = s, kept for the
# backward as the pre-LN path keeps x1), backward ONE ``vqa_ln_bwd_post`` that sums the gradients reaching y first; its
# result ds is the residual-path gradient and the branch gradient at once.
#
# Cross-attention keys / values: the K and V weights of ALL fusion layers are stacked into one [2 D n_fusion, D] weight, so
# every layer's K / V come from ONE GEMM over the image states (N = 9216 at base size; the attention kernels read the
# layer's slice of that buffer through strides), and the gradient of the image states is ONE input-gradient GEMM over the
# stacked dK / dV (K = 9216) instead of twelve GEMMs and eleven accumulation passes: deterministic, fixed order.  Cost:
# two (B M, 2 D n_fusion) buffers live across the call, 2 x 5.4 GB at batch 256 x 577 tokens.
class BertLayerSpec:
    """Frozen parameters of one post-LN BERT layer as plain fp32 device tensors + every weight the text rows multiply
    packed by ``_pack``: "qkv" (packed self-attention projection), "o", "fc1", "fc2" and, in fusion layers, "q_c" / "o_c"
    (the cross-attention's query and output projections; its K / V weights live stacked in ``FusionSpec``).  ``cross``:
    index of this layer among the fusion layers, or None."""
    __slots__ = ("wqkv", "bqkv", "wo", "bo", "ln_attn", "cross", "wq_c", "bq_c", "wo_c", "bo_c", "ln_cross", "w1", "b1",
                 "w2", "b2", "ln_out", "packed")

    def __init__(self, layer, cross):
        a = layer.attn
        self.wqkv = torch.cat([a.q.weight.detach(), a.k.weight.detach(), a.v.weight.detach()], dim=0).contiguous()
        self.bqkv = torch.cat([a.q.bias.detach(), a.k.bias.detach(), a.v.bias.detach()], dim=0).contiguous()
        self.wo, self.bo, self.ln_attn = _c(a.o.weight), _c(a.o.bias), _ln(layer.ln_attn)
        self.w1, self.b1, self.w2, self.b2 = _mlp(layer.mlp)
        self.ln_out = _ln(layer.ln_out)
        self.packed = dict(qkv=_pack(self.wqkv), o=_pack(self.wo), fc1=_pack(self.w1), fc2=_pack(self.w2))
        self.cross = cross
        if cross is not None:
            c = layer.cross
            self.wq_c, self.bq_c, self.wo_c, self.bo_c = _c(c.q.weight), _c(c.q.bias), _c(c.o.weight), _c(c.o.bias)
            self.ln_cross = _ln(layer.ln_cross)
            self.packed["q_c"], self.packed["o_c"] = _pack(self.wq_c), _pack(self.wo_c)


class FusionSpec:
    """``layers``: one BertLayerSpec per layer; ``wkv`` [2 D n_fusion, D] / ``bkv``: rows ``[2 D j, 2 D j + D)`` are the
    K weight of fusion layer j, the next D rows its V weight."""

    def __init__(self, layers, heads, eps, wkv, bkv):
        self.layers, self.heads, self.eps, self.wkv, self.bkv = layers, heads, eps, wkv, bkv
        self.n_fusion = sum(lay.cross is not None for lay in layers)
        self.first_fusion = next((i for i, lay in enumerate(layers) if lay.cross is not None), len(layers))
        self.packed_kv = _pack(wkv) if wkv is not None else (None, None)


def bert_spec(layers, heads, eps):
    """ALBEF's BERT layers (``_BertLayer`` modules) -> FusionSpec: the post-LN counterpart of ``vit_spec``."""
    specs, wkv, bkv = [], [], []
    for layer in layers:
        cross = None
        if layer.cross is not None:
            cross = len(wkv) // 2
            wkv += [layer.cross.k.weight.detach(), layer.cross.v.weight.detach()]
            bkv += [layer.cross.k.bias.detach(), layer.cross.v.bias.detach()]
        specs.append(BertLayerSpec(layer, cross))
    return FusionSpec(specs, heads, eps, torch.cat(wkv, dim=0).contiguous() if wkv else None,
                      torch.cat(bkv, dim=0).contiguous() if bkv else None)


class _FusionCall:
    """Per-call context: the spec, the key-padding bias of the text batch (tensor kept alive, strides) and the caller's
    grad mode (``Function.forward`` runs with it off and ``needs_input_grad`` only reflects ``requires_grad``)."""

    def __init__(self, spec, bias_t, bstr, grad):
        self.spec, self.bias_t, self.bstr, self.grad = spec, bias_t, bstr, grad


def _kv_slices(buf, j, b, m, heads):
    """(K, V) of fusion layer j inside a stacked (B M, 2 D n_fusion) buffer, each as a strided (B, M, H, 64) view."""
    kv = buf.view(b, m, -1, 2, heads, _attn.HEAD_DIM)
    return kv[:, :, j, 0], kv[:, :, j, 1]


def _post_ln(x, branch, ln, eps, save):
    """y = LN(x + branch); returns (y, (s, rstd) or None).  The sum s is written out only where the backward will read it."""
    rows, d = x.shape
    y, s = torch.empty_like(x), (torch.empty_like(x) if save else None)
    mean = torch.empty(rows, dtype=torch.float32, device=x.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
    ops.ln_fwd(x, ln[0], ln[1], y, mean, rstd, eps, r0=branch, x_out=s)
    return y, ((s, rstd) if save else None)


def _fusion_forward(x0, img, call, full_from, partial):
    """Layers ``>= full_from`` keep everything their backward needs; layer ``partial`` (or None) keeps what the path from
    its output to its cross-attention K / V needs (FFN and cross-attention, not the self-attention)."""
    spec = call.spec
    b, t, d = x0.shape
    rows = b * t
    heads = spec.heads
    scale = _attn.HEAD_DIM ** -0.5
    x = (x0 if x0.is_contiguous() else x0.contiguous()).view(rows, d)
    kv, m = None, 0
    if spec.n_fusion:
        if img is None or img.dim() != 3 or img.shape[0] != b or img.shape[2] != d:
            raise ValueError("the fusion layers need image states (B = {}, M, D = {}), got {}".format(
                b, d, None if img is None else tuple(img.shape)))
        m = img.shape[1]
        img2 = (img if img.is_contiguous() else img.contiguous()).view(b * m, d)
        kv = _linear(img2, spec.wkv, spec.bkv, spec.packed_kv)             # K / V of every fusion layer: one GEMM
    feats, saved = [], []
    for li, lay in enumerate(spec.layers):
        full = li >= full_from
        part = full or li == partial
        sv = {}
        qkv = _linear(x, lay.wqkv, lay.bqkv, lay.packed["qkv"])
        qkv5 = qkv.view(b, t, 3, heads, _attn.HEAD_DIM)
        o, lse, scores = _attn._forward(qkv5[:, :, 0], qkv5[:, :, 1], qkv5[:, :, 2], call.bias_t, call.bstr, scale,
                                        save_scores=full)
        p = _linear(o.view(rows, d), lay.wo, lay.bo, lay.packed["o"])
        x, st = _post_ln(x, p, lay.ln_attn, spec.eps, full)
        del p
        if full:
            sv.update(qkv=qkv, o=o, lse=lse, scores=scores, ln_attn=st)
        del qkv, qkv5, o, lse, scores
        if lay.cross is not None:
            q = _linear(x, lay.wq_c, lay.bq_c, lay.packed["q_c"]).view(b, t, heads, _attn.HEAD_DIM)
            k, v = _kv_slices(kv, lay.cross, b, m, heads)
            o, lse, scores = _attn._forward(q, k, v, None, None, scale, save_scores=part)
            p = _linear(o.view(rows, d), lay.wo_c, lay.bo_c, lay.packed["o_c"])
            x, st = _post_ln(x, p, lay.ln_cross, spec.eps, part)
            del p
            if part:
                sv.update(q_c=q, o_c=o, lse_c=lse, scores_c=scores, ln_cross=st)
            del q, o, lse, scores
        h, a = _linear_gelu(x, lay.w1, lay.b1, lay.packed["fc1"], part)
        f = _linear(a, lay.w2, lay.b2, lay.packed["fc2"])
        del a
        x, st = _post_ln(x, f, lay.ln_out, spec.eps, part)
        del f
        if part:
            sv.update(h=h, ln_out=st)
        del h
        feats.append(x.view(b, t, d))
        saved.append(sv if part else None)
    return feats, saved, kv


def _ln_post_grad(summands, st, gamma):
    """ds = LN'(sum of the one to three gradients reaching y = LN(s)), one kernel."""
    s, rstd = st
    ds = torch.empty_like(s)
    sm = [_dense(g, s) for g in summands if g is not None]
    ops.ln_bwd_post(sm[0].view(s.shape), s, rstd, gamma, ds, dy_b=sm[1].view(s.shape) if len(sm) > 1 else None,
                    g_inj=sm[2].view(s.shape) if len(sm) > 2 else None)
    return ds


def _fusion_backward(saved, kv, call, g_feats, g_states, shape, m, need_t, need_i):
    """``g_feats[l]``: gradient of feature map l + 1 (the output of layer l), ``g_states``: gradient of the final states
    (the same values as the last feature map); None = no loss on it.  Returns (gradient of the text embeddings or None,
    gradient of the image states or None)."""
    spec = call.spec
    b, t, d = shape
    rows, heads = b * t, spec.heads
    scale = _attn.HEAD_DIM ** -0.5
    n = len(spec.layers)
    stop = 0 if need_t else spec.first_fusion        # the lowest layer that is back-propagated (only partly unless need_t)
    if stop >= n:
        return None, None
    dev = call.bias_t.device
    dkv = None
    if spec.n_fusion:
        # every fusion layer's dK / dV side by side (one input-gradient GEMM afterwards) when the image states need a
        # gradient; otherwise one layer's worth of room the attention backward writes and nobody reads
        dkv = torch.empty(b * m, 2 * d * (spec.n_fusion if need_i else 1), dtype=torch.float32, device=dev)
    inc = [g_states, None, g_feats[n - 1]]           # the gradients reaching the output of the layer at hand
    for li in range(n - 1, stop - 1, -1):
        lay, sv = spec.layers[li], saved[li]
        if not any(g is not None for g in inc):      # no loss above this layer: nothing flows, its dK / dV are zero
            if lay.cross is not None and need_i:
                dk, dv = _kv_slices(dkv, lay.cross, b, m, heads)
                dk.zero_(), dv.zero_()
            inc = [None, None, g_feats[li - 1] if li > 0 else None]
            saved[li] = None
            continue
        ds = _ln_post_grad(inc, sv["ln_out"], lay.ln_out[0])              # d(x + ffn(x)): residual path and branch
        da = _linear_grad_gelu(ds, lay.w2, lay.packed["fc2"], sv["h"])      # dh
        dx = _linear_grad(da, lay.w1, lay.packed["fc1"])
        del da
        inc = [ds, dx, None]
        if lay.cross is not None:
            ds = _ln_post_grad(inc, sv["ln_cross"], lay.ln_cross[0])
            do = _linear_grad(ds, lay.wo_c, lay.packed["o_c"])
            k, v = _kv_slices(kv, lay.cross, b, m, heads)
            dk, dv = _kv_slices(dkv, lay.cross if need_i else 0, b, m, heads)
            dq = torch.empty(b, t, heads, _attn.HEAD_DIM, dtype=torch.float32, device=dev)
            _attn._backward(sv["q_c"], k, v, None, None, sv["o_c"], sv["lse_c"], do.view(b, t, heads, _attn.HEAD_DIM),
                            dq, dk, dv, scale, scores=sv["scores_c"])
            del do
            if li == stop and not need_t:            # the image states are reached; nothing below needs a gradient
                saved[li] = None
                break
            dx = _linear_grad(dq.view(rows, d), lay.wq_c, lay.packed["q_c"])
            del dq
            inc = [ds, dx, None]
        ds = _ln_post_grad(inc, sv["ln_attn"], lay.ln_attn[0])
        do = _linear_grad(ds, lay.wo, lay.packed["o"])
        dqkv = torch.empty_like(sv["qkv"])
        qkv5, dqkv5 = sv["qkv"].view(b, t, 3, heads, _attn.HEAD_DIM), dqkv.view(b, t, 3, heads, _attn.HEAD_DIM)
        _attn._backward(qkv5[:, :, 0], qkv5[:, :, 1], qkv5[:, :, 2], call.bias_t, call.bstr, sv["o"], sv["lse"],
                        do.view(b, t, heads, _attn.HEAD_DIM), dqkv5[:, :, 0], dqkv5[:, :, 1], dqkv5[:, :, 2], scale,
                        scores=sv["scores"])
        del do
        dx = _linear_grad(dqkv, lay.wqkv, lay.packed["qkv"])
        del dqkv, qkv5, dqkv5
        inc = [ds, dx, g_feats[li - 1] if li > 0 else None]
        saved[li] = None                              # this layer's activations are dead
    g_text = g_img = None
    if need_t:
        g_text = torch.add(inc[0], inc[1]).view(b, t, d) if inc[0] is not None else \
            torch.zeros(b, t, d, dtype=torch.float32, device=dev)
    if need_i and spec.n_fusion:
        g_img = _linear_grad(dkv, spec.wkv, spec.packed_kv).view(b, m, d)   # one GEMM over the stacked dK / dV
    return g_text, g_img


class _FusionEncoder(torch.autograd.Function):
    """(text embeddings (B, T, D), image states (B, M, D), call) -> (feature map 1, ..., feature map L, final states).
    The backward needs none of the Function's inputs or outputs (a post-LN stage keeps its pre-LayerNorm sum instead of
    the layer input), so everything it keeps is private to the call and is freed layer by layer."""

    @staticmethod
    def forward(ctx, text_embeds, image_states, call):
        ctx.set_materialize_grads(False)
        need_t = call.grad and ctx.needs_input_grad[0]
        need_i = call.grad and ctx.needs_input_grad[1] and call.spec.n_fusion > 0
        n = len(call.spec.layers)
        full_from = 0 if need_t else (call.spec.first_fusion + 1 if need_i else n)
        partial = call.spec.first_fusion if (need_i and not need_t) else None
        feats, saved, kv = _fusion_forward(text_embeds.detach(), None if image_states is None else image_states.detach(),
                                           call, full_from, partial)
        ctx.call, ctx.saved, ctx.kv, ctx.need = call, saved, (kv if need_t or need_i else None), (need_t, need_i)
        ctx.shape, ctx.m = tuple(text_embeds.shape), 0 if image_states is None else image_states.shape[1]
        return tuple(feats) + (feats[-1].view_as(feats[-1]),)

    @staticmethod
    def backward(ctx, *grads):
        saved, kv, ctx.saved, ctx.kv = ctx.saved, ctx.kv, None, None
        if saved is None:
            raise RuntimeError("the fused encoder's backward ran twice (its activations are freed by the first run)")
        g_text, g_img = _fusion_backward(saved, kv, ctx.call, grads[:-1], grads[-1], ctx.shape, ctx.m, *ctx.need)
        return g_text, g_img, None


def encode_fusion(text_embeds, text_masks, image_states, spec):
    """ALBEF's BERT fusion encoder on the text embeddings (B, T, D) with cross-attention into ``image_states`` (B, M, D)
    from the first fusion layer up; ``text_masks`` (B, T): 0 = padding (masked as a key of the self-attention; the
    cross-attention has no mask).  Returns ``([text_embeds, feature maps 1..L], final states)`` like the eager layer
    loop.  No host read or synchronisation: a graph capture of the attack step records it."""
    for name, ten in (("text_embeds", text_embeds), ("image_states", image_states)):
        if ten is not None and (not ten.is_cuda or ten.dtype != torch.float32 or ten.device != text_embeds.device):
            raise ops._hip.HipExtensionError("the fused encoder runs on fp32 HIP tensors of one device ({})".format(name))
    if text_masks.device != text_embeds.device:
        raise ops._hip.HipExtensionError("the fused encoder runs on fp32 HIP tensors of one device (text_masks)")
    b, t, _ = text_embeds.shape
    pad = torch.zeros(b, 1, 1, t, device=text_embeds.device)
    pad = pad.masked_fill(~text_masks.bool()[:, None, None, :], float("-inf"))
    bias_t, bstr = _attn._bias_view(pad, b, spec.heads, t, t)
    outs = _FusionEncoder.apply(text_embeds, image_states, _FusionCall(spec, bias_t, bstr, torch.is_grad_enabled()))
    return [text_embeds] + list(outs[:-1]), outs[-1]


# ------------------------------------------------------------------------------------ ALBEF's answer decoder (forward only)
# Reference computation: the second pass of ``rank_answer`` (``ALBEF_attack/models/model_vqa.py:149-203``): the causal
# ``text_decoder`` on the k candidate answers of every question, with cross-attention into the question states tiled k
# times (``tile(question_states, 0, k)``).  The candidates of one question share their keys and values, so here nothing is
# tiled: the cross-attention K / V of all layers come from ONE stacked GEMM over the B T question-state rows (not
# B k T), and the k candidates are folded into the QUERY axis of the cross-attention -- candidate rows are contiguous by
# (sample, candidate, position), so the (B k L, D) query projection is a (B, k L, H, 64) view, the keys / values are the
# (B, T, H, 64) slices of ``_kv_slices`` and the bias is the (B, 1, 1, T) question key padding.  Queries never interact:
# row by row the arithmetic of the tiled form, on the attention kernel that exists.
def decode_candidates(x0, self_bias, question_states, question_pad, k, spec):
    """``x0``: (B k, L, D) decoder embeddings of the candidates, sample-major; ``self_bias``: additive (B k, 1, L, L)
    causal-and-padding mask; ``question_states``: (B, T, D); ``question_pad``: additive (B, 1, 1, T) key padding;
    ``spec``: ``bert_spec`` of the decoder layers (every layer has cross-attention).  Returns the final states
    (B k, L, D).  Forward only (the victim runs under ``no_grad``): nothing is kept.  No host read or synchronisation."""
    for name, ten in (("x0", x0), ("self_bias", self_bias), ("question_states", question_states),
                      ("question_pad", question_pad)):
        if not ten.is_cuda or ten.dtype != torch.float32 or ten.device != x0.device:
            raise ops._hip.HipExtensionError("the fused decoder runs on fp32 HIP tensors of one device ({})".format(name))
    n, length, d = x0.shape
    b, t = question_states.shape[0], question_states.shape[1]
    if n != b * k or question_states.shape[2] != d or any(lay.cross is None for lay in spec.layers):
        raise ValueError("decode_candidates: {} candidate rows for {} questions x k = {}, width {} / {}".format(
            n, b, k, d, question_states.shape[2]))
    rows, heads = n * length, spec.heads
    scale = _attn.HEAD_DIM ** -0.5
    bias_s, bstr_s = _attn._bias_view(self_bias, n, heads, length, length)
    bias_c, bstr_c = _attn._bias_view(question_pad, b, heads, k * length, t)
    qs = (question_states if question_states.is_contiguous() else question_states.contiguous()).view(b * t, d)
    kv = _linear(qs, spec.wkv, spec.bkv, spec.packed_kv)                  # K / V of every layer, once per QUESTION
    x = (x0 if x0.is_contiguous() else x0.contiguous()).view(rows, d)
    for lay in spec.layers:
        qkv5 = _linear(x, lay.wqkv, lay.bqkv, lay.packed["qkv"]).view(n, length, 3, heads, _attn.HEAD_DIM)
        o, _lse, _ = _attn._forward(qkv5[:, :, 0], qkv5[:, :, 1], qkv5[:, :, 2], bias_s, bstr_s, scale)
        del qkv5
        x, _ = _post_ln(x, _linear(o.view(rows, d), lay.wo, lay.bo, lay.packed["o"]), lay.ln_attn, spec.eps, False)
        q = _linear(x, lay.wq_c, lay.bq_c, lay.packed["q_c"]).view(b, k * length, heads, _attn.HEAD_DIM)
        kc, vc = _kv_slices(kv, lay.cross, b, t, heads)
        o, _lse, _ = _attn._forward(q, kc, vc, bias_c, bstr_c, scale)
        del q
        x, _ = _post_ln(x, _linear(o.view(rows, d), lay.wo_c, lay.bo_c, lay.packed["o_c"]), lay.ln_cross, spec.eps, False)
        _h, a = _linear_gelu(x, lay.w1, lay.b1, lay.packed["fc1"], False)
        x, _ = _post_ln(x, _linear(a, lay.w2, lay.b2, lay.packed["fc2"]), lay.ln_out, spec.eps, False)
        del a, o
    return x.view(n, length, d)


class LmHeadSpec:
    """An LM head ``LayerNorm(gelu(dense(x))) @ word.t() + bias`` in the form ``lm_head_row_loss`` consumes: the dense
    weight packed by ``_pack``, the vocabulary weight packed by ``ops.gemm_pack_vocab`` (padded to a multiple of 256 rows,
    ``n_valid`` = the vocabulary) and the bias padded with it."""

    def __init__(self, dense, ln, word, bias):
        self.w, self.b, self.ln, self.eps = _c(dense.weight), _c(dense.bias), _ln(ln), ln.eps
        self.packed = _pack(self.w)
        self.vocab = ops.gemm_pack_vocab(_c(word))
        pad = self.vocab.N - self.vocab.n_valid
        self.bias = torch.cat([bias.detach().reshape(-1), bias.new_zeros(pad)]).contiguous()


def lm_head_row_loss(states, targets, head, ignore_index=-100):
    """Per-row cross entropy of the LM head on ``states`` (rows, D) against ``targets`` (rows,) int64 WITHOUT the
    (rows, vocabulary) logits: dense + GELU, LayerNorm, then ``ops.gemm_lse`` (``vqa_gemm_bf16x6_lse``)."""
    rows, d = states.shape
    _h, a = _linear_gelu(states, head.w, head.b, head.packed, False)
    y = torch.empty_like(a)
    mean = torch.empty(rows, dtype=torch.float32, device=a.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=a.device)
    ops.ln_fwd(a, head.ln[0], head.ln[1], y, mean, rstd, head.eps)
    return ops.gemm_lse(y, head.vocab, head.bias, targets, ignore_index=ignore_index)
