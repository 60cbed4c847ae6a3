"""Host side of the PGD hot path: the reference's cleverhans-style operators, re-designed for MI355X.

Same names, argument meaning, return values and error behaviour as the reference's
``cleverhans.torch.attacks.{fast_gradient_method, projected_gradient_descent}[_vl]`` (ALBEF copy:
``ALBEF_VQAttack/cleverhans/cleverhans/torch/attacks/*.py``; VLMO copy: ``VLMO_VQAttack/cleverhans/...``);
``flavor`` selects the copy where the two differ (loss definition and ``y`` slicing of the dual-loss loop).
The drop-in packages under ``vqattack_amd/dropin/`` bind ``flavor`` and re-export these under the reference's
module paths.

What is different underneath (and invisible to a caller):
  * the frozen white-box forward/backward is PyTorch-ROCm (``model_fn`` is the caller's), everything between two
    model calls is ONE hand-written HIP kernel launch (``ops.linf_step``: sign + step + clamp + eps-ball projection +
    clamp, 16 B/element instead of the reference's 92 B/element eager chain);
  * the cross-modal cosine loss and its gradient w.r.t. the model outputs come from one fused pass
    (``ops.neg_cos_rows``) and are handed to autograd as ``grad_tensors`` -- no autograd graph for the loss;
  * no per-step host sync: losses are written into a device buffer and fetched once when the loop ends (the
    reference does ``float(loss.cpu())`` every step, projected_gradient_descent.py:145); range-sanity flags are
    OR-ed into a device word by the kernels and read once;
  * the input is never cloned (the reference's ``x.clone()`` per step, fast_gradient_method.py:97): the loop owns
    two ping-pong image buffers.
There is no CPU path: CPU tensors raise ``HipExtensionError``.
"""
import os

import numpy as np
import torch

from . import ops
from ._hip import VQA_FLAG_BAD_LABEL, VQA_FLAG_DEGENERATE, VQA_FLAG_RANGE, HipExtensionError, dev_f32
from .features import LayerFeatures, layer_pairs

ALBEF = "albef"
VLMO = "vlmo"
MLM_VOCAB = 30522   # literal in the reference (fast_gradient_method.py:103)


# ----------------------------------------------------------------------------------------- validation
def _check_flavor(flavor):
    if flavor not in (ALBEF, VLMO):
        raise ValueError("flavor must be 'albef' or 'vlmo', got {!r}".format(flavor))


def _validate_fgm(norm, eps, clip_min, clip_max):
    if norm not in (np.inf, 1, 2):
        raise ValueError("Norm order must be either np.inf, 1, or 2, got {} instead.".format(norm))
    if eps < 0:
        raise ValueError("eps must be greater than or equal to 0, got {} instead".format(eps))
    if clip_min is not None and clip_max is not None and clip_min > clip_max:
        raise ValueError("clip_min must be less than or equal to clip_max, got clip_min={} and clip_max={}".format(
            clip_min, clip_max))


def _validate_pgd(norm, eps, eps_iter, clip_min, clip_max):
    """True -> hand the input back unchanged (the reference returns the bare tensor for eps/eps_iter == 0)."""
    if norm == 1:
        raise NotImplementedError("PGD with norm=1 is not enabled: norm=1 FGM changes only one pixel at a time "
                                  "(projected_gradient_descent.py:58-65 of the reference).")
    if norm not in (np.inf, 2):
        raise ValueError("Norm order must be either np.inf or 2.")
    if eps < 0:
        raise ValueError("eps must be greater than or equal to 0, got {} instead".format(eps))
    if eps == 0:
        return True
    if eps_iter < 0:
        raise ValueError("eps_iter must be greater than or equal to 0, got {} instead".format(eps_iter))
    if eps_iter == 0:
        return True
    assert eps_iter <= eps, (eps_iter, eps)
    if clip_min is not None and clip_max is not None and clip_min > clip_max:
        raise ValueError("clip_min must be less than or equal to clip_max, got clip_min={} and clip_max={}".format(
            clip_min, clip_max))
    return False


def _validate_decay(decay_factor):
    """None (momentum off) or the decay as a float; raised before any tensor is looked at, like the other arguments."""
    if decay_factor is None:
        return None
    decay = float(decay_factor)
    if not (0.0 <= decay < float("inf")):
        raise ValueError("decay_factor must be a finite number greater than or equal to 0, got {} instead".format(
            decay_factor))
    return decay


def _validate_ti(ti_kernel):
    """None (TI smoothing off) or the taps as a numpy float32 array: an odd int ``kernlen`` in 1..31 selects the TI
    paper's Gaussian taps (nsig = 3), a 1-D sequence of an odd number <= 31 of finite floats is used as the taps.
    Raised before any tensor is looked at, like the other arguments."""
    if ti_kernel is None:
        return None
    if isinstance(ti_kernel, (bool, np.bool_)):
        raise ValueError("ti_kernel must be None, an odd int in 1..31 or a 1-D sequence of taps, got {!r}".format(ti_kernel))
    if isinstance(ti_kernel, (int, np.integer)):
        k = int(ti_kernel)
        if k < 1 or k > ops.TI_MAX_TAPS or k % 2 == 0:
            raise ValueError("ti_kernel must be an odd kernel length in 1..{}, got {}".format(ops.TI_MAX_TAPS, k))
        return ops.ti_gaussian_taps(k, 3.0)
    try:
        taps = np.asarray(ti_kernel, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError("ti_kernel must be None, an odd int in 1..31 or a 1-D sequence of taps, got {!r}".format(ti_kernel))
    if taps.ndim != 1 or taps.size < 1 or taps.size > ops.TI_MAX_TAPS or taps.size % 2 == 0:
        raise ValueError("ti_kernel taps must be 1-D with an odd length in 1..{}, got shape {}".format(
            ops.TI_MAX_TAPS, taps.shape))
    if not np.all(np.isfinite(taps)):
        raise ValueError("ti_kernel taps must be finite")
    return taps


def _validate_di(diversity_prob, di_shrink=32, di_rng=None):
    """None (input diversity off; the other two keys are then ignored) or ``(prob, shrink, rng)``: ``diversity_prob`` a
    real number in [0, 1], ``di_shrink`` an int >= 1 (the reference's 32), ``di_rng`` None (``np.random``, what the
    reference's ``input_diversity`` draws from) or anything with a callable ``.uniform``.  Raised before any tensor is
    looked at, like the other arguments."""
    if diversity_prob is None:
        return None
    if isinstance(diversity_prob, (bool, np.bool_)) or not isinstance(diversity_prob, (int, float, np.integer, np.floating)):
        raise ValueError("diversity_prob must be None or a number in [0, 1], got {!r}".format(diversity_prob))
    prob = float(diversity_prob)
    if not 0.0 <= prob <= 1.0:        # False for NaN too
        raise ValueError("diversity_prob must be in [0, 1], got {!r}".format(diversity_prob))
    if isinstance(di_shrink, (bool, np.bool_)) or not isinstance(di_shrink, (int, np.integer)) or int(di_shrink) < 1:
        raise ValueError("di_shrink must be an int >= 1, got {!r}".format(di_shrink))
    if di_rng is not None and not callable(getattr(di_rng, "uniform", None)):
        raise ValueError("di_rng must be None or have a .uniform method (np.random, a RandomState, a Generator), got {!r}".format(
            di_rng))
    return prob, int(di_shrink), (np.random if di_rng is None else di_rng)


def _validate_si(si_copies, nesterov=False, decay_factor=None):
    """None (no scale copies, no look-ahead) or ``(scales, nesterov)``: ``si_copies`` an int n in 1..8 selects the SI
    paper's scales ``1, 1/2, ..., 2^-(n-1)``, a 1-D sequence of 1..8 finite positive floats is used as the scales;
    ``nesterov`` needs a decay factor (the look-ahead is ``eps_iter * decay_factor * m``) and, alone, means one copy at
    scale 1.  Raised before any tensor is looked at, like the other arguments."""
    if not isinstance(nesterov, (bool, np.bool_)):
        raise ValueError("nesterov must be a bool, got {!r}".format(nesterov))
    if nesterov and decay_factor is None:
        raise ValueError("nesterov=True needs decay_factor: the look-ahead is taken along the momentum")
    if si_copies is None:
        return (ops.si_scales(1), True) if nesterov else None
    what = "si_copies must be None, an int in 1..{} or a 1-D sequence of 1..{} finite positive scales, got {!r}".format(
        ops.SI_MAX_COPIES, ops.SI_MAX_COPIES, si_copies)
    if isinstance(si_copies, (bool, np.bool_)):
        raise ValueError(what)
    if isinstance(si_copies, (int, np.integer)):
        if int(si_copies) < 1 or int(si_copies) > ops.SI_MAX_COPIES:
            raise ValueError(what)
        return ops.si_scales(int(si_copies)), bool(nesterov)
    try:
        scales = np.asarray(si_copies, dtype=np.float32)
    except (TypeError, ValueError):
        raise ValueError(what)
    if scales.ndim != 1 or scales.size < 1 or scales.size > ops.SI_MAX_COPIES:
        raise ValueError(what)
    if not np.all(np.isfinite(scales)) or not np.all(scales > 0):
        raise ValueError(what)
    return scales, bool(nesterov)


def _validate_vt(vt_neighbors, vt_beta=1.5, vt_seed=None):
    """None (variance tuning off; the other two keys are then ignored) or ``(n, beta, seed)``: ``vt_neighbors`` an int N
    in 1..64, ``vt_beta`` a finite number > 0 (the neighbourhood is ``U[-beta * eps, beta * eps)``), ``vt_seed`` None (one
    seed is drawn from ``np.random`` when the state is built) or an int in ``[0, 2^64)``.  Raised before any tensor is
    looked at, like the other arguments."""
    if vt_neighbors is None:
        return None
    if isinstance(vt_neighbors, (bool, np.bool_)) or not isinstance(vt_neighbors, (int, np.integer)) or \
            not 1 <= int(vt_neighbors) <= ops.VT_MAX_NEIGHBORS:
        raise ValueError("vt_neighbors must be None or an int in 1..{}, got {!r}".format(ops.VT_MAX_NEIGHBORS, vt_neighbors))
    if isinstance(vt_beta, (bool, np.bool_)) or not isinstance(vt_beta, (int, float, np.integer, np.floating)) or \
            not 0.0 < float(vt_beta) < float("inf"):        # False for NaN too
        raise ValueError("vt_beta must be a finite number greater than 0, got {!r}".format(vt_beta))
    if vt_seed is not None and (isinstance(vt_seed, (bool, np.bool_)) or not isinstance(vt_seed, (int, np.integer))
                                or not 0 <= int(vt_seed) < 1 << 64):
        raise ValueError("vt_seed must be None or an int in [0, 2^64), got {!r}".format(vt_seed))
    return int(vt_neighbors), float(vt_beta), (None if vt_seed is None else int(vt_seed))


def _validate_admix(admix_images, admix_eta=0.2, admix_rng=None):
    """None (no mixing; the other two keys are then ignored) or ``(images, eta, rng)``: ``admix_images`` an int m2 in
    1..8, ``admix_eta`` a finite number >= 0 (the partner's share), ``admix_rng`` None (``np.random``) or anything with a
    callable ``.uniform``, as ``di_rng``.  Raised before any tensor is looked at, like the other arguments."""
    if admix_images is None:
        return None
    if isinstance(admix_images, (bool, np.bool_)) or not isinstance(admix_images, (int, np.integer)) or \
            not 1 <= int(admix_images) <= ops.ADMIX_MAX_IMAGES:
        raise ValueError("admix_images must be None or an int in 1..{}, got {!r}".format(ops.ADMIX_MAX_IMAGES, admix_images))
    if isinstance(admix_eta, (bool, np.bool_)) or not isinstance(admix_eta, (int, float, np.integer, np.floating)) or \
            not 0.0 <= float(admix_eta) < float("inf"):        # False for NaN too
        raise ValueError("admix_eta must be a finite number greater than or equal to 0, got {!r}".format(admix_eta))
    if admix_rng is not None and not callable(getattr(admix_rng, "uniform", None)):
        raise ValueError("admix_rng must be None or have a .uniform method (np.random, a RandomState, a Generator), "
                         "got {!r}".format(admix_rng))
    return int(admix_images), float(admix_eta), (np.random if admix_rng is None else admix_rng)


def _admix_batch(aspec, x):
    """Admix mixes every sample with ANOTHER sample of the batch: a batch of one is refused before any launch."""
    if aspec is not None:
        shape = getattr(x, "shape", None)
        if shape is None or len(shape) < 1 or shape[0] < 2:
            raise ValueError("admix_images needs a batch of at least 2 samples (every sample is mixed with another one "
                             "of the batch), got shape {}".format(None if shape is None else tuple(shape)))


def _two_sided(clip_min, clip_max):
    if (clip_min is not None or clip_max is not None) and (clip_min is None or clip_max is None):
        raise ValueError("One of clip_min and clip_max is None but we don't currently support one-sided clipping")


def _as_image(x, name="x"):
    if not isinstance(x, torch.Tensor):
        raise TypeError("{} must be a torch.Tensor".format(name))
    if not x.is_cuda:
        raise HipExtensionError("{} is on '{}': vqattack_amd runs this path on an MI355X HIP device only "
                                "(no CPU fallback)".format(name, x.device))
    x = x.detach()
    if x.dtype != torch.float32:
        x = x.to(torch.float32)          # reference: .to(torch.float), fast_gradient_method.py:97
    return x.contiguous()


# ----------------------------------------------------------------------------------------- losses
class _LossSlot:
    """One fp32 word of the attack's device-side loss buffer."""

    def __init__(self, buf, index):
        self.word = buf[index:index + 1]


def _feature_pairs(out, y, flavor, vl):
    """(model output, target) row-tensor pairs of the feature loss, after the reference's in-place truncation of
    both LISTS to the common token length (A: fast_gradient_method.py:121-126; V: :107-110)."""
    if flavor == ALBEF:
        n1 = min(out[1].shape[1], y[1].shape[1])
        out[1] = out[1][:, :n1, :]
        y[1] = y[1][:, :n1, :]
        n0 = min(out[0].shape[1], y[0].shape[1])
        out[0] = out[0][:, :n0, :]
        y[0] = y[0][:, :n0, :]
        return [(out[1], y[1]), (out[0], y[0])]
    if vl or out[2].shape[1] != y[2].shape[1]:
        n = min(out[2].shape[1], y[2].shape[1])
        out[2] = out[2][:, :n, :]
        y[2] = y[2][:, :n, :]
    if out[1] is None:      # batched adapter: the per-layer [CLS] rows ride in out[2] with row weight 2
        return [(out[2], y[2])]
    return [(out[1], y[1]), (out[2], y[2])]


def _feature_loss_backward(pairs, slot, leaves, sign, extra_scale=1.0, extra=None, ws=None):
    """Fused loss + gradient: one HIP pass per pair, then autograd through the model only.

    loss = sign * extra_scale * sum_pairs sum_rows -cos (+ whatever ``extra()`` adds).  ``extra`` is an optional
    callable that accumulates further terms into the slot and returns ``(tensors, grads)`` to back-propagate in the
    same autograd sweep (the CE terms of the VLMO mixed loss).
    """
    tensors, grads = [], []
    gscale = sign * extra_scale
    first = True
    for pair_index, (o_pair, t_pair) in enumerate(pairs):
        trips = layer_pairs(o_pair, t_pair)                 # per-layer (out, target, row weight)
        outs, tgts = [], []
        for (o, t, _) in trips:
            if not o.is_cuda or not t.is_cuda:
                raise HipExtensionError("model_fn outputs and targets y must be on the HIP device")
            outs.append(o if o.dtype == torch.float32 else o.to(torch.float32))
            tgts.append(t.detach() if t.dtype == torch.float32 else t.detach().to(torch.float32))
        w = trips[0][2]
        period = outs[0].shape[0] if w is not None else 1
        # layers that do not depend on a leaf (ALBEF text states below the fusion layer during image-only steps)
        # still contribute their constant to the loss value, but need no gradient pass
        for needs_grad in (True, False):
            idx = [i for i, o in enumerate(outs) if o.requires_grad == needs_grad]
            if not idx:
                continue
            ga = ops.neg_cos_rows_multi([outs[i].detach() for i in idx], [tgts[i] for i in idx], slot.word,
                                        accumulate=not first, gscale=gscale, want_grad=needs_grad, row_weight=w,
                                        weight_period=period,      # ONE launch for all layers of this modality
                                        ws=None if ws is None else ops.SubWorkspace(ws, pair_index))
            first = False
            if needs_grad:
                tensors += [outs[i] for i in idx]
                grads += ga
    if extra is not None:
        more_t, more_g = extra()
        tensors += more_t
        grads += more_g
    if not tensors:
        raise RuntimeError("model_fn's outputs do not depend on the attacked input (nothing requires grad)")
    torch.autograd.backward(tensors, grads, inputs=leaves)


def _label_sets(labels):
    """(K, rows) int64 label sets of the reference's MLM labels: 2-d (B, L) -> K = 1; 3-d (B, K, L) -> one set per
    k, summed (A: fast_gradient_method.py:131-142; V: :116-126).  `reshape` where the reference's `view` would reject
    the non-contiguous slice for batch > 1."""
    if labels.dim() == 2:
        return labels.reshape(1, -1)
    if labels.dim() == 3:
        return labels.permute(1, 0, 2).reshape(labels.shape[1], -1)
    raise ValueError("MLM labels must be 2-d or 3-d")


def _ce_backward(logits, label_sets, slot, leaves, sign, scale=1.0, accumulate=False, flag=None, ws=None,
                 per_sample=False):
    """Fused cross entropy: loss into ``slot``; returns ``(tensors, grads)`` for the autograd sweep (one HIP launch).
    ``per_sample``: normalise every label set by each SAMPLE's own valid-label count (batched drivers: per-sample
    gradients then equal the batch-1 reference's) instead of ``F.cross_entropy``'s mean over the whole batch."""
    rows_per_sample = logits.shape[1] if (per_sample and logits.dim() == 3) else 0
    if logits.shape[-1] != MLM_VOCAB:
        logits = logits.reshape(-1, MLM_VOCAB)          # the reference's .view(-1, 30522)
    l32 = logits if logits.dtype == torch.float32 else logits.to(torch.float32)
    needs_grad = l32.requires_grad
    g = ops.mlm_cross_entropy(l32.detach(), label_sets, slot.word, accumulate=accumulate, gscale=sign * scale,
                              want_grad=needs_grad, flag=flag, ws=ws, rows_per_sample=rows_per_sample)
    return ([l32], [g]) if needs_grad else ([], [])


def _loss_and_grad(model_fn, leaves, model_in, y, ls, flavor, targeted, slot, bkp=None, bkp_y=None, vl=False,
                   ws=None, flag=None, per_sample=False):
    """Run the white box, evaluate the selected loss into ``slot`` and leave d loss/d leaf in ``leaf.grad``.
    ``ws`` (``ops.Workspace``): gradient / scratch buffers reused across the iterations of one attack call;
    ``flag``: the attack's int32 device word (bad MLM labels are reported there, see ``ops.mlm_cross_entropy``)."""
    sign = -1.0 if targeted else 1.0
    with torch.enable_grad():
        out = model_fn(model_in)
        if vl:
            pairs = _feature_pairs(out, y, flavor, vl=True)     # truncation happens before the `ls` switch
            if ls == 1:
                _feature_loss_backward(pairs, slot, leaves, sign, ws=ws)
            elif ls == 0:
                t, g = _ce_backward(out[0], y[0].reshape(1, -1), slot, leaves, sign, flag=flag, ws=ws,
                                    per_sample=per_sample)
                torch.autograd.backward(t, g, inputs=leaves)
            else:
                raise UnboundLocalError("loss is undefined for ls={!r} (as in the reference)".format(ls))
            return
        if flavor == ALBEF and ls == 0:
            # label/logit length mismatch -> feature loss on the backup model (fast_gradient_method.py:102-118)
            rows = out[0].reshape(-1, MLM_VOCAB).shape[0]
            lab = y[0]
            if lab.dim() == 2:
                bad = lab.reshape(-1).shape[0] != rows
            elif lab.dim() == 3:
                bad = any(lab[:, k, :].reshape(-1).shape[0] != rows for k in range(lab.shape[1]))
            else:
                bad = False
            if bad:
                ls, out, y = 1, bkp(model_in), bkp_y
        if ls == 1:
            _feature_loss_backward(_feature_pairs(out, y, flavor, vl=False), slot, leaves, sign, ws=ws)
        elif ls == 0:
            t, g = _ce_backward(out[0], _label_sets(y[0]), slot, leaves, sign, flag=flag, ws=ws, per_sample=per_sample)
            if not t:
                raise RuntimeError("model_fn's logits do not depend on the attacked input")
            torch.autograd.backward(t, g, inputs=leaves)
        elif flavor == VLMO:
            # mixed loss, V: fast_gradient_method.py:127-131 (no truncation in this branch): feature loss / (13*Ntok)
            # + 0.1 * CE(labels) + 0.1 * sum over synonym label sets -- all CE terms in ONE fused launch
            if isinstance(out[2], LayerFeatures) and out[2].layers[0].shape[0] > 1:
                _vlmo_mixed_batched(out, y, slot, leaves, sign, flag, ws)
                return
            sets = torch.cat([y[0].reshape(1, -1)] + [syn[0].reshape(1, -1) for syn in y[3]], dim=0)
            scale = 1.0 / (out[2].shape[0] * out[2].shape[1])
            pairs = [(out[2], y[2])] if out[1] is None else [(out[1], y[1]), (out[2], y[2])]
            _feature_loss_backward(pairs, slot, leaves, sign, extra_scale=scale, ws=ws,
                                   extra=lambda: _ce_backward(out[0], sets, slot, leaves, sign, scale=0.1,
                                                              accumulate=True, flag=flag, ws=ws))
        else:
            raise UnboundLocalError("loss is undefined for ls={!r} (as in the reference)".format(ls))


def _vlmo_mixed_batched(out, y, slot, leaves, sign, flag, ws):
    """The VLMO mixed loss (``ls`` not in {0, 1}; V: fast_gradient_method.py:127-131 -- never reached by the reference's
    drivers) for a BATCHED ``LayerFeatures`` output.  The reference weighs the three terms per sample (batch 1):
    ``feature loss / (layers * Ntok)`` with that sample's own token count, ``0.1 * CE`` means over that sample's labels.
    Per sample b of the batch: the feature gradient comes from the usual ONE launch over all maps and is then scaled by
    ``1 / (layers * Ntok_b)`` row-block by row-block; the loss value is accumulated by one small loss-only launch per
    sample; the cross-entropy terms are normalised per sample (``rows_per_sample``).  A rare path: written for
    correctness, not for speed."""
    lf, tgt = out[2], y[2]
    if not isinstance(tgt, LayerFeatures):
        raise ValueError("the batched VLMO mixed loss takes LayerFeatures targets")
    layers = [t if t.dtype == torch.float32 else t.to(torch.float32) for t in lf.layers]
    targets = [t.detach() for t in tgt.layers]
    b, n = layers[0].shape[0], layers[0].shape[1]
    w = lf.row_weight if lf.row_weight is not None else tgt.row_weight
    ntok = [n] * b if w is None else [int(v) for v in (w != 0).sum(dim=1).tolist()]       # one host read (rare path)
    scales = [1.0 / (len(layers) * max(v, 1)) for v in ntok]
    scale = torch.tensor(scales, dtype=torch.float32, device=layers[0].device)
    grads = ops.neg_cos_rows_multi([t.detach() for t in layers], targets, None, accumulate=False, gscale=sign,
                                   want_grad=True, row_weight=w, weight_period=b if w is not None else 1, ws=ws)
    for g in grads:
        g.mul_(scale.view(b, 1, 1))
    for s in range(b):                                   # the loss VALUE: sum_b scale_b * (feature loss of sample b)
        ops.neg_cos_rows_multi([t[s:s + 1].detach() for t in layers], [t[s:s + 1] for t in targets], slot.word,
                               accumulate=s > 0, gscale=sign * scales[s], want_grad=False,
                               row_weight=None if w is None else w[s:s + 1].contiguous(), weight_period=1)
    sets = torch.cat([y[0].reshape(1, -1)] + [syn[0].reshape(1, -1) for syn in y[3]], dim=0)
    more_t, more_g = _ce_backward(out[0], sets, slot, leaves, sign, scale=0.1, accumulate=True, flag=flag, ws=ws,
                                  per_sample=True)
    torch.autograd.backward(list(layers) + more_t, list(grads) + more_g, inputs=leaves)


def _mixed_loss_and_grad(model_fn, leaves, model_in, y, flavor, slot, mlm_labels=None, ws=None, flag=None):
    """One white-box call for a batch whose samples stand at DIFFERENT steps of their own schedules (``attack_mixed``).

    ``model_fn(model_in) -> (out, logits)``: ``out`` is the feature list of ``pgd_attack_vl`` with the rows of the samples
    that take an MLM step this time weighted 0 (or None when every sample does), ``logits`` (n_mlm, W, V) the MLM head
    at the live label positions of those samples (or None when there are none), ``mlm_labels`` their compact labels
    (n_mlm, W) / (n_mlm, K, W).  Every sample's loss is one of the two terms of the reference's dual loop (feature loss
    A fast_gradient_method.py:120-127 / V :106-114, or MLM cross entropy A :128-142 / V :115-126, normalised per sample);
    samples do not interact in a frozen eval-mode network, so one backward of the SUM leaves each sample's own gradient
    in its slice of ``leaf.grad``."""
    with torch.enable_grad():
        out, logits = model_fn(model_in)
        ce = None
        if logits is not None:
            sets = _label_sets(mlm_labels)

            def ce(accumulate=True):
                return _ce_backward(logits, sets, slot, leaves, 1.0, accumulate=accumulate, flag=flag, ws=ws,
                                    per_sample=True)
        if out is not None:
            _feature_loss_backward(_feature_pairs(out, y, flavor, vl=True), slot, leaves, 1.0, ws=ws, extra=ce)
        elif ce is not None:
            t, g = ce(accumulate=False)
            if not t:
                raise RuntimeError("model_fn's logits do not depend on the attacked input")
            torch.autograd.backward(t, g, inputs=leaves)
        else:
            raise RuntimeError("mixed model_fn returned neither features nor logits")


# ----------------------------------------------------------------------------------------- image updates
class _Momentum:
    """The MI-FGSM state of one operator call: the momentum tensor (the caller's, updated in place, or zeros), the decay
    and -- allocated once, so that a captured iteration finds them at static addresses -- one |grad| sum per sample and
    the reduction's workspace."""

    def __init__(self, decay, like, momentum=None):
        if momentum is None:
            momentum = torch.zeros_like(like, memory_format=torch.contiguous_format)
        else:
            dev_f32(momentum, "momentum")
            if momentum.shape != like.shape or momentum.device != like.device:
                raise ValueError("momentum has shape {} on {}, expected {} on {}".format(
                    tuple(momentum.shape), momentum.device, tuple(like.shape), like.device))
        self.decay, self.m = decay, momentum
        self.sumabs = torch.empty(like.shape[0] if like.dim() > 0 else 1, dtype=torch.float32, device=like.device)
        self.ws = ops.reduce_workspace(like)

    def sums(self, grad):
        return ops.sumabs_per_sample(grad, out=self.sumabs, ws=self.ws)


class _Smoother:
    """The TI-FGSM state of one operator call: the taps and -- allocated once, so that a captured iteration finds it at a
    static address -- one tensor for the smoothed gradient.  ``scratch=False``: the update only runs the fused L-inf step
    (``ops.linf_ti_step``), which keeps the smoothed gradient in registers."""

    def __init__(self, taps, like, scratch):
        self.taps = taps
        self.ghat = torch.empty_like(like, memory_format=torch.contiguous_format) if scratch else None


class _Diversity:
    """The DI-FGSM state of one operator call: the geometry rows of ALL its gradient evaluations, drawn once on the host
    and uploaded in one copy (``(n_evals, B, 4)``), one static ``(B, 4)`` row for a captured iteration, the transformed
    image and -- unless the update only runs the fused L-inf step (``ops.linf_di_step``) -- the adjoint's result."""

    def __init__(self, spec, like, n_evals, scratch):
        prob, shrink, rng = spec
        b, _, h, w = like.shape
        self.table = ops.di_geometry(ops.di_draw(rng, b, n_evals, h, w, shrink, prob), h, w, like.device)
        self.row = torch.empty((b, 4), dtype=torch.int32, device=like.device)
        self.image = torch.empty_like(like, memory_format=torch.contiguous_format)
        self.grad = torch.empty_like(like, memory_format=torch.contiguous_format) if scratch else None
        self.geom, self.n = None, 0

    def use(self, i, static=False):
        """Make evaluation ``i``'s rows current: in place in the table, or (``static``) copied into the static row."""
        if static:
            self.row.copy_(self.table[i])
        self.geom = self.row if static else self.table[i]


class _Scales:
    """The SI-NI-FGSM state of one operator call: scales and weights on the host and -- allocated once, so that a
    captured iteration finds them at static addresses -- the scaled copies the model sees, their DI transforms when
    there is input diversity, one word for the losses of the copies after the first and, unless the update only runs the
    fused L-inf step (``ops.linf_si_step``), the combined gradient.  ``mom``: look ahead along its momentum (Nesterov)."""

    def __init__(self, spec, like, eps_iter, mom, di, scratch):
        scales, nesterov = spec
        self.scales, self.weights = scales, ops.si_weights(scales)
        self.mom = mom if nesterov else None
        self.lookahead = float(eps_iter) * mom.decay if nesterov else 0.0
        shape = (len(scales),) + tuple(like.shape)
        self.images = torch.empty(shape, dtype=torch.float32, device=like.device)
        self.transformed = torch.empty(shape, dtype=torch.float32, device=like.device) if di is not None else None
        self.ghat = torch.empty_like(like, memory_format=torch.contiguous_format) if scratch else None
        self.slot = _LossSlot(torch.zeros(1, dtype=torch.float32, device=like.device), 0)


class _Variance:
    """The variance-tuning (VMI / VNI-FGSM) state of one operator call, all of it allocated before the loop so that a
    captured iteration finds it at static addresses: one variance tensor ``v`` per evaluation kind (the dual loop's
    feature and MLM evaluations each tune their own), the running sum of the neighbours' gradients, the centre's
    x-space gradient / the tuned gradient, a chunk of ``min(N, 8)`` neighbour images, the key table of all the call's
    evaluations (row ``t`` = seed and ``t``, one upload), one static key row for a captured iteration and one word for
    the neighbours' losses."""

    def __init__(self, spec, like, eps, n_evals, kinds=1):
        n, beta, seed = spec
        if seed is None:
            seed = (int(np.random.randint(0, 1 << 32)) << 32) | int(np.random.randint(0, 1 << 32))
        self.n, self.seed = n, seed
        self.w = float(np.float32(1.0) / np.float32(n))
        self.bound = float(np.float32(beta * float(eps)))
        self.v = [torch.zeros_like(like, memory_format=torch.contiguous_format) for _ in range(kinds)]
        self.vsum = torch.empty_like(like, memory_format=torch.contiguous_format)
        self.ghat = torch.empty_like(like, memory_format=torch.contiguous_format)
        self.chunk = torch.empty((min(n, ops.VT_MAX_CHUNK),) + tuple(like.shape), dtype=torch.float32, device=like.device)
        self.table = ops.vt_key_table(seed, n_evals, like.device)
        self.row = torch.empty(3, dtype=torch.uint32, device=like.device)
        self.slot = _LossSlot(torch.zeros(1, dtype=torch.float32, device=like.device), 0)
        self.key, self.t, self.kind = None, 0, 0

    def use(self, t, static=False):
        """Make evaluation ``t``'s key current: in place in the table, or (``static``) copied into the static row."""
        if static:
            self.row.copy_(self.table[t])
        self.key = self.row if static else self.table[t]


class _Admix:
    """The Admix state of one operator call: the partner table of ALL its gradient evaluations, drawn once on the host and
    uploaded in one copy (``(n_evals, m2, B)``), one static ``(m2, B)`` row for a captured iteration, the current rows
    and -- with more than one mixed group -- the running sum ``gsum`` of the groups' weighted gradients.  ``acc``: where
    the evaluation under way keeps that sum (``gsum``, or the tensor its caller named)."""

    def __init__(self, spec, like, n_evals):
        self.images, self.eta, rng = spec
        b = like.shape[0]
        self.table = ops.admix_partners(ops.admix_draw(rng, b, n_evals, self.images), b, like.device)
        self.row = torch.empty((self.images, b), dtype=torch.int32, device=like.device)
        self.gsum = torch.empty_like(like, memory_format=torch.contiguous_format) if self.images > 1 else None
        self.rows, self.acc, self.n = None, self.gsum, 0

    def use(self, i, static=False):
        """Make evaluation ``i``'s rows current: in place in the table, or (``static``) copied into the static row."""
        if static:
            self.row.copy_(self.table[i])
        self.rows = self.row if static else self.table[i]


def _validate_stages(decay_factor=None, ti_kernel=None, diversity_prob=None, di_shrink=32, di_rng=None, si_copies=None,
                     nesterov=False, vt_neighbors=None, vt_beta=1.5, vt_seed=None):
    """The transfer keywords of an operator call as the specs ``_Chain`` takes (None: that stage is off), validated in
    this order and before any tensor is looked at."""
    return (_validate_decay(decay_factor), _validate_ti(ti_kernel), _validate_di(diversity_prob, di_shrink, di_rng),
            _validate_si(si_copies, nesterov, decay_factor), _validate_vt(vt_neighbors, vt_beta, vt_seed))


class _Chain:
    """The optional transfer stages of one operator call -- momentum, TI, DI, SI / NI, variance tuning, each None or its
    state above -- and the ONE statement of how a gradient evaluation and an image update run through them.

    The rule: the stages of an update run in the order SI combine, DI adjoint, VT tune, TI smooth, momentum.  With the
    L-inf norm the last active one runs inside the update's own launch (``ops.linf_*_step``), variance tuning only on a
    gradient that no SI / DI had to take to x space first; every other active stage writes into a scratch of its own,
    allocated here, once, so that a captured iteration finds it at a static address.  ``fused`` names that last stage.

    Built from ``_validate_stages``' specs in the order momentum, TI, DI, SI, VT: DI draws its rows and VT (without a seed)
    its seed from ``np.random``, in that order.  ``like``: the image; ``n_evals``: gradient evaluations of the call;
    ``kinds``: evaluation kinds that tune a variance of their own; ``momentum``: the caller's tensor or None (zeros).
    Without specs it is the plain update and touches no tensor of its own.

    ``admix`` (``_validate_admix``'s spec, None: off): Admix runs in SI's place in the order above.  Every evaluation sees
    m2 mixed groups of the m1 scale copies (without ``si_copies``: one copy at scale 1), in ascending group order, each
    group's copies from one launch (``ops.admix_copies``) into SI's image buffer; the weights are ``s_i / (m1 * m2)``.
    The groups 0 .. m2-2 are folded into the running sum as soon as their m1 model calls have returned --
    ``ops.si_combine`` for group 0, ``ops.admix_accumulate`` behind it -- so at most m1 images and m1 gradients are live;
    the last group's gradients are handed on with the sum, and the update folds them in its own launch
    (``ops.linf_admix_step``) where SI / Admix is the last active stage under L-inf, else through
    ``ops.admix_accumulate`` in front of the DI adjoint, VT, TI, momentum and the L2 update.  With m2 = 1 there is no
    running sum and every launch behind the model is SI's.  All copies and all VT neighbours of an evaluation share its
    partner rows (a neighbour tensor is mixed with its own samples) and its DI rows; the partner table is drawn after
    DI's rows and VT's seed.  ``call(leaf, first)`` gets ``first=True`` for the first copy of the first group only: the
    reported loss is that mixed copy's.  The leaves of all groups share SI's image buffer, so a leaf is valid until the
    next group's copies are written.

    The mixed-schedule driver runs one chain on row subsets of its state: ``leaves(.., n=)`` on the active batch prefix,
    ``update(.., rows=(lo, hi))`` on one run of samples."""

    def __init__(self, specs=(None,) * 5, like=None, norm=np.inf, eps=0.0, eps_iter=0.0, n_evals=1, kinds=1,
                 momentum=None, admix=None):
        decay, taps, dspec, sspec, vspec = specs
        if admix is not None:
            _admix_batch(admix, like)
            if sspec is None:
                sspec = (ops.si_scales(1), False)              # one copy at scale 1 per mixed image
        active = [name for name, spec in (("si", sspec), ("di", dspec), ("vt", vspec), ("ti", taps), ("mom", decay))
                  if spec is not None]
        self.norm = norm
        self.fused = active[-1] if active and norm == np.inf else None
        if self.fused == "vt" and len(active) > 1:
            self.fused = None
        self.plain = sspec is None and dspec is None           # a leaf's gradient is in x space as it is
        self.mom = None if decay is None else _Momentum(decay, like, momentum)
        for spec, key, what in ((taps, "ti_kernel", "stencil"), (dspec, "diversity_prob", "transform")):
            if spec is not None and like.dim() != 4:
                raise ValueError("{} needs a (B, C, H, W) image: the {} runs over its (H, W) planes, got shape {}".format(
                    key, what, tuple(like.shape)))
        self.ti = None if taps is None else _Smoother(taps, like, self.fused != "ti")
        self.di = None if dspec is None else _Diversity(dspec, like, n_evals, self.fused != "di")
        multi = admix is not None and admix[0] > 1             # a running sum takes the place of SI's scratch
        self.si = None if sspec is None else _Scales(sspec, like, eps_iter, self.mom, self.di,
                                                     self.fused != "si" and not multi)
        self.vt = None if vspec is None else _Variance(vspec, like, eps, n_evals, kinds)
        self.ax = None if admix is None else _Admix(admix, like, n_evals)
        if self.ax is not None:
            self.si.weights = ops.admix_weights(self.si.scales, self.ax.images)
        # the word that takes the losses nobody reports: those of the scale copies after the first and of the neighbours
        self.slot = self.si.slot if self.si is not None else (self.vt.slot if self.vt is not None else None)

    def use(self, i, static=False):
        """Make DI's rows, VT's key and Admix's partner rows of evaluation ``i`` current (``static``: copied to their
        static addresses)."""
        if self.di is not None:
            self.di.use(i, static)
        if self.vt is not None:
            self.vt.use(i, static)
        if self.ax is not None:
            self.ax.use(i, static)

    def leaves(self, adv, advance=True, ahead=True, n=None):
        """The leaves the model sees for one gradient evaluation at ``adv``, made one at a time: ``adv`` itself or its DI
        transform (the next evaluation's rows unless ``advance=False``); with SI the scaled copies from one launch, in
        ascending order -- all copies of an evaluation share its DI rows, so the adjoint is linear over them and the
        combination may precede it.  ``ahead=False``: no Nesterov look-ahead in front of the copies (``adv`` is a
        variance-tuning neighbour, drawn around the look-ahead point already).  ``n``: ``adv`` is the batch prefix
        ``[:n]``; the state is sliced to match.  With Admix the copies of one mixed group after the other, each group
        from one launch into the same buffer (no batch prefix: the partners are samples of the whole batch)."""
        si, di, ax = self.si, self.di, self.ax
        head = (lambda t: t) if n is None else (lambda t: t[:n])
        if di is not None and advance:
            di.use(di.n)
            di.n += 1
        if si is None:
            seen = adv if di is None else ops.di_transform(adv, head(di.geom), out=head(di.image))
            yield seen.detach().requires_grad_(True)
            return
        m = head(si.mom.m) if ahead and si.mom is not None else None
        if ax is not None:
            if n is not None:
                raise ValueError("Admix mixes samples of the whole batch: no batch prefix")
            if advance:
                ax.use(ax.n)
                ax.n += 1
        for j in range(1 if ax is None else ax.images):
            if ax is None:
                images = ops.si_copies(adv, si.scales, m=m, lookahead=0.0 if m is None else si.lookahead,
                                       out=si.images if n is None else si.images[:, :n])
            else:
                images = ops.admix_copies(adv, ax.rows[j], si.scales, ax.eta, m=m,
                                          lookahead=0.0 if m is None else si.lookahead, out=si.images)
            for i in range(images.shape[0]):
                seen = images[i] if di is None else ops.di_transform(images[i], head(di.geom), out=head(si.transformed[i]))
                yield seen.detach().requires_grad_(True)

    def _gradient(self, adv, call, advance=True, ahead=True, acc=None):
        """``call(leaf, first)`` on every leaf in turn: it runs the white box and the loss and leaves the gradient in
        ``leaf.grad``.  Returns the leaf's gradient, with SI the list of the copies' gradients; with Admix the list of the
        LAST group's, the groups before it folded into the running sum (``acc``, None: the state's ``gsum``) one by one."""
        ax, grads = self.ax, []
        multi = ax is not None and ax.images > 1
        if multi:
            ax.acc = ax.gsum if acc is None else acc
            m1, last = len(self.si.scales), len(self.si.scales) * ax.images - 1
        for i, leaf in enumerate(self.leaves(adv, advance, ahead)):
            call(leaf, i == 0)
            grads.append(_grad_of(leaf))
            if multi and len(grads) == m1 and i < last:
                if i < m1:
                    ops.si_combine(grads, self.si.weights, out=ax.acc)
                else:
                    ops.admix_accumulate(grads, self.si.weights, ax.acc)
                grads = []
        return grads if self.si is not None else grads[0]

    def _x_gradient(self, grad, out=None):
        """``G`` of variance tuning: what ``_gradient`` returned, taken to x space -- the SI combination, then the DI
        adjoint, each into its own scratch (the last one into ``out`` when given); without either the leaf's gradient."""
        si, di, ax = self.si, self.di, self.ax
        if ax is not None and ax.images > 1:   # in place in the running sum, which is ``out`` where nothing follows
            ops.admix_accumulate(grad, si.weights, ax.acc)
            grad = ax.acc
        elif si is not None:
            grad = ops.si_combine(grad, si.weights, out=si.ghat if (out is None or di is not None) else out)
        if di is not None:
            grad = ops.di_adjoint(grad, di.geom, out=di.grad if out is None else out)
        return grad

    def evaluate(self, adv, call, kind=0, advance=True):
        """One gradient evaluation at ``adv`` in the form ``update`` expects.  Without variance tuning: ``_gradient``.
        With it: the centre through ``_gradient``, then the ``vt.n`` neighbours ``p + r_i`` (``p`` the look-ahead point with
        Nesterov) in chunks of at most 8 images per launch through the same ``_gradient``, every one with the centre's DI
        rows and ``call(leaf, False)`` (their losses go to the scratch word).  Without SI / DI up to 8 leaf gradients are
        summed per launch; with either each neighbour's gradient is combined / adjoint-ed into its scratch and summed one
        at a time -- the same bits.  Leaves ``sum_i G(p + r_i)`` in ``vt.vsum`` and returns ``G(p)``, in x space; ``kind``
        selects the variance the update tunes."""
        si, vt, ax = self.si, self.vt, self.ax
        if vt is None:
            return self._gradient(adv, call, advance)
        if advance:
            vt.use(vt.t)
            vt.t += 1
        vt.kind = kind
        # the centre's running sum must outlive the neighbours': it is kept where G(p) ends up unless DI's adjoint follows
        acc = vt.ghat if ax is not None and ax.images > 1 and self.di is None else None
        g = self._x_gradient(self._gradient(adv, call, advance, acc=acc), out=vt.ghat)
        m, lookahead = (si.mom.m, si.lookahead) if si is not None and si.mom is not None else (None, 0.0)

        def other(leaf, _):
            call(leaf, False)

        for start in range(0, vt.n, ops.VT_MAX_CHUNK):
            count = min(ops.VT_MAX_CHUNK, vt.n - start)
            images = ops.vt_neighbors(adv, vt.key, count, vt.bound, first=start, m=m, lookahead=lookahead,
                                      out=vt.chunk[:count])
            grads = []
            for c in range(count):
                gn = self._gradient(images[c], other, advance=False, ahead=False)
                if self.plain:
                    grads.append(gn)
                else:
                    ops.vt_accumulate([self._x_gradient(gn)], vt.vsum, init=start + c == 0)
            if grads:
                ops.vt_accumulate(grads, vt.vsum, init=start == 0)
        return g

    def update(self, x, grad, x0, eps_iter, eps, clip_min, clip_max, out=None, flag=None, check_range=True, rows=None):
        """One image update along ``grad`` (what ``evaluate`` returned).  ``x0=None`` is the FGM form, ``x + eps_iter *
        direction`` clamped; otherwise the step form, projected onto the ``eps``-ball around ``x0`` as well.
        ``flag``: the FGM form reports range violations of ``x`` there (``check_range``) and, for L2 / L1, the
        degenerate-gradient bit that stands for the self-check asserts of the reference's ``optimize_linear``
        (utils.py:101-104, :110-116); the step form's L2 update reports the degenerate bit only.
        ``rows=(lo, hi)``: the update of that run of samples -- ``x``, ``grad``, ``x0``, ``out`` and the state are sliced."""
        cut = (lambda t: t) if rows is None else (lambda t: t[rows[0]:rows[1]])
        fgm = x0 is None
        x, x0, out = cut(x), None if fgm else cut(x0), None if out is None else cut(out)
        grad = [cut(g) for g in grad] if isinstance(grad, list) else cut(grad)
        step = (eps_iter, 0.0 if fgm else eps, clip_min, clip_max)
        tail = dict(flag=flag if fgm and check_range else None, out=out)     # what every L-inf kernel takes last
        si, di, vt, ti, mom = self.si, self.di, self.vt, self.ti, self.mom
        multi = self.ax is not None and self.ax.images > 1
        if multi and rows is not None:
            raise ValueError("Admix keeps one running sum for the whole batch: no update of a run of samples")
        if vt is not None:            # ``grad`` is G(p), in x space already: SI and DI are done with
            if self.fused == "vt":
                return ops.linf_vt_step(x, grad, vt.vsum, vt.v[vt.kind], x0, vt.w, *step, **tail)
            grad = ops.vt_tune(grad, vt.vsum, vt.v[vt.kind], vt.w, out=vt.ghat)
        else:
            if self.fused == "si" and multi:
                return ops.linf_admix_step(x, self.ax.acc, grad, x0, si.weights, *step, **tail)
            if self.fused == "si":
                return ops.linf_si_step(x, grad, x0, si.weights, *step, **tail)
            if multi:
                ops.admix_accumulate(grad, si.weights, self.ax.acc)
                grad = self.ax.acc
            elif si is not None:
                grad = ops.si_combine(grad, si.weights, out=cut(si.ghat))
            if self.fused == "di":
                return ops.linf_di_step(x, grad, x0, cut(di.geom), *step, **tail)
            if di is not None:
                grad = ops.di_adjoint(grad, cut(di.geom), out=cut(di.grad))
        if self.fused == "ti":
            return ops.linf_ti_step(x, grad, x0, ti.taps, *step, **tail)
        if ti is not None:
            grad = ops.ti_smooth(grad, ti.taps, out=cut(ti.ghat))
        if mom is not None:
            # a run of samples leaves the |grad| sums to the kernel's wrapper: the call's reduction workspace is sized for
            # the whole batch, and a smaller batch may need a larger one (vqa_reduce_ws_bytes)
            sums = mom.sums(grad) if rows is None else None
            if self.fused == "mom":
                return ops.linf_momentum_step(x, grad, x0, cut(mom.m), mom.decay, *step, sumabs=sums, **tail)
            grad = ops.momentum_accumulate(grad, cut(mom.m), mom.decay, sumabs=sums)
        if self.norm == np.inf:
            if fgm:
                return ops.linf_fgm(x, grad, eps_iter, clip_min, clip_max, **tail)
            return ops.linf_step(x, grad, x0, *step, **tail)
        if fgm:
            l_fgm = ops.l2_fgm if self.norm == 2 else ops.l1_fgm
            return l_fgm(x, grad, eps_iter, clip_min, clip_max, flag=flag, out=out, check_range=check_range)
        mid = ops.l2_fgm(x, grad, eps_iter, clip_min, clip_max, flag=flag, check_range=False)
        return ops.l2_project(mid, x0, eps, clip_min, clip_max, out=out)


def _check_flag(flag, norm, sanity_checks):
    """The one host read of an operator call's flag word.  Two bits are the reference's UNCONDITIONAL failures and are
    raised whenever the word is read at all (norm 1 / 2, or ``sanity_checks``): the degenerate-gradient bit
    (``optimize_linear``'s own ``assert``, utils.py:101-104,110-116) and the bad-MLM-label bit (``F.cross_entropy`` with
    a target outside the vocabulary never returns in the reference -- IndexError on the host, a device assert on a GPU,
    fast_gradient_method.py:133-139).  Only the range bit is ``sanity_checks`` material (the reference evaluates its
    range asserts under ``sanity_checks`` only: fast_gradient_method.py:162-163).  The L-inf path without
    ``sanity_checks`` never reads the word (no host sync per call); there a bad label surfaces as the NaN loss the
    kernel writes.  Returns True when no sanity bit counts against the call."""
    if flag is None or not (sanity_checks or norm != np.inf):
        return True
    bits = int(flag.item())
    # the label first: its NaN loss makes the gradient non-finite, which then trips the degenerate bit as well
    assert not bits & VQA_FLAG_BAD_LABEL, "an MLM label is outside [0, vocabulary) and is not ignore_index"
    assert not bits & VQA_FLAG_DEGENERATE, \
        "optimize_linear: the optimal perturbation does not have unit norm (all-zero or non-finite gradient)"
    if not sanity_checks:
        return True
    return (bits & VQA_FLAG_RANGE) == 0


def _grad_of(leaf):
    g = leaf.grad
    if g is None:
        raise RuntimeError("model_fn's output does not depend on the image: no gradient reached x")
    return g if g.is_contiguous() else g.contiguous()


# ----------------------------------------------------------------------------------------- FGM
def fast_gradient_method(model_fn, x, eps, norm, ori_x, clip_min=None, clip_max=None, y=None, targeted=False,
                         sanity_checks=False, ls=None, bkp=None, bkp_y=None, *, flavor=ALBEF, per_sample=False,
                         ti_kernel=None, diversity_prob=None, di_shrink=32, di_rng=None, si_copies=None,
                         admix_images=None, admix_eta=0.2, admix_rng=None):
    """One FGM step; returns ``(adv_x, loss)`` (``loss`` is a 0-d device tensor), bare ``x`` when ``eps == 0``.
    ``ti_kernel`` (extension, keyword-only): TI-FGSM smoothing of the gradient, as in ``projected_gradient_descent``.
    ``diversity_prob`` / ``di_shrink`` / ``di_rng`` (extensions, keyword-only): DI-FGSM, as there (one evaluation).
    ``si_copies`` (extension, keyword-only): SI-FGSM scale copies, as there; ``loss`` is copy 0's.
    ``admix_images`` / ``admix_eta`` / ``admix_rng`` (extensions, keyword-only): Admix, as there (one evaluation); ``loss``
    is that of the first mixed copy.
    Reference: A fast_gradient_method.py:30-165, V :36-152 (the VLMO copy has no ``bkp``/``bkp_y``)."""
    _check_flavor(flavor)
    _validate_fgm(norm, eps, clip_min, clip_max)
    specs = _validate_stages(ti_kernel=ti_kernel, diversity_prob=diversity_prob, di_shrink=di_shrink, di_rng=di_rng,
                             si_copies=si_copies)
    aspec = _validate_admix(admix_images, admix_eta, admix_rng)
    _admix_batch(aspec, x)
    if eps == 0:
        return x
    xin = _as_image(x)
    check_range = sanity_checks and (clip_min is not None or clip_max is not None)
    flag = ops.new_flag(xin.device) if (check_range or norm != np.inf) else None
    chain = _Chain(specs, xin, norm, eps, eps, admix=aspec)
    loss_buf = torch.zeros(1, dtype=torch.float32, device=xin.device)

    def call(leaf, first):      # without DI / SI the leaf shares storage with x: nothing is written in place
        _loss_and_grad(model_fn, [leaf], leaf, y, ls, flavor, targeted, _LossSlot(loss_buf, 0) if first else chain.slot,
                       bkp=bkp, bkp_y=bkp_y, flag=flag, per_sample=per_sample)

    grad = chain.evaluate(xin, call)
    _two_sided(clip_min, clip_max)
    adv = chain.update(xin, grad, None, eps, eps, clip_min, clip_max, flag=flag, check_range=check_range)
    assert _check_flag(flag, norm, sanity_checks), "input x is outside [clip_min, clip_max]"
    return adv, loss_buf[0]


def fast_gradient_method_vl(model_fn, x, eps, norm, ori_x, clip_min=None, clip_max=None, y=None, targeted=False,
                            sanity_checks=False, ls=None, text_emb_pick=None, *, flavor=ALBEF, ti_kernel=None,
                            diversity_prob=None, di_shrink=32, di_rng=None, si_copies=None, admix_images=None,
                            admix_eta=0.2, admix_rng=None):
    """FGM on ``x = [image, text_embeds]``; returns ``(adv_image, text_grad[:, text_emb_pick])``.
    ``si_copies`` (extension, keyword-only): SI-FGSM scale copies of the IMAGE, as in ``projected_gradient_descent``;
    ``x[0]`` is then copy 0's leaf, the text gradient is copy 0's and the other copies see the text embeddings detached.
    ``admix_images`` / ``admix_eta`` / ``admix_rng`` (extensions, keyword-only): Admix on the IMAGE, as there; ``x[0]`` and
    the text gradient are those of the first mixed copy (the leaf's storage is reused by the later groups).
    ``ti_kernel`` (extension, keyword-only): TI-FGSM smoothing of the IMAGE gradient, as in ``projected_gradient_descent``.
    ``diversity_prob`` / ``di_shrink`` / ``di_rng`` (extensions, keyword-only): DI-FGSM on the IMAGE, as there; ``x[0]`` of
    the caller's list is then the transformed leaf the model saw.
    Like the reference it replaces ``x[0]``/``x[1]`` of the caller's list by the leaf tensors.
    Reference: A fast_gradient_method_vl.py:30-130, V :34-141."""
    _check_flavor(flavor)
    _validate_fgm(norm, eps, clip_min, clip_max)
    specs = _validate_stages(ti_kernel=ti_kernel, diversity_prob=diversity_prob, di_shrink=di_shrink, di_rng=di_rng,
                             si_copies=si_copies)
    aspec = _validate_admix(admix_images, admix_eta, admix_rng)
    _admix_batch(aspec, x[0] if aspec is not None else None)
    if eps == 0:
        return x
    img = _as_image(x[0], "x[0]")
    emb = _as_image(x[1], "x[1]")
    check_range = sanity_checks and (clip_min is not None or clip_max is not None)
    flag = ops.new_flag(img.device) if (check_range or norm != np.inf) else None
    chain = _Chain(specs, img, norm, eps, eps, admix=aspec)
    x[1] = emb.detach().requires_grad_(True)
    loss_buf = torch.zeros(1, dtype=torch.float32, device=img.device)

    def call(leaf, first):
        if first:
            x[0] = leaf
            _loss_and_grad(model_fn, [leaf, x[1]], [leaf, x[1]], y, ls, flavor, targeted, _LossSlot(loss_buf, 0), vl=True)
        else:
            _loss_and_grad(model_fn, [leaf], [leaf, emb.detach()], y, ls, flavor, targeted, chain.slot, vl=True)

    grad = chain.evaluate(img, call)
    text_grad = ops.gather_rows(_grad_of(x[1]), text_emb_pick)
    _two_sided(clip_min, clip_max)
    adv = chain.update(img, grad, None, eps, eps, clip_min, clip_max, flag=flag, check_range=check_range)
    assert _check_flag(flag, norm, sanity_checks), "input x is outside [clip_min, clip_max]"
    return adv, text_grad


# ----------------------------------------------------------------------------------------- PGD
def _start_point(x, norm, eps, clip_min, clip_max, time, rand_minmax, init_eta, flag, out):
    """adv_0 = clamp(x + clip_eta(eta)) with eta = U(-r, r) iff ``time == 0`` (the reference derives rand_init from
    ``time`` and ignores the kwarg: projected_gradient_descent.py:106-120)."""
    eta = None
    if time == 0:
        if init_eta is not None:
            eta = _as_image(init_eta, "init_eta")
            if eta.shape != x.shape:
                raise ValueError("init_eta shape {} != x shape {}".format(tuple(eta.shape), tuple(x.shape)))
        else:
            r = eps if rand_minmax is None else rand_minmax
            eta = torch.empty_like(x, memory_format=torch.contiguous_format).uniform_(-r, r)
        if norm == 2:
            eta = ops.scale_per_sample(eta, ops.sumsq_per_sample(eta), None, eps, kind=0)
    bound = eps if norm == np.inf else float("inf")
    return ops.linf_init(x, eta, bound, clip_min, clip_max, flag=flag, out=out)


def _finish(flag, eps, eps_iter, norm, clip_min, clip_max, sanity_checks):
    ok = [eps_iter <= eps]
    if norm == np.inf and clip_min is not None:
        ok.append(eps + clip_min <= clip_max)
    ok.append(_check_flag(flag, norm, sanity_checks))     # the only host read of the flag word
    if sanity_checks:
        assert np.all(ok)


def _graphed_linf_loop(model_fn, cur, x0, y, flavor, targeted, eps_iter, eps, clip_min, clip_max, nb_iter, loss_buf,
                       chain):
    """``nb_iter`` feature-loss L-inf iterations with iterations 1.. replayed from ONE captured hipGraph.

    For the launch-bound regime (the reference's own batch 1: ~10^3 kernels of a few microseconds per iteration):
    iteration 0 runs eagerly on a side stream (it is also the warm-up capture needs), iteration 1 is captured --
    white-box forward, fused loss, autograd backward and the in-place fused step on the static image buffer --
    and replayed.  Every C-ABI entry point is capture-safe (no allocation, no sync); the only eager op per
    iteration is the 4-byte copy of the loss word into its slot of the loss buffer.
    ``model_fn`` must be capturable: no host<->device copies or host RNG inside (ALBEF's per-forward token masking
    is not; use ``mlm_probability=0`` or eager mode there).
    ``chain`` (``_Chain``, L-inf): whatever its stages launch is captured with the iteration, and all of their state was
    allocated before capture.  Momentum: the |grad| reduction and the fused momentum step take the place of the step.
    TI: the taps travel in the kernel arguments.  DI: the transform and the adjoint are captured against the static
    geometry row; a device-to-device copy of the iteration's rows into it precedes each replay (eager, like the loss word).
    SI: the gradients' addresses, which travel by value in the kernel arguments, are the graph's own and the same at every
    replay.  VT: the neighbour launches are captured against the static key row; a copy of the iteration's key (seed and
    ``t``) into it precedes each replay, like DI's rows, so that every replay draws fresh numbers from the same launches.
    Admix: the copies launches are captured against the static partner rows; a copy of the iteration's ``(m2, B)`` rows
    into them precedes each replay, like DI's rows.
    """
    word = torch.zeros(1, dtype=torch.float32, device=cur.device)

    def call(leaf, first):
        _loss_and_grad(model_fn, [leaf], leaf, y, 1, flavor, targeted, _LossSlot(word, 0) if first else chain.slot)

    def iteration():
        grad = chain.evaluate(cur, call, advance=False)
        chain.update(cur, grad, x0, eps_iter, eps, clip_min, clip_max, out=cur)       # in place: static address

    main = torch.cuda.current_stream(cur.device)
    side = torch.cuda.Stream(device=cur.device)
    side.wait_stream(main)
    with torch.cuda.stream(side):
        chain.use(0, static=True)
        iteration()
        loss_buf[0:1].copy_(word)
    main.wait_stream(side)
    if nb_iter > 1:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            iteration()
        for i in range(1, nb_iter):
            chain.use(i, static=True)
            graph.replay()
            loss_buf[i:i + 1].copy_(word)
    return cur


def projected_gradient_descent(model_fn, x, eps, eps_iter, nb_iter, norm, clip_min=None, clip_max=None, y=None,
                               ori_x=None, time=None, targeted=False, rand_init=True, rand_minmax=None,
                               sanity_checks=True, ls=None, *, flavor=ALBEF, init_eta=None, graph=None,
                               per_sample=False, decay_factor=None, momentum=None, ti_kernel=None,
                               diversity_prob=None, di_shrink=32, di_rng=None, si_copies=None, nesterov=False,
                               vt_neighbors=None, vt_beta=1.5, vt_seed=None, admix_images=None, admix_eta=0.2,
                               admix_rng=None):
    """PGD over a frozen white box; returns ``(adv_x, loss_list)``, bare ``x`` when eps or eps_iter is 0.

    ``ls == 1``: feature loss, ``model_fn`` a callable.  Otherwise the dual-loss loop: ``model_fn = [feature_fn,
    mlm_fn]``, one feature step then one MLM step per iteration with a single projection after both.
    ``init_eta`` (extension, keyword-only): the uniform draw to use when ``time == 0`` (for reproducible parity runs).
    ``per_sample`` (extension, keyword-only): batched drivers set it so that the MLM cross entropy of the dual loop is
    normalised per sample (every sample's gradient then equals the batch-1 reference's; the reported loss is the sum
    of the per-sample losses instead of ``F.cross_entropy``'s batch mean).
    ``graph`` (extension, keyword-only): capture one iteration into a hipGraph and replay it (``ls == 1``, L-inf,
    two-sided or no clipping; for small, launch-bound batches -- see ``_graphed_linf_loop``).  Unmodified drivers
    that cannot pass the keyword opt in with ``VQA_PGD_GRAPH=1`` in the environment: eligible calls that leave ``graph``
    unset are then replayed,
    every other call (dual loss, L1 / L2, one-sided clipping) runs eagerly as before.  The closure must be capturable
    (no host read such as ``.item()`` inside it).
    ``decay_factor`` (extension, keyword-only): not None turns every update into MI-FGSM's (Dong et al. 2017; the
    reference tree has it for TensorFlow only, tf2/attacks/momentum_iterative_method.py:88-95): each gradient evaluation
    g does ``m <- decay_factor * m + g / max(1e-12, mean|g|)`` per sample and the update steps along ``m``.  The dual
    loop accumulates twice per iteration into the same ``m`` (feature gradient, then MLM gradient).  ``momentum``: the
    fp32 device tensor of ``x``'s shape that holds ``m``; it is updated in place, so a driver can carry it over several
    calls (None: zeros for this call).  With ``decay_factor=None`` (default) nothing changes and ``momentum`` is ignored.
    ``ti_kernel`` (extension, keyword-only): not None turns every update into TI-FGSM's (Dong et al. 2019; the reference
    tree has it in no framework): each image gradient is convolved per (H, W) plane with a separable kernel, zero padded,
    before the update -- an odd int ``kernlen`` in 1..31 selects the paper's Gaussian (``ops.ti_gaussian_taps(kernlen,
    3)``), a 1-D sequence of an odd number <= 31 of finite floats is used as the taps.  The L-inf update does it in one
    launch (``ops.linf_ti_step``); with ``decay_factor`` the smoothed gradient is what is normalised and accumulated
    (TI-MI-FGSM); L2 smooths in front of the existing update; the dual loop smooths both gradients.  ``x`` must be
    ``(B, C, H, W)``.  With ``ti_kernel=None`` (default) nothing changes.
    ``diversity_prob`` (extension, keyword-only): not None turns every gradient evaluation into DI-FGSM's (Xie et al.
    2019; the reference defines ``input_diversity`` for torch, cleverhans/fgsm_copy.py:9-31, and leaves its call
    commented out at :133): the model sees ``T(adv)``, each sample shrunk bilinearly to a random ``(new_h, new_w)`` with
    ``H - di_shrink <= new_h < H`` and zero padded back at a random offset, with probability ``diversity_prob`` (else
    the sample is left as it is); the update then runs on ``T``'s adjoint of the gradient at ``T(adv)`` -- what autograd
    through ``interpolate`` + ``pad`` gives, here one launch for the whole batch.  All rows of the call are drawn once,
    before the loop, from ``di_rng`` (anything with ``.uniform``; None: ``np.random``, as in the reference), four draws
    per sample and evaluation (``ops.di_draw``).  The plain L-inf update applies the adjoint in the same launch
    (``ops.linf_di_step``); with ``ti_kernel`` / ``decay_factor`` / L2 the adjoint (``ops.di_adjoint``) feeds those paths
    unchanged (DI + TI, DI + MI, all three).  ``x`` must be ``(B, C, H, W)``.  With ``diversity_prob=None`` (default)
    nothing changes and no random number is drawn.
    ``si_copies`` / ``nesterov`` (extensions, keyword-only): SI-NI-FGSM (Lin et al. 2020; the reference tree has neither).
    ``si_copies`` an int n in 1..8 (the paper's scales ``1, 1/2, ..., 2^-(n-1)``) or a sequence of 1..8 finite positive
    scales: every gradient evaluation calls the model once per scaled copy ``s_i * adv``, in ascending ``i``, and the
    gradient is ``sum_i (s_i / n) * g_i`` -- the paper's average with the chain rule through the scaling.  ``nesterov``
    (needs ``decay_factor``): the copies are taken at the look-ahead point ``adv + eps_iter * decay_factor * m``, unclipped
    as in the authors' code; alone it is one copy at scale 1.  The copies come from one launch (``ops.si_copies``); the
    plain L-inf update combines the gradients in the same launch (``ops.linf_si_step``), every other path combines into
    a scratch (``ops.si_combine``) in front of the DI adjoint, the smoothing, the momentum and the update, which run
    unchanged.  With DI every copy of an evaluation is transformed with that evaluation's rows (the draws are those of
    the call without ``si_copies``).  The reported loss is copy 0's; a closure that draws random numbers draws once per
    call.  The dual loop does all of this for both of its evaluations.  With ``si_copies=None, nesterov=False``
    (default) nothing changes.
    ``vt_neighbors`` / ``vt_beta`` / ``vt_seed`` (extensions, keyword-only): variance tuning, VMI / VNI-FGSM (Wang & He
    2021; the reference tree has it in no framework).  ``vt_neighbors`` an int N in 1..64: with ``G(p)`` the image
    gradient of one evaluation at ``p`` (after the SI combination and the DI adjoint, before the smoothing), every
    evaluation steps along ``G(p) + v`` and then sets ``v <- (1 / N) * sum_i G(p + r_i) - G(p)``, ``r_i ~ U[-vt_beta *
    eps, vt_beta * eps)`` per element, ``v = 0`` at first; ``p`` is ``adv`` or, with ``nesterov``, the look-ahead point, and
    the neighbours are not clipped, as in the authors' code.  That is N more model calls per evaluation (times the scale
    copies), in ascending order after the centre's, all with the centre's DI rows.  The neighbours come from the device
    (``ops.vt_neighbors``: Philox4x32-10 keyed by ``vt_seed`` -- None draws one seed from ``np.random`` -- the evaluation
    index of the call and the neighbour index, at most 8 images per launch), their gradients are summed on the device
    (``ops.vt_accumulate``) and the plain L-inf update tunes in the same launch (``ops.linf_vt_step``); every other path
    tunes into a scratch (``ops.vt_tune``) in front of the smoothing, the momentum and the update, which run unchanged.
    The reported loss is the centre's.  The dual loop keeps one ``v`` for its feature evaluations and one for its MLM
    evaluations.  With ``vt_neighbors=None`` (default) nothing changes, ``vt_beta`` / ``vt_seed`` are ignored and no random
    number is drawn.
    ``admix_images`` / ``admix_eta`` / ``admix_rng`` (extensions, keyword-only): Admix (Wang et al. 2021; the reference
    tree has it in no framework).  ``admix_images`` an int m2 in 1..8: every gradient evaluation calls the model on m2
    groups of the scale copies ``s_i * (p + admix_eta * adv[partner_j])``, ``p`` being ``adv`` or the look-ahead point,
    ``partner_j`` another sample of the batch per sample, drawn uniformly (``ops.admix_draw``) -- group by group, copies
    ascending -- and the gradient is ``sum_j sum_i s_i / (m1 * m2) * g_ji``.  Without ``si_copies`` every mixed image is
    one copy at scale 1; the paper's setting is ``si_copies=5, admix_images=3, admix_eta=0.2``.  Each group's copies come
    from one launch (``ops.admix_copies``); a finished group is folded into a running sum (``ops.si_combine``, then
    ``ops.admix_accumulate``), so at most m1 images and gradients are live; the plain L-inf update folds the last group in
    the same launch (``ops.linf_admix_step``), every other path in front of the DI adjoint, the variance tuning, the
    smoothing, the momentum and the update, which run unchanged.  All partner rows of the call are drawn once, before the
    loop and after DI's rows and VT's seed, from ``admix_rng`` (anything with ``.uniform``; None: ``np.random``), one draw
    per sample, group and evaluation; all copies and VT neighbours of an evaluation share its rows.  The reported loss is
    that of the first mixed copy.  The batch must hold at least 2 samples (``ValueError``).  With ``admix_images=None``
    (default) nothing changes, the other two keys are ignored and no random number is drawn.
    Reference: A projected_gradient_descent.py:10-199, V :10-196.
    """
    _check_flavor(flavor)
    unchanged = _validate_pgd(norm, eps, eps_iter, clip_min, clip_max)
    specs = _validate_stages(decay_factor, ti_kernel, diversity_prob, di_shrink, di_rng, si_copies, nesterov,
                             vt_neighbors, vt_beta, vt_seed)
    aspec = _validate_admix(admix_images, admix_eta, admix_rng)
    _admix_batch(aspec, x)
    if unchanged:
        return x
    xin = _as_image(x)
    has_clip = clip_min is not None or clip_max is not None
    flag = ops.new_flag(xin.device) if has_clip else None
    buf = [torch.empty_like(xin), torch.empty_like(xin)]
    adv = _start_point(xin, norm, eps, clip_min, clip_max, time, rand_minmax, init_eta, flag, buf[0])
    cur = 0
    if y is None:
        _, y = torch.max(model_fn(xin), 1)   # kept for API parity; every VQAttack caller passes y
    x0 = _as_image(ori_x, "ori_x")
    if x0.shape != xin.shape:
        raise ValueError("ori_x shape {} != x shape {}".format(tuple(x0.shape), tuple(xin.shape)))
    dual = ls != 1
    loss_buf = torch.zeros(max(nb_iter, 1) * (2 if dual else 1), dtype=torch.float32, device=xin.device)
    n_loss = 0
    chain = _Chain(specs, xin, norm, eps, eps_iter, nb_iter * (2 if dual else 1), kinds=2 if dual else 1,
                   momentum=momentum, admix=aspec)
    ws = ops.Workspace()       # loss-gradient / CE scratch buffers live for the whole call, not per iteration
    bad_flag = flag if flag is not None else (
        ops.new_flag(xin.device) if ((dual and sanity_checks) or norm != np.inf) else None)
    if graph is None and os.environ.get("VQA_PGD_GRAPH") == "1":
        graph = not dual and norm == np.inf and (clip_min is None) == (clip_max is None)
    if graph and nb_iter > 0:
        if dual or norm != np.inf:
            raise ValueError("graph=True supports the feature-loss (ls == 1) L-inf loop only")
        _two_sided(clip_min, clip_max)
        adv = _graphed_linf_loop(model_fn, adv, x0, y, flavor, targeted, eps_iter, eps, clip_min, clip_max, nb_iter,
                                 loss_buf, chain)
        n_loss, nb_iter = nb_iter, 0

    def evaluate(fn, at, y_, ls_, kind=0, **extra):
        """One gradient evaluation at ``at`` with the loss of copy 0 in the next slot of the loss buffer."""
        slot = _LossSlot(loss_buf, n_loss)

        def call(leaf, first):
            _loss_and_grad(fn, [leaf], leaf, y_, ls_, flavor, targeted, slot if first else chain.slot, ws=ws,
                           flag=bad_flag, **extra)

        return chain.evaluate(at, call, kind=kind)

    for _ in range(nb_iter):
        if not dual:
            grad = evaluate(model_fn, adv, y, ls)
            n_loss += 1
            _two_sided(clip_min, clip_max)
            adv = chain.update(adv, grad, x0, eps_iter, eps, clip_min, clip_max, out=buf[1 - cur], flag=bad_flag)
        else:
            if flavor == ALBEF:      # A :163,177-181 slices y; V :162,175 passes it whole
                y_feat, y_mlm, extra = [y[1], y[2]], [y[0]], dict(bkp=model_fn[0], bkp_y=[y[1], y[2]])
            else:
                y_feat, y_mlm, extra = y, y, {}
            grad = evaluate(model_fn[0], adv, y_feat, 1)
            n_loss += 1
            _two_sided(clip_min, clip_max)
            mid = chain.update(adv, grad, None, eps_iter, eps, clip_min, clip_max, out=buf[1 - cur], flag=bad_flag,
                               check_range=False)
            grad = evaluate(model_fn[1], mid, y_mlm, 0, kind=1, per_sample=per_sample, **extra)
            n_loss += 1
            adv = chain.update(mid, grad, x0, eps_iter, eps, clip_min, clip_max, out=buf[cur], flag=bad_flag)
            cur = 1 - cur            # result sits in buf[cur] again after the flip below
        cur = 1 - cur
        del grad
    _finish(bad_flag, eps, eps_iter, norm, clip_min, clip_max, sanity_checks)
    loss_list = loss_buf[:n_loss].tolist()     # single device->host transfer for the whole loop
    return adv, loss_list


def projected_gradient_descent_vl(model_fn, x, eps, eps_iter, nb_iter, norm, clip_min=None, clip_max=None, y=None,
                                  ori_x=None, time=None, targeted=False, rand_init=True, rand_minmax=None,
                                  sanity_checks=True, ls=None, attack_mask=None, *, flavor=ALBEF, init_eta=None,
                                  decay_factor=None, momentum=None, ti_kernel=None, diversity_prob=None, di_shrink=32,
                                  di_rng=None, si_copies=None, nesterov=False, vt_neighbors=None, vt_beta=1.5,
                                  vt_seed=None, admix_images=None, admix_eta=0.2, admix_rng=None):
    """PGD on ``x = [image, text_embeds]`` (only the image moves); returns ``(adv_image, text_embed_gradient)`` of
    the last iteration.  Only ``ls == 1`` is supported (``ValueError`` otherwise), as in the reference.
    ``decay_factor`` / ``momentum`` (extensions, keyword-only): MI-FGSM on the image, as in
    ``projected_gradient_descent``; ``momentum`` has the image's shape.  ``ti_kernel`` (extension, keyword-only):
    TI-FGSM smoothing of the image gradient, as there.  ``diversity_prob`` / ``di_shrink`` / ``di_rng`` (extensions,
    keyword-only): DI-FGSM, as there; only the image is transformed.  ``si_copies`` / ``nesterov`` (extensions,
    keyword-only): SI-NI-FGSM on the image, as there; the text gradient is copy 0's and the other copies see the text
    embeddings detached.  ``vt_neighbors`` / ``vt_beta`` / ``vt_seed`` (extensions, keyword-only): variance tuning, as
    there; only the image is perturbed, the text gradient is the centre evaluation's and the neighbours see the text
    embeddings detached.  ``admix_images`` / ``admix_eta`` / ``admix_rng`` (extensions, keyword-only): Admix on the image,
    as there; the text gradient is that of the first mixed copy and every other copy sees the text embeddings detached.
    Reference: A projected_gradient_descent_vl.py:10-168, V :10-164."""
    _check_flavor(flavor)
    unchanged = _validate_pgd(norm, eps, eps_iter, clip_min, clip_max)
    specs = _validate_stages(decay_factor, ti_kernel, diversity_prob, di_shrink, di_rng, si_copies, nesterov,
                             vt_neighbors, vt_beta, vt_seed)
    aspec = _validate_admix(admix_images, admix_eta, admix_rng)
    _admix_batch(aspec, x[0] if aspec is not None else None)
    if unchanged:
        return x
    img = _as_image(x[0], "x[0]")
    emb = _as_image(x[1], "x[1]")
    has_clip = clip_min is not None or clip_max is not None
    flag = ops.new_flag(img.device) if (has_clip or norm != np.inf) else None
    buf = [torch.empty_like(img), torch.empty_like(img)]
    adv = _start_point(img, norm, eps, clip_min, clip_max, time, rand_minmax, init_eta, flag, buf[0])
    cur = 0
    if y is None:
        _, y = torch.max(model_fn(x), 1)
    x0 = _as_image(ori_x, "ori_x")
    if ls != 1:
        raise ValueError("projected_gradient_descent_vl supports ls == 1 only")
    text_grad = None
    loss_buf = torch.zeros(max(nb_iter, 1), dtype=torch.float32, device=img.device)
    ws = ops.Workspace()
    chain = _Chain(specs, img, norm, eps, eps_iter, nb_iter, momentum=momentum, admix=aspec)
    if attack_mask is not None and not isinstance(attack_mask, ops.RowIndex):   # validated + uploaded once per call
        attack_mask = ops.RowIndex(attack_mask, emb.shape[1], emb.device)
    for it in range(nb_iter):
        leaf_txt = emb.detach().requires_grad_(True)
        slot = _LossSlot(loss_buf, it)

        def call(leaf_img, first):
            if first:
                _loss_and_grad(model_fn, [leaf_img, leaf_txt], [leaf_img, leaf_txt], y, ls, flavor, targeted, slot,
                               vl=True, ws=ws, flag=flag)
            else:
                _loss_and_grad(model_fn, [leaf_img], [leaf_img, emb.detach()], y, ls, flavor, targeted, chain.slot,
                               vl=True, ws=ws, flag=flag)

        grad = chain.evaluate(adv, call)
        text_grad = ops.gather_rows(_grad_of(leaf_txt), attack_mask)
        _two_sided(clip_min, clip_max)
        adv = chain.update(adv, grad, x0, eps_iter, eps, clip_min, clip_max, out=buf[1 - cur], flag=flag)
        cur = 1 - cur
        del grad, leaf_txt
    _finish(flag, eps, eps_iter, norm, clip_min, clip_max, sanity_checks)
    return adv, text_grad


# ----------------------------------------------------------------------------------------- MI-FGSM
def momentum_iterative_method(model_fn, x, eps, eps_iter, nb_iter, norm, clip_min=None, clip_max=None, y=None,
                              ori_x=None, targeted=False, decay_factor=1.0, sanity_checks=True, ls=1, *, flavor=ALBEF,
                              graph=None, momentum=None, ti_kernel=None, diversity_prob=None, di_shrink=32,
                              di_rng=None, si_copies=None, nesterov=False, vt_neighbors=None, vt_beta=1.5,
                              vt_seed=None, admix_images=None, admix_eta=0.2, admix_rng=None):
    """The momentum iterative method (Dong et al. 2017) on this project's losses; returns ``(adv_x, loss_list)`` like
    ``projected_gradient_descent``, so a driver can swap one for the other.

    The reference tree ships the method for TensorFlow only (tf2/attacks/momentum_iterative_method.py) and never ported
    it to the torch operators its drivers call.  As there, the loop starts at ``x`` itself (no random start, :80-81),
    ``norm == 1`` is refused first (:54-60) and every iteration normalises the gradient by its per-sample mean absolute
    value, adds it to ``decay_factor`` times the momentum (:88-95) and steps along the momentum (:97-103).  ``ori_x``
    (centre of the eps-ball) defaults to ``x``; ``ls``, ``flavor``, ``graph``, ``momentum`` and ``ti_kernel``
    (TI-MI-FGSM, the combination the TI paper recommends) as in ``projected_gradient_descent``, which runs the loop;
    ``diversity_prob`` / ``di_shrink`` / ``di_rng`` as there too (M-DI2-FGSM; with ``ti_kernel`` TI-DIM), and so are
    ``si_copies`` / ``nesterov`` (SI-NI-FGSM; with the other keys SI-NI-TI-DIM) and ``vt_neighbors`` / ``vt_beta`` /
    ``vt_seed`` (VMI-FGSM; with ``nesterov`` VNI-FGSM) and ``admix_images`` / ``admix_eta`` / ``admix_rng`` (with the TI and
    DI keys the Admix paper's Admix-TI-DIM)."""
    if norm != 1 and decay_factor is None:
        raise ValueError("decay_factor must be a number (use projected_gradient_descent for the attack without momentum)")
    return projected_gradient_descent(model_fn, x, eps, eps_iter, nb_iter, norm, clip_min=clip_min, clip_max=clip_max,
                                      y=y, ori_x=x if ori_x is None else ori_x, time=None, targeted=targeted,
                                      sanity_checks=sanity_checks, ls=ls, flavor=flavor, graph=graph,
                                      decay_factor=decay_factor, momentum=momentum, ti_kernel=ti_kernel,
                                      diversity_prob=diversity_prob, di_shrink=di_shrink, di_rng=di_rng,
                                      si_copies=si_copies, nesterov=nesterov, vt_neighbors=vt_neighbors,
                                      vt_beta=vt_beta, vt_seed=vt_seed, admix_images=admix_images, admix_eta=admix_eta,
                                      admix_rng=admix_rng)
