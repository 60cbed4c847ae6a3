"""Tensor-level wrappers over the C ABI (one function per kernel entry point).

Every function launches on the current HIP stream of its tensors' device and returns without synchronising.
``out=`` arguments let the PGD loop ping-pong between two pre-allocated image buffers.
"""
import contextlib
import ctypes

import numpy as np
import torch

from . import _hip
from ._hip import VQA_CHECK_RANGE, VQA_CLIP, check, dev_f32, lib, ptr, same_device, stream_for

_INF = float("inf")


@contextlib.contextmanager
def _on(t):
    if t.device.index is not None and t.device.index != torch.cuda.current_device():
        with torch.cuda.device(t.device):
            yield
    else:
        yield


def _clip_args(clip_min, clip_max):
    """(mode bits, cmin, cmax); a missing bound becomes +-inf (torch.clamp with one bound)."""
    if clip_min is None and clip_max is None:
        return 0, -_INF, _INF
    return VQA_CLIP, (-_INF if clip_min is None else float(clip_min)), (_INF if clip_max is None else float(clip_max))


def _clip_mode(clip_min, clip_max, flag, check_range=True):
    """``_clip_args``; with a ``flag`` and a clip range the mode also asks for the range check (unless switched off)."""
    mode, lo, hi = _clip_args(clip_min, clip_max)
    if flag is not None and mode and check_range:
        mode |= VQA_CHECK_RANGE
    return mode, lo, hi


def _out_like(x, out):
    if out is None:
        return torch.empty_like(x, memory_format=torch.contiguous_format)
    dev_f32(out, "out")
    if out.shape != x.shape:
        raise ValueError("out has shape {}, expected {}".format(tuple(out.shape), tuple(x.shape)))
    return out


def _momentum_like(x, m):
    """The optional momentum of a copies kernel: checked against ``x``."""
    if m is not None:
        dev_f32(m, "momentum")
        if m.shape != x.shape:
            raise ValueError("momentum shape {} != x shape {}".format(tuple(m.shape), tuple(x.shape)))


def _copies_out(x, count, out, what):
    """``(out, stride)`` of a copies kernel: the ``(count,) + x.shape`` result, allocated or the caller's -- every
    ``out[i]`` contiguous, the copies possibly further apart than ``x.numel()`` -- and the distance between two copies
    in elements.  ``what``: the message's words for one copy and for all of them, ``("out[i]", "copies")``."""
    shape = (count,) + tuple(x.shape)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    else:
        dev_f32(out, "out", contiguous=False)
        if tuple(out.shape) != shape:
            raise ValueError("out has shape {}, expected {}".format(tuple(out.shape), shape))
        if not out[0].is_contiguous() or (count > 1 and out.stride(0) < x.numel()):
            raise ValueError("every {} must be contiguous and the {} must not overlap".format(*what))
    return out, (out.stride(0) if count > 1 else x.numel())


def _grad_ptrs(grads, limit, like=None):
    """The ctypes pointer array of a list of 1..``limit`` gradient tensors of one shape: that of ``like``, the running
    ``sum`` they are added to (checked here), or their first's."""
    if isinstance(grads, torch.Tensor) or not isinstance(grads, (list, tuple)):
        raise TypeError("grads must be a list or tuple of tensors{}, got {}".format(
            "" if like is not None else " (autograd hands back one per copy)", type(grads)))
    if len(grads) < 1 or len(grads) > limit:
        raise ValueError("grads must hold 1..{} tensors, got {}".format(limit, len(grads)))
    ref, name = (grads[0], "grads[0]") if like is None else (dev_f32(like, "sum"), "sum")
    for i, g in enumerate(grads):
        dev_f32(g, "grads[{}]".format(i))
        if g.shape != ref.shape:
            raise ValueError("grads[{}] has shape {}, {} {}".format(i, tuple(g.shape), name, tuple(ref.shape)))
    return (ctypes.c_void_p * len(grads))(*[g.data_ptr() for g in grads])


def _fused_step_args(x, g, x0, clip_min, clip_max, flag, out, also=(), what="grad"):
    """What the fused L-inf steps (``linf_*_step``) share in front of their launch: ``x`` and ``x0`` (None: the FGM form)
    checked, ``g`` -- checked by its own stage -- against their shape, every tensor (``also``: the stage's own) on one
    device.  Returns ``(out, mode bits, cmin, cmax)``; with a ``flag`` and a clip range the mode asks for the range check."""
    dev_f32(x, "x")
    if x0 is not None:
        dev_f32(x0, "ori_x")
    if g.shape != x.shape or (x0 is not None and x0.shape != x.shape):
        raise ValueError("shape mismatch: x {}, {} {}, ori_x {}".format(
            tuple(x.shape), what, tuple(g.shape), None if x0 is None else tuple(x0.shape)))
    same_device(x, g, x0, out, flag, *also)
    out = _out_like(x, out)
    mode, lo, hi = _clip_mode(clip_min, clip_max, flag)
    return out, mode, lo, hi


def new_flag(device):
    """int32[1] device word the kernels OR range violations into (read once at the end of an attack)."""
    return torch.zeros(1, dtype=torch.int32, device=device)


# ----------------------------------------------------------------------------------------- L-inf
def linf_init(x, eta, eps, clip_min, clip_max, flag=None, out=None):
    dev_f32(x, "x")
    if eta is not None:
        dev_f32(eta, "eta")
        if eta.shape != x.shape:
            raise ValueError("eta shape {} != x shape {}".format(tuple(eta.shape), tuple(x.shape)))
    same_device(x, eta, out, flag)
    out = _out_like(x, out)
    mode, lo, hi = _clip_mode(clip_min, clip_max, flag)
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_linf_init(ptr(x), ptr(eta), ptr(out), x.numel(), eps, lo, hi, mode, ptr(flag),
                                  stream_for(x)), "vqa_linf_init")
    return out


def linf_fgm(x, g, eps_iter, clip_min, clip_max, flag=None, out=None):
    dev_f32(x, "x"), dev_f32(g, "grad")
    if g.shape != x.shape:
        raise ValueError("grad shape {} != x shape {}".format(tuple(g.shape), tuple(x.shape)))
    same_device(x, g, out, flag)
    out = _out_like(x, out)
    mode, lo, hi = _clip_mode(clip_min, clip_max, flag)
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_linf_fgm(ptr(x), ptr(g), ptr(out), x.numel(), eps_iter, lo, hi, mode, ptr(flag),
                                 stream_for(x)), "vqa_linf_fgm")
    return out


def linf_step(x, g, x0, eps_iter, eps, clip_min, clip_max, flag=None, out=None):
    """The fused north-star kernel: FGM update + eps-ball projection + clamp, 16 B/element."""
    dev_f32(x, "x"), dev_f32(g, "grad"), dev_f32(x0, "ori_x")
    if g.shape != x.shape or x0.shape != x.shape:
        raise ValueError("shape mismatch: x {}, grad {}, ori_x {}".format(tuple(x.shape), tuple(g.shape),
                                                                          tuple(x0.shape)))
    same_device(x, g, x0, out, flag)
    out = _out_like(x, out)
    mode, lo, hi = _clip_mode(clip_min, clip_max, flag)
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_linf_step(ptr(x), ptr(g), ptr(x0), ptr(out), x.numel(), eps_iter, eps, lo, hi, mode,
                                  ptr(flag), stream_for(x)), "vqa_linf_step")
    return out


def linf_project(adv, x0, eps, clip_min, clip_max, out=None):
    dev_f32(adv, "adv_x"), dev_f32(x0, "ori_x")
    if adv.shape != x0.shape:
        raise ValueError("shape mismatch: adv {}, ori_x {}".format(tuple(adv.shape), tuple(x0.shape)))
    same_device(adv, x0, out)
    out = _out_like(adv, out)
    mode, lo, hi = _clip_args(clip_min, clip_max)
    if adv.numel() == 0:
        return out
    with _on(adv):
        check(lib().vqa_linf_project(ptr(adv), ptr(x0), ptr(out), adv.numel(), eps, lo, hi, mode,
                                     stream_for(adv)), "vqa_linf_project")
    return out


def clip_eta_linf(eta, eps):
    dev_f32(eta, "eta")
    out = torch.empty_like(eta)
    if eta.numel() == 0:
        return out
    with _on(eta):
        check(lib().vqa_clip_eta_linf(ptr(eta), ptr(out), eta.numel(), eps, stream_for(eta)), "vqa_clip_eta_linf")
    return out


def optimize_linear_linf(grad, eps):
    dev_f32(grad, "grad")
    out = torch.empty_like(grad)
    if grad.numel() == 0:
        return out
    with _on(grad):
        check(lib().vqa_optimize_linear_linf(ptr(grad), ptr(out), grad.numel(), eps, stream_for(grad)),
              "vqa_optimize_linear_linf")
    return out


def zero_out_clipped_grads(grad, x, clip_min, clip_max):
    dev_f32(grad, "grad"), dev_f32(x, "x")
    if grad.shape != x.shape:
        raise ValueError("grad shape {} != x shape {}".format(tuple(grad.shape), tuple(x.shape)))
    out = torch.empty_like(grad)
    if grad.numel() == 0:
        return out
    with _on(grad):
        check(lib().vqa_zero_out_clipped_grads(ptr(grad), ptr(x), ptr(out), grad.numel(), float(clip_min),
                                               float(clip_max), stream_for(grad)), "vqa_zero_out_clipped_grads")
    return out


# ----------------------------------------------------------------------------------------- per-sample norms
def _per_sample(t):
    batch = t.shape[0] if t.dim() > 0 else 1
    n_per = t.numel() // max(batch, 1)
    return batch, n_per


def _workspace(t):
    batch, n_per = _per_sample(t)
    nbytes = lib().vqa_reduce_ws_bytes(batch, n_per)
    return torch.empty(max(nbytes // 4, 1), dtype=torch.float32, device=t.device)


def reduce_workspace(t):
    """The workspace a per-sample reduction of a tensor shaped like ``t`` needs, for callers that reuse one (``ws=``)."""
    dev_f32(t, "t")
    return _workspace(t)


def sumsq_per_sample(t, sub=None):
    """out[b] = sum((t[b] - sub[b])**2), deterministic two-stage reduction."""
    dev_f32(t, "t")
    if sub is not None:
        dev_f32(sub, "sub")
        if sub.shape != t.shape:
            raise ValueError("shape mismatch")
    batch, n_per = _per_sample(t)
    out = torch.empty(batch, dtype=torch.float32, device=t.device)
    if t.numel() == 0:
        return out.zero_()
    ws = _workspace(t)
    with _on(t):
        check(lib().vqa_sumsq_per_sample(ptr(t), ptr(sub), ptr(out), batch, n_per, ptr(ws), stream_for(t)),
              "vqa_sumsq_per_sample")
    return out


def absmax_ties_per_sample(g):
    dev_f32(g, "grad")
    batch, n_per = _per_sample(g)
    amax = torch.empty(batch, dtype=torch.float32, device=g.device)
    ties = torch.empty(batch, dtype=torch.float32, device=g.device)
    if g.numel() == 0:
        return amax.zero_(), ties.zero_()
    ws = _workspace(g)
    with _on(g):
        check(lib().vqa_absmax_ties_per_sample(ptr(g), ptr(amax), ptr(ties), batch, n_per, ptr(ws), stream_for(g)),
              "vqa_absmax_ties_per_sample")
    return amax, ties


def l2_fgm(x, g, eps_iter, clip_min, clip_max, flag=None, out=None, check_range=True):
    """``flag``: receives VQA_FLAG_DEGENERATE when a sample's gradient norm is not finite (the reference's self-check in
    optimize_linear, utils.py:110-116) and, with ``check_range``, VQA_FLAG_RANGE for inputs outside the clip range."""
    dev_f32(x, "x"), dev_f32(g, "grad")
    if g.shape != x.shape:
        raise ValueError("shape mismatch")
    ss = sumsq_per_sample(g)
    out = _out_like(x, out)
    batch, n_per = _per_sample(x)
    mode, lo, hi = _clip_mode(clip_min, clip_max, flag, check_range)
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_l2_fgm(ptr(x), ptr(g), ptr(ss), ptr(out), batch, n_per, eps_iter, lo, hi, mode, ptr(flag),
                               stream_for(x)), "vqa_l2_fgm")
    return out


def l2_project(adv, x0, eps, clip_min, clip_max, out=None):
    dev_f32(adv, "adv_x"), dev_f32(x0, "ori_x")
    if adv.shape != x0.shape:
        raise ValueError("shape mismatch")
    ss = sumsq_per_sample(adv, sub=x0)
    out = _out_like(adv, out)
    batch, n_per = _per_sample(adv)
    mode, lo, hi = _clip_args(clip_min, clip_max)
    if adv.numel() == 0:
        return out
    with _on(adv):
        check(lib().vqa_l2_project(ptr(adv), ptr(x0), ptr(ss), ptr(out), batch, n_per, eps, lo, hi, mode,
                                   stream_for(adv)), "vqa_l2_project")
    return out


def l1_fgm(x, g, eps_iter, clip_min, clip_max, flag=None, out=None, check_range=True):
    """``flag``: receives VQA_FLAG_DEGENERATE when a sample's largest |gradient| is 0 or NaN (utils.py:101-104)."""
    dev_f32(x, "x"), dev_f32(g, "grad")
    if g.shape != x.shape:
        raise ValueError("shape mismatch")
    amax, ties = absmax_ties_per_sample(g)
    out = _out_like(x, out)
    batch, n_per = _per_sample(x)
    mode, lo, hi = _clip_mode(clip_min, clip_max, flag, check_range)
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_l1_fgm(ptr(x), ptr(g), ptr(amax), ptr(ties), ptr(out), batch, n_per, eps_iter, lo, hi, mode,
                               ptr(flag), stream_for(x)), "vqa_l1_fgm")
    return out


def scale_per_sample(t, stat, stat2, eps, kind, out=None, flag=None):
    """``flag`` (int32 device word): kinds 1 / 2 OR ``VQA_FLAG_DEGENERATE`` into it where the reference's unit-norm
    self-check of ``optimize_linear`` would fail (utils.py:101-104, :110-116)."""
    dev_f32(t, "t"), dev_f32(stat, "stat")
    out = _out_like(t, out)
    batch, n_per = _per_sample(t)
    if t.numel() == 0:
        return out
    with _on(t):
        check(lib().vqa_scale_per_sample(ptr(t), ptr(stat), ptr(stat2), ptr(out), batch, n_per, eps, kind, ptr(flag),
                                         stream_for(t)), "vqa_scale_per_sample")
    return out


# ----------------------------------------------------------------------------------------- momentum (MI-FGSM)
def _stat_like(t, stat, name):
    """A caller's per-sample statistic (one fp32 word per sample, used as is: static address for the graph loop)."""
    batch, _ = _per_sample(t)
    if stat is None:
        return torch.empty(batch, dtype=torch.float32, device=t.device)
    dev_f32(stat, name)
    if stat.numel() != batch:
        raise ValueError("{} has {} elements, expected one per sample ({})".format(name, stat.numel(), batch))
    return stat


def sumabs_per_sample(g, out=None, ws=None):
    """out[b] = sum(|g[b]|), the deterministic two-stage reduction of ``sumsq_per_sample``.  ``out`` and ``ws``
    (``reduce_workspace(g)``) are used as they are when given: nothing is allocated, as a captured loop needs."""
    dev_f32(g, "grad")
    same_device(g, out, ws)
    out = _stat_like(g, out, "out")
    batch, n_per = _per_sample(g)
    if g.numel() == 0:
        return out.zero_()
    if ws is None:
        ws = _workspace(g)
    elif dev_f32(ws, "ws").numel() * 4 < lib().vqa_reduce_ws_bytes(batch, n_per):
        raise ValueError("ws holds {} floats, too few for this reduction".format(ws.numel()))
    with _on(g):
        check(lib().vqa_sumabs_per_sample(ptr(g), ptr(out), batch, n_per, ptr(ws), stream_for(g)),
              "vqa_sumabs_per_sample")
    return out


def _momentum_args(g, m, sumabs):
    dev_f32(g, "grad"), dev_f32(m, "momentum")
    if m.shape != g.shape:
        raise ValueError("momentum shape {} != grad shape {}".format(tuple(m.shape), tuple(g.shape)))
    same_device(g, m, sumabs)
    if g.numel() == 0:
        return None
    return sumabs_per_sample(g) if sumabs is None else _stat_like(g, sumabs, "sumabs")


def momentum_accumulate(g, m, decay, sumabs=None):
    """``m <- decay * m + g / max(1e-12, mean|g[b]|)`` in place; returns ``m``.  ``sumabs``: the per-sample sum of |g|
    when the caller has it already (``sumabs_per_sample``), computed here otherwise."""
    sumabs = _momentum_args(g, m, sumabs)
    if g.numel() == 0:
        return m
    batch, n_per = _per_sample(g)
    with _on(g):
        check(lib().vqa_momentum_accumulate(ptr(g), ptr(sumabs), ptr(m), batch, n_per, float(decay), stream_for(g)),
              "vqa_momentum_accumulate")
    return m


def linf_momentum_step(x, g, x0, m, decay, eps_iter, eps, clip_min, clip_max, flag=None, out=None, sumabs=None):
    """``momentum_accumulate`` and ``linf_step`` on the new momentum in one pass, 24 B/element; ``x0=None``: and
    ``linf_fgm`` (no projection), 20 B/element.  ``m`` is updated in place; ``out`` may be ``x``."""
    out, mode, lo, hi = _fused_step_args(x, g, x0, clip_min, clip_max, flag, out)
    sumabs = _momentum_args(g, m, sumabs)
    if x.numel() == 0:
        return out
    batch, n_per = _per_sample(x)
    with _on(x):
        check(lib().vqa_linf_momentum_step(ptr(x), ptr(g), ptr(sumabs), ptr(x0), ptr(m), ptr(out), batch, n_per, float(decay),
                                           eps_iter, eps, lo, hi, mode, ptr(flag), stream_for(x)),
              "vqa_linf_momentum_step")
    return out


# ----------------------------------------------------------------------------------------- TI smoothing (TI-FGSM)
TI_MAX_TAPS = 31


def ti_gaussian_taps(kernlen=15, nsig=3.0):
    """The 1-D taps of the TI paper's ``gkern(kernlen, nsig)`` (Dong et al. 2019): the normal density at
    ``linspace(-nsig, nsig, kernlen)``, normalised in float64, as a numpy float32 array.  The paper's 2-D kernel is the
    outer product of these taps."""
    kernlen = int(kernlen)
    if kernlen < 1:
        raise ValueError("kernlen must be at least 1, got {}".format(kernlen))
    x = np.linspace(-float(nsig), float(nsig), kernlen)
    k = np.exp(-0.5 * x * x)
    return (k / k.sum()).astype(np.float32)


def _ti_taps(taps):
    """(ctypes float array, K) of a host tap sequence: what the kernels take by value in their arguments."""
    w = np.ascontiguousarray(taps, dtype=np.float32)
    if w.ndim != 1 or w.size < 1 or w.size > TI_MAX_TAPS or w.size % 2 == 0:
        raise ValueError("taps must be a 1-d sequence of an odd number (1..{}) of floats, got shape {}".format(
            TI_MAX_TAPS, w.shape))
    return (ctypes.c_float * w.size)(*w.tolist()), int(w.size)


def _ti_planes(g):
    dev_f32(g, "grad", contiguous=False)
    if g.dim() != 4 or not g.is_contiguous():
        raise ValueError("grad must be a contiguous (B, C, H, W) tensor: the stencil runs over row-major planes")
    return g.shape[0] * g.shape[1], g.shape[2], g.shape[3]


def ti_smooth(g, taps, out=None):
    """``out = ghat``: every (H, W) plane of ``g`` convolved with the separable ``taps`` (rows, then columns), zero
    padded; the bit-level contract is in ``include/vqattack_hip.h``.  ``out`` is used as given and must not be ``g``."""
    planes, h, w = _ti_planes(g)
    same_device(g, out)
    buf, k = _ti_taps(taps)
    out = _out_like(g, out)
    if g.numel() == 0:
        return out
    with _on(g):
        check(lib().vqa_ti_smooth(ptr(g), ptr(out), planes, h, w, buf, k, stream_for(g)), "vqa_ti_smooth")
    return out


def linf_ti_step(x, g, x0, taps, eps_iter, eps, clip_min, clip_max, flag=None, out=None):
    """``ti_smooth`` and ``linf_step`` on the smoothed gradient in one pass, 16 B/element; ``x0=None``: and ``linf_fgm``
    (no projection), 12 B/element.  The smoothed gradient never reaches memory; ``out`` may be ``x``."""
    planes, h, w = _ti_planes(g)
    buf, k = _ti_taps(taps)
    out, mode, lo, hi = _fused_step_args(x, g, x0, clip_min, clip_max, flag, out)
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_linf_ti_step(ptr(x), ptr(g), ptr(x0), ptr(out), planes, h, w, buf, k, eps_iter, eps, lo, hi, mode,
                                     ptr(flag), stream_for(x)), "vqa_linf_ti_step")
    return out


# ----------------------------------------------------------------------------------------- input diversity (DI-FGSM)
def di_draw(rng, batch, steps, height, width, shrink=32, prob=1.0):
    """The geometry rows ``[new_h, new_w, top, left]`` of ``steps`` x ``batch`` DI transforms as an int32 numpy array
    ``(steps, batch, 4)``.  ``rng`` is anything with ``.uniform`` (``np.random``, a ``RandomState``, a ``Generator``).
    Per step and sample, in this order, the three draws of the reference's ``input_diversity``
    (cleverhans/fgsm_copy.py:9-31, ``shrink`` in place of its 32) and one ``uniform()`` draw ``u``; with ``u >= prob``
    the row becomes the identity row ``[height, width, 0, 0]``.  All four draws are always taken, so the stream does not
    depend on ``prob``."""
    batch, steps, height, width, shrink = int(batch), int(steps), int(height), int(width), int(shrink)
    if batch < 0 or steps < 0 or height < 1 or width < 1 or shrink < 0:
        raise ValueError("di_draw: batch / steps must be >= 0, height / width >= 1, shrink >= 0")
    if height - shrink < 1:
        raise ValueError("di_draw: height - shrink must be at least 1, got height {} and shrink {}".format(height, shrink))
    table = np.empty((steps, batch, 4), dtype=np.int32)
    for s in range(steps):
        for b in range(batch):
            newh = int(rng.uniform(height - shrink, height))
            neww = int((newh / height) * width)
            top = int(rng.uniform(0, height - newh))
            left = int(rng.uniform(0, width - neww))
            u = rng.uniform()
            if neww < 1:
                raise ValueError("di_draw: new_w = {} for new_h = {} of ({}, {}): the image is too narrow for this "
                                 "shrink".format(neww, newh, height, width))
            table[s, b] = (newh, neww, top, left) if u < prob else (height, width, 0, 0)
    return table


def di_check_table(table, height, width):
    """``table`` as a C-contiguous int32 numpy array ``(..., 4)`` with every row inside the ranges of the contract."""
    t = np.asarray(table)
    if t.dtype.kind not in "iu" or t.ndim < 1 or t.shape[-1] != 4:
        raise ValueError("a DI geometry table is an integer array (..., 4) of [new_h, new_w, top, left] rows, got "
                         "dtype {} shape {}".format(t.dtype, t.shape))
    t = t.astype(np.int64)
    nh, nw, top, left = t[..., 0], t[..., 1], t[..., 2], t[..., 3]
    bad = (nh < 1) | (nh > height) | (nw < 1) | (nw > width) | (top < 0) | (top > height - nh) | (left < 0) | \
        (left > width - nw)
    if bad.any():
        row = t.reshape(-1, 4)[int(np.flatnonzero(bad.reshape(-1))[0])]
        raise ValueError("DI geometry row {} is outside its ranges for a ({}, {}) plane".format(row.tolist(), height, width))
    return np.ascontiguousarray(t.astype(np.int32))


def di_geometry(table, height, width, device):
    """Validate a geometry table against ``(height, width)`` and upload it in one copy: an int32 device tensor of the
    table's shape.  The kernels read one ``(B, 4)`` slice of it per launch."""
    return torch.from_numpy(di_check_table(table, height, width)).to(device)


def _di_args(x, geom, name):
    dev_f32(x, name, contiguous=False)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError("{} must be a contiguous (B, C, H, W) tensor: the transform runs over row-major planes".format(name))
    if not isinstance(geom, torch.Tensor) or not geom.is_cuda or geom.dtype != torch.int32 or not geom.is_contiguous() \
            or geom.dim() != 2 or geom.shape[0] != x.shape[0] or geom.shape[1] != 4:
        raise ValueError("geom must be a contiguous int32 device tensor ({}, 4) (ops.di_geometry), got {}".format(
            x.shape[0], (geom.dtype, tuple(geom.shape), str(geom.device)) if isinstance(geom, torch.Tensor) else type(geom)))
    return x.shape


def di_transform(x, geom, out=None):
    """``out = T(x)``: per sample, every (H, W) plane shrunk bilinearly to ``(new_h, new_w)`` and zero padded back at
    ``(top, left)``; the bit-level contract is in ``include/vqattack_hip.h``.  ``out`` must not be ``x``."""
    b, c, h, w = _di_args(x, geom, "x")
    same_device(x, geom, out)
    out = _out_like(x, out)
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_di_transform(ptr(x), ptr(geom), ptr(out), b, c, h, w, stream_for(x)), "vqa_di_transform")
    return out


def di_adjoint(gd, geom, out=None):
    """``out = T^T(gD)``: the gradient with respect to ``x`` of a loss whose gradient at ``di_transform(x, geom)`` is
    ``gd``; a deterministic gather.  ``out`` must not be ``gd``."""
    b, c, h, w = _di_args(gd, geom, "grad")
    same_device(gd, geom, out)
    out = _out_like(gd, out)
    if gd.numel() == 0:
        return out
    with _on(gd):
        check(lib().vqa_di_adjoint(ptr(gd), ptr(geom), ptr(out), b, c, h, w, stream_for(gd)), "vqa_di_adjoint")
    return out


def linf_di_step(x, gd, x0, geom, eps_iter, eps, clip_min, clip_max, flag=None, out=None):
    """``di_adjoint`` and ``linf_step`` on its result in one pass, at most 16 B/element; ``x0=None``: and ``linf_fgm`` (no
    projection).  The image gradient never reaches memory; ``out`` may be ``x``."""
    b, c, h, w = _di_args(gd, geom, "grad")
    out, mode, lo, hi = _fused_step_args(x, gd, x0, clip_min, clip_max, flag, out, also=(geom,))
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_linf_di_step(ptr(x), ptr(gd), ptr(x0), ptr(geom), ptr(out), b, c, h, w, eps_iter, eps, lo, hi,
                                     mode, ptr(flag), stream_for(x)), "vqa_linf_di_step")
    return out


# ----------------------------------------------------------------------------------------- scale copies (SI-NI-FGSM)
SI_MAX_COPIES = 8      # VQA_SI_MAX_COPIES of include/vqattack_hip.h (vqa_si_max_copies())


def si_scales(copies):
    """The paper's scales ``1, 1/2, ..., 2^-(copies - 1)`` (Lin et al. 2020) as a numpy float32 array."""
    copies = int(copies)
    if copies < 1 or copies > SI_MAX_COPIES:
        raise ValueError("copies must be in 1..{}, got {}".format(SI_MAX_COPIES, copies))
    return np.ldexp(np.float32(1.0), -np.arange(copies)).astype(np.float32)


def _si_host(values, name):
    """(numpy float32 array, ctypes float array) of a host sequence of 1..SI_MAX_COPIES floats."""
    w = np.ascontiguousarray(values, dtype=np.float32)
    if w.ndim != 1 or w.size < 1 or w.size > SI_MAX_COPIES:
        raise ValueError("{} must be a 1-d sequence of 1..{} floats, got shape {}".format(name, SI_MAX_COPIES, w.shape))
    return w, (ctypes.c_float * w.size)(*w.tolist())


def si_weights(scales):
    """``w_i = float32(s_i) / float32(n)``: the paper's average over the ``n`` copies together with the chain rule through
    the scaling (the gradient with respect to the image of a loss evaluated at ``s_i * image``)."""
    s, _ = _si_host(scales, "scales")
    return (s / np.float32(s.size)).astype(np.float32)


def si_copies(x, scales, m=None, lookahead=0.0, out=None):
    """``out[i] = s_i * x``, or ``s_i * (x + lookahead * m)`` with the momentum ``m``: every copy in one launch, as an
    ``(n,) + x.shape`` tensor.  No clamp, no projection.  ``out`` must not overlap ``x`` or ``m``; each ``out[i]`` must be
    contiguous, and the copies may lie further apart than ``x.numel()`` (the batch prefix of a larger buffer)."""
    s, buf = _si_host(scales, "scales")
    dev_f32(x, "x")
    _momentum_like(x, m)
    same_device(x, m, out)
    out, stride = _copies_out(x, int(s.size), out, ("out[i]", "copies"))
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_si_copies(ptr(x), ptr(m), ptr(out), x.numel(), stride, buf, int(s.size), float(lookahead),
                                  stream_for(x)), "vqa_si_copies")
    return out


def _si_grads(grads, weights):
    """(ctypes pointer array, ctypes float array, copies) of a list of same-shape gradient tensors and their weights."""
    pbuf = _grad_ptrs(grads, SI_MAX_COPIES)
    w, wbuf = _si_host(weights, "weights")
    if w.size != len(grads):
        raise ValueError("{} weights for {} gradients".format(w.size, len(grads)))
    same_device(*grads)
    return pbuf, wbuf, len(grads)


def si_combine(grads, weights, out=None):
    """``out = w_0 * g_0 + w_1 * g_1 + ...`` (ascending, one rounding per operation, starting from the first product).
    ``out`` may alias no gradient."""
    pbuf, wbuf, copies = _si_grads(grads, weights)
    same_device(grads[0], out)
    out = _out_like(grads[0], out)
    if out.numel() == 0:
        return out
    with _on(out):
        check(lib().vqa_si_combine(pbuf, wbuf, copies, ptr(out), out.numel(), stream_for(out)), "vqa_si_combine")
    return out


def linf_si_step(x, grads, x0, weights, eps_iter, eps, clip_min, clip_max, flag=None, out=None):
    """``si_combine`` and ``linf_step`` on its result in one pass, 4 * copies + 12 B/element; ``x0=None``: and
    ``linf_fgm`` (no projection).  The combined gradient never reaches memory; ``out`` may be ``x``."""
    pbuf, wbuf, copies = _si_grads(grads, weights)
    out, mode, lo, hi = _fused_step_args(x, grads[0], x0, clip_min, clip_max, flag, out, what="grads")
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_linf_si_step(ptr(x), pbuf, wbuf, copies, ptr(x0), ptr(out), x.numel(), eps_iter, eps, lo, hi,
                                     mode, ptr(flag), stream_for(x)), "vqa_linf_si_step")
    return out


# ----------------------------------------------------------------------------------------- mixed-image copies (Admix)
ADMIX_MAX_IMAGES = 8   # mixed groups per gradient evaluation (the paper's m2 = 3)


def _admix_images(images):
    if isinstance(images, (bool, np.bool_)) or not isinstance(images, (int, np.integer)) or \
            not 1 <= int(images) <= ADMIX_MAX_IMAGES:
        raise ValueError("images must be an int in 1..{}, got {!r}".format(ADMIX_MAX_IMAGES, images))
    return int(images)


def admix_draw(rng, batch, n_evals, images):
    """The partner table of ``n_evals`` gradient evaluations as an int32 numpy array ``(n_evals, images, batch)``: entry
    ``[t, j, b]`` is the sample that group ``j`` of evaluation ``t`` mixes into sample ``b``, uniform over the OTHER
    samples of the batch.  ``rng`` is anything with ``.uniform`` (``np.random``, a ``RandomState``, a ``Generator``); one
    draw ``u`` per entry, in the order evaluation, group, sample: ``k = min(int(u * (batch - 1)), batch - 2)``,
    ``partner = (b + 1 + k) mod batch``."""
    batch, n_evals, images = int(batch), int(n_evals), _admix_images(images)
    if batch < 2:
        raise ValueError("admix_draw: mixing needs another sample of the batch, got batch {}".format(batch))
    if n_evals < 0:
        raise ValueError("admix_draw: n_evals must be >= 0, got {}".format(n_evals))
    table = np.empty((n_evals, images, batch), dtype=np.int32)
    for t in range(n_evals):
        for j in range(images):
            for b in range(batch):
                k = min(int(rng.uniform() * (batch - 1)), batch - 2)
                table[t, j, b] = (b + 1 + k) % batch
    return table


def admix_check_table(table, batch):
    """``table`` as a C-contiguous int32 numpy array ``(..., batch)`` with every entry in ``[0, batch)`` and none equal to
    its own index along the last axis."""
    t = np.asarray(table)
    if t.dtype.kind not in "iu" or t.ndim < 1 or t.shape[-1] != int(batch):
        raise ValueError("an Admix partner table is an integer array (..., {}), got dtype {} shape {}".format(
            batch, t.dtype, t.shape))
    t = t.astype(np.int64)
    own = np.arange(int(batch), dtype=np.int64)
    bad = (t < 0) | (t >= int(batch)) | (t == own)
    if bad.any():
        where = np.unravel_index(int(np.flatnonzero(bad.reshape(-1))[0]), t.shape)
        raise ValueError("Admix partner {} at {} is outside [0, {}) or is the sample itself".format(
            int(t[where]), tuple(int(v) for v in where), batch))
    return np.ascontiguousarray(t.astype(np.int32))


def admix_partners(table, batch, device):
    """Validate a partner table against ``batch`` (every entry in range and not its own sample) and upload it in one
    copy: an int32 device tensor of the table's shape.  The copies kernel reads one ``(batch,)`` row of it per launch."""
    return torch.from_numpy(admix_check_table(table, batch)).to(device)


def admix_weights(scales, images):
    """``w_i = float32(s_i) / float32(n * images)``: the paper's average over the ``n`` copies of each of the ``images``
    mixed groups, with the chain rule through the scaling.  ``images = 1`` gives ``si_weights(scales)``."""
    s, _ = _si_host(scales, "scales")
    return (s / np.float32(s.size * _admix_images(images))).astype(np.float32)


def _admix_row(row, batch):
    if not isinstance(row, torch.Tensor) or not row.is_cuda or row.dtype != torch.int32 or not row.is_contiguous() \
            or tuple(row.shape) != (batch,):
        raise ValueError("partner_row must be a contiguous int32 device tensor ({},) (ops.admix_partners), got {}".format(
            batch, (row.dtype, tuple(row.shape), str(row.device)) if isinstance(row, torch.Tensor) else type(row)))
    return row


def admix_copies(x, partner_row, scales, eta, m=None, lookahead=0.0, out=None):
    """``out[i][b] = s_i * ((x[b] [+ lookahead * m[b]]) + eta * x[partner_row[b]])``: the scaled copies of ONE mixed group
    in one launch, as an ``(n,) + x.shape`` tensor; the first axis of ``x`` is the batch.  No clamp, no projection.  An
    entry of the row outside ``[0, B)`` never addresses memory (the kernel takes it for ``b``); ``admix_partners`` refuses
    such a table on the host.  ``out`` must not overlap ``x``, ``m`` or the row; each ``out[i]`` must be contiguous, and
    the copies may lie further apart than ``x.numel()`` (the batch prefix of a larger buffer)."""
    s, buf = _si_host(scales, "scales")
    dev_f32(x, "x")
    if x.dim() < 1:
        raise ValueError("x must have a batch axis")
    _momentum_like(x, m)
    batch = x.shape[0]
    _admix_row(partner_row, batch)
    same_device(x, m, out, partner_row)
    out, stride = _copies_out(x, int(s.size), out, ("out[i]", "copies"))
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_admix_copies(ptr(x), ptr(m), ctypes.c_void_p(partner_row.data_ptr()), ptr(out), batch,
                                     x.numel() // batch, stride, buf, int(s.size), float(eta), float(lookahead),
                                     stream_for(x)), "vqa_admix_copies")
    return out


def _acc_like(acc, g0):
    dev_f32(acc, "acc")
    if acc.shape != g0.shape:
        raise ValueError("acc has shape {}, grads[0] {}".format(tuple(acc.shape), tuple(g0.shape)))


def admix_accumulate(grads, weights, acc):
    """``acc = (...((acc + w_0 * g_0) + w_1 * g_1) + ...)`` exactly in place (ascending, one rounding per operation): the
    running sum of a mixed group after the first, which ``si_combine`` starts.  ``acc`` may alias no gradient."""
    pbuf, wbuf, copies = _si_grads(grads, weights)
    _acc_like(acc, grads[0])
    same_device(grads[0], acc)
    if acc.numel() == 0:
        return acc
    with _on(acc):
        check(lib().vqa_admix_accumulate(ptr(acc), pbuf, wbuf, copies, acc.numel(), stream_for(acc)),
              "vqa_admix_accumulate")
    return acc


def linf_admix_step(x, acc, grads, x0, weights, eps_iter, eps, clip_min, clip_max, flag=None, out=None):
    """``admix_accumulate`` and ``linf_step`` on its result in one pass, 4 * copies + 16 B/element; ``x0=None``: and
    ``linf_fgm`` (no projection).  Neither the sum nor ``acc`` is written; ``out`` may be ``x``."""
    pbuf, wbuf, copies = _si_grads(grads, weights)
    _acc_like(acc, grads[0])
    out, mode, lo, hi = _fused_step_args(x, grads[0], x0, clip_min, clip_max, flag, out, also=(acc,), what="grads")
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_linf_admix_step(ptr(x), ptr(acc), pbuf, wbuf, copies, ptr(x0), ptr(out), x.numel(), eps_iter,
                                        eps, lo, hi, mode, ptr(flag), stream_for(x)), "vqa_linf_admix_step")
    return out


# ----------------------------------------------------------------------------------------- variance tuning (VMI / VNI-FGSM)
VT_MAX_CHUNK = 8       # VQA_VT_MAX_CHUNK of include/vqattack_hip.h (vqa_vt_max_chunk())
VT_MAX_NEIGHBORS = 64


def vt_key_table(seed, n_evals, device):
    """The ``(n_evals, 3)`` uint32 device table of ``vt_neighbors`` keys, row ``t`` = ``(seed & 0xffffffff, seed >> 32,
    t)``, uploaded in one copy."""
    seed, n_evals = int(seed), int(n_evals)
    if seed < 0 or seed >= 1 << 64:
        raise ValueError("seed must be in [0, 2^64), got {}".format(seed))
    if n_evals < 0 or n_evals >= 1 << 32:
        raise ValueError("n_evals must be in [0, 2^32), got {}".format(n_evals))
    table = np.empty((n_evals, 3), dtype=np.uint32)
    table[:, 0] = seed & 0xFFFFFFFF
    table[:, 1] = seed >> 32
    table[:, 2] = np.arange(n_evals, dtype=np.uint32)
    return torch.from_numpy(table).to(device)


def _vt_key(key):
    if not isinstance(key, torch.Tensor):
        raise TypeError("key must be a torch.Tensor, got {}".format(type(key)))
    if not key.is_cuda:
        raise _hip.HipExtensionError("key lives on '{}': there is no CPU fallback".format(key.device))
    if key.dtype != torch.uint32 or tuple(key.shape) != (3,) or not key.is_contiguous():
        raise ValueError("key must be a contiguous uint32 row (seed_lo, seed_hi, t), got {} {}".format(
            key.dtype, tuple(key.shape)))
    return key


def vt_neighbors(x, key, count, bound, first=0, m=None, lookahead=0.0, block_offset=0, out=None):
    """``out[c] = base + r_{first + c}``, ``c < count <= VT_MAX_CHUNK``: the neighbours ``first .. first + count - 1`` of
    the evaluation whose ``(seed_lo, seed_hi, t)`` the device row ``key`` holds, in one launch, as a ``(count,) +
    x.shape`` tensor.  ``base`` is ``x``, or ``x + lookahead * m`` with the momentum ``m``; ``r ~ U[-bound, bound)`` per
    element from Philox4x32-10 (include/vqattack_hip.h states counter, key and the word-to-value chain).  No clamp.
    ``out`` must not overlap ``x``, ``m`` or ``key``; each ``out[c]`` must be contiguous, and the neighbours may lie further
    apart than ``x.numel()`` (the batch prefix of a larger buffer)."""
    count, first, block_offset = int(count), int(first), int(block_offset)
    if count < 1 or count > VT_MAX_CHUNK:
        raise ValueError("count must be in 1..{}, got {}".format(VT_MAX_CHUNK, count))
    if first < 0 or first + count > 1 << 31:
        raise ValueError("first must be >= 0 and first + count <= 2^31, got {}".format(first))
    if block_offset < 0 or block_offset >= 1 << 64:
        raise ValueError("block_offset must be in [0, 2^64), got {}".format(block_offset))
    dev_f32(x, "x")
    _vt_key(key)
    _momentum_like(x, m)
    same_device(x, m, out, key)
    out, stride = _copies_out(x, count, out, ("out[c]", "neighbours"))
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_vt_neighbors(ptr(x), ptr(m), ptr(out), x.numel(), stride, count, first, block_offset,
                                     float(bound), float(lookahead), ctypes.c_void_p(key.data_ptr()), stream_for(x)),
              "vqa_vt_neighbors")
    return out


def vt_accumulate(grads, sum, init):
    """``sum = (g_0 if init else sum + g_0) + g_1 + ...`` in place (ascending, one rounding per addition): 1..VT_MAX_CHUNK
    gradients per launch; grouping them differently gives the same bits.  ``sum`` may alias no gradient."""
    pbuf = _grad_ptrs(grads, VT_MAX_CHUNK, like=sum)
    same_device(sum, *grads)
    if sum.numel() == 0:
        return sum
    with _on(sum):
        check(lib().vqa_vt_accumulate(pbuf, len(grads), ptr(sum), sum.numel(), 1 if init else 0, stream_for(sum)),
              "vqa_vt_accumulate")
    return sum


def _vt_state(g, vsum, v):
    dev_f32(g, "grad"), dev_f32(vsum, "vsum"), dev_f32(v, "v")
    if vsum.shape != g.shape or v.shape != g.shape:
        raise ValueError("shape mismatch: grad {}, vsum {}, v {}".format(tuple(g.shape), tuple(vsum.shape),
                                                                         tuple(v.shape)))


def vt_tune(g, vsum, v, w, out=None):
    """``out = g + v`` and then ``v = w * vsum - g`` in place, one pass, 20 B/element; returns ``out`` (the tuned gradient).
    ``out`` may be ``g``; no other two of the four may overlap."""
    _vt_state(g, vsum, v)
    same_device(g, vsum, v, out)
    out = _out_like(g, out)
    if g.numel() == 0:
        return out
    with _on(g):
        check(lib().vqa_vt_tune(ptr(g), ptr(vsum), ptr(v), ptr(out), g.numel(), float(w), stream_for(g)), "vqa_vt_tune")
    return out


def linf_vt_step(x, g, vsum, v, x0, w, eps_iter, eps, clip_min, clip_max, flag=None, out=None):
    """``vt_tune`` and ``linf_step`` on its result in one pass, 28 B/element; ``x0=None``: and ``linf_fgm`` (no
    projection).  The tuned gradient never reaches memory; ``v`` is updated in place; ``out`` may be ``x``."""
    _vt_state(g, vsum, v)
    out, mode, lo, hi = _fused_step_args(x, g, x0, clip_min, clip_max, flag, out, also=(vsum, v))
    if x.numel() == 0:
        return out
    with _on(x):
        check(lib().vqa_linf_vt_step(ptr(x), ptr(g), ptr(vsum), ptr(v), ptr(x0), ptr(out), x.numel(), float(w), eps_iter,
                                     eps, lo, hi, mode, ptr(flag), stream_for(x)), "vqa_linf_vt_step")
    return out


# ----------------------------------------------------------------------------------------- loss
_COS_EPS = 1e-6 # nn.CosineSimilarity(eps=1e-6) in the reference
_partials = {}


def _partial_buf(device):
    """Per-(device, stream) scratch for the loss partials: launches on one stream are ordered, so reuse is safe."""
    # zero-initialised: the last word is the arrival counter of the in-kernel fold (the folding workgroup resets it)
    if torch.cuda.is_current_stream_capturing():
        # inside hipGraph capture the scratch must live in that graph's private pool: never cache it
        return torch.zeros(lib().vqa_neg_cos_partials(), dtype=torch.float32, device=device)
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = _partials.get(key)
    if buf is None:
        buf = torch.zeros(lib().vqa_neg_cos_partials(), dtype=torch.float32, device=device)
        _partials[key] = buf
    return buf


class Workspace:
    """Scratch tensors one attack call owns and reuses across its iterations: the loss kernels' gradient buffers
    (4.5 GB per launch at VLMO-base batch 64) and the cross-entropy row buffers.  A buffer handed out here is dead once
    ``torch.autograd.backward`` has consumed it, i.e. before the next iteration asks again for the same key."""

    def __init__(self):
        self._bufs = {}

    def get(self, key, shape, dtype, device, zero=False):
        """A buffer per ROLE (``key``), not per shape: one flat allocation sized for the largest request so far, handed
        out as a prefix view -- a driver whose active batch shrinks (``attack_mixed``: finished samples leave the batch)
        keeps ONE set of buffers instead of one per batch size.  ``zero=True``: zero-filled when (re)allocated, and only
        then; a smaller request of the same role sees the same leading rows."""
        if torch.cuda.is_current_stream_capturing():
            return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=device)
        numel = 1
        for n in shape:
            numel *= int(n)
        full = (key, dtype, device)
        buf = self._bufs.get(full)
        if buf is None or buf.numel() < numel:
            buf = (torch.zeros if zero else torch.empty)(max(numel, 1), dtype=dtype, device=device)
            self._bufs[full] = buf
        return buf[:numel].view(shape)

    def persistent(self):
        """True when a buffer handed out under a key is the SAME memory on the next request (not during graph capture)."""
        return not torch.cuda.is_current_stream_capturing()


def _scratch(ws, key, shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device) if ws is None else ws.get(key, shape, dtype, device)


def _rows_view(t, name):
    """(rows0, rows1, D, stride0, stride1) of a 2-d or 3-d fp32 tensor whose last dim is dense."""
    if t.dim() == 2:
        r0, r1, d = 1, t.shape[0], t.shape[1]
        s0, s1 = 0, t.stride(0)
    elif t.dim() == 3:
        r0, r1, d = t.shape
        s0, s1 = t.stride(0), t.stride(1)
    else:
        raise ValueError("{} must be 2-d (rows, D) or 3-d (rows0, rows1, D), got {}".format(name, tuple(t.shape)))
    return r0, r1, d, s0, s1


def _kernel_ready(t):
    if t.dim() < 2:
        return False
    if t.stride(-1) != 1 and t.shape[-1] > 1:
        return False
    if t.data_ptr() % 16:
        return False
    return all(s % 4 == 0 for s in t.stride()[:-1])


def neg_cos_rows(a, b, loss_out, accumulate, gscale=1.0, want_grad=True, row_weight=None, weight_period=1, ws=None):
    """loss_out[0] (+)= gscale * sum_rows -cos(a_row, b_row); returns d(that)/d a (same shape as ``a``) or None.

    ``a`` / ``b`` may be strided views (the reference's ``[:, :feat_len, :]`` truncations) as long as rows are
    dense.  ``loss_out`` is a 1-element fp32 device tensor (a slot of the attack's loss buffer).
    ``row_weight`` (uint8, ``weight_period * rows1`` entries): per-row integer weight, indexed by
    ``(outer % weight_period, inner)``; 0 drops a row (padded token), 2 counts it twice.
    """
    dev_f32(a, "out", contiguous=False), dev_f32(b, "y", contiguous=False)
    if a.shape != b.shape:
        raise ValueError("feature/target shape mismatch: {} vs {}".format(tuple(a.shape), tuple(b.shape)))
    d = a.shape[-1]
    if d % 4 or d > 2048:
        raise _hip.HipExtensionError("feature dim {} unsupported by vqa_neg_cos_rows (multiple of 4, <= 2048)".format(d))
    if not _kernel_ready(a):
        a = a.contiguous()
    if not _kernel_ready(b):
        b = b.contiguous()
    r0, r1, d, a0, a1 = _rows_view(a, "out")
    _, _, _, b0, b1 = _rows_view(b, "y")
    ga = None
    g0 = g1 = 0
    if want_grad:
        ga = _scratch(ws, "cos1", a.shape, torch.float32, a.device)
        _, _, _, g0, g1 = _rows_view(ga, "grad")
    if row_weight is not None:
        if row_weight.dtype != torch.uint8 or not row_weight.is_cuda or not row_weight.is_contiguous():
            raise TypeError("row_weight must be a contiguous uint8 device tensor")
        if row_weight.numel() != weight_period * r1:
            raise ValueError("row_weight has {} entries, expected weight_period*rows1 = {}".format(
                row_weight.numel(), weight_period * r1))
    if a.numel() == 0:                 # no rows: zero loss contribution, empty gradient
        if not accumulate and loss_out is not None:
            loss_out.zero_()
        return ga
    part = _partial_buf(a.device)
    with _on(a):
        st = stream_for(a)
        check(lib().vqa_neg_cos_rows(ptr(a), ptr(b), ptr(ga), ptr(part), ptr(row_weight), weight_period, r0, r1, d,
                                     a0, a1, b0, b1, g0, g1, gscale, _COS_EPS, ptr(loss_out), 1 if accumulate else 0,
                                     st), "vqa_neg_cos_rows")      # loss folded by the last workgroup: one launch
    return ga


class SubWorkspace:
    """A view of a Workspace whose keys are prefixed (per-layer fallback launches must not share one buffer)."""

    def __init__(self, ws, tag):
        self.ws, self.tag = ws, tag

    def get(self, key, shape, dtype, device, zero=False):
        return self.ws.get((self.tag, key), shape, dtype, device, zero=zero)

    def persistent(self):
        return self.ws.persistent()


def neg_cos_rows_multi(a_list, b_list, loss_out, accumulate, gscale=1.0, want_grad=True, row_weight=None,
                       weight_period=1, ws=None):
    """``neg_cos_rows`` over a list of same-shaped feature maps in ONE launch; returns the list of gradients (views of
    one ``(L, ...)`` buffer) or None.  Falls back to per-map launches when the maps do not share shape and strides."""
    n = len(a_list)
    if n != len(b_list) or n == 0:
        raise ValueError("need as many targets as feature maps")
    a0, b0 = a_list[0], b_list[0]
    uniform = (n <= lib().vqa_neg_cos_max_layers() and a0.numel() > 0 and
               all(t.shape == a0.shape and t.stride() == a0.stride() and t.dtype == torch.float32 and t.is_cuda and
                   _kernel_ready(t) for t in a_list) and
               all(t.shape == a0.shape and t.stride() == b0.stride() and t.dtype == torch.float32 and t.is_cuda and
                   _kernel_ready(t) for t in b_list) and a0.shape[-1] % 4 == 0 and a0.shape[-1] <= 2048)
    if not uniform or n == 1:
        grads = []
        for k, (a, b) in enumerate(zip(a_list, b_list)):
            grads.append(neg_cos_rows(a, b, loss_out, accumulate or k > 0, gscale, want_grad, row_weight, weight_period,
                                      ws=None if ws is None else SubWorkspace(ws, k)))
        return grads if want_grad else None
    r0, r1, d, sa0, sa1 = _rows_view(a0, "out")
    _, _, _, sb0, sb1 = _rows_view(b0, "y")
    ga = None
    g0 = g1 = 0
    if want_grad:
        ga = _scratch(ws, "cosN", (n,) + tuple(a0.shape), torch.float32, a0.device)
        _, _, _, g0, g1 = _rows_view(ga[0], "grad")
    if row_weight is not None:
        if row_weight.dtype != torch.uint8 or not row_weight.is_cuda or not row_weight.is_contiguous():
            raise TypeError("row_weight must be a contiguous uint8 device tensor")
        if row_weight.numel() != weight_period * r1:
            raise ValueError("row_weight has {} entries, expected weight_period*rows1 = {}".format(
                row_weight.numel(), weight_period * r1))
    arr = ctypes.c_void_p * n
    pa = arr(*[t.data_ptr() for t in a_list])
    pb = arr(*[t.data_ptr() for t in b_list])
    pg = arr(*[ga[i].data_ptr() for i in range(n)]) if want_grad else None
    part = _partial_buf(a0.device)
    with _on(a0):
        st = stream_for(a0)
        check(lib().vqa_neg_cos_rows_multi(pa, pb, pg, n, ptr(part), ptr(row_weight), weight_period, r0, r1, d, sa0, sa1,
                                           sb0, sb1, g0, g1, gscale, _COS_EPS, ptr(loss_out), 1 if accumulate else 0,
                                           st), "vqa_neg_cos_rows_multi")
    return [ga[i] for i in range(n)] if want_grad else None


def mlm_cross_entropy(logits, label_sets, loss_out, accumulate, gscale=1.0, want_grad=True, ignore_index=-100,
                      flag=None, ws=None, rows_per_sample=0):
    """loss_out[0] (+)= gscale * sum_k CE_mean(logits, label_sets[k]); returns d(that)/d logits or None.

    ``logits`` (..., V) fp32 with dense rows; ``label_sets`` int64 (K, rows) -- K label sets over the same rows
    (K = 1 for the reference's 2-d labels, K = labels.shape[1] for its 3-d labels).
    ``rows_per_sample``: 0 -> every label set is a mean over ALL rows (``F.cross_entropy`` on the batch, the reference's
    op); L -> rows are grouped per sample (L consecutive rows) and each sample's label sets are normalised by that
    sample's own valid-label counts, i.e. the batch-1 reference's loss summed over the samples of a batched attack.
    A label outside ``[0, V)`` that is not ``ignore_index`` makes the loss NaN and sets ``VQA_FLAG_BAD_LABEL`` in
    ``flag`` (int32 device word, optional) -- torch device-asserts there; nothing is silently dropped.
    """
    dev_f32(logits, "logits", contiguous=False)
    v = logits.shape[-1]
    flat = logits.reshape(-1, v)
    if flat.stride(1) != 1:
        flat = flat.contiguous()
    rows = flat.shape[0]
    if label_sets.dtype != torch.int64 or not label_sets.is_cuda:
        raise TypeError("label_sets must be an int64 device tensor")
    label_sets = label_sets.reshape(-1, rows).contiguous()
    k = label_sets.shape[0]
    if k > lib().vqa_ce_max_label_sets():
        raise _hip.HipExtensionError("at most {} label sets per launch".format(lib().vqa_ce_max_label_sets()))
    # With a workspace the gradient buffer is the same memory in every iteration of the attack: it is zero-filled once
    # and a byte per row remembers whether the row holds a live gradient, so the rows whose labels are all ignore_index
    # (>= 90 % of a dense (B, L, V) logits tensor in the reference's workload) are never written again.
    grad = row_state = None
    if want_grad:
        if ws is not None and ws.persistent() and rows > 0:
            grad = ws.get(("ce_grad", v), (rows, v), torch.float32, logits.device, zero=True)
            row_state = ws.get(("ce_row_state", v), (rows,), torch.uint8, logits.device, zero=True)
        else:
            grad = torch.empty((rows, v), dtype=torch.float32, device=logits.device)
    groups = 1 if rows_per_sample in (0, None) or rows == 0 else -(-rows // int(rows_per_sample))
    scratch = _scratch(ws, "ce_scratch", (max(int(lib().vqa_ce_scratch_floats(k, groups)), 1),), torch.float32,
                       logits.device)
    row_loss = _scratch(ws, "ce_rows", (max(rows, 1),), torch.float32, logits.device)
    with _on(logits):
        check(lib().vqa_ce_rows(ptr(flat), flat.stride(0), ctypes.c_void_p(label_sets.data_ptr()), k, rows, v,
                                ignore_index, int(rows_per_sample or 0), ptr(scratch), ptr(grad), ptr(row_loss), gscale,
                                ptr(loss_out), 1 if accumulate else 0, ptr(flag),
                                None if row_state is None else ctypes.c_void_p(row_state.data_ptr()),
                                stream_for(logits)), "vqa_ce_rows")
    return grad.reshape(logits.shape) if want_grad else None


# ----------------------------------------------------------------------------------------- text side
class RowIndex:
    """A validated, device-resident int64 index for ``gather_rows`` (``text_emb_pick`` / ``attack_mask``): build it once
    per attack and reuse it every iteration -- no per-call host check, no host->device copy, and a device-tensor index
    is read back exactly once."""

    def __init__(self, index, length, device):
        if not isinstance(index, torch.Tensor):
            index = torch.as_tensor(list(index), dtype=torch.int64)
        host = index.detach().cpu().to(torch.int64).reshape(-1)
        if host.numel() and (int(host.max()) >= length or int(host.min()) < -length):
            raise IndexError("index out of range for dimension 1 with size {}".format(length))
        self.length = length
        self.device_index = host.to(device)

    def __len__(self):
        return self.device_index.numel()


def gather_rows(src, index):
    """src (B, L, D)[:, index] -> (B, K, D).  ``index``: list / tensor (validated on every call) or a ``RowIndex``."""
    dev_f32(src, "text gradient")
    if src.dim() != 3:
        raise ValueError("text gradient must be (B, L, D)")
    b, l, d = src.shape
    if not isinstance(index, RowIndex):
        index = RowIndex(index, l, src.device)
    elif index.length != l or index.device_index.device != src.device:
        raise ValueError("RowIndex was prepared for length {} on {}".format(index.length, index.device_index.device))
    idx = index.device_index
    k = idx.numel()
    dst = torch.empty((b, k, d), dtype=torch.float32, device=src.device)
    if k == 0 or b == 0:
        return dst
    with _on(src):
        check(lib().vqa_gather_rows(ptr(src), ctypes.c_void_p(idx.data_ptr()), ptr(dst), b, l, k, d,
                                    stream_for(src)), "vqa_gather_rows")
    return dst


def cand_dir_sim(word, pos, type_emb, gamma, beta, ln_eps, e_ori, grad, cand):
    """Scores of candidate substitutions, one fp32 per row of ``cand`` (int32 (n, 4) = sample, position, grad row, id)."""
    for name, t in (("word", word), ("pos", pos), ("type", type_emb), ("gamma", gamma), ("beta", beta),
                    ("e_ori", e_ori), ("grad", grad)):
        dev_f32(t, name)
    if cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[1] != 4 or not cand.is_cuda:
        raise TypeError("cand must be an int32 (n, 4) device tensor")
    cand = cand.contiguous()
    n = cand.shape[0]
    d = word.shape[1]
    _, l, _ = e_ori.shape
    _, k, _ = grad.shape
    out = torch.empty(n, dtype=torch.float32, device=word.device)
    with _on(word):
        check(lib().vqa_cand_dir_sim(ptr(word), ptr(pos), ptr(type_emb), ptr(gamma), ptr(beta), ln_eps, ptr(e_ori),
                                     ptr(grad), ctypes.c_void_p(cand.data_ptr()), ptr(out), n, l, k, d,
                                     stream_for(word)), "vqa_cand_dir_sim")
    return out


def embed_tokens(tables, text_ids, out=None, rows=None):
    """BERT embeddings ``LN(word[id] + type[0] + pos[p])`` on the device in one launch.

    ``text_ids`` (B, L) int64.  ``rows=None`` embeds every token into a fresh (or given) ``(B, L, D)`` tensor;
    ``rows`` = int tensor/list of ``(sample, position)`` pairs rewrites only those rows of ``out`` in place (the words
    the joint attack just substituted) using the ids currently in ``text_ids``.
    """
    word = tables["word"]
    dev_f32(word, "word")
    b, l = text_ids.shape
    d = word.shape[1]
    if out is None:
        if rows is not None:
            raise ValueError("rows=... updates an existing embedding tensor: pass out=")
        out = torch.empty(b, l, d, dtype=torch.float32, device=word.device)
    else:
        dev_f32(out, "out")
        if tuple(out.shape) != (b, l, d):
            raise ValueError("out must be ({}, {}, {})".format(b, l, d))
    ids = text_ids.to(word.device)
    if rows is None:
        s_idx = torch.arange(b, device=word.device).repeat_interleave(l)
        p_idx = torch.arange(l, device=word.device).repeat(b)
    else:
        rows = torch.as_tensor(rows, device=word.device, dtype=torch.int64).reshape(-1, 2)
        s_idx, p_idx = rows[:, 0], rows[:, 1]
    triples = torch.stack([s_idx * l + p_idx, p_idx, ids[s_idx, p_idx]], dim=1).to(torch.int32).contiguous()
    with _on(word):
        check(lib().vqa_embed_tokens(ptr(word), ptr(tables["pos"]), ptr(tables["type_emb"]), ptr(tables["gamma"]),
                                     ptr(tables["beta"]), tables["ln_eps"], ctypes.c_void_p(triples.data_ptr()),
                                     triples.shape[0], ptr(out), d, stream_for(word)), "vqa_embed_tokens")
    return out


def greedy_accept(cand, scores, ori_ids, cur_ids, table, threshold):
    """Device-side acceptance of one substitution round (``vqa_greedy_accept``); no host synchronisation.

    ``cand`` int32 (n, 4) device rows {sample, position, grad row, id}; ``scores`` fp32 (n,) their dir_sim;
    ``ori_ids`` / ``cur_ids`` int64 (B, L) device (``cur_ids`` is updated IN PLACE); ``table`` fp32 (V, E) sentence-encoder
    stand-in.  Returns ``(new_id, rank)`` int32 (B, L): the accepted id per position (-1 elsewhere) and the order in which
    the sample accepted it."""
    dev_f32(table, "table"), dev_f32(scores, "scores")
    if cand.dtype != torch.int32 or cand.dim() != 2 or cand.shape[1] != 4 or not cand.is_cuda:
        raise TypeError("cand must be an int32 (n, 4) device tensor")
    for name, t in (("ori_ids", ori_ids), ("cur_ids", cur_ids)):
        if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or t.dim() != 2:
            raise TypeError("{} must be a contiguous int64 (B, L) device tensor".format(name))
    b, l = cur_ids.shape
    if tuple(ori_ids.shape) != (b, l):
        raise ValueError("ori_ids / cur_ids shape mismatch")
    if l > 64:
        raise _hip.HipExtensionError("vqa_greedy_accept holds one token per lane: L <= 64, got {}".format(l))
    cand = cand.contiguous()
    n = cand.shape[0]
    # candidates grouped by sample, best dir_sim first; both sorts are stable, so ties keep their proposal order like
    # python's sorted(..., reverse=True) in the reference
    by_score = torch.argsort(scores, descending=True, stable=True)
    by_sample = torch.argsort(cand[by_score, 0], stable=True)
    order = by_score[by_sample].to(torch.int32).contiguous()
    counts = torch.bincount(cand[:, 0].to(torch.int64), minlength=b)[:b] if n else torch.zeros(b, dtype=torch.int64,
                                                                                               device=cur_ids.device)
    seg = torch.zeros(b + 1, dtype=torch.int32, device=cur_ids.device)
    seg[1:] = torch.cumsum(counts, 0).to(torch.int32)
    new_id = torch.empty((b, l), dtype=torch.int32, device=cur_ids.device)
    rank = torch.empty((b, l), dtype=torch.int32, device=cur_ids.device)
    with _on(cur_ids):
        check(lib().vqa_greedy_accept(ctypes.c_void_p(cand.data_ptr()), ctypes.c_void_p(order.data_ptr()),
                                      ctypes.c_void_p(seg.data_ptr()), b, l, ctypes.c_void_p(ori_ids.data_ptr()),
                                      ctypes.c_void_p(cur_ids.data_ptr()), ctypes.c_void_p(new_id.data_ptr()),
                                      ctypes.c_void_p(rank.data_ptr()), ptr(table), table.shape[0], table.shape[1],
                                      float(threshold), stream_for(cur_ids)), "vqa_greedy_accept")
    return new_id, rank


# ----------------------------------------------------------------------------------------- white-box block glue
def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _rows_ok(name, t, numel):
    """The block-glue kernels index raw pointers from the row count: every operand is checked for device, dtype, layout
    and SIZE here (a short buffer would be an out-of-bounds access on the device, not an exception)."""
    if t is None:
        return
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise TypeError("{} must be a contiguous float32 HIP tensor".format(name))
    if t.numel() != numel:
        raise ValueError("{} has {} elements, expected {}".format(name, t.numel(), numel))


def _split_sizes(rows, d, period, split, second):
    """(elements of the segment-0 buffer, of the segment-1 buffer) of a tensor given whole or split."""
    if second is None:
        return rows * d, 0
    if period <= 0 or rows % period or not 0 <= split <= period:
        raise ValueError("a split tensor needs period > 0 dividing the row count and 0 <= split <= period")
    n0 = rows // period * split
    return n0 * d, (rows - n0) * d


def ln_fwd(x, gamma0, beta0, y0, mean, rstd, eps, r0=None, r1=None, rscale=None, x_out=None, gamma1=None, beta1=None,
           y1=None, period=0, split=0):
    """``vqa_ln_fwd`` on ``x`` (rows, D) fp32 contiguous: optional prologue ``x_out = x + rscale * r`` (r whole as ``r0`` or
    split as ``r0`` / ``r1``), then LayerNorm with the second parameter set for segment-1 rows, output whole (``y0``) or
    split (``y0`` / ``y1``).  Token layout: ``period`` rows per batch element, the first ``split`` are segment 0."""
    rows, d = x.numel() // x.shape[-1], x.shape[-1]
    _rows_ok("x", x, rows * d), _rows_ok("x_out", x_out, rows * d)
    for name, t in (("gamma0", gamma0), ("beta0", beta0), ("gamma1", gamma1), ("beta1", beta1), ("rscale", rscale)):
        _rows_ok(name, t, d)
    _rows_ok("mean", mean, rows), _rows_ok("rstd", rstd, rows)
    for name, t0, t1 in (("r", r0, r1), ("y", y0, y1)):
        n0, n1 = _split_sizes(rows, d, period, split, t1)
        _rows_ok(name + "0", t0, n0), _rows_ok(name + "1", t1, n1)
    with _on(x):
        check(lib().vqa_ln_fwd(_p(x), _p(r0), _p(r1), _p(rscale), _p(x_out), _p(gamma0), _p(beta0), _p(gamma1), _p(beta1),
                               _p(y0), _p(y1), _p(mean), _p(rstd), rows, d, period, split, eps, stream_for(x)),
              "vqa_ln_fwd")


def ln_bwd(dy0, x, mean, rstd, gamma0, dx, dy1=None, gamma1=None, g_a=None, g_inj=None, rscale=None, dr0=None, dr1=None,
           period=0, split=0):
    """``vqa_ln_bwd``: ``dx = g_a + g_inj + LayerNorm'(dy)`` and optionally ``dr = rscale * dx`` (whole or split)."""
    rows, d = x.numel() // x.shape[-1], x.shape[-1]
    for name, t in (("x", x), ("dx", dx), ("g_a", g_a), ("g_inj", g_inj)):
        _rows_ok(name, t, rows * d)
    for name, t in (("gamma0", gamma0), ("gamma1", gamma1), ("rscale", rscale)):
        _rows_ok(name, t, d)
    _rows_ok("mean", mean, rows), _rows_ok("rstd", rstd, rows)
    for name, t0, t1 in (("dy", dy0, dy1), ("dr", dr0, dr1)):
        n0, n1 = _split_sizes(rows, d, period, split, t1)
        _rows_ok(name + "0", t0, n0), _rows_ok(name + "1", t1, n1)
    with _on(x):
        check(lib().vqa_ln_bwd(_p(dy0), _p(dy1), _p(x), _p(mean), _p(rstd), _p(gamma0), _p(gamma1), _p(g_a), _p(g_inj),
                               _p(rscale), _p(dx), _p(dr0), _p(dr1), rows, d, period, split, stream_for(x)), "vqa_ln_bwd")


def ln_bwd_post(dy_a, s, rstd, gamma, ds, dy_b=None, g_inj=None):
    """``vqa_ln_bwd_post``: ``ds = LayerNorm'((dy_a + dy_b) + g_inj)`` at the saved pre-LayerNorm sum ``s`` (rows, D) of a
    post-LN block ``y = LN(s)``, ``s = x + f(x)``; ``ds`` is the gradient of ``x`` over the residual path and of ``f(x)``."""
    for name, t in (("s", s), ("dy_a", dy_a), ("ds", ds)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("{} must be a contiguous float32 HIP tensor".format(name))
    rows, d = s.numel() // s.shape[-1], s.shape[-1]
    for name, t in (("s", s), ("ds", ds), ("dy_a", dy_a), ("dy_b", dy_b), ("g_inj", g_inj)):
        _rows_ok(name, t, rows * d)
    _rows_ok("gamma", gamma, d), _rows_ok("rstd", rstd, rows)
    same_device(dy_a, dy_b, g_inj, s, rstd, gamma, ds)
    with _on(s):
        check(lib().vqa_ln_bwd_post(_p(dy_a), _p(dy_b), _p(g_inj), _p(s), _p(rstd), _p(gamma), _p(ds), rows, d,
                                    stream_for(s)), "vqa_ln_bwd_post")


def gelu_fwd(h, out=None):
    dev_f32(h, "h")
    out = torch.empty_like(h) if out is None else out
    _rows_ok("out", out, h.numel())
    if h.numel():
        with _on(h):
            check(lib().vqa_gelu_fwd(_p(h), _p(out), h.numel(), stream_for(h)), "vqa_gelu_fwd")
    return out


def gelu_bwd(h, da, out=None):
    """``out = da * gelu'(h)``; ``out=None`` overwrites ``da``."""
    dev_f32(h, "h"), dev_f32(da, "da")
    out = da if out is None else out
    _rows_ok("da", da, h.numel()), _rows_ok("out", out, h.numel())
    if h.numel():
        with _on(h):
            check(lib().vqa_gelu_bwd(_p(h), _p(da), _p(out), h.numel(), stream_for(h)), "vqa_gelu_bwd")
    return out


class PackedWeight:
    """A frozen [K, N] GEMM operand packed for ``vqa_gemm_bf16x6``: three bf16 planes in the kernel's fragment order
    (``include/vqattack_hip.h``), held as raw bytes.  ``n_valid``: how many of the N columns are real -- N itself, except
    for an LM head padded by ``gemm_pack_vocab`` (``gemm_lse`` masks the rest)."""
    __slots__ = ("data", "K", "N", "n_valid")

    def __init__(self, data, K, N, n_valid=None):
        self.data, self.K, self.N = data, K, N
        self.n_valid = N if n_valid is None else int(n_valid)
        if not 0 < self.n_valid <= N:
            raise ValueError("n_valid must be in (0, {}], got {}".format(N, n_valid))


def gemm_shape_ok(N, K):
    """Shapes the bf16x6 kernel covers: N % 128 == 0, K % 32 == 0 (any row count)."""
    return N > 0 and K > 0 and N % 128 == 0 and K % 32 == 0


def gemm_workgroups(M, N):
    """Grid of one ``vqa_gemm_bf16x6`` launch: 256 x 128 output tiles."""
    return -(-M // 256) * (N // 128)


def gemm_pack(w, trans):
    """Pack a weight once.  ``trans=True``: the forward operand ``w.t()`` of a Linear weight ``w`` [out, in]
    (K = in, N = out); ``trans=False``: ``w`` itself, the input-gradient operand (K = out, N = in)."""
    dev_f32(w, "w")
    if w.dim() != 2:
        raise ValueError("w must be 2-D, got shape {}".format(tuple(w.shape)))
    K, N = (w.shape[1], w.shape[0]) if trans else (w.shape[0], w.shape[1])
    nbytes = lib().vqa_gemm_packed_bytes(K, N)
    if nbytes == 0:
        raise ValueError("vqa_gemm_pack_b does not cover K={}, N={}".format(K, N))
    data = torch.empty(nbytes, dtype=torch.uint8, device=w.device)
    with _on(w):
        check(lib().vqa_gemm_pack_b(_p(w), w.shape[1], int(bool(trans)), _p(data), K, N, stream_for(w)), "vqa_gemm_pack_b")
    return PackedWeight(data, K, N)


VOCAB_PAD = 256      # both large tiles take N % 256 == 0


def gemm_pack_vocab(w):
    """Pack an LM-head weight ``w`` [V, K] (logits = h @ w.t()) for ``gemm_lse``: V is padded with zero rows to a multiple
    of 256, so both tiles apply, and the result carries ``n_valid = V``."""
    dev_f32(w, "w")
    if w.dim() != 2:
        raise ValueError("w must be 2-D, got shape {}".format(tuple(w.shape)))
    V, K = w.shape
    Vp = -(-V // VOCAB_PAD) * VOCAB_PAD
    if Vp != V:
        padded = torch.zeros(Vp, K, dtype=torch.float32, device=w.device)
        padded[:V] = w
        w = padded
    packed = gemm_pack(w.contiguous(), trans=True)
    return PackedWeight(packed.data, packed.K, packed.N, V)


GEMM_TILES = {"large": 0, "wide": 1}      # VQA_GEMM_TILE_256X128, VQA_GEMM_TILE_128X256 of include/vqattack_hip.h


GEMM_EPILOGUES = {"gelu": 1, "gelu_grad": 2}   # VQA_GEMM_EPI_GELU, VQA_GEMM_EPI_GELU_GRAD of include/vqattack_hip.h


def gemm_tail_plan(M, N, tile, cus):
    """Where ``vqa_gemm_bf16x6_tail`` should cut (M, N) on ``tile`` for a device of ``cus`` compute units: the row count
    ``m_split`` of the launch's full rounds (one ``tile`` workgroup per CU at a time), the rows behind it going to the
    128 x 128 tile -- or M (no cut) where the grid is below one round or a whole number of rounds, or where those rows
    need more 128 x 128 workgroups than one round holds.  Pure arithmetic, no device."""
    if tile not in GEMM_TILES:
        raise ValueError("tile must be one of {}, got {!r}".format(sorted(GEMM_TILES), tile))
    M, N, cus = int(M), int(N), int(cus)
    bm, bn = (128, 256) if tile == "wide" and N % 256 == 0 else (256, 128)     # "wide" at another N runs "large"
    ntb = N // bn
    nwg = -(-M // bm) * ntb
    full = (nwg // cus) * cus if cus > 0 else 0
    if full == 0 or nwg == full:
        return M
    m_split = (full // ntb) * bm
    tail = -(-(M - m_split) // 128) * (N // 128)
    return m_split if tail <= cus else M


def gemm(a, packed, bias=None, out=None, tile=None, epilogue=None, aux=None, m_split=None):
    """``out = a @ B (+ bias)`` on the bf16 matrix pipe (bf16x6, fp32-grade), B a ``PackedWeight``.  ``a``: fp32 (M, K)
    with unit column stride and a row stride that is a multiple of 4 floats.  ``tile``: the output tile of a workgroup,
    "large" (256 x 128) or "wide" (128 x 256: half the in-loop split work; N % 256 == 0, any other N runs "large");
    both give the same bits.  "persistent": ``gemm_persistent`` with one workgroup per compute unit (N % 256 == 0, no
    epilogue, no m_split; the same bits).  None = what ``whitebox/_fused.py`` records for the shape (``gemm_tile``, and
    ``gemm_persistent`` for a plain product that ``gemm_tail_split`` does not cut).

    ``m_split``: None, or the row from which the 128 x 128 tile takes over (``vqa_gemm_bf16x6_tail``: rows
    ``[0, m_split)`` on ``tile``, the rest on the half tile, the same bits); 0 <= m_split <= M, no epilogue.  None leaves
    the cut to ``whitebox/_fused.py`` (``gemm_tail_split``: nowhere unless the shape is listed or VQA_GEMM_TAIL=1).

    ``epilogue``: None, or the FFN's activation applied to the accumulators inside the GEMM (``vqa_gemm_bf16x6_epi``),
    with the bits of the two-step form.  "gelu": ``out = gelu(h)`` with ``h = a @ B (+ bias)``; ``aux``, if given, is
    filled with ``h`` (``aux=None``: ``h`` is not stored at all).  "gelu_grad": ``out = (a @ B (+ bias)) * gelu'(aux)``,
    ``aux`` = the forward's ``h``.  ``aux``: fp32 (M, N) on ``a``'s device, unit column stride, any row stride >= N; it
    must not overlap ``out`` or ``a`` (the C entry point refuses ``aux == out`` / ``aux == a`` with VQA_ERR_SHAPE; the
    wrapper raises ValueError first).  Layout of ``out``: contiguous without an epilogue (``vqa_gemm_bf16x6_tile`` is
    called with ldc = N), unit column stride and any row stride >= N with one (``vqa_gemm_bf16x6_epi`` takes ldc)."""
    if epilogue is not None and epilogue not in GEMM_EPILOGUES:
        raise ValueError("epilogue must be None or one of {}, got {!r}".format(sorted(GEMM_EPILOGUES), epilogue))
    if epilogue is None and aux is not None:
        raise ValueError("aux goes with an epilogue")
    if epilogue == "gelu_grad" and aux is None:
        raise ValueError("epilogue 'gelu_grad' needs aux = the pre-activation h")
    if aux is not None:
        if aux is out:
            raise ValueError("aux must not be out")
        M = a.shape[0]
        if not isinstance(aux, torch.Tensor) or tuple(aux.shape) != (M, packed.N) or aux.stride(1) != 1 or \
                (M > 1 and aux.stride(0) < packed.N):
            raise ValueError("aux must be a ({}, {}) tensor with unit column stride, got {}".format(
                M, packed.N, (tuple(aux.shape), aux.stride()) if isinstance(aux, torch.Tensor) else type(aux)))
    if tile == "persistent":
        if epilogue is not None or m_split is not None:
            raise ValueError("tile 'persistent' goes with neither an epilogue nor m_split")
        return gemm_persistent(a, packed, bias, out)
    if tile is None:
        from .whitebox import _fused
        tile = _PolicyTile(_fused.gemm_tile(a.shape[0], packed.N, packed.K))
    if tile not in GEMM_TILES:
        raise ValueError("tile must be one of {}, got {!r}".format(sorted(GEMM_TILES) + ["persistent"], tile))
    if m_split is not None:
        if epilogue is not None:
            raise ValueError("m_split does not go with an epilogue")
        if isinstance(m_split, bool) or not isinstance(m_split, int) or not 0 <= m_split <= a.shape[0]:
            raise ValueError("m_split must be an integer in [0, {}], got {!r}".format(a.shape[0], m_split))
        return _gemm_rows(a, packed, bias, out, tile, m_split)
    if epilogue is not None:
        return _gemm_epilogue(a, packed, bias, out, tile, epilogue, aux)
    return _gemm_tiled(a, packed, bias, out, tile)


class _PolicyTile(str):
    """A tile name that ``gemm`` took from ``_fused.gemm_tile`` because its caller named none: equal to the plain name
    everywhere, and the mark by which ``_gemm_tiled`` knows that ``_fused.gemm_persistent`` may replace the launch."""


def gemm_persistent(a, packed, bias=None, out=None, workgroups=None):
    """``gemm`` on the 128 x 256 tile as ONE launch of ``workgroups`` workgroups that each walk a fixed list of tiles
    (``vqa_gemm_bf16x6_persistent``): a tile's last k-step stages the next tile's first, so only a workgroup's first tile
    waits for its operands.  The bits of ``gemm(tile="wide")``.  N % 256 == 0.  ``workgroups``: None = one per compute
    unit of ``a``'s device; at least 1, a value above the tile count ``ceil(M / 128) * (N / 256)`` is clamped to it.
    ``out``: (M, N) with unit column stride and any row stride >= N."""
    dev_f32(a, "a", contiguous=False)
    if a.dim() != 2 or a.shape[1] != packed.K or a.stride(1) != 1 or a.stride(0) % 4:
        raise ValueError("a must be (M, {}) with unit column stride and a row stride % 4 == 0, got shape {} strides {}"
                         .format(packed.K, tuple(a.shape), a.stride()))
    M, N = a.shape[0], packed.N
    if N % 256:
        raise ValueError("the persistent launch runs 128 x 256 tiles: N % 256 == 0, got N = {}".format(N))
    if workgroups is not None and (isinstance(workgroups, bool) or not isinstance(workgroups, int) or workgroups < 1):
        raise ValueError("workgroups must be None or an integer >= 1, got {!r}".format(workgroups))
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    dev_f32(out, "out", contiguous=False)
    if tuple(out.shape) != (M, N) or out.stride(1) != 1 or (M > 1 and out.stride(0) < N):
        raise ValueError("out must be ({}, {}) with unit column stride, got {} strides {}".format(
            M, N, tuple(out.shape), out.stride()))
    if bias is not None:
        dev_f32(bias, "bias"), _rows_ok("bias", bias, N)
    same_device(a, packed.data, bias, out)
    if M:
        if workgroups is None:
            from .whitebox import _fused
            workgroups = _fused.device_cus(a.device)          # one query per device, shared with the tail plan
        with _on(a):
            check(lib().vqa_gemm_bf16x6_persistent(_p(a), a.stride(0), _p(packed.data), ptr(bias), _p(out),
                                                   max(out.stride(0), N), M, N, packed.K, min(workgroups, 0x7fffffff),
                                                   stream_for(a)), "vqa_gemm_bf16x6_persistent")
    return out


def gemm_half(a, packed, bias=None, out=None):
    """``gemm`` with the whole product on the 128 x 128 tile (``vqa_gemm_bf16x6_half``): the same bits."""
    return _gemm_rows(a, packed, bias, out, None, 0)


def _gemm_tiled(a, packed, bias, out, tile):
    """``tile`` from row 0 to the cut ``whitebox/_fused.py`` names for the shape -- M, the whole product on
    ``vqa_gemm_bf16x6_tile``, unless the shape is listed there or VQA_GEMM_TAIL=1 -- and the 128 x 128 tile behind it.
    An uncut product whose tile is the policy's (``_PolicyTile``) runs as ``gemm_persistent`` where
    ``_fused.gemm_persistent`` says so."""
    M = a.shape[0]
    if isinstance(tile, _PolicyTile) and packed.N % 256 == 0 and M:
        from .whitebox import _fused
        # a product that the tail plan cuts stays cut: the persistent launch takes whole products only
        if _fused.gemm_persistent(M, packed.N, packed.K) and _fused.gemm_tail_split(M, packed.N, packed.K, tile, a.device) >= M:
            return gemm_persistent(a, packed, bias, out)
    return _gemm_rows(a, packed, bias, out, tile, None)


TAIL_CALLS = [0]     # calls of vqa_gemm_bf16x6_tail with a cut inside the matrix (tests and tools read it)


def _gemm_rows(a, packed, bias, out, tile, m_split):
    """Rows ``[0, m_split)`` on ``tile``, the rest on the 128 x 128 tile; ``m_split=None``: the cut of
    ``_fused.gemm_tail_split``; ``tile=None``: every row on the 128 x 128 tile."""
    dev_f32(a, "a", contiguous=False)
    if a.dim() != 2 or a.shape[1] != packed.K or a.stride(1) != 1 or a.stride(0) % 4:
        raise ValueError("a must be (M, {}) with unit column stride and a row stride % 4 == 0, got shape {} strides {}"
                         .format(packed.K, tuple(a.shape), a.stride()))
    M = a.shape[0]
    if out is None:
        out = torch.empty(M, packed.N, dtype=torch.float32, device=a.device)
    dev_f32(out, "out")
    if tuple(out.shape) != (M, packed.N):
        raise ValueError("out must be ({}, {}), got {}".format(M, packed.N, tuple(out.shape)))
    if bias is not None:
        dev_f32(bias, "bias"), _rows_ok("bias", bias, packed.N)
    same_device(a, packed.data, bias, out)
    if M:
        planned = tile is not None and m_split is None          # an m_split of the caller's goes to the tail entry as it is
        if planned:
            from .whitebox import _fused
            m_split = _fused.gemm_tail_split(M, packed.N, packed.K, tile, a.device)
        with _on(a):
            if tile is None:
                check(lib().vqa_gemm_bf16x6_half(_p(a), a.stride(0), _p(packed.data), ptr(bias), _p(out), packed.N, M,
                                                 packed.N, packed.K, stream_for(a)), "vqa_gemm_bf16x6_half")
            elif planned and m_split >= M:
                check(lib().vqa_gemm_bf16x6_tile(_p(a), a.stride(0), _p(packed.data), ptr(bias), _p(out), packed.N, M,
                                                 packed.N, packed.K, GEMM_TILES[tile], stream_for(a)), "vqa_gemm_bf16x6_tile")
            else:
                TAIL_CALLS[0] += 1
                check(lib().vqa_gemm_bf16x6_tail(_p(a), a.stride(0), _p(packed.data), ptr(bias), _p(out), packed.N, M,
                                                 packed.N, packed.K, GEMM_TILES[tile], m_split, stream_for(a)),
                      "vqa_gemm_bf16x6_tail")
    return out


def _gemm_epilogue(a, packed, bias, out, tile, epilogue, aux):
    """``vqa_gemm_bf16x6_epi``; ``gemm`` has checked the epilogue's name and the shape of ``aux``."""
    dev_f32(a, "a", contiguous=False)
    if a.dim() != 2 or a.shape[1] != packed.K or a.stride(1) != 1 or a.stride(0) % 4:
        raise ValueError("a must be (M, {}) with unit column stride and a row stride % 4 == 0, got shape {} strides {}"
                         .format(packed.K, tuple(a.shape), a.stride()))
    M, N = a.shape[0], packed.N
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=a.device)
    dev_f32(out, "out", contiguous=False)
    if tuple(out.shape) != (M, N) or out.stride(1) != 1 or (M > 1 and out.stride(0) < N):
        raise ValueError("out must be ({}, {}) with unit column stride, got {} strides {}".format(
            M, N, tuple(out.shape), out.stride()))
    if bias is not None:
        dev_f32(bias, "bias"), _rows_ok("bias", bias, N)
    if aux is not None:
        dev_f32(aux, "aux", contiguous=False)
        if aux.data_ptr() in (out.data_ptr(), a.data_ptr()):
            raise ValueError("aux must not alias out or a")
    same_device(a, packed.data, bias, out, aux)
    if M:
        with _on(a):
            check(lib().vqa_gemm_bf16x6_epi(_p(a), a.stride(0), _p(packed.data), ptr(bias), _p(out), max(out.stride(0), N), M,
                                            N, packed.K, GEMM_TILES[tile], GEMM_EPILOGUES[epilogue], ptr(aux),
                                            max(aux.stride(0), N) if aux is not None else 0, stream_for(a)),
                  "vqa_gemm_bf16x6_epi")
    return out


GEMM_MAX_GROUPS = 4      # VQA_GEMM_MAX_GROUPS of include/vqattack_hip.h


def gemm_grouped_blocks(Ms, N):
    """Tile list of one ``vqa_gemm_bf16x6_grouped`` launch over groups of ``Ms`` rows at N columns (N % 256 == 0):
    ``(starts, grid)`` with ``starts[i]`` the 128-row blocks ahead of group i (``len(Ms) + 1`` entries, the last one the
    total) and ``grid = starts[-1] * (N // 256)`` workgroups.  Pure arithmetic, no device."""
    N = int(N)
    if N <= 0 or N % 256:
        raise ValueError("the grouped launch runs 128 x 256 tiles: N % 256 == 0, got {}".format(N))
    starts = [0]
    for m in Ms:
        m = int(m)
        if m < 0:
            raise ValueError("row counts must be >= 0, got {}".format(tuple(Ms)))
        starts.append(starts[-1] + -(-m // 128))
    return tuple(starts), starts[-1] * (N // 256)


def gemm_grouped(a_list, packed_list, bias_list=None, out_list=None, epilogue=None, aux_list=None):
    """``[gemm(a, packed, bias, tile="wide", epilogue=..., aux=...) for each group]`` as ONE launch
    (``vqa_gemm_bf16x6_grouped``): up to four products with one (K, N) and a weight each -- the expert FFNs of a multiway
    block -- whose 128 x 256 tiles share a grid, so a group too small to fill the device rides in the last round of a
    large one.  Every output has the bits of the per-group call.  Returns the outputs in the caller's order.

    ``a_list`` / ``packed_list``: per group, as ``gemm``'s ``a`` / ``packed``; all ``PackedWeight``s share (K, N), else
    ValueError.  ``bias_list`` / ``out_list`` / ``aux_list``: None, or one entry (a tensor or None) per group.  One
    ``epilogue`` (None, "gelu", "gelu_grad") serves every group; ``aux`` as in ``gemm``.  ``out`` entries: unit column
    stride and any row stride >= N.  Outputs of different groups must not overlap (not detected).  N % 256 != 0 or more
    than four groups: one ``gemm(..., tile="wide")`` per group -- the same bits (the C entry point refuses both)."""
    n = len(a_list)
    if n == 0 or len(packed_list) != n:
        raise ValueError("need one packed weight per group and at least one group")
    bias_list = [None] * n if bias_list is None else list(bias_list)
    out_list = [None] * n if out_list is None else list(out_list)
    aux_list = [None] * n if aux_list is None else list(aux_list)
    if not len(bias_list) == len(out_list) == len(aux_list) == n:
        raise ValueError("bias_list, out_list and aux_list take one entry per group")
    if epilogue is not None and epilogue not in GEMM_EPILOGUES:
        raise ValueError("epilogue must be None or one of {}, got {!r}".format(sorted(GEMM_EPILOGUES), epilogue))
    K, N = packed_list[0].K, packed_list[0].N
    if any((p.K, p.N) != (K, N) for p in packed_list):
        raise ValueError("the groups of one launch share (K, N), got {}".format([(p.K, p.N) for p in packed_list]))
    if epilogue is None and any(x is not None for x in aux_list):
        raise ValueError("aux goes with an epilogue")
    if epilogue == "gelu_grad" and any(x is None for x in aux_list):
        raise ValueError("epilogue 'gelu_grad' needs aux = the pre-activation h of every group")
    if N % 256 or n > GEMM_MAX_GROUPS:
        # (a group without rows keeps its aux out of gemm's alias check: empty tensors share the null address)
        return [gemm(a, p, b, out=o, tile="wide", epilogue=epilogue, aux=x) if a.shape[0] or x is None else
                (o if o is not None else torch.empty(0, N, dtype=torch.float32, device=a.device))
                for a, p, b, o, x in zip(a_list, packed_list, bias_list, out_list, aux_list)]
    outs = []
    for i, (a, p, b, o, x) in enumerate(zip(a_list, packed_list, bias_list, out_list, aux_list)):
        dev_f32(a, "a", contiguous=False)
        if a.dim() != 2 or a.shape[1] != K or a.stride(1) != 1 or a.stride(0) % 4:
            raise ValueError("a of group {} must be (M, {}) with unit column stride and a row stride % 4 == 0, got shape {} "
                             "strides {}".format(i, K, tuple(a.shape), a.stride()))
        M = a.shape[0]
        if o is None:
            o = torch.empty(M, N, dtype=torch.float32, device=a.device)
        dev_f32(o, "out", contiguous=False)
        if tuple(o.shape) != (M, N) or o.stride(1) != 1 or (M > 1 and o.stride(0) < N):
            raise ValueError("out of group {} must be ({}, {}) with unit column stride, got {} strides {}".format(
                i, M, N, tuple(o.shape), o.stride()))
        if b is not None:
            dev_f32(b, "bias"), _rows_ok("bias", b, N)
        if x is not None:
            if x is o:
                raise ValueError("aux must not be out")
            if not isinstance(x, torch.Tensor) or tuple(x.shape) != (M, N) or x.stride(1) != 1 or \
                    (M > 1 and x.stride(0) < N):
                raise ValueError("aux of group {} must be a ({}, {}) tensor with unit column stride, got {}".format(
                    i, M, N, (tuple(x.shape), x.stride()) if isinstance(x, torch.Tensor) else type(x)))
            dev_f32(x, "aux", contiguous=False)
            if M and x.data_ptr() in (o.data_ptr(), a.data_ptr()):
                raise ValueError("aux must not alias out or a")
        same_device(a_list[0], a, p.data, b, o, x)
        outs.append(o)
    if any(a.shape[0] for a in a_list):
        ptrs, longs = ctypes.c_void_p * n, ctypes.c_long * n
        live = [a.shape[0] > 0 for a in a_list]                   # a group without rows: its entries are not looked at

        def table(ts):
            return ptrs(*[(t.data_ptr() if t is not None and ok else None) for t, ok in zip(ts, live)])
        with _on(a_list[0]):
            check(lib().vqa_gemm_bf16x6_grouped(
                table(a_list), longs(*[a.stride(0) for a in a_list]), table([p.data for p in packed_list]),
                table(bias_list), table(outs), longs(*[max(o.stride(0), N) for o in outs]), table(aux_list),
                longs(*[max(x.stride(0), N) if x is not None else 0 for x in aux_list]),
                longs(*[a.shape[0] for a in a_list]), n, N, K, GEMM_EPILOGUES[epilogue] if epilogue else 0,
                stream_for(a_list[0])), "vqa_gemm_bf16x6_grouped")
    return outs


# Planner constants of the small-tile kernel (measured: profiles/r08/): one 64 x 128 tile per workgroup, two workgroups
# resident per CU.  The split over K raises the grid towards SMALL_TARGET_WORKGROUPS while every part keeps at least
# SMALL_MIN_KSTEPS k-steps (32 columns of A each) to amortise its prologue and its partial-tile traffic.
SMALL_TARGET_WORKGROUPS = 512
SMALL_MIN_KSTEPS = 4
SMALL_MAX_KSPLIT = 8


def gemm_small_workgroups(M, N):
    """64 x 128 output tiles of one ``vqa_gemm_bf16x6_small`` launch (times ksplit = its grid)."""
    return -(-M // 64) * (N // 128)


def gemm_small_plan(M, N, K):
    """The K split ``gemm_small`` should run (M, N, K) with: the largest one, up to SMALL_MAX_KSPLIT, that keeps the grid at
    or below SMALL_TARGET_WORKGROUPS and every part at SMALL_MIN_KSTEPS k-steps or more; 1 where the tile grid alone
    covers the device.  Pure arithmetic, no device."""
    tiles = max(1, gemm_small_workgroups(M, N))
    nk = max(1, K // 32)
    return int(max(1, min(SMALL_MAX_KSPLIT, nk // SMALL_MIN_KSTEPS, nk, SMALL_TARGET_WORKGROUPS // tiles)))


def gemm_small(a, packed, bias=None, out=None, ksplit=1):
    """``gemm`` on 64 x 128 tiles with a deterministic ``ksplit``-way split over K (``vqa_gemm_bf16x6_small``): for row
    counts whose 256 x 128 tiles cannot fill the device.  ``ksplit == 1`` gives the bits of ``gemm``; ``ksplit > 1`` the
    ordered sum of the parts' products (``include/vqattack_hip.h``), through a workspace allocated here."""
    dev_f32(a, "a", contiguous=False)
    if a.dim() != 2 or a.shape[1] != packed.K or a.stride(1) != 1 or a.stride(0) % 4:
        raise ValueError("a must be (M, {}) with unit column stride and a row stride % 4 == 0, got shape {} strides {}"
                         .format(packed.K, tuple(a.shape), a.stride()))
    ksplit = int(ksplit)
    if not 1 <= ksplit <= min(packed.K // 32, 16):
        raise ValueError("ksplit must be in [1, {}] for K={}, got {}".format(min(packed.K // 32, 16), packed.K, ksplit))
    M = a.shape[0]
    if out is None:
        out = torch.empty(M, packed.N, dtype=torch.float32, device=a.device)
    dev_f32(out, "out")
    if tuple(out.shape) != (M, packed.N):
        raise ValueError("out must be ({}, {}), got {}".format(M, packed.N, tuple(out.shape)))
    if bias is not None:
        dev_f32(bias, "bias"), _rows_ok("bias", bias, packed.N)
    same_device(a, packed.data, bias, out)
    if M:
        ws = None
        if ksplit > 1:
            ws = torch.empty(lib().vqa_gemm_small_ws_bytes(M, packed.N, ksplit), dtype=torch.uint8, device=a.device)
        with _on(a):
            check(lib().vqa_gemm_bf16x6_small(_p(a), a.stride(0), _p(packed.data), ptr(bias), _p(out), packed.N, M,
                                              packed.N, packed.K, ksplit, ptr(ws), stream_for(a)),
                  "vqa_gemm_bf16x6_small")
    return out


def gemm_lse(a, packed, bias, targets, ignore_index=-100, tile=None, want_lse=False, flag=None, want_target_logit=False):
    """Per-row cross entropy of ``logits = a @ B (+ bias)`` against ``targets`` without the logits
    (``vqa_gemm_bf16x6_lse``): ``row_loss`` (M,) = logsumexp over the first ``packed.n_valid`` columns minus the target's
    logit; exactly 0 where ``targets == ignore_index``; NaN (and VQA_FLAG_BAD_LABEL in ``flag``, an int32[1] word) for a
    target that is neither.  ``packed``: from ``gemm_pack_vocab``; columns >= ``n_valid`` are masked whatever they hold.
    ``bias``: None, (n_valid,) or (N,).  ``targets``: int64 (M,).  Returns ``row_loss``, or ``(row_loss, lse)`` with
    ``want_lse``; ``want_target_logit`` appends the target logits (M,) -- a view of the workspace, defined only where the
    target is in range: the bits ``gemm`` puts at ``[row, target]``.  Both tiles give the same bits."""
    dev_f32(a, "a", contiguous=False)
    if a.dim() != 2 or a.shape[1] != packed.K or a.stride(1) != 1 or a.stride(0) % 4:
        raise ValueError("a must be (M, {}) with unit column stride and a row stride % 4 == 0, got shape {} strides {}"
                         .format(packed.K, tuple(a.shape), a.stride()))
    M, N = a.shape[0], packed.N
    if not isinstance(targets, torch.Tensor) or not targets.is_cuda or targets.dtype != torch.int64 or \
            tuple(targets.shape) != (M,) or not targets.is_contiguous():
        raise TypeError("targets must be a contiguous int64 HIP tensor of shape ({},)".format(M))
    if bias is not None:
        dev_f32(bias, "bias")
        if bias.numel() == packed.n_valid and packed.n_valid != N:
            bias = torch.cat([bias.reshape(-1), bias.new_zeros(N - packed.n_valid)])
        _rows_ok("bias", bias, N)
    if flag is not None and (not isinstance(flag, torch.Tensor) or not flag.is_cuda or flag.dtype != torch.int32 or
                             flag.numel() != 1):
        raise TypeError("flag must be an int32[1] HIP tensor (ops.new_flag)")
    if tile is None:
        from .whitebox import _fused
        tile = _fused.gemm_tile(M, N, packed.K)
    if tile not in GEMM_TILES:
        raise ValueError("tile must be one of {}, got {!r}".format(sorted(GEMM_TILES), tile))
    same_device(a, packed.data, bias, targets, flag)
    row_loss = torch.empty(M, dtype=torch.float32, device=a.device)
    lse = torch.empty(M, dtype=torch.float32, device=a.device) if want_lse else None
    ws = torch.empty(max(1, lib().vqa_gemm_lse_ws_floats(M, N)), dtype=torch.float32, device=a.device)
    if M:
        with _on(a):
            check(lib().vqa_gemm_bf16x6_lse(_p(a), a.stride(0), _p(packed.data), ptr(bias), M, N, packed.K, packed.n_valid,
                                            _p(targets), int(ignore_index), _p(ws), _p(row_loss), ptr(lse), ptr(flag),
                                            GEMM_TILES[tile], stream_for(a)), "vqa_gemm_bf16x6_lse")
    res = (row_loss,) + ((lse,) if want_lse else ()) + ((ws[(N // 64) * 2 * M:][:M],) if want_target_logit else ())
    return res[0] if len(res) == 1 else res
