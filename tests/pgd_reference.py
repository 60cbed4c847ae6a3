"""What the PGD stream kernels' GPU tests share: placing host arrays on the device, bitwise comparison, and the numpy fp32
restatement of the chains in include/vqattack_hip.h (one rounding per operation, ascending order).
A plain module: the test files import what they need."""
import numpy as np
import torch

DEV = "cuda:0"
F = np.float32


def place(a, off):
    """Host array -> device tensor; ``off``: one float behind a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if not off:
        return t.to(DEV)
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
    view = buf[1:].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def sign(g):
    return (g > 0).astype(F) - (g < 0).astype(F)      # torch.sign: sign(NaN) = 0


def update_np(x, ghat, x0, eps_iter, eps, lo, hi, clip):
    """numpy fp32: StepOp (x0 given) or FgmOp (x0 None) of csrc/common.hpp."""
    a = x + F(eps_iter) * sign(ghat)
    if clip:
        a = np.clip(a, F(lo), F(hi))
    if x0 is None:
        return a
    out = x0 + np.clip(a - x0, -F(eps), F(eps))
    if clip:
        out = np.clip(out, F(lo), F(hi))
    assert out.dtype == F
    return out


def copies_np(x, s, m=None, lookahead=0.0):
    """si_copies: multiply, add, multiply."""
    base = x if m is None else x + F(lookahead) * m
    out = np.stack([F(si) * base for si in s])
    assert out.dtype == F
    return out


def combine_np(g, w):
    """si_combine: the chain starts from its first product."""
    with np.errstate(all="ignore"):
        acc = F(w[0]) * g[0]
        for i in range(1, len(w)):
            acc = acc + F(w[i]) * g[i]
    assert acc.dtype == F
    return acc


def accumulate_np(acc, g, w):
    """admix_accumulate: the chain starts from ``acc``."""
    with np.errstate(all="ignore"):
        a = acc
        for i in range(len(w)):
            a = a + F(w[i]) * g[i]
    assert a.dtype == F
    return a


def assert_bits(got, want, what):
    got = got.detach().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype, what
    same = np.mean(got.view(np.int32) == want.view(np.int32))
    assert same == 1.0, (what, same)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
