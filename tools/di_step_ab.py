"""A/B of the DI (input diversity) step on one device, variants alternating in one process.

    python tools/di_step_ab.py [--batch 64 256] [--size 384] [--shrink 32] [--rounds 7] [--reps 10]

  (a) eager torch, a host loop over the samples (every sample has its own output size): F.interpolate + F.pad, their
      autograd backward of the given gD, then ops.linf_step on the gathered gradient
  (b) ops.di_adjoint + ops.linf_step: two launches, the image gradient goes through memory (24 B/element)
  (c) ops.linf_di_step: one launch (at most 16 B/element)
  (d) ops.linf_step alone: the floor, no transform
  (t) ops.di_transform, against (copy) a plain device copy of the same tensor (8 B/element both)
The rows are one ops.di_draw of the reference's distribution (new_h in [size - shrink, size), probability 1).  One sample
= `reps` back-to-back launches between two device events (2 for the eager variant); per variant the median, minimum and
maximum over `rounds` samples after one warm-up round, in microseconds per step.  A difference counts when it exceeds the
larger of the two variants' max - min spreads.  One JSON line per (batch, variant).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqattack_amd import ops  # noqa: E402

EPS_ITER, EPS, LO, HI = 0.01, 0.125, -1.0, 1.0


def sample(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def eager_adjoint(x, gd, rows):
    """What autograd gives through interpolate + pad, sample by sample."""
    h, w = x.shape[2:]
    grads = []
    for s, (nh, nw, top, left) in enumerate(rows):
        leaf = x[s:s + 1].detach().requires_grad_(True)
        d = F.pad(F.interpolate(leaf, size=(nh, nw), mode="bilinear", align_corners=False, antialias=False),
                  (left, w - nw - left, top, h - nh - top))
        d.backward(gd[s:s + 1])
        grads.append(leaf.grad)
    return torch.cat(grads)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--shrink", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/di_step_ab.py measures on the GPU; there is none")
    for batch in args.batch:
        shape = (batch, 3, args.size, args.size)
        gen = torch.Generator(device="cuda").manual_seed(batch)
        x0 = torch.empty(shape, device="cuda").uniform_(-1, 1, generator=gen)
        x = (x0 + torch.empty(shape, device="cuda").uniform_(-EPS, EPS, generator=gen)).clamp_(LO, HI)
        gd = torch.randn(shape, device="cuda", generator=gen)
        out, g = torch.empty_like(x), torch.empty_like(x)
        table = ops.di_draw(np.random.RandomState(batch), batch, 1, args.size, args.size, shrink=args.shrink)[0]
        rows = [tuple(int(v) for v in r) for r in table]
        geom = ops.di_geometry(table, args.size, args.size, "cuda")
        window = float(np.mean(table[:, 0].astype(np.float64) * table[:, 1])) / (args.size * args.size)
        variants = []
        if not args.no_eager:
            variants.append(("a: eager per-sample interpolate + pad + backward + linf_step",
                             lambda: ops.linf_step(x, eager_adjoint(x, gd, rows), x0, EPS_ITER, EPS, LO, HI, out=out)))
        variants.append(("b: di_adjoint + linf_step",
                         lambda: ops.linf_step(x, ops.di_adjoint(gd, geom, out=g), x0, EPS_ITER, EPS, LO, HI, out=out)))
        variants.append(("c: linf_di_step", lambda: ops.linf_di_step(x, gd, x0, geom, EPS_ITER, EPS, LO, HI, out=out)))
        variants.append(("d: linf_step alone", lambda: ops.linf_step(x, gd, x0, EPS_ITER, EPS, LO, HI, out=out)))
        variants.append(("t: di_transform", lambda: ops.di_transform(x, geom, out=out)))
        variants.append(("copy: out.copy_(x)", lambda: out.copy_(x)))
        times = {name: [] for name, _ in variants}
        for rnd in range(args.rounds + 1):                     # round 0 warms every variant up and is dropped
            for name, fn in variants:
                t = sample(fn, 2 if name.startswith("a") else args.reps)
                if rnd:
                    times[name].append(t)
        n = x.numel()
        for name, _ in variants:
            ts = times[name]
            med = statistics.median(ts)
            rec = dict(batch=batch, size=args.size, shrink=args.shrink, mean_window_fraction=round(window, 4), variant=name,
                       median_us=round(med, 2), min_us=round(min(ts), 2), max_us=round(max(ts), 2))
            per_el = {"c": 12 + 4 * window, "t": 8, "copy": 8}.get(name.split(":")[0])
            if per_el is not None:
                rec["bytes_per_element"] = round(per_el, 2)
                rec["algorithmic_GBs"] = round(per_el * n / med / 1e3, 1)
                rec["of_8TBs"] = round(per_el * n / med / 8e6, 3)
            print(json.dumps(rec), flush=True)
        del x0, x, gd, out, g


if __name__ == "__main__":
    main()
