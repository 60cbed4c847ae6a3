"""A/B of the Admix (mixed-image copies) kernels on one device, variants alternating in one process.

    python tools/admix_step_ab.py [--batch 64 256] [--size 384] [--copies 5] [--images 3] [--rounds 7] [--reps 10]

Behind the model, with m1 = copies and m2 = images (the m1 gradient tensors stand for every group's):
  (a) eager torch, the chain Admix replaces: gsum = g * w_0, then gsum.add_(g, alpha=w_i) for the other m1 * m2 - 1
      gradients, then ops.linf_step
  (b) ops.admix_accumulate of the LAST group + ops.linf_step: two launches, the sum goes through memory
      ((4 * m1 + 8) + 16 B/element); the groups before it were folded while the model ran
  (c) ops.linf_admix_step: the same in one launch (4 * m1 + 16 B/element)
  (f) ops.admix_accumulate alone: one earlier group's fold (4 * m1 + 8 B/element)
In front of the model, one mixed group:
  (d) ops.admix_copies without the momentum, (dm) with it (4 (+ 4) + 4 + 4 * m1 B/element)
  (e) eager torch: index_select of the partners, one axpy, m1 multiplies into the same buffer
One sample = `reps` back-to-back launches between two device events; per variant the median, minimum and maximum over
`rounds` samples after one warm-up round, in microseconds.  A difference counts when it exceeds the larger of the two
variants' max - min spreads.  One JSON line per (batch, variant).
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqattack_amd import ops  # noqa: E402

EPS_ITER, EPS, LO, HI = 0.01, 0.125, -1.0, 1.0
LOOKAHEAD, ETA = 0.01, 0.2


def sample(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--copies", type=int, default=5)
    ap.add_argument("--images", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/admix_step_ab.py measures on the GPU; there is none")
    m1, m2 = args.copies, args.images
    scales = ops.si_scales(m1)
    weights = ops.admix_weights(scales, m2)
    for batch in args.batch:
        shape = (batch, 3, args.size, args.size)
        gen = torch.Generator(device="cuda").manual_seed(batch)
        x0 = torch.empty(shape, device="cuda").uniform_(-1, 1, generator=gen)
        x = (x0 + torch.empty(shape, device="cuda").uniform_(-EPS, EPS, generator=gen)).clamp_(LO, HI)
        m = torch.randn(shape, device="cuda", generator=gen)
        grads = [torch.randn(shape, device="cuda", generator=gen) for _ in range(m1)]   # separate tensors, as autograd's
        out, gsum, mixed = torch.empty_like(x), torch.zeros_like(x), torch.empty_like(x)
        images = torch.empty((m1,) + shape, device="cuda")
        table = ops.admix_partners(ops.admix_draw(np.random.RandomState(batch), batch, 1, 1), batch, "cuda")
        row = table[0, 0]
        row64 = row.to(torch.int64)

        def eager():
            torch.mul(grads[0], float(weights[0]), out=gsum)
            for k in range(1, m1 * m2):
                gsum.add_(grads[k % m1], alpha=float(weights[k % m1]))
            return ops.linf_step(x, gsum, x0, EPS_ITER, EPS, LO, HI, out=out)

        def eager_copies():
            torch.index_select(x, 0, row64, out=mixed)
            torch.add(x, mixed, alpha=ETA, out=mixed)
            for i in range(m1):
                torch.mul(mixed, float(scales[i]), out=images[i])

        def two():
            ops.admix_accumulate(grads, weights, gsum)
            return ops.linf_step(x, gsum, x0, EPS_ITER, EPS, LO, HI, out=out)

        variants = [
            ("a: eager mul + {} add_(alpha) + linf_step".format(m1 * m2 - 1), eager),
            ("b: admix_accumulate + linf_step", two),
            ("c: linf_admix_step", lambda: ops.linf_admix_step(x, gsum, grads, x0, weights, EPS_ITER, EPS, LO, HI, out=out)),
            ("f: admix_accumulate alone", lambda: ops.admix_accumulate(grads, weights, gsum)),
            ("d: admix_copies", lambda: ops.admix_copies(x, row, scales, ETA, out=images)),
            ("dm: admix_copies with momentum",
             lambda: ops.admix_copies(x, row, scales, ETA, m=m, lookahead=LOOKAHEAD, out=images)),
            ("e: eager index_select + axpy + multiplies", eager_copies),
        ]
        times = {name: [] for name, _ in variants}
        for rnd in range(args.rounds + 1):                     # round 0 warms every variant up and is dropped
            for name, fn in variants:
                t = sample(fn, args.reps)
                if rnd:
                    times[name].append(t)
        n = x.numel()
        per_el = {"a": None, "b": 4 * m1 + 8 + 16, "c": 4 * m1 + 16, "f": 4 * m1 + 8, "d": 8 + 4 * m1, "dm": 12 + 4 * m1,
                  "e": 8 + 12 + 8 * m1}
        for name, _ in variants:
            ts = times[name]
            med = statistics.median(ts)
            rec = dict(batch=batch, size=args.size, copies=m1, images=m2, variant=name, median_us=round(med, 2),
                       min_us=round(min(ts), 2), max_us=round(max(ts), 2))
            b = per_el[name.split(":")[0]]
            if b is not None:
                rec["bytes_per_element"] = b
                rec["algorithmic_GBs"] = round(b * n / med / 1e3, 1)
                rec["of_8TBs"] = round(b * n / med / 8e6, 3)
            print(json.dumps(rec), flush=True)
        del x0, x, m, grads, out, gsum, mixed, images


if __name__ == "__main__":
    main()
