"""A/B of the SI (scale copies) step on one device, variants alternating in one process.

    python tools/si_step_ab.py [--batch 64 256] [--size 384] [--copies 5] [--rounds 7] [--reps 10]

  (a) eager torch: ghat = g_0 * w_0, then ghat.add_(g_i, alpha=w_i) per further copy, then ops.linf_step
  (b) ops.si_combine + ops.linf_step: two launches, the combined gradient goes through memory (4 * copies + 4 + 16 B/element)
  (c) ops.linf_si_step: one launch (4 * copies + 12 B/element)
  (d) ops.linf_step alone: the floor, one gradient
  (t) ops.si_copies without the momentum, (tm) with it, against (mul) `copies` eager multiplies into the same buffer
One sample = `reps` back-to-back launches between two device events; per variant the median, minimum and maximum over
`rounds` samples after one warm-up round, in microseconds per step.  A difference counts when it exceeds the larger of
the two variants' max - min spreads.  One JSON line per (batch, variant).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqattack_amd import ops  # noqa: E402

EPS_ITER, EPS, LO, HI = 0.01, 0.125, -1.0, 1.0
LOOKAHEAD = 0.01


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/si_step_ab.py measures on the GPU; there is none")
    n_c = args.copies
    scales = ops.si_scales(n_c)
    weights = ops.si_weights(scales)
    for batch in args.batch:
        shape = (batch, 3, args.size, args.size)
        gen = torch.Generator(device="cuda").manual_seed(batch)
        x0 = torch.empty(shape, device="cuda").uniform_(-1, 1, generator=gen)
        x = (x0 + torch.empty(shape, device="cuda").uniform_(-EPS, EPS, generator=gen)).clamp_(LO, HI)
        m = torch.randn(shape, device="cuda", generator=gen)
        grads = [torch.randn(shape, device="cuda", generator=gen) for _ in range(n_c)]   # separate tensors, as autograd's
        out, ghat = torch.empty_like(x), torch.empty_like(x)
        images = torch.empty((n_c,) + shape, device="cuda")

        def eager():
            torch.mul(grads[0], float(weights[0]), out=ghat)
            for i in range(1, n_c):
                ghat.add_(grads[i], alpha=float(weights[i]))
            return ops.linf_step(x, ghat, x0, EPS_ITER, EPS, LO, HI, out=out)

        def eager_copies():
            for i in range(n_c):
                torch.mul(x, float(scales[i]), out=images[i])

        variants = [
            ("a: eager mul + add_(alpha) + linf_step", eager),
            ("b: si_combine + linf_step",
             lambda: ops.linf_step(x, ops.si_combine(grads, weights, out=ghat), x0, EPS_ITER, EPS, LO, HI, out=out)),
            ("c: linf_si_step", lambda: ops.linf_si_step(x, grads, x0, weights, EPS_ITER, EPS, LO, HI, out=out)),
            ("d: linf_step alone", lambda: ops.linf_step(x, grads[0], x0, EPS_ITER, EPS, LO, HI, out=out)),
            ("t: si_copies", lambda: ops.si_copies(x, scales, out=images)),
            ("tm: si_copies with momentum", lambda: ops.si_copies(x, scales, m=m, lookahead=LOOKAHEAD, out=images)),
            ("mul: eager multiplies", eager_copies),
        ]
        times = {name: [] for name, _ in variants}
        for rnd in range(args.rounds + 1):                     # round 0 warms every variant up and is dropped
            for name, fn in variants:
                t = sample(fn, args.reps)
                if rnd:
                    times[name].append(t)
        n = x.numel()
        per_el = {"a": None, "b": 4 * n_c + 4 + 16, "c": 4 * n_c + 12, "d": 16, "t": 4 + 4 * n_c, "tm": 8 + 4 * n_c,
                  "mul": 8 * n_c}
        for name, _ in variants:
            ts = times[name]
            med = statistics.median(ts)
            rec = dict(batch=batch, size=args.size, copies=n_c, variant=name, median_us=round(med, 2),
                       min_us=round(min(ts), 2), max_us=round(max(ts), 2))
            b = per_el[name.split(":")[0]]
            if b is not None:
                rec["bytes_per_element"] = b
                rec["algorithmic_GBs"] = round(b * n / med / 1e3, 1)
                rec["of_8TBs"] = round(b * n / med / 8e6, 3)
            print(json.dumps(rec), flush=True)
        del x0, x, m, grads, out, ghat, images


if __name__ == "__main__":
    main()
