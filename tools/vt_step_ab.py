"""A/B of the variance-tuning (VMI / VNI-FGSM) step on one device, variants alternating in one process.

    python tools/vt_step_ab.py [--batch 64 256] [--size 384] [--neighbors 20] [--rounds 7] [--reps 10]

The work of one gradient evaluation outside the model calls, with N neighbours in chunks of 8 (20: 8 + 8 + 4):
  (a) eager torch: per neighbour `uniform_` into a scratch and `add` into its image; `add_` per gradient after the first
      (which is copied), `div`, `sub`, `add`, then ops.linf_step
  (b) ops.vt_neighbors per chunk + ops.vt_accumulate per chunk + ops.vt_tune + ops.linf_step
  (c) the same with ops.linf_vt_step in place of the last two launches (28 against 20 + 16 B/element)
and each kernel alone, for its share of 8 TB/s: (n8) / (n8m) vt_neighbors of 8 without / with the momentum, (n1) of 1,
(s8) vt_accumulate of 8 gradients starting the sum, (s8+) adding to it, (tune) vt_tune, (step) linf_vt_step, (d) linf_step.
One sample = `reps` back-to-back runs between two device events; per variant the median, minimum and maximum over
`rounds` samples after one warm-up round, in microseconds per run.  A difference counts when it exceeds the larger of the
two variants' max - min spreads.  One JSON line per (batch, variant).
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
LOOKAHEAD, BETA, SEED = 0.01, 1.5, 20211


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
    ap.add_argument("--neighbors", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/vt_step_ab.py measures on the GPU; there is none")
    n_nb, chunk = args.neighbors, ops.VT_MAX_CHUNK
    chunks = [(s, min(chunk, n_nb - s)) for s in range(0, n_nb, chunk)]
    w = float(np.float32(1.0) / np.float32(n_nb))
    bound = float(np.float32(BETA * EPS))
    for batch in args.batch:
        shape = (batch, 3, args.size, args.size)
        gen = torch.Generator(device="cuda").manual_seed(batch)
        x0 = torch.empty(shape, device="cuda").uniform_(-1, 1, generator=gen)
        x = (x0 + torch.empty(shape, device="cuda").uniform_(-EPS, EPS, generator=gen)).clamp_(LO, HI)
        m = torch.randn(shape, device="cuda", generator=gen)
        g = torch.randn(shape, device="cuda", generator=gen)
        grads = [torch.randn(shape, device="cuda", generator=gen) for _ in range(chunk)]   # one chunk's, as autograd's
        v = torch.randn(shape, device="cuda", generator=gen)
        out, ghat, vsum, noise = (torch.empty_like(x) for _ in range(4))
        images = torch.empty((chunk,) + shape, device="cuda")
        key = ops.vt_key_table(SEED, 1, "cuda")[0]

        def eager():
            for _, count in chunks:                             # the neighbours, a chunk buffer at a time
                for c in range(count):
                    noise.uniform_(-bound, bound)
                    torch.add(x, noise, out=images[c])
            first = True
            for _, count in chunks:                             # the sum of their gradients
                for c in range(count):
                    if first:
                        vsum.copy_(grads[c])
                        first = False
                    else:
                        vsum.add_(grads[c])
            torch.add(g, v, out=ghat)                           # the tune step: ghat = g + v, v = vsum / N - g
            torch.div(vsum, float(n_nb), out=v)
            v.sub_(g)
            return ops.linf_step(x, ghat, x0, EPS_ITER, EPS, LO, HI, out=out)

        def kernels(fused):
            for first, count in chunks:
                ops.vt_neighbors(x, key, count, bound, first=first, out=images[:count])
            for first, count in chunks:
                ops.vt_accumulate(grads[:count], vsum, first == 0)
            if fused:
                return ops.linf_vt_step(x, g, vsum, v, x0, w, EPS_ITER, EPS, LO, HI, out=out)
            return ops.linf_step(x, ops.vt_tune(g, vsum, v, w, out=ghat), x0, EPS_ITER, EPS, LO, HI, out=out)

        variants = [
            ("a: eager uniform_ + add, add_, div, sub, add, linf_step", eager),
            ("b: vt_neighbors + vt_accumulate + vt_tune + linf_step", lambda: kernels(False)),
            ("c: vt_neighbors + vt_accumulate + linf_vt_step", lambda: kernels(True)),
            ("bt: vt_tune + linf_step",
             lambda: ops.linf_step(x, ops.vt_tune(g, vsum, v, w, out=ghat), x0, EPS_ITER, EPS, LO, HI, out=out)),
            ("step: linf_vt_step", lambda: ops.linf_vt_step(x, g, vsum, v, x0, w, EPS_ITER, EPS, LO, HI, out=out)),
            ("tune: vt_tune", lambda: ops.vt_tune(g, vsum, v, w, out=ghat)),
            ("d: linf_step alone", lambda: ops.linf_step(x, g, x0, EPS_ITER, EPS, LO, HI, out=out)),
            ("n8: vt_neighbors of 8", lambda: ops.vt_neighbors(x, key, chunk, bound, out=images)),
            ("n8m: vt_neighbors of 8 with momentum",
             lambda: ops.vt_neighbors(x, key, chunk, bound, m=m, lookahead=LOOKAHEAD, out=images)),
            ("n1: vt_neighbors of 1", lambda: ops.vt_neighbors(x, key, 1, bound, out=images[:1])),
            ("s8: vt_accumulate of 8, init", lambda: ops.vt_accumulate(grads, vsum, True)),
            ("s8+: vt_accumulate of 8, adding", lambda: ops.vt_accumulate(grads, vsum, False)),
        ]
        times = {name: [] for name, _ in variants}
        for rnd in range(args.rounds + 1):                     # round 0 warms every variant up and is dropped
            for name, fn in variants:
                t = sample(fn, args.reps)
                if rnd:
                    times[name].append(t)
        n = x.numel()
        per_el = {"a": None, "b": None, "c": None, "bt": 20 + 16, "step": 28, "tune": 20, "d": 16, "n8": 4 + 4 * chunk,
                  "n8m": 8 + 4 * chunk, "n1": 8, "s8": 4 * chunk + 4, "s8+": 4 * chunk + 8}
        for name, _ in variants:
            ts = times[name]
            med = statistics.median(ts)
            rec = dict(batch=batch, size=args.size, neighbors=n_nb, variant=name, median_us=round(med, 2),
                       min_us=round(min(ts), 2), max_us=round(max(ts), 2))
            b = per_el[name.split(":")[0]]
            if b is not None:
                rec["bytes_per_element"] = b
                rec["algorithmic_GBs"] = round(b * n / med / 1e3, 1)
                rec["of_8TBs"] = round(b * n / med / 8e6, 3)
            print(json.dumps(rec), flush=True)
        del x0, x, m, g, grads, v, out, ghat, vsum, noise, images


if __name__ == "__main__":
    main()
