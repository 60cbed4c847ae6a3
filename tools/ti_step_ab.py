"""A/B of the TI (translation-invariant) smoothing step on one device, variants alternating in one process.

    VQA_TUNING_LIB=1 python tools/ti_step_ab.py [--batch 64 256] [--taps 15 7] [--rounds 7] [--reps 10]

  (a) eager torch: F.conv2d(g, k2d, padding=r, groups=3), then ops.linf_step
  (b) ops.ti_smooth + ops.linf_step: two launches, the smoothed gradient goes through memory (24 B/element)
  (c) ops.linf_ti_step: one launch (16 B/element)
  (d) ops.linf_step alone: the floor, no smoothing
With the tuning build (b) and (c) run at both output tile heights (option 14: 32 and 64 rows of 64); the shipped library
has the one it was compiled with.  One sample = `reps` back-to-back launches between two device events; per variant the
median, minimum and maximum over `rounds` samples, in microseconds per step.  A difference counts when it exceeds the
larger of the two variants' max - min spreads.  One JSON line per (batch, taps, variant).
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqattack_amd import _hip, ops  # noqa: E402

EPS_ITER, EPS, LO, HI = 0.01, 0.125, -1.0, 1.0


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
    ap.add_argument("--taps", type=int, nargs="+", default=[15, 7])
    ap.add_argument("--size", type=int, default=384)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-eager", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/ti_step_ab.py measures on the GPU; there is none")
    tiles = [32, 64] if _hip.set_option(14, 32) else [None]
    for batch in args.batch:
        shape = (batch, 3, args.size, args.size)
        gen = torch.Generator(device="cuda").manual_seed(batch)
        x0 = torch.empty(shape, device="cuda").uniform_(-1, 1, generator=gen)
        x = (x0 + torch.empty(shape, device="cuda").uniform_(-EPS, EPS, generator=gen)).clamp_(LO, HI)
        g = torch.randn(shape, device="cuda", generator=gen)
        out, ghat = torch.empty_like(x), torch.empty_like(x)
        for k in args.taps:
            w = ops.ti_gaussian_taps(k)
            k2d = torch.from_numpy(w).to("cuda")
            k2d = torch.outer(k2d, k2d).expand(3, 1, k, k).contiguous()
            variants = []
            if not args.no_eager:
                variants.append(("a: eager conv2d + linf_step", None,
                                 lambda: ops.linf_step(x, F.conv2d(g, k2d, padding=k // 2, groups=3), x0, EPS_ITER, EPS,
                                                       LO, HI, out=out)))
            for th in tiles:
                tag = "" if th is None else ", tile 64 x {}".format(th)
                variants.append(("b: ti_smooth + linf_step" + tag, th,
                                 lambda: ops.linf_step(x, ops.ti_smooth(g, w, out=ghat), x0, EPS_ITER, EPS, LO, HI,
                                                       out=out)))
                variants.append(("c: linf_ti_step" + tag, th,
                                 lambda: ops.linf_ti_step(x, g, x0, w, EPS_ITER, EPS, LO, HI, out=out)))
            variants.append(("d: linf_step alone", None, lambda: ops.linf_step(x, g, x0, EPS_ITER, EPS, LO, HI, out=out)))
            times = {name: [] for name, _, _ in variants}
            for rnd in range(args.rounds + 1):                     # round 0 warms every variant up and is dropped
                for name, th, fn in variants:
                    if th is not None:
                        _hip.set_option(14, th)
                    reps = 2 if name.startswith("a") else args.reps
                    t = sample(fn, reps)
                    if rnd:
                        times[name].append(t)
            n = x.numel()
            for name, _, _ in variants:
                ts = times[name]
                med = statistics.median(ts)
                rec = dict(batch=batch, taps=k, variant=name, median_us=round(med, 2), min_us=round(min(ts), 2),
                           max_us=round(max(ts), 2))
                if name.startswith("c"):
                    rec["algorithmic_GBs_at_16B"] = round(16 * n / med / 1e3, 1)
                    rec["of_8TBs"] = round(16 * n / med / 8e6, 3)
                print(json.dumps(rec), flush=True)
        del x0, x, g, out, ghat


if __name__ == "__main__":
    main()
