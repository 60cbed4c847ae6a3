"""Per-shape A/B of the encoder GEMMs: the bf16x6 kernel (``csrc/gemm.hip``) against the library fp32 GEMM that
``torch.addmm`` / ``torch.mm`` run (with the recorded TunableOp solutions active, as in bench.py).

Random data (activations ~ N(0, 1), weights ~ N(0, 0.02^2)): bf16 MFMA loops hold a lower clock on random data than on
zeros.  The variants are interleaved in one process over several rounds; per shape the median and min time per call, the
fp32-equivalent TF/s (2 M N K / t), the bf16 MFMA TF/s the kernel sustains (6 products: 12 M N K / t) and the max / RMS
error of each against an fp64 product are reported, plus the speed-up.  One JSON line per shape, a summary at the end.

    python tools/gemm_bench.py [--model vlmo_base|albef_base|vlmo_large] [--rounds 5] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqattack_amd import ops  # noqa: E402
from vqattack_amd.whitebox import tuned_gemms  # noqa: E402

# (dim, ffn, rows per sample, text rows per sample (0 = one modality), batch)
MODELS = {"vlmo_base": (768, 3072, 591, 40, 64), "albef_base": (768, 3072, 577, 0, 256),
          "vlmo_large": (1024, 4096, 591, 40, 128)}


def shapes(model):
    """(name, M, N, K, bias) of every encoder GEMM of one layer, forward and input-gradient backward."""
    d, f, s, t, b = MODELS[model]
    rows = b * s
    out = [("qkv_fwd", rows, 3 * d, d, True), ("qkv_bwd", rows, d, 3 * d, False),
           ("proj_fwd", rows, d, d, True), ("proj_bwd", rows, d, d, False)]
    experts = [("img", b * (s - t)), ("txt", b * t)] if t else [("all", rows)]
    if t:
        experts.append(("vl", rows))
    for tag, m in experts:
        out += [("fc1_fwd_" + tag, m, f, d, True), ("fc1_bwd_" + tag, m, d, f, False),
                ("fc2_fwd_" + tag, m, d, f, True), ("fc2_bwd_" + tag, m, f, d, False)]
    return out


def err(c, ref):
    e = (c.double() - ref).abs()
    return float(e.max()), float(e.pow(2).mean().sqrt())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vlmo_base", choices=sorted(MODELS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--only", default="", help="comma-separated shape names")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    tuned = tuned_gemms.enable()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    results = []
    for name, M, N, K, has_bias in shapes(args.model):
        if args.only and name not in args.only.split(","):
            continue
        a = torch.randn(M, K, device=dev, generator=gen)
        w = torch.randn(N, K, device=dev, generator=gen) * 0.02       # Linear weight [out, in]: forward B = w.t()
        bias = torch.randn(N, device=dev, generator=gen) * 0.02 if has_bias else None
        bt = w.t()
        packed = ops.gemm_pack(w, trans=True)
        out_k = torch.empty(M, N, device=dev)
        out_l = torch.empty(M, N, device=dev)

        def run_kernel():
            ops.gemm(a, packed, bias, out=out_k)

        def run_library():
            if bias is not None:
                torch.addmm(bias, a, bt, out=out_l)
            else:
                torch.mm(a, bt, out=out_l)

        times = {"kernel": [], "library": []}
        for fn in (run_kernel, run_library):        # warm-up
            fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for key, fn in (("kernel", run_kernel), ("library", run_library)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.reps):
                    fn()
                e1.record()
                e1.synchronize()
                times[key].append(e0.elapsed_time(e1) / args.reps)
        ref = a.double() @ bt.double()
        if bias is not None:
            ref += bias.double()
        run_kernel(), run_library()
        torch.cuda.synchronize()
        ek, el = err(out_k, ref), err(out_l, ref)
        del ref
        med_k, med_l = statistics.median(times["kernel"]), statistics.median(times["library"])
        flop = 2.0 * M * N * K
        row = dict(shape=name, M=M, N=N, K=K, bias=has_bias,
                   kernel_ms_median=med_k, kernel_ms_min=min(times["kernel"]),
                   library_ms_median=med_l, library_ms_min=min(times["library"]),
                   speedup_median=med_l / med_k, speedup_min=min(times["library"]) / min(times["kernel"]),
                   kernel_fp32eq_tflops=flop / med_k / 1e9, kernel_bf16_mfma_tflops=6 * flop / med_k / 1e9,
                   library_tflops=flop / med_l / 1e9,
                   kernel_err_max=ek[0], kernel_err_rms=ek[1], library_err_max=el[0], library_err_rms=el[1])
        print(json.dumps(row), flush=True)
        results.append(row)
        del a, w, packed, out_k, out_l
        torch.cuda.empty_cache()
    summary = dict(model=args.model, tuned_gemms=tuned, device=torch.cuda.get_device_name(),
                   rounds=args.rounds, reps=args.reps, shapes=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    print("shape               speedup(med)  kernel TF  bf16 TF  lib TF  err k/lib (max)")
    for r in results:
        print("{:<20}{:>10.3f}{:>11.1f}{:>9.0f}{:>8.1f}  {:.2e}/{:.2e}".format(
            r["shape"], r["speedup_median"], r["kernel_fp32eq_tflops"], r["kernel_bf16_mfma_tflops"],
            r["library_tflops"], r["kernel_err_max"], r["library_err_max"]))


if __name__ == "__main__":
    main()
