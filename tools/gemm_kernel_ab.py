"""Two-library A/B of the large-tile bf16x6 GEMM kernels (``csrc/gemm.hip``): one build of the kernel library against
another, in ONE process, on the same operands.

Both libraries are loaded through ctypes next to each other (``--parent`` is the ``libvqattack_hip.so`` of another tree,
built there; ``--new`` defaults to this tree's) and called through the C ABI they share: ``vqa_gemm_bf16x6_tile`` for the
plain GEMM, ``vqa_gemm_bf16x6_epi`` for the GELU (h stored) and GELU' epilogues.  Per row the two are interleaved -- warm-up
passes over both, then ``--rounds`` rounds of (``--reps`` calls of the parent, ``--reps`` calls of the new build), timed
with events -- and the outputs (and the stored h) are compared bit for bit.  Reported per row: the median time per call
and the round-to-round spread (max - min) of each, their ratio, the margin (difference of the medians) against the larger
spread -- the rule of profiles/r10 onwards: a difference counts where the margin exceeds the larger spread -- and whether
the bits are equal.

Rows: the benchmark's encoder classes qkv_fwd, qkv_bwd, proj, fc1_fwd (epilogues 0 / 1 / 2), fc1_bwd at ``--rows`` row
counts on both tiles and at ``--rows-large`` on the 256 x 128 tile only.  Random data (activations ~ N(0, 1), weights and
bias ~ N(0, 0.02^2)), as in tools/gemm_bench.py.

    python tools/gemm_kernel_ab.py --parent ../parent/vqattack_amd/lib/libvqattack_hip.so [--new LIB]
                                   [--rows 35264,37824] [--rows-large 147712] [--warmup 10] [--rounds 7] [--reps 50]
                                   [--only CLASSES] [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqattack_amd import _hip  # noqa: E402

# class -> (N, K, bias, epilogues timed)
CLASSES = {"qkv_fwd": (2304, 768, True, (0,)), "qkv_bwd": (768, 2304, False, (0,)), "proj": (768, 768, True, (0,)),
           "fc1_fwd": (3072, 768, True, (0, 1, 2)), "fc1_bwd": (768, 3072, False, (0,))}
TILES = {"large": 0, "wide": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True, help="libvqattack_hip.so of the tree compared against")
    ap.add_argument("--new", default=_hip.LIB_PATH)
    ap.add_argument("--rows", default="35264,37824", help="row counts run on both tiles")
    ap.add_argument("--rows-large", default="147712", help="row counts run on the 256 x 128 tile only")
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="", help="comma-separated classes")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if os.path.realpath(args.parent) == os.path.realpath(args.new):
        raise SystemExit("--parent and --new are the same file")
    libs = {"parent": _hip.load_library(args.parent), "new": _hip.load_library(args.new)}
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = _hip.ptr
    plan = [(int(m), ("large", "wide")) for m in args.rows.split(",") if m]
    plan += [(int(m), ("large",)) for m in args.rows_large.split(",") if m]
    results = []
    for M, tiles in plan:
        for cls, (N, K, has_bias, epilogues) in CLASSES.items():
            if args.only and cls not in args.only.split(","):
                continue
            a = torch.randn(M, K, device=dev, generator=gen)
            w = torch.randn(N, K, device=dev, generator=gen) * 0.02
            bias = torch.randn(N, device=dev, generator=gen) * 0.02 if has_bias else None
            packed = torch.empty(libs["new"].vqa_gemm_packed_bytes(K, N), dtype=torch.uint8, device=dev)
            _hip.check(libs["new"].vqa_gemm_pack_b(p(w), K, 1, p(packed), K, N, stream), "vqa_gemm_pack_b")
            h_in = torch.randn(M, N, device=dev, generator=gen) if 2 in epilogues else None
            out = {k: torch.empty(M, N, device=dev) for k in libs}
            aux = {k: torch.empty(M, N, device=dev) for k in libs} if 1 in epilogues else None
            for tile in tiles:
                for epi in epilogues:
                    def call(k):
                        if epi == 0:
                            rc = libs[k].vqa_gemm_bf16x6_tile(p(a), K, p(packed), p(bias), p(out[k]), N, M, N, K, TILES[tile],
                                                              stream)
                        else:
                            x = aux[k] if epi == 1 else h_in
                            rc = libs[k].vqa_gemm_bf16x6_epi(p(a), K, p(packed), p(bias), p(out[k]), N, M, N, K, TILES[tile],
                                                             epi, p(x), N, stream)
                        if rc != 0:
                            raise RuntimeError("{} library returned {}".format(k, rc))
                    for t in list(out.values()) + (list(aux.values()) if epi == 1 else []):
                        t.fill_(float("nan"))
                    for _ in range(args.warmup):
                        call("parent"), call("new")
                    torch.cuda.synchronize()
                    times = {k: [] for k in libs}
                    for _ in range(args.rounds):
                        for k in libs:
                            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            e0.record()
                            for _ in range(args.reps):
                                call(k)
                            e1.record()
                            e1.synchronize()
                            times[k].append(e0.elapsed_time(e1) / args.reps)
                    same = torch.equal(out["parent"].view(torch.int32), out["new"].view(torch.int32))
                    if epi == 1:
                        same = same and torch.equal(aux["parent"].view(torch.int32), aux["new"].view(torch.int32))
                    med = {k: statistics.median(v) for k, v in times.items()}
                    spread = {k: max(v) - min(v) for k, v in times.items()}
                    margin, larger = med["parent"] - med["new"], max(spread.values())
                    row = dict(M=M, cls=cls, N=N, K=K, tile=tile, epilogue=epi, parent_ms=med["parent"], new_ms=med["new"],
                               parent_spread_ms=spread["parent"], new_spread_ms=spread["new"], ratio=med["parent"] / med["new"],
                               margin_ms=margin, larger_spread_ms=larger, passes_rule=margin > larger, bits_equal=bool(same),
                               new_bf16_mfma_tflops=12.0 * M * N * K / med["new"] / 1e9, times_ms=times)
                    results.append(row)
                    print("{:>6} {:<8} {:<5} epi{}  parent {:.4f} ({:.4f})  new {:.4f} ({:.4f})  {:.3f}x  margin {:+.4f}/{:.4f} {}  "
                          "bits {}  {:.0f} TF".format(M, cls, tile, epi, med["parent"], spread["parent"], med["new"], spread["new"],
                                                      row["ratio"], margin, larger, "ok" if row["passes_rule"] else "FAILS",
                                                      "equal" if same else "DIFFER", row["new_bf16_mfma_tflops"]), flush=True)
            del a, w, packed, out, aux, h_in
            torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(dict(device=torch.cuda.get_device_name(), parent=args.parent, new=args.new, warmup=args.warmup,
                           rounds=args.rounds, reps=args.reps, rows=results), fh, indent=1)
    if not all(r["bits_equal"] for r in results):
        raise SystemExit("bits differ")


if __name__ == "__main__":
    main()
