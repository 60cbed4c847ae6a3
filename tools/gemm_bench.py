"""Per-shape A/B of the encoder GEMMs: the bf16x6 kernel (``csrc/gemm.hip``) on its 256 x 128 tile ("kernel"), on its
128 x 256 tile ("wide", where N % 256 == 0) and its small-tile variant (one record per ``--ksplit`` value, plus the split
``ops.gemm_small_plan`` picks) against the library fp32 GEMM that ``torch.addmm`` / ``torch.mm`` run (with the recorded
TunableOp solutions active, as in bench.py).  For the shapes whose N is the FFN width (fc1 forward, fc2 input gradient) the
GELU epilogues of ``ops.gemm(..., epilogue=)`` are timed as further interleaved variants against the two-step form they
replace, on the tile the policy picks for the shape: "fused_gelu" (h stored) and "fused_gelu_nosave" against
"pair_gelu" (GEMM + ``vqa_gelu_fwd``), "fused_gelu_grad" against "pair_gelu_grad" (GEMM + ``vqa_gelu_bwd`` in place).
Every shape is also run whole on the 128 x 128 tile ("half", ``ops.gemm_half``).  Where ``ops.gemm_tail_plan`` cuts the
shape on this device's CU count (``VQA_GEMM_TAIL_CUS`` pins another), "tail" -- the policy tile up to the cut, the half
tile behind it (``vqa_gemm_bf16x6_tail``) -- is timed against "unsplit", the same entry point with the cut at M, by the
rule of ``_fused.TAIL_POLICY``; for comparison only, "tail_small" runs the rows behind the cut through
``gemm_small(ksplit=1)``, and "main" / "half_main" run the rows ahead of the cut (whole rounds of either tile) on the
policy tile and on the half tile, which gives the time of a round of half tiles over a round of full ones.  Each
carries ``same_bits_as_kernel``.  Where N % 256 == 0, "persistent" -- ``ops.gemm_persistent``, the 128 x 256 tile as one
launch of one workgroup per CU -- is timed against the tile ``_fused.gemm_tile`` picks for the shape (what is dispatched
without an entry in ``_fused.PERSISTENT_POLICY``), by that table's rule.  ``--image-rows`` replaces the image expert's row
count (the benchmark's own is 64 x 577 = 36928; the default here is batch x (tokens - text tokens)) and ``--rows`` the row
count of the shapes that see every token (qkv and the projections).

Random data (activations ~ N(0, 1), weights ~ N(0, 0.02^2)): bf16 MFMA loops hold a lower clock on random data than on
zeros.  The variants are interleaved in one process over several rounds; per shape the median and min time per call, the
fp32-equivalent TF/s (2 M N K / t), the bf16 MFMA TF/s the kernel sustains (6 products: 12 M N K / t) and the max / RMS
error of each against an fp64 product are reported, plus the speed-up and, per variant, the round-to-round spread
(max - min of the per-round times: the margin a difference has to beat).  One JSON line per shape, a summary at the end.
``--batch 1`` gives the shapes of the reference's own call (one sample per encoder pass); ``--graph`` times captured
graphs of ``--reps`` calls, as that path is replayed.

    python tools/gemm_bench.py [--model vlmo_base|albef_base|vlmo_large] [--batch B] [--ksplit 1,2,4,8] [--graph]
                               [--rounds 5] [--reps 10] [--warmup 3] [--only NAMES] [--out FILE]
(the per-kernel records since round 13 use --warmup 10 --rounds 7 --reps 50).

``--grouped`` times something else: per expert pair of a multiway layer (fc1 / fc2, forward and input gradient) the ONE
``ops.gemm_grouped`` launch over the image and the text expert's rows ("grouped", with the epilogue the dispatch gives
it) against the two calls that ``whitebox/_fused.py`` dispatches today ("today": each expert on the bf16x6 tile or the
library as its row count decides, GELU kernels included wherever either side launches them), by the rule of
``_fused.GROUPED_POLICY``; "image_only" is today's call on the image rows alone, so grouped - image_only is what the
text tiles cost in the image expert's last round.  ``--image-rows`` / ``--text-rows`` name the row counts (default: VLMO-base
at batch 64 with 577 image tokens, and 14 or 40 text tokens per sample).  One JSON line per pair and text row count.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqattack_amd import ops  # noqa: E402
from vqattack_amd.whitebox import _fused, tuned_gemms  # noqa: E402

# (dim, ffn, rows per sample, text rows per sample (0 = one modality), batch)
MODELS = {"vlmo_base": (768, 3072, 591, 40, 64), "albef_base": (768, 3072, 577, 0, 256),
          "vlmo_large": (1024, 4096, 591, 40, 128)}


def shapes(model, batch=0, img_rows=0, all_rows=0):
    """(name, M, N, K, bias) of every encoder GEMM of one layer, forward and input-gradient backward."""
    d, f, s, t, b = MODELS[model]
    b = batch or b
    rows = all_rows or b * s
    out = [("qkv_fwd", rows, 3 * d, d, True), ("qkv_bwd", rows, d, 3 * d, False),
           ("proj_fwd", rows, d, d, True), ("proj_bwd", rows, d, d, False)]
    experts = [("img", img_rows or b * (s - t)), ("txt", b * t)] if t else [("all", rows)]
    if t:
        experts.append(("vl", rows))
    for tag, m in experts:
        out += [("fc1_fwd_" + tag, m, f, d, True), ("fc1_bwd_" + tag, m, d, f, False),
                ("fc2_fwd_" + tag, m, d, f, True), ("fc2_bwd_" + tag, m, f, d, False)]
    return out


# (fused variant, the two-step form it replaces, the epilogue whose policy decides it)
EPILOGUE_AB = (("fused_gelu", "pair_gelu", "gelu"), ("fused_gelu_nosave", "pair_gelu", "gelu"),
               ("fused_gelu_grad", "pair_gelu_grad", "gelu_grad"))


def err(c, ref):
    e = (c.double() - ref).abs()
    return float(e.max()), float(e.pow(2).mean().sqrt())


def grouped_main(args):
    """``--grouped``: one record per (expert pair, text rows)."""
    tuned = tuned_gemms.enable()
    dev = torch.device("cuda")
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    gen = torch.Generator(device=dev).manual_seed(0)
    d, f = MODELS[args.model][:2]
    m_img = args.image_rows or 64 * 577
    # (name, N, K, bias, the GELU stage the GEMM feeds: None, "gelu" (forward) or "gelu_grad" (backward))
    pairs = [("fc1_fwd", f, d, True, "gelu"), ("fc2_fwd", d, f, True, None), ("fc2_bwd", f, d, False, "gelu_grad"),
             ("fc1_bwd", d, f, False, None)]
    results = []
    for m_txt in [int(v) for v in args.text_rows.split(",") if v]:
        for name, N, K, has_bias, stage in pairs:
            if args.only and name not in args.only.split(","):
                continue
            ex = []
            for m in (m_img, m_txt):                                    # the larger group first, as the dispatch orders them
                a = torch.randn(m, K, device=dev, generator=gen)
                w = torch.randn(N, K, device=dev, generator=gen) * 0.02
                bias = torch.randn(N, device=dev, generator=gen) * 0.02 if has_bias else None
                ex.append(dict(m=m, a=a, bt=w.t(), bias=bias, packed=ops.gemm_pack(w, trans=True),
                               h=torch.randn(m, N, device=dev, generator=gen),          # the backward's pre-activation
                               out=[torch.empty(m, N, device=dev) for _ in range(2)],     # [today, grouped]
                               act=[torch.empty(m, N, device=dev) for _ in range(2)],
                               kernel=_fused._kernel_gemms() and ops.gemm_workgroups(m, N) >= _fused.MIN_WORKGROUPS))
            for e in ex:
                e["fuse"] = bool(stage) and e["kernel"] and _fused.gelu_epilogue(e["m"], N, K, stage)
            fuse_grouped = ex[0]["fuse"]                                    # the larger group's decision serves the launch

            def gelu_kernels(e, slot):
                if stage == "gelu":
                    ops.gelu_fwd(e["out"][slot], out=e["act"][slot])
                elif stage == "gelu_grad":
                    ops.gelu_bwd(e["h"], e["out"][slot])

            def one(e):
                """What _linear / _linear_gelu / _linear_grad_gelu launch for this expert today."""
                if e["fuse"]:
                    if stage == "gelu":
                        ops.gemm(e["a"], e["packed"], e["bias"], out=e["act"][0], epilogue="gelu", aux=e["out"][0])
                    else:
                        ops.gemm(e["a"], e["packed"], e["bias"], out=e["out"][0], epilogue="gelu_grad", aux=e["h"])
                    return
                if e["kernel"]:
                    ops.gemm(e["a"], e["packed"], e["bias"], out=e["out"][0])
                elif e["bias"] is not None:
                    torch.addmm(e["bias"], e["a"], e["bt"], out=e["out"][0])
                else:
                    torch.mm(e["a"], e["bt"], out=e["out"][0])
                gelu_kernels(e, 0)

            def today():
                one(ex[1]), one(ex[0])                                      # text first, as the layer loop runs them

            def grouped():
                lists = ([e["a"] for e in ex], [e["packed"] for e in ex], [e["bias"] for e in ex])
                if fuse_grouped and stage == "gelu":
                    ops.gemm_grouped(*lists, out_list=[e["act"][1] for e in ex], epilogue="gelu",
                                     aux_list=[e["out"][1] for e in ex])
                elif fuse_grouped:
                    ops.gemm_grouped(*lists, out_list=[e["out"][1] for e in ex], epilogue="gelu_grad",
                                     aux_list=[e["h"] for e in ex])
                else:
                    ops.gemm_grouped(*lists, out_list=[e["out"][1] for e in ex])
                    for e in ex:
                        gelu_kernels(e, 1)

            variants = [("today", today), ("grouped", grouped), ("image_only", lambda: one(ex[0])),
                        ("text_only", lambda: one(ex[1]))]
            times = {key: [] for key, _ in variants}
            for _ in range(args.warmup):
                for _, fn in variants:
                    fn()
            torch.cuda.synchronize()
            for _ in range(args.rounds):
                for key, fn in variants:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.reps):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[key].append(e0.elapsed_time(e1) / args.reps)
            # bits: the image rows keep today's; the text rows have those of ops.gemm on them (today's where they run
            # the kernel already).  In-place GELU' outputs are recomputed from scratch on both sides.
            today(), grouped()
            torch.cuda.synchronize()
            final = "act" if stage == "gelu" else "out"
            img_same = bool(torch.equal(ex[0][final][0], ex[0][final][1]))
            txt_today_same = bool(torch.equal(ex[1][final][0], ex[1][final][1]))
            t = ex[1]
            ref = ops.gemm(t["a"], t["packed"], t["bias"], tile="wide")
            if stage == "gelu":
                ref = ops.gelu_fwd(ref)
            elif stage == "gelu_grad":
                ref = ops.gelu_bwd(t["h"], ref)
            txt_same = bool(torch.equal(ref, t[final][1]))
            txt_diff = float((t[final][0] - t[final][1]).abs().max())

            def stats(key):
                ts = times[key]
                return dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_spread=max(ts) - min(ts))
            starts, grid = ops.gemm_grouped_blocks((m_img, m_txt), N)
            img_grid = starts[1] * (N // 256)
            row = dict(pair=name, N=N, K=K, bias=has_bias, image_rows=m_img, text_rows=m_txt, stage=stage,
                       grouped_epilogue=stage if fuse_grouped else None, image_today_fused=ex[0]["fuse"],
                       text_today="kernel" if ex[1]["kernel"] else "library", text_today_fused=ex[1]["fuse"],
                       grid=grid, image_grid=img_grid, cus=cus, rounds_grouped=grid / cus, rounds_image=img_grid / cus,
                       policy_groups=_fused.gemm_grouped_pair((m_img, m_txt), N, K),
                       image_same_bits_as_today=img_same, text_same_bits_as_ops_gemm=txt_same,
                       text_same_bits_as_today=txt_today_same, text_max_abs_diff_to_today=txt_diff,
                       **{key: stats(key) for key, _ in variants})
            g, u = row["grouped"], row["today"]
            g["speedup_vs_today_median"] = u["ms_median"] / g["ms_median"]
            g["margin_ms"] = u["ms_median"] - g["ms_median"]
            g["larger_spread_ms"] = max(g["ms_spread"], u["ms_spread"])
            g["passes_rule"] = g["margin_ms"] > g["larger_spread_ms"]
            g["text_price_ms"] = g["ms_median"] - row["image_only"]["ms_median"]
            print(json.dumps(row), flush=True)
            results.append(row)
            del ex, ref
            torch.cuda.empty_cache()
    summary = dict(model=args.model, grouped=True, tuned_gemms=tuned, device=torch.cuda.get_device_name(), rounds=args.rounds,
                   reps=args.reps, warmup=args.warmup, pairs=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    print("pair      text rows  grouped ms (spread)   today ms (spread)   x today  margin   rule   image only  text price  text today")
    for r in results:
        g, u = r["grouped"], r["today"]
        print("{:<10}{:>9}  {:.4f} ({:.4f})     {:.4f} ({:.4f})   {:>7.3f}  {:+.4f}  {}  {:.4f}      {:+.4f}     {:.4f} {}{}  bits img {} txt {}"
              .format(r["pair"], r["text_rows"], g["ms_median"], g["ms_spread"], u["ms_median"], u["ms_spread"],
                      g["speedup_vs_today_median"], g["margin_ms"], "passes" if g["passes_rule"] else "fails ",
                      r["image_only"]["ms_median"], g["text_price_ms"], r["text_only"]["ms_median"], r["text_today"],
                      " epi " + r["grouped_epilogue"] if r["grouped_epilogue"] else "",
                      "equal" if r["image_same_bits_as_today"] else "DIFFER",
                      "equal" if r["text_same_bits_as_ops_gemm"] else "DIFFER"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="vlmo_base", choices=sorted(MODELS))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3, help="untimed passes over all variants ahead of the timed rounds")
    ap.add_argument("--only", default="", help="comma-separated shape names")
    ap.add_argument("--batch", type=int, default=0, help="samples per encoder pass (default: the model's benchmark batch)")
    ap.add_argument("--ksplit", default="1,2,4,8", help="comma-separated K splits of the small-tile kernel ('' = none)")
    ap.add_argument("--graph", action="store_true",
                    help="time each variant as ONE captured graph of --reps calls (device time without the host's launch "
                         "cost: how the batch-1 path runs, which is replayed from a captured graph)")
    ap.add_argument("--out", default="")
    ap.add_argument("--rows", type=int, default=0, help="rows of the shapes that see every token (default: batch x tokens)")
    ap.add_argument("--grouped", action="store_true",
                    help="time ops.gemm_grouped per expert pair against the two calls dispatched today (see above)")
    ap.add_argument("--image-rows", type=int, default=0,
                    help="rows of the image expert (default: batch x image tokens; with --grouped 64 x 577)")
    ap.add_argument("--text-rows", default="896,2560", help="--grouped: comma-separated row counts of the text expert")
    args = ap.parse_args()
    if args.grouped:
        return grouped_main(args)
    tuned = tuned_gemms.enable()
    dev = torch.device("cuda")
    # CUs the tail cut is planned for: the device's, or the pinned count the dispatch would use
    cus = int(os.environ.get("VQA_GEMM_TAIL_CUS") or torch.cuda.get_device_properties(dev).multi_processor_count)
    gen = torch.Generator(device=dev).manual_seed(0)
    results = []
    ksplits = [int(v) for v in args.ksplit.split(",") if v]
    for name, M, N, K, has_bias in shapes(args.model, args.batch, args.image_rows, args.rows):
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
            ops.gemm(a, packed, bias, out=out_k, tile="large")

        def run_library():
            if bias is not None:
                torch.addmm(bias, a, bt, out=out_l)
            else:
                torch.mm(a, bt, out=out_l)

        variants = [("kernel", run_kernel), ("library", run_library)]
        out_w = torch.empty(M, N, device=dev)
        if N % 256 == 0:
            variants.append(("wide", lambda: ops.gemm(a, packed, bias, out=out_w, tile="wide")))
        out_p = torch.empty(M, N, device=dev)
        if N % 256 == 0:
            variants.append(("persistent", lambda: ops.gemm_persistent(a, packed, bias, out=out_p)))
        planned = ops.gemm_small_plan(M, N, K)
        small = sorted({k for k in ksplits + [planned] if 1 <= k <= min(K // 32, 16)}) if ksplits else []
        out_s = torch.empty(M, N, device=dev)
        for k in small:
            variants.append(("small%d" % k, lambda k=k: ops.gemm_small(a, packed, bias, out=out_s, ksplit=k)))
        epi_tile = _fused.gemm_tile(M, N, K)
        # the 128 x 128 tile: alone ("half"), and behind the last full round of the policy tile's launch where
        # ops.gemm_tail_plan cuts the shape on this device ("tail", against "unsplit" = the same tile uncut).  For
        # comparison only: the same rows behind the cut on the 64 x 128 kernel ("tail_small"), and the rows ahead of the
        # cut -- whole rounds on either tile -- alone on the policy tile ("main") and on the half tile ("half_main").
        out_h = torch.empty(M, N, device=dev)
        variants.append(("half", lambda: ops.gemm_half(a, packed, bias, out=out_h)))
        cut = ops.gemm_tail_plan(M, N, epi_tile, cus)
        out_t = torch.empty(M, N, device=dev)
        if cut < M:
            def tail_small():
                ops.gemm(a[:cut], packed, bias, out=out_t[:cut], tile=epi_tile, m_split=cut)
                ops.gemm_small(a[cut:], packed, bias, out=out_t[cut:], ksplit=1)

            variants += [("unsplit", lambda: ops.gemm(a, packed, bias, out=out_t, tile=epi_tile, m_split=M)),
                         ("tail", lambda: ops.gemm(a, packed, bias, out=out_t, tile=epi_tile, m_split=cut)),
                         ("tail_small", tail_small),
                         ("main", lambda: ops.gemm(a[:cut], packed, bias, out=out_t[:cut], tile=epi_tile, m_split=cut)),
                         ("half_main", lambda: ops.gemm_half(a[:cut], packed, bias, out=out_t[:cut]))]
        if N == MODELS[args.model][1]:
            h_e, act_e, dh_e = (torch.empty(M, N, device=dev) for _ in range(3))
            h_p, act_p, dh_p = (torch.empty(M, N, device=dev) for _ in range(3))
            h_in = torch.randn(M, N, device=dev, generator=gen)          # the pre-activation the backward reads

            def pair_gelu():
                ops.gelu_fwd(ops.gemm(a, packed, bias, out=h_p, tile=epi_tile), out=act_p)

            def pair_gelu_grad():
                ops.gelu_bwd(h_in, ops.gemm(a, packed, bias, out=dh_p, tile=epi_tile))

            variants += [("pair_gelu", pair_gelu),
                         ("fused_gelu", lambda: ops.gemm(a, packed, bias, out=act_e, tile=epi_tile, epilogue="gelu", aux=h_e)),
                         ("fused_gelu_nosave", lambda: ops.gemm(a, packed, bias, out=act_e, tile=epi_tile, epilogue="gelu")),
                         ("pair_gelu_grad", pair_gelu_grad),
                         ("fused_gelu_grad",
                          lambda: ops.gemm(a, packed, bias, out=dh_e, tile=epi_tile, epilogue="gelu_grad", aux=h_in))]
        times = {key: [] for key, _ in variants}
        for _ in range(args.warmup):                # warm-up: code objects, then the clock the timed rounds run at
            for _, fn in variants:
                fn()
        torch.cuda.synchronize()
        graphs = {}
        if args.graph:
            for key, fn in variants:
                graphs[key] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[key]):
                    for _ in range(args.reps):
                        fn()
                graphs[key].replay()
            torch.cuda.synchronize()
        for _ in range(args.rounds):
            for key, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                if args.graph:
                    graphs[key].replay()
                else:
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
        small_rows = []
        for k in small:
            ops.gemm_small(a, packed, bias, out=out_s, ksplit=k)
            torch.cuda.synchronize()
            es, ts = err(out_s, ref), times["small%d" % k]
            small_rows.append(dict(ksplit=k, planned=k == planned, ms_median=statistics.median(ts), ms_min=min(ts),
                                   ms_spread=max(ts) - min(ts), err_max=es[0], err_rms=es[1],
                                   speedup_vs_library_median=statistics.median(times["library"]) / statistics.median(ts)))
        wide = None
        if "wide" in times:
            ops.gemm(a, packed, bias, out=out_w, tile="wide")
            torch.cuda.synchronize()
            ew, tw = err(out_w, ref), times["wide"]
            wide = dict(ms_median=statistics.median(tw), ms_min=min(tw), ms_spread=max(tw) - min(tw), err_max=ew[0],
                        err_rms=ew[1], same_bits_as_kernel=bool(torch.equal(out_w, out_k)),
                        speedup_vs_kernel_median=statistics.median(times["kernel"]) / statistics.median(tw),
                        bf16_mfma_tflops=12.0 * M * N * K / statistics.median(tw) / 1e9)

        def med(key):
            return statistics.median(times[key])

        def stats(key):
            ts = times[key]
            return dict(ms_median=statistics.median(ts), ms_min=min(ts), ms_spread=max(ts) - min(ts))

        ops.gemm_half(a, packed, bias, out=out_h)
        torch.cuda.synchronize()
        half = dict(stats("half"), same_bits_as_kernel=bool(torch.equal(out_h, out_k)), workgroups=-(-M // 128) * (N // 128),
                    speedup_vs_kernel_median=med("kernel") / med("half"))
        persistent = None
        if "persistent" in times:
            out_p.fill_(7.0)
            ops.gemm_persistent(a, packed, bias, out=out_p)
            torch.cuda.synchronize()
            today = "wide" if epi_tile == "wide" else "kernel"          # the variant that runs _fused.gemm_tile's tile
            u = stats(today)
            persistent = dict(stats("persistent"), same_bits_as_kernel=bool(torch.equal(out_p, out_k)), today=today,
                              tiles=-(-M // 128) * (N // 256), workgroups=min(_fused.device_cus(dev), -(-M // 128) * (N // 256)),
                              policy_lists=_fused.gemm_persistent(M, N, K), today_ms_median=u["ms_median"],
                              today_ms_spread=u["ms_spread"], speedup_vs_today_median=u["ms_median"] / med("persistent"))
            # the policy's rule: the medians' difference against the larger round-to-round spread of the two
            persistent["margin_ms"] = u["ms_median"] - persistent["ms_median"]
            persistent["larger_spread_ms"] = max(persistent["ms_spread"], u["ms_spread"])
            persistent["passes_rule"] = persistent["margin_ms"] > persistent["larger_spread_ms"]
            if "wide" in times:
                persistent["speedup_vs_wide_median"] = med("wide") / med("persistent")
        tail = None
        if "tail" in times:
            tail = dict(tile=epi_tile, cus=cus, m_split=cut, tail_workgroups=-(-(M - cut) // 128) * (N // 128),
                        policy_cuts=_fused.gemm_tail_split(M, N, K, epi_tile, dev) < M)
            for key in ("unsplit", "tail", "tail_small", "main", "half_main"):
                out_t.fill_(7.0)
                dict(variants)[key]()
                torch.cuda.synchronize()
                rows = cut if key in ("main", "half_main") else M
                tail[key] = dict(stats(key), same_bits_as_kernel=bool(torch.equal(out_t[:rows], out_k[:rows])))
            for key in ("tail", "tail_small"):
                t, u = tail[key], tail["unsplit"]
                t["speedup_vs_unsplit_median"] = u["ms_median"] / t["ms_median"]
                # the policy's rule: the medians' difference against the larger round-to-round spread of the two
                t["margin_ms"] = u["ms_median"] - t["ms_median"]
                t["larger_spread_ms"] = max(t["ms_spread"], u["ms_spread"])
                t["passes_rule"] = t["margin_ms"] > t["larger_spread_ms"]
            # rows [0, cut) are whole rounds of the policy tile and twice as many of the half tile: the time of a round
            # of half tiles over the time of a round of full ones (0.5 = a half tile costs half a full one)
            tail["half_round_over_full_round"] = tail["half_main"]["ms_median"] / (2.0 * tail["main"]["ms_median"])
        epilogue = None
        if "fused_gelu" in times:
            pair_gelu()
            pair_gelu_grad()
            ops.gemm(a, packed, bias, out=act_e, tile=epi_tile, epilogue="gelu", aux=h_e)
            ops.gemm(a, packed, bias, out=dh_e, tile=epi_tile, epilogue="gelu_grad", aux=h_in)
            torch.cuda.synchronize()
            same = torch.equal(h_e, h_p) and torch.equal(act_e, act_p) and torch.equal(dh_e, dh_p)
            fuses = {epi: _fused.gelu_epilogue(M, N, K, epi) for epi in ("gelu", "gelu_grad")}
            epilogue = dict(tile=epi_tile, policy_fuses=fuses, same_bits=bool(same))
            for key in ("pair_gelu", "fused_gelu", "fused_gelu_nosave", "pair_gelu_grad", "fused_gelu_grad"):
                epilogue[key] = stats(key)
            for fused, pair, _epi in EPILOGUE_AB:
                f, q = epilogue[fused], epilogue[pair]
                f["speedup_vs_pair_median"] = q["ms_median"] / f["ms_median"]
                # the policy's rule: the medians' difference against the larger round-to-round spread of the two
                f["margin_ms"] = q["ms_median"] - f["ms_median"]
                f["larger_spread_ms"] = max(f["ms_spread"], q["ms_spread"])
                f["passes_rule"] = f["margin_ms"] > f["larger_spread_ms"]
            del h_e, act_e, dh_e, h_p, act_p, dh_p, h_in
        del ref, graphs
        med_k, med_l = statistics.median(times["kernel"]), statistics.median(times["library"])
        flop = 2.0 * M * N * K
        row = dict(shape=name, M=M, N=N, K=K, bias=has_bias,
                   kernel_ms_median=med_k, kernel_ms_min=min(times["kernel"]),
                   library_ms_median=med_l, library_ms_min=min(times["library"]),
                   speedup_median=med_l / med_k, speedup_min=min(times["library"]) / min(times["kernel"]),
                   kernel_fp32eq_tflops=flop / med_k / 1e9, kernel_bf16_mfma_tflops=6 * flop / med_k / 1e9,
                   library_tflops=flop / med_l / 1e9,
                   kernel_ms_spread=max(times["kernel"]) - min(times["kernel"]),
                   library_ms_spread=max(times["library"]) - min(times["library"]),
                   big_workgroups=ops.gemm_workgroups(M, N), small_tiles=ops.gemm_small_workgroups(M, N), small=small_rows,
                   wide=wide, policy_tile=_fused.gemm_tile(M, N, K), half=half, tail=tail, epilogue=epilogue,
                   persistent=persistent,
                   kernel_err_max=ek[0], kernel_err_rms=ek[1], library_err_max=el[0], library_err_rms=el[1])
        print(json.dumps(row), flush=True)
        results.append(row)
        del a, w, packed, out_k, out_l, out_s, out_w, out_h, out_t, out_p
        torch.cuda.empty_cache()
    summary = dict(model=args.model, batch=args.batch or MODELS[args.model][4], tuned_gemms=tuned, device=torch.cuda.get_device_name(),
                   rounds=args.rounds, reps=args.reps, warmup=args.warmup, graph=args.graph, shapes=results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(summary, fh, indent=1)
    print("shape               speedup(med)  kernel TF  bf16 TF  lib TF  err k/lib (max)")
    for r in results:
        print("{:<20}{:>10.3f}{:>11.1f}{:>9.0f}{:>8.1f}  {:.2e}/{:.2e}".format(
            r["shape"], r["speedup_median"], r["kernel_fp32eq_tflops"], r["kernel_bf16_mfma_tflops"],
            r["library_tflops"], r["kernel_err_max"], r["library_err_max"]))
        if r["wide"]:
            wd = r["wide"]
            print("  wide tile {}   {:>8.3f}x kernel   {:.4f} ms (spread {:.4f}; kernel {:.4f} spread {:.4f})  bf16 {:.0f} TF  "
                  "bits {}".format("*" if r["policy_tile"] == "wide" else " ", wd["speedup_vs_kernel_median"],
                                   wd["ms_median"], wd["ms_spread"], r["kernel_ms_median"], r["kernel_ms_spread"],
                                   wd["bf16_mfma_tflops"], "equal" if wd["same_bits_as_kernel"] else "DIFFER"))
        hf = r["half"]
        print("  half tile    {:>8.3f}x kernel   {:.4f} ms (spread {:.4f})  {} workgroups  bits {}".format(
            hf["speedup_vs_kernel_median"], hf["ms_median"], hf["ms_spread"], hf["workgroups"],
            "equal" if hf["same_bits_as_kernel"] else "DIFFER"))
        if r["persistent"]:
            ps = r["persistent"]
            print("  persistent {} {:>8.3f}x {:<7}  {:.4f} ms (spread {:.4f}; {} {:.4f} spread {:.4f})  margin {:+.4f} {}  "
                  "{} tiles on {} workgroups  bits {}".format(
                      "*" if ps["policy_lists"] else " ", ps["speedup_vs_today_median"], ps["today"], ps["ms_median"],
                      ps["ms_spread"], ps["today"], ps["today_ms_median"], ps["today_ms_spread"], ps["margin_ms"],
                      "passes" if ps["passes_rule"] else "fails", ps["tiles"], ps["workgroups"],
                      "equal" if ps["same_bits_as_kernel"] else "DIFFER"))
        if r["tail"]:
            tl = r["tail"]
            for key in ("tail", "tail_small"):
                t, u = tl[key], tl["unsplit"]
                print("  {:<11}{} {:>8.3f}x unsplit  {:.4f} ms (spread {:.4f}; unsplit {:.4f} spread {:.4f})  margin {:+.4f} {}  "
                      "tile {} cut {} + {} half tiles on {} CUs  bits {}".format(
                          key, "*" if key == "tail" and tl["policy_cuts"] else " ", t["speedup_vs_unsplit_median"],
                          t["ms_median"], t["ms_spread"], u["ms_median"], u["ms_spread"], t["margin_ms"],
                          "passes" if t["passes_rule"] else "fails", tl["tile"], tl["m_split"], tl["tail_workgroups"],
                          tl["cus"], "equal" if t["same_bits_as_kernel"] and u["same_bits_as_kernel"] else "DIFFER"))
            print("  rows ahead of the cut: {} tile {:.4f} ms, half tile {:.4f} ms: a round of half tiles takes {:.3f} of a "
                  "round of full ones".format(tl["tile"], tl["main"]["ms_median"], tl["half_main"]["ms_median"],
                                              tl["half_round_over_full_round"]))
        if r["epilogue"]:
            ep = r["epilogue"]
            for fused, pair, epi in EPILOGUE_AB:
                f, q = ep[fused], ep[pair]
                print("  {:<18}{} {:>7.3f}x pair   {:.4f} ms (spread {:.4f}; pair {:.4f} spread {:.4f})  margin {:+.4f} {}  "
                      "tile {}  bits {}".format(fused, "*" if ep["policy_fuses"][epi] else " ",
                                                f["speedup_vs_pair_median"], f["ms_median"], f["ms_spread"], q["ms_median"],
                                                q["ms_spread"], f["margin_ms"], "passes" if f["passes_rule"] else "fails",
                                                ep["tile"], "equal" if ep["same_bits"] else "DIFFER"))
        for sm in r["small"]:
            print("  small ksplit {:<2}{} {:>8.3f}x library  {:.4f} ms (spread {:.4f}; library {:.4f} spread {:.4f})  err {:.2e}"
                  .format(sm["ksplit"], "*" if sm["planned"] else " ", sm["speedup_vs_library_median"], sm["ms_median"],
                          sm["ms_spread"], r["library_ms_median"], r["library_ms_spread"], sm["err_max"]))


if __name__ == "__main__":
    main()
