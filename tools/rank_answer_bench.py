"""The ALBEF victim's ``vqa_answer`` (ViT + fusion encoder + ``rank_answer``) at ALBEF-base, batch 256 and 64, timed with hip
events: median of 7 calls after 3 warm-ups, and the peak device memory of a call.
    python tools/rank_answer_bench.py <tree> <label> <out.json>
``<tree>``: the checkout whose ``vqattack_amd`` is measured (``.``, or an exported and built parent commit);
``VQA_FUSED_RANK`` is read by that tree itself.  Records: ``profiles/r14/``."""
import json
import os
import statistics
import sys

tree, label, out = sys.argv[1], sys.argv[2], sys.argv[3]
sys.path.insert(0, os.path.abspath(tree))
import torch                                                    # noqa: E402
from vqattack_amd.whitebox import albef                          # noqa: E402

assert os.path.abspath(albef.__file__).startswith(os.path.abspath(tree)), albef.__file__
dev = torch.device("cuda", 0)
cfg = albef.albef_base()
white = albef.FrozenAlbef(cfg, seed=0)
black = albef.FrozenAlbef.finetuned_from(white, seed=1).to(dev)
del white
res = {"label": label, "fused_rank": getattr(black, "fused_rank", None), "batches": {}}
for batch in (256, 64):
    gen = torch.Generator(device=dev).manual_seed(1234)
    images = torch.empty(batch, 3, 384, 384, device=dev).uniform_(-1, 1, generator=gen)
    ids = torch.randint(1000, cfg.vocab, (batch, 25), device=dev, generator=gen)
    ids[:, 0] = cfg.cls_id
    n = torch.randint(6, 15, (batch,), device=dev, generator=gen)
    pos = torch.arange(25, device=dev)[None, :]
    ids = torch.where(pos == (n[:, None] - 1), torch.full_like(ids, cfg.sep_id), ids)
    ids = torch.where(pos >= n[:, None], torch.zeros_like(ids), ids)
    masks = (ids != 0).long()
    times, answers = [], None
    for it in range(10):
        if it == 3:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        answers = black.vqa_answer(images, ids, masks)
        b.record()
        torch.cuda.synchronize()
        if it >= 3:
            times.append(a.elapsed_time(b))
    peak = torch.cuda.max_memory_allocated()
    res["batches"][str(batch)] = {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times),
                                  "peak_allocated_gb": peak / 2 ** 30, "growth_gb": (peak - base) / 2 ** 30,
                                  "answers": answers.tolist()}
    print(label, batch, res["batches"][str(batch)]["median_ms"], peak / 2 ** 30, flush=True)
    del images
    torch.cuda.empty_cache()
json.dump(res, open(out, "w"))
