"""The two grades of the attention backward (VQA_ATTN_BWD = f32 | x6) on the bench shape, alternating in one process.

    python tools/attn_bwd_ab.py [rounds]

B 64, H 12, S 591 (VLMO-base, 384 px; B / S from the environment), shared bias slab; scores, o and lse come from a real
forward (its default grade), go is random.  Per round and grade: HIP events over 20 back-to-back ``vqa_attn_bwd`` /
``vqa_attn_bwd_x6`` calls after 5 warm-up calls.  A call is three launches -- attn_delta_kernel, the dK / dV kernel and
attn_bwd_dq_staged_kernel -- of which only the dK / dV kernel differs between the grades, so the difference of the two
call times is that kernel's.  For the three kernels' own times run the tool under a kernel trace
(``rocprofv3 --kernel-trace --stats -- python tools/attn_bwd_ab.py 1``).  Then the largest differences of the two grades' dq / dk /
dv and a summary by the project's rule (a difference counts when it exceeds the larger of the two max - min spreads).
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vqattack_amd import attention  # noqa: E402

B, H, S, D = int(os.environ.get("B", "64")), 12, int(os.environ.get("S", "591")), 64
GRADES = ("f32", "x6")


def timeit(fn, reps=20, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    os.environ["VQA_ATTN_SPLIT"] = "1"
    g = torch.Generator(device="cuda").manual_seed(0)
    qkv = torch.randn(B, S, 3, H, D, device="cuda", generator=g)
    go = torch.randn(B, S, H, D, device="cuda", generator=g)
    spad = (S + 31) // 32 * 32
    store = torch.zeros(1, H, S, spad, device="cuda")
    store[..., :S] = torch.randn(1, H, S, S, device="cuda", generator=g) * 0.02
    bias = store[..., :S].expand(B, -1, -1, -1)
    bstr = (bias.stride(0), bias.stride(1), bias.stride(2))
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    o, lse, scores = attention._forward(q, k, v, bias, bstr, D ** -0.5, save_scores=True)
    assert scores is not None
    dqkv = torch.empty_like(qkv)

    def run():
        attention._backward(q, k, v, bias, bstr, o, lse, go, dqkv[:, :, 0], dqkv[:, :, 1], dqkv[:, :, 2], D ** -0.5,
                            scores=scores)

    out, ms = {}, {grade: [] for grade in GRADES}
    for grade in GRADES:
        os.environ["VQA_ATTN_BWD"] = grade
        assert attention.backward_grade(1, True, True) == grade
        run()
        out[grade] = dqkv.clone()
    diff = (out["f32"] - out["x6"]).abs()
    print(json.dumps(dict(what="largest |f32 - x6| (largest |f32|)",
                          **{n: "{:.3g} ({:.3g})".format(float(diff[:, :, i].max()), float(out["f32"][:, :, i].abs().max()))
                             for i, n in enumerate(("dq", "dk", "dv"))})), flush=True)
    for rnd in range(-1, rounds):                 # round -1 brings the clocks up and is not recorded
        for grade in GRADES:
            os.environ["VQA_ATTN_BWD"] = grade
            t = timeit(run)
            if rnd < 0:
                continue
            ms[grade].append(t)
            print(json.dumps(dict(round=rnd, grade=grade, bwd_ms=round(t, 4))), flush=True)
    spread = max(max(x) - min(x) for x in ms.values())
    gain = min(ms["f32"]) - max(ms["x6"])
    print(json.dumps(dict(shape=[B, H, S], f32_ms=[round(x, 4) for x in ms["f32"]], x6_ms=[round(x, 4) for x in ms["x6"]],
                          larger_spread=round(spread, 4), best_f32_minus_worst_x6=round(gain, 4),
                          counts=bool(gain > spread))), flush=True)


if __name__ == "__main__":
    main()
