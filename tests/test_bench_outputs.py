"""What a plain ``bench.py`` run reports and what ``--dump-outputs DIR`` writes.

A plain run sets up, warms up, times ``--steps`` steps and prints the headline line; the auxiliary measurements (per-launch
kernel timing, microbenches, reference-style leg, CPU baseline) come only with ``--full``.  ``--dump-outputs`` writes the
last timed step's outputs as ``DIR/<name>.npy`` (float32 / float64, < 64 MB).  The inputs and every step's random
start are seeded: the same arguments give the same outputs in every run.  The GPU runs are forked from the pre-GPU fork server of
``tests/conftest.py``: each is a fresh process, as a command-line run is.
"""
import json
import multiprocessing
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUXILIARY = ("roofline", "roofline_loss", "platform_stream_probe", "roofline_b256", "roofline_attention",
             "reference_style", "cpu_baseline")


def _parse(monkeypatch, argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_full_is_off_by_default_and_steps_are_taken_as_given(monkeypatch):
    args = _parse(monkeypatch, ["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert args.full is False and args.dump_outputs is None and args.steps == 7 and args.warmup == 3
    assert _parse(monkeypatch, ["--full"]).full is True


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--warmup", "-1"], ["--sweep", "64", "--dump-outputs", "d"],
                                  ["--dry-run", "--dump-outputs", "d"]], ids=["steps0", "warmup-1", "sweep", "dry"])
def test_invalid_combinations_are_refused(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, argv)


@pytest.mark.parametrize("joint", [0, 3])
def test_inputs_are_the_same_in_every_run(monkeypatch, joint):
    import bench
    args = _parse(monkeypatch, ["--batch", "5", "--joint", str(joint)])
    first, again = (bench.synthetic_inputs(args, 32, 16, "cpu", rank=1) for _ in range(2))
    other_rank = bench.synthetic_inputs(args, 32, 16, "cpu", rank=0)
    for a, b in zip(first, again):
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b
    assert first[0].shape == (5, 3, 32, 32) and first[1].shape == (5, 16) and int(first[4].sum()) == 5 * joint
    assert not torch.equal(first[0], other_rank[0])


def test_dump_writes_a_fixed_sample_of_the_images_and_everything_else_whole(tmp_path):
    import bench
    from vqattack_amd.attack.runner import BatchResult
    g = torch.Generator().manual_seed(3)
    adv = torch.rand(40, 3, 384, 384, generator=g)
    ids = torch.randint(0, 30522, (40, 40), generator=g)
    res = BatchResult(adv_images=adv, adv_text_ids=ids, loss_lists=[[1.0, 2.0], torch.tensor([3.0])])
    answers = torch.randint(0, 3129, (40,), generator=g)
    bench.dump_outputs(str(tmp_path / "a"), res, answers, answers % 2 == 0)
    got = {f[:-4]: np.load(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))}
    assert set(got) == {"adv_images_sample", "adv_images_sample_index", "adv_images_sum_per_sample", "adv_text_ids",
                        "loss", "adv_answers", "success"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    index = got["adv_images_sample_index"].astype(np.int64)
    assert len(index) == 16 and len(set(index.tolist())) == 16 and list(index) == sorted(index)
    assert np.array_equal(got["adv_images_sample"], adv.numpy()[index])
    assert np.allclose(got["adv_images_sum_per_sample"], adv.double().reshape(40, -1).sum(1).numpy(), rtol=1e-12)
    assert np.array_equal(got["adv_text_ids"], ids.double().numpy()) and list(got["loss"]) == [1.0, 2.0, 3.0]
    assert np.array_equal(got["success"], (answers % 2 == 0).double().numpy())
    bench.dump_outputs(str(tmp_path / "b"), res, answers, answers % 2 == 0)     # the sample is fixed, not drawn per call
    assert np.array_equal(np.load(str(tmp_path / "b" / "adv_images_sample_index.npy")), got["adv_images_sample_index"])


def _single_process_bench(out_path, argv):
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        os.environ.pop(k, None)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    sys.argv = ["bench.py"] + list(argv)
    out = open(out_path, "w")
    os.dup2(out.fileno(), 1)
    os.dup2(out.fileno(), 2)
    import bench
    bench.main()
    sys.stdout.flush()


def _bench_line(tmp_path, argv, name):
    ctx = multiprocessing.get_context("forkserver")
    out = str(tmp_path / name)
    p = ctx.Process(target=_single_process_bench, args=(out, argv))
    p.start()
    p.join(timeout=420)
    if p.is_alive():
        p.kill()
        p.join()
        pytest.fail("bench.py did not finish within 420 s")
    text = open(out).read()
    assert p.exitcode == 0, text[-3000:]
    lines = [ln for ln in text.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, text[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_reports_the_headline_and_dumps_the_last_step(tmp_path):
    argv = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--model", "vlmo_tiny", "--batch", "4", "--pgd-steps", "6"]
    recs, dumps = [], []
    for run in ("a", "b"):
        recs.append(_bench_line(tmp_path, argv + ["--dump-outputs", str(tmp_path / run)], run + ".out"))
        dumps.append({f[:-4]: np.load(str(tmp_path / run / f)) for f in sorted(os.listdir(str(tmp_path / run)))})
    rec = recs[0]
    assert rec["metric"] == "adversarial_vqa_examples_per_sec" and rec["unit"] == "examples/s" and rec["dtype"] == "f32"
    assert rec["higher_is_better"] is True and rec["steps"] == 3 and rec["warmup"] == 1
    assert rec["ms_per_step"] > 0 and abs(rec["value"] - 4 / (rec["ms_per_step"] / 1e3)) <= 0.02 * rec["value"]
    assert not [k for k in AUXILIARY if k in rec], "auxiliary measurements belong to --full"
    a, b = dumps
    assert set(a) >= {"adv_images_sample", "adv_images_sum_per_sample", "adv_text_ids", "loss", "adv_answers", "success"}
    assert a["adv_images_sample"].shape == (4, 3, 32, 32) and a["adv_images_sample"].dtype == np.float32
    assert a["loss"].shape == (6,) and a["success"].shape == (4,)
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    assert np.isfinite(a["loss"]).all() and np.isfinite(a["adv_images_sum_per_sample"]).all()
    # the same arguments in two fresh processes: the same inputs, the same random start, the same outputs
    assert set(a) == set(b) and [k for k in a if not np.array_equal(a[k], b[k])] == []
    assert rec["attack_success_rate"] == recs[1]["attack_success_rate"]


def test_every_step_starts_from_the_same_seeded_state():
    """The random start draws from torch's default generators; ``seed_step`` fixes their state before each step."""
    import bench
    bench.seed_step(2)
    first = torch.empty(1000).uniform_(-1, 1)
    torch.empty(77).uniform_()                                  # whatever ran in between
    bench.seed_step(2)
    assert torch.equal(torch.empty(1000).uniform_(-1, 1), first)
    bench.seed_step(3)
    assert not torch.equal(torch.empty(1000).uniform_(-1, 1), first)
