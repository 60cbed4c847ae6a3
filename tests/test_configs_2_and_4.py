"""BASELINE.json configs[2] (ALBEF, batch 256, 40 steps) and configs[4] (VLMO-large joint attack, batch 128) at their FULL
sizes in the driver-run GPU tests -- the thinnest part of the matrix after round 3 (ALBEF-base parity stopped at 8
steps, and no tracked test launched the ALBEF loss at the batch-256 row count or the 25-map launch at batch 128).

  * ALBEF-base, 384 px: the complete 40-step attack against the CPU oracle (reference-style batch-1 packing,
    ``adv_attack.py:119-126``; loop ``projected_gradient_descent.py:130-152``), same tolerances as the VLMO twin;
  * the loss launches of configs[2] at batch 256 -- image modality 13 x (256, 577, 768) = 5.9 GB per operand, text
    modality 13 x (256, 40, 768) with row weights -- and of configs[4] at batch 128 -- 25 x (128, 617, 1024) = 8.1 GB per
    operand -- through size-independent properties (the oracle would need hours): identity, orthogonality of the
    gradient, weighted rows, the multi-map launch against per-map launches, bitwise reproducible fold;
  * ``bench.py`` at the two configurations, a short budget, one well-formed line each.
"""
import copy
import json
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def test_albef_base_full_40_step_attack_matches_cpu_oracle():
    from oracle import cleverhans_cpu as oracle
    from oracle.adapters_ref import AlbefRefAdapters
    from tests.test_fullsize_parity import EPS, EPS_ITER, _compare, _cpu_threads, _inputs
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    from vqattack_amd.whitebox.albef import AlbefAttackAdapters, FrozenAlbef, albef_base
    steps = 40
    before = torch.get_num_threads()
    torch.set_num_threads(_cpu_threads())
    try:
        cpu_model = FrozenAlbef(albef_base(384, mlm_probability=0.0), seed=0)
        gpu_model = copy.deepcopy(cpu_model).to(DEV)
        ids, masks, img, eta = _inputs([7], 9, seed=8)
        attack = BatchedVQAttack(AlbefAttackAdapters(gpu_model), "albef", gpu_model.embedding_tables(),
                                 AttackConfig(budget=steps, sanity_checks=True))
        res = attack.attack_batch(img.to(DEV), ids.to(DEV), masks.to(DEV),
                                  torch.zeros_like(ids, dtype=torch.bool).to(DEV), init_eta=eta.to(DEV))
        ad = AlbefRefAdapters(cpu_model, ids, masks)
        tgt = ad.gen_ori_feats(img)
        with torch.enable_grad():
            adv, losses = oracle.projected_gradient_descent(
                ad.pgd_attack, img, EPS, EPS_ITER, steps, np.inf, clip_min=-1, clip_max=1,
                y=[tgt[0], tgt[1], None, None, None], ori_x=img, time=0, ls=1, flavor="albef", init_eta=eta)
    finally:
        torch.set_num_threads(before)
    same = _compare(res.adv_images[0].cpu(), adv[0].detach(), steps, full_attack=True)
    print("ALBEF-base 40 steps: {:.3%} of the pixels bit-identical to the CPU oracle".format(same))
    assert len(res.loss_lists[0]) == steps
    np.testing.assert_allclose(res.loss_lists[0], losses, rtol=1e-4)


def _loss_launch_properties(n_maps, batch, tokens, dim, weights):
    """One modality's loss launch at full size.  ``weights``: uint8 (batch, tokens) row weights or None."""
    from vqattack_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(n_maps * 1000 + batch)
    a = [torch.randn(batch, tokens, dim, device=DEV, generator=gen) for _ in range(n_maps)]
    b = [torch.randn(batch, tokens, dim, device=DEV, generator=gen) for _ in range(n_maps)]
    ws = ops.Workspace()
    slot, slot2 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    kw = dict(row_weight=weights, weight_period=batch) if weights is not None else {}
    wsum = float(weights.sum()) if weights is not None else float(batch * tokens)
    # (1) cos(a, a) = 1 on every live row: loss = -(sum of row weights) per map
    ops.neg_cos_rows_multi(a, a, slot, accumulate=False, want_grad=False, **kw)
    assert abs(float(slot) + n_maps * wsum) <= 2e-5 * n_maps * wsum
    # (2) ONE launch over all maps == per-map launches: gradients bit for bit (rows are independent), loss to fp32 sum order
    grads = ops.neg_cos_rows_multi(a, b, slot, accumulate=False, ws=ws, **kw)
    total = 0.0
    for k in (0, n_maps // 2, n_maps - 1):
        g1 = ops.neg_cos_rows(a[k], b[k], slot2, accumulate=False, **kw)
        assert torch.equal(g1, grads[k]), k
        # the gradient of a cosine is orthogonal to its argument; weight-0 rows are exactly zero
        assert float((g1 * a[k]).sum(-1).abs().max()) <= 2e-4
        if weights is not None:
            assert float(g1[weights == 0].abs().max()) == 0.0
            two = (weights == 2).nonzero()
            if two.numel():
                s, t = two[0].tolist()
                w1 = weights.clone()
                w1[s, t] = 1
                g_one = ops.neg_cos_rows(a[k], b[k], slot2, accumulate=False, row_weight=w1, weight_period=batch)
                assert torch.equal(g1[s, t], 2.0 * g_one[s, t])
        del g1
    for k in range(n_maps):
        ops.neg_cos_rows(a[k], b[k], slot2, accumulate=k > 0, want_grad=False, **kw)
    total = float(slot2)
    assert abs(float(slot) - total) <= 1e-5 * abs(total) + 1e-2
    # (3) the in-kernel fold is reproducible bit for bit, launch after launch (no float atomics)
    first = float(slot)
    for _ in range(2):
        ops.neg_cos_rows_multi(a, b, slot, accumulate=False, ws=ws, **kw)
        assert float(slot) == first
    # (4) antisymmetry in the target: -cos(a, -b) = +cos(a, b)
    ops.neg_cos_rows_multi(a, [-t for t in b[:2]] + b[2:], slot2, accumulate=False, want_grad=False, **kw)
    part = torch.zeros(1, device=DEV)
    ops.neg_cos_rows_multi(a[:2], b[:2], part, accumulate=False, want_grad=False, **kw)
    assert abs((float(slot2) + 2 * float(part)) - first) <= 1e-5 * abs(first) + 2e-2
    del a, b, grads, ws
    torch.cuda.empty_cache()


def test_albef_loss_launches_at_batch_256():
    """configs[2]: the two launches of one ALBEF feature-loss step at batch 256 -- image maps (13 x 256 x 577 x 768, no
    weights) and text maps (13 x 256 x 40 x 768, padded tokens weigh 0: ``AlbefAttackAdapters.set_text``)."""
    _loss_launch_properties(13, 256, 577, 768, None)
    r = np.random.RandomState(4)
    w = torch.zeros(256, 40, dtype=torch.uint8)
    for s in range(256):
        w[s, :2 + int(r.randint(4, 13))] = 1            # [CLS] + 4..12 words + [SEP]
    _loss_launch_properties(13, 256, 40, 768, w.to(DEV))


def test_vlmo_large_loss_launch_at_batch_128():
    """configs[4]: 25 maps of (128, 617, 1024) in ONE launch (24.3 GB of operands + gradient), VLMo row weights: [CLS]
    counts twice, padded text tokens not at all."""
    r = np.random.RandomState(5)
    w = torch.ones(128, 617, dtype=torch.uint8)
    for s in range(128):
        w[s, 2 + int(r.randint(4, 13)):40] = 0
    w[:, 0] = 2
    _loss_launch_properties(25, 128, 617, 1024, w.to(DEV))


@pytest.mark.parametrize("argv,model", [
    (["--model", "albef_base", "--batch", "256", "--pgd-steps", "2"], "albef_base"),
    (["--model", "vlmo_large", "--joint", "8", "--batch", "128", "--pgd-steps", "9"], "vlmo_large"),
], ids=["configs2-albef-b256", "configs4-vlmo-large-joint8-b128"])
def test_bench_runs_the_two_configurations_at_full_batch(argv, model, capsys, monkeypatch):
    """``python bench.py --model albef_base --batch 256`` / ``--model vlmo_large --joint 8 --batch 128`` with a short PGD
    budget (the full 40 steps take minutes): one well-formed line, the step kernel timed at the full batch."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "1", "--warmup", "0", "--full", "--no-cpu-baseline",
                                      "--no-b256"] + argv)
    for k in ("RANK", "WORLD_SIZE", "MASTER_ADDR", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    rec = json.loads(lines[0])
    batch = int(argv[argv.index("--batch") + 1])
    assert rec["metric"] == "adversarial_vqa_examples_per_sec" and rec["n_gpus"] == 1 and rec["value"] > 0
    assert rec["config"]["batch_per_gpu"] == batch and model in rec["config"]["workload"]
    roof = rec["roofline"]
    assert roof["algorithmic_bytes_per_launch"] == 16 * batch * 3 * 384 * 384 and 0 < roof["frac"] < 1
    assert rec["roofline_loss"]["launches"] >= 2 and 0 < rec["roofline_loss"]["frac"] < 1
    assert rec["roofline_attention"]["bound"] == "mfma"
    torch.cuda.empty_cache()


def test_vlmo_large_full_budget_joint_attack_matches_cpu_oracle():
    """configs[4] at the reference's FULL budget: VLMO-large (24 x 1024, 25 maps per loss launch), joint image + text attack
    with 2 substitutable words -- blocks [12, 12, 16] + 2 probe steps = 42 white-box gradient steps -- against the batch-1
    CPU oracle loop (``vlmo_module.py:1943-2055``).  Tolerances of a complete attack (tests/test_fullsize_parity.py).

    The oracle side (42 VLMO-large gradient steps on the host: 45 s of a GPU lease in round 4) is the committed fixture
    ``tests/golden/fullsize_vlmo_large_joint40.npz`` -- computed by ``tests/golden/make_fullsize_fixture.py`` in the build
    container, data only: adversarial image, substituted ids, loss trajectory, candidate proposals -- and only the product
    runs here.  ``VQA_LIVE_ORACLE=1`` also runs the oracle live and holds it against the fixture."""
    import os
    from tests.golden import make_fullsize_fixture as fx
    from tests.test_fullsize_parity import _compare
    from vqattack_amd.attack import text_update
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    from vqattack_amd.whitebox.vlmo import FrozenVlmo, VlmoAttackAdapters, vlmo_large
    case = fx.CASES["vlmo_large_joint40"]
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fullsize_vlmo_large_joint40.npz"))
    meta = json.loads(str(z["meta"]))
    assert meta["case"] == case, "the fixture was generated for another case definition: regenerate it"
    budget, words = case["budget"], len(case["att"])
    cpu_model = FrozenVlmo(vlmo_large(384), seed=case["model_seed"])
    gpu_model = copy.deepcopy(cpu_model).to(DEV)
    ids, masks, img, eta, att = fx.inputs_of(case)
    adapters = VlmoAttackAdapters(gpu_model)
    proposals = [[(int(p), [int(v) for v in vs]) for p, vs in row] for row in meta["proposals"]]
    on_device = text_update.propose_candidates(adapters.mlm_logits(ids.to(DEV), masks.to(DEV)), ids, att, threshold=0)
    assert [(int(p), [int(v) for v in vs]) for p, vs in on_device[0]] == proposals[0], \
        "the device's MLM candidate proposals differ from the ones the oracle fixture was computed with"
    sim = text_update.BagOfEmbeddingsSimilarity(seed=case["sim_seed"])
    attack = BatchedVQAttack(adapters, "vlmo", gpu_model.embedding_tables(),
                             AttackConfig(budget=budget, sanity_checks=True, sim_threshold=case["sim_threshold"]),
                             similarity_fn=sim)
    res = attack.attack_batch(img.to(DEV), ids.to(DEV), masks.to(DEV), att.to(DEV), init_eta=eta.to(DEV),
                              proposals=proposals)
    assert res.gradient_steps == budget + words
    adv, new_ids = torch.from_numpy(z["adv"]), torch.from_numpy(z["new_ids"])
    cuts = np.cumsum(z["block_lengths"])[:-1]
    losses = [b.tolist() for b in np.split(z["losses"], cuts)]
    assert [len(b) for b in losses] == [12, 12, 16]
    if os.environ.get("VQA_LIVE_ORACLE", "") not in ("", "0"):
        live_adv, live_ids, live_losses = fx.oracle_run(case, cpu_model, proposals)
        assert live_ids.tolist() == new_ids.tolist()
        _compare(live_adv[0].detach(), adv[0], budget + words, full_attack=True)
        print("live oracle vs fixture: {:.3%} of the pixels bit-identical".format(
            float((live_adv[0].detach() == adv[0]).float().mean())))
    assert res.adv_text_ids[0].cpu().tolist() == new_ids[0].tolist()
    same = _compare(res.adv_images[0].cpu(), adv[0], budget + words, full_attack=True)
    print("VLMO-large {} gradient steps: {:.3%} of the pixels bit-identical to the CPU oracle".format(budget + words, same))
    # the loss runs from -549 through 0 to +623 over a block: relative to the trajectory's scale, not to the value that
    # happens to be near the zero crossing (the two sign-PGD trajectories differ in 0.6 % of the pixels by then)
    scale = max(abs(v) for block in losses for v in block)
    for got, want in zip(res.loss_lists, losses):
        np.testing.assert_allclose(got, want, rtol=2e-4, atol=2e-4 * scale)
    del gpu_model, attack, adapters
    torch.cuda.empty_cache()


def test_albef_base_dual_loss_batch_matches_per_sample_oracle():
    """configs[2]'s white box with the reference's ``old_alg == 0`` blocks at full size: ALBEF-base, batch 2, 4 dual
    iterations (feature step without projection + MLM step through the real 30 522-word head on the fused text states,
    ``adv_attack.py:130-140,614-619``; loop ``projected_gradient_descent.py:153-189`` with the ALBEF copy's ``y`` slicing
    and ``bkp`` arguments), 2-d labels on one sample and 3-d labels (K = 2) on the other, against each sample's own
    batch-1 oracle loop."""
    from oracle import attack_loop
    from oracle.adapters_ref import AlbefRefAdapters
    from tests.test_fullsize_parity import _compare, _cpu_threads, _dual_tasks, _inputs, _sum_by_step
    from vqattack_amd.attack.runner import AttackConfig, BatchedVQAttack
    from vqattack_amd.whitebox.albef import AlbefAttackAdapters, FrozenAlbef, albef_base
    budget = 8
    before = torch.get_num_threads()
    torch.set_num_threads(_cpu_threads())
    try:
        cpu_model = FrozenAlbef(albef_base(384, mlm_probability=0.0), seed=0)
        gpu_model = copy.deepcopy(cpu_model).to(DEV)
        ids, masks, img, eta = _inputs([5, 7], 9, seed=12)
        tasks, oracle_tasks = _dual_tasks("albef", ids, None)
        attack = BatchedVQAttack(AlbefAttackAdapters(gpu_model), "albef", gpu_model.embedding_tables(),
                                 AttackConfig(budget=budget, sanity_checks=True))
        res = attack.attack_batch(img.to(DEV), ids.to(DEV), masks.to(DEV),
                                  torch.zeros_like(ids, dtype=torch.bool).to(DEV), init_eta=eta.to(DEV), dual=True,
                                  tasks=tasks)
        assert res.gradient_steps == budget and len(res.loss_lists[0]) == budget
        per_sample = []
        for s in range(2):
            n = int(masks[s].sum())
            adv, _, losses = attack_loop.attack_one(AlbefRefAdapters, cpu_model, "albef", img[s:s + 1], ids[s:s + 1, :n],
                                                    masks[s:s + 1, :n], None, None, init_eta=eta[s:s + 1], budget=budget,
                                                    task=oracle_tasks[s])
            _compare(res.adv_images[s].cpu(), adv[0].detach(), budget, full_attack=False)
            per_sample.append(losses[0])
    finally:
        torch.set_num_threads(before)
    np.testing.assert_allclose(res.loss_lists[0], _sum_by_step(per_sample), rtol=2e-4)
