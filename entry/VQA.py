#!/usr/bin/env python
"""ALBEF-flavor entry point in the style of the reference's ``ALBEF_attack/VQA.py`` (argparse + yaml, :119-134).

    python entry/VQA.py --config entry/configs/VQA.yaml [--output_dir out] [--seed 42] [--n_samples 128]
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 entry/VQA.py --config ...

File inputs instead of the synthetic set: ``--questions`` (default: the yaml's ``test_file``), ``--image_root``
(``vqa_root``), ``--vocab_file``, ``--tables_dir`` (``right_part*.txt``, ``albef_ans_table*.txt``, ``chatgpt_all_5k*.txt``
...), ``--checkpoint`` / ``--checkpoint_vqa`` (the reference's "pretrain model path" / "fine-tune model path",
``adv_attack.py:83,96``).  See ``vqattack_amd/attack/dataset.py``.

``--answer_list`` (default: the yaml's ``answer_list``) turns on the reference's scoring: the victim ranks that answer
list and ``acc_vqa`` counts answer strings that differ from ``albef_ans_table`` (``vqattack_amd/attack/answers.py``);
``adv_txt_dict_albef.txt`` is written next to ``adv_txt.json``.
"""
import argparse
import os
import sys

import yaml

from _common import (answer_scoring, file_source, finish, init_distributed, load_checkpoint, mlm_proposer,
                     seed_everything)

import torch.distributed as dist  # noqa: E402  (after _common: it sets the HSA IPC mode before torch loads)

# flags of the reference's VQA.py (:120-131) that select things this entry point does not have (its model classes, the
# Pretrain.yaml of the white box, a launcher of its own): accepted so that its command lines run, and ignored
REFERENCE_ONLY = ("config_pre", "text_encoder", "text_decoder", "device", "evaluate", "world_size", "dist_url",
                  "distributed")


def parse(argv=None):
    """``(args, cfg)``: the parsed flags and the yaml with the entry point's defaults filled in (host only)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default=os.path.join(os.path.dirname(__file__), "configs", "VQA.yaml"))
    ap.add_argument("--output_dir", default="")
    ap.add_argument("--seed", default=42, type=int)
    ap.add_argument("--n_samples", default=None, type=int)
    ap.add_argument("--image_only", action="store_true", help="no word substitution (40-step image PGD)")
    ap.add_argument("--tiny", action="store_true", help="test-sized encoder")
    ap.add_argument("--dual_every", default=0, type=int,
                    help="every n-th synthetic sample's victim answer occurs in its paraphrase -> dual loss (old_alg == 0)")
    ap.add_argument("--mixed", action="store_true",
                    help="one bucket: batches mix schedules and loss modes (attack_mixed) instead of schedule-pure buckets")
    ap.add_argument("--questions", nargs="*", default=None, help="VQA annotation json file(s) (configs: test_file)")
    ap.add_argument("--image_root", default="", help="directory of the annotation's image paths (configs: vqa_root)")
    ap.add_argument("--vocab_file", default="", help="BERT vocab.txt (needed for textual questions / tables)")
    ap.add_argument("--tables_dir", default="", help="directory of the reference's in-tree *.txt tables")
    ap.add_argument("--checkpoint", default="", help="pre-trained ALBEF checkpoint -> white box (adv_attack.py:83)")
    ap.add_argument("--checkpoint_vqa", default="", help="VQA fine-tuned checkpoint -> victim (adv_attack.py:96)")
    ap.add_argument("--sim_threshold", default=0.95, type=float,
                    help="sentence-similarity floor of a substitution (adv_attack.py:303)")
    ap.add_argument("--decay_factor", default=None, type=float,
                    help="MI-FGSM momentum decay of the image attack (Dong et al. 2017); absent: plain PGD")
    ap.add_argument("--ti_kernel", default=None, type=int,
                    help="TI-FGSM Gaussian kernel length of the image attack (Dong et al. 2019; odd, 1..31); absent: off")
    ap.add_argument("--diversity_prob", default=None, type=float,
                    help="DI-FGSM probability of the random shrink-and-pad transform of the image attack (Xie et al. 2019; "
                         "the reference's input_diversity); absent: off")
    ap.add_argument("--di_shrink", default=32, type=int, help="DI-FGSM: new_h is drawn from [H - di_shrink, H)")
    ap.add_argument("--di_seed", default=None, type=int, help="DI-FGSM: seed of the geometry draws; absent: unseeded")
    ap.add_argument("--si_copies", default=None, type=int,
                    help="SI-FGSM number of scale copies 1, 1/2, ... of the image attack (Lin et al. 2020; 1..8); absent: off")
    ap.add_argument("--nesterov", action="store_true",
                    help="NI-FGSM: take gradients at the Nesterov look-ahead point (needs --decay_factor)")
    ap.add_argument("--vt_neighbors", default=None, type=int,
                    help="variance tuning (VMI / VNI-FGSM, Wang & He 2021): neighbours per gradient evaluation (1..64); "
                         "absent: off")
    ap.add_argument("--vt_beta", default=1.5, type=float,
                    help="variance tuning: neighbours are drawn from U[-vt_beta * eps, vt_beta * eps)")
    ap.add_argument("--vt_seed", default=None, type=int, help="variance tuning: seed of the device-side draws; absent: unseeded")
    ap.add_argument("--admix_images", default=None, type=int,
                    help="Admix (Wang et al. 2021): mixed groups x + admix_eta * x' of the scale copies per gradient "
                         "evaluation, x' another sample of the batch (1..8); absent: off")
    ap.add_argument("--admix_eta", default=0.2, type=float, help="Admix: the share of the partner image")
    ap.add_argument("--admix_seed", default=None, type=int, help="Admix: seed of the partner draws; absent: unseeded")
    ap.add_argument("--mlm_checkpoint", default="", help="BertForMaskedLM state dict -> candidate proposer (adv_attack.py:110)")
    ap.add_argument("--answer_list", default=None,
                    help="ALBEF answer_list json (configs: answer_list): the victim ranks it and acc_vqa compares answer "
                         "strings with albef_ans_table, like the reference (adv_attack.py:396-397,717-730)")
    for name in REFERENCE_ONLY:
        ap.add_argument("--" + name, default=None, help="accepted for the reference's command lines; ignored")
    args = ap.parse_args(argv)
    with open(args.config) as fh:
        cfg = yaml.safe_load(fh) or {}
    cfg.setdefault("text_len", 25)               # the reference's question length (adv_attack.py:113)
    cfg.setdefault("n_samples", 0)               # 0: every question of the source
    cfg.setdefault("batch_size_test", 64)
    cfg.setdefault("image_res", 384)
    if not args.questions and cfg.get("test_file"):
        args.questions = cfg["test_file"] if isinstance(cfg["test_file"], list) else [cfg["test_file"]]
    if args.answer_list is None:
        args.answer_list = cfg.get("answer_list") or ""
    if not args.image_root:
        args.image_root = cfg.get("vqa_root", "") or ""
    ignored = [n for n in REFERENCE_ONLY if getattr(args, n) is not None]
    if ignored:
        print("VQA.py: ignoring the reference's --{} (no counterpart here)".format(", --".join(ignored)), file=sys.stderr)
    if args.checkpoint_vqa and not args.answer_list:
        print("VQA.py: warning: --checkpoint_vqa without an answer list: acc_vqa is ranked over synthetic answers "
              "(give --answer_list or the yaml's answer_list)", file=sys.stderr)
    return args, cfg


def main():
    args, cfg = parse()
    rank, world, device = init_distributed()
    seed_everything(args.seed, rank)

    from vqattack_amd.attack.runner import AttackConfig
    from vqattack_amd.attack.sweep import run_sweep
    from vqattack_amd.whitebox.albef import AlbefAttackAdapters, FrozenAlbef, albef_base, albef_tiny
    from vqattack_amd.whitebox import checkpoint
    if args.checkpoint:
        white = checkpoint.albef_from_reference(load_checkpoint(args.checkpoint), image_size=cfg["image_res"],
                                                vqa_head=False).to(device)
        mcfg = white.cfg
        if args.checkpoint_vqa:
            black = checkpoint.albef_from_reference(load_checkpoint(args.checkpoint_vqa), image_size=cfg["image_res"],
                                                    vqa_head=True, strict=False).to(device)
        else:
            black = FrozenAlbef.finetuned_from(white, seed=args.seed + 1).to(device)
    else:
        mcfg = albef_tiny() if args.tiny else albef_base(image_size=cfg["image_res"])
        white = FrozenAlbef(mcfg, seed=args.seed).to(device)
        black = FrozenAlbef.finetuned_from(white, seed=args.seed + 1).to(device)
    if "k_test" in cfg:
        black.cfg.k_test = int(cfg["k_test"])              # rank_answer's k (configs/VQA.yaml: 128)
    out_dir = os.path.join(args.output_dir, cfg.get("attack_dir", "attack_dir")) if args.output_dir else None
    text_len = min(cfg["text_len"], 8 if args.tiny else 512)
    proposer, banned = mlm_proposer(args.mlm_checkpoint, args.vocab_file, device)
    source = None
    if args.questions:
        source = file_source("albef", args.questions, args.image_root, text_len,
                             mcfg.image_size, args.vocab_file, args.tables_dir, joint=not args.image_only)
    scoring = None
    if args.answer_list:
        from vqattack_amd.attack.answers import albef_answer_ids, load_answer_list
        if source is None:
            raise SystemExit("--answer_list scores file inputs: give --questions (or the yaml's test_file)")
        scoring = answer_scoring("albef", load_answer_list(args.answer_list), args.vocab_file, args.tables_dir)
        black.set_answer_list(albef_answer_ids(scoring.vocab, scoring.tokenizer))
    res = run_sweep("albef", white, black, AlbefAttackAdapters(white), args.n_samples or cfg["n_samples"],
                    cfg["batch_size_test"], mcfg.image_size, text_len, device,
                    rank, world, joint=not args.image_only, save_dir=out_dir, seed=args.seed,
                    max_words=4 if args.tiny else 12, dual_every=args.dual_every, mixed=args.mixed,
                    force_collective=dist.is_initialized(), source=source, mlm_logits_fn=proposer, banned_ids=banned,
                    config=AttackConfig(sim_threshold=args.sim_threshold, decay_factor=args.decay_factor,
                                        ti_kernel=args.ti_kernel, diversity_prob=args.diversity_prob,
                                        di_shrink=args.di_shrink, di_seed=args.di_seed, si_copies=args.si_copies,
                                        nesterov=args.nesterov, vt_neighbors=args.vt_neighbors, vt_beta=args.vt_beta,
                                        vt_seed=args.vt_seed, admix_images=args.admix_images,
                                        admix_eta=args.admix_eta, admix_seed=args.admix_seed),
                    scoring=scoring)
    finish(rank, world, res, os.path.join(args.output_dir, "adv_txt.json") if args.output_dir else None,
           os.path.join(args.output_dir, "adv_txt_dict_albef.txt") if args.output_dir and scoring else None)


if __name__ == "__main__":
    main()
