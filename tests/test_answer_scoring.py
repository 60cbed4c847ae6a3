"""Answer-string scoring (``vqattack_amd/attack/answers.py``) against the reference-executed cases of
``tests/golden/answer_golden.json`` (``make_answer_golden.py``) and ``text_golden.json``'s ``update_adv_text`` rounds;
the vocabulary loaders; the ALBEF entry point's yaml / flag handling.  CPU only."""
import argparse
import json
import os
import pickle
import subprocess
import sys

import pytest
import torch

from vqattack_amd.attack import answers as an
from vqattack_amd.attack.wordpiece import WordPiece

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def gold():
    with open(os.path.join(GOLD, "answer_golden.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def tok(gold, tmp_path_factory):
    p = tmp_path_factory.mktemp("vocab") / "vocab.txt"
    p.write_text("\n".join(gold["vocab"]) + "\n")
    return WordPiece(str(p))


def test_special_tokens_inside_text_stay_whole(tok):
    assert tok.tokenize("red[SEP]") == ["red", "[SEP]"]
    assert tok.tokenize("playing frisbee[SEP]") == ["playing", "frisbee", "[SEP]"]
    assert tok.tokenize("the [MASK] is blue") == ["the", "[MASK]", "is", "blue"]


def test_albef_answer_rows_equal_the_references_tokenizer(gold, tok):
    rows = an.albef_answer_ids(gold["answer_list"], tok)
    assert rows.dtype == torch.int64 and rows.tolist() == gold["albef_answer_rows"]
    assert int(rows[0, 0]) == tok.cls_id                     # the decoder's start id (model_vqa.py:152)


def test_alignment_flags_equal_the_references(gold):
    assert sum(c["albef"] for c in gold["align_cases"]) not in (0, len(gold["align_cases"]))
    assert any(c["albef"] != c["vlmo"] for c in gold["align_cases"])
    for c in gold["align_cases"]:
        qid = c["ann"]["question_id"]
        answers, weights = an.answer_weights("albef", c["ann"])
        assert answers == c["albef_answers"] and weights == c["albef_weights"], qid
        answers, scores = an.answer_weights("vlmo", c["ann"], gold["id2answer"])
        assert answers == c["vlmo_answers"] and scores == c["vlmo_scores"], qid
        assert an.aligned("albef", c["ann"], c["stored"]) == c["albef"], qid
        assert an.aligned("vlmo", c["ann"], c["stored"], gold["id2answer"]) == c["vlmo"], qid


@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_decision_bits_equal_the_references(gold, tok, flavor):
    vocab = gold["answer_list"] if flavor == "albef" else gold["id2answer"]
    cases = gold[flavor + "_decisions"]
    table = {str(c["qid"]): c["stored"] for c in cases}
    sc = an.AnswerScoring(flavor, vocab, table, tok)
    after = torch.tensor([c["after"] for c in cases])
    bits = sc.decide(after, sc.table_index([c["qid"] for c in cases]))
    assert bits.tolist() == [bool(c["bit"]) for c in cases]
    assert [vocab[c["after"]] for c in cases] == [c["answer"] for c in cases]
    assert {0, 1} <= {c["bit"] for c in cases}


def test_adversarial_strings_and_victim_rows_equal_the_references(gold, tok):
    for c in gold["string_cases"]:
        flavor, q = c["flavor"], c["question"]
        words, pieces = tok.words(q.strip("?") if flavor == "vlmo" else q)
        body = []
        for k, p in enumerate(pieces):
            body += [tok.vocab[c["subs"][str(k)]]] if str(k) in c["subs"] else list(p)
        s = an.adv_words_string(flavor, words, pieces, body, tok)
        assert s == c["adv_text"], c
        ids, mask = an.victim_input(flavor, s, tok, 40)
        want = c["victim_ids"]
        if flavor == "albef":                                # [CLS] pieces, no [SEP]; padded here to the row width
            assert ids[:len(want)] == want and set(ids[len(want):]) <= {tok.pad_id} and sum(mask) == len(want), c
        else:
            assert ids == want and mask == [int(t != tok.pad_id) for t in want], c


def test_adversarial_strings_equal_update_adv_text(tmp_path):
    """The reference's own ``update_adv_text`` outputs (text_golden.json ``upd_cases``): the string rebuilt from the
    question's words and the adversarial row equals the string the reference holds in ``adv_text``."""
    with open(os.path.join(GOLD, "text_golden.json")) as fh:
        meta = json.load(fh)
    p = tmp_path / "vocab.txt"
    p.write_text("\n".join(meta["vocab"]) + "\n")
    wp = WordPiece(str(p))
    n = 0
    for case in meta["upd_cases"]:
        flavor, q = case["flavor"], case["question"]
        words, pieces = wp.words(q.strip("?") if flavor == "vlmo" else q)
        for rnd in case["rounds"]:
            ids = rnd["new_ids"]
            body = ids[1:ids.index(wp.sep_id)]
            assert an.adv_words_string(flavor, words, pieces, body, wp) == rnd["adv_text_out"], rnd["key"]
            n += 1
    assert n >= 6


def test_vocabulary_files(tmp_path):
    lst, obj = tmp_path / "a.json", tmp_path / "b.json"
    lst.write_text(json.dumps(["yes", "no"]))
    obj.write_text(json.dumps({"1": "no", "0": "yes"}))
    assert an.load_answer_list(str(lst)) == ["yes", "no"]
    assert an.load_id2answer(str(lst)) == an.load_id2answer(str(obj)) == ["yes", "no"]
    gap = tmp_path / "c.json"
    gap.write_text(json.dumps({"0": "yes", "2": "no"}))
    with pytest.raises(ValueError):
        an.load_id2answer(str(gap))


def test_a_pickled_id2answer_is_refused_with_the_export_hint(tmp_path):
    p = tmp_path / "id2answer.txt"
    p.write_bytes(pickle.dumps({0: "yes", 1: "no"}))
    with pytest.raises(ValueError) as e:
        an.load_id2answer(str(p))
    assert "dill.load" in str(e.value) and "json.dump" in str(e.value)


def test_table_strings_outside_the_vocabulary_always_count_as_success(tok):
    sc = an.AnswerScoring("vlmo", ["yes", "no", "yes"], {"1": "yes", "2": "maybe"}, tok)
    assert sc.table_index([1, 2]).tolist() == [0, -1]
    # equal strings at different indices compare equal
    assert sc.decide(torch.tensor([2, 0]), sc.table_index([1, 2])).tolist() == [False, True]


_ENTRY_SCRIPT = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/entry')
import VQA
args, cfg = VQA.parse(sys.argv[3:])
print(json.dumps(dict(questions=args.questions, answer_list=args.answer_list, image_root=args.image_root,
                      text_len=cfg['text_len'], n_samples=cfg['n_samples'], k_test=cfg.get('k_test'))))
from _common import load_checkpoint
try:
    load_checkpoint(sys.argv[2])
except SystemExit as e:
    print('REFUSED', str(e).replace('\n', ' '))
"""


def test_albef_entry_accepts_the_references_yaml_keys_and_flags(tmp_path):
    import yaml
    # the key set of the reference's configs/VQA.yaml (no text_len, no n_samples)
    cfg = {"train_file": ["vqa_train.json", "vqa_val.json", "vg_qa.json"], "test_file": ["vqa_val.json"],
           "answer_list": "answer_list.json", "vqa_root": "VQAv2", "vg_root": "VG_100K_2", "image_res": 480,
           "batch_size_train": 1, "batch_size_test": 1, "k_test": 128, "alpha": 0.4, "distill": True,
           "warm_up": True, "eos": "[SEP]", "bert_config": "configs/config_bert.json",
           "optimizer": {"opt": "adamW", "lr": 2e-5, "weight_decay": 0.02},
           "schedular": {"sched": "cosine", "lr": 2e-5, "epochs": 8, "min_lr": 1e-6, "decay_rate": 1,
                         "warmup_lr": 1e-5, "warmup_epochs": 4, "cooldown_epochs": 0}}
    path = tmp_path / "VQA.yaml"
    path.write_text(yaml.safe_dump(cfg))
    ckpt = tmp_path / "full.pth"
    torch.save({"model": {"w": torch.zeros(2)}, "config": argparse.Namespace(lr=1e-4)}, str(ckpt))
    argv = ["--config", str(path), "--config_pre", "./configs/Pretrain.yaml", "--checkpoint", "", "--output_dir",
            "output/vqa", "--evaluate", "True", "--text_encoder", "bert-base-uncased", "--text_decoder",
            "bert-base-uncased", "--device", "cuda", "--seed", "42", "--world_size", "1", "--dist_url", "env://",
            "--distributed", "False"]
    out = subprocess.run([sys.executable, "-c", _ENTRY_SCRIPT, ROOT, str(ckpt)] + argv, capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = out.stdout.splitlines()
    got = json.loads(lines[0])
    assert got == dict(questions=["vqa_val.json"], answer_list="answer_list.json", image_root="VQAv2", text_len=25,
                       n_samples=0, k_test=128)
    ignored = [ln for ln in out.stderr.splitlines() if "ignoring the reference's" in ln]
    assert len(ignored) == 1 and all("--" + n in ignored[0] for n in ("config_pre", "text_encoder", "text_decoder",
                                                                    "device", "evaluate", "world_size", "dist_url",
                                                                    "distributed"))
    assert lines[1].startswith("REFUSED") and "tensors_only.pth" in lines[1] and str(ckpt) in lines[1]
