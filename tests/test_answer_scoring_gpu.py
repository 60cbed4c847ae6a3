"""Both entry points in the answer-string mode on files (``--answer_list`` / ``id2answer=``): ``acc_vqa``, the per-sample
bits and ``skipped_misaligned`` against an independent recomputation in the test -- the victim on the re-tokenised
adversarial string, then a string comparison with the clean table (``adv_attack.py:717-730``,
``vlmo_module.py:2063-2085``).  The clean table plants entries that differ from the victim's clean prediction and one
misaligned question."""
import json
import multiprocessing
import os

import numpy as np
import pytest
import torch

from tests.test_file_inputs import GOLD, _entry_run, _entry_vqa, _make_image_set, _vocab_file
from vqattack_amd.attack import dataset as ds
from vqattack_amd.attack.wordpiece import WordPiece

SEED = 5


@pytest.fixture(scope="module")
def text_meta():
    with open(os.path.join(GOLD, "text_golden.json")) as fh:
        return json.load(fh)


def _oracle_images(arrays, indices, device):
    from oracle import pil_resize
    rows = [pil_resize.to_tensor_normalize(pil_resize.resize_bicubic_u8(arrays[i], 32, 32)) for i in indices]
    return torch.from_numpy(np.ascontiguousarray(np.stack(rows))).to(device)


def _models(flavor, ckpt, vocab_path, answers, dev):
    from vqattack_amd.whitebox import checkpoint as ck
    if flavor == "albef":
        from vqattack_amd.attack.answers import albef_answer_ids
        from vqattack_amd.whitebox.albef import FrozenAlbef
        white = ck.albef_from_reference(torch.load(ckpt, weights_only=True), image_size=32, vqa_head=False).to(dev)
        black = FrozenAlbef.finetuned_from(white, seed=SEED + 1).to(dev)
        if answers is not None:
            black.set_answer_list(albef_answer_ids(answers, WordPiece(vocab_path)))
    else:
        from vqattack_amd.whitebox.vlmo import FrozenVlmo
        white = ck.vlmo_from_reference(torch.load(ckpt, weights_only=True), image_size=32, vqa_head=False).to(dev)
        black = FrozenVlmo.finetuned_from(white, seed=SEED + 1).to(dev)
    return white, black


def _child(target, argv, out):
    ctx = multiprocessing.get_context("forkserver")
    p = ctx.Process(target=target, args=(out, argv))
    p.start()
    p.join(timeout=600)
    if p.is_alive():
        p.kill()
        p.join()
        pytest.fail("the entry point did not finish within 600 s")
    text = open(out).read()
    assert p.exitcode == 0, text[-3000:]
    return text


@pytest.mark.gpu
@pytest.mark.parametrize("flavor", ["albef", "vlmo"])
def test_entry_points_score_answer_strings_like_the_reference(tmp_path, text_meta, flavor):
    from tests.golden import encoder_cases as ec
    n, text_len = 12, (12 if flavor == "albef" else 40)
    arrays = _make_image_set(str(tmp_path / "val2014"), n, seed=9, hw=(240, 320))
    body = [w for w in text_meta["vocab"][104:] if w.isalpha()]
    r = np.random.RandomState(4)
    qids = [900 + 7 * i for i in range(n)]
    questions = [" ".join(body[j] for j in r.randint(0, len(body), r.randint(3, 7))) + "?" for _ in range(n)]
    with open(os.path.join(GOLD, "encoder_golden.json")) as fh:
        rec = json.load(fh)[flavor + "_tiny"]
    ckpt = str(tmp_path / "pretrain.pth")
    if flavor == "albef":
        tied = set(rec["tied"])
        torch.save({"model": ec.seeded_state_dict([e for e in rec["listing"] if e[0] not in tied], rec["seed"])}, ckpt)
    else:
        torch.save({"state_dict": ec.seeded_state_dict(rec["listing"], rec["seed"])}, ckpt)
    # the white box's own MLM head proposes over the checkpoint's vocabulary: the vocab file covers all of it
    n_vocab = _models(flavor, ckpt, None, None, "cpu")[0].cfg.vocab
    vocab_path = _vocab_file(tmp_path, text_meta["vocab"] + ["zq{}".format(i) for i in range(len(text_meta["vocab"]),
                                                                                             n_vocab)])
    tok = WordPiece(vocab_path)
    dev = torch.device("cuda", 0)
    # the answer vocabulary: ALBEF a 13-answer list; VLMo one string per class of the victim's classifier
    if flavor == "albef":
        vocab = body[:13]
    else:
        n_cls = _models(flavor, ckpt, vocab_path, None, "cpu")[1].cfg.n_answers
        vocab = body[:13] + ["answer{}".format(i) for i in range(13, n_cls)]
    white, black = _models(flavor, ckpt, vocab_path, vocab, dev)
    # the victim's clean prediction (the rows today's path feeds it) decides the table
    qfile = str(tmp_path / "vqa_val.json")
    ann = [{"question_id": q, "image": "val2014/img{}.npy".format(i), "dataset": "vqa", "question": questions[i]}
           for i, q in enumerate(qids)]
    with open(qfile, "w") as fh:
        json.dump(ann, fh)
    src = ds.VqaFilePairs(qfile, str(tmp_path), flavor, text_len, 32, tokenizer=tok)
    with torch.no_grad():
        clean = black.vqa_answer(_oracle_images(arrays, range(n), dev), src.ids.to(dev), src.masks.to(dev)).tolist()
    planted, misaligned = {2, 5, 8, 11}, 1
    table = {}
    for i, a in enumerate(ann):
        stored = vocab[(clean[i] + 1) % 13] if i in planted else vocab[clean[i] % len(vocab)]
        other = vocab[(vocab.index(stored) + 3) % 13]
        a["answer"] = [stored] * 6 + [other] * 4 if i != misaligned else [other] * 7 + [stored] * 3
        table[str(a["question_id"])] = stored
    with open(qfile, "w") as fh:
        json.dump(ann, fh)
    tables_dir = str(tmp_path / "tables")
    os.makedirs(tables_dir)
    with open(os.path.join(tables_dir, flavor + "_ans_table.txt"), "w") as fh:
        json.dump(table, fh)
    with open(os.path.join(tables_dir, "right_part.txt"), "w") as fh:
        fh.write("".join("{}\n".format(q) for q in qids))
    vocab_file = str(tmp_path / ("answer_list.json" if flavor == "albef" else "id2answer.json"))
    with open(vocab_file, "w") as fh:
        json.dump(vocab if flavor == "albef" else {str(i): a for i, a in enumerate(vocab)}, fh)

    out = str(tmp_path / "entry.out")
    if flavor == "albef":
        import yaml
        cfg_path = str(tmp_path / "VQA.yaml")
        with open(cfg_path, "w") as fh:
            yaml.safe_dump(dict(image_res=32, batch_size_test=8, text_len=text_len, attack_dir="attack_dir",
                                vqa_root=str(tmp_path), test_file=[qfile], answer_list=vocab_file), fh)
        out_dir = str(tmp_path / "out")
        text = _child(_entry_vqa, ["--config", cfg_path, "--output_dir", out_dir, "--seed", str(SEED), "--vocab_file",
                                   vocab_path, "--tables_dir", tables_dir, "--checkpoint", ckpt, "--sim_threshold",
                                   "0.2"], out)
        strings_file, img_dir = os.path.join(out_dir, "adv_txt_dict_albef.txt"), os.path.join(out_dir, "attack_dir")
    else:
        out_dir = img_dir = str(tmp_path / "attack_dir_VLMO_BASE")
        text = _child(_entry_run, ["with", "image_size=32", "max_text_len=40", "per_gpu_batchsize=8",
                                   "questions=" + qfile, "image_root=" + str(tmp_path), "vocab_file=" + vocab_path,
                                   "tables_dir=" + tables_dir, "pretrain_path=" + ckpt, "attack_dir=" + out_dir,
                                   "seed=" + str(SEED), "sim_threshold=0.2", "id2answer=" + vocab_file], out)
        strings_file = os.path.join(out_dir, "adv_txt_dict_VLMO_BASE.txt")
    adv_rows = json.load(open(os.path.join(out_dir, "adv_txt.json")))
    strings = json.load(open(strings_file))
    bits = json.load(open(os.path.join(out_dir, "adv_success.json")))
    sweep = json.loads(next(ln for ln in text.splitlines() if ln.startswith("sweep ")).split(" ", 1)[1])
    acc = next(ln for ln in text.splitlines() if ln.startswith("acc_vqa")).split()
    scored = [q for i, q in enumerate(qids) if i != misaligned]
    assert sweep["skipped_misaligned"] == 1 and int(acc[2]) == len(scored)
    assert sorted(map(int, adv_rows)) == sorted(map(int, strings)) == sorted(map(int, bits)) == scored

    # the string file is the decode of adv_txt.json's rows (every question word is one vocabulary token here)
    for q in scored:
        row = adv_rows[str(q)]
        body_ids = row[1:row.index(tok.sep_id)]
        if flavor == "vlmo":
            body_ids = body_ids[:-1]                                   # the question's trailing '?'
        words = [tok.tokens[t][2:] if tok.tokens[t].startswith("##") else tok.tokens[t] for t in body_ids]
        assert strings[str(q)] == " ".join(words) + ("?" if flavor == "vlmo" else ""), q

    # independent recomputation: the victim on the re-tokenised string, then a string comparison
    want, planted_differ = {}, []
    with torch.no_grad():
        for q in scored:
            i = qids.index(q)
            img = torch.load(os.path.join(img_dir, "{}.pt".format(q))).to(dev)
            ids = [tok.cls_id] + [tok.vocab[p] for p in tok.tokenize(strings[str(q)])] + \
                ([tok.sep_id] if flavor == "vlmo" else [])
            mask = [1] * len(ids) + [0] * (text_len - len(ids))
            ids = torch.tensor([ids + [tok.pad_id] * (text_len - len(ids))], device=dev)
            after = int(black.vqa_answer(img, ids, torch.tensor([mask], device=dev))[0])
            want[str(q)] = int(vocab[after] != table[str(q)])
            if i in planted:           # the bit today's path records: index after the attack on the rows vs clean index
                rows = torch.tensor([adv_rows[str(q)]], device=dev)
                today = int(black.vqa_answer(img, rows, src.masks[i:i + 1].to(dev))[0])
                planted_differ.append(want[str(q)] != int(today != clean[i]))
                if today == clean[i]:
                    assert want[str(q)] == 1, q
    assert bits == want
    assert abs(float(acc[1]) - sum(want.values()) / len(want)) < 1e-6        # a float32 mean
    assert any(planted_differ), "no planted entry shows the answer-string decision differing from the index one"
