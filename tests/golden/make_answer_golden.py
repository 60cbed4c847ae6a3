"""Generate ``tests/golden/answer_golden.json``: reference-produced cases for answer-string scoring
(``vqattack_amd/attack/answers.py``).

Build container only (needs ``/root/reference`` and ``transformers``).  Through ``tests/golden/refexec.py`` the reference's
statements are compiled from its source files, unmodified, and executed:

  * ``BertTokenizer.build_inputs_with_special_tokens`` / ``convert_tokens_to_string`` of ALBEF's own tokenizer class
    (``ALBEF_attack/models/tokenization_bert.py:240-265``) on a stub (the class does not import under the installed
    ``transformers``); the word pieces come from the library's ``BertTokenizer`` over the synthetic vocabulary of
    ``tests/golden/textworld.py`` (the class's parent machinery);
  * the answers / weights of ``vqa_dataset.__getitem__`` (``dataset/vqa_dataset.py:48-65``) and ``get_score``
    (``vlmo/utils/write_vqa.py:13-23``);
  * the alignment statements (``adv_attack.py:418-427``, ``vlmo_module.py:1733-1741``);
  * the decision statements (``adv_attack.py:726-730``, ``vlmo_module.py:2081-2086``).

Only inputs and outputs are stored.

    PYTHONDONTWRITEBYTECODE=1 python -m tests.golden.make_answer_golden
"""
import json
import os
import sys
from typing import List, Optional

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests.golden import refexec as rx  # noqa: E402
from tests.golden import textworld as tw  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
OUT_JSON = os.path.join(HERE, "answer_golden.json")
ALBEF_TOKENIZER = rx.REF + "/ALBEF_VQAttack/ALBEF_attack/models/tokenization_bert.py"
ALBEF_VQA_DATASET = rx.REF + "/ALBEF_VQAttack/ALBEF_attack/dataset/vqa_dataset.py"
VLMO_WRITE_VQA = rx.REF + "/VLMO_VQAttack/vlmo/utils/write_vqa.py"

ANSWER_LIST = ["red", "blue", "two", "cats", "playing frisbee", "dog's", "t-shirt", "yes", "kite", "3", "green",
               "cat", "red"]
ID2ANSWER = ["yes", "no", "red", "two", "cats", "playing frisbee", "kite", "blue", "3", "green", "red"]

# (question id, answers of the annotation, dataset, stored clean answer)
ALIGN_CASES = [
    (1, ["red"] * 6 + ["blue"] * 4, "vqa", "red"),                   # top weight
    (2, ["red"] * 6 + ["blue"] * 4, "vqa", "blue"),                  # present, lower weight
    (3, ["red"] * 5 + ["blue"] * 5, "vqa", "blue"),                  # tie at the top
    (4, ["red"] * 3 + ["blue"] * 3 + ["two"] * 3 + ["kite"], "vqa", "kite"),
    (5, ["red"] * 10, "vqa", "green"),                              # absent
    (6, "kite", "vg", "kite"),                                      # Visual Genome: one answer, weight 0.5
    (7, "kite", "vg", "red"),
    (8, ["two"] * 4 + ["3"] * 4 + ["yes", "no"], "vqa", "3"),        # VLMo: both at 4+ votes score 1.0
    (9, ["two"] * 5 + ["3"] * 4 + ["no"], "vqa", "3"),               # ALBEF: 0.5 vs 0.4; VLMo: tie at 1.0
    (10, ["zebra"] * 6 + ["red"] * 4, "vqa", "red"),                # VLMo: 'zebra' is not in id2answer
    (11, ["cats", "cats", "cat", "dog's", "cats", "cat", "cat", "cats", "t-shirt", "no"], "vqa", "cats"),
    (12, ["one", "two", "three"], "vqa", "three"),                   # three single votes
]

# (question id, victim's answer index after the attack, stored clean answer)
ALBEF_DECISIONS = [(1, 0, "red"), (2, 12, "red"), (3, 1, "red"), (4, 4, "playing frisbee"), (5, 7, "not in the list"),
                   (6, 11, "cats"), (7, 3, "cats")]
VLMO_DECISIONS = [(1, 2, "red"), (2, 10, "red"), (3, 0, "no"), (4, 5, "playing frisbee"), (5, 1, "absent"),
                  (6, 9, "green")]

# (flavor, question, {word index: substitute}) -> the adversarial string (update_adv_text's join) and the victim rows
STRING_CASES = [
    ("albef", "what color is the cat", {4: "dog"}),
    ("albef", "is the man holding a red umbrella near the table", {3: "flying", 8: "desk"}),
    ("albef", "how many people are in the picture", {}),
    ("albef", "what is the man's hat", {2: "woman"}),
    ("vlmo", "what color is the cat?", {4: "dog"}),
    ("vlmo", "is the man holding a red umbrella near the table?", {3: "flying", 8: "desk"}),
    ("vlmo", "how many people are in the picture", {1: "three"}),
    ("vlmo", "Which animal is on the  beach?", {1: "sport"}),
]


def _tokenizer_stub():
    methods, _ = rx.class_methods(ALBEF_TOKENIZER, "BertTokenizer",
                                  ["build_inputs_with_special_tokens", "convert_tokens_to_string"],
                                  extra_globals=dict(List=List, Optional=Optional))
    return rx.make_stub(methods, cls_token_id=tw.CLS, sep_token_id=tw.SEP)


def albef_rows(tok, stub, texts):
    """``tokenizer(texts, padding='longest')`` of ALBEF's class: prepare_for_model -> build_inputs_with_special_tokens ->
    pad to the longest with [PAD]."""
    rows = [stub.build_inputs_with_special_tokens(tok.convert_tokens_to_ids(tok.tokenize(t))) for t in texts]
    width = max(len(r) for r in rows)
    return [r + [tw.PAD] * (width - len(r)) for r in rows]


def section_rows(tok, stub, meta):
    meta["answer_list"] = ANSWER_LIST
    meta["albef_answer_rows"] = albef_rows(tok, stub, [a + "[SEP]" for a in ANSWER_LIST])   # adv_attack.py:396-397


def section_align(meta):
    getitem = rx.method_block(ALBEF_VQA_DATASET, "vqa_dataset", "__getitem__", 48, 65, ["ann"],
                              "if ann['dataset'] == 'vqa'", returns=["answers", "weights"])
    a_align = rx.method_block(rx.ALBEF_ATTACK, "Adv_attack", "evaluate", 418, 427, ["batch"], "ret = dict()")
    v_align = rx.method_block(rx.VLMO_MODULE, "VLMo", "test_step", 1733, 1741, ["batch"], "ret = dict()")
    get_score = rx.module_items(VLMO_WRITE_VQA, ["get_score"])["get_score"]
    ans2label = {a: i for i, a in enumerate(ID2ANSWER)}
    cases = []
    for qid, answers, dataset, stored in ALIGN_CASES:
        ann = {"question_id": qid, "answer": answers, "dataset": dataset}
        out = getitem(None, ann)
        # default collate of a batch of one: strings -> 1-tuples, floats -> float64 tensors
        batch = {"question_id": [qid], "answer": [(a,) for a in out["answers"]],
                 "weight": [torch.tensor([w], dtype=torch.float64) for w in out["weights"]]}
        albef = bool(a_align(rx.namespace(tcl_ans_table={str(qid): stored}), batch))
        # write_vqa.py:114-127: vote counts, answers outside ans2label dropped, get_score per kept answer
        count = {}
        for a in ([answers] if isinstance(answers, str) else answers):
            count[a] = count.get(a, 0) + 1
        kept = [a for a in count if a in ans2label]
        vbatch = {"qid": [qid], "vqa_answer": [kept], "vqa_scores": [[get_score(count[a]) for a in kept]]}
        vlmo = bool(v_align(rx.namespace(vlmo_ans_table={str(qid): stored}), vbatch)) if kept else False
        cases.append(dict(ann=ann, stored=stored, albef_answers=out["answers"], albef_weights=out["weights"],
                          vlmo_answers=kept, vlmo_scores=vbatch["vqa_scores"][0], albef=albef, vlmo=vlmo))
    meta["id2answer"] = ID2ANSWER
    meta["align_cases"] = cases


def section_decide(meta):
    a726 = rx.method_block(rx.ALBEF_ATTACK, "Adv_attack", "evaluate", 726, 726, ["data_loader", "topk_id", "pred"],
                           "ans_after_attack", returns=["ans_after_attack"])
    a727 = rx.method_block(rx.ALBEF_ATTACK, "Adv_attack", "evaluate", 727, 730, ["ans_after_attack", "qid_key"],
                           "if ans_after_attack")
    v2081 = rx.method_block(rx.VLMO_MODULE, "VLMo", "test_step", 2081, 2086, ["out_v", "qid_key", "old_alg"],
                            "if out_v['preds'][0]")
    loader = rx.namespace(dataset=rx.namespace(answer_list=ANSWER_LIST))
    albef = []
    for qid, after, stored in ALBEF_DECISIONS:
        self = rx.namespace(acc_list=[], tcl_ans_table={str(qid): stored})
        ans = a726(self, loader, torch.tensor([after, 0]), torch.tensor(0))["ans_after_attack"]
        a727(self, ans, str(qid))
        albef.append(dict(qid=qid, after=after, stored=stored, answer=ans, bit=self.acc_list[-1]))
    vlmo = []
    for qid, after, stored in VLMO_DECISIONS:
        self = rx.namespace(acc_list=[], count_kdd=0, vlmo_ans_table={str(qid): stored})
        logits = torch.zeros(1, len(ID2ANSWER))
        logits[0, after] = 1.0
        # objectives.py:822-824 with id2answer given (the reference reads it from a dill pickle there)
        out_v = {"qids": None, "preds": [ID2ANSWER[p.item()] for p in logits.argmax(dim=-1)]}
        v2081(self, out_v, str(qid), 0)
        vlmo.append(dict(qid=qid, after=after, stored=stored, answer=out_v["preds"][0], bit=self.acc_list[-1]))
    meta["albef_decisions"], meta["vlmo_decisions"] = albef, vlmo


def section_strings(tok, stub, meta):
    cases = []
    for flavor, question, subs in STRING_CASES:
        # update_adv_text: words of the (VLMo: '?'-stripped) lower-cased text, replaced, joined (adv_attack.py:267,324;
        # vlmo_module.py:1644,1702)
        words = (question.strip("?") if flavor == "vlmo" else question).replace("\n", "").lower().split(" ")
        for k, v in subs.items():
            words[k] = v
        text = stub.convert_tokens_to_string(words) + ("?" if flavor == "vlmo" else "")
        if flavor == "albef":
            rows = albef_rows(tok, stub, [text])[0]                                          # adv_attack.py:722
        else:
            rows = tok(text, padding="max_length", truncation=True, max_length=40)["input_ids"]  # vlmo_module.py:2069
        cases.append(dict(flavor=flavor, question=question, subs={str(k): v for k, v in subs.items()}, adv_text=text,
                          victim_ids=rows))
    meta["string_cases"] = cases


def main():
    vocab = tw.build_vocab()
    tok = tw.make_tokenizer(vocab)
    stub = _tokenizer_stub()
    meta = dict(vocab=vocab)
    section_rows(tok, stub, meta)
    section_align(meta)
    section_decide(meta)
    section_strings(tok, stub, meta)
    with open(OUT_JSON, "w") as fh:
        json.dump(meta, fh, indent=0)
    print("wrote", OUT_JSON)


if __name__ == "__main__":
    main()
