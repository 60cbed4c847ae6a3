"""Answer-string scoring: the reference's success decision over its answer vocabulary (opt-in, host code).

The reference counts a sample as attacked when the victim's answer STRING after the attack differs from the answer
stored for that question in its clean table:

  * ALBEF: ``answer_list[topk_id[pred]] != tcl_ans_table[qid]`` (``adv_attack.py:717-730``), the victim ranking the
    ``answer_list`` json (``vqa_dataset.py:24``) tokenised as ``tokenizer(answer + '[SEP]', padding='longest')``
    (``adv_attack.py:396-397``);
  * VLMo: ``id2answer[argmax] != vlmo_ans_table[qid]`` (``vlmo_module.py:2063-2085``, ``objectives.py:812-829``).

It attacks a question only when that stored answer is among the annotation's answers with the top weight
(``adv_attack.py:418-427``, ``vlmo_module.py:1733-1741``), and it feeds the victim the adversarial question as a STRING
(``adv_text``, built by ``update_adv_text``, ``adv_attack.py:265-324`` / ``vlmo_module.py:1642-1702``), re-tokenised
(``adv_attack.py:722``; ``vlmo_module.py:2069-2077``).  This module restates those pieces; ``AnswerScoring`` bundles
them for ``run_sweep(scoring=...)``.  ``tests/golden/answer_golden.json`` pins them against the reference's statements.
"""
import json

import torch

from .wordpiece import convert_tokens_to_string

# what a user runs once, where the reference's environment is installed, to turn its dill-pickled id2answer.txt
# (objectives.py:818-820) into the JSON this module reads: a pickle is never loaded here
ID2ANSWER_EXPORT = ("python -c \"import dill, json; d = dill.load(open('id2answer.txt', 'rb')); "
                    "json.dump(d if isinstance(d, (list, dict)) else list(d), open('id2answer.json', 'w'))\"")


def _read_json(path, what):
    with open(path, "rb") as fh:
        raw = fh.read()
    try:
        return json.loads(raw.decode("utf-8"))
    except (UnicodeDecodeError, ValueError):
        hint = (" The reference's id2answer.txt is a dill pickle, which is never loaded here; export it to JSON once "
                "with:\n  " + ID2ANSWER_EXPORT) if what == "id2answer" else ""
        raise ValueError("{}: the {} file is not JSON.{}".format(path, what, hint)) from None


def load_answer_list(path):
    """ALBEF's ``answer_list`` json: a list of answer strings (``vqa_dataset.py:24``)."""
    obj = _read_json(path, "answer_list")
    if not isinstance(obj, list) or not all(isinstance(a, str) for a in obj):
        raise ValueError("{}: expected a JSON list of answer strings".format(path))
    return obj


def load_id2answer(path):
    """VLMo's ``id2answer``: a JSON list of answer strings, or a ``{id: answer}`` object whose ids are 0..n-1."""
    obj = _read_json(path, "id2answer")
    if isinstance(obj, dict):
        try:
            keys = sorted(obj, key=int)
        except ValueError:
            raise ValueError("{}: the keys of the id2answer object are not integers".format(path)) from None
        if [int(k) for k in keys] != list(range(len(keys))):
            raise ValueError("{}: the ids of the id2answer object are not 0..{}".format(path, len(keys) - 1))
        obj = [obj[k] for k in keys]
    if not isinstance(obj, list) or not all(isinstance(a, str) for a in obj):
        raise ValueError("{}: expected a JSON list of answer strings or an {{id: answer}} object".format(path))
    return obj


def albef_answer_ids(answers, tokenizer):
    """``tokenizer([a + '[SEP]' for a in answers], padding='longest')`` of ALBEF's own ``BertTokenizer``
    (``adv_attack.py:396-397``): one sequence is ``[CLS] ids`` with no trailing ``[SEP]`` (``tokenization_bert.py:262``)
    and the literal ``[SEP]`` in the text stays one token -> rows ``[CLS] pieces [SEP] pad...`` (n, L) int64.  The
    decoder starts from ``answer_ids[0, 0]`` = ``[CLS]`` (``model_vqa.py:152``)."""
    rows = [[tokenizer.cls_id] + [tokenizer.vocab[p] for p in tokenizer.tokenize(a + "[SEP]")] for a in answers]
    width = max((len(r) for r in rows), default=0)
    return torch.tensor([r + [tokenizer.pad_id] * (width - len(r)) for r in rows],
                        dtype=torch.int64).reshape(len(rows), width)


def _vqa_score(count):
    """``get_score`` of ``vlmo/utils/write_vqa.py:13-23``."""
    return 0.0 if count == 0 else 0.3 if count == 1 else 0.6 if count == 2 else 0.9 if count == 3 else 1.0


def answer_weights(flavor, ann, vocab=None):
    """The (answers, weights) the reference's data pipeline attaches to an annotation entry.

    ALBEF (``vqa_dataset.py:48-62``): for ``dataset == 'vqa'`` every distinct answer weighs ``count / len(answers)``
    (accumulated as repeated ``1 / len`` additions, like there); ``'vg'``: ``[answer]`` with weight 0.5.
    VLMo (``write_vqa.py:114-127``): every distinct answer that is in the answer vocabulary (``vocab``; None = all) gets
    ``get_score(count)``; answers outside the vocabulary do not survive into ``vqa_answer``."""
    answers = ann.get("answer")
    if answers is None:
        raise ValueError("question {}: the annotation has no 'answer' field".format(ann.get("question_id")))
    if flavor == "albef":
        dataset = ann.get("dataset") or "vqa"
        if dataset == "vg":
            return [answers], [0.5]
        if dataset != "vqa":
            raise ValueError("question {}: unknown dataset {!r}".format(ann.get("question_id"), dataset))
        weight = {}
        for a in answers:
            weight[a] = weight.get(a, 0.0) + 1 / len(answers)
        return list(weight), list(weight.values())
    answers = [answers] if isinstance(answers, str) else answers
    count = {}
    for a in answers:
        count[a] = count.get(a, 0) + 1
    vocab = set(vocab) if vocab is not None else None
    kept = [a for a in count if vocab is None or a in vocab]
    return kept, [_vqa_score(count[a]) for a in kept]


def aligned(flavor, ann, stored, vocab=None):
    """The reference's alignment skip (``adv_attack.py:418-427``, ``vlmo_module.py:1733-1741``): a question is attacked
    only when its stored clean answer is among the annotation's answers AND carries the maximum weight / score (ties at
    the maximum are aligned: VLMo answers with four or more votes all score 1.0).  ``vocab``: VLMo's id2answer."""
    answers, weights = answer_weights(flavor, ann, vocab)
    if stored not in answers:
        return False
    return weights[answers.index(stored)] == max(weights)


def adv_words_string(flavor, words, pieces, body, tokenizer):
    """The reference's ``adv_text`` after ``update_adv_text``: the question's whitespace words, each attacked word
    replaced by its substitute, joined by ``convert_tokens_to_string`` (``adv_attack.py:267,324``); VLMo works on
    ``text.strip('?')`` and appends ``'?'`` (``vlmo_module.py:1644,1702``).

    ``words`` / ``pieces``: the source's words of the question and each word's piece ids (``VqaFilePairs.word_pieces``;
    a word is None for a pre-tokenised entry); ``body``: the adversarial row's ids between ``[CLS]`` and ``[SEP]``.  A
    word whose pieces are unchanged keeps its text; a changed word is its decoded pieces; words cut off by the row's
    length limit are never attacked and keep their text."""
    out, at = [], 0
    for w, p in zip(words, pieces):
        p = tuple(p)
        got = tuple(body[at:at + len(p)]) if at + len(p) <= len(body) else p
        out.append(w if (got == p and w is not None) else tokenizer.decode_word(got))
        at += len(p)
    s = convert_tokens_to_string(out)
    return s + "?" if flavor == "vlmo" else s


def victim_input(flavor, text, tokenizer, text_len):
    """The row the victim reads after the attack, from the adversarial string: ALBEF's tokenizer on one sequence,
    ``[CLS] pieces`` with no ``[SEP]`` (``adv_attack.py:722``); VLMo ``[CLS] pieces [SEP]`` padded / truncated to
    ``max_length`` (``vlmo_module.py:2069-2077``: 40 = the model's ``max_text_len``).  Returns (ids, mask) lists of
    ``text_len`` (ALBEF rows longer than that are cut: the row is the victim's text width)."""
    ids = [tokenizer.vocab[p] for p in tokenizer.tokenize(text)]
    if flavor == "albef":
        ids = ([tokenizer.cls_id] + ids)[:text_len]
    else:
        ids = [tokenizer.cls_id] + ids[:text_len - 2] + [tokenizer.sep_id]
    return ids + [tokenizer.pad_id] * (text_len - len(ids)), [1] * len(ids) + [0] * (text_len - len(ids))


class AnswerScoring:
    """What ``run_sweep(scoring=...)`` needs to score like the reference: the answer vocabulary (ALBEF ``answer_list`` /
    VLMo ``id2answer``), the clean-answer table (``{qid: answer}``, ``albef_ans_table`` / ``vlmo_ans_table``) and the
    tokenizer (``wordpiece.WordPiece``)."""

    def __init__(self, flavor, vocab, clean_answers, tokenizer):
        if flavor not in ("albef", "vlmo"):
            raise ValueError(flavor)
        if tokenizer is None:
            raise ValueError("answer-string scoring needs a tokenizer (vocab file)")
        if not clean_answers:
            raise ValueError("answer-string scoring needs the clean-answer table ({}_ans_table*.txt)".format(flavor))
        self.flavor, self.vocab, self.table, self.tokenizer = flavor, list(vocab), dict(clean_answers), tokenizer
        self._first = {}
        for i, a in enumerate(self.vocab):
            self._first.setdefault(a, i)
        # vocabulary index -> index of the first entry with the same string: equal strings compare equal on the device
        self.canonical = torch.tensor([self._first[a] for a in self.vocab], dtype=torch.int64)

    def stored(self, qid):
        key = str(qid)
        if key not in self.table:
            raise KeyError("question {} has no entry in the clean-answer table".format(qid))
        return self.table[key]

    def is_aligned(self, ann):
        return aligned(self.flavor, ann, self.stored(ann["question_id"]), self.vocab if self.flavor == "vlmo" else None)

    def table_index(self, qids):
        """(n,) int64: the vocabulary index of each question's stored answer, -1 when the string is not in the
        vocabulary (every prediction differs from it: always a success)."""
        return torch.tensor([self._first.get(self.stored(q), -1) for q in qids], dtype=torch.int64)

    def decide(self, after, table_index):
        """``vocab[after] != table[qid]`` as a gather and compare on ``after``'s device."""
        return self.canonical.to(after.device)[after] != table_index.to(after.device)

    def adv_string(self, source, i, row):
        """``adv_text`` of sample ``i`` of a ``VqaFilePairs`` whose adversarial row is ``row`` (list of ids)."""
        if source.questions[i] is not None and not bool(source.attackable[i].any()):
            # no attackable word: update_adv_text never runs and adv_text stays the question the dataset hands over
            # (adv_attack.py:588 after pre_question, vlmo_module.py:1938 as written)
            if self.flavor == "albef":
                from .dataset import pre_question
                return pre_question(source.questions[i])
            return source.questions[i]
        body = row[1:1 + int(source.masks[i].sum()) - 2]
        words, pieces = source.word_pieces[i]
        return adv_words_string(self.flavor, words, pieces, body, self.tokenizer)
