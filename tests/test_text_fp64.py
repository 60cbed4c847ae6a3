"""Text scoring against float64 for what it feeds: a RANKING (``vqa_cand_dir_sim``) and a chain of THRESHOLD DECISIONS
(``vqa_greedy_accept``), on BERT-like tables with outlier channels and near-synonym rows (``tests/trained_stats.py``;
the caps on what may be left undecided are checked from float64 alone in ``test_trained_stats.py``).
"""
import numpy as np
import pytest
import torch

from tests import trained_stats as ts

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
PAIR_CAP, SAMPLE_CAP = 0.02, 0.05


@pytest.mark.parametrize("d", [768, 1024])
def test_cand_dir_sim_values_and_ranking_against_fp64(d):
    """Scores within 2x torch fp32 on the device + 4 * 2^-24 of the float64 restatement of the header's formula; every
    pair of candidates of one (sample, position) whose float64 scores differ by more than 4x the measured kernel error is
    ordered as in float64, and at most 2 % of the pairs are closer than that."""
    from vqattack_amd import ops
    cpu = ts.text_tables(d)
    ori, cand, syn = ts.text_candidates(cpu)
    tabs = {k: (t.to(DEV) if torch.is_tensor(t) else t) for k, t in cpu.items()}
    ori, cand = ori.to(DEV), cand.to(DEV)
    pos = torch.arange(ts.TEXT_LEN, device=DEV)[None].expand_as(ori)
    e_ori = ts.bert_embed(tabs, ori, pos, torch.float32).contiguous()         # the given fp32 e_ori
    got = ops.cand_dir_sim(tabs["word"], tabs["pos"], tabs["type_emb"], tabs["gamma"], tabs["beta"], tabs["ln_eps"],
                           e_ori, tabs["grad"], cand)
    s64, _ = ts.dir_sim(tabs, e_ori, cand, torch.float64)
    s32, _ = ts.dir_sim(tabs, e_ori, cand, torch.float32)
    ek, et = float((got.double() - s64).abs().max()), float((s32.double() - s64).abs().max())
    syn = syn.to(DEV)
    ek_syn = float((got.double() - s64)[syn].abs().max())
    gap = 4.0 * ek
    left, decided = ts.left_out_pairs(s64, gap, ts.TEXT_CANDS)
    print("FP64 cand_dir_sim D={}: kernel/torch max err {:.3g}/{:.3g} (near-synonyms {:.3g}); gap {:.3g}, pairs left out "
          "{:.4%}".format(d, ek, et, ek_syn, gap, left))
    assert ek <= 2.0 * et + 4.0 * U
    assert left <= PAIR_CAP
    g64, gk = s64.view(-1, ts.TEXT_CANDS), got.double().view(-1, ts.TEXT_CANDS)
    order64 = g64[:, :, None] > g64[:, None, :]
    order_k = gk[:, :, None] > gk[:, None, :]
    assert bool((order64 == order_k)[decided].all()), int((order64 != order_k)[decided].sum())


@pytest.mark.parametrize("threshold", ts.GREEDY_THRESHOLDS)
@pytest.mark.parametrize("e", [64, 512])
def test_greedy_accept_decisions_against_fp64(e, threshold):
    """Every sample whose float64 loop never came within 1e-5 of its threshold is accepted exactly as in float64 (ids
    and ranks); at most 5 % of the samples are closer.  Sample 0 is a decidable close call on the RISEN threshold; samples
    1 .. 8 hold an exact tie with it (a candidate that proposes the word already there), which `>` rejects."""
    from vqattack_amd import ops
    case = ts.greedy_case(e)
    want_id, want_rank, smallest, risen = ts.greedy_accept64(case, threshold)
    ori = case["ori"].to(DEV)
    cur = ori.clone()
    new_id, rank = ops.greedy_accept(case["cand"].to(DEV), case["scores"].to(DEV), ori, cur, case["table"].to(DEV),
                                     threshold)
    new_id, rank, cur = new_id.cpu().numpy(), rank.cpu().numpy(), cur.cpu().numpy()
    judged = smallest > ts.GREEDY_MARGIN
    left = 1.0 - float(judged.mean())
    n_acc = int((want_id >= 0).sum())
    print("FP64 greedy_accept E={} threshold={}: samples left out {:.2%}; {} acceptances; smallest judged margin {:.3g}; "
          "sample 0 misses the risen threshold by {:.3g}".format(e, threshold, left, n_acc, float(smallest[judged].min()),
                                                                min(risen[0])))
    assert left <= SAMPLE_CAP
    assert judged[0] and ts.GREEDY_MARGIN < min(risen[0]) < 1e-3
    assert np.array_equal(new_id[judged], want_id[judged])
    assert np.array_equal(rank[judged], want_rank[judged])
    final = np.where(want_id >= 0, want_id, case["ori"].numpy())
    assert np.array_equal(cur[judged], final[judged])
    assert n_acc >= ts.GREEDY_B // 2 or threshold > 0.9
