"""ALBEF's answer ranking on the graph-free path (``FrozenAlbef.fused_rank``): ``_fused.decode_candidates`` + the LM loss
from ``ops.gemm_lse`` against the eager ``_decode`` + ``F.cross_entropy`` form and against the same victim in float64.

Reference: a ``.double()`` copy of the victim run eagerly on the device (its attention through a float64 softmax written
out here: the HIP attention is fp32 only).  Rule: the fused path's maximum error against it is at most twice the eager
fp32 path's own, or 1e-4 relative, whichever is larger -- the two paths use different GEMMs (bf16x6 / the library).
Compared per ANSWER ID, not per rank: near ties may swap ranks.
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
IDS = [[101, 5, 6, 7, 102, 0, 0, 0], [101, 8, 9, 102, 0, 0, 0, 0], [101, 3, 4, 5, 6, 7, 102, 0]]


def _perturb_layernorms(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for mod in model.modules():
            if isinstance(mod, torch.nn.LayerNorm):
                mod.weight.add_((torch.randn(mod.weight.shape, generator=g) * 0.2).to(mod.weight.device))
                mod.bias.add_((torch.randn(mod.bias.shape, generator=g) * 0.1).to(mod.bias.device))


def _victim(cfg, seed):
    from vqattack_amd.whitebox.albef import FrozenAlbef
    model = FrozenAlbef(cfg, seed=seed, vqa_head=True).to(DEV)
    _perturb_layernorms(model, seed + 7)
    with torch.no_grad():                                    # a decoder bias away from zero: the LSE epilogue adds it
        model.dec_bias.copy_(0.5 * torch.randn(cfg.vocab, generator=torch.Generator().manual_seed(seed + 9)).to(DEV))
    return model


def _question(b, t, d, seed, ragged=True):
    g = torch.Generator(device=DEV).manual_seed(seed)
    states = torch.randn(b, t, d, device=DEV, generator=g)
    masks = torch.ones(b, t, dtype=torch.long, device=DEV)
    if ragged:
        for i in range(b):
            masks[i, t - (2 * i + 1) % (t - 1):] = 0             # a different number of padded positions per sample
    return states, masks


@pytest.fixture(scope="module")
def small():
    from vqattack_amd.whitebox.albef import AlbefConfig
    cfg = AlbefConfig(dim=128, vit_depth=1, bert_depth=1, fusion_layer=0, heads=2, patch=8, image_size=32, n_answers=13,
                      decoder_depth=2, k_test=5, mlm_probability=0.0, vocab=1500, max_position=32)
    return _victim(cfg, 4)


@pytest.fixture(scope="module")
def base():
    """Base width, one decoder layer, the full vocabulary: 30522 -> 30720 columns, all 480 column blocks."""
    from vqattack_amd.whitebox.albef import AlbefConfig
    cfg = AlbefConfig(dim=768, vit_depth=1, bert_depth=1, fusion_layer=0, heads=12, n_answers=5, decoder_depth=1, k_test=3,
                      mlm_probability=0.0, vocab=30522, max_position=32)
    return _victim(cfg, 3)


def _mha64(q, k, v, bias=None):
    """softmax(q k^T / sqrt(d) + bias) v on (B, S, H, d) operands, in the operands' dtype."""
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) * q.shape[-1] ** -0.5
    if bias is not None:
        s = s + bias.to(s.dtype)
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, dim=-1), v)


def _rank(model, states, masks, fused):
    model.fused_rank = fused
    try:
        ids, probs, ll = model.rank_answer(states, masks, want_log_probs=True)
    finally:
        model.fused_rank = False
    return ids, probs, ll


def _reference(model, states, masks, monkeypatch):
    from vqattack_amd.whitebox import albef
    ref = copy.deepcopy(model).double()
    with monkeypatch.context() as mp:
        mp.setattr(albef, "mha", _mha64)
        return _rank(ref, states.double(), masks, False)


def _by_answer(ids, values, ref_ids, ref_values):
    """max |value - reference| over the answer ids both rankings hold, per question; (error, max |reference|, pairs)."""
    err, top, pairs = 0.0, 0.0, 0
    for i in range(ids.shape[0]):
        mine = {int(a): float(x) for a, x in zip(ids[i], values[i])}
        for a, x in zip(ref_ids[i], ref_values[i]):
            if int(a) in mine:
                err, top, pairs = max(err, abs(mine[int(a)] - float(x))), max(top, abs(float(x))), pairs + 1
    return err, top, pairs


def _check_against_fp64(model, b, t, seed, monkeypatch, label):
    states, masks = _question(b, t, model.cfg.dim, seed)
    fused, eager = _rank(model, states, masks, True), _rank(model, states, masks, False)
    ref = _reference(model, states, masks, monkeypatch)
    # the first pass is the same code on both paths: the same candidates
    assert [sorted(r.tolist()) for r in fused[0]] == [sorted(r.tolist()) for r in eager[0]]
    same_set = [sorted(r.tolist()) for r in fused[0]] == [sorted(r.tolist()) for r in ref[0]]
    for name, col in (("log-likelihood", 2), ("probs", 1)):
        if name == "probs" and not same_set:      # a softmax over another candidate set is another quantity
            continue
        ef, top, pairs = _by_answer(fused[0], fused[col], ref[0], ref[col])
        ee, _, _ = _by_answer(eager[0], eager[col], ref[0], ref[col])
        print("RANK {} B={} {}: fused / eager max err vs fp64 {:.3e} / {:.3e} (max |ref| {:.3e}, {} answers)".format(
            label, b, name, ef, ee, top, pairs))
        assert pairs >= b * (model.cfg.k_test - 1)
        assert ef <= max(2.0 * ee, 1e-4 * max(1.0, top)), (name, ef, ee, top)


@pytest.mark.parametrize("b", [1, 3])
def test_small_model_against_fp64(small, b, monkeypatch):
    _check_against_fp64(small, b, 8, 20 + b, monkeypatch, "small")


def test_base_width_against_fp64(base, monkeypatch):
    _check_against_fp64(base, 2, 25, 31, monkeypatch, "base")


def test_the_fused_path_is_what_ran(small, monkeypatch):
    """With fused_rank on, the eager _decode sees the start token only (B rows); off, it sees the B k candidates."""
    from vqattack_amd.whitebox import albef
    states, masks = _question(3, 8, small.cfg.dim, 5)
    eager_decode = albef.FrozenAlbef._decode

    def start_only(self, ids, atts, question_states, question_atts):
        if ids.shape[0] > states.shape[0]:
            raise AssertionError("the eager _decode ran on the candidates")
        return eager_decode(self, ids, atts, question_states, question_atts)
    monkeypatch.setattr(albef.FrozenAlbef, "_decode", start_only)
    ids, probs, _ = _rank(small, states, masks, True)
    assert tuple(ids.shape) == (3, small.cfg.k_test) and bool(torch.isfinite(probs).all())
    with pytest.raises(AssertionError, match="ran on the candidates"):
        _rank(small, states, masks, False)


def test_two_fused_runs_give_identical_bits(small):
    states, masks = _question(3, 8, small.cfg.dim, 6)
    first, again = _rank(small, states, masks, True), _rank(small, states, masks, True)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_weight_updates_and_invalidate_fused_are_followed(small):
    model = copy.deepcopy(small)
    states, masks = _question(3, 8, model.cfg.dim, 7)

    def agree():
        fused, eager = _rank(model, states, masks, True), _rank(model, states, masks, False)
        err, top, pairs = _by_answer(fused[0], fused[2], eager[0], eager[2])
        assert pairs == 3 * model.cfg.k_test and err <= 1e-4 * max(1.0, top), (err, top)
        return fused[2]
    before = agree()
    with torch.no_grad():                                    # in place ON the parameters: weights_key sees it
        model.dec_layers[1].cross.k.weight.mul_(1.5)
        model.dec_word.weight.mul_(1.25)
    after = agree()
    assert not torch.equal(before, after)
    model.dec_layers[0].mlp.fc1.weight.data.mul_(0.5)        # through .data: invisible to weights_key
    model.dec_bias.data.add_(0.3 * torch.randn(model.cfg.vocab, device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)))
    model.invalidate_fused()
    assert not torch.equal(after, agree())


def test_fused_rank_does_not_write_the_logits(base):
    """Base width, B = 8, k = 16, L = 5: after a warm-up call (the packed caches), the peak of the fused rank_answer stays
    below the rows x vocabulary x 4 bytes of logits it no longer writes; the eager path exceeds that."""
    model = copy.deepcopy(base)
    g = torch.Generator().manual_seed(12)
    n, length = 40, 5
    ans = torch.zeros(n, length, dtype=torch.long)
    ans[:, 0] = model.cfg.bos_id
    ans[:, 1:4] = torch.randint(1000, model.cfg.vocab, (n, 3), generator=g)
    ans[:, 4] = model.cfg.sep_id
    model.set_answer_list(ans.to(DEV))
    model.cfg.k_test = 16
    states, masks = _question(8, 25, model.cfg.dim, 13)
    logits_bytes = 8 * 16 * (length - 1) * model.cfg.vocab * 4
    growth = {}
    for fused in (True, False):
        _rank(model, states, masks, fused)                   # warm-up
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        start = torch.cuda.memory_allocated()
        _rank(model, states, masks, fused)
        torch.cuda.synchronize()
        growth[fused] = torch.cuda.max_memory_allocated() - start
    print("RANK memory: fused {:.1f} MB, eager {:.1f} MB, logits {:.1f} MB".format(
        growth[True] / 2 ** 20, growth[False] / 2 ** 20, logits_bytes / 2 ** 20))
    assert growth[True] < logits_bytes < growth[False], (growth, logits_bytes)


def test_graph_capture_records_the_fused_ranking(small):
    """No host read on the fused path: a capture of rank_answer replays to the eager launch's bits."""
    states, masks = _question(3, 8, small.cfg.dim, 8)
    want = _rank(small, states, masks, True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got = _rank(small, states, masks, True)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(got, want):
        assert torch.equal(a, b)
