"""The image update of the PGD operators (``attacks._Chain.update``) against the launch sequences recorded from the three
hand-written ladders it replaced (tests/golden/update_chain_trace.json, from commit b34c08f; generator and recorder:
tests/golden/make_update_chain_golden.py).  No device: ``ops`` is a recorder and the chain's states live on a small CPU
image.  An entry is equal when every launch has the same name, in the same order, with the same effective arguments --
tensors compared by the buffer they view and their rows, host values by value."""
import json
import os

import numpy as np
import pytest
import torch

from tests.golden import make_update_chain_golden as gold
from vqattack_amd import attacks
from vqattack_amd.attack import runner

with open(gold.OUT) as f:
    GOLDEN = json.load(f)
CASES = list(gold.cases())


def _chain(monkeypatch, subset, norm, momentum=False):
    """(recorder, chain, which scratches it allocated): the chain built for real, on a CPU image, through the recorder."""
    rec = gold.Recorder(attacks.ops)
    monkeypatch.setattr(attacks, "ops", rec)
    monkeypatch.setattr(runner, "ops", rec)
    monkeypatch.setattr(attacks, "dev_f32", lambda t, *a, **k: t)
    m = rec.name("mom.m", gold.image()) if momentum and "mom" in subset else None
    chain = attacks._Chain(gold.specs(subset), gold.image(), norm, gold.EPS, gold.EPS_ITER, gold.N_EVALS, momentum=m)
    states = {s: getattr(chain, s) for s in gold.STAGES}
    if m is not None:
        states["mom"] = None                # the driver's own tensor, named above; its |grad| sums stay unused
    return rec, chain, gold.finish_states(rec, states)


def _trace(monkeypatch, form, norm, subset):
    rec, chain, scratch = _chain(monkeypatch, subset, gold.NORMS[norm], momentum=form == "runs")
    x, grad, x0, out, flag = gold.inputs(rec, subset)
    if form == "runs":
        driver = runner.BatchedVQAttack.__new__(runner.BatchedVQAttack)
        driver.cfg = runner.AttackConfig(eps=gold.EPS, eps_iter=gold.EPS_ITER, clip_min=gold.CLIP[0], clip_max=gold.CLIP[1],
                                         decay_factor=0.5 if "mom" in subset else None)
        driver._update_runs(x, grad, x0, gold.NOW, chain)
    else:
        chain.update(x, grad, x0 if form == "step" else None, gold.EPS_ITER, gold.EPS, gold.CLIP[0], gold.CLIP[1], out=out,
                     flag=flag, check_range=form != "fgm_nocheck")
    return {"calls": rec.calls, "scratch": scratch}


def test_the_golden_covers_every_case_and_names_its_commit():
    assert GOLDEN["recorded_from"] == gold.PARENT
    assert sorted(GOLDEN["entries"]) == sorted(gold.key(*c) for c in CASES)
    assert len(CASES) == 32 * (2 + 3 + 3) + 16
    # the two examples of the ladder's rule, by name
    names = lambda k: [c[0] for c in GOLDEN["entries"][k]["calls"]]
    assert names("step|inf|mom+ti+di+si+vt") == ["vt_tune", "ti_smooth", "sumabs_per_sample", "linf_momentum_step"]
    assert names("step|inf|di+si") == ["si_combine", "linf_di_step"]


@pytest.mark.parametrize("form,norm,subset", CASES, ids=[gold.key(*c) for c in CASES])
def test_update_launches_what_the_ladders_launched(monkeypatch, form, norm, subset):
    got = json.loads(json.dumps(_trace(monkeypatch, form, norm, subset)))       # tuples -> lists, like the file
    assert got == GOLDEN["entries"][gold.key(form, norm, subset)]


@pytest.mark.parametrize("subset", [s for s in gold.SUBSETS if "vt" not in s], ids=lambda s: gold.key("rows", "inf", s))
@pytest.mark.parametrize("fgm", [False, True], ids=["step", "fgm"])
def test_a_row_range_is_the_same_sequence_on_sliced_arguments(monkeypatch, subset, fgm):
    """``update(.., rows=(lo, hi))`` against the golden of the whole batch: the same launches with every per-sample
    tensor cut to rows ``[lo:hi)``.  One difference is intended and stated here: a run does not use the call's |grad| sums
    (their reduction workspace is sized for the whole batch), so the sums launch is absent and ``sumabs`` is None."""
    lo, hi = 1, 4
    rec, chain, _ = _chain(monkeypatch, subset, np.inf)
    x, grad, x0, out, flag = gold.inputs(rec, subset)
    chain.update(x, grad, None if fgm else x0, gold.EPS_ITER, gold.EPS, gold.CLIP[0], gold.CLIP[1], out=out, flag=flag,
                 rows=(lo, hi))
    whole, cut = "[0:{}]".format(gold.BATCH), "[{}:{}]".format(lo, hi)

    def sliced(v):
        if isinstance(v, list):
            return [sliced(u) for u in v]
        return v[:-len(whole)] + cut if isinstance(v, str) and v.endswith(whole) and not v.startswith("flag") else v

    want = []
    for name, args in GOLDEN["entries"][gold.key("fgm" if fgm else "step", "inf", subset)]["calls"]:
        if name == "sumabs_per_sample":
            continue
        args = {k: sliced(v) for k, v in args.items()}
        if "sumabs" in args:
            args["sumabs"] = None
        want.append([name, args])
    assert json.loads(json.dumps(rec.calls)) == want


def test_the_chain_without_stages_touches_no_tensor_of_its_own():
    chain = attacks._Chain()
    assert chain.fused is None and chain.slot is None
    assert all(getattr(chain, s) is None for s in gold.STAGES)
