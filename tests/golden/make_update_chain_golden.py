"""Generate tests/golden/update_chain_trace.json: which ``ops`` launches the image update of the PGD operators makes, in
which order and on which tensors, for every combination of the five transfer stages -- recorded from the three hand-written
ladders of commit b34c08f (``attacks._fgm_then_project``, ``attacks._fgm_update``, ``BatchedVQAttack._update_runs``), the
last commit that had them.  ``tests/test_update_chain.py`` drives ``attacks._Chain`` the same way and compares.

    git worktree add ../parent b34c08f
    python tests/golden/make_update_chain_golden.py ../parent

Nothing here needs a device: the ladders touch tensors only through ``ops``, which is replaced by a ``Recorder``, and the
states are built by the code under test on a small CPU image.  A trace entry lists the calls by name with every argument
the real wrapper would have received (defaults filled in): tensors by the name of the buffer they view and their rows
(``x[0:5]``, ``si.ghat[2:4]``), host values as they are.  This module imports nothing of the package itself, so that the
test can share the recorder and the cases.
"""
import importlib
import inspect
import itertools
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "update_chain_trace.json")
PARENT = "b34c08f"
STAGES = ("mom", "ti", "di", "si", "vt")
SUBSETS = [frozenset(s) for k in range(6) for s in itertools.combinations(STAGES, k)]
NORMS = {"inf": np.inf, "2": 2, "1": 1}
# (form, norms): the step form (PGD's update), the FGM form with and without the range check (the FGM operators; the
# middle update of the dual loop), the per-run updates of the mixed-schedule driver (L-inf, no variance tuning)
FORMS = (("step", ("inf", "2")), ("fgm", ("inf", "2", "1")), ("fgm_nocheck", ("inf", "2", "1")), ("runs", ("inf",)))
BATCH, EPS, EPS_ITER, CLIP, N_EVALS = 5, 0.125, 0.01, (-1.0, 1.0), 2
NOW = ["F", "F", "N", "N", "M"]            # one global step of the mixed driver: three runs
HOST = ("di_draw", "di_check_table", "di_geometry", "si_scales", "si_weights", "vt_key_table", "ti_gaussian_taps",
        "new_flag")                         # host-side helpers of ops: they run as they are


def key(form, norm, subset):
    return "{}|{}|{}".format(form, norm, "+".join(s for s in STAGES if s in subset) or "plain")


def image():
    return torch.zeros(BATCH, 1, 2, 2)


def specs(subset):
    """(decay, taps, DI spec, SI spec, VT spec) as the ``_validate_*`` functions return them; None: stage off."""
    return (0.5 if "mom" in subset else None,
            np.array([0.25, 0.5, 0.25], dtype=np.float32) if "ti" in subset else None,
            (1.0, 1, np.random.RandomState(0)) if "di" in subset else None,
            (np.array([1.0, 0.5], dtype=np.float32), False) if "si" in subset else None,
            (2, 1.5, 7) if "vt" in subset else None)


class Recorder:
    """Stands in for the ``ops`` module of the code under test.  ``names``: storage address -> buffer name."""

    def __init__(self, real):
        self.real, self.calls, self.names, self.keep = real, [], {}, []

    def name(self, label, t):
        self.names[t.untyped_storage().data_ptr()] = (label, t)
        return t

    def name_state(self, label, obj):
        """Name every tensor a state object holds ``label.attribute`` (lists: ``label.attribute[i]``)."""
        for attr, value in sorted(vars(obj).items()) if obj is not None else ():
            for i, t in enumerate(value if isinstance(value, list) else [value]):
                if isinstance(t, torch.Tensor):
                    self.name("{}.{}{}".format(label, attr, "[{}]".format(i) if isinstance(value, list) else ""), t)

    def describe(self, v):
        if isinstance(v, torch.Tensor):
            label, base = self.names[v.untyped_storage().data_ptr()]       # KeyError: a tensor nobody named
            row = base.stride(0) if base.dim() > 1 else 1
            lo = (v.storage_offset() - base.storage_offset()) // row
            return "{}[{}:{}]".format(label, lo, lo + v.shape[0])
        if isinstance(v, (list, tuple)):
            return [self.describe(x) for x in v]
        if isinstance(v, np.ndarray):
            return v.tolist()
        return v if v is None or isinstance(v, (bool, int, str)) else float(v)

    def __getattr__(self, name):
        real = getattr(self.real, name)
        if name in HOST or not inspect.isfunction(real):
            return real
        if name == "reduce_workspace":
            return lambda t: torch.zeros(1)
        sig = inspect.signature(real)

        def op(*a, **kw):
            bound = sig.bind(*a, **kw)
            bound.apply_defaults()
            args = {k: self.describe(v) for k, v in bound.arguments.items()}
            if "x0" in args and args["x0"] is None and "eps" in args:
                args["eps"] = None         # without x0 the fused steps take their FGM form, which never reads eps
            self.calls.append([name, args])
            if bound.arguments.get("out") is not None:
                return bound.arguments["out"]
            if name == "momentum_accumulate":
                return bound.arguments["m"]
            first = next(v for v in bound.arguments.values() if isinstance(v, (torch.Tensor, list)))
            fresh = torch.zeros_like(first[0] if isinstance(first, list) else first)
            self.keep.append(fresh)
            return self.name("{}()".format(name), fresh)

        return op


def inputs(rec, subset):
    """The sentinels of one update: image, gradient (with SI and no VT the list of the copies'), centre, output, flag."""
    x, x0, out = (rec.name(n, image()) for n in ("x", "x0", "out"))
    flag = rec.name("flag", torch.zeros(1))
    if "si" in subset and "vt" not in subset:
        grad = [rec.name("grad{}".format(i), image()) for i in range(2)]
    else:
        grad = rec.name("grad", image())
    return x, grad, x0, out, flag


def parent_states(attacks, rec, subset, norm):
    """The states as the operators of b34c08f build them, in their order (momentum, TI, DI, SI, VT)."""
    decay, taps, dspec, sspec, vspec = specs(subset)
    like = image()
    mom = None if decay is None else attacks._Momentum(decay, like, None)
    ti = attacks._smoother(taps, like, norm, decay)
    di = attacks._diversity(dspec, like, N_EVALS, norm, decay, taps, vt=vspec is not None)
    si = attacks._scales(sspec, like, EPS_ITER, norm, mom, ti, di, vt=vspec is not None)
    vt = attacks._variance(vspec, like, EPS, N_EVALS)
    if vt is not None:
        vt.kind, vt.plain = 0, si is None and di is None           # as _evaluate_vt sets them
    return dict(mom=mom, ti=ti, di=di, si=si, vt=vt)


def finish_states(rec, states):
    """Name the states' tensors and give DI its current rows."""
    if states["di"] is not None:
        states["di"].geom = torch.zeros(BATCH, 4, dtype=torch.int32)
    for label, obj in states.items():
        rec.name_state(label, obj)
    return {"si.ghat": states["si"] is not None and states["si"].ghat is not None,
            "ti.ghat": states["ti"] is not None and states["ti"].ghat is not None,
            "di.grad": states["di"] is not None and states["di"].grad is not None}


def trace_parent(attacks, runner, form, norm, subset):
    rec = Recorder(attacks.ops)
    attacks.ops = runner.ops = rec
    try:
        if form == "runs":
            like = image()
            decay, taps, dspec, sspec, _ = specs(subset)
            mom = None if decay is None else rec.name("mom.m", image())
            ti = attacks._smoother(taps, like, np.inf, decay)
            di = attacks._diversity(dspec, like, N_EVALS, np.inf, decay, ti)
            si = attacks._scales(sspec, like, EPS_ITER, np.inf,
                                 None if mom is None else SimpleNamespace(decay=decay, m=mom), ti, di)
            scratch = finish_states(rec, dict(mom=None, ti=ti, di=di, si=si, vt=None))
            x, grad, x0, _, _ = inputs(rec, subset)
            driver = runner.BatchedVQAttack.__new__(runner.BatchedVQAttack)
            driver.cfg = runner.AttackConfig(eps=EPS, eps_iter=EPS_ITER, clip_min=CLIP[0], clip_max=CLIP[1], decay_factor=decay)
            driver._update_runs(x, grad, x0, NOW, mom, ti, di, si)
        else:
            states = parent_states(attacks, rec, subset, NORMS[norm])
            scratch = finish_states(rec, states)
            x, grad, x0, out, flag = inputs(rec, subset)
            if form == "step":
                attacks._fgm_then_project(x, grad, x0, EPS_ITER, EPS, NORMS[norm], CLIP[0], CLIP[1], out, flag=flag, **states)
            else:
                attacks._fgm_update(x, grad, EPS_ITER, NORMS[norm], CLIP[0], CLIP[1], flag=flag, out=out,
                                    check_range=form == "fgm", **states)
    finally:
        attacks.ops = runner.ops = rec.real
    return {"calls": rec.calls, "scratch": scratch}


def cases():
    for form, norms in FORMS:
        for norm in norms:
            for subset in SUBSETS:
                if form != "runs" or "vt" not in subset:
                    yield form, norm, subset


def main():
    sys.path.insert(0, os.path.abspath(sys.argv[1]))
    attacks = importlib.import_module("vqattack_amd.attacks")
    runner = importlib.import_module("vqattack_amd.attack.runner")
    assert os.path.abspath(attacks.__file__).startswith(os.path.abspath(sys.argv[1])), attacks.__file__
    attacks.dev_f32 = lambda t, *a, **k: t
    blob = {"recorded_from": PARENT, "entries": {key(*c): trace_parent(attacks, runner, *c) for c in cases()}}
    with open(OUT, "w") as f:
        json.dump(blob, f, indent=0, sort_keys=True)
    distinct = {json.dumps(e["calls"]) for e in blob["entries"].values()}
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(blob["entries"]), "entries,", len(distinct), "distinct traces")


if __name__ == "__main__":
    main()
