"""Every instance of the shared gradient fold (csrc/fold.hpp) keeps its registers and its loop structure (no GPU needed:
hipcc cross-compiles here).

si.hip instantiates `grad_fold_vec_kernel<false, ...>`, admix.hip `<true, ...>`.  The kernel's loop is written out by
hand because every other form of it that was tried costs scalar registers (fold.hpp, profiles/r26, profiles/r28): above
96 of them a SIMD holds fewer than 8 waves.  The seeded 8-gradient image forms stood at 98 and 100 when they were added
(profiles/r27) and may not grow.  A source edit or a compiler update that breaks any of this changes no result: these
tests read registers, scratch, occupancy and the loop's load / store / wait sequence from the assembly
(`tools/isa_loop_mix.py`).
"""
import os
import re
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"),
                                reason="needs hipcc")
SGPR_LIMIT = {"false": 96, "true": 100}


@pytest.fixture(scope="module")
def folds():
    """{(seed, form, copies, slots, nt): (meta, sequence)} of every grad_fold_vec_kernel instance of the two files."""
    import isa_loop_mix
    found = {}
    for src, seed in (("si.hip", "false"), ("admix.hip", "true")):
        for name, meta, body in isa_loop_mix.kernels(isa_loop_mix.assembly(src)):
            m = re.match(r"vqa::grad_fold_vec_kernel<(\w+), (\d+), (\d+), (\d+), (\d+)>$", name)
            if m:
                assert m.group(1) == seed, (src, name)         # each file instantiates its own SEED value only
                found[(seed,) + tuple(int(v) for v in m.groups()[1:])] = (meta, isa_loop_mix.memory_sequence(body))
    return found


def test_every_instance_is_there(folds):
    # 3 forms x 8 copy counts x the NT masks {0, 2} without an image, {0, 2, 4, 6} with one
    for seed in ("false", "true"):
        keys = sorted(k[1:] for k in folds if k[0] == seed)
        want = sorted((form, c, 1 if seed == "true" or c > 3 else 2, nt)
                      for form in (0, 1, 2) for c in range(1, 9) for nt in ((0, 2) if form == 0 else (0, 2, 4, 6)))
        assert keys == want, seed


def test_no_scratch_eight_waves_and_the_scalar_register_limits(folds):
    for key, (meta, _seq) in folds.items():
        assert meta["ScratchSize"] == "0", key
        assert meta["Occupancy"] == "8", key
        assert int(meta["sgpr_count"]) <= SGPR_LIMIT[key[0]], (key, meta["sgpr_count"])


def test_every_load_of_a_tile_is_issued_before_the_first_wait(folds):
    for key, (_meta, seq) in folds.items():
        _seed, form, copies, slots, _nt = key
        waits = [i for i, s in enumerate(seq) if s.startswith("w")]
        loads = [i for i, s in enumerate(seq) if s == "L"]
        streams = copies + (key[0] == "true") + (form != 0) + (form == 2)
        assert len(loads) == slots * streams, (key, seq)
        assert waits and max(loads) < min(waits), (key, seq)


def test_the_stores_of_a_tile_form_one_run(folds):
    """The unseeded fold of ONE gradient without an image, `<false, 0, 1, 2, NT>` (out = w_0 * g_0, two slots), is the
    instance that breaks this first: without the scheduling barrier fold.hpp gives it, each slot is stored as soon as
    its single product is done, `L L w1 S w1 S`."""
    broken = {}
    for key, (_meta, seq) in folds.items():
        stores = [i for i, s in enumerate(seq) if s == "S"]
        if len(stores) != key[3] or stores != list(range(stores[0], stores[0] + key[3])):
            broken[key] = " ".join(seq)
    assert not broken, broken
