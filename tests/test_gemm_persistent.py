"""The persistent launch of the bf16x6 GEMM's 128 x 256 tile (``csrc/gemm.hip``: ``gemm_bf16x6_persistent_kernel`` behind
``vqa_gemm_bf16x6_persistent``, ``ops.gemm_persistent`` / ``ops.gemm(tile="persistent")``) and its dispatch
(``_fused.PERSISTENT_POLICY``, ``VQA_GEMM_PERSISTENT``).

CPU: the new kernel's k-loop from the compiler's assembly (tools/isa_loop_mix.py --innermost), the existing large-tile
kernels' loops against the counts recorded in profiles/r16/loop_mix.txt, the entry point's return codes (every check
precedes the first launch), what ``ops.gemm`` calls with the wrappers stubbed, on meta tensors.
GPU: the bits of ``ops.gemm(tile="wide")`` and of the register-staged small kernel at ``ksplit == 1`` over 1 to 4 k-steps
(one step: the first is also the last; odd / even: the buffer parity flips / stays across tiles), row counts with a
ragged last block, whose tiles end a workgroup's list or are followed by another tile, grids from one workgroup to more
than there are tiles, the vector and the dword epilogue, sentinels around the output; the same call twice; a captured call replayed; refused calls
write nothing; a two-expert encoder with every plain GEMM persistent against the same encoder with none.
"""
import ctypes
import functools
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "gemm_bf16x6_persistent_kernel"
ERR_NULL, ERR_SHAPE, ERR_ALIGN = -1, -2, -3
# every kernel that runs a 256 x 128, 128 x 256 or 128 x 128 tile, as profiles/r16/loop_mix.txt names it
LARGE_TILE = ("gemm_bf16x6_kernel", "gemm_bf16x6_wide_kernel", "gemm_bf16x6_half_kernel") + tuple(
    "{}<{}>".format(k, e) for k in ("gemm_bf16x6_epi_kernel", "gemm_bf16x6_wide_epi_kernel") for e in (1, 2, 3)) + tuple(
    "gemm_bf16x6_grouped_kernel<{}>".format(e) for e in (0, 1, 2))


# ---------------------------------------------------------------------------------------------------------- CPU: assembly
@functools.lru_cache(maxsize=None)
def _mix():
    spec = importlib.util.spec_from_file_location("isa_loop_mix", os.path.join(ROOT, "tools", "isa_loop_mix.py"))
    mix = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mix)
    return mix


@functools.lru_cache(maxsize=None)
def _assembly():
    return _mix().assembly("gemm.hip")


@functools.lru_cache(maxsize=None)
def _gemm_kernels(innermost):
    mix = _mix()
    return {name.split("::")[-1]: (meta, body) for name, meta, body in mix.kernels(_assembly(), innermost=innermost)}


def _loop_lines(body):
    return [(l.split()[0], l) for l in body.split("\n") if l.startswith("\t") and l.split() and not l.strip().startswith(";")]


def _count(seq, pre):
    return sum(o.startswith(pre) for o in seq)


def test_k_loop_is_the_wide_loop():
    """Per k-step 96 MFMAs, the six pieces of packed B as direct-to-LDS loads and no direct load of another width, the
    three planes of one piece of A as the only LDS writes, 24 fragment reads, two ordinary loads of A, one barrier; no
    scratch, two waves per SIMD.  The same counts as the wide kernel's loop."""
    kernels = _gemm_kernels(True)
    meta, body = kernels[KERNEL]
    ops_ = [o for o, _l in _loop_lines(body)]
    ref = [o for o, _l in _loop_lines(kernels["gemm_bf16x6_wide_kernel"][1])]
    print(KERNEL, meta, {pre: _count(ops_, pre) for pre in ("v_mfma", "global_load_lds_dwordx4", "ds_write", "ds_read", "global_load", "v_")})
    assert _count(ops_, "v_mfma") == 96
    assert sum(o == "global_load_lds_dwordx4" for o in ops_) == 6 and _count(ops_, "global_load_lds") == 6
    assert sum(o == "ds_write_b128" for o in ops_) == 3 and _count(ops_, "ds_write") == 3, "B is written to LDS from registers"
    assert sum(o == "ds_read_b128" for o in ops_) == 24 and _count(ops_, "ds_read") == 24
    assert sum(o == "global_load_dwordx4" for o in ops_) == 2 and _count(ops_, "global_load") == 8
    assert _count(ops_, "global_store") == 0 and _count(ops_, "scratch_") == 0 and _count(ops_, "buffer_") == 0
    assert sum(o == "s_barrier" for o in ops_) == 1
    assert meta["ScratchSize"] == "0" and meta["Occupancy"] == "2" and int(meta["NumVgprs"]) <= 256, meta
    for pre in ("v_mfma", "global_load", "ds_write", "ds_read", "s_barrier"):
        assert _count(ops_, pre) == _count(ref, pre), pre
    # the last step is written out behind the loop, so the loop selects nothing: no vector work the wide loop does not have
    valu = lambda seq: sum(o.startswith("v_") and not o.startswith("v_mfma") for o in seq)
    assert valu(ops_) <= valu(ref) + 4, (valu(ops_), valu(ref))


def test_k_loop_waits_for_its_direct_loads_and_spaces_its_global_loads():
    _meta, body = _gemm_kernels(True)[KERNEL]
    seq = _mix().memory_sequence(body)
    print(KERNEL, " ".join(seq))
    assert seq.count("|") == 1 and seq.count("L") == 8 and seq.count("S") == 0
    pending = seen = 0
    for op, line in _loop_lines(body):
        if op.startswith("global_load_lds"):
            pending, seen = pending + 1, seen + 1
        elif op == "s_waitcnt" and "vmcnt(0)" in line:
            pending = 0
        elif op == "s_barrier":
            assert pending == 0, "{} direct loads outstanding at the barrier".format(pending)
    assert seen == 6 and pending == 0
    order = "".join("M" if o.startswith("v_mfma") else "G" for o, _l in _loop_lines(body) if o.startswith(("v_mfma", "global_load")))
    assert order.index("M") <= 2, "more than two global loads ahead of the first MFMA"
    assert "GGG" not in order, "three global loads with no MFMA between them"
    assert order[:order.rindex("G")].count("M") <= 48, "a load of the next step issued in the second half of the step"


def test_the_steps_outside_the_k_loop_wait_for_their_direct_loads():
    """The blocks of the tile loop as tools/isa_loop_mix.py lists them without --innermost (the tile's last step, which
    stages the next tile, and the epilogue; the k-loop's own block is the test above): every barrier has the direct
    loads ahead of it waited for, and the steps hold whole multiples of the k-loop's counts."""
    _meta, body = _gemm_kernels(False)[KERNEL]
    ops_ = [o for o, _l in _loop_lines(body)]
    steps = sum(o == "s_barrier" for o in ops_)
    assert _count(ops_, "global_store") > 0, "the epilogue is not among these blocks"
    assert steps >= 1 and _count(ops_, "v_mfma") == 96 * steps and _count(ops_, "global_load_lds") == 6 * steps
    assert _count(ops_, "ds_write") == 3 * steps and _count(ops_, "ds_read") == 24 * steps
    pending = 0
    for op, line in _loop_lines(body):
        if op.startswith("global_load_lds"):
            pending += 1
        elif op == "s_waitcnt" and "vmcnt(0)" in line:
            pending = 0
        elif op == "s_barrier":
            assert pending == 0, "{} direct loads outstanding at a barrier".format(pending)


def test_existing_large_tile_loops_are_those_of_round_16():
    """The loops of the kernels this change must not touch, line by line as tools/isa_loop_mix.py --waits prints them,
    against the record of the round before (no nested loop among them: --innermost prints the same)."""
    mix = _mix()
    recorded = {}
    lines = open(os.path.join(ROOT, "profiles", "r16", "loop_mix.txt")).read().split("\n")
    for n, line in enumerate(lines):
        found = re.match(r"vqa::(\S+)\s+vgpr\s+(\d+) occ (\d+) scratch (\d+) \| loop: mfma\s+(\d+) valu\s+(\d+) \(slow\s+(\d+)\) "
                         r"lds\s+(\d+) vmem\s+(\d+)", line)
        if found:
            waits = next(l for l in lines[n + 1:n + 3] if re.match(r"\s+[LSAw|]", l) and "v_" not in l)
            recorded[found.group(1)] = (tuple(int(v) for v in found.groups()[1:]), waits.split())
    assert set(LARGE_TILE) <= set(recorded), sorted(set(LARGE_TILE) - set(recorded))
    now = _gemm_kernels(True)
    for name in LARGE_TILE:
        meta, body = now[name]
        ins = [o for o, _l in _loop_lines(body)]
        valu = [x for x in ins if x.startswith("v_") and not x.startswith("v_mfma")]
        slow = [x for x in valu if x.startswith(("v_mul_lo", "v_mul_hi", "v_mad_u64", "v_mad_i64"))]
        counts = (int(meta["NumVgprs"]), int(meta["Occupancy"]), int(meta["ScratchSize"]), _count(ins, "v_mfma"), len(valu),
                  len(slow), _count(ins, "ds_"), sum(x.startswith(("global_", "buffer_")) for x in ins))
        assert (counts, mix.memory_sequence(body)) == recorded[name], name
        assert body == _gemm_kernels(False)[name][1], name + ": --innermost changes what is reported"


# ---------------------------------------------------------------------------------------------------------- CPU: return codes
def _host_call(A, packed, bias, C, lda=64, ldc=256, M=4, N=256, K=64, workgroups=1):
    from vqattack_amd import _hip
    return _hip.lib().vqa_gemm_bf16x6_persistent(A, lda, packed, bias, C, ldc, M, N, K, workgroups, None)


def test_argument_validation_returns_error_codes_without_touching_a_gpu():
    """Host addresses: no launch is reached with a bad argument, and the good call below has no rows."""
    buf = (ctypes.c_char * 4096)()
    base = (ctypes.addressof(buf) + 63) & ~63
    A, packed, bias, C = base, base + 1024, base + 2048, base + 3072
    assert _host_call(A, packed, bias, C, M=0) == 0
    assert _host_call(A, packed, bias, C, N=384) == ERR_SHAPE and _host_call(A, packed, bias, C, N=128, ldc=128) == ERR_SHAPE
    assert _host_call(A, packed, bias, C, N=0) == ERR_SHAPE and _host_call(A, packed, bias, C, K=48) == ERR_SHAPE
    assert _host_call(A, packed, bias, C, workgroups=0) == ERR_SHAPE and _host_call(A, packed, bias, C, workgroups=-3) == ERR_SHAPE
    assert _host_call(A, packed, bias, C, M=0, workgroups=0) == ERR_SHAPE          # ... also where there is nothing to launch
    assert _host_call(None, packed, bias, C) == ERR_NULL and _host_call(A, None, bias, C) == ERR_NULL
    assert _host_call(A, packed, bias, None) == ERR_NULL
    assert _host_call(A, packed, None, C, M=0) == 0                                 # the bias alone may be missing
    assert _host_call(A, packed, bias, C, M=-1) == ERR_SHAPE and _host_call(A, packed, bias, C, ldc=255) == ERR_SHAPE
    assert _host_call(A, packed, bias, C, lda=66) == ERR_SHAPE and _host_call(A, packed, bias, C, lda=32) == ERR_SHAPE
    assert _host_call(A, packed, bias, C, M=1 << 40) == ERR_SHAPE                   # more than 2^31 - 1 tiles
    assert _host_call(A + 4, packed, bias, C) == ERR_ALIGN and _host_call(A, packed, bias, C + 2) == ERR_ALIGN
    assert _host_call(A, packed + 8, bias, C) == ERR_ALIGN and _host_call(A, packed, bias + 2, C) == ERR_ALIGN
    del buf


def test_header_and_binding_name_the_entry_point():
    from vqattack_amd import _hip
    header = open(os.path.join(ROOT, "include", "vqattack_hip.h")).read()
    assert "int vqa_gemm_bf16x6_persistent(" in header
    assert len(_hip.SIGNATURES["vqa_gemm_bf16x6_persistent"][1]) == 11
    source = open(os.path.join(ROOT, "vqattack_amd", "csrc", "gemm.hip")).read()
    assert "// Persistent:" in source[:source.index("#include")]


# ---------------------------------------------------------------------------------------------------------- CPU: dispatch
class _Packed:
    def __init__(self, K, N):
        self.K, self.N, self.data = K, N, None


def _stub(monkeypatch, switch=None, policy=None, **env):
    """``ops.gemm`` on meta tensors with the launching wrappers recorded: run(rows, N, K, **kw) -> the calls."""
    import torch
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    for name in ("VQA_GEMM_PERSISTENT", "VQA_GEMM", "VQA_GEMM_TAIL", "VQA_GEMM_TAIL_CUS"):
        monkeypatch.delenv(name, raising=False)
    if switch is not None:
        monkeypatch.setenv("VQA_GEMM_PERSISTENT", switch)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    monkeypatch.setattr(_fused, "PERSISTENT_POLICY", {} if policy is None else policy)
    calls = []
    monkeypatch.setattr(ops, "gemm_persistent", lambda a, pk, bias=None, out=None, workgroups=None:
                        calls.append(("persistent", a.shape[0], pk.N, pk.K, workgroups)))
    monkeypatch.setattr(ops, "_gemm_rows", lambda a, pk, bias, out, tile, m_split:
                        calls.append((str(tile), a.shape[0], pk.N, pk.K) if m_split is None else ("rows", str(tile), m_split)))
    monkeypatch.setattr(ops, "_gemm_epilogue", lambda a, pk, bias, out, tile, epilogue, aux: calls.append(("epi", tile, epilogue)))

    def run(rows, N, K, **kw):
        del calls[:]
        ops.gemm(torch.empty(rows, K, device="meta"), _Packed(K, N), **kw)
        return list(calls)
    return run


# the benchmark's plain large-tile GEMMs (VLMo-base, batch 64): WIDE_POLICY lists three classes, the qkv classes run 256 x 128
_TODAY = [((37824, 768, 768), "wide"), ((36928, 3072, 768), "wide"), ((36928, 768, 3072), "wide"),
          ((37824, 2304, 768), "large"), ((37824, 768, 2304), "large")]


def test_unset_switch_and_empty_table_call_what_is_called_today(monkeypatch):
    run = _stub(monkeypatch)
    for shape, tile in _TODAY:
        assert run(*shape) == [(tile,) + shape]
    run = _stub(monkeypatch, switch="0", policy={(768, 768): (1, 1 << 30)})
    assert run(37824, 768, 768) == [("wide", 37824, 768, 768)]


def test_switch_runs_every_plain_product_with_n_256_persistent(monkeypatch):
    run = _stub(monkeypatch, switch="1")
    for shape, _tile in _TODAY:
        assert run(*shape) == [("persistent",) + shape + (None,)]
    assert run(5000, 384, 64) == [("large", 5000, 384, 64)]                          # N % 256 != 0: no 128 x 256 tile
    # a tile of the caller's, an epilogue and a cut of the caller's are left alone
    assert run(37824, 768, 768, tile="wide") == [("wide", 37824, 768, 768)]
    assert run(37824, 768, 768, tile="large") == [("large", 37824, 768, 768)]
    assert run(37824, 768, 768, m_split=128) == [("rows", "wide", 128)]
    import torch
    aux = torch.empty(36928, 3072, device="meta")
    assert run(36928, 3072, 768, epilogue="gelu_grad", aux=aux) == [("epi", "wide", "gelu_grad")]
    assert run(37824, 768, 768, tile="persistent") == [("persistent", 37824, 768, 768, None)]
    # a product that the tail plan cuts stays cut (888 tiles on 256 CUs: 3 full rounds and a part of one)
    run = _stub(monkeypatch, switch="1", VQA_GEMM_TAIL="1", VQA_GEMM_TAIL_CUS="256")
    assert run(37824, 768, 768) == [("wide", 37824, 768, 768)]
    assert run(32768, 768, 768) == [("persistent", 32768, 768, 768, None)]           # 768 tiles: whole rounds, no cut


def test_listed_class_is_persistent_within_its_rows_only(monkeypatch):
    run = _stub(monkeypatch, policy={(768, 768): (35264, 37824)})
    assert run(37824, 768, 768) == [("persistent", 37824, 768, 768, None)]
    assert run(35264, 768, 768) == [("persistent", 35264, 768, 768, None)]
    assert run(40000, 768, 768) == [("large", 40000, 768, 768)]                      # outside the rows of either table
    assert run(36928, 3072, 768) == [("wide", 36928, 3072, 768)]
    for mode in ("large", "wide"):                                                   # a forced tile is a forced tile
        run = _stub(monkeypatch, policy={(768, 768): (35264, 37824)}, VQA_GEMM=mode)
        assert run(37824, 768, 768) == [(mode, 37824, 768, 768)]
        run = _stub(monkeypatch, switch="1", VQA_GEMM=mode)                          # ... for the switch as for the table
        assert run(37824, 768, 768) == [(mode, 37824, 768, 768)]


def test_shipped_table_is_well_formed():
    from vqattack_amd.whitebox import _fused
    for (n, k), (lo, hi) in _fused.PERSISTENT_POLICY.items():
        assert n % 256 == 0 and k % 32 == 0 and 1 <= lo <= hi


def test_wrapper_checks_its_arguments():
    import torch
    from vqattack_amd import ops
    a = torch.empty(5, 64, device="meta")
    with pytest.raises(ValueError):
        ops.gemm(a, _Packed(64, 256), tile="persistent", m_split=3)
    with pytest.raises(ValueError):
        ops.gemm(a, _Packed(64, 256), tile="persistent", epilogue="gelu")
    with pytest.raises(ValueError):
        ops.gemm(a, _Packed(64, 256), tile="resident")


# ---------------------------------------------------------------------------------------------------------- GPU
def _torch():
    import torch
    return torch, torch.device("cuda", 0)


SENTINEL = 7.0
ROWS = (1, 127, 128, 129, 385, 513)
# (ldc - N, floats C is offset by, lda - K): the 16-byte epilogue on a padded C and a strided A; the dword epilogue for an
# odd row stride and for a C one float off its 16-byte boundary
LAYOUTS = [(4, 0, 4), (1, 0, 0), (4, 1, 4)]


def _problem(M, N, K, has_bias, pad, seed):
    torch, dev = _torch()
    from vqattack_amd import ops
    g = torch.Generator(device=dev).manual_seed(seed)
    a = torch.randn(M, K + pad, device=dev, generator=g)[:, :K]
    w = torch.randn(N, K, device=dev, generator=g) * 0.05
    bias = torch.randn(N, device=dev, generator=g) * 0.05 if has_bias else None
    return a, ops.gemm_pack(w, trans=True), bias


def _guarded(M, N, ldc, c_off, guard=2):
    """An (M, N) output view with row stride ldc, ``c_off`` floats into its buffer, every other float a sentinel."""
    torch, dev = _torch()
    store = torch.full((c_off + (M + guard) * ldc,), SENTINEL, device=dev)
    view = store[c_off:].view(M + guard, ldc)
    return store, view, view[:M, :N]


def _untouched(store, view, M, N, c_off):
    return bool((view[:M, N:] == SENTINEL).all()) and bool((view[M:] == SENTINEL).all()) and \
        bool((store[:c_off] == SENTINEL).all())


def _grids(tiles):
    return sorted({1, 2, 3, 5, 8, tiles, tiles + 7})


@pytest.mark.gpu
@pytest.mark.parametrize("K", [32, 64, 96, 128])
@pytest.mark.parametrize("N", [256, 512])
def test_every_grid_has_the_bits_of_the_wide_tile_and_of_the_small_kernel(N, K):
    torch, dev = _torch()
    from vqattack_amd import ops
    for mi, M in enumerate(ROWS):
        tiles = -(-M // 128) * (N // 256)
        for vi, (ldc_pad, c_off, lda_pad) in enumerate(LAYOUTS):
            a, packed, bias = _problem(M, N, K, (mi + vi) % 2 == 0, lda_pad, 100 * mi + 10 * vi + N + K)
            assert M == 1 or a.stride(0) == K + lda_pad
            want = ops.gemm(a, packed, bias, tile="wide")
            assert torch.equal(want, ops.gemm_small(a, packed, bias, ksplit=1))
            for workgroups in _grids(tiles):
                store, view, out = _guarded(M, N, N + ldc_pad, c_off)
                got = ops.gemm_persistent(a, packed, bias, out=out, workgroups=workgroups)
                assert got is out and torch.equal(out, want), (M, workgroups, ldc_pad, c_off)
                assert _untouched(store, view, M, N, c_off), (M, workgroups, "a float outside the output was written")
    # the wrapper's own output and grid (one workgroup per CU, clamped to the tiles), twice, and through ops.gemm
    first = ops.gemm_persistent(a, packed, bias)
    again = ops.gemm_persistent(a, packed, bias, out=first)
    assert again is first and first.is_contiguous() and torch.equal(first, want)
    assert torch.equal(ops.gemm(a, packed, bias, tile="persistent"), want)


@pytest.mark.gpu
def test_many_tiles_per_workgroup_and_a_ragged_tile_followed_by_another():
    """2049 rows x 768 columns: 17 row blocks x 3 column blocks = 51 tiles, the last three ragged (one row each).  The
    ragged block is always the last row block, but it has three tiles: one workgroup runs all 51 in one list, so ragged
    tiles 48 and 49 are each followed by another tile (their guarded stores ahead of the next k-loop), and 3 to 300
    workgroups deal the tiles out in every other way.  K = 96: the buffer parity flips at every tile."""
    torch, dev = _torch()
    from vqattack_amd import ops
    M, N, K = 2049, 768, 96
    a, packed, bias = _problem(M, N, K, True, 0, 7)
    want = ops.gemm(a, packed, bias, tile="wide")
    assert torch.equal(want, ops.gemm_small(a, packed, bias, ksplit=1))
    for workgroups in (1, 3, 5, 8, 13, 50, 51, 300):
        store, view, out = _guarded(M, N, N, 0)
        ops.gemm_persistent(a, packed, bias, out=out, workgroups=workgroups)
        assert torch.equal(out, want), workgroups
        assert _untouched(store, view, M, N, 0), workgroups


def _c_call(a, packed, bias, c_ptr, ldc, M, N, K, workgroups):
    from vqattack_amd import _hip
    return _hip.lib().vqa_gemm_bf16x6_persistent(a.data_ptr() if a is not None else None, a.stride(0) if a is not None else K,
                                                 packed.data.data_ptr(), bias.data_ptr() if bias is not None else None,
                                                 c_ptr, ldc, M, N, K, workgroups, _hip.stream_for(packed.data))


@pytest.mark.gpu
def test_a_refused_call_leaves_the_output_at_its_sentinel():
    torch, dev = _torch()
    from vqattack_amd import ops
    M, N, K = 200, 256, 64
    a, packed, bias = _problem(M, N, K, True, 0, 3)
    a384, packed384, bias384 = _problem(M, 384, K, True, 0, 4)
    out = torch.full((M, 384), SENTINEL, device=dev)
    p = out.data_ptr()
    codes = {
        "n": _c_call(a384, packed384, bias384, p, 384, M, 384, K, 4),
        "workgroups0": _c_call(a, packed, bias, p, N, M, N, K, 0),
        "workgroups-1": _c_call(a, packed, bias, p, N, M, N, K, -1),
        "null_a": _c_call(None, packed, bias, p, N, M, N, K, 4),
        "null_c": _c_call(a, packed, bias, None, N, M, N, K, 4),
        "ldc": _c_call(a, packed, bias, p, N - 1, M, N, K, 4),
        "c_align": _c_call(a, packed, bias, p + 2, N, M, N, K, 4),
        "empty": _c_call(a, packed, bias, p, N, 0, N, K, 4),
    }
    torch.cuda.synchronize()
    assert codes["n"] == codes["workgroups0"] == codes["workgroups-1"] == codes["ldc"] == ERR_SHAPE, codes
    assert codes["null_a"] == codes["null_c"] == ERR_NULL and codes["c_align"] == ERR_ALIGN and codes["empty"] == 0, codes
    assert bool((out == SENTINEL).all()), "a refused or empty call wrote to C"
    assert _c_call(a, packed, bias, p, 384, M, N, K, 4) == 0                         # and the same operands, intact, run
    torch.cuda.synchronize()
    assert torch.equal(out[:, :N], ops.gemm_small(a, packed, bias, ksplit=1)) and bool((out[:, N:] == SENTINEL).all())
    with pytest.raises(ValueError):
        ops.gemm_persistent(a384, packed384, bias384)
    with pytest.raises(ValueError):
        ops.gemm_persistent(a, packed, bias, workgroups=0)


@pytest.mark.gpu
def test_a_captured_call_replays_on_fresh_inputs():
    """The tile list is blockIdx arithmetic: a captured launch has nothing to reset, and reads its operands anew."""
    torch, dev = _torch()
    from vqattack_amd import ops
    M, N, K = 385, 512, 96
    a, packed, bias = _problem(M, N, K, True, 0, 21)
    a = a.contiguous()
    out = torch.zeros(M, N, device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                          # load the library and warm the allocator outside the capture
        ops.gemm_persistent(a, packed, bias, out=out, workgroups=3)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gemm_persistent(a, packed, bias, out=out, workgroups=3)
    gen = torch.Generator(device=dev).manual_seed(99)
    for _round in range(2):
        a.copy_(torch.randn(a.shape, device=dev, generator=gen))
        out.fill_(SENTINEL)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.gemm(a, packed, bias, tile="wide"))


def _two_expert_spec(d, heads, depth, seed):
    """A VLMo-shaped encoder whose layers all have a text and an image FFN (4 d wide), from random frozen weights."""
    torch, dev = _torch()
    from vqattack_amd.whitebox import _fused
    g = torch.Generator(device=dev).manual_seed(seed)
    rnd = lambda *shape, s=0.05: torch.randn(*shape, device=dev, generator=g) * s
    ln = lambda: (1.0 + rnd(d, s=0.1), rnd(d, s=0.1))
    mlp = lambda: (rnd(4 * d, d), rnd(4 * d), rnd(d, 4 * d), rnd(d))
    layers = [_fused.LayerSpec(ln(), rnd(3 * d, d), rnd(3 * d), rnd(d, d), rnd(d), 0.5 + rnd(d, s=0.1), [ln(), ln()],
                               [mlp(), mlp()], 0.5 + rnd(d, s=0.1), 1e-6) for _ in range(depth)]
    return _fused.EncoderSpec(layers, ln(), 1e-6, heads)


@pytest.mark.gpu
def test_encoder_with_every_plain_gemm_persistent_has_the_bits_of_the_encoder_with_none(monkeypatch):
    """3 samples x (5 text + 20 image tokens) at width 256 (4 heads of 64, FFN 1024), two experts in both layers.  With
    MIN_WORKGROUPS at 1 every GEMM runs a bf16x6 kernel, whose tiles all give the same bits, so the persistent launch
    must not change a bit of the feature maps, the final states or the input gradient."""
    torch, dev = _torch()
    from vqattack_amd import ops
    from vqattack_amd.whitebox import _fused
    for name in ("VQA_GEMM", "VQA_GEMM_TAIL", "VQA_GEMM_GROUPED", "VQA_GEMM_EPILOGUE"):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setattr(_fused, "MIN_WORKGROUPS", 1)
    spec = _two_expert_spec(256, 4, 2, 11)
    g = torch.Generator(device=dev).manual_seed(12)
    x0 = torch.randn(3, 25, 256, device=dev, generator=g)
    seen = []
    real = ops.gemm_persistent

    def counted(a, packed, *args, **kw):
        seen.append((a.shape[0], packed.N, packed.K))
        return real(a, packed, *args, **kw)
    monkeypatch.setattr(ops, "gemm_persistent", counted)
    results, grads = {}, None
    for switch in ("0", "1"):
        monkeypatch.setenv("VQA_GEMM_PERSISTENT", switch)
        del seen[:]
        x = x0.clone().requires_grad_(True)
        feats, states = _fused.encode(x, spec, None, 5)
        outs = list(feats[1:]) + [states]
        if grads is None:
            grads = [torch.randn(o.shape, device=dev, generator=g) for o in outs]
        torch.autograd.backward(outs, grads, inputs=[x])
        results[switch] = ([o.detach() for o in outs], x.grad, list(seen))
    assert results["0"][2] == [], "VQA_GEMM_PERSISTENT=0 reached the persistent entry point"
    calls = results["1"][2]
    # per layer: qkv, projection, two experts' fc1 and fc2, forward and input gradient
    assert len(calls) == 2 * 2 * 6, calls
    assert {(n, k) for _m, n, k in calls} == {(768, 256), (256, 768), (256, 256), (1024, 256), (256, 1024)}
    for o0, o1 in zip(results["0"][0], results["1"][0]):
        assert bool(torch.isfinite(o0).all()) and torch.equal(o0, o1)
    assert float(results["0"][1].abs().max()) > 0 and torch.equal(results["0"][1], results["1"][1])
