"""Which kernel families the conv containment test (tests/test_containment_gpu.py) reaches -- planner queries only, no GPU.

The GPU test runs one small representative per (op, stride, kernel family, tensor type).  Here: its case list still reaches every
family the per-kernel geometry lists reach, and every family of the benchmark's kernel plan that the small shapes do NOT reach is
written down with its reason (those are contained at the bench shapes by tests/test_bench_layers_gpu.py).  A planner change that
un-covers a family fails here, without a GPU."""
import json

from tests import bench_layers as BL
from tests import test_containment_gpu as C

# kernel family (symbol text before '<') of tests/golden/bench_kernel_plan.json -> why no small case of the containment test reaches it.
# Empty: the imported geometry lists reach every family of the benchmark's plan at small shapes.
NOT_REACHED_AT_SMALL_SHAPES = {}


def _names(keys):
    return {name for key in keys for name in key[2].split('+')}


def test_case_list_reaches_every_family_of_the_geometry_lists():
    reached = set()
    for case in C.conv_cases():
        reached |= C.families_of(case)
    wanted = set()
    for case in C.candidates():
        wanted |= C.families_of(case)
    assert wanted - reached == set(), sorted(wanted - reached)
    # one ladder entry per family, on a case of the list
    cases = set(C.conv_cases())
    assert {(op, c.geom[5]) for c, op in C.family_ladder_cases()} >= {(k[0], k[1]) for k in wanted}
    assert all(c in cases for c, _ in C.family_ladder_cases())
    assert len(C.family_ladder_cases()) == len(wanted)


def test_split_k_ladder_cases_split_deeply():
    """The extra ladder cases are there for the split-K clamp: at the full workspace each plans four slabs or more, with no workspace
    one."""
    import ctypes
    L, lib = C._lib()
    deep = 0
    for case, op in C.split_k_ladder_cases():
        splits = []
        for claim in C._rungs(C.ws_full(case.geom, op)):
            name, s, fl = ctypes.create_string_buffer(192), ctypes.c_int(0), ctypes.c_double(0)
            assert lib.pg_conv_kernel(ctypes.byref(C.conv_geom(case.geom)), C.OPCODE[op] + 16 * (case.algo | C.io_bits(case.storage, op)), claim, name,
                                      192, ctypes.byref(s), ctypes.byref(fl)) == 0
            splits.append(s.value)
        assert splits[0] == 1 and splits[-1] >= 4 and max(splits) == splits[-1], (case, op, splits)
        deep += len(set(splits)) >= 3
    assert deep >= 2, deep              # (the bf16 ones: another split at almost every rung)


def test_representatives_are_the_smallest_candidates():
    reps = C.representatives()
    for case in C.candidates():
        for key in C.families_of(case):
            assert C.elements(reps[key]) <= C.elements(case), (key, reps[key], case)


def test_bench_plan_families_not_reached_are_listed():
    with open(BL.PLAN_FILE) as f:
        plan = json.load(f)
    bench = {part.split('<')[0] for syms in plan.values() for sym in syms for part in sym.split('+')}
    reached = _names(C.representatives())
    assert bench - reached == set(NOT_REACHED_AT_SMALL_SHAPES), (sorted(bench - reached), sorted(NOT_REACHED_AT_SMALL_SHAPES))
    assert all(isinstance(why, str) and why for why in NOT_REACHED_AT_SMALL_SHAPES.values())
    # the fp32 PG_ALGO_AUTO Winograd families and the fast buffer-load families are reached at small shapes: never excused
    for name in NOT_REACHED_AT_SMALL_SHAPES:
        assert not name.startswith('k_wino') and not name.endswith('_fast'), name
    for name in ('k_wino_gemm', 'k_wino_bgemm_s3', 'k_wino_wgrad_gemm_s3', 'k_b2s_fast', 'k_s2b_fast', 'k_wgrad_fast'):
        assert name in reached, name


def test_workspace_ladder_rungs():
    assert C._rungs(0) == [0]
    assert C._rungs(256) == [0, 256]
    assert C._rungs(4096) == [0, 256, 2048, 3840, 4096]
    assert C._rungs(1 << 20) == [0, 256, 65536, 524288, (1 << 20) - 256, 1 << 20]
    for full in (0, 256, 512, 768, 98304, 17039360):
        r = C._rungs(full)
        assert r[0] == 0 and r[-1] == full and all(x % 256 == 0 for x in r) and r == sorted(set(r))


def test_queries_at_reduced_workspaces_name_no_winograd_kernel_at_zero():
    """The planner side of the ladder: pg_conv_kernel succeeds at every rung for every ladder case, and with no workspace it names no
    Winograd kernel (the header: the Winograd paths fall back to the implicit GEMM)."""
    for case, op in C.ladder_cases():
        algo_io = case.algo | C.io_bits(case.storage, op)
        for claim in C._rungs(C.ws_full(case.geom, op)):
            rc, sym = C.kernel_name(case.geom, C.OPCODE[op], algo_io, claim)
            assert rc == 0, (case, op, claim, rc)
            if claim == 0:
                assert 'k_wino' not in sym, (case, op, sym)
                full_sym = C.kernel_name(case.geom, C.OPCODE[op], algo_io, C.ws_full(case.geom, op))[1]
                if 'k_wino' in full_sym and op != 'wgrad':      # ... and there is no Winograd operand to hand over any more
                    assert C.hand_query(case, op, 'u', 0) == 0, (case, op)
                    assert op != 'b2s' or C.hand_query(case, op, 'v_keep', 0) == 0, (case, op)
