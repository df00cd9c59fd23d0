"""The Gamma-tiling planner (``pbvi_gamma_tiling_plan``): pure host arithmetic, so its properties are checked with no GPU
and no engine.  ``bytes_needed`` of a plan is the chunk's Gamma rows, score slabs and tile lists plus -- with more than
one chunk -- the full score matrix."""
import ctypes as C

import pytest

from pomdp_pbvi_exploration_amd import engine as eng
from pomdp_pbvi_exploration_amd.engine import gamma_tiling_plan

SHAPES = [(S, A, O) for S in (600, 2400, 30000, 61875) for A, O in ((6, 3), (16, 5), (2, 2))]
AMPLE = 1 << 50


def whole_bytes(S, A, O, V, B, dtype):
    rows, n, need = gamma_tiling_plan(S, A, O, V, B, dtype, AMPLE)
    assert n == 1 and rows >= V and rows % 4 == 0
    return need


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('S,A,O', SHAPES)
def test_planner_properties_over_a_grid_of_shapes(S, A, O, dtype):
    for V, B in ((1, 1), (7, 64), (1386, 100), (6000, 256), (8192, 1024), (100000, 300)):
        if A * O * (V + 1) + 2 * A > 2**31 - 1:
            continue
        whole = whole_bytes(S, A, O, V, B, dtype)
        # the smallest tiled plan: 4 rows per chunk (rows requested explicitly)
        floor = gamma_tiling_plan(S, A, O, V, B, dtype, AMPLE, chunk_rows=4)[2] if V > 4 else whole
        for budget in (0, floor - 1, floor, (floor + whole) // 2, whole - 1, whole, 2 * whole):
            if budget < min(floor, whole):
                with pytest.raises(MemoryError) as err:
                    gamma_tiling_plan(S, A, O, V, B, dtype, budget)
                assert 'budget' in str(err.value) and str(budget) in str(err.value)
                continue
            rows, n, need = gamma_tiling_plan(S, A, O, V, B, dtype, budget)
            assert rows % 4 == 0 and rows >= 4
            assert n * rows >= V > (n - 1) * rows
            assert need <= budget
            if budget >= whole:
                assert n == 1 and need == whole
            else:
                assert n > 1
                # nothing larger with fewer chunks would have fitted
                fewer = -(-V // (n - 1))
                fewer += -fewer % 4
                if fewer < V:
                    assert gamma_tiling_plan(S, A, O, V, B, dtype, AMPLE, chunk_rows=fewer)[2] > budget


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('S,A,O', SHAPES[::3])
def test_bytes_needed_is_monotone_in_chunk_rows(S, A, O, dtype):
    V, B = 6000, 256
    last = 0
    for rows in list(range(4, 400, 4)) + list(range(400, V, 248)):
        got_rows, n, need = gamma_tiling_plan(S, A, O, V, B, dtype, AMPLE, chunk_rows=rows)
        assert got_rows == rows and n == -(-V // rows) and n > 1
        assert need >= last, (rows, need, last)
        last = need
    # a requested size is rounded up to a multiple of 4; at or beyond V it is one chunk, which needs no score matrix
    assert gamma_tiling_plan(S, A, O, V, B, dtype, AMPLE, chunk_rows=101)[0] == 104
    rows, n, need = gamma_tiling_plan(S, A, O, V, B, dtype, AMPLE, chunk_rows=V + 100)
    assert n == 1 and need == whole_bytes(S, A, O, V, B, dtype)
    # an explicit size that does not fit the budget is refused too
    with pytest.raises(MemoryError):
        gamma_tiling_plan(S, A, O, V, B, dtype, last - 1, chunk_rows=V - 4 - V % 4)


def test_sea_robin_shape_fits_a_fraction_of_gamma():
    """|S| = 61875, A*O = 48... the reference died allocating 21.95 GB of Gamma at |V| = 1386; with 4 GiB for the scoring
    stage the planner tiles it, and every byte it counts stays within the budget."""
    S, A, O, V, B = 61875, 16, 3, 1386, 300
    gamma_whole = A * O * (V + 1) * 61888 * 4
    assert whole_bytes(S, A, O, V, B, 'f32') > gamma_whole
    rows, n, need = gamma_tiling_plan(S, A, O, V, B, 'f32', 4 << 30)
    assert n > 1 and need <= 4 << 30 and n * rows >= V


def test_bad_arguments():
    for args in ((0, 2, 2, 10, 10), (600, 0, 2, 10, 10), (600, 2, -1, 10, 10), (600, 2, 2, 0, 10), (600, 2, 2, 10, 0)):
        with pytest.raises(ValueError):
            gamma_tiling_plan(*args, 'f32', AMPLE)
    with pytest.raises(ValueError):
        gamma_tiling_plan(600, 2, 2, 10, 10, 'f32', -1)
    with pytest.raises(ValueError):
        gamma_tiling_plan(600, 2, 2, 10, 10, 'f32', AMPLE, chunk_rows=-4)
    with pytest.raises(ValueError):
        gamma_tiling_plan(600, 2, 2, 10, 10, 'f16', AMPLE)
    with pytest.raises(ValueError):
        gamma_tiling_plan(600, 1000, 1000, 10**6, 10, 'f32', AMPLE)      # A*O*(V+1) beyond int32
    lib = eng.load_library()
    out = C.c_int64(0)
    assert lib.pbvi_gamma_tiling_plan(600, 2, 2, 10, 10, 2, AMPLE, C.byref(out), C.byref(out), C.byref(out)) == -1
    assert lib.pbvi_gamma_tiling_plan(600, 2, 2, 10, 10, 0, AMPLE, None, C.byref(out), C.byref(out)) == -1
    assert lib.pbvi_set_gamma_tiling(None, 1, 0) == -1 and b'handle' in lib.pbvi_last_error()


def test_stats_struct_mirrors_the_header():
    assert eng.PbviStats._fields_[-1] == ('gamma_chunks', C.c_int32)
