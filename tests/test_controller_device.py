"""``pbvi_controller_value_iteration`` against ``pomdp.controller_numpy``: the kernel and the restatement share one
definition of a sweep, operation for operation, so rows and changes are compared with ``np.array_equal`` -- on the wave and
block edges of S, node counts around the node tile of 4 with several nodes per action and actions without a node, random
models, a controller in which no node is its own successor, across the seam between two enqueued batches of sweeps, and
through ``Blind_Solver``.  Every shape is small; every case takes well under a second."""
import gc

import numpy as np
import pytest

import controller_cases as cc
import fib_cases as fc
import model_cases as mc
from pomdp_pbvi_exploration_amd import Blind_Solver, controller_numpy, pessimistic_start
from pomdp_pbvi_exploration_amd.engine import controller_value_iteration, debug_live_bytes

pytestmark = pytest.mark.gpu

EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 600)                # around one wave (64) and one block (256) of states
ACTION_CASES = ((1, 1, 1), (2, 2, 2), (7, 5, 4), (9, 2, 4), (17, 5, 1))     # (A, O, R)
NODE_COUNTS = (1, 3, 4, 5, 9)                                   # around a node tile of 4
BATCH = 64                                                      # sweeps the entry enqueues between two synchronisations


def device(t, na, ns, v0, gamma, limit, horizon):
    return controller_value_iteration(t.reachable_states, t.reachable_transitional_observation_table,
                                      t.expected_rewards_table, na, ns, v0, gamma, limit, horizon)


def assert_same_sweeps(t, na, ns, gamma, tag):
    for start, v0 in cc.starts(t, gamma, len(na)).items():
        want_rows, want_changes = controller_numpy(t, na, ns, v0, gamma, 0.0, 3)
        rows, changes = device(t, na, ns, v0, gamma, 0.0, 3)
        assert len(changes) == 3, (tag, start)
        assert np.array_equal(changes, want_changes), (tag, start, changes, want_changes)
        assert np.array_equal(rows, want_rows), (tag, start, np.abs(rows - want_rows).max())


@pytest.mark.parametrize('S', EDGE_SIZES)
@pytest.mark.parametrize('name', list(mc.STRUCTURES))
def test_three_sweeps_bit_equal_on_structures(name, S):
    t = fc.structure_case(name, S)
    _, A, O, _ = cc.shape(t)
    assert_same_sweeps(t, *cc.blind(A, O), 0.95, (name, S, 'blind'))
    assert_same_sweeps(t, *cc.random_controller(5, A, O, S), 0.95, (name, S, 'random5'))


@pytest.mark.parametrize('N', NODE_COUNTS)
@pytest.mark.parametrize('A,O,R', ACTION_CASES)
def test_three_sweeps_bit_equal_around_the_node_tile(A, O, R, N):
    assert_same_sweeps(fc.dense_random_case(A, O, R), *cc.random_controller(N, A, O, 0), 0.95, (A, O, R, N))


@pytest.mark.parametrize('seed', range(8))
def test_three_sweeps_bit_equal_on_random_models(seed):
    t, gamma = fc.random_tables(seed)
    _, A, O, _ = cc.shape(t)
    assert_same_sweeps(t, *cc.blind(A, O), gamma, (seed, 'blind'))
    assert_same_sweeps(t, *cc.random_controller(7, A, O, seed), gamma, (seed, 'random7'))


@pytest.mark.parametrize('name', list(mc.STRUCTURES))
def test_successors_are_followed(name):
    """N = 4, ``succ[n][o] = (n + 1 + o) % N``: no node is its own successor, so an implementation that ignores ``succ``
    cannot pass."""
    t = fc.structure_case(name, 257)
    _, A, O, _ = cc.shape(t)
    na, ns = cc.shifting(4, A, O)
    assert not (ns == np.arange(4)[:, None]).any()
    assert_same_sweeps(t, na, ns, 0.95, name)


# --------------------------------------------------------------------------- #
# Stopping
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('name', list(mc.STRUCTURES))
def test_stopping_across_the_batch_seam(name):
    """The run converges in the second batch: the sweeps enqueued behind the converged one must leave its rows alone, and
    the entry must report the sweep that met the limit, not the last one it enqueued."""
    t = fc.structure_case(name, 257)
    _, A, O, _ = cc.shape(t)
    na, ns = cc.blind(A, O)
    v0 = pessimistic_start(t, 0.9, A)
    want_rows, want_changes = controller_numpy(t, na, ns, v0, 0.9, 1e-4, 200)
    assert BATCH < len(want_changes) < 2 * BATCH, len(want_changes)
    rows, changes = device(t, na, ns, v0, 0.9, 1e-4, 200)
    assert len(changes) == len(want_changes)
    assert np.array_equal(changes, want_changes)
    assert np.array_equal(rows, want_rows)


@pytest.mark.parametrize('horizon', (0, 1, 10, BATCH, BATCH + 6))
def test_horizon_cuts_the_run(horizon):
    """No sweep (``v0`` comes back), one, and horizons that end the run before it converges: inside the first batch, at the
    seam and behind it."""
    t = fc.structure_case('ragged', 257)
    _, A, O, _ = cc.shape(t)
    na, ns = cc.blind(A, O)
    v0 = pessimistic_start(t, 0.9, A)
    want_rows, want_changes = controller_numpy(t, na, ns, v0, 0.9, 1e-4, horizon)
    assert len(want_changes) == horizon and (horizon == 0 or want_changes[-1] >= 1e-4)
    rows, changes = device(t, na, ns, v0, 0.9, 1e-4, horizon)
    assert changes.shape == (horizon,) and np.array_equal(changes, want_changes)
    assert np.array_equal(rows, want_rows)
    if horizon == 0:
        assert np.array_equal(rows, v0)


# --------------------------------------------------------------------------- #
# Solver and memory
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('key', list(fc.FILE_MODELS))
def test_solver_on_the_device_equals_the_host(key):
    model, gamma = fc.file_model(key)
    host, hist_host = Blind_Solver(gamma=gamma, eps=1e-3).solve(model, use_gpu=False, print_progress=False)
    dev, hist_dev = Blind_Solver(gamma=gamma, eps=1e-3).solve(model, use_gpu=True, print_progress=False)
    assert np.array_equal(dev.alpha_vector_array, host.alpha_vector_array)
    assert np.array_equal(dev.actions, host.actions)
    assert hist_dev.value_function_changes == hist_host.value_function_changes
    assert len(hist_host.value_function_changes) > 0


def test_a_call_leaves_no_device_memory_behind():
    t = fc.structure_case('hub', 600)
    _, A, O, _ = cc.shape(t)
    na, ns = cc.random_controller(9, A, O, 0)
    v0 = pessimistic_start(t, 0.9, 9)
    gc.collect()
    base = debug_live_bytes()
    device(t, na, ns, v0, 0.9, 1e-4, 200)
    assert debug_live_bytes() == base
    device(t, na, ns, v0, 0.9, 1e-4, 0)
    assert debug_live_bytes() == base
