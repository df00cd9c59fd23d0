"""``pbvi_mdp_value_iteration`` against a restatement of its sweep written here as explicit loops: the successor sum in the
order of r, the maximum over the actions in the order of a, no product fused with a sum -- what ``k_vi_sweep`` does,
operation for operation, so rows and changes are compared with ``np.array_equal`` -- on the wave and block edges of S,
(A, R) other than 1, a mostly negative start, across the seam between two enqueued batches of sweeps, and for horizons that
cut the run (0 included).  Every shape is small; every case takes well under a second."""
import gc

import numpy as np
import pytest

import fib_cases as fc
import model_cases as mc
from pomdp_pbvi_exploration_amd.engine import debug_live_bytes, mdp_value_iteration

pytestmark = pytest.mark.gpu

EDGE_SIZES = (1, 63, 64, 65, 255, 256, 257, 600)                # around one wave (64) and one block (256) of states
SHAPE_CASES = ((1, 1, 1), (2, 2, 2), (7, 5, 4), (9, 2, 4))      # (A, O, R) of fib_cases.dense_random_case
BATCH = 64                                                      # sweeps the entry enqueues between two synchronisations


def mdp_tables(t):
    """``(reachable_states, P = sum_o RTO, ER)``: what ``VI_Solver`` and ``test_engine_memory.py`` feed the entry."""
    return t.reachable_states, t.reachable_transitional_observation_table.sum(axis=2), t.expected_rewards_table


def starts(S, seed=0):
    """Zeros, and a mostly negative start, so that a maximum which started at 0 shows."""
    return {'zeros': np.zeros(S), 'negative': np.random.default_rng(seed).normal(size=S) - 3.0}


def vi_numpy(t, v0, gamma, limit, horizon):
    """``(rows [A,S], changes)`` of at most ``horizon`` sweeps from ``v0 [S]``, stopping behind the first sweep whose change
    is below ``limit``; rows are zero when no sweep ran."""
    rs, P, er = mdp_tables(t)
    S, A, R = rs.shape
    v = np.array(v0, dtype=np.float64)
    rows = np.zeros((A, S))
    changes = []
    for _ in range(horizon):
        acc = P[:, :, 0] * v[rs[:, :, 0]]
        for r in range(1, R):
            acc = acc + P[:, :, r] * v[rs[:, :, r]]
        rows = np.ascontiguousarray((er + gamma * acc).T)
        best = rows[0]
        for a in range(1, A):
            best = np.where(rows[a] > best, rows[a], best)
        changes.append(float(np.max(np.abs(best - v))))
        v = best
        if changes[-1] < limit:
            break
    return rows, np.array(changes, dtype=np.float64)


def device(t, v0, gamma, limit, horizon):
    rs, P, er = mdp_tables(t)
    return mdp_value_iteration(rs, P, er, v0, gamma, limit, horizon)


def assert_same_sweeps(t, gamma, tag):
    for start, v0 in starts(t.expected_rewards_table.shape[0]).items():
        want_rows, want_changes = vi_numpy(t, v0, gamma, 0.0, 3)
        rows, changes = device(t, v0, gamma, 0.0, 3)
        assert len(changes) == 3, (tag, start)
        assert np.array_equal(changes, want_changes), (tag, start, changes, want_changes)
        assert np.array_equal(rows, want_rows), (tag, start, np.abs(rows - want_rows).max())


@pytest.mark.parametrize('S', EDGE_SIZES)
@pytest.mark.parametrize('name', list(mc.STRUCTURES))
def test_three_sweeps_bit_equal_on_structures(name, S):
    assert_same_sweeps(fc.structure_case(name, S), 0.95, (name, S))


@pytest.mark.parametrize('A,O,R', SHAPE_CASES)
def test_three_sweeps_bit_equal_on_dense_shapes(A, O, R):
    assert_same_sweeps(fc.dense_random_case(A, O, R), 0.95, (A, O, R))


# --------------------------------------------------------------------------- #
# Stopping
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('name', list(mc.STRUCTURES))
def test_stopping_across_the_batch_seam(name):
    """The run converges in the second batch: the sweeps enqueued behind the converged one must leave its rows alone, and
    the entry must report the sweep that met the limit, not the last one it enqueued."""
    t = fc.structure_case(name, 257)
    v0 = np.zeros(257)
    want_rows, want_changes = vi_numpy(t, v0, 0.9, 1e-4, 200)
    assert BATCH < len(want_changes) < 2 * BATCH, len(want_changes)
    rows, changes = device(t, v0, 0.9, 1e-4, 200)
    assert len(changes) == len(want_changes)
    assert np.array_equal(changes, want_changes)
    assert np.array_equal(rows, want_rows)


@pytest.mark.parametrize('horizon', (0, 1, 10, BATCH, BATCH + 6))
def test_horizon_cuts_the_run(horizon):
    """No sweep (the entry succeeds, counts zero iterations and returns rows of 0.0), one, and horizons that end the run
    before it converges: inside the first batch, at the seam and behind it."""
    t = fc.structure_case('ragged', 257)
    v0 = starts(257)['negative']
    want_rows, want_changes = vi_numpy(t, v0, 0.9, 1e-4, horizon)
    assert len(want_changes) == horizon and (horizon == 0 or want_changes[-1] >= 1e-4)
    rows, changes = device(t, v0, 0.9, 1e-4, horizon)
    assert changes.shape == (horizon,) and np.array_equal(changes, want_changes)
    assert np.array_equal(rows, want_rows)
    if horizon == 0:
        assert rows.shape == want_rows.shape and not rows.any() and not np.signbit(rows).any()


# --------------------------------------------------------------------------- #
# Memory
# --------------------------------------------------------------------------- #
def test_a_call_leaves_no_device_memory_behind():
    t = fc.structure_case('hub', 600)
    gc.collect()
    base = debug_live_bytes()
    device(t, np.zeros(600), 0.9, 1e-4, 200)
    assert debug_live_bytes() == base
    device(t, np.zeros(600), 0.9, 1e-4, 0)
    assert debug_live_bytes() == base
