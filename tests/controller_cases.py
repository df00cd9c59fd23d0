"""Controllers, starts and independent references shared by ``test_controller.py`` and ``test_controller_device.py`` (no
tests here).

A controller is ``(node_action [N], node_succ [N,O])``.  ``dense_sweep`` is one Jacobi sweep written a second way -- RTO
scattered into the dense ``[S,A,O,S]`` tensor of ``fib_cases.dense_rto``, one matrix-vector product per (node, observation)
-- and ``exact_rows`` solves the fixed point as one dense linear system of N * S unknowns with ``np.linalg.solve``: neither
shares a loop, a gather or a summation order with ``pomdp.controller_numpy``.
"""
import numpy as np

import fib_cases as fc
from pomdp_pbvi_exploration_amd import pessimistic_start


def blind(A, O):
    """One node per action that is its own successor under every observation: "always take action a"."""
    return np.arange(A), np.tile(np.arange(A)[:, None], (1, O))


def random_controller(N, A, O, seed):
    """Seeded random actions and successors (actions may repeat or be absent; a node may be its own successor)."""
    rng = np.random.default_rng(1000 * N + 10 * A + O + seed)
    return rng.integers(0, A, N), rng.integers(0, N, (N, O))


def shifting(N, A, O):
    """``succ[n][o] = (n + 1 + o) % N`` for o < N - 1: with N > O no node is its own successor, so rows computed from a
    node's own old row instead of its successors' are wrong."""
    assert N > O
    return np.arange(N) % A, (np.arange(N)[:, None] + 1 + np.arange(O)[None, :]) % N


def shape(t):
    return t.reachable_transitional_observation_table.shape                 # (S, A, O, R)


def starts(t, gamma, N, seed=0):
    """``{'pessimistic': min ER / (1 - gamma), 'negative': N(0,1) - 3}``: the start of every solver here, and rows that
    differ from node to node and from state to state."""
    S = shape(t)[0]
    return {'pessimistic': pessimistic_start(t, gamma, N),
            'negative': np.random.default_rng(seed).normal(size=(N, S)) - 3.0}


# --------------------------------------------------------------------------- #
# Independent references
# --------------------------------------------------------------------------- #
def dense_sweep(D, er, node_action, node_succ, V, gamma):
    """One sweep on ``V [N,S]`` through the dense tensor ``D [S,A,O,S]``: ``(rows [N,S], change)``."""
    O = D.shape[2]
    new = np.empty_like(V)
    for n, a in enumerate(node_action):
        new[n] = er[:, a] + gamma * sum(D[:, a, o, :] @ V[node_succ[n, o]] for o in range(O))
    return new, float(np.max(np.abs(new - V)))


def exact_rows(t, node_action, node_succ, gamma):
    """The controller's value ``[N,S]``: the solution of ``(I - gamma M) v = b`` with
    ``M[(n,s),(n',s')] = sum_{o: succ[n][o] = n'} D[s,a_n,o,s']`` and ``b[(n,s)] = ER[s,a_n]``."""
    S, A, O, R = shape(t)
    N = len(node_action)
    assert N * S < 2000, 'keep the dense system small'
    D = fc.dense_rto(t)
    M = np.zeros((N, S, N, S))
    for n, a in enumerate(node_action):
        for o in range(O):
            M[n, :, node_succ[n, o], :] += D[:, a, o, :]
    b = t.expected_rewards_table[:, node_action].T.reshape(N * S)
    v = np.linalg.solve(np.eye(N * S) - gamma * M.reshape(N * S, N * S), b)
    return v.reshape(N, S)
