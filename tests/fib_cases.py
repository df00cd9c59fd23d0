"""Models, starts and independent references shared by ``test_fib.py`` and ``test_fib_device.py`` (no tests here).

``dense_sweep`` is the Fast Informed Bound written a second way -- RTO scattered into a dense ``[S,A,O,S]`` tensor, one
matrix product per sweep -- so it shares no loop, no gather and no summation order with ``pomdp.fib_numpy``.
``exact_value`` is the k-step optimal value of a belief by brute-force recursion over the belief tree, and
``mdp_sweeps`` the MDP's Q-values after k sweeps: the two sides of the sandwich the bound must sit in.
"""
import os
from types import SimpleNamespace

import numpy as np

import model_cases as mc
from conftest import GOLDEN
from pomdp_pbvi_exploration_amd import load_POMDP_file

FILE_MODELS = {'tiger': 'tiger.95.POMDP', 'tiger-grid': 'tiger-grid.POMDP', 'hallway': 'hallway.POMDP'}
_FILES = {}
# (A, O, R) around k_fib_sweep<TW, PAIRS>'s a'-tiles: TW = 4 up to A = 4, else 8; double2 loads for even A.  Per instantiation
# a full tile, a short one and (TW = 8) a full tile followed by a tail, over which the running maximum is carried:
#   TW 4 scalar: 1, 3            TW 4 pairs: 2, 4
#   TW 8 scalar: 5, 7 (short), 9 (full + 1), 17 (two full + 1)
#   TW 8 pairs:  6 (short), 8 (full), 10, 12 (full + pair tail), 16 (two full)
ACTION_CASES = ((1, 1, 1), (2, 2, 2), (7, 5, 4), (8, 1, 2), (9, 2, 4), (17, 5, 1),
                (3, 2, 2), (4, 3, 2), (5, 2, 3), (6, 2, 2), (10, 2, 2), (12, 1, 3), (16, 2, 1))


def tables(rs, rto, er):
    """The three tables under ``Model``'s attribute names (what ``fib_numpy`` reads)."""
    return SimpleNamespace(reachable_states=np.asarray(rs, dtype=np.int64),
                           reachable_transitional_observation_table=np.asarray(rto, dtype=np.float64),
                           expected_rewards_table=np.asarray(er, dtype=np.float64))


def structure_case(name, S, **kw):
    """``model_cases.STRUCTURES[name]`` at S states (its default A and O unless given) with normal expected rewards."""
    rs, rto = mc.STRUCTURES[name](S, **kw)
    er = np.random.default_rng(1).normal(size=rto.shape[:2])
    return tables(rs, rto, er)


def random_tables(seed):
    """The model of ``model_cases.random_case(seed)`` and its discount."""
    S, A, O, R, rs, rto, er, _, _, gamma = mc.random_case(seed)
    return tables(rs, rto, er), gamma


def dense_random_case(A, O, R, S=70, seed=0):
    """Random successors and strictly positive RTO at a chosen action count (the a'-tile edges of the kernel)."""
    rng = np.random.default_rng(100 * A + 10 * O + R + seed)
    rs = rng.integers(0, S, (S, A, R))
    rto = rng.random((S, A, O, R)) + 0.01
    rto /= rto.sum(axis=(2, 3), keepdims=True)
    return tables(rs, rto, rng.normal(size=(S, A)))


def starts(t, seed=0):
    """``{'negative': N(0,1) - 3, 'rewards': ER.T}``: the first is mostly negative, so a maximum that started at 0
    shows; the second is the start of every solver here."""
    S, A = t.expected_rewards_table.shape
    return {'negative': np.random.default_rng(seed).normal(size=(A, S)) - 3.0,
            'rewards': np.ascontiguousarray(t.expected_rewards_table.T)}


def file_model(key):
    """``(Model, gamma)`` of a committed example file, loaded once."""
    if key not in _FILES:
        model, solver = load_POMDP_file(os.path.join(GOLDEN, 'models', FILE_MODELS[key]))
        _FILES[key] = (model, solver.gamma)
    return _FILES[key]


# --------------------------------------------------------------------------- #
# Independent references
# --------------------------------------------------------------------------- #
def dense_rto(t):
    """``D[s,a,o,s'] = sum_{r: rs[s,a,r] = s'} RTO[s,a,o,r]``."""
    rs, rto = t.reachable_states, t.reachable_transitional_observation_table
    S, A, O, R = rto.shape
    D = np.zeros((S, A, O, S))
    s, a, o, r = np.meshgrid(np.arange(S), np.arange(A), np.arange(O), np.arange(R), indexing='ij')
    np.add.at(D, (s, a, o, rs[s, a, r]), rto)
    return D


def dense_sweep(D, er, Q, gamma):
    """One sweep on ``Q [A,S]`` through the dense tensor: ``(rows [A,S], change)``."""
    S, A, O, _ = D.shape
    inner = (D.reshape(S * A * O, S) @ Q.T).reshape(S, A, O, A)               # [s,a,o,a']
    new = (er + gamma * inner.max(axis=3).sum(axis=2)).T
    return new, float(np.max(np.abs(new - Q)))


def mdp_sweeps(t, gamma, k):
    """MDP Q-values ``[A,S]`` after k sweeps from 0: ``Q_k = ER + gamma * sum_r P max_a' Q_{k-1}``, ``P = sum_o RTO``."""
    rs, rto, er = t.reachable_states, t.reachable_transitional_observation_table, t.expected_rewards_table
    P = rto.sum(axis=2)
    Q = np.zeros(er.shape)
    for _ in range(k):
        Q = er + gamma * np.einsum('sar,sar->sa', P, Q.max(axis=1)[rs])
    return Q.T


def exact_value(t, gamma, k, b):
    """The optimal k-step value of belief ``b`` (terminal value 0) by recursion over the whole belief tree.  The value is
    positively homogeneous, so the recursion runs on unnormalised successors ``u_ao[s'] = sum_{s,r} u[s] RTO[s,a,o,r]``
    and never divides: ``V_k(u) = max_a (u . ER[:,a] + gamma * sum_o V_{k-1}(u_ao))``."""
    rs, rto, er = t.reachable_states, t.reachable_transitional_observation_table, t.expected_rewards_table
    S, A, O, R = rto.shape

    def V(u, depth):
        if depth == 0:
            return 0.0
        best = -np.inf
        for a in range(A):
            tail = 0.0
            if depth > 1:
                for o in range(O):
                    nxt = np.bincount(rs[:, a, :].ravel(), weights=(u[:, None] * rto[:, a, o, :]).ravel(), minlength=S)
                    tail += V(nxt, depth - 1)
            best = max(best, float(u @ er[:, a]) + gamma * tail)
        return best

    return V(np.asarray(b, dtype=np.float64), k)
