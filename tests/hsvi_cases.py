"""Point sets, belief rows and derived error bounds shared by ``test_hsvi_device.py`` (no tests here).

The bounds are derived from the summation orders and the number formats, never fitted to observed differences:

``sawtooth_bound``  ``gap_i`` is passed in and ``r_i = min b/p`` is an exact minimum of correctly rounded quotients, so both
    are bit-exact between host and device.  What differs is ``v0 = sum_s b[s] c[s]``, summed in another order with possibly
    fused multiply-adds: at most ``8 * S * 2^-53 * sum_s |b[s] c[s]|`` (the bar of ``tests/test_infotaxis.py``).  ``w_i = v0 +
    gap_i * r_i`` then rounds twice on each side, ``2^-52 * (|v0| + |gap_i r_i|)`` at the most.  Floored at 1e-15.

``successor_bounds``  the device's normaliser adds the masses of 256-state blocks in block order, NumPy pairwise: two sums
    of S non-negative terms, each within ``S * 2^-53`` (relative) of the exact sum, and one rounded division each, so a
    successor entry differs by ``eps_b = (2 S + 2) * 2^-53`` relative; an fp32 engine rounds the quotient to fp32, which may
    move it by one fp32 ulp more, ``2^-23``.  ``v0`` and every ``r_i`` inherit that relative perturbation, the minimum over
    points is perturbed by no more than its largest term: ``eps_b * (sum |b c| + max_i |gap_i| r_i)`` on top of the sawtooth
    bound.  ``Z`` itself is a re-ordered sum of S terms: ``8 * S * 2^-53 * Z``.  ``Q = b . ER + gamma * sum_o Z * value`` adds
    the re-ordered reward sum, ``8 * S * 2^-53 * sum |b ER|``, the two factors' bounds, and O + 1 roundings of the result.
"""
from types import SimpleNamespace

import numpy as np

import model_cases as mc
import test_device_rollout as tdr
from pomdp_pbvi_exploration_amd.pomdp import _rollout_tables, sawtooth_numpy

EPS = 2.0 ** -53
SUPPORTS = (1, 63, 64, 65, None)          # non-zeros of a point, cycled; None = every state
BIG_S = 2053                              # just above the 2048 states one x-block of the push kernels walks


def r32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


_BIG = {}


def get_case(name):
    """``test_device_rollout.get_case`` plus ``'identity_big'``: a ``model_cases.STRUCTURES`` model with S = 2053."""
    if name != 'identity_big':
        return tdr.get_case(name)
    if name not in _BIG:
        rng = np.random.default_rng(2053)
        rs, rto = mc.STRUCTURES['identity'](BIG_S, A=2, O=2)
        m = tdr._tables(BIG_S, 2, 2, 1, rs, rto, rng.normal(size=(BIG_S, 2)), [5])
        _BIG[name] = SimpleNamespace(m=m, gamma=0.95, alpha=rng.normal(size=(5, BIG_S)), acts=rng.integers(0, 2, 5),
                                     b0=np.full((1, BIG_S), 1.0 / BIG_S), s0=np.zeros(1, dtype=np.int64))
    return _BIG[name]


def corner_values(rng, S):
    return rng.normal(size=S) * 3.0 + 10.0


def make_points(rng, S, P, corner, supports=SUPPORTS):
    """``(points [P,S], values [P], gaps [P])``: supports of 1, 63, 64, 65 and S states in turn (clipped to S), entries
    representable in fp32 (so that a copy of a point is the same number in both engines), every point below the corner
    interpolation by a gap in [-2, -0.1]; ``gaps`` is computed once, here, as the caller of the engine must.  (A successor
    can collapse onto one state and so equal a one-state point: ``supports=SUPPORTS[1:]`` where no hit may occur.)"""
    pts = np.zeros((P, S))
    for i in range(P):
        k = supports[i % len(supports)]
        k = S if k is None else min(k, S)
        s = rng.choice(S, size=k, replace=False)
        w = rng.random(k) + 0.05
        pts[i, s] = w / w.sum()
    pts = r32(pts)
    values = pts @ corner - rng.uniform(0.1, 2.0, size=P)
    return pts, values, values - pts @ corner


def make_rows(rng, S, B, points, n_hit):
    """B belief rows (fp32-representable): copies of points inside and outside the hit window, the uniform belief, a row
    whose support misses point 0's, random sparse rows -- as many of these as B allows, in this order of preference."""
    P = points.shape[0]
    rows = []
    if P and n_hit > 0:
        rows.append(points[n_hit - 1])                        # the last point the hit test may see
    rows.append(np.full(S, 1.0 / S))
    if P:
        free = np.flatnonzero(points[0] == 0)
        lone = np.zeros(S)
        lone[free[0] if free.size else 0] = 1.0               # (point 0 covers every state only when S == 1)
        rows.append(lone)
    if P > n_hit:
        rows.append(points[P - 1])                            # a copy of a point OUTSIDE the window: no hit
    if P and n_hit > 1:
        rows.append(points[0])
    while len(rows) < B:
        rows.append(mc.sparse_beliefs(rng, 1, S, density=0.3)[0])
    return r32(np.array(rows[:B]))


def w_matrix(points, gaps, corner, rows, n):
    """``(v0 [B], W [B,n], M [B])``: the host's ``w_i`` of the first n points and ``M = max_i |gap_i| r_i`` (0 for n = 0)."""
    v0 = rows @ corner
    W = np.empty((rows.shape[0], n))
    M = np.zeros(rows.shape[0])
    with np.errstate(divide='ignore', invalid='ignore'):
        for i in range(n):
            s = np.flatnonzero(points[i] > 0)
            r = np.min(rows[:, s] / points[i, s], axis=1)
            W[:, i] = v0 + gaps[i] * r
            M = np.maximum(M, np.abs(gaps[i]) * r)
    return v0, W, M


def sawtooth_bound(S, corner, rows, v0, M):
    return np.maximum(8.0 * S * EPS * (np.abs(rows) @ np.abs(corner)) + 2.0 * EPS * (np.abs(v0) + M), 1e-15)


def successor_bounds(m, dtype, points, gaps, corner, rows, gamma, n_visible, host):
    """``(tol_q [n,A], tol_z [n,A,O], tol_value [n,A,O])`` for ``pbvi_upper_q`` against ``upper_q_numpy``'s ``host = (Q, action, Z,
    value, hit)`` on ``rows`` (the module docstring has the derivation)."""
    t = _rollout_tables(m)
    S, A, O, R = t.state_count, t.action_count, t.observation_count, t.reachable_state_count
    cast = np.float32 if dtype == 'f32' else np.float64
    rto = np.asarray(t.reachable_transitional_observation_table).astype(cast).astype(np.float64)
    er = np.asarray(t.expected_rewards_table).astype(cast).astype(np.float64)
    rs = np.asarray(t.reachable_states).astype(np.int64)
    _, _, Z, value, _ = host
    n = rows.shape[0]
    eps_b = (2.0 * S + 2.0) * EPS + (2.0 ** -23 if dtype == 'f32' else 0.0)
    tol_z = np.maximum(8.0 * S * EPS * Z, 1e-15)
    tol_v = np.zeros((n, A, O))
    for a in range(A):
        for o in range(O):
            for k in range(n):
                if Z[k, a, o] == 0:
                    continue
                u = np.bincount(rs[:, a, :].ravel(), weights=(rows[k][:, None] * rto[:, a, o, :]).ravel(), minlength=S)
                succ = (u / Z[k, a, o]).astype(cast).astype(np.float64)[None, :]
                v0, _, M = w_matrix(points, gaps, corner, succ, n_visible)
                tol_v[k, a, o] = sawtooth_bound(S, corner, succ, v0, M)[0] + eps_b * (np.abs(succ[0]) @ np.abs(corner) + M[0])
    val = np.where(Z == 0, 0.0, value)
    terms = tol_z * np.abs(val) + Z * tol_v + 2.0 * EPS * np.abs(Z * val)
    tol_q = 8.0 * S * EPS * (np.abs(rows) @ np.abs(er)) + gamma * terms.sum(axis=2) + (O + 1) * 2.0 * EPS * (
        np.abs(rows @ er) + gamma * np.abs(Z * val).sum(axis=2))
    return np.maximum(tol_q, 1e-15), tol_z, tol_v
