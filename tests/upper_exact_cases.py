"""Exact inputs for the sawtooth's point, tie and hit rules, shared by ``test_upper_exact.py`` (no tests here).

The method: belief rows whose entries are multiples of ``2^-q`` (``q <= 10``) and corner values that are small integers make
``v0 = sum_s b[s] c[s]`` exact in every summation order, fused or not; ``b / p`` is one correctly rounded fp64 division and
``v0 + gap * r`` rounds twice on host and device alike.  ``value``, ``point`` and ``hit`` of ``pbvi_upper_bound`` can then be
compared with ``==`` against ``sawtooth_numpy`` for arbitrary fp32-representable points and arbitrary gaps.  Model tables of
powers of two do the same for the successors of ``pbvi_upper_q``.

A *scene* is one point store and the rows evaluated against it, with a record (``plant``) of what was planted where:

``positions``  the unique minimum of row k sits at a chosen (chunk, wave, slot): point t is ``2 * b_t`` with gap -1e3, so
    ``r_t = 1/2`` and ``w_t = v0 - 500``.  Every other planted point has ``r < 1/2`` on that row (both rows sum to 1), every
    filler point sums to 1 within fp32 rounding, hence ``r <= 1 + 2^-20`` and ``w >= v0 - 2.1``.
``ties``  the same construction with one point stored twice (equal gaps): ``w_i == w_j`` as floats.  Row ``e_z`` lies off
    the support of every negative-gap point (``r = 0``, ``w == v0``) and on the support of a ``gap == 0`` and a positive-gap
    point: no point may be named.
``hits``  rows that are copies of points at every position class, and points stored twice with DIFFERENT values.
``near``  rows that differ from a point in an entry of the second or third trip of the lane loop only, rows equal to a point
    on its support with mass elsewhere, rows on a strict subset of a point's support, one-state points.
``seams``  the 256-state trips of ``k_ub_row``: mass on the last state only and on states 0, 256 and 512.
"""
from types import SimpleNamespace

import numpy as np

import test_device_rollout as tdr
from hsvi_cases import r32
from pomdp_pbvi_exploration_amd.pomdp import _successor_rows, sawtooth_numpy

UB_PPB = 64            # points one block of k_ub_pairs reduces: UB_PPB of csrc/upper_kernels.h
UB_WAVES = 4           # its waves; wave w walks the points w, w + 4, ... of the chunk (k_ub_pairs, csrc/upper_kernels.hip)
Q = 10                 # rows are multiples of 2^-Q
SUPPORTS = (1, 5, 63, 64, 65, 129, None)      # non-zeros of a dyadic row, cycled; None = every state
POINT_COUNTS = (63, 64, 65, 127, 128, 129, 300)
STATE_COUNTS = (2, 64, 65, 130, 257, 600)
PLANT_GAP = -1e3
# (i, j), i < j, of one point stored twice: one wave at two slots; two waves with the lower index in the higher wave, and
# in the lower wave; two chunks (the second and, where there is one, a later chunk)
PAIRS = ((10, 42), (7, 8), (13, 18), (21, 85), (25, 281))
GAP0_AT, GAP_POS_AT = 6, 9                    # the gap == 0 and the positive-gap point of the 'ties' scene


def position(i):
    """``(chunk, wave, slot)`` of point i in ``k_ub_pairs``."""
    return i // UB_PPB, i % UB_WAVES, (i % UB_PPB) // UB_WAVES


def index_at(chunk, wave, slot):
    return chunk * UB_PPB + slot * UB_WAVES + wave


def position_classes(P):
    """The point indices below P at chunk in {first, second, last}, every wave, its first and its last slot: slot 15, in a
    last chunk that is not full the wave's last point below P."""
    last = (P - 1) // UB_PPB
    out = []
    for chunk in sorted({0, min(1, last), last}):
        for wave in range(UB_WAVES):
            mine = [i for i in range(chunk * UB_PPB + wave, min(P, (chunk + 1) * UB_PPB), UB_WAVES)]
            out += sorted({mine[0], mine[-1]}) if mine else []
    return out


def windows(P):
    """The ``(n_visible, n_hit)`` pairs a store of P points is evaluated under, each clipped to P; the last two have
    ``n_visible`` and ``n_hit`` in different chunks."""
    raw = [(P, P), (0, P), (1, P), (63, 64), (64, 64), (64, 65), (65, 128), (60, 130), (70, 200)]
    out = []
    for v, h in raw:
        w = (min(v, P), min(h, P))
        if w not in out:
            out.append(w)
    return out


def dyadic_rows(rng, S, support, q=Q, n=1):
    """``[n, S]`` rows on ``support`` random states (``None``: all; clipped to S) whose entries are positive multiples of
    ``2^-q`` summing to exactly 1.0: every entry, every partial sum and (``q <= 10 < 24``) its fp32 image are exact."""
    k = S if support is None else min(support, S)
    units = 1 << q
    assert q <= 10 and 1 <= k <= units
    rows = np.zeros((n, S))
    for r in range(n):
        s = np.sort(rng.choice(S, size=k, replace=False))
        rows[r, s] = (1 + rng.multinomial(units - k, np.full(k, 1.0 / k))) / units
    assert np.all(rows.sum(axis=1) == 1.0) and np.array_equal(r32(rows), rows)
    return rows


def integer_corner(rng, S):
    return rng.integers(5, 20, size=S).astype(np.float64)


def filler_points(rng, S, P):
    """P random fp32-representable points that sum to 1 within fp32 rounding, on 5, 63, 64, 65, 129 and S states in turn
    (clipped to S, at least 2), with gaps in [-2, -0.1]; neither dyadic nor exact."""
    pts = np.zeros((P, S))
    for i in range(P):
        k = SUPPORTS[1 + i % (len(SUPPORTS) - 1)]
        k = S if k is None else max(2, min(k, S))
        s = rng.choice(S, size=k, replace=False)
        w = rng.random(k) + 0.05
        pts[i, s] = w / w.sum()
    return r32(pts), rng.uniform(-2.0, -0.1, size=P)


def _distinct(rng, S, n, supports):
    """n pairwise distinct dyadic rows, supports cycled."""
    rows, seen = [], set()
    k = 0
    while len(rows) < n:
        row = dyadic_rows(rng, S, supports[k % len(supports)])[0]
        k += 1
        if row.tobytes() not in seen:
            seen.add(row.tobytes())
            rows.append(row)
    return rows


def _wide(S):
    """Supports of the planted rows: at least two states, so that no planted point is a one-state point."""
    return tuple(sorted({min(S if k is None else max(2, min(k, S)), 1 << Q) for k in SUPPORTS[1:]}))


def _scene(kind, S, P, corner, pts, gaps, rows, plant, values=None):
    rows = np.array(rows)
    if values is None:
        values = pts @ corner + gaps
    return SimpleNamespace(kind=kind, S=S, P=P, corner=corner, points=pts, values=values, gaps=gaps, rows=rows, plant=plant)


def positions_scene(S, P):
    rng = np.random.default_rng(1000 * S + P)
    corner = integer_corner(rng, S)
    pts, gaps = filler_points(rng, S, P)
    classes = position_classes(P)
    rows = _distinct(rng, S, len(classes), _wide(S))
    for t, b in zip(classes, rows):
        pts[t] = 2.0 * b
        gaps[t] = PLANT_GAP
    plant = {'min': [(k, t) for k, t in enumerate(classes)]}
    rows = rows + [dyadic_rows(rng, S, k)[0] for k in SUPPORTS]          # generic rows: fillers decide
    return _scene('positions', S, P, corner, pts, gaps, rows, plant)


def ties_scene(S, P):
    rng = np.random.default_rng(2000 * S + P)
    corner = integer_corner(rng, S)
    pts, gaps = filler_points(rng, S, P)
    pairs = [(i, j) for i, j in PAIRS if j < P]
    rows = _distinct(rng, S, len(pairs), _wide(S))
    values = pts @ corner + gaps
    for (i, j), b in zip(pairs, rows):
        pts[i] = pts[j] = 2.0 * b
        gaps[i] = gaps[j] = PLANT_GAP
        values[i], values[j] = 1.0, 2.0
    z = S - 1
    lone = np.zeros(S)
    lone[z] = 1.0
    for at, p, g in ((GAP0_AT, 0.5, 0.0), (GAP_POS_AT, 0.25, 0.5)):     # w == v0 exactly; w = v0 + 2 > v0
        pts[at] = 0.0
        pts[at, z] = p
        gaps[at] = g
    plant = {'tie': [(k, i, j) for k, (i, j) in enumerate(pairs)], 'v0': [len(rows)]}
    return _scene('ties', S, P, corner, pts, gaps, rows + [lone], plant, values)


def hits_scene(S, P):
    rng = np.random.default_rng(3000 * S + P)
    corner = integer_corner(rng, S)
    pts, gaps = filler_points(rng, S, P)
    classes = position_classes(P)
    pairs = [(i, j) for i, j in PAIRS if j < P]
    own = _distinct(rng, S, len(classes) + len(pairs), _wide(S))
    for t, b in zip(classes, own):
        pts[t] = b
    for (i, j), b in zip(pairs, own[len(classes):]):
        pts[i] = pts[j] = b
    values = pts @ corner + gaps
    for i, j in pairs:
        values[j] = values[i] + 1.0                                     # a wrong hit index shows in `value`
    rows = [pts[t] for t in classes] + [pts[i] for i, _ in pairs]
    plant = {'hit': [(k, t) for k, t in enumerate(classes)] + [(len(classes) + k, i) for k, (i, _) in enumerate(pairs)],
             'dup': pairs}
    return _scene('hits', S, P, corner, pts, gaps, rows, plant, values)


def _bump(row, entry):
    """The row with ``2^-Q`` more at the ``entry``-th state of its support (ascending state order, as the store keeps it)."""
    out = row.copy()
    out[np.flatnonzero(row)[entry]] += 2.0 ** -Q
    return out


def _move(row, first):
    """The row with ``2^-Q`` moved between two entries at or behind ``first`` of its support; no entry becomes zero."""
    s = np.flatnonzero(row)[first:]
    rich = [k for k in range(len(s)) if row[s[k]] >= 2.0 ** (1 - Q)]
    assert rich and len(s) >= 2
    d = rich[0]
    t = d + 1 if d + 1 < len(s) else d - 1
    out = row.copy()
    out[s[d]] -= 2.0 ** -Q
    out[s[t]] += 2.0 ** -Q
    assert np.count_nonzero(out) == np.count_nonzero(row) and np.array_equal(out[:s[0]], row[:s[0]])
    return out


def near_scene(S, P=129):
    """``plant['near']``: rows that are no hit; ``plant['hit']``: (row, point) that are.  Needs S >= 5."""
    rng = np.random.default_rng(4000 * S + P)
    corner = integer_corner(rng, S)
    pts, gaps = filler_points(rng, S, P)
    rows, near, hit = [], [], []

    def put(at, point, copies, others):
        pts[at] = point
        for r in copies:
            hit.append((len(rows), at))
            rows.append(r)
        for r in others:
            near.append(len(rows))
            rows.append(r)

    if S >= 65:                                                       # 65 entries: only the 65th differs (second trip)
        d = dyadic_rows(rng, S, 65)[0]
        put(2, d, [d], [_bump(d, 64)])
    if S >= 129:                                                      # 129 entries: only the 129th differs (third trip)
        d = dyadic_rows(rng, S, 129)[0]
        put(66, d, [d], [_bump(d, 128)])
    if S >= 66:                                                       # up to 200 entries: 2^-Q moved between entries >= 64, >= 128
        d = dyadic_rows(rng, S, min(S, 200))[0]
        put(128, d, [d], [_move(d, 64)] + ([_move(d, 128)] if S >= 130 else []))
    wide = dyadic_rows(rng, S, min(S, 10))[0]                         # superset row: equal on the point's support, mass elsewhere
    part = wide.copy()
    part[np.flatnonzero(wide)[np.count_nonzero(wide) // 2:]] = 0.0
    put(5, part, [], [wide])
    small = dyadic_rows(rng, S, min(S - 2, 5))[0]                     # subset row: the point has two more states
    more = small.copy()
    more[np.flatnonzero(small == 0)[:2]] = 2.0 ** -4
    put(9, more, [], [small])
    a, b, c = 0, S // 2, S - 1                                        # one-state points: 1.0 at a, 0.5 at c
    ea, eb, ec = (np.eye(S)[k] for k in (a, b, c))
    put(12, ea, [ea], [eb, 0.5 * ea + 0.5 * eb])
    put(70, 0.5 * ec, [], [ec])
    return _scene('near', S, P, corner, pts, gaps, rows, {'near': near, 'hit': hit})


def seams_scene(S, P=65):
    """Rows with their mass on the last state and on the first states of the 256-state trips of ``k_ub_row``; points 3 and 4
    are copies of them (a miscounted ``bnnz`` loses the hit)."""
    rng = np.random.default_rng(5000 * S + P)
    corner = integer_corner(rng, S)
    pts, gaps = filler_points(rng, S, P)
    last = np.eye(S)[S - 1]
    at = [s for s in (0, 256, 512) if s < S]
    trips = np.zeros(S)
    trips[at] = {1: [1.0], 2: [0.5, 0.5], 3: [0.5, 0.25, 0.25]}[len(at)]
    pts[3], pts[4] = last, trips
    rows = [last, trips, dyadic_rows(rng, S, None)[0], 0.5 * last + 0.5 * trips]
    return _scene('seams', S, P, corner, pts, gaps, rows, {'hit': [(0, 3), (1, 4)]})


SCENES = {'positions': positions_scene, 'ties': ties_scene, 'hits': hits_scene, 'near': near_scene, 'seams': seams_scene}
_CACHE = {}


def scene(kind, S, P):
    """The scene, built once, with ``host[(n_visible, n_hit)] = sawtooth_numpy(...)`` filled in by ``host_result``."""
    key = (kind, S, P)
    if key not in _CACHE:
        _CACHE[key] = SCENES[kind](S, P)
        _CACHE[key].host = {}
    return _CACHE[key]


def host_result(sc, n_visible, n_hit):
    key = (n_visible, n_hit)
    if key not in sc.host:
        out = sawtooth_numpy(sc.points, sc.values, sc.gaps, sc.corner, sc.rows, n_visible, n_hit)
        for a in out:
            a.setflags(write=False)
        sc.host[key] = out
    return sc.host[key]


# --------------------------------------------------------------------------------------------------------------------- #
# exact models
# --------------------------------------------------------------------------------------------------------------------- #
TWINS = (1, 3)                                                        # two actions with identical tables
_MODELS = {}


def exact_model(kind, S=130):
    """``SimpleNamespace(m, gamma, alpha, twins)`` of a model whose tables are powers of two, ``kind = 'R<1|2>-<tier>'`` or
    ``'seam'``.

    ``R = 1``: every action is a permutation of the states.  ``R = 2``: state s goes to ``pi(s) // 2`` and to ``pi(s)`` with
    probability 1/2 each, so successors merge states.  Observation probabilities ``(1/2, 1/4, 1/4, 0)``: the last observation
    is impossible under every action.  ``tier = 'power'``: the same law at every landing state, so ``Z`` is a power of two
    and every successor of a dyadic row is dyadic (``rto`` holds 1/4 and 1/8 with R = 2).  ``tier = 'dyadic'``: odd landing
    states observe with ``(1/4, 1/4, 1/2, 0)``; ``u`` and ``Z`` stay exact sums of multiples of ``2^-(Q+3)``, the quotient
    rounds once.  ``ER`` is integer, ``gamma = 0.5``, actions ``TWINS`` are the same tables.
    ``'seam'``: S = 4, A = O = 8 (``A * O = 64``), R = 1, tier 'power'."""
    key = (kind, S)
    if key in _MODELS:
        return _MODELS[key]
    rng = np.random.default_rng(sum(map(ord, kind)) + S)
    if kind == 'seam':
        S, A, R, tier = 4, 8, 1, 'power'
        law = np.array([[2.0 ** -k for k in (1, 2, 3, 4, 5, 6, 6)] + [0.0]] * 2)
        perms = [(np.arange(S) * (1 + 2 * (a % 2)) + a // 2) % S for a in range(A)]
        perms[7] = perms[1]
        twins = (1, 7)
    else:
        R, tier = int(kind[1]), kind[3:]
        assert kind[0] == 'R' and R in (1, 2) and tier in ('power', 'dyadic') and np.gcd(7, S) == 1
        A, twins = 4, TWINS
        law = np.array([[0.5, 0.25, 0.25, 0.0], [0.25, 0.25, 0.5, 0.0] if tier == 'dyadic' else [0.5, 0.25, 0.25, 0.0]])
        s = np.arange(S)
        perms = [(s + 1) % S, (7 * s + 3) % S, S - 1 - s, (7 * s + 3) % S]
    O = law.shape[1]
    rs = np.zeros((S, A, R), dtype=np.int64)
    rto = np.zeros((S, A, O, R))
    for a, pi in enumerate(perms):
        lands = [pi] if R == 1 else [pi // 2, pi]
        for r, to in enumerate(lands):
            rs[:, a, r] = to
            rto[:, a, :, r] = law[to % 2] / R
    er = rng.integers(-3, 4, size=(S, A)).astype(np.float64)
    er[:, twins[1]] = er[:, twins[0]]
    assert np.array_equal(rto.sum(axis=(2, 3)), np.ones((S, A)))
    m = tdr._tables(S, A, O, R, rs, rto, er, [0])
    out = SimpleNamespace(m=m, gamma=0.5, alpha=rng.integers(-3, 4, size=(3, S)).astype(np.float64), twins=twins, kind=kind)
    _MODELS[key] = out
    return out


def model_rows(rng, S, B):
    """B dyadic rows, supports cycled from 5 states up (a one-state row's successors collide with each other)."""
    return np.array(_distinct(rng, S, B, _wide(S)))


def successors(case, rows, cast):
    """``(Z [n,A,O], succ [n,A,O,S])``: the successors as an engine of number format ``cast`` holds them (NaN where Z == 0)."""
    m = case.m
    rto = np.asarray(m.reachable_transitional_observation_table, dtype=cast).astype(np.float64)
    n = rows.shape[0]
    Z = np.zeros((n, m.action_count, m.observation_count))
    succ = np.full((n, m.action_count, m.observation_count, m.state_count), np.nan)
    for a, o, u in _successor_rows(rows, m.reachable_states, rto):
        Z[:, a, o] = u.sum(axis=1)
        ok = Z[:, a, o] != 0
        succ[ok, a, o] = (u[ok] / Z[ok, a, o, None]).astype(cast).astype(np.float64)
    return Z, succ


def _nudge(row, cast):
    """The row with the last entry of its support enlarged by ``2^-10`` of itself (rounded to ``cast``): same support, one
    entry differs, and far enough that the sawtooth AT the near-copy is not the point's own value to the last bit."""
    out = row.copy()
    s = np.flatnonzero(row)[-1]
    out[s] = float(cast(row[s] * (1.0 + 2.0 ** -10)))
    assert out[s] != row[s]
    return out


def q_scene(kind, dtype, S=130, P=129, B=40):
    """Rows, and a store whose points are host-computed successors of chosen ``(row, a, o)`` at every position class, the
    same successor stored twice at ``PAIRS`` (different values), near-copies (``plant['near']``: point indices) and fillers.
    ``plant['succ']``: ``(point, row, a, o)``."""
    key = ('q', kind, dtype, S, P, B)
    if key in _CACHE:
        return _CACHE[key]
    case = exact_model(kind, S)
    S = case.m.state_count
    cast = np.float32 if dtype == 'f32' else np.float64
    rng = np.random.default_rng(6000 + S + P)
    corner = integer_corner(rng, S)
    rows = model_rows(rng, S, B)
    Z, succ = successors(case, rows, cast)
    pts, gaps = filler_points(rng, S, P)
    classes = position_classes(P)
    pairs = [(i, j) for i, j in PAIRS if j < P]
    chosen = []
    free = [i for i in range(P) if i not in classes and all(i not in p for p in pairs)]
    near = free[:6]
    slots = classes + [i for i, _ in pairs] + near
    for k, at in enumerate(slots):
        row, a, o = k % B, (0, 1, 2)[k % 3], (k // 3) % 3
        assert Z[row, a, o] != 0
        chosen.append((at, row, a, o))
        pts[at] = succ[row, a, o]
    for i, j in pairs:
        pts[j] = pts[i]
    for at in near:
        pts[at] = _nudge(pts[at], cast)
    values = pts @ corner + gaps
    for i, j in pairs:
        values[j] = values[i] + 1.0
    sc = _scene('q', S, P, corner, pts, gaps, rows, {'succ': chosen[:len(classes) + len(pairs)], 'near': near, 'dup': pairs}, values)
    sc.case, sc.host, sc.Z, sc.succ = case, {}, Z, succ
    _CACHE[key] = sc
    return sc
