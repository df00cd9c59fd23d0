"""The sawtooth's point, tie and hit rules, bit for bit, on exact inputs (``upper_exact_cases.py`` has the method and the
scenes).  Host tests first: they establish that the inputs are exact and that the planted structure is what
``sawtooth_numpy`` sees, so that a device failure cannot be a bad case.  The device tests compare ``pbvi_upper_bound`` and
``pbvi_upper_q`` with ``==`` against the host; the only tolerance in this file is ``hsvi_cases.successor_bounds`` for the
values and ``Q`` of the tier-'dyadic' models that are no hit.

Near-hit rows on a point of exactly 65 (129) entries differ from it in the 65th (129th) entry alone, so they sum to
``1 + 2^-10``; the rows that move ``2^-10`` between two entries of the second (third) trip sit on a point of up to 200
entries and sum to 1."""
from types import SimpleNamespace

import numpy as np
import pytest

import hsvi_cases as hc
import model_cases as mc
import test_device_rollout as tdr
import upper_exact_cases as uc
from pomdp_pbvi_exploration_amd import sawtooth_numpy, upper_q_numpy
from pomdp_pbvi_exploration_amd.pomdp import _successor_rows, upper_q_first_argmax

KINDS = ('positions', 'ties', 'hits')
NEAR_S = (64, 65, 130, 257, 600)
SEAM_S = (255, 256, 257, 513)
HOST_S, HOST_P = 130, 129                                           # the scenes of the loop restatement


def all_scenes():
    for S in uc.STATE_COUNTS:
        for P in uc.POINT_COUNTS:
            for kind in KINDS:
                yield uc.scene(kind, S, P)
    for S in NEAR_S:
        yield uc.scene('near', S, 129)
    for S in SEAM_S:
        yield uc.scene('seams', S, 65)


# --------------------------------------------------------------------------------------------------------------------- #
# host (no GPU)
# --------------------------------------------------------------------------------------------------------------------- #
def loop_sawtooth(sc, n_visible, n_hit, defect=None):
    """``sawtooth_numpy`` restated as plain loops over rows, points and states: strict ``<`` in ascending index behind ``v0``,
    the hit as equal non-zero counts plus elementwise equality.  ``defect`` plants one of five mistakes."""
    S = sc.S
    pts = [[(s, float(p[s])) for s in range(S) if p[s] > 0] for p in sc.points[:n_hit]]
    value, point, hit = [], [], []
    for row in sc.rows:
        b = row.tolist()
        v0, nnz = 0.0, 0
        for s in range(S):
            v0 += b[s] * sc.corner[s]
            nnz += b[s] != 0
        best, arg, h = v0, -1, -1
        for i in range(n_hit):
            if i < n_visible:
                r = float('inf')
                for s, p in pts[i]:
                    q = b[s] / p
                    if q < r:
                        r = q
                w = v0 + sc.gaps[i] * r
                if w < best or (defect == 'le' and w == best):
                    best, arg = w, i
            if (h < 0 or defect == 'last_hit') and (i < n_visible or defect != 'visible_window'):
                same = nnz == len(pts[i]) or defect == 'no_nnz'
                for s, p in (pts[i][:64] if defect == 'first64' else pts[i]):
                    if b[s] != p:
                        same = False
                        break
                if same:
                    h = i
        value.append(sc.values[h] if h >= 0 else best)
        point.append(arg)
        hit.append(h)
    return np.array(value), np.array(point), np.array(hit)


def test_v0_is_exact_in_every_order():
    """``rows @ c`` equals the ``longdouble`` sum and the sum in reversed state order, for the rows of every scene."""
    n = 0
    for sc in all_scenes():
        v0 = sc.rows @ sc.corner
        wide = (sc.rows.astype(np.longdouble) * sc.corner.astype(np.longdouble)).sum(axis=1)
        assert np.array_equal(v0.astype(np.longdouble), wide), (sc.kind, sc.S, sc.P)
        assert np.array_equal(v0, sc.rows[:, ::-1] @ sc.corner[::-1]), (sc.kind, sc.S, sc.P)
        assert np.array_equal(hc.r32(sc.rows), sc.rows) and np.array_equal(hc.r32(sc.points), sc.points)
        n += 1
    assert n == 3 * len(uc.STATE_COUNTS) * len(uc.POINT_COUNTS) + len(NEAR_S) + len(SEAM_S)


@pytest.mark.parametrize('kind', ['R1-power', 'R2-power', 'R1-dyadic', 'R2-dyadic', 'seam'])
def test_model_sums_are_exact(kind):
    """``_successor_rows``, ``Z`` and ``b . ER`` of the exact models against a ``longdouble`` loop over (s, r)."""
    case = uc.exact_model(kind)
    m = case.m
    S, A, O, R = m.state_count, m.action_count, m.observation_count, m.reachable_state_count
    rows = uc.model_rows(np.random.default_rng(3), S, 12)
    rs, rto, er = m.reachable_states, m.reachable_transitional_observation_table, m.expected_rewards_table
    assert np.array_equal(hc.r32(rto), rto) and np.array_equal(er, np.round(er))
    wide = rows.astype(np.longdouble)
    assert np.array_equal((rows @ er).astype(np.longdouble), wide @ er.astype(np.longdouble))
    assert np.array_equal(rows @ er, rows[:, ::-1] @ er[::-1])
    impossible = 0
    for a, o, u in _successor_rows(rows, rs, rto):
        ul = np.zeros((rows.shape[0], S), dtype=np.longdouble)
        for s in range(S):
            for r in range(R):
                ul[:, rs[s, a, r]] += wide[:, s] * np.longdouble(rto[s, a, o, r])
        assert np.array_equal(u.astype(np.longdouble), ul), (a, o)
        z = u.sum(axis=1)
        assert np.array_equal(z.astype(np.longdouble), ul.sum(axis=1)) and np.array_equal(z, u[:, ::-1].sum(axis=1))
        impossible += int(np.all(z == 0))
        if kind.endswith('power') or kind == 'seam':                 # Z is a power of two: the successor is dyadic
            assert np.all((z == 0) | (np.frexp(z)[0] == 0.5))
            ok = z != 0
            assert np.array_equal(hc.r32(u[ok] / z[ok, None]), u[ok] / z[ok, None])
    assert impossible >= A                                          # the last observation, under every action
    a, b = case.twins
    assert np.array_equal(rs[:, a], rs[:, b]) and np.array_equal(rto[:, a], rto[:, b]) and np.array_equal(er[:, a], er[:, b])


def test_planted_structure_is_what_the_host_sees():
    """Under the window (P, P): every position class is the unique minimum of its row; every tie pair has ``w_i == w_j`` and
    names ``min(i, j)``; the row that ties with ``v0`` names no point; copies hit the lowest index and return its value;
    no near-hit row hits."""
    seen = {k: 0 for k in ('min', 'tie', 'v0', 'hit', 'dup', 'near')}
    for sc in all_scenes():
        value, point, hit = uc.host_result(sc, sc.P, sc.P)
        v0 = sc.rows @ sc.corner
        tag = (sc.kind, sc.S, sc.P)
        if sc.kind == 'positions':
            _, W, _ = hc.w_matrix(sc.points, sc.gaps, sc.corner, sc.rows, sc.P)
            assert [t for _, t in sc.plant['min']] == uc.position_classes(sc.P)
        for k, t in sc.plant.get('min', []):
            assert point[k] == t and hit[k] == -1 and value[k] == v0[k] + uc.PLANT_GAP * 0.5, (tag, k, t)
            assert np.count_nonzero(W[k] == W[k].min()) == 1 and W[k, t] < v0[k], (tag, k, t)
            seen['min'] += 1
        for k, i, j in sc.plant.get('tie', []):
            assert i < j and np.array_equal(sc.points[i], sc.points[j]) and sc.gaps[i] == sc.gaps[j], (tag, i, j)
            _, W, _ = hc.w_matrix(sc.points, sc.gaps, sc.corner, sc.rows[k:k + 1], sc.P)
            assert W[0, i] == W[0, j] == W[0].min() and np.count_nonzero(W[0] == W[0].min()) == 2, (tag, i, j)
            assert point[k] == i and hit[k] == -1 and value[k] == W[0, i], (tag, i, j)
            seen['tie'] += 1
        for k in sc.plant.get('v0', []):
            _, W, _ = hc.w_matrix(sc.points, sc.gaps, sc.corner, sc.rows[k:k + 1], sc.P)
            assert W[0].min() == v0[k] and np.count_nonzero(W[0] == v0[k]) >= sc.P - 1, tag     # all but the positive gap
            assert W[0, uc.GAP0_AT] == v0[k] and W[0, uc.GAP_POS_AT] > v0[k], tag
            assert point[k] == -1 and hit[k] == -1 and value[k] == v0[k], tag
            seen['v0'] += 1
        for k, t in sc.plant.get('hit', []):
            assert hit[k] == t and value[k] == sc.values[t], (tag, k, t)
            seen['hit'] += 1
        if sc.kind == 'hits':                                       # a copy beyond n_hit is no hit, one beyond n_visible is
            for n_visible, n_hit in uc.windows(sc.P)[1:]:
                wv, _, wh = uc.host_result(sc, n_visible, n_hit)
                for k, t in sc.plant['hit']:
                    assert wh[k] == (t if t < n_hit else -1), (tag, n_visible, n_hit, k, t)
                    assert t >= n_hit or wv[k] == sc.values[t], (tag, n_visible, n_hit, k, t)
        for i, j in sc.plant.get('dup', []):
            assert np.array_equal(sc.points[i], sc.points[j]) and sc.values[i] != sc.values[j], (tag, i, j)
            seen['dup'] += 1
        for k in sc.plant.get('near', []):
            assert hit[k] == -1, (tag, k)
            seen['near'] += 1
    assert all(n > 0 for n in seen.values()), seen
    # positions: every (chunk, wave, slot) class of the largest store (its last chunk holds 44 points: slots 0 to 10)
    assert {uc.position(t) for t in uc.position_classes(300)} == {(c, w, s) for c in (0, 1, 4) for w in range(4)
                                                                  for s in (0, 10 if c == 4 else 15)}
    assert uc.position(uc.index_at(2, 3, 9)) == (2, 3, 9)


HOST_WINDOWS = [(HOST_P, HOST_P), (0, HOST_P), (64, 65)]


@pytest.mark.parametrize('kind', KINDS + ('near',))
def test_sawtooth_numpy_equals_the_loop_restatement(kind):
    sc = uc.scene(kind, HOST_S, HOST_P)
    for n_visible, n_hit in HOST_WINDOWS:
        for got, want in zip(uc.host_result(sc, n_visible, n_hit), loop_sawtooth(sc, n_visible, n_hit)):
            assert np.array_equal(got, want), (kind, n_visible, n_hit)


@pytest.mark.parametrize('defect,kind,window', [('le', 'ties', (HOST_P, HOST_P)), ('no_nnz', 'near', (HOST_P, HOST_P)),
                                                ('first64', 'near', (HOST_P, HOST_P)), ('last_hit', 'hits', (HOST_P, HOST_P)),
                                                ('visible_window', 'hits', (0, HOST_P))])
def test_planted_host_defects_fail(defect, kind, window):
    """Each stand-in for ``sawtooth_numpy`` -- ``<=`` for ``<``, the hit without the non-zero count, the hit over the first
    64 entries, the last hit, ``n_visible`` as the hit window -- disagrees with it on the scene named: the cases discriminate."""
    sc = uc.scene(kind, HOST_S, HOST_P)
    host = uc.host_result(sc, *window)
    bad = loop_sawtooth(sc, *window, defect=defect)
    wrong = [int(np.count_nonzero(~((g == w) | ((g != g) & (w != w))))) for g, w in zip(host, bad)]
    print(f'{defect}: rows that differ in (value, point, hit) = {wrong}')
    assert sum(wrong) > 0, defect


_HOST_Q = {}


def host_q(sc, dtype, B, n_visible, n_hit):
    key = (id(sc), B, n_visible, n_hit)
    if key not in _HOST_Q:
        cast = np.float32 if dtype == 'f32' else np.float64
        _HOST_Q[key] = upper_q_numpy(sc.case.m, sc.points, sc.values, sc.gaps, sc.corner, sc.rows[:B], sc.case.gamma, n_visible,
                                     n_hit, table_dtype=cast)
    return _HOST_Q[key]


# (hits, impossible (row, a, o), both over 40 rows x 4 actions x 4 observations) that upper_q_numpy sees per exact model
Q_COUNTS = {'R1-power': (84, 160), 'R2-power': (84, 160), 'R1-dyadic': (30, 160), 'R2-dyadic': (28, 160)}


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['R1-power', 'R2-power', 'R1-dyadic', 'R2-dyadic'])
def test_upper_q_numpy_on_the_exact_models(kind, dtype):
    """Every model's scene has successor hits at every position class and impossible observations; a near-copy is never
    hit and its value is no successor's; the twin actions have the same ``Q`` bits and the later twin is never chosen."""
    sc = uc.q_scene(kind, dtype)
    case = sc.case
    Q, act, Z, sval, shit = host_q(sc, dtype, 40, sc.P, sc.P)
    hits, impossible = int(np.count_nonzero(shit >= 0)), int(np.count_nonzero(Z == 0))
    print(f'{kind} {dtype}: {hits} successor hits, {impossible} impossible observations of {Z.size}')
    assert len(set(sc.values.tolist())) == sc.P
    assert (hits, impossible) == Q_COUNTS[kind] and hits >= len(sc.plant['succ'])
    assert set(uc.position_classes(sc.P)) <= set(shit[shit >= 0].tolist())
    for at, row, a, o in sc.plant['succ']:
        assert shit[row, a, o] == at and sval[row, a, o] == sc.values[at], (at, row, a, o)
    for i, j in sc.plant['dup']:
        assert j not in shit
    assert not set(sc.plant['near']) & set(shit.ravel().tolist())
    for n_visible, n_hit in uc.windows(sc.P):
        _, _, Zw, svalw, shitw = host_q(sc, dtype, 40, n_visible, n_hit)
        for i in sc.plant['near']:
            assert not np.any(svalw[(shitw < 0) & (Zw != 0)] == sc.values[i]), (n_visible, n_hit, i)
    a, b = case.twins
    assert np.array_equal(Q[:, a], Q[:, b]) and not np.any(act == b) and np.any(act == a)


# --------------------------------------------------------------------------------------------------------------------- #
# device
# --------------------------------------------------------------------------------------------------------------------- #
def engine_for(S, dtype, mode='sparse'):
    return tdr.make_engine(uc.exact_model('R1-power', S), dtype, mode)


def fill(eng, sc):
    eng.upper_reset(sc.corner)
    eng.upper_append(sc.points, sc.values, sc.gaps)
    assert eng.upper_count == sc.P


def check_scene(eng, sc, tag):
    """value, point and hit of every window of the scene ``==`` the host's."""
    fill(eng, sc)
    eng.set_beliefs(sc.rows)
    for n_visible, n_hit in uc.windows(sc.P):
        got = eng.upper_bound_resident(n_visible, n_hit)
        for name, g, w in zip(('value', 'point', 'hit'), got, uc.host_result(sc, n_visible, n_hit)):
            assert np.array_equal(g, w, equal_nan=True), (tag, sc.kind, sc.S, sc.P, n_visible, n_hit, name, np.flatnonzero(g != w))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('S', uc.STATE_COUNTS)
@pytest.mark.parametrize('kind', KINDS)
def test_upper_bound_equals_the_host(kind, S, dtype):
    """Positions, ties and hits: P in {63, 64, 65, 127, 128, 129, 300}, every window of ``upper_exact_cases.windows``."""
    eng = engine_for(S, dtype)
    try:
        for P in uc.POINT_COUNTS:
            check_scene(eng, uc.scene(kind, S, P), dtype)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('S', NEAR_S)
def test_near_hits_are_no_hits(S, dtype):
    eng = engine_for(S, dtype)
    try:
        sc = uc.scene('near', S, 129)
        check_scene(eng, sc, dtype)
        _, _, hit = eng.upper_bound_resident()
        assert np.all(hit[sc.plant['near']] == -1) and all(hit[k] == t for k, t in sc.plant['hit'])
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('S', SEAM_S)
def test_row_kernel_seams(S, dtype):
    """Mass on the last state and on states 0, 256 and 512; a NaN at the last state gives NaN, -1, -1 and leaves its
    neighbours the bits they get alone."""
    eng = engine_for(S, dtype)
    try:
        sc = uc.scene('seams', S, 65)
        check_scene(eng, sc, dtype)
        clean = eng.upper_bound_resident()
        bad = sc.rows.copy()
        bad[1, S - 1] = np.nan
        eng.set_beliefs(bad)
        value, point, hit = eng.upper_bound_resident()
        assert np.isnan(value[1]) and point[1] == -1 and hit[1] == -1
        keep = np.arange(len(bad)) != 1
        for got, want in zip((value, point, hit), clean):
            assert np.array_equal(got[keep], want[keep])
        for k in np.flatnonzero(keep):
            eng.set_beliefs(sc.rows[k:k + 1])
            for got, want in zip(eng.upper_bound_resident(), clean):
                assert np.array_equal(got, want[k:k + 1])
    finally:
        eng.close()


@pytest.mark.gpu
def test_dense_mode_engine():
    eng = engine_for(130, 'f32', 'dense')
    try:
        for kind in KINDS + ('near',):
            check_scene(eng, uc.scene(kind, 130, 129), 'dense')
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('kind,P', [('positions', 300), ('ties', 300), ('hits', 300), ('near', 129)])
def test_sorted_block(kind, P):
    """300 exact rows in an fp32 engine are re-ordered inside the engine: everything above holds in the caller's order,
    and rows [i0, i0 + 7) alone get the same bits."""
    S = 130
    sc = uc.scene(kind, S, P)
    rng = np.random.default_rng(300)
    pad = np.concatenate([uc.dyadic_rows(rng, S, k, n=50) for k in uc.SUPPORTS])
    rows = np.concatenate([sc.rows, pad])[:300]
    order = rng.permutation(300)
    rows = rows[order]
    eng = engine_for(S, 'f32')
    try:
        fill(eng, sc)
        eng.set_beliefs(rows)
        for n_visible, n_hit in [(P, P), (0, P), (64, 65)]:
            whole = eng.upper_bound_resident(n_visible, n_hit)
            host = sawtooth_numpy(sc.points, sc.values, sc.gaps, sc.corner, rows, n_visible, n_hit)
            for got, want in zip(whole, host):
                assert np.array_equal(got, want), (kind, n_visible, n_hit)
        whole = eng.upper_bound_resident()
        for i0 in (0, 7, 293):
            eng.set_beliefs(rows[i0:i0 + 7])
            for got, want in zip(eng.upper_bound_resident(), whole):
                assert np.array_equal(got, want[i0:i0 + 7]), (kind, i0)
    finally:
        eng.close()


def device_q(eng, sc, n_visible, n_hit):
    return eng.upper_q_resident(sc.case.gamma, n_visible, n_hit, want_p_obs=True, want_succ_value=True)


def check_q_exact(eng, sc, dtype, B, wins):
    eng.set_beliefs(sc.rows[:B])
    a, b = sc.case.twins
    hits = 0
    for n_visible, n_hit in wins:
        Q, act, Z, sval, shit = host_q(sc, dtype, B, n_visible, n_hit)
        q, action, p_obs, value = device_q(eng, sc, n_visible, n_hit)
        tag = (sc.case.kind, dtype, B, n_visible, n_hit)
        assert np.array_equal(p_obs, Z), tag
        assert np.array_equal(value, sval, equal_nan=True), (tag, np.argwhere(~((value == sval) | (Z == 0))))
        assert np.array_equal(value[shit >= 0], sc.values[shit[shit >= 0]]), tag
        assert np.array_equal(q, Q), tag
        assert np.array_equal(action, act), tag
        assert np.array_equal(q[:, a], q[:, b]) and not np.any(action == b), tag
        hits += int(np.count_nonzero(shit >= 0))
    return hits


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['R1-power', 'R2-power'])
def test_upper_q_equals_the_host_on_power_of_two_models(kind, dtype):
    """``q``, ``action``, ``p_obs`` and ``succ_value`` ``==`` ``upper_q_numpy``'s with successor hits at every position class,
    duplicates and near-copies in the store, B in {1, 5, 40}, every window; the twin actions have equal bits and the earlier
    is chosen; a NaN row gives a ``Q`` row of NaN and action 0."""
    sc = uc.q_scene(kind, dtype)
    eng = tdr.make_engine(sc.case, dtype)
    try:
        fill(eng, sc)
        for B in (1, 5, 40):
            hits = check_q_exact(eng, sc, dtype, B, uc.windows(sc.P))
            assert hits > 0, (kind, B)
        clean = device_q(eng, sc, sc.P, sc.P)
        bad = sc.rows[:5].copy()
        bad[2, np.flatnonzero(bad[2])[0]] = np.nan
        eng.set_beliefs(bad)
        q, action, p_obs, value = device_q(eng, sc, sc.P, sc.P)
        assert np.all(np.isnan(q[2])) and action[2] == 0
        keep = [0, 1, 3, 4]
        for got, want in zip((q, action, p_obs, value), clean):
            assert np.array_equal(got[keep], want[keep], equal_nan=True)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('kind', ['R1-dyadic', 'R2-dyadic'])
def test_upper_q_hit_pattern_on_dyadic_models(kind, dtype):
    """``Z`` is an exact sum and no power of two: ``p_obs ==``, the hit pattern is exact (a hit returns the point's value, a
    near-copy's value is never returned), the other values and ``Q`` lie within ``hsvi_cases.successor_bounds``."""
    sc = uc.q_scene(kind, dtype)
    eng = tdr.make_engine(sc.case, dtype)
    P = sc.P
    try:
        fill(eng, sc)
        # (B = 40 under three windows only: `successor_bounds` walks every (row, a, o) on the host, 0.3 s per window there)
        for B, wins in ((1, uc.windows(P)), (5, uc.windows(P)), (40, [(P, P), (0, P), (64, 65)])):
            eng.set_beliefs(sc.rows[:B])
            for n_visible, n_hit in wins:
                host = host_q(sc, dtype, B, n_visible, n_hit)
                Q, act, Z, sval, shit = host
                q, action, p_obs, value = device_q(eng, sc, n_visible, n_hit)
                tag = (kind, dtype, B, n_visible, n_hit)
                assert np.array_equal(p_obs, Z) and np.array_equal(np.isnan(value), Z == 0), tag
                assert np.array_equal(value[shit >= 0], sc.values[shit[shit >= 0]]), tag
                miss = (shit < 0) & (Z != 0)
                for i in sc.plant['near']:
                    assert not np.any(value[miss] == sc.values[i]), (tag, i)
                tol_q, _, tol_v = hc.successor_bounds(sc.case.m, dtype, sc.points, sc.gaps, sc.corner, sc.rows[:B], sc.case.gamma,
                                                      n_visible, host)
                assert np.all(np.abs(value - sval)[miss] <= tol_v[miss]), tag
                assert np.all(np.abs(q - Q) <= tol_q), tag
                assert np.array_equal(action, upper_q_first_argmax(q)), tag
            assert np.any(host_q(sc, dtype, B, P, P)[4] >= 0)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_upper_q_belief_seam(dtype):
    """``A * O = 64``: at most ``65535 // 64 = 1023`` beliefs' successors go through one launch, so 1100 beliefs take two.
    Everything equals the host; rows 1022, 1023, 1024 and the last get the bits they get in a block of 7."""
    B, P = 1100, 70
    sc = uc.q_scene('seam', dtype, S=4, P=P, B=B)
    assert sc.case.m.action_count * sc.case.m.observation_count == 64 and 65535 // 64 == 1023 < B
    eng = tdr.make_engine(sc.case, dtype)
    try:
        fill(eng, sc)
        hits = check_q_exact(eng, sc, dtype, B, [(P, P), (1, P)])
        assert hits > 0
        whole = device_q(eng, sc, P, P)
        for i0 in (1020, B - 7):
            eng.set_beliefs(sc.rows[i0:i0 + 7])
            for got, want in zip(device_q(eng, sc, P, P), whole):
                assert np.array_equal(got, want[i0:i0 + 7], equal_nan=True), i0
    finally:
        eng.close()


def check_closure(eng, S, A, O, rows, corner, rng, tag):
    """The rows ``belief_update`` returns for chosen (row, a, o), stored as points with distinct values, are exactly the
    successors ``upper_q`` evaluates: it returns those values at those (row, a, o)."""
    n = rows.shape[0]
    acts, obs = np.arange(n) % A, (np.arange(n) // A) % O
    kids = np.asarray(eng.belief_update(rows, acts, obs), dtype=np.float64)
    assert np.all(np.isfinite(kids)) and len({k.tobytes() for k in kids}) == n, tag
    P = 70
    pts, gaps = uc.filler_points(rng, S, P)
    slots = uc.position_classes(P)[:n]
    assert len(slots) == n
    pts[slots] = kids
    values = pts @ corner + gaps
    assert len(set(values.tolist())) == P
    eng.upper_reset(corner)
    eng.upper_append(pts, values, values - pts @ corner)
    eng.set_beliefs(rows)
    _, _, value = eng.upper_q_resident(0.5, want_succ_value=True)
    assert np.array_equal(value[np.arange(n), acts, obs], values[slots]), (tag, value[np.arange(n), acts, obs], values[slots])
    return kids


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('S', [257, 512])
def test_closure_with_belief_update_on_inexact_inputs(S, dtype):
    """What the descent relies on, promised up to 512 states: ``belief_update`` adds the masses of at most two 256-state
    blocks with atomics, ``upper_q`` adds them in block order, and two partial sums commute (three do not)."""
    rng = np.random.default_rng(S)
    rs, rto = mc.ragged_model(S, O=3)
    A, O, R = rto.shape[1], rto.shape[2], rto.shape[3]
    case = SimpleNamespace(m=tdr._tables(S, A, O, R, rs, rto, rng.normal(size=(S, A)), [0]), alpha=rng.normal(size=(3, S)))
    rows = hc.r32(mc.sparse_beliefs(rng, 12, S))
    eng = tdr.make_engine(case, dtype)
    try:
        check_closure(eng, S, A, O, rows, hc.corner_values(rng, S), rng, (S, dtype))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('S', [600, 2053])
def test_closure_with_belief_update_on_dyadic_inputs(S, dtype):
    """Above 512 states on exact inputs, where the mass is the same in every order; the rows also equal the host's."""
    case = uc.exact_model('R2-power', S)
    rng = np.random.default_rng(S)
    rows = uc.model_rows(rng, S, 12)
    eng = tdr.make_engine(case, dtype)
    try:
        kids = check_closure(eng, S, 4, 3, rows, uc.integer_corner(rng, S), rng, (S, dtype))
        _, succ = uc.successors(case, rows, np.float64)
        n = np.arange(12)
        assert np.array_equal(kids, succ[n, n % 4, (n // 4) % 3])
    finally:
        eng.close()
