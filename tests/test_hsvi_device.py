"""The support-restricted sawtooth upper bound and the HSVI descent built on it: ``sawtooth_numpy`` / ``upper_q_numpy`` on
the host, ``pbvi_upper_bound`` / ``pbvi_upper_q`` and the device point store on the GPU, and ``sawtooth='support'`` through
``BeliefValueMapping``, ``PBVI_Solver.expand_hsvi`` and ``HSVI_Solver``.

The reference's sawtooth takes ``min(b / p)`` over ALL states and is NaN (0/0) for every belief that shares a zero with a
point; that stays the default and is pinned by ``test_hsvi_and_rollouts.py``.  The error bounds of the GPU comparisons are
derived in ``hsvi_cases.py``."""
import os
import random

import numpy as np
import pytest

import hsvi_cases as hc
import model_cases as mc
import test_device_rollout as tdr
from conftest import GOLDEN, load_npz
from pomdp_pbvi_exploration_amd import (Belief, BeliefValueMapping, HSVI_Solver, PBVI_Solver, ValueFunction, VI_Solver,
                                        load_POMDP_file, sawtooth_numpy, synth, upper_q_numpy)
from pomdp_pbvi_exploration_amd.pomdp import upper_q_first_argmax
from test_policy_eval import mirror_model

MODELS = os.path.join(GOLDEN, 'models')
FILES = {'tiger': 'tiger.95.POMDP', 'grid4x3': '4x3.95-no_loop_2_grid.POMDP'}
BOUND_CASES = ['tiger', 'grid4x3', 'ragged', 'olf_R1', 'olf_R5', 'identity_big']
POINT_COUNTS = [0, 1, 65, 300]
BLOCKS = [1, 5, 7]

_MODELS = {}


def file_model(key):
    """``(model, gamma, MDP solution)`` of a golden POMDP file or of the small olfactory model (built once)."""
    if key not in _MODELS:
        if key in FILES:
            model, pbvi = load_POMDP_file(os.path.join(MODELS, FILES[key]))
            gamma = pbvi.gamma
        else:
            sm = synth.olfactory_model(H=15, W=40, R=int(key[-1]), f32=True)
            model, gamma = mirror_model(sm), sm.gamma
        mdp, _ = VI_Solver(gamma=gamma, eps=1e-6).solve(model, print_progress=False)
        _MODELS[key] = (model, float(gamma), mdp)
    return _MODELS[key]


def windows(P):
    """The (n_visible, n_hit) pairs a point count is evaluated under: every point, and n_visible < n_hit < P when P allows."""
    out = [(P, P)]
    if P >= 3:
        out.append((P // 2, P - P // 4))
    return out


# --------------------------------------------------------------------------------------------------------------------- #
# host (no GPU)
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('key', ['tiger', 'grid4x3'])
def test_support_sawtooth_reproduces_the_reference_probes(key):
    """All 32 probes of the fixture are finite and have full support, where the two definitions coincide."""
    g = load_npz('hsvi_and_rollouts.npz')
    model, _, mdp = file_model(key)
    ub = BeliefValueMapping(model, mdp, sawtooth='support')
    for p, v in zip(g[f'{key}_ub_points'], g[f'{key}_ub_values']):
        ub.add(Belief(model, p), float(v))
    ub.update()
    probes = g[f'{key}_ub_probes']
    assert np.all(probes > 0) and np.all(np.isfinite(g[f'{key}_ub_probe_values']))
    got = [ub.evaluate(Belief(model, p)) for p in probes]
    np.testing.assert_allclose(got, g[f'{key}_ub_probe_values'], rtol=1e-12)
    np.testing.assert_allclose(ub.evaluate_block(probes), g[f'{key}_ub_probe_values'], rtol=1e-12)


def test_shared_zeros_reference_is_nan_support_is_the_loop():
    """One point on states {0, 1, 2}, a probe on {0, 1}: the reference's quotient is 0/0 at every other state."""
    model, _, mdp = file_model('grid4x3')
    S = model.state_count
    p = np.zeros(S)
    p[:3] = [0.5, 0.25, 0.25]
    q = np.zeros(S)
    q[:2] = [0.3, 0.7]
    ref = BeliefValueMapping(model, mdp)
    sup = BeliefValueMapping(model, mdp, sawtooth='support')
    for ub in (ref, sup):
        ub.add(Belief(model, p), 0.5)
        ub.update()
    with np.errstate(divide='ignore', invalid='ignore'):
        assert np.isnan(ref.evaluate(Belief(model, q)))             # the current behaviour, kept as the default
    c = sup.corner_values
    v0 = float((q[None, :] @ c)[0])                                # (the row product sawtooth_numpy takes)
    gap = 0.5 - float(np.dot(p, c))
    r = min(q[s] / p[s] for s in range(S) if p[s] > 0)             # = 0: the probe has no mass on state 2
    want = min(v0, v0 + gap * r)
    assert sup.evaluate(Belief(model, q)) == want
    assert sup.gaps == [gap]
    with pytest.raises(ValueError):
        BeliefValueMapping(model, mdp, sawtooth='other')
    with pytest.raises(ValueError):
        ref.evaluate_block(q[None, :])


def test_sawtooth_numpy_properties():
    rng = np.random.default_rng(5)
    S, P = 37, 65
    c = hc.corner_values(rng, S)
    pts, values, gaps = hc.make_points(rng, S, P, c)
    n_visible, n_hit = 30, 50
    rows = hc.make_rows(rng, S, 12, pts, n_hit)
    value, point, hit = sawtooth_numpy(pts, values, gaps, c, rows, n_visible, n_hit)
    v0 = rows @ c
    assert np.all(value[hit < 0] <= v0[hit < 0])                    # the bound never exceeds the corner interpolation
    assert hit[0] == n_hit - 1 and value[0] == values[n_hit - 1]     # a copy of a point inside the window returns its value
    assert hit[3] == -1                                              # a copy of point P - 1, outside the window, is no hit
    assert hit[4] == 0 and value[4] == values[0]
    # a point at or beyond n_visible does not lower U: the same rows with those points' gaps made enormous
    deep = gaps.copy()
    deep[n_visible:] = -1e6
    value2, point2, _ = sawtooth_numpy(pts, values, deep, c, rows, n_visible, n_hit)
    assert np.array_equal(value, value2) and np.array_equal(point, point2) and np.all(point < n_visible)
    # disjoint supports: r_i = 0 for every point, so U = v0 and no point is named
    lone = np.zeros((1, S))
    lone[0, 5] = 1.0
    far = pts[:, 5] == 0
    value3, point3, hit3 = sawtooth_numpy(pts[far], values[far], gaps[far], c, lone)
    assert value3[0] == c[5] and point3[0] == -1 and hit3[0] == -1
    # no points at all, a NaN row, and bad windows
    value4, point4, hit4 = sawtooth_numpy(np.zeros((0, S)), [], [], c, rows)
    assert np.array_equal(value4, v0) and np.all(point4 == -1) and np.all(hit4 == -1)
    bad = rows[:2].copy()
    bad[1, 3] = np.nan
    value5, point5, hit5 = sawtooth_numpy(pts, values, gaps, c, bad)
    assert np.isnan(value5[1]) and point5[1] == -1 and hit5[1] == -1 and value5[0] == values[n_hit - 1]
    with pytest.raises(ValueError):
        sawtooth_numpy(pts, values, gaps, c, rows, n_visible=51, n_hit=50)
    with pytest.raises(ValueError):
        sawtooth_numpy(pts, values, gaps, c, rows, n_hit=P + 1)


@pytest.mark.parametrize('R', [1, 5])
def test_host_descent_reference_stalls_support_descends(R):
    """One descent from the start belief over a mapping that already holds one point, as every expansion after the first
    does: the reference's bound is NaN on every successor (they all share zeros with the point), no action is chosen and the
    chain is the start belief alone; the support-restricted bound descends with finite gaps."""
    model, gamma, mdp = file_model(f'olf_R{R}')
    assert model.state_count == 600
    vf = ValueFunction(model, model.expected_rewards_table.T, model.actions)
    start = Belief(model)
    seed_point = start.update(0, 0)
    chains = {}
    for mode in ('reference', 'support'):
        ub = BeliefValueMapping(model, mdp, sawtooth=mode)
        ub.add(seed_point, float(np.dot(seed_point.values, ub.corner_values)) - 1.0)
        ub.update()
        trace = []
        with np.errstate(divide='ignore', invalid='ignore'):
            chains[mode] = PBVI_Solver(gamma=gamma, eps=1e-6).expand_hsvi(model, start, vf, ub, max_generation=6, trace=trace)
        if mode == 'support':
            assert len(trace) == 6 and all(np.all(np.isfinite(step['gaps'])) and step['observation'] >= 0 for step in trace)
    assert len(chains['reference']) == 1 and chains['reference'].belief_list[0] == start
    assert len(chains['support']) > 1
    with pytest.raises(ValueError):
        PBVI_Solver(gamma=gamma).expand_hsvi(model, start, vf, BeliefValueMapping(model, mdp), sawtooth='support')


@pytest.mark.parametrize('key', ['tiger', 'grid4x3'])
def test_support_hsvi_solve_runs_and_repeats(key):
    model, gamma, _ = file_model(key)
    runs = []
    for _ in range(2):
        np.random.seed(0)
        random.seed(0)
        vf, hist = HSVI_Solver(gamma=gamma, eps=1e-6, sawtooth='support').solve(model, expansions=5, max_belief_growth=6,
                                                                                 print_progress=False)
        runs.append((vf.alpha_vector_array, list(vf.actions), hist.beliefs_counts))
    assert np.all(np.isfinite(runs[0][0])) and runs[0][2][-1] > 1
    assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]
    with pytest.raises(ValueError):
        HSVI_Solver(sawtooth='other')
    assert 'sawtooth' not in HSVI_Solver().expand_function_params     # the default passes nothing new down


# --------------------------------------------------------------------------------------------------------------------- #
# device
# --------------------------------------------------------------------------------------------------------------------- #
def make_engine(c, dtype, mode='sparse'):
    return tdr.make_engine(c, dtype, mode)


def fill_store(eng, corner, pts, values, gaps):
    eng.upper_reset(corner)
    if len(pts):
        eng.upper_append(pts, values, gaps)


def check_bound_call(eng, S, c, pts, values, gaps, rows, n_visible, n_hit, tag):
    eng.set_beliefs(rows)
    value, point, hit = eng.upper_bound_resident(n_visible, n_hit)
    hv, hp, hh = sawtooth_numpy(pts, values, gaps, c, rows, n_visible, n_hit)
    v0, W, M = hc.w_matrix(pts, gaps, c, rows, n_visible)
    tol = hc.sawtooth_bound(S, c, rows, v0, M)
    err = np.abs(value - hv)
    print(f'{tag}: largest value difference {err.max():.3e} (bound {tol[np.argmax(err / tol)]:.3e})')
    assert np.array_equal(hit, hh), tag
    assert np.array_equal(value[hh >= 0], values[hh[hh >= 0]]), tag
    assert np.all(err <= tol), (tag, err, tol)
    floor = np.minimum(v0, W.min(axis=1)) if n_visible else v0
    named = np.where(point >= 0, W[np.arange(len(rows)), np.maximum(point, 0)] if n_visible else v0, v0)
    assert np.all((point >= -1) & (point < n_visible)), tag
    assert np.all(named <= floor + 2.0 * tol), (tag, named, floor)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('name', BOUND_CASES)
def test_upper_bound_matches_the_host(name, dtype):
    """``pbvi_upper_bound`` against ``sawtooth_numpy``: P in {0, 1, 65, 300} points with supports of 1, 63, 64, 65 and S
    states, blocks of 1, 5 and 7 rows (copies of points inside and outside the hit window, the uniform belief, a row off
    point 0's support, sparse rows), every point visible and ``n_visible < n_hit < P``.  Hits are exact; values agree within
    ``hsvi_cases.sawtooth_bound`` (derived there); the named point's host ``w`` is within twice the bound of the host
    minimum, no row excluded."""
    case = hc.get_case(name)
    S = case.m.state_count
    rng = np.random.default_rng(sum(map(ord, name)) + 17)
    c = hc.corner_values(rng, S)
    eng = make_engine(case, dtype)
    try:
        for P in POINT_COUNTS:
            pts, values, gaps = hc.make_points(rng, S, P, c)
            fill_store(eng, c, pts, values, gaps)
            assert eng.upper_count == P
            for n_visible, n_hit in windows(P):
                for B in BLOCKS:
                    rows = hc.make_rows(rng, S, B, pts, n_hit)
                    check_bound_call(eng, S, c, pts, values, gaps, rows, n_visible, n_hit, (name, dtype, P, n_visible, n_hit, B))
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['sparse', 'dense'])
def test_upper_bound_on_a_sorted_block_and_a_dense_engine(mode):
    """300 rows of an fp32 engine are re-ordered inside the engine: every row's results are the bits it gets in a block of
    7, in the caller's order.  The same on a dense-mode engine."""
    case = hc.get_case('ragged')
    S = case.m.state_count
    rng = np.random.default_rng(300)
    c = hc.corner_values(rng, S)
    pts, values, gaps = hc.make_points(rng, S, 65, c)
    rows = hc.r32(mc.sparse_beliefs(rng, 300, S))
    eng = make_engine(case, 'f32', mode)
    try:
        fill_store(eng, c, pts, values, gaps)
        eng.set_beliefs(rows)
        whole = eng.upper_bound_resident()
        q_whole = eng.upper_q_resident(case.gamma, want_p_obs=True, want_succ_value=True)
        for i0 in (0, 7, 294):
            eng.set_beliefs(rows[i0:i0 + 7])
            part = eng.upper_bound_resident()
            q_part = eng.upper_q_resident(case.gamma, want_p_obs=True, want_succ_value=True)
            for w, p in zip(whole + q_whole, part + q_part):
                assert np.array_equal(w[i0:i0 + 7], p, equal_nan=True)
        hv, _, hh = sawtooth_numpy(pts, values, gaps, c, rows)
        assert np.array_equal(whole[2], hh) and np.allclose(whole[0], hv, rtol=1e-12)
    finally:
        eng.close()


def q_rows(case, rng, B, dtype):
    """The case's start belief and sparse rows; full-support rows on tiger, where a belief on one of the two states stays
    there under `listen` and would meet the one-state points."""
    S = case.m.state_count
    more = mc.sparse_beliefs(rng, max(B - 1, 1), S, density=0.3) if S > 2 else rng.dirichlet(np.ones(S), size=max(B - 1, 1))
    rows = np.concatenate([case.b0[:1], more])[:B]
    return hc.r32(rows) if dtype == 'f32' else rows


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['tiger', 'grid4x3', 'ragged', 'olf_R1'])
def test_upper_q_matches_the_host(name, dtype):
    """``pbvi_upper_q`` against ``upper_q_numpy`` on random points -- none of them a successor, which the host restatement
    confirms (zero hits) -- with 0 and 65 points and blocks of 1 and 5 rows.  ``Q``, ``p_obs`` and the successors' values agree
    within ``hsvi_cases.successor_bounds``; the action is the first maximum of the returned row.  The grid's rows meet
    impossible observations: ``p_obs == 0`` exactly on both sides, the successor's value NaN, the term 0."""
    case = hc.get_case(name)
    m = case.m
    S = m.state_count
    rng = np.random.default_rng(sum(map(ord, name)) + 29)
    c = hc.corner_values(rng, S)
    cast = np.float32 if dtype == 'f32' else np.float64
    eng = make_engine(case, dtype)
    try:
        for P in (0, 65):
            pts, values, gaps = hc.make_points(rng, S, P, c, supports=hc.SUPPORTS[1:])
            fill_store(eng, c, pts, values, gaps)
            for n_visible, n_hit in windows(P):
                for B in (1, 5):
                    rows = q_rows(case, rng, B, dtype)
                    host = upper_q_numpy(m, pts, values, gaps, c, rows, case.gamma, n_visible, n_hit, table_dtype=cast)
                    Q, _, Z, sval, shit = host
                    assert np.all(shit == -1)                   # no successor is a point: no hit can occur
                    if name == 'grid4x3':
                        assert np.any(Z == 0)                   # a row with an impossible observation
                    tol_q, tol_z, tol_v = hc.successor_bounds(m, dtype, pts, gaps, c, rows, case.gamma, n_visible, host)
                    eng.set_beliefs(rows)
                    q, act, p_obs, value = eng.upper_q_resident(case.gamma, n_visible, n_hit, want_p_obs=True,
                                                                want_succ_value=True)
                    tag = (name, dtype, P, n_visible, n_hit, B)
                    print(f'{tag}: Q {np.abs(q - Q).max():.3e} (bound {tol_q.max():.3e}), p_obs {np.abs(p_obs - Z).max():.3e}, '
                          f'values {np.nanmax(np.abs(value - sval), initial=0.0):.3e} (bound {tol_v.max():.3e})')
                    assert np.array_equal(p_obs == 0, Z == 0) and np.array_equal(np.isnan(value), Z == 0), tag
                    assert np.all(np.abs(p_obs - Z) <= tol_z), tag
                    ok = Z != 0
                    assert np.all(np.abs(value - sval)[ok] <= tol_v[ok]), tag
                    assert np.all(np.abs(q - Q) <= tol_q), (tag, np.abs(q - Q), tol_q)
                    assert np.array_equal(act, upper_q_first_argmax(q)), tag
                    q2, act2 = eng.upper_q_resident(case.gamma, n_visible, n_hit)
                    assert np.array_equal(q2, q) and np.array_equal(act2, act)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['ragged', 'olf_R1'])
def test_results_do_not_depend_on_the_block(name, dtype):
    """A belief's results are the same bits alone in the block, as row 3 of a block of 7, and across two calls."""
    case = hc.get_case(name)
    S = case.m.state_count
    rng = np.random.default_rng(8)
    c = hc.corner_values(rng, S)
    pts, values, gaps = hc.make_points(rng, S, 65, c)
    rows = hc.make_rows(rng, S, 7, pts, 65)
    eng = make_engine(case, dtype)
    try:
        fill_store(eng, c, pts, values, gaps)

        def both():
            return eng.upper_bound_resident(40, 60) + eng.upper_q_resident(case.gamma, 40, 60, want_p_obs=True,
                                                                           want_succ_value=True)
        eng.set_beliefs(rows)
        block, again = both(), both()
        eng.set_beliefs(rows[3:4])
        alone = both()
        for x, y, z in zip(block, again, alone):
            assert np.array_equal(x, y, equal_nan=True) and np.array_equal(x[3:4], z, equal_nan=True)
    finally:
        eng.close()


@pytest.mark.gpu
def test_store_semantics_and_side_effects():
    case = hc.get_case('olf_R1')
    S = case.m.state_count
    rng = np.random.default_rng(9)
    c = hc.corner_values(rng, S)
    pts, values, gaps = hc.make_points(rng, S, 65, c)
    rows = hc.make_rows(rng, S, 7, pts, 65)
    eng = make_engine(case, 'f64')
    try:
        # a backup's result is still fetchable, and unchanged, after both calls
        eng.set_beliefs(rows)
        eng.run(case.gamma)
        before = eng.fetch()
        fill_store(eng, c, pts, values, gaps)
        one = eng.upper_bound_resident() + eng.upper_q_resident(case.gamma)
        after = eng.fetch()
        for f in ('unique_alpha', 'index', 'actions', 'best_alpha_ind', 'keep'):
            assert np.array_equal(getattr(before, f), getattr(after, f)), f
        assert np.array_equal(eng.fetch_beliefs(), rows) and eng.alpha_count == case.alpha.shape[0]
        # two appends equal one
        eng.upper_reset(c)
        assert eng.upper_count == 0
        eng.upper_append(pts[:20], values[:20], gaps[:20])
        assert eng.upper_append(pts[20:], values[20:], gaps[20:]) == 65
        two = eng.upper_bound_resident() + eng.upper_q_resident(case.gamma)
        for x, y in zip(one, two):
            assert np.array_equal(x, y)
        # a reset empties the store: the corner interpolation alone, no point named, no hit
        eng.upper_reset(c)
        value, point, hit = eng.upper_bound_resident()
        assert eng.upper_count == 0 and np.all(point == -1) and np.all(hit == -1)
        assert np.all(np.abs(value - rows @ c) <= hc.sawtooth_bound(S, c, rows, rows @ c, 0.0))
        # a row with a NaN: NaN, -1, -1, and its neighbours untouched
        fill_store(eng, c, pts, values, gaps)
        bad = rows.copy()
        bad[2, 5] = np.nan
        eng.set_beliefs(bad)
        value, point, hit = eng.upper_bound_resident()
        assert np.isnan(value[2]) and point[2] == -1 and hit[2] == -1
        keep = np.arange(7) != 2
        assert np.array_equal(value[keep], one[0][keep]) and np.array_equal(hit[keep], one[2][keep])
    finally:
        eng.close()


@pytest.mark.gpu
def test_mapping_keeps_a_cursor_per_engine():
    """``BeliefValueMapping.evaluate_block`` through an engine appends only the points added since its last call."""
    model, gamma, mdp = file_model('grid4x3')
    gm = model.to_gpu('f64')
    eng = gm.engine
    g = load_npz('hsvi_and_rollouts.npz')
    probes = g['grid4x3_ub_probes']
    ub = BeliefValueMapping(model, mdp, sawtooth='support')
    ub.add(Belief(model, probes[0]), 1.0)
    ub.update()
    assert np.allclose(ub.evaluate_block(probes, engine=eng), ub.evaluate_block(probes), rtol=1e-12)
    assert eng.upper_count == 1 and ub._cursor[eng.serial][1] == 1
    epoch = eng.upper_epoch
    ub.add(Belief(model, probes[1]), 1.5)
    ub.add(Belief(model, probes[2]), 0.5)
    got = ub.evaluate_block(probes, engine=eng)                    # stale cache: the new points are hits, not yet visible
    assert eng.upper_count == 3 and eng.upper_epoch == epoch         # appended, not re-sent
    assert got[1] == 1.5 and got[2] == 0.5 and np.allclose(got, ub.evaluate_block(probes), rtol=1e-12)
    ub.update()
    assert np.allclose(ub.evaluate_block(probes, engine=eng), ub.evaluate_block(probes), rtol=1e-12)


@pytest.mark.gpu
def test_argument_errors():
    case = hc.get_case('ragged')
    S = case.m.state_count
    rng = np.random.default_rng(10)
    c = hc.corner_values(rng, S)
    pts, values, gaps = hc.make_points(rng, S, 5, c)
    rows = hc.make_rows(rng, S, 5, pts, 5)
    eng = make_engine(case, 'f64')
    try:
        lib, h = eng._lib, eng._h
        eng.upper_reset(c)
        for call in (lambda: eng.upper_bound_resident(), lambda: eng.upper_q_resident(0.9)):
            eng.B = 1
            with pytest.raises(ValueError, match='no belief block'):
                call()
        eng.B = 0
        eng.set_beliefs(rows)
        eng.after_oom()                                              # (no corner set on an engine back in its fresh state)
        eng.set_alpha(case.alpha)
        eng.set_beliefs(rows)
        for call in (lambda: eng.upper_bound_resident(0, 0), lambda: eng.upper_q_resident(0.9, 0, 0),
                     lambda: eng.upper_append(pts, values, gaps)):
            with pytest.raises(ValueError, match='no corner'):
                call()
        fill_store(eng, c, pts, values, gaps)
        for n_visible, n_hit, text in ((3, 2, 'n_visible'), (-1, 2, 'n_visible'), (2, 6, 'n_hit')):
            with pytest.raises(ValueError, match=text):
                eng.upper_bound_resident(n_visible, n_hit)
            with pytest.raises(ValueError, match=text):
                eng.upper_q_resident(0.9, n_visible, n_hit)
        assert lib.pbvi_upper_bound(h, 5, 5, None, None, None) == -1 and b'NULL' in lib.pbvi_last_error()
        assert lib.pbvi_upper_q(h, 0.9, 5, 5, None, None, None, None) == -1 and b'NULL' in lib.pbvi_last_error()
        assert lib.pbvi_upper_reset(h, None) == -1
        for bad in (np.where(pts < 0.1, pts, -pts), np.zeros_like(pts), np.where(pts > 0, np.nan, pts)):
            with pytest.raises(ValueError):
                eng.upper_append(bad, values, gaps)
        with pytest.raises(ValueError):
            eng.upper_append(pts, np.full(5, np.nan), gaps)
        assert eng.upper_count == 5                                  # a refused append leaves the store as it was
        value, _, hit = eng.upper_bound_resident()
        hv, _, hh = sawtooth_numpy(pts, values, gaps, c, rows)
        assert np.array_equal(hit, hh) and np.allclose(value, hv, rtol=1e-12)
    finally:
        eng.close()


@pytest.mark.gpu
def test_calls_obey_the_allocation_cap():
    """Under a 2 MiB cap the [B][A][O] arrays of ``pbvi_upper_q`` for 4000 beliefs of a model with 64 (action, observation)
    pairs do not fit, nor does a point store of 10^5 points: ``MemoryError``, after which the same engine -- back in its
    fresh state, the store empty -- answers correctly."""
    from pomdp_pbvi_exploration_amd import engine as engine_mod
    rng = np.random.default_rng(12)
    S, A, O, R = 4, 8, 8, 1
    rs = rng.integers(0, S, (S, A, R))
    rto = rng.random((S, A, O, R))
    rto /= rto.sum(axis=(2, 3), keepdims=True)
    from types import SimpleNamespace
    case = SimpleNamespace(m=tdr._tables(S, A, O, R, rs, rto, rng.normal(size=(S, A)), [0]), alpha=rng.normal(size=(3, S)))
    c = hc.corner_values(rng, S)
    pts, values, gaps = hc.make_points(rng, S, 5, c)
    b = mc.sparse_beliefs(rng, 4000, S, density=0.7)
    many = np.repeat(pts, 20000, axis=0)
    b = hc.r32(b)
    eng = make_engine(case, 'f32')
    prev = engine_mod.debug_alloc_limit(2)
    try:
        fill_store(eng, c, pts, values, gaps)
        eng.set_beliefs(b)
        with pytest.raises(MemoryError):                          # (Engine._ck has called pbvi_engine_after_oom)
            eng.upper_q_resident(0.9)
        assert eng.B == 0 and eng.upper_count == 0
        eng.upper_reset(c)
        with pytest.raises(MemoryError):
            eng.upper_append(many, np.repeat(values, 20000), np.repeat(gaps, 20000))
        assert eng.upper_count == 0
        engine_mod.debug_alloc_limit(prev)
        fill_store(eng, c, pts, values, gaps)
        eng.set_beliefs(b[:9])
        host = upper_q_numpy(case.m, pts, values, gaps, c, b[:9], 0.9, table_dtype=np.float32)
        tol_q, _, _ = hc.successor_bounds(case.m, 'f32', pts, gaps, c, b[:9], 0.9, 5, host)
        q, act = eng.upper_q_resident(0.9)
        assert np.all(np.abs(q - host[0]) <= tol_q) and np.array_equal(act, upper_q_first_argmax(q))
    finally:
        engine_mod.debug_alloc_limit(prev)
        eng.close()


@pytest.mark.gpu
def test_successor_chunks_give_the_unchunked_bits():
    """With little memory at hand ``pbvi_upper_q`` materialises the successors a few beliefs at a time; the results are the
    bits of the call that held them all at once."""
    from pomdp_pbvi_exploration_amd import engine as engine_mod
    case = hc.get_case('olf_R1')
    S, A, O = case.m.state_count, case.m.action_count, case.m.observation_count
    rng = np.random.default_rng(13)
    c = hc.corner_values(rng, S)
    pts, values, gaps = hc.make_points(rng, S, 65, c)
    rows = mc.sparse_beliefs(rng, 40, S, density=0.2)
    per_belief = A * O * S * 16                                    # un-normalised and normalised fp64 successors
    outs = []
    prev = engine_mod.debug_alloc_limit(-1)
    try:
        for capped in (True, False):
            eng = make_engine(case, 'f64')
            try:
                fill_store(eng, c, pts, values, gaps)
                eng.set_beliefs(rows)
                if capped:                                        # room for fewer than 40 beliefs' successors in half of what is left
                    cap = -(-eng.device_bytes // (1 << 20)) + 2
                    assert (cap << 20) - eng.device_bytes < 40 * per_belief
                    engine_mod.debug_alloc_limit(cap)
                outs.append(eng.upper_q_resident(case.gamma, want_p_obs=True, want_succ_value=True))
            finally:
                engine_mod.debug_alloc_limit(-1)
                eng.close()
    finally:
        engine_mod.debug_alloc_limit(prev)
    for x, y in zip(*outs):
        assert np.array_equal(x, y, equal_nan=True)


# Start beliefs and lengths of the descent test.  Verified on the CPU: from each start the host 'support' descent of that many
# steps meets no hit -- no successor of any action equals a stored point -- which the test asserts again before it looks at
# the device.  (Tiger returns to (0.5, 0.5) behind every opened door, so its fifth step meets a point from any start; the
# grid's own start belief meets one at its fifth step, a full-support start does not within six.)
DESCENT_STARTS = {'tiger': (np.array([0.3, 0.7]), 4), 'grid4x3': (np.random.default_rng(5).dirichlet(np.ones(12)), 6),
                  'olf_R1': (None, 6)}                             # None: the model's start belief


@pytest.mark.gpu
@pytest.mark.parametrize('key', ['tiger', 'grid4x3', 'olf_R1'])
def test_device_descent_follows_the_host_descent(key):
    """One ``'support'`` descent through the fp64 engine takes the host descent's (action, observation) sequence.  Where the
    two part, the host's own margin between the two candidates at that step must be below the derived bound of the
    quantity that decided (``hsvi_cases.successor_bounds``); a hit on either side fails the test."""
    model, gamma, mdp = file_model(key)
    start, steps = DESCENT_STARTS[key]

    def descend(mdl):
        vf = ValueFunction(mdl, mdl.expected_rewards_table.T, mdl.actions)
        ub = BeliefValueMapping(mdl, mdp, sawtooth='support')
        b = Belief(mdl) if start is None else Belief(mdl, start.copy())
        trace = []
        PBVI_Solver(gamma=gamma, eps=1e-9).expand_hsvi(mdl, b, vf, ub, max_generation=steps, trace=trace)
        return trace, ub

    host, ub = descend(model)
    assert len(host) == steps and all(step['hits'] == 0 for step in host)
    dev, _ = descend(model.to_gpu('f64'))
    assert all(step['hits'] == 0 for step in dev)
    rows, values, gaps = ub.point_arrays()
    alpha = model.expected_rewards_table.T
    for t, (hs, ds) in enumerate(zip(host, dev)):
        n_vis = min(1, t)                                          # the stale cache: the first point, from the second step on
        b = hs['belief'][None, :]
        hq = upper_q_numpy(model, rows[:t], values[:t], gaps[:t], ub.corner_values, b, gamma, n_vis, t)
        assert np.array_equal(hq[0][0], hs['q'])
        tol_q, tol_z, tol_v = hc.successor_bounds(model, 'f64', rows[:t], gaps[:t], ub.corner_values, b, gamma, n_vis, hq)
        if ds['action'] != hs['action']:
            margin = abs(hs['q'][hs['action']] - hs['q'][ds['action']])
            assert margin <= tol_q[0, hs['action']] + tol_q[0, ds['action']], (key, t, 'action', margin)
            break
        if ds['observation'] != hs['observation']:
            obs = list(hs['observations'])
            i, j = obs.index(hs['observation']), obs.index(ds['observation'])
            a = hs['action']
            Z, val = hq[2][0, a], hq[3][0, a]
            # score = Z * (upper - lower): the upper bound's and Z's tolerances, and a lower bound re-summed over S terms
            # (|alpha . b'| <= max |alpha|) of a successor that is itself perturbed by (2 S + 2) * 2^-53
            low_tol = (10.0 * model.state_count + 2.0) * hc.EPS * np.abs(alpha).max()
            tol = [tol_z[0, a, o] * abs(hs['gaps'][k]) + Z[o] * (tol_v[0, a, o] + low_tol) for k, o in ((i, obs[i]), (j, obs[j]))]
            margin = abs(hs['scores'][i] - hs['scores'][j])
            assert margin <= sum(tol), (key, t, 'observation', margin)
            break
    else:
        assert len(dev) == steps
