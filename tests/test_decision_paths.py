"""The stages behind the scoring stage, against exact and high-precision references: the fp64 re-decision of near-ties
(``k_refine``, its grid-wide passes, ``k_refine_split``), the action tail (``k_action_select``, ``k_refine_action``,
``k_action_final``) and the repeat of the decision after a failed speculation.  tests/test_score_window.py pins everything
up to the end of the scoring stage; this module pins what the engine returns.

Family E (tests/decision_cases.py) is exact arithmetic with planted candidates: the reference has no rounding, every
entry has exactly k candidates on every route, and alpha' rows are compared byte for byte.  Family N is the inexact
near-tie construction of ``test_adversarial_near_ties`` against ``np.longdouble``.  Which path of the refinement ran is
read from ``Engine.debug_refine_counts`` and compared with ``path_model`` below, a restatement of k_refine's routing.

Settings that force a path (read per call unless noted):
  default, more than 8 candidates in a 256-column chunk     GEMM path (weights, fp64 MFMA GEMM, k_refine_slot_argmax)
  PBVI_REFINE_W_SLOTS=0                                     item path only (k_refine_items / _first / _merge)
  PBVI_REFINE_W_SLOTS=1                                     slot 0 on the GEMM path, k_refine_merge starts at slot 1
  PBVI_REFINE_W_SLOTS=0 PBVI_REFINE_ITEM_CAP=n              voided items: the entry's own block scores, k_refine_merge merges
  PBVI_REFINE_SLOT_CAP=1                                    slot exhaustion: the entry's own block decides
  PBVI_REFINE_DEFER_MIN=-1                                  every candidate to the grid-wide passes, however few
  PBVI_REFINE_Q2_CAP=n                                      k_refine_split's hand-over overflows: scored in k_refine's block,
                                                            with the same bits (n = 1, 100, 300)
  PBVI_REFINE_INBLOCK, PBVI_NO_L1_SCREEN (once per process) no work list at all / no level-1 screen: in a child process
"""
import contextlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from decision_cases import (E_B, E_KS, E_S, E_V, E_VARIANTS, N_VARIANTS, chunk_counts, digest, e_gain_units, e_plain_alpha,
                            e_problem, n_problem, planted_positions, ref_backup, undecidable)
from oracle import pbvi_oracle as orc
from test_score_window import PIPELINES, U24, configure, f32r, ref_magnitude, ref_scores, sparse_rto, successors

gpu = pytest.mark.gpu

F32_RTOL = 1e-6                                              # tests/test_gpu_parity.py
F64_RTOL = 1e-12

# name -> (engine dtype, model variant, Engine mode): test_score_window's thirteen and the pure fp64 pipeline
ROUTES = dict(PIPELINES)
ROUTES['f64_pure'] = ('f64', 'proj', 'sparse')
WINDOWED = [n for n in ROUTES if n != 'f64_pure']
# fp32 engines whose projected Gamma rows are in HBM get k_refine's level-1 screen (engine.hip: refine)
L1_ROUTES = ('f32_projected', 'split_projected_parent', 'split_projected_pipelined')
# alpha-side fp32 scores and screens carry a window on the reward term b . ER (k_action_select); the belief side's is exact
REWARD_WINDOW = [n for n in WINDOWED if not n.endswith('belief') and n != 'f32_belief_side']
E_SHAPE = {'proj': (3, False), 'fused1': (1, True), 'fused3': (3, True)}       # model variant -> (R, consecutive successors)


def has_l1(name):
    return name in L1_ROUTES and os.environ.get('PBVI_NO_L1_SCREEN') is None


def e_case(name, k, variant, late=False, actions=None):
    R, regular = E_SHAPE[ROUTES[name][1]]
    return e_problem(R, regular, k, variant, late, actions)


def n_case(name, actions=None, eps=0.0, **kw):
    return n_problem(ROUTES[name][1], ROUTES[name][0] == 'f32', actions, eps, **kw)


@contextlib.contextmanager
def routed_engine(name, prob):
    """An engine of `prob`'s model routed as `name` says; yields (engine, assertions on (stats, probe) that the route ran)."""
    from pomdp_pbvi_exploration_amd.engine import debug_split_schedule
    dtype, _, mode = ROUTES[name]
    eng = prob.engine(dtype, mode)
    prev = debug_split_schedule('pipelined' if name.endswith('pipelined') else 'parent')
    try:
        if name == 'f64_pure':
            eng.set_f64_screen('off')
            eng.set_formulation('alpha')
            checks = [lambda st, p: st['screened'] == 0 and p['push'] == 0 and p['qcount'] == 0]
        else:
            checks = configure(eng, name, prob)
        eng.debug_score_probe(True)
        yield eng, checks
    finally:
        debug_split_schedule(prev)
        eng.close()


def run_backup(eng, prob, checks=()):
    eng.set_alpha(prob.alpha)
    eng.set_beliefs(prob.b)
    st = eng.run(prob.gamma)
    res = eng.fetch()
    if checks:
        p = eng.debug_score_probe_fetch()
        for i, ok in enumerate(checks):
            assert ok(st, p), (i, st)
    return st, res


def check_result(prob, res, dtype, tag):
    """Indices and actions exact; rows byte for byte (exact families) or within the parity tolerances."""
    ref = prob.ref
    bad = np.argwhere(res.best_alpha_ind != ref['best'])
    assert bad.size == 0, (tag, len(bad), bad[:5].tolist(), res.best_alpha_ind[tuple(bad[0])], ref['best'][tuple(bad[0])])
    assert np.array_equal(res.actions, ref['actions']), (tag, np.flatnonzero(res.actions != ref['actions'])[:8])
    got = np.asarray(res.alpha)
    if prob.exact:
        want = ref['rows'].astype(np.float32 if dtype == 'f32' else np.float64)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), tag
    else:
        rtol = F32_RTOL if dtype == 'f32' else F64_RTOL
        want = ref['rows']
        np.testing.assert_allclose(got.astype(np.float64), want, rtol=rtol,
                                   atol=rtol * max(1e-300, float(np.max(np.abs(want)))) * 1e-3, err_msg=tag)


def check_value_max(eng, prob, tag):
    """max_value_resident (k_refine's PROJ = false instantiations, G = 1) on the resident set and block: exact family only."""
    val, idx = eng.max_value_resident()
    sc = prob.b @ prob.alpha.T                               # exact
    assert np.array_equal(idx, np.argmax(sc, axis=1)), tag
    assert np.array_equal(val, sc.max(axis=1)), tag


def path_model(l1, counts, defer_min=8):
    """k_refine's routing of an entry whose candidates fall into the 256-column chunks as `counts` says:
    (deferred to the grid-wide passes?, candidates listed when the slot takes the item path, handed to k_refine_split
    when the level-1 screen separates nothing)."""
    k = sum(counts)
    if defer_min >= 0 and k <= 32 and (l1 or k <= 8):        # collected whole: level-1 screen / the fast path
        return False, 0, l1 and k <= 8
    first = next((c for c, n in enumerate(counts) if n > defer_min), None)
    if first is None:                                        # chunk loop, every chunk in the entry's own block
        return False, 0, False
    return True, sum(counts[first:]), False


# --------------------------------------------------------------------------- #
# CPU: the references and the families do what they say
# --------------------------------------------------------------------------- #
def test_ref_backup_on_hand_written_cases():
    # S = 2, A = 2, O = 1, R = 1, identity successors: score[b, a, v] = gamma b . (rto[:, a] alpha[v])
    rs = np.array([[[0], [0]], [[1], [1]]])
    rto = np.array([[[[0.5]], [[1.0]]], [[[0.5]], [[1.0]]]])             # action 0 halves, action 1 keeps
    er = np.array([[1.0, 0.0], [0.0, 0.0]])
    alpha = np.array([[2.0, 0.0], [0.0, 2.0], [2.0, 0.0]])                # row 2 copies row 0
    b = np.array([[1.0, 0.0], [0.0, 1.0], [0.5, 0.5]])
    r = ref_backup(alpha, b, rs, rto, er, 0.5)
    assert r['best'][:, :, 0].tolist() == [[0, 0], [1, 1], [0, 0]]        # first maximum among copies and ties
    assert r['values'].astype(float).tolist() == [[1.5, 1.0], [0.5, 1.0], [0.75, 0.5]]
    assert r['actions'].tolist() == [0, 1, 0]
    assert r['rows'].tolist() == [[1.5, 0.0], [0.0, 1.0], [1.5, 0.0]]
    # an exact tie of two actions resolves to the first
    r = ref_backup(alpha, np.array([[0.0, 1.0]]), rs, np.ones_like(rto), np.zeros((2, 2)), 0.5)
    assert r['values'][0, 0] == r['values'][0, 1] and r['actions'].tolist() == [0]
    # ... and the whole thing is the oracle's on a random model
    rng = np.random.default_rng(8)
    S, A, O, R, V, B = 50, 3, 2, 2, 11, 7
    rs, rto = successors(rng, S, A, R, False), sparse_rto(rng, S, A, O, R)
    er, alpha, b = rng.normal(size=(S, A)), rng.normal(size=(V, S)), rng.random((B, S))
    new, act, best = orc.backup_core(alpha, b, rs, rto, er, 0.9)
    r = ref_backup(alpha, b, rs, rto, er, 0.9)
    assert np.array_equal(r['best'], best) and np.array_equal(r['actions'], act)
    np.testing.assert_allclose(r['rows'], new, rtol=1e-13, atol=1e-14)


def test_planted_positions_cover_the_edges():
    for k in E_KS:
        pos = planted_positions(k)
        assert len(pos) == k == len(set(pos)) and pos == sorted(pos) and 0 < pos[0] and pos[-1] < E_V
        assert 255 in pos and 256 in pos                     # the chunk boundary of the candidate scan
        if k >= 3:
            assert pos[-1] == E_V - 1 and sum(p >= 512 for p in pos) >= 1       # the last, partly filled chunk
        if k >= 8:
            assert {254, 255, 256, 257, 511, 512} <= set(pos)
    assert chunk_counts(planted_positions(9)) == [3, 3, 3]
    assert chunk_counts(planted_positions(33)) == [12, 10, 11] and chunk_counts(planted_positions(33, late=True)) == [3, 19, 11]
    # what the layouts mean for k_refine (path_model): 8 | 9 and 32 | 33 are where the routing changes
    assert path_model(False, chunk_counts(planted_positions(8))) == (False, 0, False)
    assert path_model(True, chunk_counts(planted_positions(8))) == (False, 0, True)
    assert path_model(False, chunk_counts(planted_positions(9))) == (False, 0, False)
    assert path_model(False, chunk_counts(planted_positions(32))) == (True, 32, False)
    assert path_model(True, chunk_counts(planted_positions(32))) == (False, 0, False)
    assert path_model(True, chunk_counts(planted_positions(33))) == (True, 33, False)
    assert path_model(True, chunk_counts(planted_positions(33, late=True))) == (True, 30, False)
    assert path_model(True, chunk_counts(planted_positions(2)), defer_min=-1) == (True, 2, False)


@pytest.mark.parametrize('variant', E_VARIANTS)
@pytest.mark.parametrize('k', E_KS)
@pytest.mark.parametrize('shape', sorted(set(E_SHAPE.values())))
def test_family_e_margins_and_gap_classes(shape, k, variant):
    R, regular = shape
    p = e_problem(R, regular, k, variant)
    assert p.S == E_S and p.S % 32 != 0 and p.V == E_V and p.B == E_B and (p.A, p.O) == (2, 2)
    assert np.array_equal(p.alpha, f32r(p.alpha)) and np.array_equal(p.b * 64, np.round(p.b * 64))
    assert set(np.unique(p.rto)) == {0.25, 0.75} and np.array_equal(p.er, np.round(p.er))
    sc, mag = p.ref['scores'], p.mag
    assert np.array_equal(mag, ref_magnitude(p.alpha, p.b, p.rs, p.rto, p.gamma)) and np.all(mag > 0)       # nothing dead
    # exactness: longdouble sums give the same numbers
    assert np.array_equal(ref_scores(p.alpha, p.b, p.rs, p.rto, p.gamma, np.longdouble).astype(np.float64), sc)
    pos = np.array(p.positions)
    others = np.setdiff1d(np.arange(p.V), pos)
    top = sc.max(axis=2)
    # every other row lies more than 2^-8 of the magnitude below the maximum -- the widest window the project has (the split
    # GEMM's over this model's ten K tiles) is 130 times narrower -- and the planted ones within twice the narrowest window
    assert np.all(top[:, :, None] - sc[:, :, others] > 2.0 ** -8 * mag[:, :, None])
    widest = (8.0 * U24 * (np.sqrt(10 * 32 * 3.0) + 1.0) + 3.1 * 2.0 ** -16) * (1.0 + 2.0 ** -11) + 6.0 * U24
    assert 2.0 * widest < 2.0 ** -8 / 25
    narrow2 = 2.0 * 8.0 * U24 * (np.sqrt(32.0) + 1.0)
    assert np.all(top[:, :, None] - sc[:, :, pos] < narrow2 * mag[:, :, None])               # exactly k candidates everywhere
    # the gap class of the variant, per entry, in units of 2^-24 mag
    gain = e_gain_units(R, regular, p.positions, p.step)
    touching = np.zeros(p.B, dtype=bool)
    touching[0::2] = True
    assert np.all(gain[~touching] == 0) and np.all((gain[touching] > 0) == (variant != 'copies'))
    l1 = 2.0 * (R + 4)
    if variant == 'l1_gap':
        assert np.all(gain[touching] < l1) and np.all(gain[touching] <= 0.5 * l1)
    if variant == 'window_gap':
        assert np.all(gain[touching] > l1) and np.all(gain[touching] < narrow2 / U24)
        assert np.all(gain[touching] >= 2.0 * l1)            # (beyond the screen's own rounding as well)
    # who wins: the raised row (the last planted index) where the belief has weight on T's predecessor, else the smallest index
    want = np.where(touching[:, None] & (variant != 'copies'), pos[-1], pos[0])
    assert np.array_equal(p.ref['best'].reshape(p.B, 4), np.broadcast_to(want, (p.B, 4)))
    # the value maxima (b . alpha): some beliefs carry weight on T itself, the others see plain copies
    vm = np.argmax(p.b @ p.alpha.T, axis=1)
    assert set(vm.tolist()) == ({pos[0]} if variant == 'copies' else {pos[0], pos[-1]})


@pytest.mark.parametrize('variant', list(N_VARIANTS))
def test_family_n_has_no_undecidable_entry(variant):
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('np.longdouble is no wider than float64 here')
    for f32 in (True, False):
        p = n_problem(variant, f32)
        und, gap = undecidable(p)
        rel = (gap / p.mag)[(gap > 0) & (p.mag > 0)]
        print(f'\n[family N] {variant} f32={f32}: smallest non-zero relative gap {rel.min():.3e}, exact ties {(gap == 0).sum()}')
        assert und.sum() == 0
        assert np.array_equal(p.alpha[7], p.alpha[3])


def test_family_n_defeats_fp32_accumulation():
    """Scores accumulated in np.float32 (a GEMM without a window and a re-decision) pick another index than the
    longdouble reference in 6.2 % of the 420 entries of the projected-route model (seed 42), and in 6.2 % and 6.0 % of the
    entries of the two fused-route models (NumPy's float32 einsum; a GEMM's longer chains do worse).  Asserted: more than
    a tenth of the measured share, each."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('np.longdouble is no wider than float64 here')
    measured = {'proj': 0.062, 'fused1': 0.062, 'fused3': 0.060}
    for variant in N_VARIANTS:
        p = n_problem(variant, True)
        naive = np.argmax(ref_scores(p.alpha, p.b, p.rs, p.rto, p.gamma, np.float32), axis=2)
        share = float(np.mean(naive.reshape(p.ref['best'].shape) != p.ref['best']))
        print(f'\n[family N] {variant}: fp32-accumulated scores pick another index in {100 * share:.1f} % of {naive.size} entries')
        assert share > 0.1 * measured[variant]


@pytest.mark.parametrize('variant', ['proj', 'fused1'])
def test_action_models_plant_what_they_say(variant):
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('np.longdouble is no wider than float64 here')
    p = n_problem(variant, True, 'copy')
    v = p.ref['values']
    assert np.array_equal(v[:, 0], v[:, 2])                  # the copy's values are bit-equal
    pair_on_top = int(np.sum(v[:, 0] >= v[:, 1]))
    print(f'\n[actions] {variant}: the planted pair is best for {pair_on_top} of {p.B} beliefs')
    assert 10 <= pair_on_top <= p.B - 10
    assert set(p.ref['actions'].tolist()) == {0, 1}          # copies resolve to action 0
    for eps in (1e-8, 1e-10):
        q = n_problem(variant, True, 'eps', eps)
        assert np.array_equal(q.er, f32r(q.er))
        differs = int(np.sum(q.er[:, 2] != q.er[:, 0]))
        print(f'[actions] {variant} eps={eps:g}: {differs} of {q.S} rewards differ from the copy after rounding to fp32')
        assert differs < q.S // 2                            # most round back to the copy's
    # exact arithmetic: the raised reward wins where the belief holds weight on its state and the pair is best
    e = e_problem(3, False, 33, 'copies', False, 'raised')
    ev = e.ref['values']
    w = e.b[:, 77] > 0
    assert np.all(ev[w, 2] > ev[w, 0]) and np.all(ev[~w, 2] == ev[~w, 0])
    assert np.all(ev[w, 2] - ev[w, 0] == 2.0 ** -24)         # 4 / 64 of the step
    assert {0, 2} <= set(e.ref['actions'].tolist())


# --------------------------------------------------------------------------- #
# GPU: family E on every route
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize('k', E_KS)
@pytest.mark.parametrize('name', list(ROUTES))
def test_family_e_on_every_route(name, k):
    dtype = ROUTES[name][0]
    l1 = has_l1(name)
    first = e_case(name, k, 'copies')
    with routed_engine(name, first) as (eng, checks):
        for variant in E_VARIANTS:
            p = e_case(name, k, variant)
            tag = f'{name} k={k} {variant}'
            st, res = run_backup(eng, p, checks)
            check_result(p, res, dtype, tag)
            pairs = p.B * p.A * p.O
            assert st['n_pairs'] == pairs and st['n_dead'] == 0 and st['n_refined_actions'] <= p.B, (tag, st)
            if name == 'f64_pure':
                assert st['n_refined'] == 0 and st['n_refine_candidates'] == 0, (tag, st)
            else:
                assert st['n_refined'] == pairs, (tag, st)
                c = eng.debug_refine_counts()
                deferred, listed, split = path_model(l1, chunk_counts(p.positions))
                print(f'\n[paths] {tag}: {c}  candidates {st["n_refine_candidates"]}')
                assert c['slots'] == (pairs if deferred else 0) and c['items'] == 0, (tag, c)
                assert c['w_slot_cap'] >= pairs and c['defer_min'] == 8, (tag, c)
                if os.environ.get('PBVI_REFINE_INBLOCK') is None and not deferred:
                    assert st['n_refine_candidates'] == k * pairs, (tag, st)     # include/pbvi_hip.h: exact off the GEMM path
                assert st['n_refine_candidates'] >= 2 * pairs, (tag, st)
                if l1:                                       # entries the screen separates nothing of: (i), (ii) all, (iii) the untouched
                    want_q2 = 0 if not split else (pairs // 2 if variant == 'window_gap' else pairs)
                    assert c['q2'] == want_q2, (tag, c)
            if dtype == 'f32':
                check_value_max(eng, p, tag)
                c = eng.debug_refine_counts()
                deferred, listed, _ = path_model(False, chunk_counts(p.positions))
                # (the step of variant (iii) is sized for the backup's scores: in b . alpha the raised row may leave the
                # copies outside the window of the beliefs that hold weight on T, which then have a single candidate)
                loose = int(np.sum(p.b[:, p.T] > 0)) if variant == 'window_gap' else 0
                assert 0 < 4 * loose <= p.B or variant != 'window_gap', tag
                want = p.B if deferred else 0
                assert max(0, want - loose) <= c['slots'] <= want and c['items'] == 0 and c['q2'] == 0, (tag, c)


# --------------------------------------------------------------------------- #
# GPU: the forced paths
# --------------------------------------------------------------------------- #
# setting -> (environment, candidates k, layouts (late?), variants)
FORCED = {
    'gemm_default': ({}, 33, (False,), ('copies', 'l1_gap')),
    'items_only': ({'PBVI_REFINE_W_SLOTS': '0'}, 33, (False, True), ('copies', 'l1_gap')),
    'one_gemm_slot': ({'PBVI_REFINE_W_SLOTS': '1'}, 33, (False, True), ('copies', 'l1_gap')),
    'items_void_all': ({'PBVI_REFINE_W_SLOTS': '0', 'PBVI_REFINE_ITEM_CAP': '20'}, 33, (False, True), ('copies', 'l1_gap')),
    'items_void_some': ({'PBVI_REFINE_W_SLOTS': '0', 'PBVI_REFINE_ITEM_CAP': '50'}, 33, (False, True), ('copies', 'l1_gap')),
    'slots_exhausted': ({'PBVI_REFINE_SLOT_CAP': '1'}, 33, (False, True), ('copies', 'l1_gap')),
    'defer_all_k2': ({'PBVI_REFINE_DEFER_MIN': '-1'}, 2, (False,), ('copies', 'l1_gap', 'window_gap')),
    'defer_all_k3': ({'PBVI_REFINE_DEFER_MIN': '-1'}, 3, (False,), ('copies', 'l1_gap', 'window_gap')),
    'defer_all_k3_items': ({'PBVI_REFINE_DEFER_MIN': '-1', 'PBVI_REFINE_W_SLOTS': '0'}, 3, (False,), ('copies', 'l1_gap')),
    'split_overflow': ({'PBVI_REFINE_Q2_CAP': '1'}, 8, (False,), ('l1_gap',)),
}
FORCED_ROUTES = ('f32_projected', 'f32_fused_r1', 'f64_screen_alpha')


def check_forced_counts(setting, c, n, listed, k, deferred, split, tag):
    """`c` = debug_refine_counts after a pass over n entries of k candidates each (`listed` of them behind the first chunk
    that defers), against the table of the module docstring."""
    if setting == 'split_overflow':
        if split:
            assert c['q2_cap'] == 1 and c['q2'] == n > c['q2_cap'], (tag, c)
        return
    assert deferred, tag
    if setting == 'gemm_default':
        assert c['slots'] == n and c['items'] == 0 and c['w_slot_cap'] >= n, (tag, c)
    elif setting == 'items_only' or setting == 'defer_all_k3_items':
        assert c['w_slot_cap'] == 0 and c['slots'] == n and c['items'] == listed * c['slots'] <= c['item_cap'], (tag, c)
        assert (listed == k) == (c['items'] == k * c['slots']), (tag, c)
    elif setting == 'one_gemm_slot':
        assert c['w_slot_cap'] == 1 and c['slots'] == n > 1 and c['items'] == listed * (n - 1), (tag, c)
        assert 0 < c['items'] < k * c['slots'], (tag, c)
    elif setting.startswith('items_void'):
        assert c['w_slot_cap'] == 0 and c['slots'] == n and c['items'] == listed * n > c['item_cap'], (tag, c)
        assert (c['item_cap'] < k) if setting == 'items_void_all' else (k <= c['item_cap'] < 2 * k), (tag, c)
    elif setting == 'slots_exhausted':
        assert c['slot_cap'] == 1 and c['slots'] > c['slot_cap'] and c['items'] == 0, (tag, c)
    elif setting.startswith('defer_all_k'):
        assert k <= 8 and c['defer_min'] == -1 and c['slots'] == n and c['items'] == 0, (tag, c)


@gpu
@pytest.mark.parametrize('name', FORCED_ROUTES)
@pytest.mark.parametrize('setting', list(FORCED))
def test_forced_refinement_paths(setting, name, monkeypatch):
    env, k, layouts, variants = FORCED[setting]
    dtype = ROUTES[name][0]
    l1 = has_l1(name)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    defer_min = int(env.get('PBVI_REFINE_DEFER_MIN', 8))
    with routed_engine(name, e_case(name, k, 'copies')) as (eng, checks):
        for late in layouts:
            for variant in variants:
                p = e_case(name, k, variant, late)
                tag = f'{setting} {name} k={k} late={late} {variant}'
                st, res = run_backup(eng, p, checks)
                check_result(p, res, dtype, tag)
                pairs = p.B * p.A * p.O
                assert st['n_refined'] == pairs, (tag, st)
                c = eng.debug_refine_counts()
                print(f'\n[forced] {tag}: {c}')
                deferred, listed, split = path_model(l1, chunk_counts(p.positions), defer_min)
                check_forced_counts(setting, c, pairs, listed, k, deferred, split, tag)
                if dtype == 'f32':                           # the value maxima: the same kernels with PROJ = false, G = 1
                    check_value_max(eng, p, tag + ' value-max')
                    c = eng.debug_refine_counts()
                    print(f'[forced] {tag} value-max: {c}')
                    deferred, listed, _ = path_model(False, chunk_counts(p.positions), defer_min)
                    check_forced_counts(setting, c, p.B, listed, k, deferred, False, tag + ' value-max')
    # the inexact family through the same capacities: the reference's results (what ran depends on its candidate counts)
    p = n_case(name)
    with routed_engine(name, p) as (eng, checks):
        st, res = run_backup(eng, p, checks)
        check_result(p, res, dtype, f'{setting} {name} family N')
        print(f'[forced] {setting} {name} family N: {eng.debug_refine_counts()}')


@gpu
@pytest.mark.parametrize('cap', [1, 100, 300])
def test_split_overflow_keeps_equal_scores_equal(cap, monkeypatch):
    """The copy-action model (A = 7: five copies of one action; V = 8, so every entry goes through the level-1 screen) with
    k_refine_split's hand-over cut to `cap` of its 1799 entries: which entries find room is a race, and the members of a
    duplicate action group land on either side of it.  Their exact scores must still be the same bits, or the action
    tail's first maximum goes to a copy.  (Caught by ``test_action_mapping_at_every_action_count[256-1]``: 65792 entries
    against the default capacity of 16384; the overflow used to sum the whole tile list at once, the hand-over in sixteen
    parts.)"""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('np.longdouble is no wider than float64 here')
    monkeypatch.setenv('PBVI_REFINE_Q2_CAP', str(cap))
    p = n_problem('proj', True, 'copy', 0.0, 299, 7, 1, 64, 8, 257)
    with routed_engine('f32_projected', p) as (eng, checks):
        for _ in range(2):                                   # (a race: twice)
            st, res = run_backup(eng, p, checks)
            c = eng.debug_refine_counts()
            print(f'\n[split overflow] cap {cap}: {c}, refined actions {st["n_refined_actions"]}')
            assert c['q2_cap'] == cap and (c['q2'] > cap or cap > 100), c      # both sides of the capacity are populated
            check_result(p, res, 'f32', f'split overflow cap={cap}')
            assert st['n_refined_actions'] >= planted_pair_best(p) > 0


def child_digests():
    """What tests/decision_paths_child.py prints: (label, problem) of family E at k = 3 and 33 and family N on the
    projected fp32 route."""
    out = [(f'E{k}{v}', e_case('f32_projected', k, v)) for k in (3, 33) for v in E_VARIANTS]
    return out + [('N', n_case('f32_projected'))]


def run_child_cases():
    lines = []
    for label, p in child_digests():
        with routed_engine('f32_projected', p) as (eng, checks):
            st, res = run_backup(eng, p, checks)
            c = eng.debug_refine_counts()
            rows = np.asarray(res.alpha)
            if not p.exact:                                  # inexact rows are compared by the parent's tolerance, not here
                check_result(p, res, 'f32', label)
                rows = np.zeros(0)
            lines.append(f'decision-sha256 {label} {digest(res.best_alpha_ind, res.actions, rows)} '
                         f'items={c["items"]} slots={c["slots"]} q2={c["q2"]} w={c["w_slot_cap"]}')
    return lines


@gpu
@pytest.mark.parametrize('switch', ['PBVI_REFINE_INBLOCK', 'PBVI_NO_L1_SCREEN'])
def test_once_per_process_switches_in_a_child(switch):
    """``PBVI_REFINE_INBLOCK`` (no work list: every candidate in the entry's own block) and ``PBVI_NO_L1_SCREEN`` are read
    once per process: a fresh child each, one at a time, under its own time limit; the digests of (indices, actions, row
    bytes) must be the reference's."""
    env = dict(os.environ)
    env[switch] = '1'
    child = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'decision_paths_child.py')], env=env, cwd=REPO,
                           stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stdout + child.stderr
    got = {ln.split()[1]: ln.split()[2:] for ln in child.stdout.splitlines() if ln.startswith('decision-sha256 ')}
    want = child_digests()
    assert sorted(got) == sorted(label for label, _ in want), child.stdout + child.stderr
    for label, p in want:
        ref = p.ref
        rows = ref['rows'].astype(np.float32) if p.exact else np.zeros(0)
        assert got[label][0] == digest(ref['best'], ref['actions'], rows), (switch, label, got[label])
        counts = dict(kv.split('=') for kv in got[label][1:])
        if switch == 'PBVI_REFINE_INBLOCK':                  # no work list at all
            assert counts == {'items': '0', 'slots': '0', 'q2': '0', 'w': '0'}, (label, counts)
        elif p.exact:                                        # no screen: nothing is handed to k_refine_split
            assert counts['q2'] == '0' and (int(counts['slots']) > 0) == (p.k == 33), (label, counts)


# --------------------------------------------------------------------------- #
# GPU: family N on every route
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize('name', list(ROUTES))
def test_family_n_on_every_route(name):
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('np.longdouble is no wider than float64 here')
    dtype = ROUTES[name][0]
    p = n_case(name)
    und, _ = undecidable(p)
    assert und.sum() == 0                                    # (fp64 operands included: no allowance below)
    with routed_engine(name, p) as (eng, checks):
        st, res = run_backup(eng, p, checks)
        check_result(p, res, dtype, name)
        print(f'\n[family N] {name}: refined {st["n_refined"]} of {st["n_pairs"]}, actions {st["n_refined_actions"]}, '
              f'counts {eng.debug_refine_counts() if name != "f64_pure" else None}')
        if name == 'f64_pure':
            assert st['n_refined'] == 0
        else:
            assert st['n_refined'] > 0.5 * st['n_pairs'], st
        assert st['n_refined_actions'] <= p.B


# --------------------------------------------------------------------------- #
# GPU: the action tail
# --------------------------------------------------------------------------- #
def planted_pair_best(p):
    """Beliefs whose best action value is attained by more than one action (the planted copies)."""
    v = p.ref['values']
    return int(np.sum((v == v.max(axis=1, keepdims=True)).sum(axis=1) > 1))


@gpu
@pytest.mark.parametrize('name', list(ROUTES))
def test_action_copies_and_near_copies(name):
    """Action 2 = action 0 (exactly, or up to 1e-8 / 1e-10 of its rewards): first maximum, from exact values."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('np.longdouble is no wider than float64 here')
    dtype = ROUTES[name][0]
    models = [('copy', n_case(name, 'copy')), ('copy plain', n_case(name, 'copy', plain=True))]
    if dtype == 'f32':
        models += [(f'eps{eps:g}', n_case(name, 'eps', eps)) for eps in (1e-8, 1e-10)]
    models += [('E copy', e_case(name, 33, 'l1_gap', False, 'copy')), ('E raised', e_case(name, 33, 'copies', False, 'raised'))]
    for label, p in models:
        with routed_engine(name, p) as (eng, checks):
            st, res = run_backup(eng, p, checks)
            tag = f'{name} {label}'
            check_result(p, res, dtype, tag)
            tied = planted_pair_best(p)
            print(f'\n[actions] {tag}: refined actions {st["n_refined_actions"]} of {p.B}, planted pair best and tied for {tied}')
            assert st['n_refined_actions'] <= p.B, (tag, st)
            if label in ('copy', 'copy plain', 'E copy'):
                assert tied >= 10 and set(res.actions.tolist()) <= {0, 1}, tag
                if name in REWARD_WINDOW:
                    assert st['n_refined_actions'] >= tied > 0, (tag, st)
            if label == 'copy plain' and name in WINDOWED:
                # hardly an entry was refined: the scores behind the tied values still carry their windows, so the pair is
                # queued on the belief side too (whose reward term is exact), and k_refine_action re-scores them itself
                assert st['n_refined'] < 0.2 * st['n_pairs'] and st['n_refined_actions'] >= tied > 0, (tag, st)
            if name == 'f64_pure':
                assert st['n_refined_actions'] == 0, (tag, st)


@gpu
@pytest.mark.parametrize('O', [1, 2])
@pytest.mark.parametrize('A', [1, 3, 7, 86, 129, 256])
def test_action_mapping_at_every_action_count(A, O):
    """k_action_select's ``lb = tid / A``, ``per_block = 256 / A`` with ties at action counts that do not divide 256, one
    and several blocks: the copy model tiled cyclically from its 3-action base."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('np.longdouble is no wider than float64 here')
    for name in ('f32_projected', 'f32_belief_side', 'f64_screen_alpha'):
        dtype = ROUTES[name][0]
        for B in (1, 5, 257):
            p = n_problem('proj', dtype == 'f32', 'copy', 0.0, 42 + B, A, O, 64, 8, B)
            with routed_engine(name, p) as (eng, checks):
                st, res = run_backup(eng, p, checks)
                tag = f'{name} A={A} O={O} B={B}'
                print(f'\n[action mapping] {tag}: refined actions {st["n_refined_actions"]}, {eng.debug_refine_counts()}')
                check_result(p, res, dtype, tag)
                tied = planted_pair_best(p)
                assert st['n_refined_actions'] <= B, (tag, st)
                if A == 1:
                    assert st['n_refined_actions'] == 0 and tied == 0, (tag, st)
                elif name in REWARD_WINDOW:
                    assert st['n_refined_actions'] >= tied, (tag, st, tied)
                    assert B == 1 or tied > 0, tag


@gpu
@pytest.mark.parametrize('name', ['f32_projected', 'f32_fused_r1', 'f32_belief_side', 'f64_screen_alpha'])
def test_run_fetch_with_planted_actions(name):
    """``run_fetch_into`` on the copy and the 1e-8 model: the slots, index, actions and rows of ``run`` + ``fetch`` -- the
    early rows' provisional decision is overturned by the ACTION refinement here."""
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('np.longdouble is no wider than float64 here')
    from pomdp_pbvi_exploration_amd.engine import PinnedBuffer
    dtype = ROUTES[name][0]
    for label, p in [('copy', n_case(name, 'copy'))] + ([('eps', n_case(name, 'eps', 1e-8))] if dtype == 'f32' else []):
        with routed_engine(name, p) as (eng, checks):
            st, want = run_backup(eng, p, checks)
            check_result(p, want, dtype, f'{name} {label}')
            buf = PinnedBuffer(p.B * p.S * 8 + 3 * p.B * 4 + 8192)
            rows = buf.carve((p.B, p.S), eng.np_dtype)
            slot, index, actions = (buf.carve((p.B,), np.int32) for _ in range(3))
            best = np.empty((p.B, p.A, p.O), dtype=np.int32)
            for with_best in (False, True):                  # the publish kernel, then the staged copy
                rows[:] = np.nan
                slot[:], index[:], actions[:] = -7, -7, -7
                st2, U, used = eng.run_fetch_into(p.gamma, rows, slot, index, actions, best=best if with_best else None)
                tag = f'{name} {label} best={with_best}'
                assert U == want.unique_alpha.shape[0] and U <= used <= p.B, tag
                assert np.array_equal(index, want.index) and np.array_equal(actions, want.actions), tag
                assert np.array_equal(actions, p.ref['actions']), tag
                assert len(set(slot[:U].tolist())) == U and np.all((slot[:U] >= 0) & (slot[:U] < used)), tag
                assert np.asarray(rows)[slot[:U]].tobytes() == np.asarray(want.unique_alpha).tobytes(), tag
                if with_best:
                    assert np.array_equal(best, p.ref['best']), tag
                for key in ('n_refined', 'n_refined_actions', 'n_unique'):
                    assert st2[key] == st[key], (tag, key)


@gpu
@pytest.mark.parametrize('name', ['f32_projected', 'f32_fused_r1', 'f64_screen_alpha'])
def test_speculation_repeats_the_decision(name):
    """One engine, alpha sets plain, tied, tied, plain, tied on the copy-action model: after a backup that deferred nothing
    the next one speculates, finds deferred work at the end and runs the decision stages again -- its results and counts
    are those of the synchronous call that follows it."""
    dtype = ROUTES[name][0]
    R, regular = E_SHAPE[ROUTES[name][1]]
    tied = e_case(name, 33, 'l1_gap', False, 'copy')
    plain = tied.with_alpha(e_plain_alpha(R, regular, 'copy'))
    seen = []
    with routed_engine(name, tied) as (eng, checks):
        for label, p in (('plain', plain), ('tied', tied), ('tied', tied), ('plain', plain), ('tied', tied)):
            st, res = run_backup(eng, p, checks)
            check_result(p, res, dtype, f'{name} {label} #{len(seen)}')
            c = eng.debug_refine_counts()
            assert (c['slots'] > 0) == (label == 'tied'), (label, c)
            seen.append(st)
    for key in ('n_refined', 'n_refined_actions', 'n_unique', 'n_refine_candidates'):
        assert seen[1][key] == seen[2][key] == seen[4][key], (key, [s[key] for s in seen])
        assert seen[0][key] == seen[3][key], key
    assert seen[1]['n_refined_actions'] >= planted_pair_best(tied) > 0


# --------------------------------------------------------------------------- #
# GPU: the read-out's own contract
# --------------------------------------------------------------------------- #
@gpu
def test_refine_counts_contract():
    """Nothing to read before the first refinement pass, nor on a pure fp64 engine, which never runs one; afterwards the
    counts are those of the most recent pass: the backup's, then the value maxima's."""
    p = e_case('f32_projected', 33, 'copies')
    with routed_engine('f32_projected', p) as (eng, checks):
        with pytest.raises(ValueError, match='no refinement has run'):
            eng.debug_refine_counts()
        run_backup(eng, p, checks)
        c = eng.debug_refine_counts()
        assert sorted(c) == sorted(['items', 'slots', 'q2', 'item_cap', 'slot_cap', 'w_slot_cap', 'q2_cap', 'defer_min'])
        assert c == eng.debug_refine_counts()                # reading changes nothing
        assert c['slots'] == p.B * p.A * p.O and c['q2_cap'] == min(p.B * p.A * p.O, 16384) and c['item_cap'] >= 1 << 16
        eng.max_value_resident()
        assert eng.debug_refine_counts()['slots'] == p.B
    with routed_engine('f64_pure', p) as (eng, checks):
        run_backup(eng, p, checks)
        with pytest.raises(ValueError, match='no refinement has run'):
            eng.debug_refine_counts()
