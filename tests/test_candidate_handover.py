"""k_argmax hands the candidates of every row it queues to k_refine (``hcand`` / ``hncand``, backup_kernels.h) and appends a
block's queued rows with one atomic.  Neither may change a result:

1. hand-over equals scan   every case runs once here (hand-over on) and once in a child process with
                           ``PBVI_NO_CAND_HANDOVER=1`` (read once per process: k_refine ignores the lists and walks the
                           scores itself); what the score probe captured behind the argmax (first maxima, windows, the
                           queue as a set), the result (indices, actions, row bytes), the Q-values of the same block
                           (``q_values_resident``: Q, its actions and the refined ``best`` -- the argmax and the
                           refinement once more, on the ``pbvi_q_values`` route, and the refined scores summed into Q)
                           and every counter (``n_refined``, ``n_refine_candidates``, ``n_refined_actions``,
                           ``debug_refine_counts``) go into one sha256 per case and the two digests must be equal.  In this process the counters are also held
                           against the rule itself, evaluated on the host from the probe's scores: an entry's candidates
                           are the columns with score >= m - 2E, and ``n_refine_candidates`` is their number over the
                           queued entries.
2. the window's edge       a runner-up on the smallest fp32 score >= m - 2E is a candidate, the next fp32 below is not.
3. the queue as a set      B * G below, at and one above a block's rows; every row queued; none; some.
4. order independence      plain -> tied -> tied -> plain through one engine: each call equals a fresh engine's.

The inputs are exact: rto in {0.25, 0.75}, gamma = 0.5, beliefs in multiples of 1/64, small-integer alpha rows and rewards
(tests/decision_cases.py, family E).  Every sum is exact in fp32 in any order, so the k copies of the top row tie bit for
bit on every (belief, group) whatever the GEMM's schedule, every other row lies at least 0.25 below, and each queued entry
has exactly k candidates.  In those cases the first candidate always wins, so the ``later_winner`` cases add one where it
does not: eight candidates tie at 1.5 in fp32, and the third of them is 2^-25 higher in exact arithmetic (below half an
fp32 ulp of the sum), so the refinement's answer depends on what the list holds behind its first element.
"""
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from decision_cases import Problem
from test_score_window import gap_case, ragged_chunk_rows, ref_argmax, successors

gpu = pytest.mark.gpu
GAMMA = 0.5
BLOCK_ROWS = 16                                              # backup_kernels.hip: ARGMAX_BLOCK_ROWS
QCAND = 8                                                    # backup_kernels.h


# --------------------------------------------------------------------------- #
# Inputs
# --------------------------------------------------------------------------- #
def tie_positions(V, k):
    """k columns of [0, V): spread evenly, the last column among them from k = 2 on; k = 8 and 9 also get neighbours across
    the 256-column boundary when V has one."""
    pos = set(np.linspace(0, V - 1, k).round().astype(int).tolist()) if k > 1 else {V // 2}
    extra = [255, 256, 3, 64, 1023, 1024, 1, 2]
    for v in extra:
        if len(pos) >= k:
            break
        if v < V:
            pos.add(v)
    v = 0
    while len(pos) < k:
        pos.add(v)
        v += 1
    out = sorted(pos)
    assert len(out) == k
    return out


@functools.lru_cache(maxsize=None)
def tie_problem(S, V, B, k, R=1, regular=False, A=2, O=2, identity=False, seed=0):
    """The top row (integers in [-8, 8]) at ``tie_positions(V, k)``; every other row is the top row minus 2 or 3 minus
    0 / 1 / 2 per state.  identity: every state is its own successor."""
    rng = np.random.default_rng(7000 + 31 * S + 7 * V + B + 1000 * R + seed)
    rs = np.arange(S, dtype=np.int64)[:, None, None].repeat(A, axis=1).repeat(R, axis=2) if identity else successors(rng, S, A, R, regular)
    rto = np.where(rng.random((S, A, 1, R)) < 0.5, 0.25, 0.75) * np.ones((1, 1, O, 1))
    if O > 1:
        rto[:, :, 1, :] = 1.0 - rto[:, :, 0, :]
    er = rng.integers(-4, 5, size=(S, A)).astype(np.float64)
    top = rng.integers(-8, 9, size=S).astype(np.float64)
    alpha = top[None, :] - rng.integers(2, 4, size=(V, 1)) - rng.integers(0, 3, size=(V, S))
    pos = tie_positions(V, k)
    alpha[pos] = top
    b = np.zeros((B, S))
    for i in range(B):
        np.add.at(b[i], rng.integers(0, S, size=64), 1.0 / 64.0)
    return Problem(np.ascontiguousarray(rs), rto, er, alpha, b, GAMMA, True, positions=pos, k=k)


LATER_COLUMNS = (1, 9, 20, 31, 40, 47, 55, 63)               # the eight candidates; column 20 wins in fp64
LATER_WINNER = 20


@functools.lru_cache(maxsize=None)
def later_winner_problem():
    """test_score_window.gap_case's model (S = 24, one K tile, A * O = 2, gamma RTO = 1/2 with gamma = 1) and its belief 0,
    (1/4, 1/2, 1/4) on states 0 .. 2.  The rows at LATER_COLUMNS are the constant 3 and score 1.5; row LATER_WINNER holds
    3 + 2^-22 on state 2 and scores 1.5 + 2^-25 exactly, which every fp32 summation order rounds to 1.5."""
    rs, rto, alpha, b = gap_case(64, LATER_COLUMNS[0], LATER_COLUMNS[1], 2.0 ** -10)
    alpha[list(LATER_COLUMNS)] = 3.0
    alpha[LATER_WINNER, 2] = 3.0 + 2.0 ** -22
    er = np.zeros((rs.shape[0], 1))
    return Problem(rs, rto, er, alpha, b[:1], 1.0, True, positions=list(LATER_COLUMNS), k=len(LATER_COLUMNS))


def route_engine(prob, route):
    """fp32 engine on the projected route by default; the named routes of the issue otherwise."""
    eng = prob.engine('f64' if route == 'f64_screen' else 'f32')
    if route == 'f64_screen':
        eng.set_f64_screen('always')
        eng.set_formulation('alpha')
    else:
        eng.set_formulation('belief' if route == 'belief' else 'alpha')
        eng.set_fused_projection(1 if route == 'fused' else 0)
    if route == 'tiled':
        eng.set_gamma_tiling('always', ragged_chunk_rows(prob.V))
    eng.debug_score_probe(True)
    return eng


# label -> (problem arguments, route, run with the belief-dominance test)
def build_cases():
    cases = {}
    for k in (1, 2, 8, 9, 33, 300):                          # candidates per entry (k = 1: nothing queued by the main argmax;
        cases[f'cand_k{k}'] = (dict(S=33, V=300, B=7, k=k), 'projected', k == 1)      # the dominance test's value-max flags all)
    for i, V in enumerate((3, 63, 64, 255, 256, 257, 1024, 1025, 1029)):
        cases[f'V{V}'] = (dict(S=33, V=V, B=3, k=min(V, 8 + i % 2)), 'projected', False)
    for S in (33, 4097):
        for B in (1, 255, 257):
            cases[f'S{S}_B{B}'] = (dict(S=S, V=260, B=B, k=8), 'projected', False)
    cases['route_fused_r1'] = (dict(S=330, V=300, B=40, k=8, R=1, regular=True), 'fused', False)
    cases['route_projected_r1'] = (dict(S=330, V=300, B=40, k=8, R=1, regular=True), 'projected', False)
    cases['route_l1_r3_k8'] = (dict(S=330, V=300, B=40, k=8, R=3), 'projected', False)
    cases['route_l1_r3_k9'] = (dict(S=330, V=300, B=40, k=9, R=3), 'projected', False)
    cases['route_f64_screen'] = (dict(S=330, V=300, B=40, k=8, R=2), 'f64_screen', False)
    cases['route_belief_side'] = (dict(S=330, V=300, B=40, k=8, R=2), 'belief', False)
    cases['route_belief_side_V1029'] = (dict(S=33, V=1029, B=3, k=9), 'belief', False)
    cases['route_tiled_3_chunks'] = (dict(S=330, V=300, B=40, k=8, R=2), 'tiled', False)
    cases['later_winner_projected'] = (None, 'projected', False)          # level-1 screen, then k_refine_split
    cases['later_winner_fused'] = (None, 'fused', False)                  # the eight scored together in the entry's block
    return cases


CASES = build_cases()
GROUPS = {'cand': [c for c in CASES if c.startswith('cand')], 'V': [c for c in CASES if c.startswith('V')],
          'shape': [c for c in CASES if c.startswith('S')], 'route': [c for c in CASES if c.startswith('route')],
          'later': [c for c in CASES if c.startswith('later')]}


def host_candidates(p):
    """(queued [B][G], candidates per entry [B][G]) by the rule, from what the probe captured."""
    m, idx, m2, flag = ref_argmax(p['score'], p['E'])
    live = ~p['dead'].astype(bool)
    count = (p['score'] >= (m - 2.0 * p['E'])[:, :, None]).sum(axis=2)
    return flag & live, count


def run_case(label):
    """One backup of the case; (digest line, stats, probe, result)."""
    kw, route, dominance = CASES[label]
    prob = later_winner_problem() if kw is None else tie_problem(**kw)
    eng = route_engine(prob, route)
    try:
        eng.set_alpha(prob.alpha)
        eng.set_beliefs(prob.b)
        st = eng.run(prob.gamma, belief_dominance_prune=dominance)
        res = eng.fetch()
        p = eng.debug_score_probe_fetch()
        counts = eng.debug_refine_counts()
        res.q = eng.q_values_resident(prob.gamma, want_best=True)          # (Q [B, A], actions [B], best [B, A, O]), caller order
    finally:
        eng.close()
    h = hashlib.sha256()
    for name in ('perm', 'best_v', 'best_score', 'E'):
        h.update(np.ascontiguousarray(p[name]).tobytes())
    h.update(np.sort(p['queue'].astype(np.int64)).tobytes())
    h.update(np.ascontiguousarray(res.best_alpha_ind, dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(res.actions, dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(res.alpha).tobytes())
    for arr in res.q:
        h.update(np.ascontiguousarray(arr).tobytes())
    numbers = {k: int(st[k]) for k in ('n_refined', 'n_refine_candidates', 'n_refined_actions')}
    numbers.update({k: counts[k] for k in ('items', 'slots', 'q2')})
    line = f'handover-sha256 {label} {h.hexdigest()} {json.dumps(numbers, sort_keys=True)}'
    return line, st, p, res, prob


@functools.lru_cache(maxsize=None)
def child_lines(group):
    """The group's cases in a child process with the hand-over switched off."""
    env = dict(os.environ)
    env['PBVI_NO_CAND_HANDOVER'] = '1'
    child = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'candidate_handover_child.py'), group], env=env,
                           cwd=REPO, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=240)
    assert child.returncode == 0, child.stdout + child.stderr
    return {ln.split()[1]: ln for ln in child.stdout.splitlines() if ln.startswith('handover-sha256 ')}


# --------------------------------------------------------------------------- #
# CPU: the inputs are what they say
# --------------------------------------------------------------------------- #
def test_cases_plant_exact_ties():
    for V, k in ((3, 2), (300, 1), (300, 9), (1029, 8), (260, 260)):
        pos = tie_positions(V, k)
        assert len(set(pos)) == k and 0 <= pos[0] and pos[-1] < V and (k == 1 or pos[-1] == V - 1)
    prob = tie_problem(S=33, V=300, B=7, k=9)
    sc = prob.ref['scores']
    assert np.array_equal(sc, sc.astype(np.float32).astype(np.float64))          # exact in fp32
    top = sc.max(axis=2)
    assert np.all((sc == top[:, :, None]).sum(axis=2) == 9)
    rest = np.delete(sc, prob.positions, axis=2)
    assert np.all(top - rest.max(axis=2) >= 0.25)
    assert sorted(sum(GROUPS.values(), [])) == sorted(CASES)


# --------------------------------------------------------------------------- #
# 1. hand-over equals scan
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize('label', list(CASES))
def test_handover_equals_scan(label):
    line, st, p, res, prob = run_case(label)
    group = next(g for g, labels in GROUPS.items() if label in labels)
    theirs = child_lines(group)
    assert label in theirs, sorted(theirs)
    print(f'\n[handover] on:  {line}\n[handover] off: {theirs[label]}')
    assert theirs[label] == line
    # the rule on the host, from the probe: who is queued, how many candidates each entry has
    queued, count = host_candidates(p)
    assert np.array_equal(np.sort(p['queue'].astype(np.int64)), np.flatnonzero(queued.ravel())), label
    k = prob.k
    if label.startswith('S4097'):                            # the pairs' K lists are split: scores are slab 0 plus continuation tiles
        assert 0 < p['chain_steps'] < (4097 + 31) // 32, (label, p['chain_steps'])
    if label.startswith('later'):                            # the first candidate is the fp32 maximum, a later one the exact one
        assert np.all(p['best_v'] == LATER_COLUMNS[0]) and np.all(res.best_alpha_ind == LATER_WINNER), label
        assert np.all(p['score'][:, :, list(LATER_COLUMNS)] == 1.5), label
    assert queued.all() if k > 1 else not queued.any(), label
    assert np.all(count == k), (label, np.unique(count))
    # (the counter sees every candidate where the entry's own block collects them whole: up to 8, or up to 32 in front of the
    # level-1 screen of the projected route; the dominance test's value-max refines entries of its own)
    route, dominance = CASES[label][1:]
    if not dominance:
        assert st['n_refined'] == int(queued.sum()), (label, st)
        if k <= QCAND or (k <= 32 and route == 'projected'):
            assert st['n_refine_candidates'] == int(count[queued].sum()), (label, st)
    # ... and the decision is the reference's
    ref = prob.ref
    assert np.array_equal(res.best_alpha_ind, ref['best']) and np.array_equal(res.actions, ref['actions']), label
    want = ref['rows'].astype(np.asarray(res.alpha).dtype)
    assert np.asarray(res.alpha).tobytes() == want.tobytes(), label
    q, q_act, q_best = res.q
    assert np.array_equal(q_best, ref['best']), label
    np.testing.assert_allclose(q, ref['values'].astype(np.float64), rtol=1e-12, atol=0, err_msg=label)     # exact in fp64


# --------------------------------------------------------------------------- #
# 2. the window's edge
# --------------------------------------------------------------------------- #
def edge_problem(V, gap):
    """test_score_window.gap_case's belief 0: the winner p scores 1.5, its exact copy c too, row q scores 1.5 - gap."""
    p_, q, c = V // 2, V // 2 + 5, V - 1
    rs, rto, alpha, b = gap_case(V, p_, q, gap)
    alpha[c] = alpha[p_]
    er = np.zeros((rs.shape[0], 1))
    return Problem(rs, rto, er, alpha, b[:1], 1.0, True, p=p_, q=q, c=c)


def run_edge(V, gap):
    prob = edge_problem(V, gap)
    eng = prob.engine('f32')
    try:
        eng.set_score_split('off')
        eng.set_formulation('alpha')
        eng.set_fused_projection(0)
        eng.debug_score_probe(True)
        eng.set_alpha(prob.alpha)
        eng.set_beliefs(prob.b)
        st = eng.run(1.0)
        res = eng.fetch()
        p = eng.debug_score_probe_fetch()
    finally:
        eng.close()
    queued, count = host_candidates(p)
    return prob, st, p, res, queued, count


def edge_lines(V=64):
    """The two edge runs as digest lines (this process and the child print the same)."""
    _, _, p0, _, _, _ = run_edge(V, 2.0 ** -10)               # far outside: E alone is wanted (m = mag = 1.5 in every run)
    E = float(p0['E'][0, 0])
    u = 2.0 ** -23                                           # fp32 spacing in [1, 2)
    j = int(np.floor(2.0 * E / u))
    assert 8 <= j < 2 ** 12 and j * u <= 2.0 * E < (j + 1) * u
    lines = []
    for name, gap, want in (('edge_in', j * u, 3), ('edge_out', (j + 1) * u, 2)):
        prob, st, p, res, queued, count = run_edge(V, gap)
        assert np.all(p['E'] == E) and np.all(p['best_score'] == 1.5)
        assert np.all(p['score'][:, :, prob.q] == 1.5 - gap)                     # exact: the score is where it was put
        assert queued.all() and np.all(count == want), (name, count)             # the rule on the host
        assert st['n_refine_candidates'] == want * queued.sum(), (name, st)      # ... and what the refinement took
        assert np.all(res.best_alpha_ind == prob.p)
        lines.append(f'handover-sha256 {name} {int(st["n_refined"])} {int(st["n_refine_candidates"])} '
                     f'{res.best_alpha_ind.ravel().tolist()}')
    return lines


@gpu
def test_candidate_at_the_windows_edge():
    mine = edge_lines()
    theirs = child_lines('edge')
    assert [theirs.get(ln.split()[1]) for ln in mine] == mine, (mine, theirs)


# --------------------------------------------------------------------------- #
# 3. the queue as a set
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize('B,A,O', [(3, 2, 2), (4, 2, 2), (BLOCK_ROWS + 1, 1, 1), (BLOCK_ROWS - 1, 1, 1), (8 * BLOCK_ROWS + 3, 1, 3)])
@pytest.mark.parametrize('what', ['all', 'none', 'some'])
def test_block_appends_keep_the_queue_a_set(B, A, O, what):
    """B * G = 12, 16, 17, 15, 393 rows against blocks of 16: every row queued, none, and those of the beliefs without
    mass on state 0 (identity successors: the second copy is 4 lower there)."""
    assert (B * A * O - BLOCK_ROWS) in (-4, 0, 1, -1, 377)
    prob = tie_problem(S=33, V=72 if A == 2 else 70, B=B, k=1 if what == 'none' else 2, A=A, O=O, identity=True)   # (4-column and scalar reader)
    alpha, b = prob.alpha.copy(), prob.b.copy()
    if what == 'some':
        alpha[prob.positions[-1], 0] -= 4.0
        b[::2, 1] += b[::2, 0]
        b[::2, 0] = 0.0
    eng = prob.engine('f32')
    try:
        eng.set_formulation('alpha')
        eng.debug_score_probe(True)
        eng.set_alpha(alpha)
        eng.set_beliefs(b)
        st = eng.run(GAMMA)
        p = eng.debug_score_probe_fetch()
    finally:
        eng.close()
    queued, count = host_candidates(p)
    queue = np.sort(p['queue'].astype(np.int64))
    assert len(queue) == p['qcount'] == st['n_refined']
    assert np.array_equal(queue, np.flatnonzero(queued.ravel()))
    n = int(queued.sum())
    has0 = b[p['perm'].astype(np.int64), 0] > 0
    if what == 'some':
        assert np.array_equal(queued, np.repeat(~has0[:, None], A * O, axis=1)) and 0 < n < B * A * O
    else:
        assert n == (B * A * O if what == 'all' else 0)
    assert st['n_refine_candidates'] == int(count[queued].sum()) == 2 * n


# --------------------------------------------------------------------------- #
# 4. order independence
# --------------------------------------------------------------------------- #
@gpu
def test_stale_candidate_lists_do_not_leak():
    """plain -> tied (8 copies) -> tied (3 copies, other columns) -> plain through one engine: each call equals a fresh
    engine's call on the same inputs (test_gpu_parity.py::test_speculative_refinement_recovers_when_ties_appear's order)."""
    kw = dict(S=330, V=700, B=40)
    plain, tied8, tied3 = (tie_problem(k=k, **kw) for k in (1, 8, 3))
    assert tied3.positions != tied8.positions[:3] and np.array_equal(plain.b, tied8.b)

    def call(eng, prob):
        eng.set_alpha(prob.alpha)
        st = eng.run(GAMMA)
        res = eng.fetch()
        return (res.best_alpha_ind.copy(), res.actions.copy(), np.asarray(res.alpha).tobytes(),
                int(st['n_refined']), int(st['n_refine_candidates']), int(st['n_refined_actions']))

    def engine():
        eng = plain.engine('f32')
        eng.set_formulation('alpha')
        eng.set_beliefs(plain.b)
        return eng

    one = engine()
    try:
        for i, prob in enumerate((plain, tied8, tied3, plain)):
            got = call(one, prob)
            fresh = engine()
            try:
                want = call(fresh, prob)
            finally:
                fresh.close()
            for g, w in zip(got, want):
                assert np.array_equal(g, w) if isinstance(g, np.ndarray) else g == w, (i, g, w)
            assert np.array_equal(got[0], prob.ref['best']) and got[4] == prob.k * got[3] * (prob.k > 1), i
    finally:
        one.close()
