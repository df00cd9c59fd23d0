"""The two byte masks of a backup against exact references: no tolerances.

``keep``  (K5, ``k_keep``; src/pomdp.py:1510-1512) is ``b.alpha'[b] > max_v b.alpha_v``.  On the inputs of
``mask_cases.keep_case`` the margin is exactly +-2^-(23+j) (j = 1 .. 10) or 0 at magnitudes of 1.5: 2^-24 .. 2^-34 of the
magnitude, below what an fp32 GEMM resolves, while float64 arithmetic on them is exact in any order.  An engine that
compared against fp32 maxima, or wrote the mask through the wrong permutation, gets a different mask.

The dead-triple map (``k_dead``) is ``supp(b) n supp(RTO[:, a, o, :]) = {}``.  ``mask_cases.DEAD_CASES`` place beliefs
and supports tile by tile so that each case walks one named branch of the kernel; the probe's map, ``stats['n_dead']``,
``q_values``' best rows and the backup's results are compared with the definition and with ``orc.backup_core``.
"""
import functools

import numpy as np
import pytest

import mask_cases as mc
from model_cases import assert_backup_matches_oracle
from oracle import pbvi_oracle as orc
from test_score_window import host_window

# --------------------------------------------------------------------------- #
# CPU: the keep builder
# --------------------------------------------------------------------------- #
KEEP_B = (40, 300)
KEEP_V = (48, 80)
SCALES = (1.0, 2.0 ** 20, 2.0 ** -20)
# |best - runner-up| of every alpha and action decision of a keep case, over the widest fp32 tie window (split GEMM, belief
# side, one chain over all of S) times the decision's magnitude.  By construction the alpha gap is >= 1/4 against a magnitude of
# about 1 and the action gap is 1 against about 2; test_keep_case_decisions_are_no_near_ties found 1318x .. 2374x (alpha
# rows) and 2005x .. 3362x (actions) and holds both above this factor.
CLEARANCE = 1000.0


def f32_exact(x):
    return np.array_equal(np.asarray(x, np.float64).astype(np.float32).astype(np.float64), x)


def keep_quantities(case, dtype):
    """(rows, actions, best, nv, old, keep) of the backup and K5 from the oracle's statements, in ``dtype``."""
    al, b, rto, er = (x.astype(dtype) for x in (case.alpha, case.b, case.rto, case.er))
    rows, act, best = orc.backup_core(al, b, case.rs, rto, er, dtype(case.gamma))
    nv = np.sum(b * rows, axis=1)
    old = np.max(np.matmul(b, al.T), axis=1)
    return rows, act, best, nv, old, orc.belief_dominance_mask(al, b, rows)


@pytest.mark.parametrize('B,V,scale', [(40, 48, s) for s in SCALES] + [(40, 80, s) for s in SCALES] +
                         [(300, 48, 1.0), (300, 80, 2.0 ** 20), (300, 80, 2.0 ** -20)])
def test_keep_case_is_exact(B, V, scale):
    """The exactness claim: float64 == long double bit for bit for the backup, nv and old; the margin is the stated one;
    and, independently of any floating-point format, the same margin in integer arithmetic."""
    case = mc.keep_case(B, V, scale)
    r64, a64, v64, nv64, old64, keep64 = keep_quantities(case, np.float64)
    rld, ald, vld, nvld, oldld, keepld = keep_quantities(case, np.longdouble)
    assert rld.dtype == np.longdouble and nvld.dtype == np.longdouble
    for x64, xld in ((r64, rld), (nv64, nvld), (old64, oldld)):
        assert np.array_equal(x64.astype(np.longdouble), xld)
    assert np.array_equal(a64, ald) and np.array_equal(v64, vld) and np.array_equal(keep64, keepld)
    assert np.array_equal(nv64 - old64, case.margin) and np.array_equal(keep64, case.margin > 0)
    assert np.array_equal(keep64, case.mask)
    assert np.array_equal(r64, case.rows) and np.array_equal(a64, case.actions) and np.array_equal(v64, case.best)
    # integers: b in units of 2^-10, rows and alpha in units of scale 2^-23
    bi = np.rint(case.b * 1024.0).astype(np.int64)
    ri = np.rint(case.rows / scale * 2.0 ** 23).astype(np.int64)
    ai = np.rint(case.alpha / scale * 2.0 ** 23).astype(np.int64)
    assert np.array_equal(bi / 1024.0, case.b) and np.array_equal(ri * scale * 2.0 ** -23, case.rows)
    assert np.array_equal(ai * scale * 2.0 ** -23, case.alpha)
    margin_i = (bi * ri).sum(axis=1) - (bi @ ai.T).max(axis=1)
    assert np.array_equal(margin_i, case.sgn * 2 ** (10 - case.j))                    # units of 2^-33: sgn 2^-(23+j)
    # old itself is no fp32 number (an engine that rounds its maxima to fp32 on the way to K5 gets another mask) ...
    old32 = old64.astype(np.float32).astype(np.float64)
    assert np.all((old32 != old64)[case.j >= 2]) and (nv64 > old32)[case.j >= 2].tolist() != case.mask[case.j >= 2].tolist()
    assert ((nv64 > old32) != case.mask).sum() >= B // 8
    # ... while an fp32 engine holds every input, and every row it has to return, exactly
    assert all(f32_exact(x) for x in (case.alpha, case.b, case.er, case.rto, case.rows))


@pytest.mark.parametrize('B', KEEP_B)
@pytest.mark.parametrize('V', KEEP_V)
def test_keep_case_ladder_and_order(B, V):
    case = mc.keep_case(B, V)
    rungs = {(int(j), int(s)) for j, s in zip(case.j, case.sgn)}
    assert rungs == {(j, s) for j in mc.LADDER for s in (1, -1, 0)}                   # every rung with +, - and 0
    assert np.array_equal(np.abs(case.margin), np.abs(case.sgn) * 2.0 ** -(23.0 + case.j))
    assert np.all(case.b.sum(axis=1) == 1.0) and np.all(case.b[np.arange(B), case.s0] == 2.0 ** -case.j.astype(float))
    nz = case.b != 0
    assert np.all(nz.sum(axis=1) >= 2)
    assert np.array_equal(np.argmax(nz, axis=1) // mc.TILE, case.block_of)            # one block each, pairwise disjoint
    assert np.array_equal(np.sort(case.block_of), np.arange(B)) and np.all(nz.sum(axis=0) <= 1)
    rows_nz, states_nz = np.nonzero(nz)
    assert np.array_equal(states_nz // mc.TILE, case.block_of[rows_nz])
    m = case.mask.astype(int)
    assert (np.diff(m) != 0).sum() >= B // 8                                         # not monotone
    if B > 256:
        assert not np.array_equal(m[256:], m[:B - 256])                              # not periodic with the row tile
    # the engine sorts a block of more than one row tile by first non-zero K tile: a mask written or read through the
    # wrong side of that permutation is another mask
    perm = case.sort_perm()
    assert np.array_equal(perm, mc.first_tile_perm(case.b)) and not np.array_equal(perm, np.arange(B))
    inv = np.argsort(perm)
    assert not np.array_equal(case.mask[perm], case.mask) and not np.array_equal(case.mask[inv], case.mask)
    assert (case.mask[perm] != case.mask).sum() >= B // 8 and (case.mask[inv] != case.mask).sum() >= B // 8


@pytest.mark.parametrize('B', KEEP_B)
@pytest.mark.parametrize('V', KEEP_V)
def test_keep_case_decisions_are_no_near_ties(B, V):
    """No best-alpha or action decision of a keep case is near a tie: the margin over (2 x the widest fp32 window x the
    magnitude) is printed and must exceed CLEARANCE."""
    case = mc.keep_case(B, V)
    w = host_window({'tol_rel': -1.0, 'chain_steps': case.S // mc.TILE, 'split': 1, 'push': 1})
    sc = case.gamma * case.b @ case.alpha.T                                           # [B][V]: O = 1, both actions alike
    top = np.sort(sc, axis=1)
    mag = case.gamma * np.abs(case.b) @ np.abs(case.alpha).max(axis=0)
    clear_v = ((top[:, -1] - top[:, -2]) / (2.0 * w * mag)).min()
    assert np.array_equal(np.argmax(sc, axis=1), case.winner)
    val = case.b @ case.er + top[:, -1:]                                              # [B][A]
    mag_a = np.abs(case.b) @ np.abs(case.er) + mag[:, None]
    clear_a = ((val[:, 0] - val[:, 1]) / (2.0 * w * mag_a.max(axis=1))).min()
    print(f'\n[keep-case] B={B} V={V}: window {w:.3e}, clearance alpha {clear_v:.0f}x, action {clear_a:.0f}x')
    assert clear_v > CLEARANCE and clear_a > CLEARANCE


# --------------------------------------------------------------------------- #
# CPU: the dead-map builder
# --------------------------------------------------------------------------- #
def all_dead_cases():
    return list(mc.DEAD_CASES) + ['sorted_block', 'second_w0_iteration']


def dead_case(name):
    if name == 'sorted_block':
        return mc.sorted_dead_case()
    if name == 'second_w0_iteration':
        return mc.big_dead_case()
    return mc.DEAD_CASES[name]


@functools.lru_cache(maxsize=None)
def dead_oracle(name):
    c = dead_case(name)
    return orc.backup_core(c.alpha, c.b, c.rs, c.rto, c.er, c.gamma)


def test_dead_ref_on_hand_written_rows():
    rto = np.zeros((4, 1, 2, 2))
    rto[1, 0, 0, 1] = 0.25                                   # g0: state 1 (through slot 1)
    rto[3, 0, 1, 0] = 2.0 ** -160                            # g1: state 3, a value fp32 cannot hold
    b = np.array([[0.0, 0.5, 0.0, 0.0], [0.5, 0.0, 0.5, 0.0], [0.0, 0.0, 0.0, 1e-300], [0.0, 0.0, 0.0, 0.0]])
    assert mc.dead_ref(b, rto).tolist() == [[False, True], [True, True], [True, False], [True, True]]
    n_cand, first, tile = mc.tile_structure(b, rto)
    assert n_cand.tolist() == [[1, 1], [1, 1], [1, 1], [0, 0]] and first.tolist() == [[0, -1], [-1, -1], [-1, 0], [-1, -1]]


@pytest.mark.parametrize('name', all_dead_cases())
def test_dead_case_structure(name):
    """Each case is what its name says: the candidate tiles of the named (belief, group) pairs and the position of the
    first one that holds a common state, counted in NumPy."""
    c = dead_case(name)
    n_cand, first, tile = mc.tile_structure(c.b, c.rto)
    assert np.array_equal(first < 0, c.dead) and np.array_equal(c.dead, mc.dead_ref(c.b, c.rto))
    assert c.claims or name == 'sorted_block'
    for i, g, n, pos, t in c.claims:
        assert (int(n_cand[i, g]), int(first[i, g]), int(tile[i, g])) == (n, pos, t), (name, i, g)
    assert c.dead.any() and not c.dead.all()
    # the branch that the name promises, for (belief 0, group 1) -- the triple whose only overlap is the planted one
    pos, t, n = int(first[0, 1]), int(tile[0, 1]), int(n_cand[0, 1])
    if name.startswith('disjoint_'):
        want = int(name.split('_')[1])
        assert int(n_cand[0, 0]) == want and c.dead[0, 0] and (n, pos) == (want, want - 1)
    if name in ('t1_second_of_pair', 't1_second_pair', 'last_of_word'):
        assert pos % 2 == 1                                  # the second tile of a pair: lanes 32-63
    if name == 'odd_last_candidate':
        assert n % 2 == 1 and pos == n - 1                   # t1 = -1 beside it
    if name == 'last_of_word':
        assert t % mc.WORD == 63 and t // mc.WORD == 0 and n == pos + 2      # ... and one more candidate, in word 1
    if name.startswith('bit_') or name.startswith('word1_bit_'):
        assert t % mc.WORD == int(name.rsplit('_', 1)[1]) and t // mc.WORD == int(name.startswith('word1'))
    if name.startswith('kt'):
        kt, w = (int(x) for x in name[2:].split('_word'))
        assert c.k_tiles == kt and t // mc.WORD == w and c.S % mc.TILE != 0
    if name.startswith('last_state'):
        rem = int(name.rsplit('rem', 1)[1])
        assert c.S % mc.TILE == rem and c.R == 2
        for i, g in ((0, 0), (3, 3)):                        # the only common state is S - 1
            common = np.flatnonzero((c.b[i] != 0) & (c.rto[:, 0, g, :] != 0).any(axis=1))
            assert common.tolist() == [c.S - 1]
        assert np.all(c.rto[:, :, :, 1] == 0) and np.all(c.rs[:, :, 1] == 2) and c.b[0, 2] != 0     # the pad slot points into supp(b0)
    if name == 'second_w0_iteration':
        assert c.S == 131072 + 64 + 5 and c.k_tiles > 4096 and (c.k_tiles + 63) // 64 == 65
        assert int(tile[0, 0]) // mc.WORD == 64 and int(tile[1, 1]) // mc.WORD == 64 and int(tile[1, 1]) * mc.TILE + 4 == c.S - 1
        assert int(n_cand[2].min()) == 3 and c.dead[2].all()   # candidates in words 0 .. 63 only, no common state
    if name == 'sorted_block':
        perm = mc.first_tile_perm(c.b)
        assert c.B == 300 and not np.array_equal(c.dead[perm], c.dead) and not np.array_equal(c.dead[np.argsort(perm)], c.dead)
        assert (c.dead[perm] != c.dead).any(axis=1).sum() >= c.B // 8
        elem_only = c.dead & (n_cand > 0)                    # candidates, no common state
        assert elem_only.sum() >= c.B // 8 and (~c.dead).sum() >= c.B // 2
    # the alpha set: on every live triple the reference's first argmax is a row other than 0
    want_v = dead_oracle(name)[2].reshape(c.B, -1)
    assert np.all(want_v[~c.dead] != 0) and np.all(want_v[c.dead] == 0)
    assert all(f32_exact(x) for x in (c.alpha, c.b, c.er, c.rto))


def test_tiny_case_structure():
    c = mc.TinyCase()
    assert c.dead.tolist() == [[False, False, True], [False, True, False], [False, True, True]]
    f32 = lambda x: x.astype(np.float32).astype(np.float64)
    d32 = mc.dead_ref(f32(c.b), f32(c.rto))
    for i, g in c.tiny_triples:                              # live in fp64, gone in the fp32 copy
        assert not c.dead[i, g] and d32[i, g]
    _, _, want_v = orc.backup_core(c.alpha, c.b, c.rs, c.rto, c.er, c.gamma)
    sc = np.einsum('bs,aovs->baov', c.b, orc.gamma_projection(c.alpha, c.rs, c.rto, c.gamma)).reshape(c.B, c.O, c.V)
    for i, g in c.tiny_triples:
        top = np.sort(sc[i, g])
        mag = c.gamma * np.abs(c.b[i]) @ (np.abs(c.rto[:, 0, g, 0]) * np.abs(c.alpha).max(axis=0))
        assert want_v[i, 0, g] == c.V - 1 and top[-1] > 0
        assert top[-1] - top[-2] > 1e6 * (c.S * c.R + 2.0) * 2.0 ** -53 * mag       # far outside the fp64 rounding bound


# --------------------------------------------------------------------------- #
# GPU: keep
# --------------------------------------------------------------------------- #
def make_engine(case, dtype):
    from pomdp_pbvi_exploration_amd.engine import Engine
    return Engine(case.S, case.A, case.O, case.R, case.rs, case.rto, case.er, dtype=dtype)


KEEP_VARIANTS = ('alpha', 'belief', 'tiled', 'run_fetch', 'repeat')
# engine modes: fp32 with the value-max setting on and off, fp64 behind the forced screen and pure
KEEP_MODES = {'f32': ('f32', True, None), 'f32_vmax_fast': ('f32', False, None),
              'f64_screen': ('f64', True, 'always'), 'f64_pure': ('f64', True, 'off')}


def check_keep_result(case, dtype, alpha_new, actions, best, keep, tag):
    T = np.float32 if dtype == 'f32' else np.float64
    assert alpha_new.dtype == T, tag
    got = np.asarray(keep).astype(bool)
    wrong = np.flatnonzero(got != case.mask)
    assert wrong.size == 0, (tag, 'keep differs at', wrong[:10].tolist(), 'margins', case.margin[wrong[:10]].tolist())
    assert np.array_equal(np.asarray(best, dtype=np.int64), case.best), tag
    assert np.array_equal(np.asarray(actions, dtype=np.int64), case.actions), tag
    assert np.array_equal(alpha_new, case.rows.astype(T)), tag                       # representable: bit for bit


def run_keep_case(B, V, mode, variant, scale=1.0):
    from pomdp_pbvi_exploration_amd.engine import PinnedBuffer
    dtype, vmax_exact, screen = KEEP_MODES[mode]
    case = mc.keep_case(B, V, scale)
    tag = f'keep B={B} V={V} {mode} {variant} scale={scale}'
    eng = make_engine(case, dtype)
    pin = rows = None
    try:
        if dtype == 'f32':
            eng.set_score_split('off')
        else:
            eng.set_f64_screen(screen)
        eng.set_formulation('belief' if variant == 'belief' else 'alpha')
        if variant == 'tiled':
            eng.set_fused_projection(False)
            eng.set_gamma_tiling('always', mc.keep_chunk_rows(V))
        if not vmax_exact:
            eng.set_value_max_exact(False)
        if variant == 'run_fetch':
            T = eng.np_dtype
            pin = PinnedBuffer(B * case.S * np.dtype(T).itemsize + 4096)
            rows = pin.carve((B, case.S), T)
            slot, index, act = (np.full(B, -1, dtype=np.int32) for _ in range(3))
            best, keep = np.full((B, case.A, case.O), -1, dtype=np.int32), np.full(B, 7, dtype=np.uint8)
            eng.set_alpha(case.alpha)
            eng.set_beliefs(case.b)
            stats, U, _ = eng.run_fetch_into(case.gamma, rows, slot, index, act, best=best, keep=keep, belief_dominance_prune=True)
            assert set(np.unique(keep).tolist()) <= {0, 1}, tag
            check_keep_result(case, dtype, rows[slot[index]], act, best, keep, tag)
        else:
            res = eng.backup_full(case.alpha, case.b, case.gamma, belief_dominance_prune=True)
            stats = res.stats
            check_keep_result(case, dtype, res.alpha, res.actions, res.best_alpha_ind, res.keep, tag)
        route = eng.debug_value_max_route()
        assert route['calls'] >= 1 and route['rows'] == B and route['alpha_rows'] == V, (tag, route)
        if dtype == 'f32':                                   # either side of vmax_skinny's 64 rows; never the un-rescored GEMM
            assert route['route'] == ('f32_skinny' if V <= 64 else 'f32_wide_exact'), (tag, route)
        else:
            assert route['route'] in ('f64_mfma', 'f64_plain'), (tag, route)
            assert stats['screened'] == int(screen == 'always'), (tag, stats)
        # (engine.hip, choose_push: pure fp64 scoring projects beliefs only where its MFMA GEMM runs, B A O V >= 64 x 64)
        push = variant == 'belief' and (mode != 'f64_pure' or B * case.A * case.O * V >= 64 * 64)
        assert stats['formulation'] == (2 if push else 1), (tag, stats)
        if variant == 'tiled':
            assert stats['gamma_chunks'] == 3, (tag, stats)
        if variant == 'repeat':                              # the same block again: cached tile lists, dead map and sort order
            stats2 = eng.run(case.gamma, belief_dominance_prune=True)
            res2 = eng.fetch()
            check_keep_result(case, dtype, res2.alpha, res2.actions, res2.best_alpha_ind, res2.keep, tag + ' (second backup)')
            assert stats2['n_dead'] == stats['n_dead'] == 0, (tag, stats2)
        if not vmax_exact:                                   # the setting still holds for the call it is documented for
            val, _ = eng.max_value_resident()
            assert eng.debug_value_max_route()['route'] == ('f32_skinny' if V <= 64 else 'f32_wide_fast'), tag
            old = (case.b @ case.alpha.T).max(axis=1)
            assert np.all(np.abs(val - old) <= 1e-5 * np.abs(old)), tag
    finally:
        eng.close()
        if pin is not None:
            rows = None                                      # (the buffer refuses to close under a carved array)
            pin.close()


@pytest.mark.gpu
@pytest.mark.parametrize('variant', KEEP_VARIANTS)
@pytest.mark.parametrize('mode', list(KEEP_MODES))
@pytest.mark.parametrize('V', KEEP_V)
@pytest.mark.parametrize('B', KEEP_B)
def test_keep_is_the_exact_mask(B, V, mode, variant):
    """keep, rows, actions and indices of a belief-dominance backup whose margins are +-2^-(23+j) or 0: every belief, no
    exceptions -- on fp32 engines also after ``set_value_max_exact(False)``, which is a setting of ``max_value`` alone."""
    run_keep_case(B, V, mode, variant)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', list(KEEP_MODES))
@pytest.mark.parametrize('V', KEEP_V)
@pytest.mark.parametrize('scale', SCALES[1:])
def test_keep_under_dynamic_range(scale, V, mode):
    """The alpha set and er times 2^20 and 2^-20: the same masks."""
    assert np.array_equal(mc.keep_case(300, V, scale).mask, mc.keep_case(300, V).mask)
    run_keep_case(300, V, mode, 'alpha', scale)


# --------------------------------------------------------------------------- #
# GPU: the dead-triple map
# --------------------------------------------------------------------------- #
DEAD_MODES = {'f32': ('f32', None), 'f64_screen': ('f64', 'always'), 'f64_pure': ('f64', 'off')}


def probe_dead(eng, B, G):
    p = eng.debug_score_probe_fetch()
    perm = p['perm'].astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(B))
    dead = np.zeros((B, G), dtype=bool)
    dead[perm] = p['dead'].astype(bool)                      # engine order -> caller order
    return dead, perm


def run_dead_case(c, name, mode, want):
    dtype, screen = DEAD_MODES[mode]
    want_rows, want_a, want_v = want
    G = c.A * c.O
    tag = f'dead {name} {mode}'
    pure = mode == 'f64_pure'
    dead_want = np.zeros_like(c.dead) if pure else c.dead    # pure fp64 scoring keeps no map: every triple is scored
    eng = make_engine(c, dtype)
    try:
        if dtype == 'f64':
            eng.set_f64_screen(screen)
        eng.debug_score_probe(True)
        res = eng.backup_full(c.alpha, c.b, c.gamma)
        dead, perm = probe_dead(eng, c.B, G)
        if dtype == 'f64':
            assert res.stats['screened'] == int(screen == 'always'), (tag, res.stats)
        assert np.array_equal(perm, mc.first_tile_perm(c.b) if c.B > (256 if dtype == 'f32' else 128) else np.arange(c.B)), tag
        wrong = np.argwhere(dead != dead_want)
        assert wrong.size == 0, (tag, 'dead map differs at (belief, group)', wrong[:10].tolist())
        assert res.stats['n_dead'] == int(dead_want.sum()), (tag, res.stats['n_dead'], int(dead_want.sum()))
        assert_backup_matches_oracle(res, c.alpha, want_rows, want_a, want_v, dtype, tag)
        assert np.array_equal(res.best_alpha_ind, want_v), tag                       # (exact inputs: no duplicate-row leeway needed)
        # the same block again: the cached map and count
        stats2 = eng.run(c.gamma)
        res2 = eng.fetch()
        dead2, _ = probe_dead(eng, c.B, G)
        assert np.array_equal(dead2, dead_want) and stats2['n_dead'] == int(dead_want.sum()), (tag, stats2['n_dead'])
        assert np.array_equal(res2.best_alpha_ind, want_v) and np.array_equal(res2.actions, want_a), tag
        eng.debug_score_probe(False)
        q, act, best = eng.q_values_resident(c.gamma, want_best=True)
        best = best.reshape(c.B, G)
        assert np.all(best[c.dead] == 0), tag
        assert np.array_equal(best[~c.dead], want_v.reshape(c.B, G)[~c.dead]), tag
        assert np.array_equal(act, want_a), tag
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('mode', list(DEAD_MODES))
@pytest.mark.parametrize('name', all_dead_cases())
def test_dead_map_is_its_definition(name, mode):
    """The probe's dead map, ``n_dead`` (first backup and repeat), ``q_values``' best rows and the backup itself on one
    hand-built case (``mask_cases``: the case's ``branch`` names the part of ``k_dead`` it walks).  A pure-fp64 engine keeps
    no map, reports none and still matches the oracle."""
    c = dead_case(name)
    run_dead_case(c, name, mode, dead_oracle(name))


@pytest.mark.gpu
def test_screened_f64_keeps_triples_that_fp32_cannot_see():
    """Belief or RTO entries of 2^-160: the triple is live in fp64 while its fp32 copy is all zero.  Behind the screen
    ``k_dead`` runs on the fp64 engine's own operands -- ``blk_.rows`` (the caller's fp64 beliefs) and ``view()``, whose
    support bytes and tile words were built from the fp64 RTO when the engine was created (engine.hip,
    ``side_stream_work``: "from the supports of the ORIGINAL operands") -- never on the screen's fp32 copies.  So the triple
    is live, its all-zero fp32 scores tie inside a zero window, and the fp64 refinement decides it."""
    c = mc.TinyCase()
    want_rows, want_a, want_v = orc.backup_core(c.alpha, c.b, c.rs, c.rto, c.er, c.gamma)
    eng = make_engine(c, 'f64')
    try:
        eng.set_f64_screen('always')
        eng.debug_score_probe(True)
        res = eng.backup_full(c.alpha, c.b, c.gamma)
        dead, _ = probe_dead(eng, c.B, c.A * c.O)
        assert res.stats['screened'] == 1, res.stats
        assert np.array_equal(dead, c.dead), dead.tolist()
        assert res.stats['n_dead'] == int(c.dead.sum()) == 4, res.stats['n_dead']
        for i, g in c.tiny_triples:
            assert res.best_alpha_ind[i, 0, g] == want_v[i, 0, g] == c.V - 1, (i, g, res.best_alpha_ind[i, 0].tolist())
        assert_backup_matches_oracle(res, c.alpha, want_rows, want_a, want_v, 'f64', 'tiny')
        assert np.array_equal(res.best_alpha_ind, want_v)
        stats2 = eng.run(c.gamma)
        assert stats2['n_dead'] == 4 and np.array_equal(eng.fetch().best_alpha_ind, want_v)
    finally:
        eng.close()
