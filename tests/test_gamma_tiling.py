"""Gamma tiled over the alpha set (``pbvi_set_gamma_tiling``): the alpha-side score stage walks the alpha set in chunks
through one chunk-sized Gamma buffer and folds each chunk's partial slabs into a full-width score matrix
(``k_fold_chunk``); argmax, refinement and the later stages run once on that matrix.  Compared against the reference's
fixtures and against the untiled engine (mode ``'off'``) of the same build -- never tiled against tiled.  Bars as in
test_gpu_parity.py: indices and actions exact, alpha' within 1e-6 (fp32 engines) / 1e-12 (fp64 engines) relative."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_npz
from oracle import pbvi_oracle as orc
from pomdp_pbvi_exploration_amd import synth
from pomdp_pbvi_exploration_amd.engine import Engine

pytestmark = pytest.mark.gpu

F32_RTOL = 1e-6
F64_RTOL = 1e-12
# the suite is also run with PBVI_FORMULATION=belief: tiling is then a no-op that reports 0 chunks
BELIEF_ENV = os.environ.get('PBVI_FORMULATION', '') in ('belief', '2')


def assert_alpha_close(x, ref, rtol):
    x = np.asarray(x, dtype=np.float64)
    np.testing.assert_allclose(x, ref, rtol=rtol, atol=rtol * max(1e-300, float(np.max(np.abs(ref)))) * 1e-3)


def small(R):
    z = load_npz(f'olfactory_small_R{R}.npz')
    return z, z['reachable_states'].astype(np.int64), z['rto'].astype(np.float64), z['expected_rewards'].astype(np.float64)


def alpha_side(eng):
    if not BELIEF_ENV:
        eng.set_formulation('alpha')


def check_path(stats, chunks):
    """Every call: the alpha side ran, with the expected number of Gamma chunks."""
    if BELIEF_ENV:
        assert stats['formulation'] == 2 and stats['gamma_chunks'] == 0, stats
    else:
        assert stats['formulation'] == 1 and stats['gamma_chunks'] == chunks, stats


def configure(eng, config):
    if config == 'f32_fp32gemm':
        eng.set_score_split('off')
    elif config == 'f32_split':
        eng.set_score_split('always')
    elif config == 'f64_screen':
        eng.set_f64_screen('always')
    elif config == 'f64_pure':
        eng.set_f64_screen('off')


CONFIGS = ['f32_fp32gemm', 'f32_split', 'f64_screen', 'f64_pure']


@pytest.mark.parametrize('config', CONFIGS)
@pytest.mark.parametrize('R', [5, 1])
def test_reference_fixtures_with_forced_tiling(R, config):
    """The S = 600 olfactory fixtures (R = 5; R = 1 with the fused projection off) in 3 chunks of 20, 20 and 8 alpha rows,
    then with one chunk: the fixture's indices and actions, rows within the bar; one chunk is the untiled path."""
    z, rs, rto, er = small(R)
    S, A, Rr = rs.shape
    dtype = config[:3]
    rtol = F32_RTOL if dtype == 'f32' else F64_RTOL
    gamma = float(z['gamma'])
    V = z['alpha'].shape[0]
    assert V == 48
    eng = Engine(S, A, rto.shape[2], Rr, rs, rto, er, dtype=dtype)
    configure(eng, config)
    alpha_side(eng)
    if R == 1:
        eng.set_fused_projection(False)
    assert eng.gamma_tiling == ('off', 0) or os.environ.get('PBVI_GAMMA_TILING')
    eng.set_gamma_tiling('off')
    plain = eng.backup_full(z['alpha'], z['beliefs'], gamma, belief_dominance_prune=True)
    check_path(plain.stats, 1)
    for rows, chunks in ((20, 3), (48, 1), (1000, 1)):
        eng.set_gamma_tiling('always', rows)
        assert eng.gamma_tiling == ('always', rows)
        res = eng.backup_full(z['alpha'], z['beliefs'], gamma, belief_dominance_prune=True)
        check_path(res.stats, chunks)
        assert np.array_equal(res.best_alpha_ind, z['core_best']), int(np.sum(res.best_alpha_ind != z['core_best']))
        assert np.array_equal(res.actions, z['core_actions'])
        assert_alpha_close(res.alpha, z['core_alpha'], rtol)
        if dtype == 'f64':
            assert np.array_equal(res.keep, z['core_keep'])
        assert np.array_equal(res.keep, plain.keep)
        if config == 'f32_split' and not BELIEF_ENV:
            assert res.stats['score_split'] == plain.stats['score_split'] == 1
        if dtype == 'f32':
            assert np.array_equal(res.alpha, plain.alpha) and np.array_equal(res.best_alpha_ind, plain.best_alpha_ind)
    eng.close()


def random_model(rng, S, A, O, R):
    rs = rng.integers(0, S, size=(S, A, R))
    p = rng.random((S, A, R))
    p[rng.random((S, A, R)) < 0.3] = 0.0
    p[:, :, 0] += 1e-3
    p /= p.sum(axis=2, keepdims=True)
    obs = rng.random((S, A, O))
    obs[rng.random((S, A, O)) < 0.3] = 0.0
    obs[:, :, 0] += 1e-3
    obs /= obs.sum(axis=2, keepdims=True)
    rto = p[:, :, None, :] * obs[rs[:, :, None, :], np.arange(A)[None, :, None, None], np.arange(O)[None, None, :, None]]
    er = rng.normal(size=(S, A))
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    return rs, r32(rto), r32(er)


def seam_inputs():
    """The near-tie alpha set of test_adversarial_near_ties (rows that differ by 1e-5 ... 1e-9 relative) at V = 253 -- not a
    multiple of 4 -- with exact twins that fall into DIFFERENT chunks for chunk sizes 4, 100 and 252."""
    rng = np.random.default_rng(42)
    S, A, O, R, V, B = 2000, 2, 2, 2, 253, 320
    rs, rto, er = random_model(rng, S, A, O, R)
    base = rng.random(S) * 10.0 + 1.0
    alpha = np.empty((V, S))
    for v in range(V):
        eps = 10.0 ** -(5 + (v % 5))
        alpha[v] = base * (1.0 + eps * rng.standard_normal(S))
    for twin, first in ((7, 3), (130, 3), (252, 101), (99, 98), (100, 98), (205, 2)):
        alpha[twin] = alpha[first]
    alpha = alpha.astype(np.float32).astype(np.float64)
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.05)
    b[:, 0] += 1e-3
    b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    return S, A, O, R, rs, rto, er, alpha, b, 0.95


@pytest.mark.parametrize('rows', [4, 100, 252])
@pytest.mark.parametrize('config', ['f32_fp32gemm', 'f32_split', 'f64_screen'])
def test_same_decisions_as_the_untiled_engine_across_chunk_seams(config, rows):
    """Exact twins in different chunks (the lower global index must win, as np.argmax), near-ties everywhere, a ragged last
    chunk, the belief-dominance test: fp32 engines give the untiled engine's bits, and both give the oracle's indices."""
    S, A, O, R, rs, rto, er, alpha, b, gamma = seam_inputs()
    V = alpha.shape[0]
    dtype = config[:3]
    want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, gamma)
    for twin in (7, 130, 252, 99, 100, 205):
        assert not np.any(want_v == twin)                     # the reference picks the first of tied rows
    eng = Engine(S, A, O, R, rs, rto, er, dtype=dtype)
    configure(eng, config)
    alpha_side(eng)
    eng.set_gamma_tiling('off')
    plain = eng.backup_full(alpha, b, gamma, belief_dominance_prune=True)
    check_path(plain.stats, 1)
    eng.set_gamma_tiling('always', rows)
    for _ in range(2):                                        # twice: the second call re-uses every chunk buffer
        res = eng.backup_full(alpha, b, gamma, belief_dominance_prune=True)
        check_path(res.stats, -(-V // rows))
        assert np.array_equal(res.best_alpha_ind, want_v), int(np.sum(res.best_alpha_ind != want_v))
        assert np.array_equal(res.actions, want_a)
        assert np.array_equal(res.best_alpha_ind, plain.best_alpha_ind) and np.array_equal(res.actions, plain.actions)
        assert np.array_equal(res.keep, plain.keep)
        if dtype == 'f32':
            assert np.array_equal(res.alpha, plain.alpha)
            assert res.stats['n_refined'] > 0.5 * res.stats['n_pairs']     # the refinement did the deciding
        else:
            assert_alpha_close(res.alpha, np.asarray(plain.alpha, dtype=np.float64), F64_RTOL)
        assert_alpha_close(res.alpha, want_rows, F32_RTOL if dtype == 'f32' else F64_RTOL)
    # back to one Gamma on the same engine: the untiled path again, same bits
    eng.set_gamma_tiling('off')
    again = eng.backup_full(alpha, b, gamma, belief_dominance_prune=True)
    check_path(again.stats, 1)
    assert np.array_equal(again.alpha, plain.alpha) and np.array_equal(again.best_alpha_ind, plain.best_alpha_ind)
    eng.close()


@pytest.mark.parametrize('prune', [False, True])
def test_run_fetch_with_early_rows_on_a_tiled_call(prune):
    """``pbvi_backup_run_fetch`` (rows of the provisional decision leave under the refinement) on a tiled call against
    ``run`` + ``fetch`` of the untiled engine, bit for bit."""
    from pomdp_pbvi_exploration_amd.engine import PinnedBuffer
    S, A, O, R, rs, rto, er, alpha, b, gamma = seam_inputs()
    B = b.shape[0]
    eng = Engine(S, A, O, R, rs, rto, er, dtype='f32')
    alpha_side(eng)
    eng.set_alpha(alpha)
    eng.set_beliefs(b)
    eng.set_gamma_tiling('off')
    st = eng.run(gamma, prune)
    check_path(st, 1)
    want = eng.fetch()
    buf = PinnedBuffer(B * S * 4 + 4 * B * 4 + B * A * O * 4 + B + 8192)
    rows = buf.carve((B, S), eng.np_dtype)
    slot, index, actions = (buf.carve((B,), np.int32) for _ in range(3))
    best = buf.carve((B, A, O), np.int32)
    keep = buf.carve((B,), np.uint8)
    eng.set_gamma_tiling('always', 100)
    for _ in range(2):
        rows[:] = np.nan
        st2, U, used = eng.run_fetch_into(gamma, rows, slot, index, actions, best=best, keep=keep, belief_dominance_prune=prune)
        check_path(st2, 3)
        assert U == want.unique_alpha.shape[0] and used >= U
        assert np.array_equal(index, want.index) and np.array_equal(actions, want.actions)
        assert np.array_equal(best, want.best_alpha_ind) and np.array_equal(keep.astype(bool), want.keep.astype(bool))
        assert np.array_equal(np.asarray(rows)[slot[:U]], want.unique_alpha)
    del rows, slot, index, actions, best, keep
    buf.close()
    eng.close()


def test_alpha_side_backup_that_does_not_fit_is_served_tiled():
    """The capability: the shape and cap of test_backup_that_does_not_fit_is_done_in_belief_chunks (R = 5, V = 6000, B = 256,
    fp32, the engine may allocate 1600 MiB more).  Untiled, the alpha side raises MemoryError there (Gamma alone is 1.0 GB
    beside 0.8 GB of refinement work lists) and the solver falls back to belief chunks.  With ``tile_gamma`` the ONE engine
    call succeeds on the alpha side within the cap, and the result is the uncapped untiled backup's."""
    from pomdp_pbvi_exploration_amd import PBVI_Solver, ValueFunction, BeliefSet
    from pomdp_pbvi_exploration_amd.engine import debug_alloc_limit
    from test_policy_eval import mirror_model
    m = synth.olfactory_model(H=30, W=80, R=5, f32=False)
    gm = mirror_model(m).to_gpu(dtype='f32')
    rng = np.random.default_rng(11)
    V, B = 6000, 256
    vf = ValueFunction(gm, rng.standard_normal((V, m.S)), rng.integers(0, m.A, V))
    bs = BeliefSet(gm, synth.belief_points(m, B).astype(np.float64))
    eng = gm.engine

    def key(res):
        arr, a = np.asarray(res.alpha_vector_array), np.asarray(res.actions)
        order = np.lexsort(arr.T[::-1])
        return arr[order], a[order]

    tiled = PBVI_Solver(gamma=m.gamma, eps=1e-6)
    tiled.tile_gamma = True
    plain = PBVI_Solver(gamma=m.gamma, eps=1e-6)
    assert plain.tile_gamma is False and eng.gamma_tiling[0] == 'off'
    cap = eng.device_bytes // (1 << 20) + 1600
    peak = []
    prev = debug_alloc_limit(cap)
    try:
        # mode off under the cap: MemoryError from the engine call, and the engine recovers
        eng.set_formulation('alpha')
        eng.sync_rows('alpha', vf.alpha_vector_list, lambda v: v.values, owner=vf)
        eng.sync_rows('belief', bs.belief_list, lambda b: b.values, owner=bs)
        with pytest.raises(MemoryError):
            eng.run(m.gamma, False)
        assert eng.alpha_count == 0                           # back to the freshly created state
        # tile_gamma: one engine call, alpha side, within the cap
        got = tiled.backup(gm, bs, vf, belief_dominance_prune=False)
        peak.append(eng.device_bytes)
        assert eng.gamma_tiling[0] == 'auto'
        assert tiled._belief_chunk is None
        assert eng.last_stats['formulation'] == 1 and eng.last_stats['gamma_chunks'] > 1, eng.last_stats
        chunks = eng.last_stats['gamma_chunks']
        # left to choose the side, the tiled engine follows its cost model (alpha side at this shape) ...
        eng.set_formulation('auto')
        got_auto = tiled.backup(gm, bs, vf, belief_dominance_prune=False)
        peak.append(eng.device_bytes)
        assert tiled._belief_chunk is None
        assert eng.last_stats['formulation'] == 1 and eng.last_stats['gamma_chunks'] > 1, eng.last_stats
        # ... where the untiled one takes the belief side for memory
        eng.set_gamma_tiling('off')
        plain.backup(gm, bs, vf, belief_dominance_prune=False)
        assert plain._belief_chunk is None and eng.last_stats['formulation'] == 2 and eng.last_stats['gamma_chunks'] == 0
    finally:
        debug_alloc_limit(prev)
    assert max(peak) <= cap << 20, (peak, cap)
    eng.set_gamma_tiling('off')
    eng.set_formulation('alpha')
    want = plain.backup(gm, bs, vf, belief_dominance_prune=False)     # uncapped, untiled, the reference's order
    assert eng.last_stats['formulation'] == 1 and eng.last_stats['gamma_chunks'] == 1 and plain._belief_chunk is None
    eng.set_formulation('auto')
    print(f'capped alpha-side backup: {chunks} Gamma chunks, engine held {max(peak) >> 20} MiB of {cap} MiB')
    rw, aw = key(want)
    for g in (got, got_auto):
        rg, ag = key(g)
        assert rw.shape == rg.shape and np.array_equal(aw, ag)
        np.testing.assert_allclose(rg, rw, rtol=1e-6, atol=0)


def test_full_size_r5_in_four_chunks_against_reference():
    """olfactory_full_R5_1024.npz (|S| = 30000, R = 5, V = B = 1024) with Gamma in 4 chunks of 256 alpha rows: 0 of 18432
    indices differ from the reference's."""
    path = os.path.join(GOLDEN, 'olfactory_full_R5_1024.npz')
    z = np.load(path, allow_pickle=False)
    V, B = int(z['V']), int(z['B'])
    m = synth.olfactory_model(R=int(z['R']))
    alpha, _ = synth.alpha_set(m, V)
    beliefs = synth.belief_points(m, B)
    if synth.checksum(m.reachable_states, m.rto, m.expected_rewards, alpha, beliefs) != str(z['inputs_sha256']):
        pytest.skip('host regenerated different input bits than the fixture machine (exp/libm); parity unpinned here')
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f32')
    alpha_side(eng)
    eng.set_gamma_tiling('always', V // 4)
    res = eng.backup_full(alpha, beliefs, m.gamma, belief_dominance_prune=True)
    check_path(res.stats, 4)
    mism = int(np.sum(res.best_alpha_ind != z['core_best']))
    assert res.best_alpha_ind.size == 18432 and mism == 0, f'{mism} of {res.best_alpha_ind.size} best_alpha_ind differ'
    assert np.array_equal(res.actions, z['core_actions'])
    a64 = res.alpha.astype(np.float64)
    np.testing.assert_allclose(a64.sum(axis=1), z['row_sum'], rtol=F32_RTOL)
    np.testing.assert_allclose(np.sum(beliefs * a64, axis=1), z['b_dot'], rtol=F32_RTOL)
    np.testing.assert_allclose(a64[z['sample_b'], z['sample_s']], z['sample_val'], rtol=F32_RTOL, atol=1e-12)
    assert len(orc.dedup_rows(res.alpha, res.actions)[1]) == int(z['n_unique'])
    held_tiled = eng.device_bytes
    eng.set_gamma_tiling('off')
    plain = eng.backup_full(alpha, beliefs, m.gamma, belief_dominance_prune=True)
    check_path(plain.stats, 1)
    assert np.array_equal(plain.alpha, res.alpha) and np.array_equal(plain.best_alpha_ind, res.best_alpha_ind)
    assert np.array_equal(plain.keep, res.keep)
    print(f"4 chunks: project {res.stats['ms_project']:.2f} score {res.stats['ms_score']:.2f} fold+argmax {res.stats['ms_argmax']:.2f} "
          f"total {res.stats['ms_total']:.2f} ms, held {held_tiled >> 20} MiB; untiled total {plain.stats['ms_total']:.2f} ms, "
          f"held {eng.device_bytes >> 20} MiB")
    eng.close()


def test_settings_are_checked_and_ignored_where_gamma_is_compact():
    z, rs, rto, er = small(1)
    eng = Engine(600, 6, 3, 1, rs, rto, er, dtype='f32')
    with pytest.raises(ValueError):
        eng._ck(eng._lib.pbvi_set_gamma_tiling(eng._h, 3, 0))
    with pytest.raises(ValueError):
        eng._ck(eng._lib.pbvi_set_gamma_tiling(eng._h, 1, -4))
    with pytest.raises(KeyError):
        eng.set_gamma_tiling('sometimes')
    alpha_side(eng)
    eng.set_gamma_tiling('always', 8)
    res = eng.backup_full(z['alpha'], z['beliefs'], float(z['gamma']))
    if res.stats['fused_projection'] == 1:                    # R = 1, fused: Gamma is compact already
        check_path(res.stats, 1)
    assert np.array_equal(res.best_alpha_ind, z['core_best'])
    eng.close()
    z5, rs, rto, er = small(5)
    dense = Engine(600, 6, 3, 5, rs, rto, er, dtype='f32', mode='dense')
    dense.set_gamma_tiling('always', 8)
    res = dense.backup_full(z5['alpha'], z5['beliefs'], float(z5['gamma']))
    assert res.stats['gamma_chunks'] == 1 and np.array_equal(res.best_alpha_ind, z5['core_best'])
    dense.close()
