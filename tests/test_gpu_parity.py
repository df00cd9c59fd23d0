"""Parity of the HIP engine (through the C-ABI) with the oracle / the reference's golden outputs.

Bar (BASELINE.json north_star): argmax indices bit-exact, fp32 alpha values within 1e-6
relative; f64 engines within 1e-12.  All tests here need a real MI355X.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_npz
from model_cases import assert_backup_matches_oracle, random_case as _random_case
from oracle import pbvi_oracle as orc
from pomdp_pbvi_exploration_amd import (Belief, BeliefSet, PBVI_Solver, ValueFunction, load_POMDP_file, synth)
from pomdp_pbvi_exploration_amd.engine import Engine
from score_cases import shifted_model

pytestmark = pytest.mark.gpu

F32_RTOL = 1e-6
F64_RTOL = 1e-12



# The suite is also run with the engine's debug switches set; assertions about which path a DEFAULT
# engine takes only hold without them.
SCREEN_DEFAULT = os.environ.get('PBVI_F64_SCREEN', 'auto') in ('', 'auto', '1')
FUSION_ALLOWED = os.environ.get('PBVI_NO_FUSED_PROJECT') is None
DEFAULT_PIPELINE = SCREEN_DEFAULT and os.environ.get('PBVI_FORMULATION', 'auto') in ('', 'auto', '0')

def rel_err(x, ref):
    scale = np.maximum(np.abs(ref), 1e-30)
    return float(np.max(np.abs(np.asarray(x, dtype=np.float64) - ref) / np.maximum(scale, np.max(np.abs(ref)) * 1e-6)))


def assert_alpha_close(x, ref, rtol):
    x = np.asarray(x, dtype=np.float64)
    np.testing.assert_allclose(x, ref, rtol=rtol, atol=rtol * max(1e-300, float(np.max(np.abs(ref)))) * 1e-3)


def small(R):
    z = load_npz(f'olfactory_small_R{R}.npz')
    return z, z['reachable_states'].astype(np.int64), z['rto'].astype(np.float64), z['expected_rewards'].astype(np.float64)


@pytest.mark.parametrize('R', [1, 5])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_small_olfactory_matches_reference(R, dtype):
    z, rs, rto, er = small(R)
    S, A, Rr = rs.shape
    eng = Engine(S, A, rto.shape[2], Rr, rs, rto, er, dtype=dtype)
    res = eng.backup_full(z['alpha'], z['beliefs'], float(z['gamma']), belief_dominance_prune=True)
    assert np.array_equal(res.best_alpha_ind, z['core_best']), 'best_alpha_ind differs from the reference'
    assert np.array_equal(res.actions, z['core_actions'])
    assert_alpha_close(res.alpha, z['core_alpha'], F32_RTOL if dtype == 'f32' else F64_RTOL)
    if dtype == 'f64':
        assert np.array_equal(res.keep, z['core_keep'])
    st = res.stats
    assert st['n_pairs'] == z['beliefs'].shape[0] * A * 3 and st['ms_total'] > 0
    # dedup of the engine rows reproduces the reference ValueFunction (first position, last action)
    rows, acts = orc.dedup_rows(res.alpha, res.actions)
    assert rows.shape == z['plain_alpha'].shape and np.array_equal(acts, z['plain_actions'])
    eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_dense_projection_mode(dtype):
    """BASELINE config 2 path (K1 as batched MFMA GEMMs over densified T.O matrices) on the small
    olfactory model and on a random model with repeated successors and multi-tile shapes."""
    z, rs, rto, er = small(5)
    eng = Engine(600, 6, 3, 5, rs, rto, er, dtype=dtype, mode='dense')
    res = eng.backup_full(z['alpha'], z['beliefs'], float(z['gamma']), belief_dominance_prune=True)
    assert np.array_equal(res.best_alpha_ind, z['core_best']) and np.array_equal(res.actions, z['core_actions'])
    assert_alpha_close(res.alpha, z['core_alpha'], F32_RTOL if dtype == 'f32' else F64_RTOL)
    assert res.stats['project_flops'] == 2 * 18 * 48 * 600 * 600
    eng.close()
    rng = np.random.default_rng(11)
    S, A, O, R, V, B = (700, 2, 3, 4, 300, 70) if dtype == 'f32' else (90, 2, 3, 4, 40, 30)
    rs, rto, er = random_model(rng, S, A, O, R)
    alpha = rng.normal(scale=3.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.4)
    b[:, 1] += 1e-3
    b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    new, act, best = orc.backup_core(alpha, b, rs, rto, er, 0.95)
    eng = Engine(S, A, O, R, rs, rto, er, dtype=dtype, mode='dense')
    res = eng.backup_full(alpha, b, 0.95)
    assert np.array_equal(res.best_alpha_ind, best) and np.array_equal(res.actions, act)
    assert_alpha_close(res.alpha, new, F32_RTOL if dtype == 'f32' else F64_RTOL)
    eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_device_dedup_is_consistent_with_reference_dedup(dtype):
    """K6: unique rows + index reproduce the per-belief matrix, and the rows handed to ValueFunction equal
    the reference's byte-dedup result (first position, order of first occurrence) incl. the prune variant."""
    z, rs, rto, er = small(1)
    eng = Engine(600, 6, 3, 1, rs, rto, er, dtype=dtype)
    res = eng.backup_full(z['alpha'], z['beliefs'], float(z['gamma']), belief_dominance_prune=True)
    U = res.unique_alpha.shape[0]
    assert U == res.stats['n_unique'] == eng.unique_count and 1 <= U <= 64
    assert res.index.min() == 0 and res.index.max() == U - 1
    full = eng.fetch_full()                                   # expanded on the device
    assert np.array_equal(full, res.alpha)
    # index[b] points at the first belief with b's key, so unique rows appear in first-occurrence order
    first = np.array([np.flatnonzero(res.index == u)[0] for u in range(U)])
    assert np.all(np.diff(first) > 0)
    key = np.concatenate([res.actions[:, None], res.best_alpha_ind[np.arange(64), res.actions]], axis=1)
    assert len({tuple(k) for k in key}) == U
    # different keys may still give identical bytes: ValueFunction's byte dedup (oracle restatement) finishes the job
    rows, acts = orc.dedup_rows(*res.value_function_rows(use_keep=False))
    assert rows.shape == z['plain_alpha'].shape and np.array_equal(acts, z['plain_actions'])
    assert_alpha_close(rows, z['plain_alpha'], F32_RTOL if dtype == 'f32' else F64_RTOL)
    if dtype == 'f64':
        rows, acts = orc.dedup_rows(*res.value_function_rows(use_keep=True))
        assert rows.shape == z['prune_alpha'].shape and np.array_equal(acts, z['prune_actions'])
    eng.close()


def test_grid4x3_every_reference_call_f64():
    """BASELINE config 1: 4x3 grid, fp64, every backup call of the reference's seeded FSVI run."""
    z = load_npz('grid4x3_fsvi.npz')
    t = load_npz('grid4x3_tables.npz')
    rs, rto, er = t['reachable_states'], t['rto'], t['expected_rewards']
    eng = Engine(12, 4, 6, rs.shape[2], rs, rto, er, dtype='f64')
    for i in range(int(z['n_calls'])):
        res = eng.backup_full(z[f'c{i}_alpha'], z[f'c{i}_beliefs'], 0.95, belief_dominance_prune=True)
        assert np.array_equal(res.best_alpha_ind, z[f'c{i}_core_best']), f'call {i}'
        assert np.array_equal(res.actions, z[f'c{i}_core_actions']), f'call {i}'
        assert_alpha_close(res.alpha, z[f'c{i}_core_alpha'], F64_RTOL)
        assert np.array_equal(res.keep, z[f'c{i}_core_keep']), f'call {i}'
    eng.close()


def test_grid4x3_f32_engine_against_oracle_on_rounded_inputs():
    z = load_npz('grid4x3_fsvi.npz')
    t = load_npz('grid4x3_tables.npz')
    r32 = lambda a: a.astype(np.float32).astype(np.float64)
    rs, rto, er = t['reachable_states'], r32(t['rto']), r32(t['expected_rewards'])
    eng = Engine(12, 4, 6, rs.shape[2], rs, rto, er, dtype='f32')
    for i in (0, 3, 9):
        alpha, b = r32(z[f'c{i}_alpha']), r32(z[f'c{i}_beliefs'])
        new, act, best = orc.backup_core(alpha, b, rs, rto, er, 0.95)
        res = eng.backup_full(alpha, b, 0.95)
        assert np.array_equal(res.best_alpha_ind, best) and np.array_equal(res.actions, act)
        assert_alpha_close(res.alpha, new, F32_RTOL)
    eng.close()


def test_python_api_backup_on_gpu_objects():
    """The reference seam: PBVI_Solver.backup on .to_gpu() objects returns the reference ValueFunction."""
    z = load_npz('grid4x3_fsvi.npz')
    model, _ = load_POMDP_file(os.path.join(GOLDEN, 'models', '4x3.95-no_loop_2_grid.POMDP'))
    solver = PBVI_Solver(gamma=0.95)
    gm = model.gpu_model
    for i in (1, 5):
        vf = ValueFunction(gm, z[f'c{i}_alpha'], z[f'c{i}_actions'])
        bs = BeliefSet(gm, z[f'c{i}_beliefs'])
        assert vf.is_on_gpu and bs.is_on_gpu
        out = solver.backup(gm, bs, vf, append=bool(z[f'c{i}_append']), belief_dominance_prune=False)
        assert out.alpha_vector_array.shape == z[f'c{i}_out_alpha'].shape
        assert_alpha_close(out.alpha_vector_array, z[f'c{i}_out_alpha'], F64_RTOL)
        assert np.array_equal(out.actions, z[f'c{i}_out_actions'])
        out = solver.backup(gm, bs, vf)                       # notebook-style direct call: prune on, append off
        assert out.alpha_vector_array.shape == z[f'c{i}_prune_alpha'].shape
        assert np.array_equal(out.actions, z[f'c{i}_prune_actions'])


def test_kat_tiger_on_gpu_and_full_solve():
    kat = json.load(open(os.path.join(GOLDEN, 'kat.json')))
    model, solver = load_POMDP_file(os.path.join(GOLDEN, 'models', 'tiger.95.POMDP'))
    gm = model.gpu_model
    vf0 = ValueFunction(gm, model.expected_rewards_table.T, model.actions)
    out = solver.backup(gm, BeliefSet(gm, [Belief(gm)]), vf0, belief_dominance_prune=False)
    np.testing.assert_allclose(out.alpha_vector_array, [[-1.95, -1.95]], rtol=1e-14)
    assert list(out.actions) == [0]
    model.end_actions = [1, 2]
    vf, hist = solver.solve(model, expansions=8, update_passes=8, use_gpu=True, print_progress=False)
    assert hist.beliefs_counts == kat['kat3_belief_counts']
    assert len(vf) == 5
    order = np.lexsort(np.asarray(kat['kat3_alpha']).T)
    got = np.asarray(vf.alpha_vector_array)
    np.testing.assert_allclose(got[np.lexsort(got.T)], np.asarray(kat['kat3_alpha'])[order], rtol=1e-9)


def random_model(rng, S, A, O, R):
    rs = rng.integers(0, S, size=(S, A, R))
    p = rng.random((S, A, R))
    p[rng.random((S, A, R)) < 0.3] = 0.0          # padded / impossible successors
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


@pytest.mark.parametrize('S,A,O,R,V,B', [(12, 4, 6, 3, 1, 1), (33, 1, 1, 1, 5, 3), (100, 3, 2, 4, 257, 300),
                                         (1000, 2, 5, 2, 64, 513), (257, 5, 3, 1, 300, 17)])
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_ragged_shapes_and_mixed_sign_alpha(S, A, O, R, V, B, dtype):
    """Edge shapes (single rows, sizes straddling the 256/32 padding, one action/observation) with
    mixed-sign alpha and sparse beliefs; oracle on the same (f32-representable) inputs."""
    rng = np.random.default_rng(S * 7 + V)
    rs, rto, er = random_model(rng, S, A, O, R)
    alpha = rng.normal(scale=10.0, size=(V, S)).astype(np.float32).astype(np.float64)
    if V > 2:
        alpha[2] = alpha[0]                                   # exact duplicate: first index must win
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.3)
    b[:, 0] += 1e-3
    b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    new, act, best = orc.backup_core(alpha, b, rs, rto, er, 0.9)
    eng = Engine(S, A, O, R, rs, rto, er, dtype=dtype)
    res = eng.backup_full(alpha, b, 0.9, belief_dominance_prune=True)
    assert np.array_equal(res.best_alpha_ind, best)
    assert np.array_equal(res.actions, act)
    assert_alpha_close(res.alpha, new, F32_RTOL if dtype == 'f32' else F64_RTOL)
    keep = orc.belief_dominance_mask(alpha, b, np.asarray(res.alpha, dtype=np.float64))
    assert np.array_equal(res.keep, keep)
    val, idx = eng.max_value(alpha, b)
    np.testing.assert_allclose(val, orc.max_value_per_belief(alpha, b), rtol=1e-12, atol=1e-12)
    assert np.array_equal(idx, np.argmax(b @ alpha.T, axis=1))
    eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_prune_dominated_matches_reference_loop(dtype):
    rng = np.random.default_rng(5)
    S, V = 700, 90
    base = rng.random((V, S))
    base[10] = base[3] - 0.5             # dominated
    base[11] = base[4]                   # duplicate pair: both go
    base[12] = np.maximum(base[5], base[6]) + 0.1   # dominates 5 and 6
    base = base.astype(np.float32).astype(np.float64)
    rs = np.zeros((S, 1, 1), dtype=np.int64)
    eng = Engine(S, 1, 1, 1, rs, np.ones((S, 1, 1, 1)), np.zeros((S, 1)), dtype=dtype)
    keep = eng.prune_dominated(base)
    assert np.array_equal(keep, orc.prune_dominated_mask(base))
    assert not keep[10] and not keep[11] and not keep[4] and not keep[5] and not keep[6] and keep[12]
    eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_prune_level2_matches_the_reference_fixture(dtype):
    """SURVEY 8a row a12 pinned to the reference: the rows ``ValueFunction.prune(2)`` of the reference kept on the seeded
    set of prune_level2.npz (make_golden.py prune), through ``pbvi_prune_dominated`` and through the Python seam."""
    z = load_npz('prune_level2.npz')
    alpha, kept = z['alpha'], z['kept']
    S = alpha.shape[1]
    rs = np.zeros((S, 1, 1), dtype=np.int64)
    eng = Engine(S, 1, 1, 1, rs, np.ones((S, 1, 1, 1)), np.zeros((S, 1)), dtype=dtype)
    keep = eng.prune_dominated(alpha)
    assert np.array_equal(np.flatnonzero(keep), kept)
    assert not keep[-1] and not keep[-2]                    # the +0 / -0 pair: each dominates the other
    eng.close()
    m = synth.olfactory_model(H=15, W=40, R=1)
    from pomdp_pbvi_exploration_amd import Model
    gm = Model(states=m.S, actions=m.A, observations=m.O, reachable_states=m.reachable_states,
               observation_table=m.observation_table, end_states=[m.goal], start_probabilities=list(m.start_belief)).to_gpu(dtype)
    vf = ValueFunction(gm, alpha, z['actions'])
    assert len(vf) == alpha.shape[0]
    vf.prune(2)
    assert np.array_equal(np.asarray(vf.alpha_vector_array, dtype=np.float64), alpha[kept])
    assert np.array_equal(vf.actions, z['actions'][kept])


def test_value_function_size_limiter_on_the_engine():
    """SURVEY 8f-1, second half (src/pomdp.py:2347-2365): the usefulness scan of the |V| limiter on the device
    (``pbvi_value_max_store`` indices over the whole belief store) inside the reference's seeded FSVI run of
    limiter_fsvi.npz -- the deletion draws from np.random, so the |V| trajectory only reproduces if every ``useful`` set
    along the way is the reference's.  f64 engine: the reference's arithmetic."""
    from test_host_api import _limiter_solve
    z, vf, hist = _limiter_solve(use_gpu=True)
    assert vf.is_on_gpu
    assert hist.beliefs_counts == list(z['belief_counts'])
    assert hist.alpha_vector_counts == list(z['alpha_counts'])
    np.testing.assert_allclose(hist.value_function_changes, z['changes'], rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(np.asarray(vf.alpha_vector_array), z['final_alpha'], rtol=1e-9, atol=1e-12)
    assert np.array_equal(vf.actions, z['final_actions'])


def test_gemm_alone_decides_almost_everything():
    """With the fp64 refinement window shut, the raw MFMA score GEMM must still reproduce the
    reference argmax except on genuine near-ties (guards against refinement masking a GEMM bug)."""
    z, rs, rto, er = small(5)
    eng = Engine(600, 6, 3, 5, rs, rto, er, dtype='f32')
    eng.set_tie_window(1e-30)
    res = eng.backup_full(z['alpha'], z['beliefs'], float(z['gamma']))
    agree = np.mean(res.best_alpha_ind == z['core_best'])
    assert agree > 0.97, agree
    eng.set_tie_window(-1.0)
    res = eng.backup_full(z['alpha'], z['beliefs'], float(z['gamma']))
    assert np.array_equal(res.best_alpha_ind, z['core_best'])
    eng.close()


def test_errors_are_reported_not_fatal():
    z, rs, rto, er = small(1)
    eng = Engine(600, 6, 3, 1, rs, rto, er, dtype='f32')
    with pytest.raises(ValueError):
        eng.run(0.99)                                        # nothing resident yet
    with pytest.raises(ValueError):
        eng.set_alpha(np.zeros((3, 599)))
    with pytest.raises(ValueError):
        Engine(600, 6, 3, 1, rs + 600, rto, er)
    eng.set_alpha(z['alpha'])
    eng.append_alpha(z['alpha'][:7])
    assert eng.alpha_count == 48 + 7
    eng.close()


def full_inputs(R, V, B):
    m = synth.olfactory_model(R=R)
    alpha, _ = synth.alpha_set(m, V)
    beliefs = synth.belief_points(m, B)
    return m, alpha, beliefs


@pytest.mark.parametrize('tag', ['R1', 'R5', 'R5_1024'])
def test_full_size_against_reference_summary(tag):
    """BASELINE configs 2-3 (|S|=30000): the engine against the reference's own backup on the same
    regenerated inputs (R = 1 at V = B = 1024; the stochastic R = 5 variant at V = B = 512 and at the benchmark's
    V = B = 1024).  Indices exact; row sums, b.alpha' and 4096 sampled values within 1e-6."""
    R = int(tag[1])
    path = os.path.join(GOLDEN, f'olfactory_full_{tag}.npz')
    if not os.path.exists(path):
        pytest.skip('full-size fixture missing')
    z = np.load(path, allow_pickle=False)
    V, B = int(z['V']), int(z['B'])
    m, alpha, beliefs = full_inputs(R, V, B)
    sha = synth.checksum(m.reachable_states, m.rto, m.expected_rewards, alpha, beliefs)
    if sha != str(z['inputs_sha256']):
        pytest.skip('host regenerated different input bits than the fixture machine (exp/libm); parity unpinned here')
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f32')
    res = eng.backup_full(alpha, beliefs, m.gamma, belief_dominance_prune=True)
    mism = int(np.sum(res.best_alpha_ind != z['core_best']))
    assert mism == 0, f'{mism} of {res.best_alpha_ind.size} best_alpha_ind differ'
    assert np.array_equal(res.actions, z['core_actions'])
    a64 = res.alpha.astype(np.float64)
    np.testing.assert_allclose(a64.sum(axis=1), z['row_sum'], rtol=F32_RTOL)
    np.testing.assert_allclose(np.sum(beliefs * a64, axis=1), z['b_dot'], rtol=F32_RTOL)
    np.testing.assert_allclose(a64[z['sample_b'], z['sample_s']], z['sample_val'], rtol=F32_RTOL, atol=1e-12)
    assert len(orc.dedup_rows(res.alpha, res.actions)[1]) == int(z['n_unique'])
    val, _ = eng.max_value(alpha, beliefs)
    np.testing.assert_allclose(val, z['value_max'], rtol=1e-12)
    # belief dominance: equal wherever the f64 margin is not inside f32 rounding of alpha'
    margin = np.abs(z['b_dot'] - z['value_max']) / np.maximum(np.abs(z['value_max']), 1e-30)
    clear = margin > 1e-6
    assert np.array_equal(res.keep[clear], z['core_keep'][clear])
    print(f"R={R}: refined {res.stats['n_refined']}/{res.stats['n_pairs']} pairs, dead {res.stats['n_dead']}, "
          f"score GEMM {res.stats['ms_score']:.2f} ms, total {res.stats['ms_total']:.2f} ms")

    # size-independent properties at the full size ------------------------------------------ #
    again = eng.backup_full(alpha, beliefs, m.gamma)
    assert np.array_equal(again.alpha, res.alpha) and np.array_equal(again.best_alpha_ind, res.best_alpha_ind)  # deterministic
    perm = np.argsort(synth.splitmix64(5, np.arange(B, dtype=np.uint64)))
    pb = eng.backup_full(alpha, beliefs[perm], m.gamma)
    assert np.array_equal(pb.alpha, res.alpha[perm]) and np.array_equal(pb.actions, res.actions[perm])          # belief order is free
    vperm = np.argsort(synth.splitmix64(6, np.arange(V, dtype=np.uint64)))
    pv = eng.backup_full(alpha[vperm], beliefs, m.gamma)
    # alpha order only renames indices -- except all-tie triples (P(o|b,a)=0), where both runs pick index 0
    mism = vperm[pv.best_alpha_ind] != res.best_alpha_ind
    assert np.all((pv.best_alpha_ind[mism] == 0) & (res.best_alpha_ind[mism] == 0))
    assert np.array_equal(pv.actions, res.actions)
    np.testing.assert_allclose(np.sum(beliefs * pv.alpha, axis=1), np.sum(beliefs * res.alpha, axis=1), rtol=F32_RTOL)
    sc = eng.backup_full(alpha * 2.0, beliefs, m.gamma)                                                           # scaling by 2 is exact
    assert np.array_equal(sc.best_alpha_ind, res.best_alpha_ind)
    eng.close()


def _check_against_full_fixture(res, z, beliefs):
    mism = int(np.sum(res.best_alpha_ind != z['core_best']))
    assert mism == 0, f'{mism} of {res.best_alpha_ind.size} best_alpha_ind differ'
    assert np.array_equal(res.actions, z['core_actions'])
    a64 = res.alpha.astype(np.float64)
    np.testing.assert_allclose(a64.sum(axis=1), z['row_sum'], rtol=F32_RTOL)
    np.testing.assert_allclose(np.sum(beliefs * a64, axis=1), z['b_dot'], rtol=F32_RTOL)
    np.testing.assert_allclose(a64[z['sample_b'], z['sample_s']], z['sample_val'], rtol=F32_RTOL, atol=1e-12)
    assert len(orc.dedup_rows(res.alpha, res.actions)[1]) == int(z['n_unique'])


def _full_fixture(R):
    """R: 1, 5 or a tag such as '5_1024' (olfactory_full_R5_1024.npz)."""
    path = os.path.join(GOLDEN, f'olfactory_full_R{R}.npz')
    if not os.path.exists(path):
        pytest.skip('full-size fixture missing')
    z = np.load(path, allow_pickle=False)
    m, alpha, beliefs = full_inputs(int(z['R']), int(z['V']), int(z['B']))
    if synth.checksum(m.reachable_states, m.rto, m.expected_rewards, alpha, beliefs) != str(z['inputs_sha256']):
        pytest.skip('host regenerated different input bits than the fixture machine (exp/libm); parity unpinned here')
    return z, m, alpha, beliefs


def test_full_size_dense_projection_against_reference():
    """BASELINE config 2 (C3) at its full size: S=30000, V=B=1024, the projection as |A||O| MFMA GEMMs over the densified
    65 GB of T.O matrices, against the reference's own outputs for this workload (olfactory_full_R1.npz).  Run twice:
    with zero-tile skipping (what the engine does by itself) and with every tile of both GEMMs multiplied (what bench.py
    measures as c3_dense) -- skipped tiles only ever add +0, so the results must be the same bits."""
    from pomdp_pbvi_exploration_amd.engine import debug_gemm_dense
    z, m, alpha, beliefs = _full_fixture(1)
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f32', mode='dense')
    res = eng.backup_full(alpha, beliefs, m.gamma)
    _check_against_full_fixture(res, z, beliefs)
    assert res.stats['project_flops'] == 2 * 18 * 1024 * 30000 * 30000
    prev = debug_gemm_dense(True)
    try:
        full = eng.backup_full(alpha, beliefs, m.gamma)
    finally:
        debug_gemm_dense(prev)
    assert full.stats['project_flops_executed'] >= full.stats['project_flops'] > res.stats['project_flops_executed']
    assert np.array_equal(full.best_alpha_ind, res.best_alpha_ind) and np.array_equal(full.actions, res.actions)
    assert np.array_equal(full.alpha, res.alpha)
    print(f"dense C3: projection GEMM {full.stats['ms_project_gemm']:.1f} ms true-dense, {res.stats['ms_project_gemm']:.2f} ms with "
          f"zero tiles skipped; step {full.stats['ms_total']:.1f} / {res.stats['ms_total']:.2f} ms")
    eng.close()


def test_full_size_poisoned_allocations():
    """Regression for the round-1 abort: the full-size sparse backup with every fresh device allocation
    filled with 0xFF (NaN / -1).  A kernel that reads memory the engine did not write -- or a poison fill that races
    with the engine's streams, which is what the abort was -- shows up as wrong indices or a fault at THIS shape, where
    the first call allocates ~4 GB inside pbvi_backup_run."""
    from pomdp_pbvi_exploration_amd.engine import debug_poison
    z, m, alpha, beliefs = _full_fixture(1)
    prev = debug_poison(True)
    try:
        eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f32')
        res = eng.backup_full(alpha, beliefs, m.gamma, belief_dominance_prune=True)
        _check_against_full_fixture(res, z, beliefs)
        # second call with a smaller alpha set: buffers are re-used with shifted row groups and stale contents
        half = eng.backup_full(alpha[:600], beliefs, m.gamma)
        eng.close()
    finally:
        debug_poison(prev)
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f32')
    clean = eng.backup_full(alpha[:600], beliefs, m.gamma)
    assert np.array_equal(half.best_alpha_ind, clean.best_alpha_ind) and np.array_equal(half.actions, clean.actions)
    assert np.array_equal(half.alpha, clean.alpha)
    eng.close()


def test_row_stores_select_in_host_order():
    """Device row stores: rows uploaded once, working sets selected by id in the caller's order.  The
    selection order decides argmax ties (lowest index wins), exactly as a re-uploaded matrix would."""
    z, rs, rto, er = small(5)
    eng = Engine(600, 6, 3, 5, rs, rto, er, dtype='f32')
    alpha, b, g = z['alpha'].astype(np.float64), z['beliefs'].astype(np.float64), float(z['gamma'])
    a0 = eng.store_rows('alpha', alpha[:30])
    a1 = eng.store_rows('alpha', alpha[30:])
    b0 = eng.store_rows('belief', b)
    assert (a0, a1, b0) == (0, 30, 0)
    # host order: the later-uploaded block first (ValueFunction.extend puts new vectors first), plus a duplicate
    order = np.concatenate([np.arange(30, 48), np.arange(0, 30), [35]])
    eng.select_alpha(order)
    eng.select_beliefs(np.arange(64)[::-1])
    eng.run(g)
    res = eng.fetch()
    ref = eng.backup_full(alpha[order], b[::-1], g)               # same sets, re-uploaded the plain way
    assert np.array_equal(res.best_alpha_ind, ref.best_alpha_ind) and np.array_equal(res.actions, ref.actions)
    assert np.array_equal(res.alpha, ref.alpha)
    new, act, best = orc.backup_core(alpha[order], b[::-1], rs, rto, er, g)
    assert np.array_equal(res.best_alpha_ind, best) and np.array_equal(res.actions, act)
    assert not np.any(res.best_alpha_ind == 48)                    # the duplicate (last position) never wins a tie
    val, idx = eng.max_value_resident()
    np.testing.assert_allclose(val, orc.max_value_per_belief(alpha[order], b[::-1]), rtol=1e-12)
    with pytest.raises(ValueError):
        eng.select_alpha([0, 999])
    eng.reset_store('alpha')
    assert eng.store_rows('alpha', alpha[:2]) == 0
    eng.close()


def test_value_max_over_the_belief_store_in_place(monkeypatch):
    """pbvi_value_max_store: compute_change's maxima with the belief store itself as the GEMM operand -- no gather, no
    sort, zero maps and tile lists extended as rows arrive.  Equal to the gathered-block path and to the oracle, across
    appends that leave partial 256-row blocks, for f32 (exact re-scoring) and f64 engines."""
    m = synth.olfactory_model(H=15, W=40, R=5)
    beliefs = synth.belief_points(m, 700, max_depth=24)
    for dtype, n_alpha in (('f32', 80), ('f32', 40), ('f64', 40)):
        alpha, _ = synth.alpha_set(m, n_alpha)
        alpha[7] = alpha[3]                                           # an exact tie: the lower index must win
        want = orc.max_value_per_belief(alpha.astype(np.float64), beliefs.astype(np.float64))
        # f32 engines against more than 64 alpha rows re-score every belief on its own (bit-identical whatever block it
        # rides in); the fp64 tile engine -- fp64 engines, and fp32 ones against at most 64 rows -- splits K by the shape of
        # its grid, so launches of different shapes agree to summation order (a few ulps), indices exactly
        same = np.array_equal if (dtype, n_alpha) == ('f32', 80) else (lambda a, b: np.allclose(a, b, rtol=1e-14, atol=0.0))
        eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype=dtype)
        eng.store_rows('alpha', alpha)
        eng.select_alpha(np.arange(len(alpha)))
        done = 0
        for upto in (100, 256, 300, 700):                         # partial block, exact block, straddling, several blocks
            eng.store_rows('belief', beliefs[done:upto])
            done = upto
            val, idx = eng.max_value_store()
            assert len(val) == upto
            eng.select_beliefs(np.arange(upto))
            v2, i2 = eng.max_value_resident()
            assert same(val, v2) and np.array_equal(idx, i2)
            np.testing.assert_allclose(val, want[:upto], rtol=1e-12 if dtype == 'f64' else 1e-7)
            assert not np.any(idx == 7)
        v_part, _ = eng.max_value_store(513)
        assert same(v_part, val[:513])
        # the resident block survives the store scan untouched
        v3, i3 = eng.max_value_resident()
        assert same(v3, v2) and np.array_equal(i3, i2)
        # Engine.max_value_objects takes the store path for large belief sets
        monkeypatch.setattr(Engine, '_STORE_SCAN_MIN', 64)
        ids = np.arange(700, dtype=np.int32)[::2]
        got = eng._vmax_block(np.arange(len(alpha), dtype=np.int32), ids)
        assert same(got, val[ids])
        monkeypatch.undo()
        eng.reset_store('belief')
        eng.store_rows('belief', beliefs[5:9])
        v4, _ = eng.max_value_store()
        assert same(v4, val[5:9])
        with pytest.raises(ValueError):
            eng.max_value_store(5)
        eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_working_alpha_set_grown_at_the_front_equals_an_uploaded_one(dtype):
    """pbvi_alpha_select: a selection that is k new store rows followed by the previous selection (the solve loop's
    new-then-old value function) is gathered into free rows in front of the resident set instead of re-gathering
    everything; a much smaller selection in between (compute_change's fresh rows) goes beside it.  After every step the
    engine must behave exactly as one that was handed the same rows with pbvi_alpha_set: same indices, actions and rows,
    same value-max -- through several prepends, a small selection, exhausted free rows (fresh layout) and, for fp64
    engines, the fp32 screen's incremental copy."""
    m = synth.olfactory_model(H=15, W=40, R=5)
    pool, _ = synth.alpha_set(m, 2100)
    pool[1700] = pool[3]                                             # a tie across the old / new boundary: lower index wins
    beliefs = synth.belief_points(m, 300, max_depth=24)
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype=dtype)
    ref = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype=dtype)
    if dtype == 'f64':
        eng.set_f64_screen('always')
        ref.set_f64_screen('always')
    eng.store_rows('alpha', pool)
    eng.set_beliefs(beliefs)
    ids = np.arange(0, 300, dtype=np.int32)

    def check(ids):
        eng.select_alpha(ids)
        st = eng.run(m.gamma, True)
        got = eng.fetch()
        want = ref.backup_full(pool[ids], beliefs, m.gamma, belief_dominance_prune=True)
        assert np.array_equal(got.best_alpha_ind, want.best_alpha_ind) and np.array_equal(got.actions, want.actions)
        assert np.array_equal(got.keep, want.keep) and np.array_equal(got.index, want.index)
        assert np.array_equal(got.unique_alpha, want.unique_alpha)
        v1, i1 = eng.max_value_resident()
        v2, i2 = ref.max_value_resident()
        assert np.array_equal(v1, v2) and np.array_equal(i1, i2)
        return st

    check(ids)
    layouts_taken = []
    assert eng.alpha_layout() == (True, 512, 1)                      # free rows: max(512, V / 2)
    nxt = 300
    for k in (40, 1, 200, 300, 0, 500, 700):                         # 300 + ... : the free rows (512) run out on the way
        if k == 200:                                                 # a small selection in between leaves the big one alone
            small = np.array([5, 1700, 3, 77], dtype=np.int32)
            eng.select_alpha(small)
            v, i = eng.max_value_resident()
            vr, ir = ref.max_value(pool[small], beliefs)
            assert np.array_equal(v, vr) and np.array_equal(i, ir)
            assert not np.any(i == 2)                                # rows 1 and 2 of the small set are equal: the later never wins
            assert eng.alpha_layout()[0] is False                    # beside the big selection, which is untouched:
        ids = np.concatenate([np.arange(nxt, nxt + k, dtype=np.int32), ids])
        nxt += k
        check(ids)
        layouts_taken.append(eng.alpha_layout())
    # 40, 1, 200 fit the 512 free rows (271 left); 300 does not: fresh layout (841 rows: 512 free... max(512, 420)); 0 and
    # 500 fit; 700 does not
    assert layouts_taken == [(True, 472, 1), (True, 471, 1), (True, 271, 1), (True, 512, 2), (True, 512, 2), (True, 12, 2),
                             (True, 1020, 3)]
    # any other selection (not an extension) starts a fresh layout
    check(ids[::-1].copy())
    eng.close()
    ref.close()


@pytest.mark.parametrize('n_alpha', [5, 16, 17, 33, 48, 49, 64, 65, 130])
def test_value_max_column_tile_widths(n_alpha):
    """The fp64 tile engine's 16 / 32 / 48 / 64 / 128-column variants (fp64 engines: every width; fp32 engines: up to 64
    rows, both operands widened) on either side of each boundary: values against the oracle, exact ties to the lower
    index, a belief count that leaves a partial 128-row block."""
    m = synth.olfactory_model(H=15, W=40, R=5)
    alpha, _ = synth.alpha_set(m, n_alpha)
    alpha[n_alpha - 1] = alpha[2]                                     # exact tie across the width of the tile
    beliefs = synth.belief_points(m, 333, max_depth=24)
    want = orc.max_value_per_belief(alpha.astype(np.float64), beliefs.astype(np.float64))
    scores = beliefs.astype(np.float64) @ alpha.astype(np.float64).T
    for dtype in ('f32', 'f64'):
        eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype=dtype)
        val, idx = eng.max_value(alpha, beliefs)
        np.testing.assert_allclose(val, want, rtol=1e-12)
        assert not np.any(idx == n_alpha - 1)
        # the index is a maximiser of the fp64 scores (up to their own rounding) and never the later of two equal rows
        np.testing.assert_allclose(scores[np.arange(len(idx)), idx], want, rtol=1e-12)
        eng.close()


def test_value_max_skinny_at_full_size():
    """S = 30000: a few hundred beliefs against 40 alpha rows -- the shape compute_change produces -- through the K-split
    skinny tiles of both engine types (a handful of tile pairs, each split along K); values against NumPy's fp64 dots."""
    m = synth.olfactory_model(H=75, W=400, R=1)
    alpha, _ = synth.alpha_set(m, 40)
    alpha[31] = alpha[7]
    beliefs = synth.belief_points(m, 300, max_depth=50)
    want = (beliefs.astype(np.float64) @ alpha.astype(np.float64).T).max(axis=1)
    for dtype in ('f32', 'f64'):
        eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype=dtype)
        val, idx = eng.max_value(alpha, beliefs)
        np.testing.assert_allclose(val, want, rtol=1e-12)
        assert not np.any(idx == 31)
        eng.close()


def test_value_max_without_fp64_rescoring_stays_within_the_f32_bar():
    """pbvi_set_value_max_exact(0) (what compute_change uses on f32 engines): the fp32 GEMM's maxima, within 1e-6
    relative of the exact ones; exact mode is back afterwards; max_value_objects keeps exact and inexact results apart."""
    from pomdp_pbvi_exploration_amd.mdp import AlphaVector
    m = synth.olfactory_model(H=15, W=40, R=5)
    alpha, _ = synth.alpha_set(m, 80)          # more than 64 rows: the fp32 stream-K GEMM (fewer take the fp64-accumulating tile)
    beliefs = synth.belief_points(m, 300, max_depth=24)
    want = orc.max_value_per_belief(alpha.astype(np.float64), beliefs.astype(np.float64))
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f32')
    eng.store_rows('alpha', alpha)
    eng.store_rows('belief', beliefs)
    eng.select_alpha(np.arange(80))
    eng.select_beliefs(np.arange(300))
    exact, _ = eng.max_value_resident()
    np.testing.assert_allclose(exact, want, rtol=1e-12)
    eng.set_value_max_exact(False)
    fast, _ = eng.max_value_resident()
    fast_store, _ = eng.max_value_store()
    eng.set_value_max_exact(True)
    np.testing.assert_allclose(fast, want, rtol=1e-6)
    np.testing.assert_allclose(fast_store, want, rtol=1e-6)
    assert not np.array_equal(fast, exact)                         # it really is the un-rescored value
    again, _ = eng.max_value_resident()
    assert np.array_equal(again, exact)

    class Row:
        def __init__(self, v):
            self.values = v
    A, Bl = [AlphaVector(r, 0) for r in alpha], [Row(r) for r in beliefs]
    v_fast = eng.max_value_objects(A, Bl, lambda v: v.values, lambda x: x.values, exact=False)
    v_exact = eng.max_value_objects(A, Bl, lambda v: v.values, lambda x: x.values)
    np.testing.assert_allclose(v_exact, want, rtol=1e-12)
    np.testing.assert_allclose(v_fast, want, rtol=1e-6)
    eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('B', [40, 300])
def test_backup_in_the_belief_side_formulation_also_yields_the_value_maxima(dtype, B):
    """pbvi_backup_fetch_value_max: in the belief-side formulation the beliefs ride along as extra rows of the score
    GEMM, so the backup also knows max_v b.alpha_v of its beliefs (compute_change's next question).  f64 engines: the
    value pbvi_value_max returns; f32 engines: the GEMM's maxima (1e-6); caller order also when the block is sorted;
    an alpha-side backup has no such values."""
    import ctypes as C
    m = synth.olfactory_model(H=15, W=40, R=5)
    alpha, _ = synth.alpha_set(m, 200)
    beliefs = synth.belief_points(m, B, max_depth=24)
    want = orc.max_value_per_belief(alpha.astype(np.float64), beliefs.astype(np.float64))
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype=dtype)
    eng.set_alpha(alpha)
    eng.set_beliefs(beliefs)
    out = np.empty(B, dtype=np.float64)
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    eng.set_formulation('belief')
    st = eng.run(m.gamma)
    assert st['formulation'] == 2
    if st['screened']:     # (PBVI_F64_SCREEN=always) a screened backup's GEMM rows are fp32: it offers no exact maxima
        assert eng._lib.pbvi_backup_fetch_value_max(eng._h, ptr) == -4
        eng.close()
        return
    assert eng._lib.pbvi_backup_fetch_value_max(eng._h, ptr) == 0
    np.testing.assert_allclose(out, want, rtol=1e-12 if dtype == 'f64' else 1e-6)
    res_push = eng.fetch()
    exact, _ = eng.max_value_resident()
    if dtype == 'f64':
        assert np.array_equal(out, exact)
    eng.set_formulation('alpha')
    st = eng.run(m.gamma)
    assert st['formulation'] == 1
    assert eng._lib.pbvi_backup_fetch_value_max(eng._h, ptr) == -4
    res_pull = eng.fetch()                                          # the extra rows changed nothing of the backup itself
    assert np.array_equal(res_push.best_alpha_ind, res_pull.best_alpha_ind) and np.array_equal(res_push.actions, res_pull.actions)
    eng.close()


def test_solver_loop_on_gpu_keeps_rows_resident():
    """FSVI on the 4x3 grid through the Python API with use_gpu=True: every backup goes through the row
    stores; the trajectory equals the host NumPy path's (same seeds)."""
    import random
    from pomdp_pbvi_exploration_amd import FSVI_Solver
    z = load_npz('grid4x3_fsvi.npz')
    results = []
    for use_gpu in (False, True):
        model, _ = load_POMDP_file(os.path.join(GOLDEN, 'models', '4x3.95-no_loop_2_grid.POMDP'))
        model.end_states = [3, 6]
        np.random.seed(0)
        random.seed(0)
        vf, hist = FSVI_Solver(gamma=0.95, eps=1e-6).solve(model, expansions=10, max_belief_growth=10, use_gpu=use_gpu,
                                                           print_progress=False)
        results.append((hist.alpha_vector_counts, np.asarray(vf.alpha_vector_array, dtype=np.float64), np.asarray(vf.actions)))
    assert results[0][0] == results[1][0] == list(z['alpha_counts'])
    np.testing.assert_allclose(results[1][1], results[0][1], rtol=1e-10, atol=1e-12)
    assert np.array_equal(results[0][2], results[1][2])


@pytest.mark.parametrize('seed', range(8))
def test_random_shapes_f32(seed):
    """Random models / sizes through every device-side mechanism (tile lists, stream-K shares, belief
    reordering, tail rows, key dedup): indices exact, values within 1e-6 of the oracle."""
    rng = np.random.default_rng(1000 + seed)
    S = int(rng.integers(40, 2500))
    A, O, R = int(rng.integers(1, 5)), int(rng.integers(1, 5)), int(rng.integers(1, 4))
    V, B = int(rng.integers(1, 700)), int(rng.integers(1, 900))
    rs, rto, er = random_model(rng, S, A, O, R)
    # block-structured sparsity so zero tiles really occur on both operands
    lo, hi = sorted(rng.integers(0, S, size=2))
    rto[lo:hi, :, O - 1, :] = 0.0
    alpha = rng.normal(scale=5.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.2)
    for i in range(B):                                       # each belief lives on a window of states
        w0 = int(rng.integers(0, S))
        mask = np.zeros(S, dtype=bool)
        mask[w0:w0 + max(8, S // 6)] = True
        b[i] *= mask
        b[i, w0] += 1e-3
    b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    gamma = float(rng.choice([0.5, 0.9, 0.99]))
    new, act, best = orc.backup_core(alpha, b, rs, rto, er, gamma)
    eng = Engine(S, A, O, R, rs, rto, er, dtype='f32')
    res = eng.backup_full(alpha, b, gamma, belief_dominance_prune=True)
    assert np.array_equal(res.best_alpha_ind, best), (S, A, O, R, V, B)
    assert np.array_equal(res.actions, act)
    assert_alpha_close(res.alpha, new, F32_RTOL)
    assert np.array_equal(eng.fetch_full(), res.alpha)
    keep = orc.belief_dominance_mask(alpha, b, np.asarray(res.alpha, dtype=np.float64))
    assert np.array_equal(res.keep, keep)
    eng.close()


def test_no_read_of_unwritten_device_memory():
    """Poisoned allocations (0xFF = NaN / -1): shapes where (a,o) groups share GEMM tiles with each other and
    with the tail rows, so a projection that skipped tiles the GEMM still reads would show up."""
    from pomdp_pbvi_exploration_amd.engine import debug_poison
    prev = debug_poison(True)
    try:
        rng = np.random.default_rng(77)
        for (S, A, O, R, V, B) in [(1828, 1, 1, 1, 136, 125), (700, 2, 3, 2, 100, 300), (333, 3, 2, 1, 257, 40)]:
            rs, rto, er = random_model(rng, S, A, O, R)
            lo, hi = S // 3, 2 * S // 3
            rto[lo:hi, :, O - 1, :] = 0.0                       # one group without support where ER / others have it
            alpha = rng.normal(scale=5.0, size=(V, S)).astype(np.float32).astype(np.float64)
            b = rng.random((B, S)) * (rng.random((B, S)) < 0.3)
            b[:, lo] += 1e-3
            b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
            new, act, best = orc.backup_core(alpha, b, rs, rto, er, 0.95)
            for mode in ('sparse', 'dense'):
                eng = Engine(S, A, O, R, rs, rto, er, dtype='f32', mode=mode)
                for V_use in (V, max(1, V // 2)):               # second run re-uses buffers with shifted row groups
                    n2, a2, b2 = (new, act, best) if V_use == V else orc.backup_core(alpha[:V_use], b, rs, rto, er, 0.95)
                    res = eng.backup_full(alpha[:V_use], b, 0.95, belief_dominance_prune=True)
                    assert np.array_equal(res.best_alpha_ind, b2) and np.array_equal(res.actions, a2), (S, V_use, mode)
                    assert_alpha_close(res.alpha, n2, F32_RTOL)
                eng.close()
    finally:
        debug_poison(prev)


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_batched_belief_update(dtype):
    """Bayes step on the device against the oracle's restatement of Belief.update."""
    z, rs, rto, er = small(5)
    b = z['beliefs'].astype(np.float64)
    rng = np.random.default_rng(3)
    act = rng.integers(0, 6, size=64)
    obs = rng.integers(0, 2, size=64)                      # observation 2 (goal) is impossible for most beliefs
    eng = Engine(600, 6, 3, 5, rs, rto, er, dtype=dtype)
    out = eng.belief_update(b, act, obs)
    ref = np.stack([orc.belief_update(b[i], int(act[i]), int(obs[i]), rs, rto) for i in range(64)])
    np.testing.assert_allclose(out, ref, rtol=2e-6 if dtype == 'f32' else 1e-12, atol=1e-12)
    np.testing.assert_allclose(out.sum(axis=1), 1.0, atol=1e-5)
    # impossible observation -> 0/0 = NaN, like the reference
    out2 = eng.belief_update(b[:3], [0, 0, 0], [2, 2, 2])
    with np.errstate(invalid='ignore', divide='ignore'):
        ref2 = np.stack([orc.belief_update(b[i], 0, 2, rs, rto) for i in range(3)])
    assert np.array_equal(np.isnan(out2), np.isnan(ref2))
    # large enough block to be reordered internally: results must come back in the caller's order
    m = synth.olfactory_model(H=15, W=40, R=5)
    bb = synth.belief_points(m, 300, max_depth=16)
    a3, o3 = rng.integers(0, 6, size=300), np.zeros(300, dtype=np.int64)
    out3 = eng.belief_update(bb, a3, o3)
    ref3 = np.stack([orc.belief_update(bb[i], int(a3[i]), 0, rs, rto) for i in range(300)])
    np.testing.assert_allclose(out3, ref3, rtol=2e-6 if dtype == 'f32' else 1e-12, atol=1e-12)
    eng.close()


@pytest.mark.parametrize('S,B', [(2000, 128), (30000, 300)])
def test_adversarial_near_ties(S, B):
    """alpha-vectors that differ by 1e-5 ... 1e-9 relative (far below f32 GEMM rounding for the small gaps):
    every argmax must match the fp64 reference exactly, which only the window + fp64 refinement can deliver."""
    rng = np.random.default_rng(42)
    A, O, R = 2, 2, 1 if S > 5000 else 2
    rs, rto, er = random_model(rng, S, A, O, R)
    base = rng.random(S) * 10.0 + 1.0
    V = 96
    alpha = np.empty((V, S))
    for v in range(V):
        eps = 10.0 ** -(5 + (v % 5))                         # 1e-5 .. 1e-9
        alpha[v] = base * (1.0 + eps * rng.standard_normal(S))
    alpha[7] = alpha[3]                                       # and exact duplicates
    alpha = alpha.astype(np.float32).astype(np.float64)
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.05)
    b[:, 0] += 1e-3
    b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    new, act, best = orc.backup_core(alpha, b, rs, rto, er, 0.95)
    # sanity: the case really is adversarial for f32 (top-2 gaps below 1e-6 relative are common)
    G = orc.gamma_projection(alpha, rs, rto, 0.95)
    sc = np.tensordot(b[:16], G, (1, 3))
    top2 = np.sort(sc, axis=3)[..., -2:]
    gaps = (top2[..., 1] - top2[..., 0]) / np.maximum(np.abs(top2[..., 1]), 1e-30)
    assert np.median(gaps) < 1e-6
    eng = Engine(S, A, O, R, rs, rto, er, dtype='f32')
    res = eng.backup_full(alpha, b, 0.95)
    assert np.array_equal(res.best_alpha_ind, best), int(np.sum(res.best_alpha_ind != best))
    assert np.array_equal(res.actions, act)
    assert_alpha_close(res.alpha, new, F32_RTOL)
    assert res.stats['n_refined'] > 0.5 * res.stats['n_pairs']      # refinement did the deciding
    eng.close()


# --------------------------------------------------------------------------- #
# fp64 engines behind their fp32 screen (pbvi_set_f64_screen)
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('R', [1, 5])
def test_f64_engine_screened_equals_pure_at_full_size(R):
    """fp64 engine at |S|=30000: by default its scores come from the fp32 stream-K GEMM on rounded copies of the operands
    and every unclear (belief, action, observation) is re-decided from the fp64 originals.  Against the reference's own
    outputs (indices exact, values to 1e-12) and against the pure fp64 pipeline of the same engine (same bits)."""
    z, m, alpha, beliefs = _full_fixture(R)
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f64')
    if not SCREEN_DEFAULT:
        eng.set_f64_screen('auto')
    res = eng.backup_full(alpha, beliefs, m.gamma, belief_dominance_prune=True)
    assert res.stats['screened'] == 1
    assert np.array_equal(res.best_alpha_ind, z['core_best']), int(np.sum(res.best_alpha_ind != z['core_best']))
    assert np.array_equal(res.actions, z['core_actions'])
    a64 = np.asarray(res.alpha, dtype=np.float64)
    np.testing.assert_allclose(a64.sum(axis=1), z['row_sum'], rtol=F64_RTOL)
    np.testing.assert_allclose(np.sum(beliefs * a64, axis=1), z['b_dot'], rtol=F64_RTOL)
    np.testing.assert_allclose(a64[z['sample_b'], z['sample_s']], z['sample_val'], rtol=F64_RTOL, atol=1e-15)
    assert np.array_equal(res.keep, z['core_keep'])
    eng.set_f64_screen('off')
    pure = eng.backup_full(alpha, beliefs, m.gamma, belief_dominance_prune=True)
    assert pure.stats['screened'] == 0
    assert np.array_equal(pure.best_alpha_ind, res.best_alpha_ind) and np.array_equal(pure.actions, res.actions)
    assert np.array_equal(pure.alpha, res.alpha) and np.array_equal(pure.keep, res.keep)
    print(f"R={R}: screened {res.stats['ms_total']:.2f} ms (refined {res.stats['n_refined']}/{res.stats['n_pairs']}), "
          f"pure fp64 {pure.stats['ms_total']:.2f} ms")
    eng.close()


@pytest.mark.parametrize('formulation', ['alpha', 'belief'])
@pytest.mark.parametrize('R', [1, 5])
def test_f64_screen_forced_on_small_models(R, formulation):
    """The screen forced on the S=600 fixtures (where it would not engage by itself), both formulations: the reference's
    indices, actions, keep mask and values as for the pure fp64 engine."""
    z, rs, rto, er = small(R)
    S, A, Rr = rs.shape
    eng = Engine(S, A, rto.shape[2], Rr, rs, rto, er, dtype='f64')
    eng.set_f64_screen('always')
    eng.set_formulation(formulation)
    res = eng.backup_full(z['alpha'], z['beliefs'], float(z['gamma']), belief_dominance_prune=True)
    assert res.stats['screened'] == 1 and res.stats['formulation'] == (1 if formulation == 'alpha' else 2)
    assert np.array_equal(res.best_alpha_ind, z['core_best']) and np.array_equal(res.actions, z['core_actions'])
    assert_alpha_close(res.alpha, z['core_alpha'], F64_RTOL)
    assert np.array_equal(res.keep, z['core_keep'])
    eng.close()


def test_f64_screen_decides_what_fp32_cannot_see():
    """Genuinely fp64 operands: alpha-vectors 1e-7 ... 1e-11 apart (many of them the SAME fp32 number after rounding),
    beliefs and tables that are not fp32-representable.  The screen sees exact ties or noise there; every argmax must
    still be the fp64 reference's, which only the re-decision from the fp64 originals can deliver."""
    rng = np.random.default_rng(43)
    S, A, O, R, V, B = 3000, 2, 2, 2, 96, 128
    rs, rto, er = random_model(rng, S, A, O, R)
    rto = rto * (1.0 + 1e-9 * rng.standard_normal(rto.shape))          # not fp32-representable
    base = rng.random(S) * 10.0 + 1.0
    alpha = np.empty((V, S))
    for v in range(V):
        alpha[v] = base * (1.0 + 10.0 ** -(7 + (v % 5)) * rng.standard_normal(S))
    alpha[7] = alpha[3]                                                 # and exact duplicates
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.05)
    b[:, 0] += 1e-3
    b = b / b.sum(axis=1, keepdims=True)
    new, act, best = orc.backup_core(alpha, b, rs, rto, er, 0.95)
    eng = Engine(S, A, O, R, rs, rto, er, dtype='f64')
    eng.set_f64_screen('always')
    res = eng.backup_full(alpha, b, 0.95)
    assert res.stats['screened'] == 1
    assert np.array_equal(res.best_alpha_ind, best), int(np.sum(res.best_alpha_ind != best))
    assert np.array_equal(res.actions, act)
    assert_alpha_close(res.alpha, new, F64_RTOL)
    assert res.stats['n_refined'] > 0.5 * res.stats['n_pairs']
    eng.close()


# --------------------------------------------------------------------------- #
# MDP value iteration on the device
# --------------------------------------------------------------------------- #
def test_device_value_iteration_reproduces_reference_csv():
    """The reference's stored VI solution (see tests/test_host_api.py) from the device sweeps: R = 1, so every
    operation matches NumPy's and the rows are bit-identical to the host solver's."""
    from pomdp_pbvi_exploration_amd.mdp import VI_Solver
    from test_host_api import clipped_olfactory_mdp
    model = clipped_olfactory_mdp()
    ref = ValueFunction.load_from_file(os.path.join(GOLDEN, 'ref_value_function_61x361.csv.gzip'), model)
    host_vf, host_hist = VI_Solver(gamma=0.99, eps=1e-4).solve(model, print_progress=False)
    dev_vf, dev_hist = VI_Solver(gamma=0.99, eps=1e-4).solve(model, use_gpu=True, print_progress=False)
    assert len(dev_hist.iteration_times) == len(host_hist.iteration_times) == 460
    assert dev_hist.value_function_changes == host_hist.value_function_changes
    assert np.array_equal(dev_vf.alpha_vector_array, host_vf.alpha_vector_array)
    assert np.array_equal(dev_vf.actions, host_vf.actions)
    np.testing.assert_allclose(dev_vf.alpha_vector_array, ref.alpha_vector_array, rtol=0, atol=1e-12)


@pytest.mark.parametrize('seed', range(3))
def test_device_value_iteration_random_mdp(seed):
    """Stochastic MDPs (R > 1: the sum over r may associate differently from einsum's): 1e-13 relative; horizon
    cut-offs and per-sweep tracking follow the host solver."""
    from pomdp_pbvi_exploration_amd.mdp import Model as MDPModel, VI_Solver
    rng = np.random.default_rng(50 + seed)
    S, A, R = int(rng.integers(5, 3000)), int(rng.integers(1, 6)), int(rng.integers(2, 6))
    rs = np.stack([np.stack([rng.choice(S, size=R, replace=False) for _ in range(A)]) for _ in range(S)])
    model = MDPModel(states=S, actions=A, reachable_states=rs, rewards=lambda s, a, sn: ((s * 7 + a * 3 + sn) % 11) / 10.0)
    p = rng.random((S, A, R))
    model.reachable_probabilities = p / p.sum(axis=2, keepdims=True)
    for horizon, level in ((10000, 1), (7, 1), (5, 2)):
        solver = VI_Solver(horizon=horizon, gamma=0.9, eps=1e-3)
        host_vf, host_hist = solver.solve(model, history_tracking_level=level, print_progress=False)
        dev_vf, dev_hist = solver.solve(model, use_gpu=True, history_tracking_level=level, print_progress=False)
        assert len(dev_hist.iteration_times) == len(host_hist.iteration_times)
        np.testing.assert_allclose(dev_hist.value_function_changes, host_hist.value_function_changes, rtol=1e-9, atol=1e-13)
        np.testing.assert_allclose(dev_vf.alpha_vector_array, host_vf.alpha_vector_array, rtol=1e-13, atol=0)
        assert np.array_equal(dev_vf.actions, host_vf.actions)
        if level >= 2:
            assert len(dev_hist.value_functions) == len(host_hist.value_functions)
            np.testing.assert_allclose(dev_hist.value_functions[2].alpha_vector_array,
                                       host_hist.value_functions[2].alpha_vector_array, rtol=1e-13, atol=0)


# --------------------------------------------------------------------------- #
# Belief-side formulation (pbvi_set_formulation): same results as the alpha-side order
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('R', [1, 5])
def test_formulations_agree_and_auto_picks_by_shape(R, dtype):
    """Projecting the beliefs instead of the alpha-vectors re-associates the same sums: indices identical, values
    within 1e-6 of the oracle, on both; the automatic choice takes the belief side only when B << V."""
    if dtype == 'f64' and os.environ.get('PBVI_F64_SIMPLE'):
        pytest.skip('debug mode: the plain fp64 GEMM has no belief-side formulation')
    z = load_npz(f'olfactory_small_R{R}.npz')
    rs, rto, er = z['reachable_states'], z['rto'].astype(np.float64), z['expected_rewards'].astype(np.float64)
    S, A, O, Rr = rto.shape[0], rto.shape[1], rto.shape[2], rto.shape[3]
    alpha, b = z['alpha'].astype(np.float64), z['beliefs'].astype(np.float64)
    gamma = float(z['gamma'])
    want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, gamma)
    eng = Engine(S, A, O, Rr, rs, rto, er, dtype=dtype)
    tol = 1e-6 if dtype == 'f32' else 1e-12
    for which, expect in (('alpha', 1), ('belief', 2)):
        eng.set_formulation(which)
        eng.set_alpha(alpha)
        eng.set_beliefs(b)
        st = eng.run(gamma)
        assert st['formulation'] == expect
        res = eng.fetch()
        assert np.array_equal(res.actions, want_a)
        assert np.array_equal(res.best_alpha_ind, want_v)
        np.testing.assert_allclose(res.alpha, want_rows, rtol=tol, atol=tol * 0.1)
    # auto: 64 beliefs x 48 alpha-vectors -> alpha side; 4 beliefs x 2000 alpha-vectors -> belief side
    eng.set_formulation('auto')
    assert eng.run(gamma)['formulation'] == 1
    rng = np.random.default_rng(0)
    big = np.concatenate([alpha] + [alpha[rng.integers(0, len(alpha), 488)] * rng.uniform(0.5, 1.0, (488, 1)) for _ in range(4)])
    big = big.astype(np.float32).astype(np.float64)
    eng.set_formulation('auto')
    eng.set_alpha(big)
    eng.set_beliefs(b[:4])
    st = eng.run(gamma)
    assert st['formulation'] == 2
    res = eng.fetch()
    w_rows, w_a, w_v = orc.backup_core(big, b[:4], rs, rto, er, gamma)
    assert np.array_equal(res.actions, w_a) and np.array_equal(res.best_alpha_ind, w_v)
    np.testing.assert_allclose(res.alpha, w_rows, rtol=tol, atol=tol * 0.1)
    eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_max_value_objects_incremental_equals_from_scratch(dtype):
    """compute_change's max_v b.alpha_v on growing alpha / belief sets: the cached incremental evaluation
    (Engine.max_value_objects) returns what a from-scratch evaluation returns, for every query order the solve
    loop produces (grown set, previous set again, unrelated set, after a store reset)."""
    from pomdp_pbvi_exploration_amd.mdp import AlphaVector
    z = load_npz('olfactory_small_R5.npz')
    rs, rto, er = z['reachable_states'], z['rto'].astype(np.float64), z['expected_rewards'].astype(np.float64)
    alpha, b = z['alpha'].astype(np.float64), z['beliefs'].astype(np.float64)
    eng = Engine(rto.shape[0], rto.shape[1], rto.shape[2], rto.shape[3], rs, rto, er, dtype=dtype)

    class Row:                      # stands in for Belief: anything with .values
        def __init__(self, v):
            self.values = v
    A = [AlphaVector(r, 0) for r in alpha]
    Bl = [Row(r) for r in b]
    tol = 1e-12

    def check(a_idx, b_idx):
        got = eng.max_value_objects([A[i] for i in a_idx], [Bl[i] for i in b_idx], lambda v: v.values, lambda x: x.values)
        want = orc.max_value_per_belief(alpha[a_idx], b[b_idx])
        np.testing.assert_allclose(got, want, rtol=tol, atol=tol)

    a1, a2 = list(range(0, 20)), list(range(0, 33))
    b1, b2 = list(range(0, 30)), list(range(0, 64))
    check(a1, b1)                   # cold
    check(a2, b2)                   # alpha set and belief set both grew
    check(a1, b2)                   # the previous alpha set again, on the grown belief set
    check(a1, b2)                   # exact hit
    check(a2, b2)                   # exact hit of the other entry
    check(list(range(40, 48)), b1)  # unrelated alpha set
    check(list(range(10, 48)), b2[::-1])   # superset of none of the entries' sets... except the last; reordered beliefs
    eng.reset_store('alpha')
    for v in A:
        v.__dict__.pop('_dev', None)
    check(a2, b1)                   # ids restart after the reset: the cache must not survive it
    eng.close()


@pytest.mark.parametrize('formulation', ['alpha', 'belief'])
def test_exact_ties_with_hundreds_of_candidates(formulation):
    """Value functions are full of exact ties (every alpha-vector has the same value at an absorbing goal).  Here all
    arithmetic is exact by construction (dyadic beliefs / RTO / gamma, small-integer alpha rows drawn from five
    distinct rows), so every triple has ~140 exactly tied candidates: np.argmax takes the first, and so must the
    engine -- through the grid-wide refinement pass that scores long candidate lists."""
    rng = np.random.default_rng(77)
    S, A, O, R, V, B = 300, 2, 2, 1, 700, 40
    rs = rng.integers(0, S, size=(S, A, R))
    pick = rng.random((S, A)) < 0.5
    rto = np.empty((S, A, O, R))
    rto[:, :, 0, 0] = np.where(pick, 0.25, 0.75)
    rto[:, :, 1, 0] = 1.0 - rto[:, :, 0, 0]
    er = rng.integers(-4, 5, size=(S, A)).astype(np.float64)
    base = rng.integers(-8, 9, size=(5, S)).astype(np.float64)
    alpha = base[rng.integers(0, 5, size=V)]
    b = np.zeros((B, S))
    for i in range(B):
        np.add.at(b[i], rng.integers(0, S, size=64), 1.0 / 64.0)
    want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, 0.5)
    eng = Engine(S, A, O, R, rs, rto, er, dtype='f32')
    eng.set_formulation(formulation)
    eng.set_alpha(alpha)
    eng.set_beliefs(b)
    st = eng.run(0.5)
    res = eng.fetch()
    assert st['n_refine_candidates'] > 8 * st['n_refined'] > 0        # every refined triple left the in-block path
    assert np.array_equal(res.best_alpha_ind, want_v)
    assert np.array_equal(res.actions, want_a)
    np.testing.assert_array_equal(res.alpha, want_rows)
    val, idx = eng.max_value_resident()                               # value-max path: same machinery, G = 1
    sc = b @ alpha.T
    assert np.array_equal(idx, np.argmax(sc, axis=1))
    np.testing.assert_array_equal(val, sc.max(axis=1))
    eng.close()


@pytest.mark.parametrize('S,A,O,V,B,regular', [(1000, 2, 2, 512, 70, False), (4097, 3, 1, 300, 300, True), (2500, 1, 3, 777, 40, False),
                                                (30000, 2, 2, 256, 260, True)])
def test_fused_projection_gives_the_bits_of_the_projected_pipeline(S, A, O, V, B, regular):
    """Score GEMM with the Gamma tiles generated in its operand staging (R = 1) against the same engine with the projection
    as a kernel of its own (``pbvi_set_fused_projection``): same products, same rounding, same summation order, so every
    output -- indices, actions, alpha' bytes, and the refinement's work -- is identical, and both are the oracle's.  Shapes:
    groups that end inside a 256-row tile (V not a multiple of 256: straddling tiles stay projected), S not a multiple of 32,
    successor maps that are shifts (``regular``: 16-byte alpha loads) or random (every K tile takes the gather path)."""
    rng = np.random.default_rng(S + V)
    if regular:
        rs = ((np.arange(S)[:, None] + rng.integers(-5, 6, size=A)[None, :]) % S)[:, :, None].astype(np.int64)
    else:
        rs = rng.integers(0, S, size=(S, A, 1))
    p = rng.random((S, A, O))
    p[rng.random((S, A, O)) < 0.3] = 0.0
    p[:, :, 0] += 1e-3
    rto = (p / p.sum(axis=2, keepdims=True))[:, :, :, None].astype(np.float32).astype(np.float64)
    er = rng.normal(size=(S, A)).astype(np.float32).astype(np.float64)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.2)
    b[:, rng.integers(0, S, size=B)] += 1e-3
    b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, 0.9)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    out = {}
    for fused in (True, False):
        eng.set_fused_projection(fused)
        res = eng.backup_full(alpha, b, 0.9, belief_dominance_prune=True)
        assert res.stats['fused_projection'] == int(fused and FUSION_ALLOWED)
        assert np.array_equal(res.best_alpha_ind, want_v) and np.array_equal(res.actions, want_a), fused
        assert_alpha_close(res.alpha, want_rows, F32_RTOL)
        out[fused] = res
    f, u = out[True], out[False]
    assert np.array_equal(f.alpha, u.alpha) and np.array_equal(f.keep, u.keep)
    for k in ('n_refined', 'n_refine_candidates', 'n_refined_actions', 'n_dead', 'n_unique', 'score_tiles_run'):
        assert f.stats[k] == u.stats[k], k
    eng.close()


@pytest.mark.parametrize('S,A,O,R,V,B', [(4100, 2, 2, 2, 512, 70), (3000, 3, 1, 3, 300, 300), (9000, 1, 3, 5, 777, 40),
                                          (30000, 2, 2, 5, 256, 260), (5000, 2, 2, 7, 256, 64), (2048, 2, 2, 4, 256, 300)])
def test_fused_projection_with_several_reachable_states(S, A, O, R, V, B):
    """Score GEMM that generates its Gamma tiles from R = 2..7 successors per (s, a) (gemm.hip, scheduler 2c: the padded-ELL
    SpMM of src/pomdp.py:1485-1491 inside the B-operand staging) against the same engine with the projection as a kernel of
    its own: k_project's arithmetic operation for operation, so every output is identical, and both are the oracle's.
    Successor maps are shifts per (action, slot) with a sprinkle of random successors -- K tiles with such a chunk are
    projected and read, so generated and read K steps alternate inside one tile list -- and zero-probability pad slots as
    the reference's Model pads them (src/mdp.py:308-335)."""
    rng = np.random.default_rng(S + V + R)
    rs, rto, er = shifted_model(rng, S, A, O, R)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.2)
    b[:, rng.integers(0, S, size=B)] += 1e-3
    b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, 0.9)
    eng = Engine(S, A, O, R, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    out = {}
    for fused in (2, 1, 0):                                             # 1: "where it is faster" is R = 1 only
        eng.set_fused_projection(fused)
        res = eng.backup_full(alpha, b, 0.9, belief_dominance_prune=True)
        assert res.stats['fused_projection'] == int(fused == 2 and FUSION_ALLOWED)
        assert np.array_equal(res.best_alpha_ind, want_v) and np.array_equal(res.actions, want_a), fused
        assert_alpha_close(res.alpha, want_rows, F32_RTOL)
        out[fused] = res
    f, u = out[2], out[0]
    assert np.array_equal(f.alpha, u.alpha) and np.array_equal(f.keep, u.keep)
    for k in ('n_refined', 'n_refine_candidates', 'n_refined_actions', 'n_dead', 'n_unique', 'score_tiles_run'):
        assert f.stats[k] == u.stats[k], k
    eng.close()


def test_fused_projection_is_not_chosen_without_grid_structure():
    """R > 1 with random successors: every K tile would have to be projected AND read, so the engine keeps the projection
    kernel; R = 8 exceeds the 16 issue points of a K step."""
    rng = np.random.default_rng(5)
    for S, A, O, R in ((1200, 2, 2, 3), (1200, 1, 2, 8)):
        if R == 3:
            rs = rng.integers(0, S, size=(S, A, R))
        else:
            rs = (np.arange(S)[:, None, None] + rng.integers(-9, 10, size=(A, R))[None]) % S
        rs, rto, er = rs.astype(np.int64), *random_model(rng, S, A, O, R)[1:]
        alpha = rng.normal(size=(260, S)).astype(np.float32).astype(np.float64)
        b = rng.random((40, S))
        b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
        want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, 0.9)
        eng = Engine(S, A, O, R, rs, rto, er, dtype='f32')
        eng.set_formulation('alpha')
        eng.set_fused_projection(2)
        res = eng.backup_full(alpha, b, 0.9)
        assert res.stats['fused_projection'] == 0
        assert np.array_equal(res.best_alpha_ind, want_v) and np.array_equal(res.actions, want_a)
        eng.close()


_SEA_ROBIN = {}


def _sea_robin_case():
    if not _SEA_ROBIN:
        rng = np.random.default_rng(61875)
        H, W, A, O, V, B = 165, 375, 16, 2, 300, 100
        S = H * W
        y, x = np.divmod(np.arange(S), W)
        moves = [(-1, 0), (0, 1), (1, 0), (0, -1), (-2, 0), (0, 2), (2, 0), (0, -2), (-1, 1), (1, 1), (1, -1), (-1, -1), (0, 0),
                 (0, 5), (5, 0), (0, -5)]
        rs = np.stack([((y + dy) % H) * W + (x + dx) % W for dy, dx in moves], axis=1)[:, :, None].astype(np.int64)
        p = 0.05 + 0.9 * rng.random((S, A))
        p[rng.random((S, A)) < 0.2] = 0.0                                  # states where one observation is impossible
        rto = np.stack([p, 1.0 - p], axis=2)[:, :, :, None].astype(np.float32).astype(np.float64)
        er = (rng.random((S, A)) < 0.01).astype(np.float64)
        alpha = (rng.random((V, S)) * rng.random((V, 1)) * 10.0).astype(np.float32).astype(np.float64)
        b = rng.random((B, S)) * (rng.random((B, S)) < 0.1)
        b[:, 17] += 1e-3
        b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
        _SEA_ROBIN['case'] = (S, A, O, rs, rto, er, alpha, b, orc.backup_core_tiled(alpha, b, rs, rto, er, 0.99))
    return _SEA_ROBIN['case']


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_sea_robin_shape_against_oracle(dtype):
    """The shape of the reference's largest other model family (Sea_Robin_Real.ipynb: S=61875, A=16, O=2, one reachable
    state; its CuPy run went out of memory at |V|=1386): 32 (a,o) groups, S not a multiple of 32, V not a multiple of 256,
    successor maps that are grid moves with wrap-around.  Synthetic tables (the notebook's data files are not shipped);
    fp32 engine (fused GEMM) and fp64 engine (large enough for the screen to engage by itself), both formulations,
    against the oracle."""
    S, A, O, rs, rto, er, alpha, b, (want_rows, want_a, want_v) = _sea_robin_case()
    eng = Engine(S, A, O, 1, rs, rto, er, dtype=dtype)
    eng.set_formulation('alpha')
    res = eng.backup_full(alpha, b, 0.99)
    if dtype == 'f32':
        assert res.stats['fused_projection'] == int(FUSION_ALLOWED)
    elif SCREEN_DEFAULT:
        assert res.stats['screened'] == 1
    assert np.array_equal(res.best_alpha_ind, want_v), int(np.sum(res.best_alpha_ind != want_v))
    assert np.array_equal(res.actions, want_a)
    assert_alpha_close(res.alpha, want_rows, F32_RTOL if dtype == 'f32' else F64_RTOL)
    eng.set_formulation('belief')
    push = eng.backup_full(alpha, b, 0.99)
    assert push.stats['formulation'] == 2
    assert np.array_equal(push.best_alpha_ind, want_v) and np.array_equal(push.actions, want_a)
    eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_device_row_hashes_equal_the_host_hash(dtype):
    """pbvi_backup_fetch_row_hashes: the numbers the host's alpha-vector container keys on, computed where the rows are,
    equal ``_AlphaKey.hash_of`` of the fetched rows -- so a row hashed on the device and the same row hashed on the host
    meet in one dictionary slot -- and PBVI_Solver.backup hands them to the vectors it creates."""
    from pomdp_pbvi_exploration_amd.mdp import _AlphaKey
    from pomdp_pbvi_exploration_amd import Model
    z, rs, rto, er = small(5)
    eng = Engine(600, 6, 3, 5, rs, rto, er, dtype=dtype)
    res = eng.backup_full(z['alpha'], z['beliefs'], float(z['gamma']))
    h = eng.fetch_row_hashes()
    assert h.shape == (res.unique_alpha.shape[0],)
    assert [int(x) for x in h] == [_AlphaKey.hash_of(r) for r in res.unique_alpha]
    eng.close()
    m = synth.olfactory_model(H=15, W=40, R=1)
    gm = Model(states=m.S, actions=m.A, observations=m.O, reachable_states=m.reachable_states,
               observation_table=m.observation_table, end_states=[m.goal], start_probabilities=list(m.start_belief)).to_gpu(dtype)
    alpha, acts = synth.alpha_set(m, 40)
    rows = synth.belief_points(m, 30, max_depth=16)
    out = PBVI_Solver(gamma=m.gamma).backup(gm, BeliefSet(gm, [Belief(gm, r) for r in rows]), ValueFunction(gm, alpha, acts),
                                           append=True, belief_dominance_prune=False)
    new = [v for v in out.alpha_vector_list if '_hash' in v.__dict__]
    assert len(new) > 0 and all(v._hash == _AlphaKey.hash_of(v.values) for v in new)
    assert len(out) == len({v.values.tobytes() for v in out.alpha_vector_list})          # byte-dedup semantics intact


def test_speculative_refinement_recovers_when_ties_appear():
    """After a backup whose refinement deferred nothing the engine stops reading the deferred-work counts in the middle of
    the pipeline: it enqueues the later stages at once and checks the counts at the end.  Here the first backup has no
    ties (distinct random alpha rows), the second one -- same engine -- has ~140 exactly tied candidates per triple, so
    the speculation fails: the deferred passes run late and the later stages are repeated.  Results must be the oracle's
    either way, and the third backup (ties again) takes the synchronous route."""
    rng = np.random.default_rng(78)
    S, A, O, R, V, B = 300, 2, 2, 1, 700, 40
    rs = rng.integers(0, S, size=(S, A, R))
    pick = rng.random((S, A)) < 0.5
    rto = np.empty((S, A, O, R))
    rto[:, :, 0, 0] = np.where(pick, 0.25, 0.75)
    rto[:, :, 1, 0] = 1.0 - rto[:, :, 0, 0]
    er = rng.integers(-4, 5, size=(S, A)).astype(np.float64)
    plain = rng.normal(scale=3.0, size=(V, S)).astype(np.float32).astype(np.float64)
    base = rng.integers(-8, 9, size=(5, S)).astype(np.float64)
    tied = base[rng.integers(0, 5, size=V)]
    b = np.zeros((B, S))
    for i in range(B):
        np.add.at(b[i], rng.integers(0, S, size=64), 1.0 / 64.0)
    eng = Engine(S, A, O, R, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_beliefs(b)
    for k, alpha in enumerate((plain, plain, plain, tied, tied, plain, tied)):
        want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, 0.5)
        eng.set_alpha(alpha)
        st = eng.run(0.5, belief_dominance_prune=(k % 2 == 0))
        res = eng.fetch()
        assert np.array_equal(res.best_alpha_ind, want_v), k
        assert np.array_equal(res.actions, want_a), k
        if alpha is tied:
            assert st['n_refine_candidates'] > 8 * st['n_refined'] > 0
            np.testing.assert_array_equal(res.alpha, want_rows)
        else:
            assert_alpha_close(res.alpha, want_rows, F32_RTOL)
    eng.close()


@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_belief_walk_matches_host_updates(dtype):
    """pbvi_belief_walk: chained Bayes updates with restarts equal Belief.update applied step by step (fp64 engines:
    to rounding of the normaliser; f32 engines: to the f32 rounding of the model tables), and the rows it leaves in
    the belief store are the ones a following selection reads."""
    m = synth.olfactory_model(H=15, W=40, R=5, f32=(dtype == 'f32'))
    from test_policy_eval import mirror_model
    model = mirror_model(m)
    rng = np.random.default_rng(9)
    b0 = Belief(model)
    n = 40
    acts = rng.integers(0, m.A, size=n)
    obs = np.zeros(n, dtype=int)
    restart = rng.random(n) < 0.15
    restart[0] = True
    want, b = [], b0
    for i in range(n):
        if restart[i]:
            b = b0
        for o in rng.permutation(m.O):              # an observation that is possible from here
            nb = b.update(int(acts[i]), int(o))
            if np.isfinite(nb.values).all():
                obs[i] = o
                b = nb
                break
        want.append(b.values)
    want = np.array(want)
    eng = Engine.for_model(model, dtype=dtype)
    got, first = eng.belief_walk(b0.values, acts, obs, restart)
    from pomdp_pbvi_exploration_amd.mdp import _RowKey
    keys = eng.belief_walk_keys(len(acts))                       # the hash of the host's dedup key, from the device
    assert [int(k) for k in keys] == [int(_RowKey(r)) for r in got]
    with pytest.raises(ValueError):
        eng.belief_walk_keys(len(acts) + 1)
    tol = 1e-13 if dtype == 'f64' else 1e-6
    np.testing.assert_allclose(got, want, rtol=tol, atol=tol * 1e-3)
    assert np.allclose(got.sum(axis=1), 1.0, atol=1e-12)
    got2, first2 = eng.belief_walk(b0.values, acts[:5], obs[:5], None)     # appended after the first walk's rows
    assert first2 == first + n
    eng.select_beliefs(np.arange(first, first + n))
    np.testing.assert_allclose(eng.fetch_beliefs(), got.astype(eng.np_dtype), rtol=0, atol=0)
    eng.close()


def test_exact_ties_on_a_support_wider_than_the_lds_tile_list():
    """|S| = 131072 with dense dyadic beliefs: 4096 non-zero tiles per belief, twice what the refinement keeps in
    LDS -- the kernel falls back to the belief's global tile list.  Exact arithmetic again, so np.argmax's first
    index is the only right answer."""
    rng = np.random.default_rng(5)
    S, A, O, R, V, B = 131072, 1, 2, 1, 30, 3
    rs = rng.integers(0, S, size=(S, A, R))
    rto = np.empty((S, A, O, R))
    rto[:, :, 0, 0] = np.where(rng.random((S, A)) < 0.5, 0.25, 0.75)
    rto[:, :, 1, 0] = 1.0 - rto[:, :, 0, 0]
    er = rng.integers(-2, 3, size=(S, A)).astype(np.float64)
    base = rng.integers(-4, 5, size=(3, S)).astype(np.float64)
    alpha = base[rng.integers(0, 3, size=V)]
    b = np.zeros((B, S))
    b[0, :] = 1.0 / S
    b[1, :S // 2] = 2.0 / S
    b[2, S // 2:] = 2.0 / S
    want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, 0.5)
    eng = Engine(S, A, O, R, rs, rto, er, dtype='f32')
    eng.set_alpha(alpha)
    eng.set_beliefs(b)
    st = eng.run(0.5)
    res = eng.fetch()
    assert st['n_refined'] > 0 and st['n_refine_candidates'] >= 2 * st['n_refined']
    assert np.array_equal(res.best_alpha_ind, want_v)
    assert np.array_equal(res.actions, want_a)
    np.testing.assert_array_equal(res.alpha, want_rows)
    eng.close()


@pytest.mark.parametrize('name', ['tiger-grid.POMDP', 'hallway.POMDP', 'cheese.95.POMDP', '4x4.95.POMDP', '4x3.95.POMDP',
                                  'cit.POMDP'])
def test_fsvi_solves_of_example_models_match_reference_gpu(name, tmp_path):
    """The reference's seeded FSVI solves of its example models (up to 28 observations, 56 reachable states per
    (s, a)) through use_gpu=True: the fp64 engine reproduces the trajectories and the final alpha set; the f32 engine
    runs the same loop and agrees on the value of the start belief to f32 accuracy."""
    from test_host_api import solve_example
    if os.environ.get('PBVI_F64_SCREEN') == 'always' and name in ('4x4.95.POMDP', '4x3.95.POMDP'):
        # These symmetric grids have beliefs at which two actions tie EXACTLY in fp64; which one wins is rounding noise of
        # the summation order.  The pure fp64 pipeline happens to break those ties like the
        # reference's BLAS; a screened backup re-evaluates tied actions with its refinement's order and the seeded run
        # forks.  The screen never engages by itself at these sizes.
        pytest.skip('exact action-value ties: the forced screen breaks them in a different (equally valid) order')
    vf, hist, want = solve_example(name, tmp_path, use_gpu=True, engine_dtype='f64')
    assert hist.beliefs_counts == list(want['beliefs'])
    assert hist.alpha_vector_counts == list(want['alphas'])
    # The alpha SET must be the reference's.  Its order may differ where two actions tie exactly at a belief (the
    # symmetric 4x4 grid): the reference's pick then depends on its BLAS summation order, the engine's on its own.
    got = np.asarray(vf.alpha_vector_array, dtype=np.float64)
    key = lambda rows, acts: sorted((int(a),) + tuple(np.round(r, 8)) for r, a in zip(rows, acts))   # noqa: E731
    assert key(got, vf.actions) == key(want['alpha'], want['actions'])
    if name != '4x4.95.POMDP':
        assert np.array_equal(np.asarray(vf.actions), want['actions'])
        np.testing.assert_allclose(got, want['alpha'], rtol=1e-9, atol=1e-9)
    vf32, hist32, _ = solve_example(name, tmp_path, use_gpu=True, engine_dtype='f32')
    b0 = vf32.model.start_probabilities
    v64 = float(np.max(want['alpha'] @ b0))
    v32 = float(np.max(np.asarray(vf32.alpha_vector_array, dtype=np.float64) @ b0))
    assert hist32.beliefs_counts == list(want['beliefs'])
    assert abs(v32 - v64) <= 1e-4 * max(1.0, abs(v64))


@pytest.mark.parametrize('formulation', ['alpha', 'belief'])
@pytest.mark.parametrize('R', [1, 5])
def test_full_size_f64_engine_against_reference_summary(R, formulation):
    """The same full-size reference fixture through the fp64 engine (fp64 MFMA GEMM, no windows, no refinement),
    both operand formulations: indices exact, values to 1e-12."""
    if formulation == 'belief' and os.environ.get('PBVI_F64_SIMPLE'):
        pytest.skip('debug mode: the plain fp64 GEMM has no belief-side formulation')
    path = os.path.join(GOLDEN, f'olfactory_full_R{R}.npz')
    if not os.path.exists(path):
        pytest.skip('full-size fixture missing')
    z = np.load(path, allow_pickle=False)
    V, B = int(z['V']), int(z['B'])
    m, alpha, beliefs = full_inputs(R, V, B)
    if synth.checksum(m.reachable_states, m.rto, m.expected_rewards, alpha, beliefs) != str(z['inputs_sha256']):
        pytest.skip('host regenerated different input bits than the fixture machine (exp/libm); parity unpinned here')
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f64')
    eng.set_formulation(formulation)
    res = eng.backup_full(alpha, beliefs, m.gamma, belief_dominance_prune=True)
    assert res.stats['formulation'] == (1 if formulation == 'alpha' else 2)
    mism = int(np.sum(res.best_alpha_ind != z['core_best']))
    assert mism == 0, f'{mism} of {res.best_alpha_ind.size} best_alpha_ind differ'
    assert np.array_equal(res.actions, z['core_actions'])
    np.testing.assert_allclose(res.alpha.sum(axis=1), z['row_sum'], rtol=1e-12)
    np.testing.assert_allclose(np.sum(beliefs * res.alpha, axis=1), z['b_dot'], rtol=1e-12)
    np.testing.assert_allclose(res.alpha[z['sample_b'], z['sample_s']], z['sample_val'], rtol=1e-12, atol=1e-15)
    eng.close()


def test_backup_of_a_belief_set_larger_than_one_engine_block():
    """PBVI_Solver.backup splits belief sets beyond BELIEF_BLOCK into engine calls; rows and actions equal the
    single-call result (here with a block of 20 on the 64-belief small fixture)."""
    z = load_npz('olfactory_small_R1.npz')
    m = synth.olfactory_model(H=int(z['H']), W=int(z['W']), R=1)
    from test_policy_eval import mirror_model
    model = mirror_model(m).to_gpu('f32')
    vf = ValueFunction(model, z['alpha'].astype(np.float64), z['alpha_actions'].astype(int))
    bs = BeliefSet(model, z['beliefs'].astype(np.float64))
    solver = PBVI_Solver(gamma=float(z['gamma']))
    whole = solver.backup(model, bs, vf, belief_dominance_prune=False)
    solver.BELIEF_BLOCK = 20
    parts = solver.backup(model, bs, vf, belief_dominance_prune=False)
    assert np.array_equal(whole.alpha_vector_array, parts.alpha_vector_array)
    assert np.array_equal(whole.actions, parts.actions)


def test_end_to_end_fsvi_at_headline_scale_matches_reference():
    """The reference's own FSVI solve loop at S=30000 (40 expansions of <= 100 beliefs, seeds 0; 419 s and 9.3 s per
    backup on the fixture machine's CPU) through use_gpu=True with the fp64 engine: belief-count trajectory, |V|
    trajectory, per-backup changes and the value of the start belief."""
    import random
    from pomdp_pbvi_exploration_amd import FSVI_Solver, Model
    z = load_npz('olfactory_e2e_fsvi40.npz')
    m = synth.olfactory_model(R=1, f32=False)
    model = Model(states=m.S, actions=m.A, observations=m.O, reachable_states=m.reachable_states,
                  observation_table=m.observation_table, end_states=[m.goal], start_probabilities=list(m.start_belief))
    np.random.seed(0)
    random.seed(0)
    vf, hist = FSVI_Solver(gamma=m.gamma, eps=1e-6).solve(model, expansions=40, max_belief_growth=100, use_gpu=True,
                                                          engine_dtype='f64', print_progress=False)
    # The sampled (action, observation) trajectories do not depend on the arithmetic: belief counts must be equal.
    assert hist.beliefs_counts == list(z['beliefs'])
    # |V| follows the reference exactly for the first 29 backups; from then on single alpha rows may differ where the
    # reference's argmax is decided by rounding noise between exactly tied candidates.
    # (The forks are decided by the summation order of one GEMM: with a debug switch that sends the early backups through
    # another kernel -- the pure fp64 GEMM with its K split, the belief-side formulation -- the first one comes earlier.)
    got, want = np.array(hist.alpha_vector_counts), z['alphas']
    strict = 25 if DEFAULT_PIPELINE else 9
    assert np.array_equal(got[:strict], want[:strict])
    assert np.all(np.abs(got - want) <= (np.maximum(2, want // 100) if DEFAULT_PIPELINE else np.maximum(3, want // 50)))
    np.testing.assert_allclose(hist.value_function_changes[:strict - 1], z['changes'][:strict - 1], rtol=1e-9, atol=1e-12)
    alpha = np.asarray(vf.alpha_vector_array, dtype=np.float64)
    v_b0 = float(np.max(alpha @ np.asarray(model.start_probabilities)))
    # On the reference's trajectory the value of the start belief is the reference's; a run that forked at one of those
    # ties is a different, equally valid PBVI run whose value function differs by what the fork found or missed (a
    # one-ulp change of a belief's normaliser is enough to pick the other branch late in the run).
    # (The default pipeline reproduces the reference's value to the last digit although its |V| is off by one row from
    # backup 29 on; with every backup forced into the belief-side formulation -- the debug mode the suite is also run
    # in -- the run forks at backup 31 and ends 3 % lower.)
    assert abs(v_b0 - float(z['value_b0'])) <= (1e-9 if DEFAULT_PIPELINE else 0.1) * abs(float(z['value_b0']))
    print(f'end to end: |V|={len(vf)} backup mean {np.mean(hist.backup_times) * 1e3:.2f} ms '
          f'(reference on the fixture machine: {float(z["ref_backup_mean_s"]):.2f} s)')


def test_value_function_prune_level2_on_gpu_objects():
    """ValueFunction.prune(2) with the set on the GPU works on the AlphaVector objects (kept vectors keep their
    device rows) and keeps exactly what the host loop of src/mdp.py:857-866 keeps."""
    rng = np.random.default_rng(8)
    model, _ = load_POMDP_file(os.path.join(GOLDEN, 'models', '4x3.95-no_loop_2_grid.POMDP'))
    base = rng.normal(size=(30, model.state_count))
    rows = np.concatenate([base, base[:10] - rng.random((10, model.state_count)), base[5:8]])   # dominated + duplicates
    acts = rng.integers(0, model.action_count, size=len(rows))
    host = ValueFunction(model, rows.copy(), acts)
    host.prune(2)
    gm = model.to_gpu('f64')
    dev = ValueFunction(gm, rows.copy(), acts)
    n_before = len(dev)
    dev.prune(2)
    assert len(dev) == len(host) < n_before
    assert np.array_equal(dev.alpha_vector_array, host.alpha_vector_array)
    assert np.array_equal(dev.actions, host.actions)
    dev.prune(2)                                          # already at that level: unchanged
    assert len(dev) == len(host)


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_rows_rebuilt_from_keys_are_the_rows_of_the_backup(dtype):
    """pbvi_backup_fetch_unique_keys + pbvi_assemble_rows (what ranks exchange instead of rows): keys are
    (a*, v*[a*, :]) of each distinct row, and assembling them against the resident alpha set gives the same bytes."""
    z = load_npz('olfactory_small_R5.npz')
    rs, rto, er = z['reachable_states'], z['rto'].astype(np.float64), z['expected_rewards'].astype(np.float64)
    alpha, b = z['alpha'].astype(np.float64), z['beliefs'].astype(np.float64)
    gamma = float(z['gamma'])
    eng = Engine(rto.shape[0], rto.shape[1], rto.shape[2], rto.shape[3], rs, rto, er, dtype=dtype)
    eng.set_alpha(alpha)
    eng.set_beliefs(b)
    eng.run(gamma)
    res = eng.fetch()
    keys = eng.fetch_unique_keys()
    assert keys.shape == (res.unique_alpha.shape[0], 1 + rto.shape[2])
    first = np.array([np.flatnonzero(res.index == u)[0] for u in range(len(keys))])
    assert np.array_equal(keys[:, 0], res.actions[first])
    assert np.array_equal(keys[:, 1:], res.best_alpha_ind[first, res.actions[first], :])
    rebuilt = eng.assemble_rows(keys[::-1], gamma)            # any order, any subset
    assert np.array_equal(rebuilt, res.unique_alpha[::-1])
    # the packed exchange message holds the same pieces: [U | index | actions | keep | keys padded to B rows]
    B, U, kw = len(b), len(keys), keys.shape[1]
    packed = np.full(1 + 3 * B + B * kw, -7, dtype=np.int32)
    eng.fetch_exchange_into(packed.ctypes.data)
    assert packed[0] == U
    assert np.array_equal(packed[1:1 + B], res.index) and np.array_equal(packed[1 + B:1 + 2 * B], res.actions)
    assert np.array_equal(packed[1 + 2 * B:1 + 3 * B], res.keep.astype(np.int32))
    body = packed[1 + 3 * B:].reshape(B, kw)
    assert np.array_equal(body[:U], keys) and not body[U:].any()
    with pytest.raises(ValueError):
        bad = keys.copy()
        bad[0, 1] = alpha.shape[0] + 5
        eng.assemble_rows(bad, gamma)
    eng.close()


def test_rccl_exchange_single_rank_matches_direct_fetch():
    """The multi-GPU step of bench.py --gpus N (EngineShard.run_resident_packed -> one all_gather_into_tensor of the
    packed integers -> rows rebuilt from the keys with pbvi_assemble_rows on device tensors) through a real RCCL
    process group of one rank: the rebuilt rows, index, actions and keep equal what the engine returns directly.
    Runs in a child process, torch first: torch brings its own HIP runtime, which has to be the one that opens the
    device (bench.py imports in the same order)."""
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'rccl_single_rank_check.py')
    out = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert 'rccl single-rank exchange ok' in out.stdout


def test_sharded_backup_on_the_engine_two_ranks():
    """SURVEY 8e as a product path: two ranks (one HIP engine each, sharing this box's GPU, gloo carrying the exchange)
    run ``FSVI_Solver.solve(use_gpu=True)`` and direct ``PBVI_Solver.backup`` calls; the beliefs are sharded by the solver
    itself, every replica appends the same rows, and the results equal the single-process engine's / the reference's
    seeded trajectory.  (tests/dist_engine_check.py holds the ranks' code.)"""
    import socket
    import subprocess
    import sys
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dist_engine_check.py')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                          '--master-addr', '127.0.0.1', '--master-port', str(port), script],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-6000:]
    assert 'sharded engine backup ok' in out.stdout


def _c5_fixture():
    path = os.path.join(GOLDEN, 'olfactory_c5_B8192.npz')
    if not os.path.exists(path):
        pytest.skip('C5 fixture missing (make_golden.py c5)')
    return np.load(path, allow_pickle=False)


def test_c5_8192_beliefs_on_one_engine_against_reference():
    """BASELINE config 5's workload (|S|=30000, V=1024, B=8192) on ONE engine -- the strong-scaling baseline of
    ``bench.py --scaling strong --beliefs-total 8192`` -- against the reference's outputs for all 8192 beliefs
    (olfactory_c5_B8192.npz: the reference run in 8 blocks of 1024, make_golden.py c5)."""
    z = _c5_fixture()
    B, V = int(z['B']), int(z['V'])
    m = synth.olfactory_model(R=1)
    alpha, _ = synth.alpha_set(m, V)
    beliefs = synth.belief_points(m, B)
    import hashlib
    h = hashlib.sha256()
    for a in (m.reachable_states, m.rto, m.expected_rewards, alpha, beliefs):
        h.update(np.ascontiguousarray(a).tobytes())
    if h.hexdigest() != str(z['inputs_sha256']):
        pytest.skip('host regenerated different input bits than the fixture machine (exp/libm); parity unpinned here')
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f32')
    res = eng.backup_full(alpha, beliefs, m.gamma)
    mism = int(np.sum(res.best_alpha_ind != z['core_best']))
    assert mism == 0, f'{mism} of {res.best_alpha_ind.size} best_alpha_ind differ'
    assert np.array_equal(res.actions, z['core_actions'])
    u64 = res.unique_alpha.astype(np.float64)
    np.testing.assert_allclose(u64.sum(axis=1)[res.index], z['row_sum'], rtol=F32_RTOL)
    np.testing.assert_allclose(u64[res.index[z['sample_b']], z['sample_s']], z['sample_val'], rtol=F32_RTOL, atol=1e-12)
    assert len(orc.dedup_rows(*res.value_function_rows())[1]) == int(z['n_unique'])
    val, _ = eng.max_value_resident()
    np.testing.assert_allclose(val, z['value_max'], rtol=1e-12)
    print(f"C5 on one engine: {res.stats['ms_total']:.2f} ms for {B} beliefs, {res.stats['n_unique']} distinct keys")
    eng.close()


def test_c5_sharded_over_two_ranks_against_reference():
    """The same workload sharded: two ranks of 4096 beliefs, one HIP engine each, the product step of the multi-GPU path
    (local backup, one all-gather of integers, global dedup, append to every replica's alpha store), merged result against
    the reference's outputs for all 8192 beliefs.  (tests/dist_c5_check.py holds the ranks' code.)"""
    _c5_fixture()
    import socket
    import subprocess
    import sys
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dist_c5_check.py')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2',
                          '--master-addr', '127.0.0.1', '--master-port', str(port), script],
                         capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-6000:]
    assert 'c5 sharded ok' in out.stdout


def test_memory_error_contract_of_solve_and_engine_recovery(capsys):
    """``src/pomdp.py:2399-2401``: an out-of-memory inside the solve loop ends the loop and returns the value function and
    history "as is".  A cap on the engine's device bytes (``pbvi_debug_alloc_limit``) makes the allocation failure
    deterministic: the C-ABI returns -2, the seam raises ``MemoryError``, ``solve`` prints the reference's message and returns
    the partial result -- the seeded host solve cut at the same backup -- and the engine, returned to its freshly created
    state (``pbvi_engine_after_oom``), serves the next call."""
    import random
    from pomdp_pbvi_exploration_amd import FSVI_Solver
    from pomdp_pbvi_exploration_amd.engine import debug_alloc_limit
    from test_policy_eval import mirror_model
    m = synth.olfactory_model(H=30, W=80, R=1, f32=False)
    model = mirror_model(m)

    def run(expansions, use_gpu):
        np.random.seed(3)
        random.seed(3)
        return FSVI_Solver(gamma=m.gamma, eps=1e-6).solve(model, expansions=expansions, max_belief_growth=40, use_gpu=use_gpu,
                                                          print_progress=False)
    run(2, True)                                            # engine created, first buffers allocated
    eng = model.gpu_model.engine
    held = eng.device_bytes
    prev = debug_alloc_limit(held // (1 << 20) + 24)        # 24 MiB of head room: the row stores outgrow it within a dozen expansions
    try:
        capsys.readouterr()
        vf, hist = run(80, True)
        out = capsys.readouterr().out
    finally:
        debug_alloc_limit(prev)
    n_done = len(hist.backup_times)
    assert 'Memory full' in out and 'Returning value function and history as is' in out
    assert 0 < n_done < 80 and len(vf) > 0, n_done
    # the partial result is the seeded run cut where the memory ran out (host solve of as many expansions)
    want_vf, want_hist = run(n_done, False)
    assert hist.alpha_vector_counts[:n_done + 1] == want_hist.alpha_vector_counts[:n_done + 1]
    if len(vf) != len(want_vf):
        # the backup itself got through (in belief chunks, test_backup_that_does_not_fit_is_done_in_belief_chunks) and the
        # memory ran out right behind it, in compute_change: "as is" then holds that backup's rows, like the reference's loop
        want_vf, _ = run(n_done + 1, False)
    np.testing.assert_allclose(np.asarray(vf.alpha_vector_array, dtype=np.float64), want_vf.alpha_vector_array, rtol=1e-9, atol=1e-12)
    # the engine is usable again: a direct backup on GPU objects equals the host's
    gm = model.gpu_model
    rows = synth.belief_points(m, 20, max_depth=10)
    host_vf = ValueFunction(model, want_vf.alpha_vector_array, want_vf.actions)
    got = PBVI_Solver(gamma=m.gamma).backup(gm, BeliefSet(gm, [Belief(gm, r) for r in rows]), host_vf.to_gpu() if hasattr(host_vf, 'to_gpu') else host_vf,
                                           belief_dominance_prune=False)
    ref = PBVI_Solver(gamma=m.gamma).backup(model, BeliefSet(model, [Belief(model, r) for r in rows]), host_vf, belief_dominance_prune=False)
    assert np.array_equal(got.actions, ref.actions)
    np.testing.assert_allclose(np.asarray(got.alpha_vector_array, dtype=np.float64), ref.alpha_vector_array, rtol=1e-9, atol=1e-12)


def test_engine_call_over_the_allocation_cap_raises_memory_error_and_recovers():
    from pomdp_pbvi_exploration_amd.engine import debug_alloc_limit
    z, rs, rto, er = small(1)
    eng = Engine(600, 6, 3, 1, rs, rto, er, dtype='f32')
    want = eng.backup_full(z['alpha'], z['beliefs'], float(z['gamma']))
    big = np.tile(z['alpha'], (400, 1))                     # 19200 alpha rows: ~46 MB, Gamma ~0.8 GB
    prev = debug_alloc_limit(eng.device_bytes // (1 << 20) + 64)
    try:
        with pytest.raises(MemoryError):
            eng.backup_full(big, z['beliefs'], float(z['gamma']))
        assert eng.alpha_count == 0                       # back to the freshly created state
        again = eng.backup_full(z['alpha'], z['beliefs'], float(z['gamma']))
    finally:
        debug_alloc_limit(prev)
    assert np.array_equal(again.best_alpha_ind, want.best_alpha_ind) and np.array_equal(again.alpha, want.alpha)
    eng.close()


def test_f64_screen_steps_aside_when_alpha_leaves_the_fp32_range():
    """An fp64 engine's fp32 screen narrows the alpha set; a value beyond FLT_MAX would become inf there and the screen's
    scores NaN.  The narrowing kernel flags it and the backup is decided by the fp64 pipeline alone."""
    z, rs, rto, er = small(1)
    alpha = z['alpha'].astype(np.float64).copy()
    alpha[3] *= 1e36                                         # finite in fp64, inf in fp32
    alpha[7] *= -1e36
    want_rows, want_a, want_v = orc.backup_core(alpha, z['beliefs'].astype(np.float64), rs, rto, er, float(z['gamma']))
    eng = Engine(600, 6, 3, 1, rs, rto, er, dtype='f64')
    eng.set_f64_screen('always')
    res = eng.backup_full(alpha, z['beliefs'], float(z['gamma']))
    assert np.array_equal(res.best_alpha_ind, want_v) and np.array_equal(res.actions, want_a)
    np.testing.assert_allclose(res.alpha, want_rows, rtol=1e-12)
    ok = eng.backup_full(z['alpha'].astype(np.float64), z['beliefs'], float(z['gamma']))       # a representable set: screened again
    assert ok.stats['screened'] == 1 and np.array_equal(ok.best_alpha_ind, z['core_best'])
    eng.close()


def test_pinned_buffer_outlives_its_arrays():
    import gc
    from pomdp_pbvi_exploration_amd.engine import PinnedBuffer
    buf = PinnedBuffer(1 << 16)
    a = buf.carve((16, 16), np.float32)
    view = a[2:]
    with pytest.raises(RuntimeError):
        buf.close()                                          # arrays carved from it are alive
    del a
    gc.collect()
    with pytest.raises(RuntimeError):
        buf.close()                                          # ... and so is a view of one
    view[:] = 1.0                                            # still valid memory
    del view
    gc.collect()
    buf.close()


def test_fused_engine_holds_only_the_projected_tiles_of_gamma():
    """With the projection fused into the score GEMM only the Gamma tiles that are still projected exist in memory (the tail
    tile and tiles that straddle two groups): at V a multiple of 256 that is ONE 256-row tile instead of A*O*V rows -- the
    buffer the reference's CuPy path could not allocate (Sea_Robin_Real.ipynb:913).  Switching the same engine to the
    projected pipeline allocates the full buffer; results are the same bits."""
    rng = np.random.default_rng(3)
    S, A, O, V, B = 30000, 2, 2, 1024, 300
    rs = ((np.arange(S)[:, None] + np.array([1, -400])[None, :]) % S)[:, :, None].astype(np.int64)
    p = rng.random((S, A, O))
    rto = (p / p.sum(axis=2, keepdims=True))[:, :, :, None].astype(np.float32).astype(np.float64)
    er = rng.normal(size=(S, A)).astype(np.float32).astype(np.float64)
    alpha = rng.normal(size=(V, S)).astype(np.float32).astype(np.float64)
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.1)
    b[:, 5] += 1e-3
    b = (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    fused = eng.backup_full(alpha, b, 0.9)
    held_fused = eng.device_bytes
    eng.set_fused_projection(False)
    plain = eng.backup_full(alpha, b, 0.9)
    held_plain = eng.device_bytes
    if FUSION_ALLOWED and os.environ.get('PBVI_NO_COMPACT_GAMMA') is None:
        assert fused.stats['fused_projection'] == 1
        gamma_rows = A * O * (V + 1) + 2 * A
        full = (gamma_rows + 255) // 256 * 256 * 30016 * 4
        assert held_plain - held_fused > 0.9 * (full - 256 * 30016 * 4), (held_fused, held_plain, full)
    assert np.array_equal(fused.best_alpha_ind, plain.best_alpha_ind) and np.array_equal(fused.alpha, plain.alpha)
    eng.close()


@pytest.mark.parametrize('case', ['olfactory_f32', 'olfactory_f64', 'ties_f32', 'prune_f32'])
def test_run_fetch_with_early_rows_equals_run_then_fetch(case):
    """``pbvi_backup_run_fetch``: the rows of the provisional decision (first maxima of the fp32 scores) leave for the host
    while the refinement runs; final keys are matched against them and only changed rows are appended.  Whatever the
    refinement overturns, the result read through ``slot`` is the plain ``run`` + ``fetch_compact`` result bit for bit:
    the small olfactory fixture (fp32 and screened fp64), an alpha set of near-duplicates in which the refinement
    overturns many first maxima, and the belief-dominance call (where the early path steps aside)."""
    from pomdp_pbvi_exploration_amd.engine import PinnedBuffer
    z, rs, rto, er = small(1)
    S, A, O = 600, 6, 3
    dtype = 'f64' if case.endswith('f64') else 'f32'
    alpha, beliefs = z['alpha'].astype(np.float64), np.tile(z['beliefs'].astype(np.float64), (5, 1))      # 320 beliefs: sorted blocks
    if case == 'ties_f32':
        rng = np.random.default_rng(4)
        base = alpha[:6]
        alpha = (np.repeat(base, 40, axis=0) * (1.0 + 3e-7 * rng.standard_normal((240, 1)))).astype(np.float32).astype(np.float64)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype=dtype)
    if dtype == 'f64':
        eng.set_f64_screen('always')
    eng.set_formulation('alpha')
    eng.set_alpha(alpha)
    eng.set_beliefs(beliefs)
    B = beliefs.shape[0]
    prune = case == 'prune_f32'
    st = eng.run(float(z['gamma']), prune)
    want = eng.fetch()
    item = 4 if dtype == 'f32' else 8
    buf = PinnedBuffer(B * S * item + 4 * B * 4 + B * A * O * 4 + B + 8192)
    rows = buf.carve((B, S), eng.np_dtype)
    slot, index, actions = (buf.carve((B,), np.int32) for _ in range(3))
    best = buf.carve((B, A, O), np.int32)
    keep = buf.carve((B,), np.uint8)
    for _ in range(2):                                       # twice: the second call re-uses every buffer of the first
        rows[:] = np.nan
        st2, U, used = eng.run_fetch_into(float(z['gamma']), rows, slot, index, actions, best=best, keep=keep,
                                          belief_dominance_prune=prune)
        assert U == want.unique_alpha.shape[0] and used >= U
        assert np.array_equal(index, want.index) and np.array_equal(actions, want.actions)
        assert np.array_equal(best, want.best_alpha_ind) and np.array_equal(keep.astype(bool), want.keep.astype(bool))
        assert np.all((slot[:U] >= 0) & (slot[:U] < used)) and len(set(slot[:U].tolist())) == U
        assert np.array_equal(np.asarray(rows)[slot[:U]], want.unique_alpha)
        assert st2['n_refined'] == st['n_refined']
    if case == 'ties_f32':
        assert st['n_refined'] > 100                         # the refinement had work: keys were overturned
    del rows, slot, index, actions, best, keep
    buf.close()
    eng.close()


def test_backup_that_does_not_fit_is_done_in_belief_chunks():
    """Where the reference's CuPy path dies (``Sea_Robin_Real.ipynb:913``: Gamma[A,O,V,S] does not fit), the seam finishes the
    backup: (a) a block whose working set does not fit (``MemoryError`` from the engine) is backed up in belief chunks,
    halved until one fits; (b) left to choose, the engine takes the belief-side formulation by itself when Gamma alone
    exceeds what it may still allocate, whatever its cost model says.  Same rows and actions as the uncapped backup."""
    from pomdp_pbvi_exploration_amd import PBVI_Solver, ValueFunction, BeliefSet
    from pomdp_pbvi_exploration_amd.engine import debug_alloc_limit
    from test_policy_eval import mirror_model
    m = synth.olfactory_model(H=30, W=80, R=5, f32=False)            # R = 5: Gamma is held whole on the alpha side
    gm = mirror_model(m).to_gpu(dtype='f32')                         # one engine, one cap (an fp64 engine and its screen have one each)
    rng = np.random.default_rng(11)
    V, B = 6000, 256
    vf = ValueFunction(gm, rng.standard_normal((V, m.S)), rng.integers(0, m.A, V))
    bs = BeliefSet(gm, synth.belief_points(m, B).astype(np.float64))
    solver = PBVI_Solver(gamma=m.gamma, eps=1e-6)
    eng = gm.engine

    def key(res):
        arr, a = np.asarray(res.alpha_vector_array), np.asarray(res.actions)
        order = np.lexsort(arr.T[::-1])
        return arr[order], a[order]

    # measured: the alpha side holds 2.2 GB here (Gamma 1.0 GB = 18 x 6001 rows x 2432 x 4 B, row stores, work lists, score
    # slabs), the belief side 1.2 GB for the block and 0.9 GB for half of it
    prev = debug_alloc_limit(eng.device_bytes // (1 << 20) + 1600)
    try:
        eng.set_formulation('alpha')
        got_a = solver.backup(gm, bs, vf, belief_dominance_prune=False)
        chunk = solver._belief_chunk
        assert eng.formulation == 'alpha'                            # the caller's setting is back
        eng.set_formulation('auto')
        solver._belief_chunk = None
        got_b = solver.backup(gm, bs, vf, belief_dominance_prune=False)
        assert solver._belief_chunk is None and eng.last_stats['formulation'] == 2
    finally:
        debug_alloc_limit(prev)
    assert chunk == B // 2, chunk
    eng.set_formulation('alpha')
    want = solver.backup(gm, bs, vf, belief_dominance_prune=False)   # uncapped, the reference's order
    assert eng.last_stats['formulation'] == 1 and solver._belief_chunk is None
    eng.set_formulation('auto')
    rw, aw = key(want)
    for got in (got_a, got_b):
        rg, ag = key(got)
        assert rw.shape == rg.shape and np.array_equal(aw, ag)
        np.testing.assert_allclose(rg, rw, rtol=1e-6, atol=0)


@pytest.mark.parametrize('q2_cap', [None, 3])
def test_duplicate_rows_through_the_level1_screen_and_the_split_rescoring(q2_cap, monkeypatch):
    """An alpha set in which every row has a twin (and some a triplet): on an fp32 engine with projected rows in HBM (R = 5)
    the level-1 screen of the refinement cannot separate the twins, so every queued entry goes to ``k_refine_split`` -- or,
    with room for only 3 entries in the hand-over, most of them stay with the entry's own block.  Either way the first of
    the tied rows wins, as in the reference (np.argmax)."""
    if q2_cap is not None:
        monkeypatch.setenv('PBVI_REFINE_Q2_CAP', str(q2_cap))
    z, rs, rto, er = small(5)
    S, A, Rr = rs.shape
    base = z['alpha'].astype(np.float32)
    alpha = np.concatenate([base, base, base[:7]]).astype(np.float64)          # row v, its twin at v + V, triplets for v < 7
    b = z['beliefs'].astype(np.float64)
    gamma = float(z['gamma'])
    want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, gamma)
    assert want_v.max() < len(base)                                           # the reference picks the first of the tied rows
    eng = Engine(S, A, rto.shape[2], Rr, rs, rto, er, dtype='f32')
    res = eng.backup_full(alpha.astype(np.float32), b.astype(np.float32), gamma)
    assert np.array_equal(res.best_alpha_ind, want_v) and np.array_equal(res.actions, want_a)
    np.testing.assert_allclose(res.alpha, want_rows, rtol=1e-6, atol=1e-7)
    assert res.stats['n_refined'] > 0
    eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_random_models_against_the_oracle(dtype):
    """60 random models / shapes per engine type (1750 more were run once by hand in five engine modes): indices, actions and
    rows against the oracle.  Between EXACT duplicates of an alpha row the engine returns the first (the tied scores are
    equal in exact arithmetic); NumPy's BLAS may round the later column's dot product one ulp higher and pick that one --
    the reference never holds duplicates (``ValueFunction`` drops them), so such entries are compared by row content."""
    for seed in range(60):
        S, A, O, R, rs, rto, er, alpha, b, gamma = _random_case(seed)
        if dtype == 'f32':
            alpha, b = alpha.astype(np.float32).astype(np.float64), b.astype(np.float32).astype(np.float64)
            rto, er = rto.astype(np.float32).astype(np.float64), er.astype(np.float32).astype(np.float64)
        want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, gamma)
        eng = Engine(S, A, O, R, rs, rto, er, dtype=dtype)
        cast = (lambda x: x) if dtype == 'f64' else (lambda x: x.astype(np.float32))
        res = eng.backup_full(cast(alpha), cast(b), gamma)
        eng.close()
        assert_backup_matches_oracle(res, alpha, want_rows, want_a, want_v, dtype, seed)
