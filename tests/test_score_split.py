"""The backup's score GEMM on bf16 MFMAs with a three-term operand split (gemm.hip, scheduler 2d; pbvi_set_score_split):
the scores change by at most the split's error bound, the tie window widens by that bound, and every output -- indices,
actions, keep flags, alpha' bytes -- is the fp32 GEMM's and the oracle's."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from oracle import pbvi_oracle as orc
from pomdp_pbvi_exploration_amd import synth
from pomdp_pbvi_exploration_amd.engine import Engine
from score_cases import random_model

pytestmark = pytest.mark.gpu

FUSION_ALLOWED = os.environ.get('PBVI_NO_FUSED_PROJECT') is None
F32_RTOL = 2e-5


def beliefs(rng, B, S, density=0.2):
    b = rng.random((B, S)) * (rng.random((B, S)) < density)
    b[:, rng.integers(0, S, size=B)] += 1e-3
    return (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)


def run_modes(eng, alpha, b, gamma, modes=('always', 'off')):
    out = {}
    for mode in modes:
        eng.set_score_split(mode)
        out[mode] = eng.backup_full(alpha, b, gamma, belief_dominance_prune=True)
    return out


def check_same(out, want, keep_ref=None):
    want_rows, want_a, want_v = want
    for mode, res in out.items():
        assert np.array_equal(res.best_alpha_ind, want_v), (mode, int(np.sum(res.best_alpha_ind != want_v)))
        assert np.array_equal(res.actions, want_a), mode
        np.testing.assert_allclose(res.alpha.astype(np.float64), want_rows, rtol=F32_RTOL, atol=1e-9)
        if keep_ref is not None:
            assert np.array_equal(res.keep, keep_ref), mode
    s, f = out['always'], out['off']
    assert s.stats['score_split'] == 1 and f.stats['score_split'] == 0
    assert np.array_equal(s.alpha, f.alpha) and np.array_equal(s.keep, f.keep)


@pytest.mark.parametrize('S,A,O,V,B,regular', [(1000, 2, 2, 300, 70, False), (4097, 3, 1, 513, 300, True),
                                                (2500, 1, 3, 777, 40, False)])
def test_split_equals_fp32_on_random_models(S, A, O, V, B, regular):
    """Mixed-sign alpha with an exact duplicate row (the lowest index wins), V not a multiple of 256."""
    rng = np.random.default_rng(S + V)
    rs, rto, er = random_model(rng, S, A, O, regular)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    alpha[5] = alpha[2]
    b = beliefs(rng, B, S)
    want = orc.backup_core(alpha, b, rs, rto, er, 0.9)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    out = run_modes(eng, alpha, b, 0.9)
    keep = orc.belief_dominance_mask(alpha, b, np.asarray(out['off'].alpha, dtype=np.float64))
    check_same(out, want, keep)
    eng.close()


def test_near_ties_inside_the_split_window():
    """alpha rows 1e-5 .. 1e-4 apart (relative): inside the split's window, outside the fp32 one -- the refinement decides."""
    rng = np.random.default_rng(7)
    S, A, O, V, B = 3000, 2, 2, 96, 128
    rs, rto, er = random_model(rng, S, A, O, True)
    base = rng.random(S) * 10.0 + 1.0
    alpha = np.empty((V, S))
    for v in range(V):
        eps = 10.0 ** -(4 + (v % 2))                         # 1e-4, 1e-5
        alpha[v] = base * (1.0 + eps * rng.standard_normal(S))
    alpha[9] = alpha[4]
    alpha = alpha.astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S, 0.05)
    want = orc.backup_core(alpha, b, rs, rto, er, 0.95)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    out = run_modes(eng, alpha, b, 0.95)
    check_same(out, want)
    assert out['always'].stats['n_refined'] >= out['off'].stats['n_refined']
    eng.close()


def test_beliefs_below_the_normal_range():
    """Beliefs whose whole mass lies near the bottom of the fp32 range (entries ~2^-141 .. 2^-123): their lo parts are bf16
    subnormals and many hi parts and products are subnormal too, so these parts carry ~2^-8 of every score.  Were they
    flushed anywhere on the split path, scores would move by far more than the window and argmaxes would flip; the fp32
    path's own rounding there stays ~2^-30 relative."""
    rng = np.random.default_rng(11)
    S, A, O, V, B = 1500, 2, 2, 200, 64
    rs, rto, er = random_model(rng, S, A, O, False)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S, 0.3)
    b[B // 2:] *= 2.0 ** -116                                 # half the block: all of its mass tiny
    b = b.astype(np.float32).astype(np.float64)
    tiny = b[B // 2:][b[B // 2:] > 0]
    assert tiny.max() < 2.0 ** -118 and np.mean(tiny < 2.0 ** -126) > 0.1      # lo parts subnormal; some entries too
    want = orc.backup_core(alpha, b, rs, rto, er, 0.9)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    out = run_modes(eng, alpha, b, 0.9)
    check_same(out, want)
    eng.close()


@pytest.mark.parametrize('S,A,O,V,B,regular', [(1000, 2, 2, 512, 70, False), (4097, 3, 1, 300, 300, True),
                                                (30000, 2, 2, 256, 260, True)])
def test_split_fused_and_projected_routes_agree_bit_for_bit(S, A, O, V, B, regular):
    """Forced split: Gamma generated in the operand staging vs read from the projected rows -- the same LDS image, the same
    MFMAs, so outputs and refinement statistics are identical."""
    rng = np.random.default_rng(S + V)
    rs, rto, er = random_model(rng, S, A, O, regular)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S)
    want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, 0.9)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_score_split('always')
    out = {}
    for fused in (True, False):
        eng.set_fused_projection(fused)
        res = eng.backup_full(alpha, b, 0.9, belief_dominance_prune=True)
        assert res.stats['fused_projection'] == int(fused and FUSION_ALLOWED)
        assert res.stats['score_split'] == 1
        assert np.array_equal(res.best_alpha_ind, want_v) and np.array_equal(res.actions, want_a), fused
        out[fused] = res
    f, u = out[True], out[False]
    assert np.array_equal(f.alpha, u.alpha) and np.array_equal(f.keep, u.keep)
    for k in ('n_refined', 'n_refine_candidates', 'n_refined_actions', 'n_dead', 'n_unique', 'score_tiles_run'):
        assert f.stats[k] == u.stats[k], k
    eng.close()


@pytest.mark.parametrize('tag', ['1', '5_1024'])
def test_full_size_fixtures_with_the_split_forced(tag):
    path = os.path.join(GOLDEN, f'olfactory_full_R{tag}.npz')
    if not os.path.exists(path):
        pytest.skip('full-size fixture missing')
    z = np.load(path, allow_pickle=False)
    m = synth.olfactory_model(R=int(z['R']))
    alpha, _ = synth.alpha_set(m, int(z['V']))
    b = synth.belief_points(m, int(z['B']))
    if synth.checksum(m.reachable_states, m.rto, m.expected_rewards, alpha, b) != str(z['inputs_sha256']):
        pytest.skip('host regenerated different input bits than the fixture machine (exp/libm); parity unpinned here')
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f32')
    eng.set_score_split('always')
    res = eng.backup_full(alpha, b, m.gamma)
    assert res.stats['score_split'] == 1                                   # (R > 1: through the projected route)
    assert int(np.sum(res.best_alpha_ind != z['core_best'])) == 0
    assert np.array_equal(res.actions, z['core_actions'])
    eng.close()


def test_alpha_near_the_top_of_the_range():
    """Gamma entries within 0.4 % of FLT_MAX, above the largest finite bf16: hi saturates there instead of rounding to inf
    (gamma = 1, one observation, so Gamma = alpha), and the results stay the oracle's.  One-hot beliefs keep every score
    finite."""
    rng = np.random.default_rng(3)
    S, A, O, V, B = 700, 2, 1, 40, 30
    rs, rto, er = random_model(rng, S, A, O, True)
    fmax = float(np.finfo(np.float32).max)
    alpha = (1.0 - rng.random((V, S)) * 0.003) * fmax
    alpha[:, ::2] *= -1.0
    alpha = alpha.astype(np.float32).astype(np.float64)
    b = np.zeros((B, S))
    b[np.arange(B), rng.integers(0, S, size=B)] = 1.0
    want = orc.backup_core(alpha, b, rs, rto, er, 1.0)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    out = run_modes(eng, alpha, b, 1.0)
    for res in out.values():
        assert np.array_equal(res.best_alpha_ind, want[2]) and np.array_equal(res.actions, want[1])
    assert out['always'].stats['score_split'] == 1
    assert np.array_equal(out['always'].alpha, out['off'].alpha)
    eng.close()


def test_tie_window_override_switches_the_split_off():
    rng = np.random.default_rng(5)
    S, A, O, V, B = 1000, 2, 2, 64, 32
    rs, rto, er = random_model(rng, S, A, O, True)
    alpha = rng.normal(size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_score_split('always')
    assert eng.backup_full(alpha, b, 0.9).stats['score_split'] == 1
    eng.set_tie_window(1e-3)
    assert eng.backup_full(alpha, b, 0.9).stats['score_split'] == 0
    eng.set_tie_window(-1.0)
    assert eng.backup_full(alpha, b, 0.9).stats['score_split'] == 1
    eng.set_score_split('off')
    assert eng.backup_full(alpha, b, 0.9).stats['score_split'] == 0
    eng.close()
