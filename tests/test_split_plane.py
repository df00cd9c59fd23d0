"""The split score GEMM reads the belief block from its pre-split plane (split_bf16.h), written by the block's gather or
rebuilt before the GEMM when it is stale.  Whatever path put the block in place, the outputs must equal the oracle's and
the fp32 GEMM's (PBVI_SCORE_SPLIT off) byte for byte."""
import numpy as np
import pytest

from oracle import pbvi_oracle as orc
from pomdp_pbvi_exploration_amd.engine import Engine

pytestmark = pytest.mark.gpu

F32_RTOL = 2e-5


def model(rng, S, A, O, R=1):
    rs = ((np.arange(S)[:, None, None] + rng.integers(-5, 6, size=(1, A, R))) % S).astype(np.int64)
    p = rng.random((S, A, O, R))
    p[rng.random((S, A, O, R)) < 0.3] = 0.0
    p[:, :, 0, 0] += 1e-3
    rto = (p / p.sum(axis=(2, 3), keepdims=True)).astype(np.float32).astype(np.float64)
    er = rng.normal(size=(S, A)).astype(np.float32).astype(np.float64)
    return rs, rto, er


def beliefs(rng, B, S, density=0.2):
    b = rng.random((B, S)) * (rng.random((B, S)) < density)
    b[:, rng.integers(0, S, size=B)] += 1e-3
    return (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)


def run(eng, mode, gamma=0.9):
    eng.set_score_split(mode)
    stats = eng.run(gamma, belief_dominance_prune=True)
    res = eng.fetch()
    res.stats = stats
    return res


def check(eng, want, gamma=0.9):
    """A split run on the resident block: the split is taken and matches the oracle and the fp32 GEMM."""
    s = run(eng, 'always', gamma)
    f = run(eng, 'off', gamma)
    assert s.stats['score_split'] == 1 and f.stats['score_split'] == 0
    rows, act, v = want
    assert np.array_equal(s.best_alpha_ind, v) and np.array_equal(s.actions, act)
    np.testing.assert_allclose(s.alpha.astype(np.float64), rows, rtol=F32_RTOL, atol=1e-9)
    assert np.array_equal(s.alpha, f.alpha) and np.array_equal(s.keep, f.keep)
    assert np.array_equal(s.best_alpha_ind, f.best_alpha_ind) and np.array_equal(s.actions, f.actions)
    return s


def test_reselected_blocks_and_a_stale_plane():
    """Blocks from the belief store, backed up in turn and re-selected; one block is put in place while the split is off
    (the gather writes no plane), so the next split run must rebuild it."""
    rng = np.random.default_rng(11)
    S, A, O, V = 3000, 2, 2, 400
    rs, rto, er = model(rng, S, A, O)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b1, b2 = beliefs(rng, 300, S), beliefs(rng, 520, S, density=0.05)
    w1 = orc.backup_core(alpha, b1, rs, rto, er, 0.9)
    w2 = orc.backup_core(alpha, b2, rs, rto, er, 0.9)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_alpha(alpha)
    id1 = eng.store_rows('belief', b1)
    id2 = eng.store_rows('belief', b2)
    ids1, ids2 = np.arange(id1, id1 + len(b1)), np.arange(id2, id2 + len(b2))
    eng.set_score_split('always')
    eng.select_beliefs(ids1)
    check(eng, w1)
    eng.select_beliefs(ids2)
    check(eng, w2)
    eng.select_beliefs(ids1)
    check(eng, w1)
    eng.set_score_split('off')
    eng.select_beliefs(ids2)                          # no plane written for this block
    check(eng, w2)
    eng.set_score_split('always')
    eng.select_beliefs(ids1)
    check(eng, w1)
    eng.close()


def test_set_beliefs_blocks_of_odd_sizes():
    """pbvi_beliefs_set blocks of 1, 255, 257 and 700 rows (padding rows of the plane are zero) after a larger block."""
    rng = np.random.default_rng(12)
    S, A, O, V = 2500, 3, 2, 300
    rs, rto, er = model(rng, S, A, O)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_alpha(alpha)
    for B in (700, 1, 255, 257):
        b = beliefs(rng, B, S)
        eng.set_beliefs(b)
        check(eng, orc.backup_core(alpha, b, rs, rto, er, 0.9))
    eng.close()


def test_bf16_subnormal_beliefs():
    """Belief entries whose hi or lo part is a bf16 subnormal, and entries below the fp32 normal range."""
    rng = np.random.default_rng(13)
    S, A, O, V, B = 2000, 2, 2, 260, 300
    rs, rto, er = model(rng, S, A, O)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S)
    tiny = rng.random((B, S)) < 0.05
    b[tiny] = rng.choice([1e-39, 3e-40, 2.0 ** -126 * 1.0078125, 2.0 ** -120 + 2.0 ** -132], size=int(tiny.sum()))
    b = b.astype(np.float32).astype(np.float64)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_alpha(alpha)
    eng.set_beliefs(b)
    check(eng, orc.backup_core(alpha, b, rs, rto, er, 0.9))
    eng.close()


def test_five_successors_projected_route():
    """R = 5: the split reads the projected Gamma rows; the belief side still comes from the plane."""
    rng = np.random.default_rng(14)
    S, A, O, V = 3000, 2, 2, 300
    rs, rto, er = model(rng, S, A, O, R=5)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    eng = Engine(S, A, O, 5, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_alpha(alpha)
    for B in (400, 130):
        b = beliefs(rng, B, S)
        eng.set_beliefs(b)
        check(eng, orc.backup_core(alpha, b, rs, rto, er, 0.9))
    eng.close()


def test_fused_and_projected_routes_agree_after_reselect():
    rng = np.random.default_rng(15)
    S, A, O, V = 4097, 3, 1, 513
    rs, rto, er = model(rng, S, A, O)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b1, b2 = beliefs(rng, 300, S), beliefs(rng, 200, S)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_alpha(alpha)
    id1 = eng.store_rows('belief', b1)
    id2 = eng.store_rows('belief', b2)
    eng.select_beliefs(np.arange(id1, id1 + len(b1)))
    run(eng, 'always')
    eng.select_beliefs(np.arange(id2, id2 + len(b2)))
    run(eng, 'always')
    eng.select_beliefs(np.arange(id1, id1 + len(b1)))
    out = {}
    for fused in (True, False):
        eng.set_fused_projection(fused)
        out[fused] = check(eng, orc.backup_core(alpha, b1, rs, rto, er, 0.9))
    f, u = out[True], out[False]
    assert np.array_equal(f.alpha, u.alpha) and np.array_equal(f.keep, u.keep)
    for k in ('n_refined', 'n_refine_candidates', 'n_refined_actions', 'n_unique', 'score_tiles_run'):
        assert f.stats[k] == u.stats[k], k
    eng.close()
