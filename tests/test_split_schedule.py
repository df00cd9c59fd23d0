"""The split score GEMM's two K-step schedules (gemm.hip: tile_run_split; pbvi_debug_split_schedule): the pipelined one,
whose LDS fragment reads run a group ahead of the MFMAs behind counted waits, against the parent one (the default).
Both read the same LDS image and add the same terms in the same order, so the raw slab buffer (pbvi_debug_slabs) is the
same bytes and every output and counter of the backup is equal.  A wrong wait count would not fault -- no address
differs -- it would hand an MFMA a register the read has not reached yet, i.e. other bits."""
import numpy as np
import pytest

from pomdp_pbvi_exploration_amd.engine import Engine, debug_split_schedule
from score_cases import beliefs, random_model

pytestmark = pytest.mark.gpu

COUNTERS = ('n_refined', 'n_refine_candidates', 'n_refined_actions', 'n_unique', 'score_tiles_run')


FILL = 0xA5


def run_both(eng, alpha, b, gamma, order=('parent', 'pipelined')):
    """The same backup under both schedules, in `order`: (result, slab bytes) of each.  The slab buffer is a grow-and-keep
    buffer that both runs write, so every byte of it is set to FILL before each run: what a run leaves in the buffer is
    what its own kernel wrote, and a kernel that did not run, or skipped a region, shows as FILL bytes the other run lacks."""
    out = {}
    prev = debug_split_schedule('parent')
    try:
        eng.backup_full(alpha, b, gamma)                   # the buffer exists at its final size from here on
        for schedule in order:
            debug_split_schedule(schedule)
            eng.debug_slabs_fill(FILL)
            res = eng.backup_full(alpha, b, gamma)         # (no dominance stage: its GEMM would re-use the slab buffer)
            assert res.stats['score_split'] == 1, schedule
            out[schedule] = (res, eng.debug_slabs())
    finally:
        debug_split_schedule(prev)
    return out


def check_equal(out):
    (p, p_slabs), (n, n_slabs) = out['parent'], out['pipelined']
    assert p_slabs.size == n_slabs.size and p_slabs.size > 0
    assert np.count_nonzero(p_slabs != FILL) > p_slabs.size // 64          # the runs did write scores over the fill
    differ = int(np.count_nonzero(p_slabs != n_slabs))
    assert differ == 0, f'{differ} of {p_slabs.size} slab bytes differ'
    assert np.array_equal(p.alpha, n.alpha)
    assert np.array_equal(p.actions, n.actions)
    assert np.array_equal(p.best_alpha_ind, n.best_alpha_ind)
    assert np.array_equal(p.keep, n.keep)
    for k in COUNTERS:
        assert p.stats[k] == n.stats[k], k


def test_the_switch_reports_the_previous_schedule():
    assert debug_split_schedule('pipelined') == 'parent'               # the default
    assert debug_split_schedule('parent') == 'pipelined'
    assert debug_split_schedule('parent') == 'parent'


@pytest.mark.parametrize('S,A,O,V,B,regular,fused,order', [
    (1000, 2, 2, 512, 70, False, True, ('parent', 'pipelined')),      # irregular successors: gathered alphas
    (4097, 3, 1, 300, 300, True, True, ('pipelined', 'parent')),      # two m-tiles, stream-K continuation slabs
    (4097, 3, 1, 300, 300, True, False, ('parent', 'pipelined')),     # the projected route: B rows read from fp32 Gamma
])
def test_schedules_agree_bit_for_bit(S, A, O, V, B, regular, fused, order):
    rng = np.random.default_rng(S + V)
    rs, rto, er = random_model(rng, S, A, O, regular)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_score_split('always')
    eng.set_fused_projection(fused)
    out = run_both(eng, alpha, b, 0.9, order)
    if not fused:
        assert out['pipelined'][0].stats['fused_projection'] == 0
    check_equal(out)
    eng.close()


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('S,k_tiles', [(40, 1), (40, 2), (100, 1), (100, 2), (100, 3)])
def test_short_segments(S, k_tiles, fused):
    """Beliefs supported on the first 1, 2 or 3 K tiles (32 states each), so every tile list has that many entries: the
    loop's first, only and last steps.  Enough pairs (A O V / 256 = 204) that a stream-K share holds a whole list -- with
    fewer, every segment would be cut down to one tile.  Asserted from the tile count: every pair lists k_tiles tiles, and
    the share size of the plan (cost units per block; a pair costs its tiles + 1) equals one pair's cost, so shares and
    pairs coincide and every segment is a whole list."""
    A, O, V, B = 2, 2, 13000, 40
    rng = np.random.default_rng(100 * S + k_tiles)
    rs, rto, er = random_model(rng, S, A, O, True)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S, density=0.5, support=min(S, 32 * k_tiles))
    assert np.all(b[:, 32 * k_tiles:] == 0) and np.any(b[:, 32 * (k_tiles - 1):] > 0)    # the last tile is not empty
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_score_split('always')
    eng.set_fused_projection(fused)
    out = run_both(eng, alpha, b, 0.9)
    check_equal(out)
    tiles = out['pipelined'][0].stats['score_tiles_run']
    pairs = tiles // k_tiles
    assert tiles == pairs * k_tiles and pairs >= 204, (tiles, pairs)
    blocks = 256                                            # one persistent block per CU of the MI355X
    assert -(-pairs * (k_tiles + 1) // blocks) == k_tiles + 1, (tiles, pairs)
    eng.close()
