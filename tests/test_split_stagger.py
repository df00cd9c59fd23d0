"""The split score GEMM's stagger (gemm.hip: tile_run_split; pbvi_debug_split_stagger): with it, waves 4-7 of a block
scale, split and store the next tile's B rows first and run the step's MFMAs last, out of phase with waves 0-3, which run
the parent step.  Same terms in the same order on the same LDS image, so against the lockstep kernel the raw slab buffer
(pbvi_debug_slabs) is the same bytes and every output and counter of the backup is equal, whichever of the two runs first.
A misplaced wait or a missed tail condition of the late half's two-tile lookahead would not fault -- no address differs --
it would store a tile from registers that have not arrived, or skip a tile's store: other bits.

The method is test_split_schedule.run_both's: the slab buffer is brought to its final size, then every byte of it is set to
FILL before each run, so what a run leaves in the buffer is what its own kernel wrote."""
import numpy as np
import pytest

from pomdp_pbvi_exploration_amd.engine import Engine, debug_split_schedule, debug_split_stagger
from score_cases import beliefs, random_model
from test_split_schedule import COUNTERS, FILL

pytestmark = pytest.mark.gpu

ORDERS = (('lockstep', 'staggered'), ('staggered', 'lockstep'))


def run_orders(eng, alpha, b, gamma):
    """The same backup with the stagger off and on, in both run orders: per order, {name: (result, slab bytes)}"""
    outs = []
    prev = debug_split_stagger(True)
    try:
        assert debug_split_schedule('parent') == 'parent'  # the stagger belongs to the parent schedule
        eng.backup_full(alpha, b, gamma)                   # the buffer exists at its final size from here on
        for order in ORDERS:
            out = {}
            for name in order:
                debug_split_stagger(name == 'staggered')
                eng.debug_slabs_fill(FILL)
                res = eng.backup_full(alpha, b, gamma)     # (no dominance stage: its GEMM would re-use the slab buffer)
                assert res.stats['score_split'] == 1, name
                out[name] = (res, eng.debug_slabs())
            outs.append(out)
    finally:
        debug_split_stagger(prev)
    return outs


def check_equal(out):
    (p, p_slabs), (n, n_slabs) = out['lockstep'], out['staggered']
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


def test_the_switch_reports_the_previous_value():
    first = debug_split_stagger(False)
    try:
        assert debug_split_stagger(True) is False
        assert debug_split_stagger(True) is True
        assert debug_split_stagger(False) is True
        assert debug_split_schedule('parent') == 'parent'                  # a second switch, not a third schedule
    finally:
        debug_split_stagger(first)


@pytest.mark.parametrize('S,A,O,V,B,regular,fused', [
    (1000, 2, 2, 512, 70, False, True),       # irregular successors: gathered alphas
    (4097, 3, 1, 300, 300, True, True),       # two m-tiles, stream-K continuation slabs
    (4097, 3, 1, 300, 300, True, False),      # the projected route: B rows read from fp32 Gamma
])
def test_stagger_agrees_bit_for_bit(S, A, O, V, B, regular, fused):
    rng = np.random.default_rng(S + V)
    rs, rto, er = random_model(rng, S, A, O, regular)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_score_split('always')
    eng.set_fused_projection(fused)
    outs = run_orders(eng, alpha, b, 0.9)
    if not fused:
        assert outs[0]['staggered'][0].stats['fused_projection'] == 0
    for out in outs:
        check_equal(out)
    eng.close()


@pytest.mark.parametrize('fused', [True, False])
@pytest.mark.parametrize('S,k_tiles', [(40, 1), (100, 2), (100, 3), (130, 4)])
def test_short_segments(S, k_tiles, fused):
    """test_split_schedule.test_short_segments' construction: beliefs supported on the first k_tiles K tiles (32 states
    each), so every tile list has 1, 2, 3 or 4 entries -- the late half's first, only and last steps, and both tail
    conditions of its lookahead (no store and no DMA for the last tile, no register loads for the last two).  207 pairs
    (A O V / 256, rounded up): the share of the plan (cost units per block of 256; a pair costs its tiles + 1) equals one
    pair's cost for each of the four lengths, so shares and pairs coincide and every segment is a whole list."""
    A, O, V, B = 2, 2, 13200, 40
    rng = np.random.default_rng(100 * S + k_tiles)
    rs, rto, er = random_model(rng, S, A, O, True)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S, density=0.5, support=min(S, 32 * k_tiles))
    assert np.all(b[:, 32 * k_tiles:] == 0) and np.any(b[:, 32 * (k_tiles - 1):] > 0)    # the last tile is not empty
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    eng.set_formulation('alpha')
    eng.set_score_split('always')
    eng.set_fused_projection(fused)
    outs = run_orders(eng, alpha, b, 0.9)
    for out in outs:
        check_equal(out)
    tiles = outs[0]['staggered'][0].stats['score_tiles_run']
    pairs = tiles // k_tiles
    assert tiles == pairs * k_tiles and pairs >= 204, (tiles, pairs)
    blocks = 256                                            # one persistent block per CU of the MI355X
    assert -(-pairs * (k_tiles + 1) // blocks) == k_tiles + 1, (tiles, pairs)
    eng.close()
