"""The engine's bookkeeping of device memory: ``device_bytes`` against ``debug_live_bytes`` (allocated minus freed, counted
by the buffers themselves), what ``after_oom`` keeps, a growth that is refused half-way, and the teardown.

Every test runs the tiger model and the 4x3 grid on an fp32 and an fp64 engine; the fp64 engine screens every backup in
fp32 (``set_f64_screen('always')``), so the screen's buffers are counted too.  ``debug_live_bytes`` is process-wide: the
tests compare its difference from a base taken (after a ``gc.collect()``) before their first engine exists, so engines that
other tests of the process left alive do not matter.

What ``after_oom`` keeps, by hand for the tiger model (S = 2, A = 3, O = 2, R = 2; S_pad = 32, one K tile, one 64-tile bit
word; T = bytes of the engine's number format):

    rs 4 A R S_pad = 768 | rto T A O R S_pad = 1536 (fp32) / 3072 | er T A S_pad = 384 / 768 | sup A O S_pad = 192
    counters 32 | nzB (A O + 1) k_tiles = 7 | nzBw 8 A O words = 48 | rto64 8 A O R S_pad = 3072 (fp32 engines given
    fp64 tables)                                                                       -> 6039 (fp32), 4887 (fp64) at creation
    in_ptr 4 A (S + 1) = 36 | in_src 4 A S R = 48 (the inverse lists: first Bayes step, refinement or belief-side scoring)
    e_cnt 16 (first run_fetch behind fp32 scores) | scr_flag 4, the screen's own tables, 6039 - 3072 = 2967, and the
    screen's inverse lists, 84 again (fp64)

-- 6139 bytes on the fp32 engine, 8042 on the screened fp64 one.  (irr_, the fused GEMM's map, does not exist on either
model: every K tile has irregular successors and R > 1.  chain_max_, dense_ and nzD_ belong to Gamma tiling and to
PBVI_DENSE engines.)  The tests take the creation part from a fresh engine -- its ``device_bytes`` after the first
``set_alpha`` / ``set_beliefs`` minus what those two allocate, by the formulas of ``upload_bytes`` -- and add the buffers
built on first use by the formulas above; on the tiger model the creation part is also compared with the hand figures.
"""
import gc

import numpy as np
import pytest

from test_device_rollout import SEED, end_mask, get_case

MIB = 1 << 20
CASES = [(name, dtype) for name in ('tiger', 'grid4x3') for dtype in ('f32', 'f64')]
pytestmark = [pytest.mark.gpu, pytest.mark.parametrize('name,dtype', CASES)]


def round_up(x, m):
    return (x + m - 1) // m * m


def live_base():
    from pomdp_pbvi_exploration_amd.engine import debug_live_bytes
    gc.collect()
    return debug_live_bytes()


def new_engine(c, dtype, rto_dtype=np.float64):
    from pomdp_pbvi_exploration_amd.engine import Engine
    m = c.m
    eng = Engine(m.state_count, m.action_count, m.observation_count, m.reachable_state_count, m.reachable_states,
                 np.asarray(m.reachable_transitional_observation_table, dtype=rto_dtype), m.expected_rewards_table, dtype=dtype)
    if dtype == 'f64':
        eng.set_f64_screen('always')
    return eng


def upload_bytes(m, dtype, V, B):
    """What the first ``set_alpha`` of V rows and the first ``set_beliefs`` of B rows allocate (first allocations are exact)."""
    T, S_pad = (4 if dtype == 'f32' else 8), round_up(m.state_count, 32)
    k_tiles, B_pad = S_pad // 32, round_up(B, 256)
    alpha = round_up(V + 1, 256) * S_pad * T
    block = B * S_pad * T + B_pad * S_pad * T + B * k_tiles + 4 * B + 4 * B + (B_pad // 256) * k_tiles   # stage, block, flags, keys,
    return alpha + block                                                                                    # order, zero map


def inverse_list_bytes(m):
    """in_ptr + in_src (module docstring)"""
    S, A, R = m.state_count, m.action_count, m.reachable_state_count
    return 4 * A * (S + 1) + 4 * A * S * R


def likely_step(m, b, a=0):
    """(observation most likely after action a in belief b, the updated belief)"""
    rto, rs = m.reachable_transitional_observation_table, m.reachable_states
    o = int(np.argmax(np.einsum('s,sor->o', b, rto[:, a])))
    nb = np.zeros_like(b)
    np.add.at(nb, rs[:, a, :], b[:, None] * rto[:, a, o, :])
    return o, nb / nb.sum()


def exercise(eng, c, check=lambda step: None):
    """One call of every allocating entry of the engine, ``check(step)`` after each."""
    from pomdp_pbvi_exploration_amd.engine import PinnedBuffer
    m, gamma = c.m, c.gamma
    S, A, O = m.state_count, m.action_count, m.observation_count
    rng = np.random.default_rng(11)
    beliefs = rng.dirichlet(np.ones(S), 300)
    mask = end_mask(m)
    check('start')
    for n in (5, 5, 290):                                   # 5 rows, exactly twice as many, then past the doubling
        eng.store_rows('belief', beliefs[:n])
        check(f'store_rows belief {n}')
    for n in (5, 5, 40):
        eng.store_rows('alpha', rng.normal(size=(n, S)))
        check(f'store_rows alpha {n}')
    eng.set_alpha(c.alpha)
    check('set_alpha')
    eng.append_alpha(rng.normal(size=(300, S)))             # 313 rows do not fit the 256 of the first allocation
    check('append_alpha (re-allocation)')
    eng.max_value_store()                                   # more than 64 alpha rows: per-row tile lists on fp32 engines
    check('max_value_store')
    eng.select_alpha(np.arange(50))                         # a primary set, free rows in front of it
    check('select_alpha primary')
    eng.select_alpha(np.arange(5))                          # a small set beside it
    check('select_alpha small')
    eng.select_alpha(np.arange(50))
    eng.append_alpha(rng.normal(size=(3, S)))               # the view does not start the allocation: move to the plain layout
    assert eng.alpha_count == 53
    check('append_alpha (plain layout)')
    eng.max_value_store(100)
    check('max_value_store, few alpha rows')
    eng.select_beliefs(np.arange(300))                      # more than one row block: sorted
    check('select_beliefs')
    for f in ('alpha', 'belief', 'auto'):
        eng.set_formulation(f)
        eng.run(gamma)
        check(f'run {f}')
        eng.fetch()
        check(f'fetch {f}')
    eng.run(gamma, belief_dominance_prune=True)
    check('run with belief dominance')
    B = eng.B
    buf = PinnedBuffer(B * S * 8 + 3 * B * 4 + 8192)
    rows = buf.carve((B, S), eng.np_dtype)
    slot, index, actions = (buf.carve((B,), np.int32) for _ in range(3))
    eng.run_fetch_into(gamma, rows, slot, index, actions)
    check('run_fetch_into')
    eng.q_values_resident(gamma, want_best=True)
    check('q_values_resident')
    eng.max_value_resident()
    check('max_value_resident')
    alpha = rng.normal(size=(70, S))
    eng.prune_dominated(alpha)
    check('prune_dominated')
    eng.prune_dominated_masked(alpha, np.arange(70) >= 60)
    check('prune_dominated_masked')
    obs = [likely_step(m, b)[0] for b in beliefs[:40]]
    eng.belief_update(beliefs[:40], np.zeros(40, dtype=np.int32), obs)
    check('belief_update')
    for n in (10, 3):                                       # with and without the quarters that leave during the chain
        b, walk_obs = beliefs[0], []
        for _ in range(n):
            o, b = likely_step(m, b)
            walk_obs.append(o)
        eng.belief_walk(beliefs[0], np.zeros(n, dtype=np.int32), walk_obs)
        check(f'belief_walk {n}')
    eng.set_beliefs(beliefs[:40])
    assert eng.advance_beliefs(np.zeros(40, dtype=np.int32), obs, keep=np.arange(40) % 3 != 0) == 26
    check('advance_beliefs')
    eng.set_alpha(c.alpha)
    for lookahead in (0, 1):
        eng.set_beliefs(c.b0[:40])
        eng.rollout(c.acts, c.s0[:40], mask, SEED, 5, lookahead=lookahead, gamma=gamma)
        check(f'rollout lookahead {lookahead}')
    eng.set_beliefs(c.b0[:40])
    eng.rollout_infotaxis(c.s0[:40], mask, SEED, 5)
    check('rollout_infotaxis')
    eng.set_beliefs(beliefs[:40])
    eng.infotaxis_resident(want_p_obs=True, want_entropy=True)
    check('infotaxis_resident')
    keys = np.column_stack([rng.integers(0, A, 6)] + [rng.integers(0, eng.alpha_count, 6) for _ in range(O)])
    eng.assemble_rows(keys, gamma)
    check('assemble_rows')
    eng.assemble_rows_store(keys, gamma)
    check('assemble_rows_store')


def test_device_bytes_is_what_the_buffers_hold(name, dtype):
    from pomdp_pbvi_exploration_amd.engine import debug_live_bytes
    c = get_case(name)
    base = live_base()
    eng = new_engine(c, dtype)

    def check(step):
        held, live = eng.device_bytes, debug_live_bytes() - base
        assert held == live, f'after {step}: device_bytes {held}, live {live}'
    try:
        check('creation')
        exercise(eng, c, check)
        eng.after_oom()
        check('after_oom')
    finally:
        eng.close()


def test_after_oom_keeps_the_model_lifetime_buffers_only(name, dtype):
    c = get_case(name)
    m = c.m
    fresh = new_engine(c, dtype)
    fresh.set_alpha(c.alpha)
    fresh.set_beliefs(c.b0)
    created = fresh.device_bytes - upload_bytes(m, dtype, c.alpha.shape[0], c.b0.shape[0])
    fresh.close()
    if name == 'tiger':
        assert created == {'f32': 6039, 'f64': 4887}[dtype]
    bound = created + inverse_list_bytes(m) + 16            # + e_cnt
    if dtype == 'f64':                                      # scr_flag + the screen: an fp32 engine given fp32 tables + its lists
        screen = new_engine(c, 'f32', rto_dtype=np.float32)
        bound += 4 + screen.device_bytes + inverse_list_bytes(m)
        screen.close()
    if name == 'tiger':
        assert bound == {'f32': 6139, 'f64': 8042}[dtype]
    eng = new_engine(c, dtype)
    try:
        held = []
        for _ in range(2):
            exercise(eng, c)
            assert eng.device_bytes > bound + MIB           # (the working buffers were there)
            eng.after_oom()
            held.append(eng.device_bytes)
        print(f'{name} {dtype}: after_oom leaves {held}, bound {bound}')
        assert held[0] <= bound
        assert held[1] == held[0]
    finally:
        eng.close()


def test_refused_growth_leaves_the_count_as_it_was(name, dtype):
    """``append_alpha`` and ``store_rows`` under a cap that the new allocation of their grow-and-keep step exceeds: MemoryError,
    the engine holds what it counts, and its next backup is a fresh engine's bit for bit."""
    from pomdp_pbvi_exploration_amd.engine import debug_alloc_limit, debug_live_bytes
    c = get_case(name)
    S = c.m.state_count
    row_bytes = round_up(S, 32) * (4 if dtype == 'f32' else 8)
    big = np.zeros((5 * MIB // row_bytes + 1, S))           # 5 MiB of device rows against 4 MiB of head room
    small = np.random.default_rng(3).normal(size=(5, S))
    beliefs = np.random.default_rng(4).dirichlet(np.ones(S), 20)
    base = live_base()
    eng = new_engine(c, dtype)
    try:
        eng.set_alpha(c.alpha)
        for which in ('alpha', 'belief'):
            eng.store_rows(which, small)
        prev = debug_alloc_limit(eng.device_bytes // MIB + 4)
        try:
            with pytest.raises(MemoryError):
                eng.append_alpha(big)
            assert eng.device_bytes == debug_live_bytes() - base
            assert eng.alpha_count == 0                     # (Engine._ck has called pbvi_engine_after_oom)
            for which in ('alpha', 'belief'):
                eng.store_rows(which, small)
                with pytest.raises(MemoryError):
                    eng.store_rows(which, big)
                assert eng.device_bytes == debug_live_bytes() - base
        finally:
            debug_alloc_limit(prev)
        got = eng.backup_full(c.alpha, beliefs, c.gamma)
        assert eng.device_bytes == debug_live_bytes() - base
        fresh = new_engine(c, dtype)
        try:
            want = fresh.backup_full(c.alpha, beliefs, c.gamma)
        finally:
            fresh.close()
        for field in ('unique_alpha', 'index', 'actions', 'best_alpha_ind', 'keep'):
            assert np.array_equal(getattr(got, field), getattr(want, field)), field
    finally:
        eng.close()


def test_closed_engines_hold_nothing(name, dtype):
    from pomdp_pbvi_exploration_amd.engine import debug_live_bytes, mdp_value_iteration
    c = get_case(name)
    m = c.m
    base = live_base()
    eng = new_engine(c, dtype)
    exercise(eng, c)
    assert debug_live_bytes() - base == eng.device_bytes > MIB
    mdp_value_iteration(m.reachable_states, m.reachable_transitional_observation_table.sum(axis=2), m.expected_rewards_table,
                        np.zeros(m.state_count), c.gamma, 1e-6, 10)               # (buffers of its own, gone when it returns)
    assert debug_live_bytes() - base == eng.device_bytes
    eng.close()
    del eng
    gc.collect()
    assert debug_live_bytes() == base
