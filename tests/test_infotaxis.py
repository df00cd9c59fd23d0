"""Infotaxis: ``infotaxis_numpy`` / ``rollout_infotaxis_numpy`` / ``Infotaxis_Agent`` on the host, ``pbvi_infotaxis`` /
``pbvi_rollout_infotaxis`` on the device.

The quantity is ``G[b,a] = sum_o (Z ln Z - N)`` with ``Z = sum_s' u``, ``N = sum_s' u ln u`` and ``u`` the un-normalised Bayes
update of ``b`` with ``(a, o)`` -- the expected entropy of the next belief.  The device sums the same terms in another
(fixed) order, so every device value is compared with the host statement, evaluated on the values as the engine holds
them, within

    ``8 * S * 2^-53 * M``,   floored at 1e-15,

``M`` the sum of the magnitudes of the terms (``sum_o (|Z ln Z| + sum_s' |u ln u|)`` for ``G``, ``Z`` for ``p_obs``,
``sum_s |b ln b|`` for the entropy): the worst case of re-ordering a sum of S terms plus the 1-2 ulp of ``log`` and of a
contracted multiply-add.  The bound is derived, not measured, and is the same for fp32 and fp64 engines (both accumulate
in fp64).  ``out_action`` is compared exactly with the first argmin of the returned row.
"""
import ctypes as C
import hashlib
import json
from types import SimpleNamespace

import numpy as np
import pytest

import model_cases as mc
import test_device_rollout as tdr
from pomdp_pbvi_exploration_amd import pomdp as pomdp_mod
from pomdp_pbvi_exploration_amd.pomdp import (Agent, Belief, Infotaxis_Agent, Model, infotaxis_first_argmin, infotaxis_numpy,
                                              rollout_draw, rollout_infotaxis_numpy, rollout_numpy, rollout_uniform)
from test_device_rollout import (BELIEF_TOL, CASES, N_SIM, SEED, T_STEPS, VALUE_TOL, _assert_padding, end_mask, get_case, r32)

XBLOCK_STATES = 2048                      # landing states one block of k_succ_entropy walks (SE_NT chunks of 256)


def tables(S, A, O, R, rs, rto, end_states=()):
    return tdr._tables(S, A, O, R, rs, rto, np.zeros((S, A)), end_states)


def structure(name, S, O=2):
    rs, rto = mc.STRUCTURES[name](S, O=O)
    return tables(S, rto.shape[1], rto.shape[2], rto.shape[3], rs, rto)


def bound(S, M):
    return np.maximum(8.0 * S * 2.0 ** -53 * np.asarray(M), 1e-15)


# --------------------------------------------------------------------------------------------------------------------- #
# host (no GPU)
# --------------------------------------------------------------------------------------------------------------------- #
def entropy(p):
    p = p[p > 0]
    return float(-np.sum(p * np.log(p)))


def brute_force(m, b):
    """``sum_o P(o|b,a) H(Belief.update(a, o))`` for every action, with one ``Belief.update`` per (a, o)."""
    rto = m.reachable_transitional_observation_table
    G = np.zeros(m.action_count)
    bel = Belief.__new__(Belief)
    bel.model, bel._values = m, b
    for a in range(m.action_count):
        for o in range(m.observation_count):
            p = float(np.sum(b[:, None] * rto[:, a, o, :]))
            if p > 0.0:
                G[a] += p * entropy(bel.update(a, o).values)
    return G


def host_beliefs(m, n, seed):
    rng = np.random.default_rng(seed)
    b = mc.sparse_beliefs(rng, n, m.state_count, density=0.4)
    b[0] = 1.0 / m.state_count
    return b


@pytest.mark.parametrize('name', ['tiger', 'grid4x3', 'ragged'])
def test_host_statement_against_belief_update(name):
    m = get_case(name).m
    b = host_beliefs(m, 7, 1)
    G, action, p_obs, H = infotaxis_numpy(m, b)
    assert G.shape == (7, m.action_count) and p_obs.shape == (7, m.action_count, m.observation_count) and H.shape == (7,)
    want = np.array([brute_force(m, row) for row in b])
    np.testing.assert_allclose(G, want, rtol=0, atol=1e-10)
    assert np.array_equal(action, np.argmin(G, axis=1))
    np.testing.assert_allclose(H, [entropy(row) for row in b], rtol=0, atol=1e-10)
    # one row at a time = the block; any chunking of the rows = the block
    for i in range(7):
        assert np.array_equal(infotaxis_numpy(m, b[i:i + 1])[0][0], G[i])
    assert np.array_equal(pomdp_mod._infotaxis_terms(m, b, rows_at_once=3)[0], G)


def test_tiger_known_answer():
    m = get_case('tiger').m                                        # actions: listen, open-left, open-right
    G, action, p_obs, H = infotaxis_numpy(m, np.array([[0.5, 0.5]]))
    listen = -(0.85 * np.log(0.85) + 0.15 * np.log(0.15))
    assert listen == pytest.approx(0.42270908780599087, abs=1e-15)
    np.testing.assert_allclose(G[0], [listen, np.log(2.0), np.log(2.0)], rtol=0, atol=1e-14)
    assert action[0] == 0
    assert H[0] == pytest.approx(np.log(2.0), abs=1e-15)
    masked = G.copy()
    masked[:, 0] = np.nan                                          # listen masked out: the first of the two tied opens
    assert masked[0, 1] == masked[0, 2] and infotaxis_first_argmin(masked)[0] == 1


@pytest.mark.parametrize('name', ['tiger', 'grid4x3', 'ragged', 'olf_R5'])
def test_observation_probabilities_sum_to_the_tables_mass(name):
    m = get_case(name).m
    b = host_beliefs(m, 5, 2)
    p_obs = infotaxis_numpy(m, b)[2]
    mass = b @ m.reachable_transitional_observation_table.sum(axis=(2, 3))            # [n, A]: 1 where the tables are normalised
    np.testing.assert_allclose(p_obs.sum(axis=2), mass, rtol=0, atol=1e-12)
    np.testing.assert_allclose(mass, 1.0, rtol=0, atol=1e-6)


def test_first_argmin_and_nans():
    nan = np.nan
    G = np.array([[nan, 2.0, 1.0], [nan, nan, nan], [1.0, nan, 1.0], [3.0, nan, 2.0], [np.inf, np.inf, nan], [nan, np.inf, 5.0]])
    assert infotaxis_first_argmin(G).tolist() == [2, 0, 0, 2, 0, 2]


def test_one_hot_belief():
    m = structure('identity', 33, O=3)
    b = np.zeros((2, 33))
    b[0, 5] = b[1, 32] = 1.0
    G, action, p_obs, H = infotaxis_numpy(m, b)
    assert np.all(H == 0.0)
    np.testing.assert_allclose(G, 0.0, rtol=0, atol=1e-15)        # the state is known and stays known
    np.testing.assert_allclose(p_obs[0], m.reachable_transitional_observation_table[5, :, :, 0], rtol=0, atol=1e-16)
    # a model that spreads the state: G = sum_o (Z ln Z - sum_s' u ln u) with u read off the one table row
    m = get_case('ragged').m
    s = 7
    b = np.zeros((1, m.state_count))
    b[0, s] = 1.0
    G = infotaxis_numpy(m, b)[0][0]
    for a in range(m.action_count):
        want = 0.0
        for o in range(m.observation_count):
            u = np.bincount(m.reachable_states[s, a], weights=m.reachable_transitional_observation_table[s, a, o], minlength=m.state_count)
            want += u.sum() * entropy(u / u.sum()) if u.sum() > 0 else 0.0            # Z ln Z - sum u ln u = Z H(u / Z)
        assert G[a] == pytest.approx(want, abs=1e-12)


def test_host_rollout_chunks_and_done_semantics():
    c = get_case('grid4x3')
    run = lambda lo, hi, seed=SEED: rollout_infotaxis_numpy(c.m, c.b0[lo:hi], c.s0[lo:hi], seed, lo, T_STEPS)
    whole, first, second = run(0, 50), run(0, 20), run(20, 50)
    for k in range(4):
        assert np.array_equal(whole[k], np.concatenate([first[k], second[k]], axis=-1)), k
    assert not np.array_equal(whole[0], run(0, 50, SEED + 1)[0])
    states, actions, observations, steps = whole
    assert states.dtype == actions.dtype == observations.dtype == steps.dtype == np.int32
    assert np.array_equal(states[0], c.s0[:50])
    _assert_padding(states, actions, observations, steps, c.m.end_states)
    assert np.any(steps < T_STEPS)
    # the first step's actions are the host statement's; the surviving beliefs come back on request
    assert np.array_equal(actions[0], infotaxis_numpy(c.m, c.b0[:50])[1])
    out = rollout_infotaxis_numpy(c.m, c.b0[:50], c.s0[:50], SEED, 0, T_STEPS, return_beliefs=True)
    assert out[4].shape == (int(np.sum(steps == T_STEPS) - np.sum(np.isin(states[T_STEPS], c.m.end_states))), c.m.state_count)
    for bad in (dict(T=0), dict(start_states=np.full(50, c.m.state_count))):
        with pytest.raises(ValueError):
            rollout_infotaxis_numpy(**{**dict(model=c.m, beliefs=c.b0[:50], start_states=c.s0[:50], seed=1, first_sim_id=0, T=3), **bad})


def test_infotaxis_agent_on_the_host():
    model, _ = tdr.grid_model()
    agent = Infotaxis_Agent(model)
    n, T = 40, 30
    np.random.seed(3)
    totals, hists = agent.run_n_simulations_parallel(n=n, max_steps=T, print_progress=False, print_stats=False, device_rng_seed=11)
    s0 = np.array([h.states[0] for h in hists])
    b0 = np.repeat(np.asarray(model.start_probabilities, dtype=np.float64)[None, :], n, axis=0)
    states, actions, observations, steps = rollout_infotaxis_numpy(model, b0, s0, 11, 0, T)
    assert len(hists) == n and len(totals) == n
    for i, h in enumerate(hists):
        k = int(steps[i])
        assert h.states == states[:k + 1, i].tolist() and h.actions == actions[:k, i].tolist()
        assert h.observations == observations[:k, i].tolist() and len(h.rewards) == k
    # one belief, a block of beliefs, and the default (NumPy stream) paths take the host statement's action
    b = host_beliefs(pomdp_mod._rollout_tables(model), 6, 4)
    want = infotaxis_numpy(model, b)[1]
    assert np.array_equal(agent.get_best_action(b), want)
    assert agent.get_best_action(Belief(model, b[2])) == want[2]
    np.random.seed(8)
    h = agent.simulate(max_steps=12, print_progress=False, print_stats=False)
    assert h.actions[0] == infotaxis_numpy(model, np.asarray(model.start_probabilities)[None, :])[1][0]
    np.random.seed(8)
    _, one_by_one = agent.run_n_simulations(n=3, max_steps=12, print_progress=False, print_stats=False)
    assert one_by_one[0].states == h.states and one_by_one[0].actions == h.actions
    np.random.seed(9)
    _, par = agent.run_n_simulations_parallel(n=25, max_steps=15, print_progress=False, print_stats=False)
    assert len(par) == 25 and all(p.actions[0] == h.actions[0] for p in par)


def _digest_arrays(arrays):
    return hashlib.sha256(b''.join(np.ascontiguousarray(x, dtype=np.int32).tobytes() for x in arrays)).hexdigest()


def test_agent_and_rollout_numpy_are_unchanged():
    """One seeded run of each per lookahead; the digests were recorded from the code before ``Agent`` and ``rollout_numpy``
    began to share their loops with the infotaxis policy."""
    c = get_case('grid4x3')
    want = {0: '6e66dbe59f2f1849bdba8d12e5094ab963f86ce40c241c4ea322d01a42f7e702',
            1: '0e8ea2b3eb2f74ab27922c79d2336f323a749d8728458a37bc9be07895d87f65'}
    for lookahead in (0, 1):
        out = rollout_numpy(c.m, c.alpha, c.acts, c.b0[:60], c.s0[:60], 77, 5, 30, lookahead, c.gamma)
        assert _digest_arrays(out) == want[lookahead], lookahead
    model, vf, gamma = tdr._grid_agent()
    want = {0: 'be4759e9d1b43237499670705b716e2eb4d6d5b9a0fd8ab22ec8a1212ebcebd8',
            1: '20179b28b98452ce6ab7e21f51f909fd639e1e379eb28f1ed8e5cfd727b86876'}
    for lookahead in (0, 1):
        agent = Agent(model, vf, lookahead=lookahead, gamma=gamma)
        np.random.seed(21)
        _, hists = agent.run_n_simulations_parallel(n=40, max_steps=25, print_progress=False, print_stats=False)
        blob = json.dumps([[list(map(int, h.states)), list(map(int, h.actions)), list(map(int, h.observations))] for h in hists])
        assert hashlib.sha256(blob.encode()).hexdigest() == want[lookahead], lookahead


# --------------------------------------------------------------------------------------------------------------------- #
# device
# --------------------------------------------------------------------------------------------------------------------- #
def make_engine(m, dtype, mode='sparse'):
    """An engine over the tables, WITHOUT an alpha set."""
    from pomdp_pbvi_exploration_amd.engine import Engine
    return Engine(m.state_count, m.action_count, m.observation_count, m.reachable_state_count, m.reachable_states,
                  m.reachable_transitional_observation_table, m.expected_rewards_table, dtype=dtype, mode=mode)


def held(m, b, dtype):
    """Tables and beliefs as an engine of ``dtype`` holds them, back in fp64."""
    if dtype == 'f64':
        return m, np.asarray(b, dtype=np.float64)
    m = SimpleNamespace(**vars(m))
    m.reachable_transitional_observation_table = r32(m.reachable_transitional_observation_table)
    return m, r32(b)


def check_values(m, b, dtype, mode='sparse', tag=''):
    """pbvi_infotaxis on a fresh engine against the host statement on the values the engine holds."""
    S = m.state_count
    mh, bh = held(m, b, dtype)
    G, Z, H, MG, MH = pomdp_mod._infotaxis_terms(mh, bh)
    eng = make_engine(m, dtype, mode)
    try:
        eng.set_beliefs(b)
        g, act, p_obs, ent = eng.infotaxis_resident(want_p_obs=True, want_entropy=True)
        g2, act2 = eng.infotaxis_resident()                     # the short form, and a second call: equal bits
    finally:
        eng.close()
    for name, got, want, M in (('G', g, G, MG), ('p_obs', p_obs, Z, Z), ('entropy', ent, H, MH)):
        assert got.shape == want.shape and got.dtype == np.float64, (tag, name)
        err, lim = np.abs(got - want), bound(S, M)
        worst = float(np.max(err / lim))
        print(f'{tag} {dtype} {mode} {name}: largest error / bound = {worst:.3e} (largest error {float(err.max()):.3e})')
        assert np.all(err <= lim), (tag, name, worst)
    assert np.array_equal(act, infotaxis_first_argmin(g)), tag    # exactly, from the returned row
    assert g2.tobytes() == g.tobytes() and np.array_equal(act2, act), tag
    return g, act


B_SIZES, O_SIZES = [1, 3, 4, 5, 257], [1, 2, 3, 5]
STRUCTURE_CASES = [(name, S) for name in mc.STRUCTURES for S in (31, 33, 255, 256, 257, 600)]


@pytest.mark.gpu
@pytest.mark.parametrize('i', range(len(STRUCTURE_CASES)), ids=[f'{n}-{S}' for n, S in STRUCTURE_CASES])
def test_values_on_the_structures(i):
    """Every structure at every S around the 32-state pad and the 256-state chunk, B around the four beliefs a thread
    shares and past one sorted block, O around the four observations of a pass; both engine types."""
    name, S = STRUCTURE_CASES[i]
    B, O = B_SIZES[i % 5], O_SIZES[(i + i // 4) % 4]
    m = structure(name, S, O=O)
    assert m.observation_count == O
    b = mc.sparse_beliefs(np.random.default_rng(100 + i), B, S)
    for dtype in ('f64', 'f32'):
        check_values(m, b, dtype, tag=f'{name} S={S} B={B} O={O}')


def test_structure_cases_cover_every_size():
    combos = {(B_SIZES[i % 5], O_SIZES[(i + i // 4) % 4]) for i in range(len(STRUCTURE_CASES))}
    assert {B for B, _ in combos} == set(B_SIZES) and {O for _, O in combos} == set(O_SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize('seed', range(6))
def test_values_on_random_models(seed):
    S, A, O, R, rs, rto, er, alpha, b, gamma = mc.random_case(seed)
    check_values(tables(S, A, O, R, rs, rto), b, 'f64' if seed % 2 else 'f32', tag=f'random {seed} S={S} A={A} O={O} R={R} B={b.shape[0]}')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('name', ['tiger', 'grid4x3', 'olf_R1', 'olf_R5'])
def test_values_on_the_named_models(name, dtype):
    c = get_case(name)
    b = host_beliefs(c.m, 5, 3)
    b[1] = c.b0[0]
    g, act = check_values(c.m, b, dtype, tag=name)
    if name == 'tiger':
        assert act[0] == 0 and g[0, 1] == g[0, 2]                 # listen; the two opens tie exactly


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_values_past_one_x_block(dtype):
    """S just above the states one block walks: the finish kernel adds two partials per (b, a, o); the hub's inverse list
    holds every state."""
    m = structure('hub', XBLOCK_STATES + 1, O=3)
    b = mc.sparse_beliefs(np.random.default_rng(5), 5, m.state_count)
    check_values(m, b, dtype, tag='hub past one x-block')


@pytest.mark.gpu
def test_values_on_a_dense_engine():
    m = structure('ragged', 257, O=3)
    check_values(m, mc.sparse_beliefs(np.random.default_rng(6), 5, 257), 'f64', mode='dense', tag='ragged dense')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_a_rows_bits_do_not_depend_on_the_block(dtype):
    """The no-atomics property: a row's G (and p_obs, entropy) has the same bits alone in a block as among 257 rows (a
    sorted block), and at any position in it."""
    m = get_case('olf_R5').m
    rng = np.random.default_rng(9)
    b = mc.sparse_beliefs(rng, 257, m.state_count, density=0.1)
    eng = make_engine(m, dtype)
    try:
        eng.set_beliefs(b)
        whole = eng.infotaxis_resident(want_p_obs=True, want_entropy=True)
        for i in (0, 1, 130, 256):
            eng.set_beliefs(b[i:i + 1])
            alone = eng.infotaxis_resident(want_p_obs=True, want_entropy=True)
            for k in range(4):
                assert alone[k][0].tobytes() == whole[k][i].tobytes(), (i, k)
        order = rng.permutation(257)
        eng.set_beliefs(b[order])
        moved = eng.infotaxis_resident(want_p_obs=True, want_entropy=True)
        for k in range(4):
            assert moved[k].tobytes() == np.ascontiguousarray(whole[k][order]).tobytes(), k
        eng.set_beliefs(b[order[:6]])                             # a group of four and a group of two
        few = eng.infotaxis_resident()
        assert few[0].tobytes() == np.ascontiguousarray(whole[0][order[:6]]).tobytes()
    finally:
        eng.close()


@pytest.mark.gpu
def test_block_alpha_set_and_backup_are_untouched():
    c = get_case('olf_R5')
    eng, fresh = tdr.make_engine(c, 'f32'), tdr.make_engine(c, 'f32')
    try:
        block = c.b0[:40] * 0 + mc.sparse_beliefs(np.random.default_rng(2), 40, c.m.state_count)
        eng.set_beliefs(block)
        eng.infotaxis_resident(want_p_obs=True, want_entropy=True)
        assert eng.B == 40 == int(eng._lib.pbvi_beliefs_count(eng._h)) and eng.alpha_count == c.alpha.shape[0]
        assert np.array_equal(eng.fetch_beliefs(), block.astype(np.float32))
        eng.run(c.gamma)
        got = eng.fetch()
        fresh.set_beliefs(block)
        fresh.run(c.gamma)
        want = fresh.fetch()
        assert np.array_equal(got.actions, want.actions) and np.array_equal(got.best_alpha_ind, want.best_alpha_ind)
        assert np.array_equal(got.alpha, want.alpha)
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
def test_argument_errors():
    m = get_case('grid4x3').m
    f64p, i32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    eng = make_engine(m, 'f64')
    try:
        lib = eng._lib
        g = np.empty((3, m.action_count))
        assert lib.pbvi_infotaxis(eng._h, g.ctypes.data_as(f64p), None, None, None) == -1 and b'belief' in lib.pbvi_last_error()
        s0, mask = np.zeros(3, dtype=np.int32), end_mask(m)
        roll = lambda s0=s0, mask=mask, T=4: lib.pbvi_rollout_infotaxis(
            eng._h, s0.ctypes.data_as(i32p) if s0 is not None else None, mask.ctypes.data_as(u8p) if mask is not None else None,
            0, SEED, T, None, None, None, None)
        assert roll() == -1 and b'belief' in lib.pbvi_last_error()
        eng.set_beliefs(host_beliefs(m, 3, 0))
        assert lib.pbvi_infotaxis(eng._h, None, None, None, None) == -1 and b'NULL out_g' in lib.pbvi_last_error()
        assert lib.pbvi_infotaxis(eng._h, g.ctypes.data_as(f64p), None, None, None) == 0            # every optional output NULL
        assert np.array_equal(g, eng.infotaxis_resident()[0])
        bad = s0.copy()
        bad[2] = m.state_count
        for kw, code, word in ((dict(s0=bad), -1, b'start state'), (dict(T=0), -1, b'T'), (dict(s0=None), -1, b'NULL'),
                               (dict(mask=None), -1, b'NULL'), (dict(T=(1 << 31) // 3 + 1), -4, b'int32')):
            assert roll(**kw) == code and word in lib.pbvi_last_error(), kw.keys()
            assert lib.pbvi_beliefs_count(eng._h) == 3                                              # nothing ran
        assert roll() == 0                                                                          # and no alpha set was needed
    finally:
        eng.close()


@pytest.mark.gpu
def test_partials_obey_the_allocation_cap():
    """A * O = 64 pairs per belief make the partial sums (and p_obs) several times the belief block: under a 2 MiB cap
    the block of 4000 beliefs fits and the partials (4 MiB) do not."""
    from pomdp_pbvi_exploration_amd import engine as engine_mod
    rng = np.random.default_rng(12)
    S, A, O, R = 4, 8, 8, 1
    rs = rng.integers(0, S, (S, A, R))
    rto = rng.random((S, A, O, R))
    rto /= rto.sum(axis=(2, 3), keepdims=True)
    m = tables(S, A, O, R, rs, rto)
    b = mc.sparse_beliefs(rng, 4000, S, density=0.7)
    eng = make_engine(m, 'f32')
    prev = engine_mod.debug_alloc_limit(2)
    try:
        eng.set_beliefs(b)
        with pytest.raises(MemoryError):                          # (Engine._ck has called pbvi_engine_after_oom)
            eng.infotaxis_resident()
        assert eng.B == 0
        engine_mod.debug_alloc_limit(prev)
        eng.set_beliefs(b[:9])
        g, act = eng.infotaxis_resident()
        mh, bh = held(m, b[:9], 'f32')
        G, _, _, MG, _ = pomdp_mod._infotaxis_terms(mh, bh)
        assert np.all(np.abs(g - G) <= bound(S, MG)) and np.array_equal(act, infotaxis_first_argmin(g))
    finally:
        engine_mod.debug_alloc_limit(prev)
        eng.close()


def replay(c, dtype, first_id, out, rows=slice(None)):
    """``test_device_rollout.replay`` for the infotaxis policy: the simulator part exactly, the recorded action's host G
    within ``VALUE_TOL[dtype] * M`` of the host minimum at the host-replayed belief; returns the surviving host beliefs."""
    states, actions, observations, steps = out
    m, _, b0 = tdr.as_engine_holds(c, dtype)
    O, R = m.observation_count, m.reachable_state_count
    rto = m.reachable_transitional_observation_table.reshape(m.state_count, m.action_count, O * R)
    ends = np.zeros(m.state_count, dtype=bool)
    ends[m.end_states] = True
    s0 = c.s0[rows]
    n, T = s0.size, actions.shape[0]
    assert states.shape == (T + 1, n) and actions.shape == observations.shape == (T, n) and steps.shape == (n,)
    assert np.array_equal(states[0], s0)
    block = pomdp_mod._HostBeliefBlock(m, None, b0[rows].copy())
    alive, s = np.arange(n), s0.astype(np.int64)
    want_steps = np.full(n, T)
    worst = 0.0
    for t in range(T):
        if alive.size == 0:
            break
        a = actions[t, alive].astype(np.int64)
        assert np.all((a >= 0) & (a < m.action_count)), t
        G, _, _, MG, _ = pomdp_mod._infotaxis_terms(m, block.b)
        rows_ = np.arange(alive.size)
        gap = (G[rows_, a] - G.min(axis=1)) / np.maximum(MG[rows_, a], 1e-300)
        worst = max(worst, float(gap.max()))
        assert np.all(gap <= VALUE_TOL[dtype]), (t, float(gap.max()))
        k = rollout_draw(rto[s, a], rollout_uniform(SEED, np.uint64(first_id) + alive.astype(np.uint64), t))
        sn = m.reachable_states[s, a, k % R]
        assert np.array_equal(observations[t, alive], k // R), t
        assert np.array_equal(states[t + 1, alive], sn), t
        done = ends[sn]
        want_steps[alive[done]] = t + 1
        block.advance(a, k // R, ~done)
        if dtype == 'f32':
            block.b = r32(block.b)                                                 # the engine stores fp32 beliefs
        alive, s = alive[~done], sn[~done]
    print(f'largest G gap of a recorded action: {worst:.3e} of M (bar {VALUE_TOL[dtype]:.0e})')
    assert np.array_equal(steps, want_steps)
    _assert_padding(states, actions, observations, steps, m.end_states)
    return block.b if alive.size else np.zeros((0, m.state_count))


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('name', CASES)
def test_device_rollout_replays_on_the_host(name, dtype):
    c = get_case(name)
    eng = make_engine(c.m, dtype)
    try:
        eng.set_beliefs(c.b0)
        out = eng.rollout_infotaxis(c.s0, end_mask(c.m), SEED, T_STEPS, first_sim_id=1000)
        assert all(x.dtype == np.int32 for x in out)
        want_b = replay(c, dtype, 1000, out)
        running = int(np.sum(~np.isin(out[0][out[3], np.arange(N_SIM)], c.m.end_states)))
        assert want_b.shape[0] == running
        assert eng.B == running == int(eng._lib.pbvi_beliefs_count(eng._h))
        if running:
            got = eng.fetch_beliefs().astype(np.float64)
            err = float(np.abs(got - want_b).max())
            print(f'largest belief difference after {T_STEPS} steps: {err:.3e} (bar {BELIEF_TOL[dtype]:.0e})')
            np.testing.assert_allclose(got, want_b, rtol=BELIEF_TOL[dtype], atol=BELIEF_TOL[dtype])
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_rollout_does_not_depend_on_blocking(dtype):
    c = get_case('olf_R5')
    eng = make_engine(c.m, dtype)
    try:
        def run(lo, hi):
            eng.set_beliefs(c.b0[lo:hi])
            out = eng.rollout_infotaxis(c.s0[lo:hi], end_mask(c.m), SEED, T_STEPS, first_sim_id=lo)
            return out, (eng.fetch_beliefs() if eng.B else np.zeros((0, c.m.state_count)))
        (whole, b_whole), (first, b_first), (second, b_second) = run(0, N_SIM), run(0, 100), run(100, N_SIM)
        for k in range(4):
            assert np.array_equal(whole[k], np.concatenate([first[k], second[k]], axis=-1)), k
        np.testing.assert_allclose(b_whole, np.concatenate([b_first, b_second]), rtol=BELIEF_TOL[dtype], atol=BELIEF_TOL[dtype])
    finally:
        eng.close()


def ragged_agent_model():
    """A ``Model`` over ``mc.ragged_model(37)``'s random tables: no two actions tie at a visited belief."""
    S = 37
    rs, rto = mc.ragged_model(S, O=3)
    A, O = rto.shape[1], rto.shape[2]
    model = Model(states=S, actions=A, observations=O, reachable_states=rs, end_states=[3, 11],
                  start_probabilities=list(np.full(S, 1.0 / S)))
    model.reachable_probabilities = rto.sum(axis=2)
    model.reachable_transitional_observation_table = rto
    return model


@pytest.mark.gpu
def test_agent_gpu_equals_host():
    """Infotaxis_Agent: the same histories from the counter-based rollout with the model on the GPU (fp64 engine) and on
    the host, the same actions for a block of beliefs, and a default (NumPy stream) run with the block on the device."""
    model = ragged_agent_model()
    n, T = 300, 40
    np.random.seed(4)
    start = [int(s) for s in np.random.choice(model.state_count, size=n, p=model.start_probabilities)]
    gm = model.to_gpu('f64')
    pair = []
    for agent in (Infotaxis_Agent(model), Infotaxis_Agent(gm)):
        totals, hists = agent.run_n_simulations_parallel(n=n, max_steps=T, start_states=start, print_progress=False,
                                                         print_stats=False, device_rng_seed=7)
        pair.append((list(totals), [(h.states, h.actions, h.observations, list(h.rewards)) for h in hists]))
    assert pair[0] == pair[1]
    assert any(len(h[1]) < T for h in pair[0][1])
    b = host_beliefs(pomdp_mod._rollout_tables(model), 9, 5)
    assert np.array_equal(Infotaxis_Agent(gm).get_best_action(b), Infotaxis_Agent(model).get_best_action(b))
    runs = []
    for agent in (Infotaxis_Agent(model), Infotaxis_Agent(gm)):
        np.random.seed(6)
        _, hists = agent.run_n_simulations_parallel(n=50, max_steps=20, print_progress=False, print_stats=False)
        runs.append([(h.states, h.actions, h.observations) for h in hists])
    assert runs[0] == runs[1]
