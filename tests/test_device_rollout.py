"""Device-resident policy rollouts: ``pbvi_rollout`` / ``Engine.rollout`` and their host restatement ``rollout_numpy``.

The draws are counter-based -- simulation ``i`` uses ``u(i, t) = uniform01(splitmix64(seed, i), t)`` at step ``t`` and one
sequential fp64 prefix sum over ``RTO[s, a, :, :]`` -- so the simulator part of a trajectory is an exact function of the
recorded ``(s, a)`` and is compared exactly.  Action selection goes through GEMMs whose summation order differs between
host and device, so the GPU tests REPLAY the device's trajectories on the host instead of comparing them lock-step with
the host's own argmax: the recorded action must be worth the host maximum at the project's parity bars (1e-12 relative for
fp64 engines, 1e-6 for fp32 ones), at the host-replayed belief.
"""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import model_cases as mc
from pomdp_pbvi_exploration_amd import pomdp as pomdp_mod
from pomdp_pbvi_exploration_amd import synth
from pomdp_pbvi_exploration_amd.pomdp import (Agent, Model, SimulationSet, ValueFunction, load_POMDP_file, rollout_draw,
                                              rollout_numpy, rollout_uniform)

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
N_SIM, T_STEPS, SEED = 257, 40, 20240607
VALUE_TOL = {'f64': 1e-12, 'f32': 1e-6}
BELIEF_TOL = {'f64': 1e-10, 'f32': 1e-5}
CASES = ['tiger', 'grid4x3', 'ragged', 'duplicate', 'olf_R1', 'olf_R5']


def r32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


# --------------------------------------------------------------------------------------------------------------------- #
# cases: tables under Model's attribute names, an alpha set with actions, start beliefs and start states (seeded, built once)
# --------------------------------------------------------------------------------------------------------------------- #
_CASES = {}


def _tables(S, A, O, R, rs, rto, er, end_states):
    return SimpleNamespace(state_count=S, action_count=A, observation_count=O, reachable_state_count=R,
                           reachable_states=np.asarray(rs, dtype=np.int64), reachable_transitional_observation_table=np.asarray(rto),
                           expected_rewards_table=np.asarray(er), end_states=list(end_states))


def grid_model():
    model, solver = load_POMDP_file(os.path.join(GOLDEN, 'models', '4x3.95-no_loop_2_grid.POMDP'))
    model.end_states = [3, 6]
    return model, solver.gamma


def get_case(name):
    """SimpleNamespace(m = tables, gamma, alpha [V,S], acts [V], b0 [n,S], s0 [n])"""
    if name in _CASES:
        return _CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    if name in ('tiger', 'grid4x3'):
        if name == 'tiger':
            model, solver = load_POMDP_file(os.path.join(GOLDEN, 'models', 'tiger.95.POMDP'))
            gamma = solver.gamma
        else:
            model, gamma = grid_model()
        m = pomdp_mod._rollout_tables(model)
        start = np.asarray(model.start_probabilities, dtype=np.float64)
        V = 12
        alpha = rng.normal(size=(V, m.state_count))
        acts = rng.integers(0, m.action_count, V)
    elif name in ('ragged', 'duplicate'):
        S = 37
        rs, rto = mc.ragged_model(S, O=3) if name == 'ragged' else mc.duplicate_successor_model(S)
        A, O, R = rto.shape[1], rto.shape[2], rto.shape[3]
        m = _tables(S, A, O, R, rs, rto, rng.normal(size=(S, A)), [3, 11])
        gamma = 0.95
        start = np.full(S, 1.0 / S)
        V = 9
        alpha = rng.normal(size=(V, S))
        acts = rng.integers(0, A, V)
    else:
        sm = synth.olfactory_model(H=15, W=40, R=int(name[-1]), f32=True)
        m = pomdp_mod._rollout_tables(sm)
        gamma = sm.gamma
        start = sm.start_belief
        alpha, acts = synth.alpha_set(sm, 33)
    b0 = np.repeat(start[None, :], N_SIM, axis=0)
    s0 = rng.choice(m.state_count, size=N_SIM, p=start / start.sum())
    _CASES[name] = SimpleNamespace(m=m, gamma=float(gamma), alpha=alpha, acts=np.asarray(acts, dtype=np.int64), b0=b0, s0=s0)
    return _CASES[name]


def end_mask(m):
    mask = np.zeros(m.state_count, dtype=np.uint8)
    mask[np.asarray(m.end_states, dtype=np.int64)] = 1
    return mask


# --------------------------------------------------------------------------------------------------------------------- #
# host (no GPU)
# --------------------------------------------------------------------------------------------------------------------- #
def test_uniform_range_and_repeatability():
    ids = np.arange(1000, dtype=np.uint64)[:, None] + np.uint64(1 << 40)
    t = np.arange(50)[None, :]
    u = rollout_uniform(SEED, ids, t)
    assert u.dtype == np.float64 and u.shape == (1000, 50)
    assert u.min() >= 0.0 and u.max() < 1.0
    assert np.array_equal(u, rollout_uniform(SEED, ids, t))
    assert u[17, 9] == rollout_uniform(SEED, int(ids[17, 0]), 9)                       # element by element = as an array
    assert u[17, 9] == synth.uniform01(int(synth.splitmix64(SEED, ids[17, 0])), 9)     # the definition, spelled out
    assert not np.array_equal(u, rollout_uniform(SEED + 1, ids, t))
    assert abs(u.mean() - 0.5) < 5 * np.sqrt(1.0 / 12.0 / u.size)


def test_streams_are_distinct():
    u = rollout_uniform(SEED, np.arange(100, dtype=np.uint64)[:, None], np.arange(100)[None, :])
    assert np.unique(u).size == 10000


def _law_case(name):
    """(weights [O*R] fp64, outcome of each k as s' * O + o) for one (s, a) with at least three possible (s', o)."""
    c = get_case(name)
    m = c.m
    O, R = m.observation_count, m.reachable_state_count
    rto = m.reachable_transitional_observation_table.reshape(m.state_count, m.action_count, O * R)
    for s in range(m.state_count):
        for a in range(m.action_count):
            k = np.arange(O * R)
            outcome = m.reachable_states[s, a, k % R] * O + k // R
            if np.unique(outcome[rto[s, a] > 0]).size >= 3:
                return rto[s, a], outcome
    raise AssertionError('no (s, a) with three outcomes')


@pytest.mark.parametrize('name', ['tiger', 'ragged'])
def test_draw_has_the_law_of_the_table(name):
    """N draws through rollout_numpy's sampler at one (s, a): every (s', o) outcome's frequency within 5 standard
    deviations of a binomial proportion, 5 * sqrt(p (1 - p) / N), of its RTO mass; outcomes of mass 0 never occur."""
    N = 200000
    w, outcome = _law_case(name)
    u = rollout_uniform(SEED, np.arange(N, dtype=np.uint64), 3)
    k = rollout_draw(np.broadcast_to(w, (N, w.size)), u)
    assert not np.any(w[k] == 0.0)
    total = w.sum()
    drawn = outcome[k]
    for oc in np.unique(outcome):
        p = w[outcome == oc].sum() / total
        freq = np.mean(drawn == oc)
        if p == 0.0:
            assert freq == 0.0
        else:
            assert abs(freq - p) <= 5.0 * np.sqrt(p * (1.0 - p) / N), (name, oc, p, freq)


def test_draw_edges():
    w = np.array([[0.0, 0.25, 0.0, 0.75, 0.0]])
    assert rollout_draw(w, np.array([0.0]))[0] == 1                      # u = 0 skips the leading zero weight
    assert rollout_draw(w, np.array([0.25]))[0] == 3                     # u * total == c[k] moves on (strict <)
    assert rollout_draw(w, np.array([np.nextafter(1.0, 0.0)]))[0] == 3
    assert rollout_draw(w, np.array([1.0]))[0] == 3                      # nothing satisfies <: the last positive entry
    with pytest.raises(ValueError):
        rollout_draw(np.zeros((1, 4)), np.array([0.5]))


@pytest.mark.parametrize('lookahead', [0, 1])
def test_chunks_give_the_unchunked_answer(lookahead):
    c = get_case('olf_R5')
    run = lambda lo, hi: rollout_numpy(c.m, c.alpha, c.acts, c.b0[lo:hi], c.s0[lo:hi], SEED, lo, 12, lookahead, c.gamma)
    whole, first, second = run(0, 50), run(0, 20), run(20, 50)
    for k in range(4):
        assert np.array_equal(whole[k], np.concatenate([first[k], second[k]], axis=-1)), k
    assert not np.array_equal(whole[2], rollout_numpy(c.m, c.alpha, c.acts, c.b0[:50], c.s0[:50], SEED + 1, 0, 12, lookahead, c.gamma)[2])


def _assert_padding(states, actions, observations, steps, ends):
    T, n = actions.shape
    for i in range(n):
        k = int(steps[i])
        assert 1 <= k <= T
        assert np.all(states[:k + 1, i] >= 0) and np.all(actions[:k, i] >= 0) and np.all(observations[:k, i] >= 0)
        assert np.all(states[k + 1:, i] == -1) and np.all(actions[k:, i] == -1) and np.all(observations[k:, i] == -1)
        assert not np.any(np.isin(states[1:k, i], ends))                # no step is taken after entering an end state
        assert k == T or states[k, i] in ends                           # stopped early = entered one


def test_done_semantics_on_the_grid():
    c = get_case('grid4x3')
    states, actions, observations, steps = rollout_numpy(c.m, c.alpha, c.acts, c.b0, c.s0, SEED, 0, T_STEPS, 0, c.gamma)
    assert states.dtype == actions.dtype == observations.dtype == steps.dtype == np.int32
    assert np.array_equal(states[0], c.s0)
    _assert_padding(states, actions, observations, steps, c.m.end_states)
    assert np.any(steps < T_STEPS)                                  # some simulations do finish early here


def _grid_agent():
    model, gamma = grid_model()
    rng = np.random.default_rng(5)
    vf = ValueFunction(model, rng.normal(size=(12, model.state_count)), rng.integers(0, model.action_count, 12).astype(int))
    return model, vf, gamma


def test_agent_seam_on_the_host():
    model, vf, gamma = _grid_agent()
    n, T = 60, 30
    agent = Agent(model, vf)
    np.random.seed(3)
    totals, hists = agent.run_n_simulations_parallel(n=n, max_steps=T, print_progress=False, print_stats=False, device_rng_seed=11)
    s0 = np.array([h.states[0] for h in hists])
    b0 = np.repeat(np.asarray(model.start_probabilities, dtype=np.float64)[None, :], n, axis=0)
    states, actions, observations, steps = rollout_numpy(model, vf.alpha_vector_array, vf.actions, b0, s0, 11, 0, T)
    sims = SimulationSet(model)
    assert len(hists) == n and len(totals) == n
    for i, h in enumerate(hists):
        k = int(steps[i])
        assert len(h.actions) == len(h.observations) == len(h.rewards) == k and len(h.states) == k + 1
        assert h.states == states[:k + 1, i].tolist() and h.actions == actions[:k, i].tolist()
        assert h.observations == observations[:k, i].tolist()
        want = sims._step_rewards(states[:k, i].astype(int), actions[:k, i].astype(int), states[1:k + 1, i].astype(int),
                                  observations[:k, i].astype(int))
        assert np.array_equal(np.asarray(h.rewards, dtype=np.float64), np.asarray(want, dtype=np.float64))
        assert totals[i] == pytest.approx(float(np.sum(want)), rel=1e-12, abs=1e-12)      # (a sum in another order)
    # same seed, same trajectories, whatever NumPy's global stream holds (the start states were given)
    np.random.seed(99)
    _, again = agent.run_n_simulations_parallel(n=n, max_steps=T, start_states=[int(s) for s in s0], print_progress=False,
                                                print_stats=False, device_rng_seed=11)
    assert all(a.states == h.states and a.actions == h.actions and a.observations == h.observations for a, h in zip(again, hists))


def test_default_path_is_untouched():
    """device_rng_seed=None is the method as it was: same trajectories under the same np.random.seed, with the keyword
    spelled out or left out."""
    model, vf, _ = _grid_agent()
    agent = Agent(model, vf)
    runs = []
    for kw in ({}, {'device_rng_seed': None}, {}):
        np.random.seed(21)
        totals, hists = agent.run_n_simulations_parallel(n=40, max_steps=25, print_progress=False, print_stats=False, **kw)
        runs.append((list(totals), [(h.states, h.actions, h.observations, list(h.rewards)) for h in hists]))
    assert runs[0] == runs[1] == runs[2]


def test_host_rollout_rejects_bad_arguments():
    c = get_case('tiger')
    ok = dict(model=c.m, alpha=c.alpha, alpha_actions=c.acts, beliefs=c.b0[:4], start_states=c.s0[:4], seed=1, first_sim_id=0, T=3)
    rollout_numpy(**ok)
    for bad in (dict(T=0), dict(start_states=np.array([0, 1, 2, 0])), dict(alpha_actions=c.acts + 3), dict(lookahead=2), dict(seed=-1)):
        with pytest.raises(ValueError):
            rollout_numpy(**{**ok, **bad})


# --------------------------------------------------------------------------------------------------------------------- #
# device
# --------------------------------------------------------------------------------------------------------------------- #
def make_engine(c, dtype, mode='sparse'):
    from pomdp_pbvi_exploration_amd.engine import Engine
    m = c.m
    eng = Engine(m.state_count, m.action_count, m.observation_count, m.reachable_state_count, m.reachable_states,
                 m.reachable_transitional_observation_table, m.expected_rewards_table, dtype=dtype, mode=mode)
    eng.set_alpha(c.alpha)
    return eng


def as_engine_holds(c, dtype):
    """The case's tables, alpha set and start beliefs in the engine's number format, back in fp64."""
    if dtype == 'f64':
        return c.m, c.alpha, c.b0
    m = SimpleNamespace(**vars(c.m))
    m.reachable_transitional_observation_table = r32(m.reachable_transitional_observation_table)
    m.expected_rewards_table = r32(m.expected_rewards_table)
    return m, r32(c.alpha), r32(c.b0)


def replay(c, dtype, lookahead, first_id, out, rows=slice(None)):
    """Replays a device rollout on the host, step by step, and checks every (simulation, step); returns the host-replayed
    beliefs of the simulations still running."""
    states, actions, observations, steps = out
    m, alpha, b0 = as_engine_holds(c, dtype)
    O, R = m.observation_count, m.reachable_state_count
    rto = m.reachable_transitional_observation_table.reshape(m.state_count, m.action_count, O * R)
    ends = np.zeros(m.state_count, dtype=bool)
    ends[m.end_states] = True
    s0 = c.s0[rows]
    n, T = s0.size, actions.shape[0]
    assert states.shape == (T + 1, n) and actions.shape == observations.shape == (T, n) and steps.shape == (n,)
    assert np.array_equal(states[0], s0)
    block = pomdp_mod._HostBeliefBlock(m, SimpleNamespace(alpha_vector_array=alpha), b0[rows].copy())
    alive, s = np.arange(n), s0.astype(np.int64)
    want_steps = np.full(n, T)
    worst = 0.0
    for t in range(T):
        if alive.size == 0:
            break
        a = actions[t, alive].astype(np.int64)
        assert np.all((a >= 0) & (a < m.action_count)), t
        # (b) the recorded action is worth the host maximum at the host-replayed belief
        if lookahead == 0:
            scores = block.b @ alpha.T                                             # [alive, V]
            of_action = np.where(c.acts[None, :] == a[:, None], scores, -np.inf).max(axis=1)
            best, scale = scores.max(axis=1), np.abs(scores).max(axis=1)
        else:
            q = pomdp_mod._q_values_numpy(m, block.b, alpha, c.gamma)
            of_action, best, scale = q[np.arange(alive.size), a], q.max(axis=1), np.abs(q).max(axis=1)
        gap = (best - of_action) / np.maximum(scale, 1e-300)
        worst = max(worst, float(gap.max()))
        assert np.all(gap <= VALUE_TOL[dtype]), (t, float(gap.max()))
        # (a) the recorded (s', o) is the definition's for the recorded s, a and u(i, t)
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
    print(f'largest value gap of a recorded action: {worst:.3e} (bar {VALUE_TOL[dtype]:.0e})')
    assert np.array_equal(steps, want_steps)
    _assert_padding(states, actions, observations, steps, m.end_states)
    return block.b if alive.size else np.zeros((0, m.state_count))


@pytest.mark.gpu
@pytest.mark.parametrize('lookahead', [0, 1])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('name', CASES)
def test_device_rollout_replays_on_the_host(name, dtype, lookahead):
    c = get_case(name)
    eng = make_engine(c, dtype)
    try:
        eng.set_beliefs(c.b0)
        out = eng.rollout(c.acts, c.s0, end_mask(c.m), SEED, T_STEPS, first_sim_id=1000, lookahead=lookahead, gamma=c.gamma)
        assert all(x.dtype == np.int32 for x in out)
        want_b = replay(c, dtype, lookahead, 1000, out)
        # (c) the resident block: the survivors' beliefs in caller order
        running = int(np.sum(~np.isin(out[0][out[3], np.arange(N_SIM)], c.m.end_states)))
        assert want_b.shape[0] == running
        assert eng.B == running == int(eng._lib.pbvi_beliefs_count(eng._h))
        if running:
            got = eng.fetch_beliefs().astype(np.float64)
            err = float(np.abs(got - want_b).max())
            print(f'largest belief difference after {T_STEPS} steps: {err:.3e} (bar {BELIEF_TOL[dtype]:.0e})')
            np.testing.assert_allclose(got, want_b, rtol=BELIEF_TOL[dtype], atol=BELIEF_TOL[dtype])
        if name in ('grid4x3', 'olf_R5'):
            assert running < N_SIM                                # the done-filter ran
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('lookahead', [0, 1])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_result_does_not_depend_on_blocking(dtype, lookahead):
    """One call on 257 rows (a sorted block of two GEMM row tiles) = two calls on 100 and 157 rows with first_sim_id 0 / 100,
    exactly, in every output.  (The engine drops finished rows after every step and has no knob for it.)"""
    c = get_case('olf_R5')
    eng = make_engine(c, dtype)
    try:
        def run(lo, hi):
            eng.set_beliefs(c.b0[lo:hi])
            out = eng.rollout(c.acts, c.s0[lo:hi], end_mask(c.m), SEED, T_STEPS, first_sim_id=lo, lookahead=lookahead, gamma=c.gamma)
            return out, (eng.fetch_beliefs() if eng.B else np.zeros((0, c.m.state_count)))
        (whole, b_whole), (first, b_first), (second, b_second) = run(0, N_SIM), run(0, 100), run(100, N_SIM)
        for k in range(4):
            assert np.array_equal(whole[k], np.concatenate([first[k], second[k]], axis=-1)), k
        assert np.any(whole[3] < T_STEPS)
        np.testing.assert_allclose(b_whole, np.concatenate([b_first, b_second]), rtol=BELIEF_TOL[dtype], atol=BELIEF_TOL[dtype])
    finally:
        eng.close()


@pytest.mark.gpu
def test_backup_after_a_rollout_is_the_fresh_engines():
    c = get_case('olf_R5')
    eng, fresh = make_engine(c, 'f32'), make_engine(c, 'f32')
    try:
        eng.set_beliefs(c.b0)
        eng.rollout(c.acts, c.s0, end_mask(c.m), SEED, 6, lookahead=1, gamma=c.gamma)
        block = eng.fetch_beliefs()
        assert 0 < block.shape[0] == eng.B
        eng.run(c.gamma)
        got = eng.fetch()
        fresh.set_beliefs(block)
        fresh.run(c.gamma)
        want = fresh.fetch()
        assert np.array_equal(got.actions, want.actions) and np.array_equal(got.best_alpha_ind, want.best_alpha_ind)
        assert np.array_equal(got.alpha, want.alpha)
        assert eng.alpha_count == c.alpha.shape[0]
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
def test_trajectory_buffers_obey_the_allocation_cap():
    from pomdp_pbvi_exploration_amd import engine as engine_mod
    c = get_case('tiger')
    eng = make_engine(c, 'f64')
    prev = engine_mod.debug_alloc_limit(64)                       # 64 MiB; the trajectories of 200000 steps need 590 MiB
    try:
        eng.set_beliefs(c.b0)
        with pytest.raises(MemoryError):                          # (Engine._ck has called pbvi_engine_after_oom)
            eng.rollout(c.acts, c.s0, end_mask(c.m), SEED, 200000)
        assert eng.B == 0 and eng.alpha_count == 0
        engine_mod.debug_alloc_limit(prev)
        eng.set_alpha(c.alpha)
        eng.set_beliefs(c.b0)
        out = eng.rollout(c.acts, c.s0, end_mask(c.m), SEED, 5, first_sim_id=1000)
        replay(c, 'f64', 0, 1000, out)
    finally:
        engine_mod.debug_alloc_limit(prev)
        eng.close()


@pytest.mark.gpu
def test_argument_errors():
    c = get_case('grid4x3')
    i32p, u8p = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    acts, s0, mask = c.acts.astype(np.int32), c.s0.astype(np.int32), end_mask(c.m)

    def call(eng, acts=acts, s0=s0, lookahead=0, T=5):
        rc = eng._lib.pbvi_rollout(eng._h, acts.ctypes.data_as(i32p), lookahead, c.gamma, s0.ctypes.data_as(i32p),
                                   mask.ctypes.data_as(u8p), 0, SEED, T, None, None, None, None)
        return rc, eng._lib.pbvi_last_error().decode()

    eng = make_engine(c, 'f64')
    dense = make_engine(c, 'f64', mode='dense')
    try:
        rc, msg = call(eng)
        assert rc == -1 and 'belief' in msg                      # no resident block yet
        eng.set_beliefs(c.b0)
        dense.set_beliefs(c.b0)
        bad_state, bad_action = s0.copy(), acts.copy()
        bad_state[200] = c.m.state_count
        bad_action[-1] = c.m.action_count
        for kw, code, word in ((dict(s0=bad_state), -1, 'start state'), (dict(acts=bad_action), -1, 'alpha_actions'),
                               (dict(T=0), -1, 'T'), (dict(lookahead=2), -1, 'lookahead'),
                               (dict(T=(1 << 31) // N_SIM + 1), -4, 'int32')):
            rc, msg = call(eng, **kw)
            assert rc == code and word in msg, (kw.keys(), rc, msg)
            assert eng._lib.pbvi_beliefs_count(eng._h) == N_SIM   # nothing ran: the block is as it was
        rc, msg = call(dense, lookahead=1)
        assert rc == -4 and 'PBVI_DENSE' in msg
        assert call(dense, lookahead=0)[0] == 0                  # the reference policy runs on a dense engine
        assert call(eng)[0] == 0
    finally:
        eng.close()
        dense.close()


@pytest.mark.gpu
def test_agent_seam_gpu_equals_host():
    """Agent.run_n_simulations_parallel(n=300, device_rng_seed=7) on the 4x3 grid: the same histories with the value function
    on the GPU (fp64 engine) and on the host.  (Twelve seeded normal alpha rows: no two actions tie at a visited belief.)"""
    model, vf, gamma = _grid_agent()
    n, T = 300, 40
    np.random.seed(4)
    start = [int(s) for s in np.random.choice(model.state_count, size=n, p=model.start_probabilities)]
    results = []
    for lookahead in (0, 1):
        host = Agent(model, vf, lookahead=lookahead, gamma=gamma)
        gm = model.to_gpu('f64')
        dev = Agent(gm, ValueFunction(model, vf.alpha_vector_array, vf.actions).to_gpu(), lookahead=lookahead, gamma=gamma)
        pair = []
        for agent in (host, dev):
            totals, hists = agent.run_n_simulations_parallel(n=n, max_steps=T, start_states=start, print_progress=False,
                                                             print_stats=False, device_rng_seed=7)
            pair.append((list(totals), [(h.states, h.actions, h.observations, list(h.rewards)) for h in hists]))
        assert pair[0] == pair[1], lookahead
        assert any(len(h[1]) < T for h in pair[0][1])
        results.append(pair[0])
