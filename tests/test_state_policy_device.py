"""State policies on the device: ``pbvi_state_policy_set`` / ``pbvi_state_policy`` / ``pbvi_rollout_state_policy`` against
the host statements ``state_policy_numpy`` / ``rollout_state_policy_numpy``.

The definition (include/pbvi_hip.h) fixes the order of every add, so actions, states and the BITS of the votes are compared
exactly: there is no tolerance in the one-shot call.  A rollout is compared entry for entry with the host's; only the
beliefs left in the block after it pass through Bayes steps whose sums the device takes in another order, and are held to
``test_device_rollout``'s belief bars.

The voting and Thompson walks take the chunks in groups of 128 (32768 states): the tests "past one chunk group" run every
rule with two and three groups, with a last group of one chunk, on the rows of ``state_policy_cases.seam_rows``, whose host
side ``test_state_policy`` holds to the loop definitions and shows to catch a wrong grouping."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import model_cases as mc
import state_policy_cases as spc
import test_device_rollout as tdr
import test_infotaxis as tit
import test_rollout_env as tre
from pomdp_pbvi_exploration_amd import pomdp as pomdp_mod
from pomdp_pbvi_exploration_amd import synth
from pomdp_pbvi_exploration_amd.pomdp import (FrameEnvironment, SimulationSet, StatePolicy_Agent, TableEnvironment,
                                              rollout_state_policy_numpy, rollout_uniform, state_policy_numpy)
from test_device_rollout import BELIEF_TOL, CASES, SEED, T_STEPS, _assert_padding, end_mask, get_case

NP_DTYPE = {'f64': np.float64, 'f32': np.float32}
T_ROLL = 12


def case_table(name, seed=0):
    m = get_case(name).m
    return spc.action_table(m.state_count, m.action_count, seed)


def block_rows(S, n, seed=0):
    """``n`` rows: ``state_policy_cases.belief_rows`` (chunk edges, one-hots, ties, all mass in the last chunk) filled up with
    sparse rows."""
    edge = spc.belief_rows(S, seed)
    rng = np.random.default_rng(50 + S + seed)
    fill = mc.sparse_beliefs(rng, max(n - edge.shape[0], 1), S, density=0.1)
    return np.concatenate([edge, fill])[:n]


def given_uniforms(n):
    u = np.random.default_rng(n).random(n)
    u[:len(spc.UNIFORMS)] = spc.UNIFORMS[:n]
    u[-1] = 1.0
    return u


def check_one_shot(eng, b, sa, A, dtype, tag, every_row=()):
    """Every rule, hashed and given uniforms, on the resident block ``b``; each uniform of ``every_row`` given to every row."""
    n = b.shape[0]
    npdt = NP_DTYPE[dtype]
    eng.set_state_policy(sa)
    eng.set_beliefs(b)
    act, st = eng.state_policy_resident(0, want_state=True)
    want = state_policy_numpy(b, sa, 0, table_dtype=npdt)
    assert np.array_equal(act, want[0]) and np.array_equal(st, want[1]), (tag, 'mls')
    act, st, votes = eng.state_policy_resident(1, want_state=True, want_votes=True)
    want = state_policy_numpy(b, sa, 1, table_dtype=npdt, action_count=A)
    assert votes.shape == (n, A) and votes.tobytes() == want[2].tobytes(), (tag, 'votes', float(np.abs(votes - want[2]).max()))
    assert np.array_equal(act, want[0]) and np.all(st == -1), (tag, 'voting')
    assert np.array_equal(eng.state_policy_resident(1), act)                       # the short form, and a second call
    for seed, first, t in ((SEED, 0, 0), (SEED + 1, 1 << 40, 7), (3, 5, (1 << 31) - 1)):
        u = rollout_uniform(seed, np.uint64(first) + np.arange(n, dtype=np.uint64), (1 << 33) + t)
        act, st = eng.state_policy_resident(2, seed=seed, first_sim_id=first, t=t, want_state=True)
        want = state_policy_numpy(b, sa, 2, u, table_dtype=npdt)
        assert np.array_equal(st, want[1]) and np.array_equal(act, want[0]), (tag, 'thompson hashed', seed)
    u = given_uniforms(n)
    act, st = eng.state_policy_resident(2, uniforms=u, want_state=True)
    want = state_policy_numpy(b, sa, 2, u, table_dtype=npdt)
    assert np.array_equal(st, want[1]) and np.array_equal(act, want[0]), (tag, 'thompson given')
    held = b.astype(npdt).astype(np.float64)
    assert np.all(held[np.arange(n), st] > 0)                                      # the drawn state has mass
    for x in (0.0, 1.0):
        st = eng.state_policy_resident(2, uniforms=np.full(n, x), want_state=True)[1]
        edge = [np.flatnonzero(row > 0)[0 if x == 0.0 else -1] for row in held]
        assert np.array_equal(st, edge), (tag, x)
    for x in every_row:
        act, st = eng.state_policy_resident(2, uniforms=np.full(n, x), want_state=True)
        want = state_policy_numpy(b, sa, 2, np.full(n, x), table_dtype=npdt)
        assert np.array_equal(st, want[1]) and np.array_equal(act, want[0]), (tag, x, np.flatnonzero(st != want[1]))
    assert eng.B == n


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('name', CASES)
def test_one_shot_on_the_named_models(name, dtype):
    c = get_case(name)
    S, A = c.m.state_count, c.m.action_count
    eng = tit.make_engine(c.m, dtype)
    try:
        b = np.concatenate([c.b0[:2], block_rows(S, 255)])                        # 257 rows: a sorted block
        check_one_shot(eng, b, case_table(name), A, dtype, name)
        check_one_shot(eng, b[:5], case_table(name, 1), A, dtype, name + '-5')
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('S,A', [(255, 9), (256, 17), (257, 9), (513, 17)])
def test_one_shot_on_bare_blocks(S, A, dtype):
    """Chunk edges at more than one register tile of actions (9 and 17 > 8), on a small random model."""
    rs, rto = mc.ragged_model(S, A=A, O=2)
    m = tit.tables(S, A, 2, rto.shape[3], rs, rto)
    eng = tit.make_engine(m, dtype)
    try:
        for n in (257, 3):
            check_one_shot(eng, block_rows(S, n), spc.action_table(S, A), A, dtype, f'{S}-{A}-{n}')
        # a table that names fewer actions than the model has: the other votes are +0.0
        sa = spc.action_table(S, 3)
        eng.set_state_policy(sa)
        votes = eng.state_policy_resident(1, want_votes=True)[1]
        assert votes.tobytes() == state_policy_numpy(block_rows(S, 3), sa, 1, table_dtype=NP_DTYPE[dtype], action_count=A)[2].tobytes()
        assert not np.any(votes[:, 3:]) and not np.any(np.signbit(votes))
    finally:
        eng.close()


def seam_block(S, fill=4, seed=0):
    """``(names, rows)``: ``state_policy_cases.seam_rows`` (the boundary row first) and ``fill`` sparse rows."""
    rows = spc.seam_rows(S, seed)
    names = ['boundary'] + [k for k in rows if k != 'boundary']
    sparse = spc.r32(mc.sparse_beliefs(np.random.default_rng(60 + S + seed), fill, S, density=0.1))
    return names + ['sparse'] * fill, np.concatenate([np.array([rows[k] for k in names]), sparse])


def check_seam_one_shot(m, dtype, tag):
    """Every rule on the seam rows under the vote-tie table; every seam uniform on every row, the boundary row among them."""
    S, A = m.state_count, m.action_count
    names, b = seam_block(S)
    sa = spc.seam_tie_table(S, A)
    assert b.shape[0] <= 16
    eng = tit.make_engine(m, dtype)
    try:
        check_one_shot(eng, b, sa, A, dtype, tag, every_row=spc.SEAM_UNIFORMS)
        act, st, votes = eng.state_policy_resident(1, want_state=True, want_votes=True)
        tie = names.index('vote_tie')                             # both sides of the seam: the same bits, the lower action
        assert votes[tie, 1].tobytes() == votes[tie, A - 1].tobytes() == np.float64(0.25).tobytes() and act[tie] == 1
        assert np.count_nonzero(votes[tie]) == 2
        first, last_front, first_behind, last = spc.seam_marks(S)
        st = eng.state_policy_resident(0, want_state=True)[1]     # MLS's tie across the seam: the lowest of the equal maxima
        assert st[0] == (first if last > first_behind else first_behind)
        for u, want in ((0.5, first_behind), (float(np.nextafter(0.5, 0.0)), last_front)):
            assert eng.state_policy_resident(2, uniforms=np.full(b.shape[0], u), want_state=True)[1][0] == want, (tag, u)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('S,A', [(32767, 3), (32768, 9), (32769, 9), (65537, 17)])
def test_one_shot_past_one_chunk_group(S, A, dtype):
    """One group with a ragged last chunk, one full group, two groups (the second: one chunk of one state), three groups; 9 and
    17 actions cross the register tile of 8 and the seam in one launch."""
    rs, rto = spc.bare_model(S, A)
    check_seam_one_shot(tit.tables(S, A, 1, 1, rs, rto), dtype, f'{S}-{A}')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_one_shot_on_the_sea_robin_shape(dtype):
    """S = 61875 = 165 x 375, A = 16: two groups, the second of 114 chunks, the last of them ragged."""
    S, A, O, rs, rto, _, _, _ = synth.sea_robin_like(V=1, B=1)
    assert (S, A) == (61875, 16)
    check_seam_one_shot(tit.tables(S, A, O, 1, rs, rto), dtype, 'sea-robin')


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('S', spc.MLS_WRAP_SIZES)
def test_mls_lane_wrap_on_the_f32_engine(S, dtype):
    """Above 1024 states a lane of the fp32 engine (512: of the fp64 engine) holds more than one load, and compares its
    candidates itself: ties one lane stride apart, where the lower state must win."""
    A = 9
    rs, rto = spc.bare_model(S, A)
    b = np.concatenate([spc.belief_rows(S), spc.lane_tie_rows(S), np.array(list(spc.seam_rows(S).values()))])
    eng = tit.make_engine(tit.tables(S, A, 1, 1, rs, rto), dtype)
    try:
        check_one_shot(eng, b, spc.seam_tie_table(S, A), A, dtype, f'wrap-{S}')
        ties = spc.lane_tie_rows(S)
        eng.set_beliefs(ties)
        st = eng.state_policy_resident(0, want_state=True)[1]
        assert st.tolist() == [spc.first_greater_loop(row) for row in ties], S
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_seam_rows_do_not_depend_on_the_block(dtype):
    """At S = 32769 (two groups) the seam rows alone, reversed and inside a 257-row block, which the engine sorts: the same
    actions, states and vote bits."""
    S, A = 32769, 9
    names, b = seam_block(S, fill=0)
    n = b.shape[0]
    u = np.resize(np.array(spc.SEAM_UNIFORMS), n)                 # (the boundary row, row 0, has 0.0 here and every other one below)
    rng = np.random.default_rng(S)
    big = np.concatenate([spc.r32(mc.sparse_beliefs(rng, 257 - n, S, density=0.05)), b])
    where = rng.permutation(257)
    big_u = np.concatenate([rng.random(257 - n), u])
    rs, rto = spc.bare_model(S, A)
    eng = tit.make_engine(tit.tables(S, A, 1, 1, rs, rto), dtype)

    def every_rule(rows, uu):
        eng.set_beliefs(rows)
        return (eng.state_policy_resident(0, want_state=True) + eng.state_policy_resident(1, want_state=True, want_votes=True)
                + eng.state_policy_resident(2, uniforms=uu, want_state=True))
    try:
        sa = spc.seam_tie_table(S, A)
        eng.set_state_policy(sa)
        alone = every_rule(b, u)
        want = (state_policy_numpy(b, sa, 0, table_dtype=NP_DTYPE[dtype])[:2] + state_policy_numpy(b, sa, 1, table_dtype=NP_DTYPE[dtype], action_count=A)
                + state_policy_numpy(b, sa, 2, u, table_dtype=NP_DTYPE[dtype])[:2])
        for k in range(len(alone)):
            assert np.array_equal(alone[k], want[k]), k
        moved = every_rule(b[::-1], u[::-1])
        for k in range(len(alone)):
            assert moved[k].tobytes() == np.ascontiguousarray(alone[k][::-1]).tobytes(), k
        for x in spc.SEAM_UNIFORMS:                               # the boundary row alone, on and one ulp below every cumulative sum
            one = every_rule(b[:1], np.array([x]))
            act, st, _ = state_policy_numpy(b[:1], sa, 2, np.array([x]), table_dtype=NP_DTYPE[dtype])
            assert one[5][0] == act[0] and one[6][0] == st[0], x
        inside = every_rule(big[where], big_u[where])
        back = np.argsort(where)[257 - n:]                        # where the seam rows went
        for k in range(len(alone)):
            assert np.ascontiguousarray(inside[k][back]).tobytes() == alone[k].tobytes(), (k, names)
    finally:
        eng.close()


@pytest.mark.gpu
def test_one_shot_on_a_dense_engine():
    c = get_case('grid4x3')
    eng = tit.make_engine(c.m, 'f64', mode='dense')
    try:
        check_one_shot(eng, block_rows(c.m.state_count, 40), case_table('grid4x3'), c.m.action_count, 'f64', 'dense')
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
def test_a_rows_results_do_not_depend_on_the_block(dtype):
    """The same rows alone, reversed and inside a larger (sorted) block: the same actions, states and vote bits."""
    c = get_case('olf_R5')
    S, A = c.m.state_count, c.m.action_count
    b = block_rows(S, 257)
    u = given_uniforms(257)
    eng = tit.make_engine(c.m, dtype)

    def every_rule(rows, uu):
        eng.set_beliefs(rows)
        return (eng.state_policy_resident(0, want_state=True) + eng.state_policy_resident(1, want_state=True, want_votes=True)
                + eng.state_policy_resident(2, uniforms=uu, want_state=True))
    try:
        eng.set_state_policy(case_table('olf_R5'))
        whole = every_rule(b, u)
        for i in (0, 1, 130, 256):
            alone = every_rule(b[i:i + 1], u[i:i + 1])
            for k in range(len(whole)):
                assert alone[k][0].tobytes() == whole[k][i].tobytes(), (i, k)
        moved = every_rule(b[::-1], u[::-1])
        for k in range(len(whole)):
            assert moved[k].tobytes() == np.ascontiguousarray(whole[k][::-1]).tobytes(), k
        order = np.random.default_rng(9).permutation(257)[:6]
        few = every_rule(b[order], u[order])
        for k in range(len(whole)):
            assert few[k].tobytes() == np.ascontiguousarray(whole[k][order]).tobytes(), k
    finally:
        eng.close()


def rollout_case(name):
    """``test_device_rollout``'s case ``name`` with what ``check_rollout`` reads besides: the case's name, its table ``sa``,
    the steps ``T`` and the simulation ``cut`` at which the run is cut into two calls."""
    return SimpleNamespace(**vars(get_case(name)), name=name, sa=case_table(name), T=T_ROLL, cut=100)


def check_rollout(case, dtype, rule, kind=None):
    """One device run against the host's, entry for entry; the same run cut into two calls; the block left behind.
    ``case``: the name of a case of ``test_device_rollout``, or a case object as ``rollout_case`` returns."""
    c = rollout_case(case) if isinstance(case, str) else case
    name, sa, n, T, cut = c.name, c.sa, c.b0.shape[0], c.T, c.cut
    m, _, b0 = tdr.as_engine_holds(c, dtype)
    env = None if kind is None else tre.case_env(name, kind)
    frames = isinstance(env, FrameEnvironment)
    eng = tit.make_engine(c.m, dtype)

    def device(lo, hi):
        sub = None if env is None else env.rows(lo, hi)
        eng.set_beliefs(c.b0[lo:hi])
        out = eng.rollout_state_policy(c.s0[lo:hi], end_mask(c.m), SEED, T, first_sim_id=1000 + lo, rule=rule,
                                       use_env=env is not None,
                                       shifts=np.broadcast_to(sub.shifts, (hi - lo,)) if frames else None,
                                       end_observation=-1 if env is None else env.end_observation)
        return out, (eng.fetch_beliefs().astype(np.float64) if eng.B else np.zeros((0, m.state_count)))
    try:
        eng.set_state_policy(sa)
        if env is not None:
            tre.install(eng, env)
        got, block = device(0, n)
        want = rollout_state_policy_numpy(m, b0, c.s0, sa, rule, SEED, 1000, T, table_dtype=NP_DTYPE[dtype],
                                          return_beliefs=True, env=env)
        assert all(x.dtype == np.int32 for x in got[:4]) and len(got) == 5 and got[4].dtype == np.uint8
        for k, what in enumerate(('states', 'actions', 'observations', 'steps')):
            differ = int(np.sum(got[k] != want[k]))
            assert differ == 0, (name, dtype, rule, kind, what, differ)
        assert np.array_equal(got[4], want[5] if env is not None else np.zeros(n, dtype=np.uint8))
        if env is None:
            _assert_padding(got[0], got[1], got[2], got[3], c.m.end_states)
        for i in range(n):                                        # -1 behind the last step, in every array
            k = int(got[3][i])
            assert 1 <= k <= T and np.all(got[0][:k + 1, i] >= 0) and np.all(got[1][:k, i] >= 0) and np.all(got[2][:k, i] >= 0)
            assert np.all(got[0][k + 1:, i] == -1) and np.all(got[1][k:, i] == -1) and np.all(got[2][k:, i] == -1)
        running = int(np.sum((got[3] == T) & (got[4] == 0) & ~np.isin(got[0][-1], c.m.end_states)))
        assert running == eng.B == int(eng._lib.pbvi_beliefs_count(eng._h))
        assert block.shape == want[4].shape and eng.B == want[4].shape[0]
        if block.shape[0]:
            np.testing.assert_allclose(block, want[4], rtol=BELIEF_TOL[dtype], atol=BELIEF_TOL[dtype])
        (first, b_first), (second, b_second) = device(0, cut), device(cut, n)
        for k in range(5):
            assert np.array_equal(got[k], np.concatenate([first[k], second[k]], axis=-1)), (name, dtype, rule, kind, k)
        assert b_first.shape[0] + b_second.shape[0] == block.shape[0]
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('rule', [0, 1, 2])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('name', CASES)
def test_device_rollout_equals_the_hosts(name, dtype, rule):
    check_rollout(name, dtype, rule)


@pytest.mark.gpu
@pytest.mark.parametrize('rule', [0, 1, 2])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('name,kind', [('olf_R5', 'frames'), ('ragged', 'table')])
def test_device_rollout_against_an_environment_equals_the_hosts(name, kind, dtype, rule):
    check_rollout(name, dtype, rule, kind)


_SEAM_ROLLOUTS = {}


def seam_rollout_case(R, rows_down=0):
    """The 75 x 440 olfactory grid (S = 33000: two chunk groups, one ragged chunk in the second), 40 simulations started in
    ``synth.belief_points`` beliefs, 6 steps.  The start box of the model ends at grid row 54 and the second group begins in
    row 74, so those beliefs keep their mass in the first group; ``rows_down`` moves them down the (wrap-around) grid."""
    if (R, rows_down) not in _SEAM_ROLLOUTS:
        sm = synth.olfactory_model(H=75, W=440, R=R)
        b0 = np.roll(synth.belief_points(sm, 40), rows_down * sm.W, axis=1)
        rng = np.random.default_rng(440 + R)
        s0 = np.array([rng.choice(sm.S, p=row / row.sum()) for row in b0])
        _SEAM_ROLLOUTS[R, rows_down] = SimpleNamespace(m=pomdp_mod._rollout_tables(sm), alpha=np.zeros((1, sm.S)), b0=b0, s0=s0,
                                                       name=f'olf75x440_R{R}+{rows_down}', sa=spc.action_table(sm.S, sm.A), T=6, cut=17)
    return _SEAM_ROLLOUTS[R, rows_down]


@pytest.mark.gpu
@pytest.mark.parametrize('rule', [0, 1, 2])
@pytest.mark.parametrize('dtype', ['f64', 'f32'])
@pytest.mark.parametrize('R,rows_down', [(1, 0), (5, 0), (5, 37)])
def test_rollout_past_one_chunk_group(R, rows_down, dtype, rule):
    """``check_rollout`` with two chunk groups under every step's policy call.  Moved 37 rows down, the goal's row is the
    grid's last one: every start belief then holds 0.9 to 3 % of its mass behind the seam (the second group is 0.7 % of the
    states), which is part of every vote and every Thompson prefix, and some Thompson draws land there."""
    c = seam_rollout_case(R, rows_down)
    assert c.m.state_count == 33000 and c.b0.shape[0] == 40
    assert rows_down == 0 or np.all(c.b0[:, spc.GROUP:].sum(axis=1) > 0.005)
    check_rollout(c, dtype, rule)


@pytest.mark.gpu
def test_argument_errors():
    m = get_case('grid4x3').m
    sa = case_table('grid4x3').astype(np.int32)
    f64p, i32p, u8p, i64p = C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    eng = tit.make_engine(m, 'f64')
    try:
        lib = eng._lib
        act, u = np.empty(3, dtype=np.int32), np.array([0.0, 0.5, 1.0])
        ap, sp, up = act.ctypes.data_as(i32p), sa.ctypes.data_as(i32p), u.ctypes.data_as(f64p)
        s0, mask = np.zeros(3, dtype=np.int32), end_mask(m)
        shifts = np.zeros(3, dtype=np.int64)

        def call(rule=0, t=0, uniforms=None, out=ap):
            return lib.pbvi_state_policy(eng._h, rule, SEED, 0, t, uniforms, out, None, None)

        def roll(rule=0, use_env=0, end_observation=-1, shifts=None, T=4, lost=None):
            return lib.pbvi_rollout_state_policy(eng._h, rule, use_env, s0.ctypes.data_as(i32p), mask.ctypes.data_as(u8p),
                                                 end_observation, None if shifts is None else shifts.ctypes.data_as(i64p), 0, SEED, T,
                                                 None, None, None, None, None if lost is None else lost.ctypes.data_as(u8p))
        assert call() == -1 and b'no belief block' in lib.pbvi_last_error()
        assert roll() == -1
        eng.set_beliefs(tit.host_beliefs(m, 3, 0))
        assert call() == -1 and b'no state policy set' in lib.pbvi_last_error()
        assert roll() == -1 and b'no state policy set' in lib.pbvi_last_error()
        assert lib.pbvi_state_policy_set(eng._h, None) == -1 and b'NULL' in lib.pbvi_last_error()
        for bad, at in ((-1, 2), (m.action_count, 0), (1 << 20, m.state_count - 1)):
            sb = sa.copy()
            sb[at] = bad
            assert lib.pbvi_state_policy_set(eng._h, sb.ctypes.data_as(i32p)) == -1
            assert f'state_actions[{at}]'.encode() in lib.pbvi_last_error()
            assert call() == -1 and b'no state policy set' in lib.pbvi_last_error()
        with pytest.raises(ValueError):
            eng.set_state_policy(sa[:-1])
        assert lib.pbvi_state_policy_set(eng._h, sp) == 0
        for rule in (3, -1):
            assert call(rule=rule) == -1 and b'rule must be' in lib.pbvi_last_error()
            assert roll(rule=rule) == -1 and b'rule must be' in lib.pbvi_last_error()
        assert call(out=None) == -1 and b'NULL out_action' in lib.pbvi_last_error()
        for rule in (0, 1):
            assert call(rule=rule, uniforms=up) == -1 and b'uniforms belong to rule 2' in lib.pbvi_last_error()
        for bad in (-1e-9, np.nextafter(1.0, 2.0), np.nan):
            ub = u.copy()
            ub[1] = bad
            assert call(rule=2, uniforms=ub.ctypes.data_as(f64p)) == -1 and b'uniforms[1]' in lib.pbvi_last_error()
        for t in (-1, 1 << 31):
            assert call(rule=2, t=t) == -1 and b't must be' in lib.pbvi_last_error()
        assert call(rule=2, uniforms=up) == 0 and call(rule=2, t=(1 << 31) - 1) == 0 and call() == 0   # every optional output NULL
        assert np.array_equal(act, eng.state_policy_resident(0))
        with pytest.raises(ValueError):
            eng.state_policy_resident(0, want_votes=True)
        with pytest.raises(ValueError):
            eng.state_policy_resident(2, uniforms=u[:2])
        assert roll(use_env=1) == -1 and b'no environment set' in lib.pbvi_last_error()
        assert roll(use_env=2) == -1 and b'use_env' in lib.pbvi_last_error()
        assert roll(shifts=shifts) == -1 and b'shifts' in lib.pbvi_last_error()
        assert roll(end_observation=0) == -1 and b'end_observation' in lib.pbvi_last_error()
        assert roll(T=0) == -1 and b'T' in lib.pbvi_last_error()
        eng.set_environment_table(tre.other_table('grid4x3'))
        assert roll(use_env=1, shifts=shifts) == -1 and b'frame environment' in lib.pbvi_last_error()
        assert roll(use_env=1, end_observation=m.observation_count) == -1 and b'end_observation' in lib.pbvi_last_error()
        assert lib.pbvi_beliefs_count(eng._h) == 3                                                  # nothing ran
        # pbvi_rollout_env does not number the new source
        for policy in (3, 4):
            assert lib.pbvi_rollout_env(eng._h, policy, None, 0.9, s0.ctypes.data_as(i32p), mask.ctypes.data_as(u8p), -1, None, 0, SEED,
                                        4, None, None, None, None, None) == -1 and b'policy must be 0' in lib.pbvi_last_error()
        lost = np.full(3, 7, dtype=np.uint8)
        assert roll(lost=lost) == 0 and np.all(lost == 0)                                           # the model's world loses nobody
        eng.set_beliefs(tit.host_beliefs(m, 3, 0))
        assert roll(rule=2, use_env=1, end_observation=0, lost=lost) == 0
        eng.clear_state_policy()
        eng.set_beliefs(tit.host_beliefs(m, 3, 0))
        assert roll() == -1 and b'no state policy set' in lib.pbvi_last_error()
        assert call() == -1 and b'no state policy set' in lib.pbvi_last_error()
    finally:
        eng.close()


@pytest.mark.gpu
def test_block_alpha_set_backup_and_greedy_policies_are_untouched():
    """Set, the three rules and clear in the middle of other work: a following backup, infotaxis and space-aware call equal a
    fresh engine's."""
    c = get_case('olf_R5')
    w = np.arange(c.m.state_count, dtype=np.float64) % 17
    eng, fresh = tdr.make_engine(c, 'f32'), tdr.make_engine(c, 'f32')
    try:
        block = mc.sparse_beliefs(np.random.default_rng(2), 40, c.m.state_count)
        eng.set_beliefs(block)
        eng.set_state_weights(w)
        before = eng.infotaxis_resident(want_p_obs=True, want_entropy=True) + eng.space_aware_resident(0, want_terms=True)
        eng.run(c.gamma)                                          # a backup whose results wait to be fetched
        eng.set_state_policy(case_table('olf_R5'))
        for rule in (0, 1, 2):
            eng.state_policy_resident(rule, seed=5, want_state=True, want_votes=rule == 1)
        eng.clear_state_policy()
        eng.set_state_policy(case_table('olf_R5', 1))
        first = eng.state_policy_resident(1, want_votes=True)
        assert eng.B == 40 == int(eng._lib.pbvi_beliefs_count(eng._h)) and eng.alpha_count == c.alpha.shape[0]
        assert np.array_equal(eng.fetch_beliefs(), block.astype(np.float32))
        got = eng.fetch()
        fresh.set_beliefs(block)
        fresh.set_state_weights(w)
        fresh.run(c.gamma)
        want = fresh.fetch()
        assert np.array_equal(got.actions, want.actions) and np.array_equal(got.best_alpha_ind, want.best_alpha_ind)
        assert np.array_equal(got.alpha, want.alpha)
        after = eng.infotaxis_resident(want_p_obs=True, want_entropy=True) + eng.space_aware_resident(0, want_terms=True)
        clean = fresh.infotaxis_resident(want_p_obs=True, want_entropy=True) + fresh.space_aware_resident(0, want_terms=True)
        for x, y, z in zip(before, after, clean):
            assert x.tobytes() == y.tobytes() == z.tobytes()
        eng.run(c.gamma)                                          # and a backup after it
        again = eng.fetch()
        assert np.array_equal(again.actions, want.actions) and np.array_equal(again.alpha, want.alpha)
        # the table is the engine's: another table, other votes; the same table again, the same bits
        eng.set_state_policy(case_table('olf_R5'))
        second = eng.state_policy_resident(1, want_votes=True)
        assert not np.array_equal(first[1], second[1])
        fresh.set_state_policy(case_table('olf_R5'))
        assert fresh.state_policy_resident(1, want_votes=True)[1].tobytes() == second[1].tobytes()
    finally:
        eng.close()
        fresh.close()


@pytest.mark.gpu
def test_table_and_scratch_obey_the_allocation_cap_and_after_oom_drops_the_table():
    """The table, the results and Thompson's per-chunk sums are engine buffers: each is accounted to the byte.  The votes of
    16000 beliefs and 64 actions are 8 MiB: under a cap with 2 MiB of room the call fails with PBVI_ENOMEM; the table is a
    working buffer, so after the engine recovered none is set."""
    from pomdp_pbvi_exploration_amd import engine as engine_mod
    rng = np.random.default_rng(12)
    S, A, O, R = 4, 64, 1, 1
    rs = rng.integers(0, S, (S, A, R))
    rto = np.ones((S, A, O, R))
    m = tit.tables(S, A, O, R, rs, rto)
    b = mc.sparse_beliefs(rng, 16000, S, density=0.7)
    sa = spc.action_table(S, A)
    eng = tit.make_engine(m, 'f32')
    prev = engine_mod.debug_alloc_limit(-1)
    try:
        held_before = eng.device_bytes
        eng.set_state_policy(sa)
        assert eng.device_bytes == held_before + S * 4            # sized exactly, and accounted
        eng.clear_state_policy()
        assert eng.device_bytes == held_before
        eng.set_state_policy(sa)
        eng.set_beliefs(b)
        held = eng.device_bytes
        eng.state_policy_resident(2, seed=1)                      # action [B], state [B] int32 and (P_c, m_c) [B][1][2] fp64
        assert eng.device_bytes == held + 16000 * (4 + 4 + 16)
        engine_mod.debug_alloc_limit((eng.device_bytes >> 20) + 2)        # 2 MiB of room: the votes (8 MiB) do not fit
        with pytest.raises(MemoryError):                          # (Engine._ck has called pbvi_engine_after_oom)
            eng.state_policy_resident(1)
        assert eng.B == 0
        engine_mod.debug_alloc_limit(-1)
        eng.set_beliefs(b[:9])
        with pytest.raises(Exception, match='no state policy set'):
            eng.state_policy_resident(0)
        eng.set_state_policy(sa)
        act, st, votes = eng.state_policy_resident(1, want_state=True, want_votes=True)
        want = state_policy_numpy(b[:9], sa, 1, table_dtype=np.float32, action_count=A)
        assert np.array_equal(act, want[0]) and votes.tobytes() == want[2].tobytes()
    finally:
        engine_mod.debug_alloc_limit(prev)
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize('rule', ['mls', 'voting', 'thompson'])
def test_agent_gpu_equals_host(rule):
    """StatePolicy_Agent: the same histories from the counter-based rollout with the model on the GPU (fp64 engine) and on the
    host, in the model's world and against an environment; the same actions for a block of beliefs under one NumPy seed."""
    model = tit.ragged_agent_model()
    n, T = 300, 40
    np.random.seed(4)
    start = [int(s) for s in np.random.choice(model.state_count, size=n, p=model.start_probabilities)]
    gm = model.to_gpu('f64')
    sa = spc.action_table(model.state_count, model.action_count)
    rng = np.random.default_rng(42)
    table = rng.random((model.state_count, model.action_count, model.observation_count)) + 0.05
    envs = [None, TableEnvironment(table / table.sum(axis=2, keepdims=True), end_observation=0),
            FrameEnvironment(rng.integers(0, model.observation_count, (T + 7, 2, model.state_count)).astype(np.uint8),
                             np.arange(model.action_count) % 2, shifts=np.arange(n) % 8)]
    host, dev = StatePolicy_Agent(model, sa, rule), StatePolicy_Agent(gm, sa, rule)
    for env in envs:
        pair = []
        for agent in (host, dev):
            totals, hists = agent.run_n_simulations_parallel(n=n, max_steps=T, start_states=start, print_progress=False,
                                                             print_stats=False, device_rng_seed=7, environment=env)
            pair.append((list(totals), [(h.states, h.actions, h.observations, list(h.rewards), h.lost) for h in hists]))
        assert pair[0] == pair[1]
        assert any(len(h[1]) < T for h in pair[0][1])
    b = tit.host_beliefs(pomdp_mod._rollout_tables(model), 9, 5)
    acts = []
    for agent in (host, dev):
        np.random.seed(6)
        acts.append(agent.get_best_action(b))
    assert np.array_equal(acts[0], acts[1])
    runs = []
    for agent in (host, dev):
        np.random.seed(6)
        sims = SimulationSet(agent.model)
        sims.reference_indexing = False                           # (the reference's indexing needs as many simulations as successors)
        _, hists = agent.run_n_simulations_parallel(n=50, simulator_set=sims, max_steps=20, print_progress=False, print_stats=False)
        runs.append([(h.states, h.actions, h.observations) for h in hists])
    assert runs[0] == runs[1]
