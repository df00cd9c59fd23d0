"""Controller evaluation on the host: ``controller_numpy`` against an independent dense restatement and against the exact
solution of the linear system, the blind-policy bound inside the sandwich ``blind <= FIB <= MDP`` on committed example
models, stopping, the refusals of the C entry and of its binding, and ``HSVI_Solver(lower_init=...)``.  No GPU is needed."""
import ctypes as C

import numpy as np
import pytest

import controller_cases as cc
import fib_cases as fc
import model_cases as mc
import pomdp_pbvi_exploration_amd as pkg
from pomdp_pbvi_exploration_amd import (Blind_Solver, FIB_Solver, HSVI_Solver, VI_Solver, ValueFunction, controller_numpy,
                                        evaluate_controller, pessimistic_start)
from pomdp_pbvi_exploration_amd import engine as eng

STRUCTURE_CASES = [(name, S) for name in mc.STRUCTURES for S in (1, 5, 65)]


def controllers(t, seed=0):
    """The blind controller and a random one of 7 nodes for the model ``t``."""
    S, A, O, R = cc.shape(t)
    return {'blind': cc.blind(A, O), 'random7': cc.random_controller(7, A, O, seed)}


# --------------------------------------------------------------------------- #
# 1. One sweep against the dense restatement
# --------------------------------------------------------------------------- #
def check_against_dense(t, gamma, tag):
    """One sweep of ``controller_numpy`` against one dense sweep at the project's fp64 bar (``test_fib.py``'s): the two
    associate their sums differently, so this is closeness, not equality."""
    D = fc.dense_rto(t)
    for kind, (na, ns) in controllers(t).items():
        for start, v0 in cc.starts(t, gamma, len(na)).items():
            want, want_change = cc.dense_sweep(D, t.expected_rewards_table, na, ns, v0, gamma)
            rows, changes = controller_numpy(t, na, ns, v0, gamma, 0.0, 1)
            assert rows.shape == v0.shape and changes.shape == (1,), (tag, kind, start)
            scale = np.abs(want).max()
            np.testing.assert_allclose(rows, want, rtol=1e-12, atol=1e-12 * scale, err_msg=f'{tag} {kind} {start}')
            np.testing.assert_allclose(changes[0], want_change, rtol=1e-12, atol=1e-12 * scale, err_msg=f'{tag} {kind} {start}')


@pytest.mark.parametrize('name,S', STRUCTURE_CASES)
def test_one_sweep_matches_dense_restatement_on_structures(name, S):
    check_against_dense(fc.structure_case(name, S), 0.95, (name, S))


@pytest.mark.parametrize('seed', range(8))
def test_one_sweep_matches_dense_restatement_on_random_models(seed):
    t, gamma = fc.random_tables(seed)
    check_against_dense(t, gamma, seed)


# --------------------------------------------------------------------------- #
# 2. Converged run against the exact solve
# --------------------------------------------------------------------------- #
def contraction_bound(change, gamma):
    """``|V_k - V*| <= gamma / (1 - gamma) * |V_k - V_{k-1}|`` (the sweep contracts by gamma in the max norm), with a
    relative 1e-9 and an absolute 1e-12 for the rounding of both sides."""
    return change * gamma / (1 - gamma) * (1 + 1e-9) + 1e-12


@pytest.mark.parametrize('name', list(mc.STRUCTURES))
def test_blind_run_converges_to_the_exact_solution_from_below(name):
    gamma, limit = 0.9, 1e-4
    t = fc.structure_case(name, 257)
    S, A, O, R = cc.shape(t)
    na, ns = cc.blind(A, O)
    exact = cc.exact_rows(t, na, ns, gamma)
    v0 = pessimistic_start(t, gamma, A)
    rows, changes = controller_numpy(t, na, ns, v0, gamma, limit, 1000)
    assert 1 < len(changes) < 1000 and changes[-1] < limit
    assert np.abs(rows - exact).max() <= contraction_bound(changes[-1], gamma), (name, changes[-1])
    assert (rows <= exact + 1e-9).all(), name                               # stopped anywhere, still a lower bound
    prev = v0
    for k in range(1, 6):                                                   # ... because the iterates rise
        cur, _ = controller_numpy(t, na, ns, v0, gamma, 0.0, k)
        assert (cur >= prev - 1e-12).all(), (name, k)
        prev = cur


@pytest.mark.parametrize('name', list(mc.STRUCTURES))
def test_random_controller_converges_to_the_exact_solution(name):
    gamma, limit = 0.9, 1e-4
    t = fc.structure_case(name, 257)
    S, A, O, R = cc.shape(t)
    na, ns = cc.random_controller(7, A, O, 0)
    rows, changes = controller_numpy(t, na, ns, np.zeros((7, S)), gamma, limit, 1000)
    assert 1 < len(changes) < 1000 and changes[-1] < limit
    assert np.abs(rows - cc.exact_rows(t, na, ns, gamma)).max() <= contraction_bound(changes[-1], gamma), (name, changes[-1])


def test_indirection_controller_converges_to_the_exact_solution():
    """Nine nodes none of which is its own successor, at S = 70."""
    gamma = 0.9
    t = fc.dense_random_case(7, 5, 4)
    na, ns = cc.shifting(9, 7, 5)
    rows, changes = controller_numpy(t, na, ns, pessimistic_start(t, gamma, 9), gamma, 1e-6, 1000)
    assert changes[-1] < 1e-6
    exact = cc.exact_rows(t, na, ns, gamma)
    assert np.abs(rows - exact).max() <= contraction_bound(changes[-1], gamma)
    assert (rows <= exact + 1e-9).all()


# --------------------------------------------------------------------------- #
# 3. The blind bound inside the sandwich on the example models
# --------------------------------------------------------------------------- #
_SOLVED = {}


def solved(key):
    """``(model, gamma, MDP solution at its fixed point, FIB solution from it, blind solution, blind history)``, once."""
    if key not in _SOLVED:
        model, gamma = fc.file_model(key)
        mdp, _ = VI_Solver(gamma=gamma, eps=1e-13).solve(model, print_progress=False)
        fib, _ = FIB_Solver(gamma=gamma, eps=1e-3).solve(model, mdp_solution=mdp, print_progress=False)
        blind, hist = Blind_Solver(gamma=gamma, eps=1e-3).solve(model, print_progress=False)
        _SOLVED[key] = (model, gamma, mdp, fib, blind, hist)
    return _SOLVED[key]


@pytest.mark.parametrize('key', list(fc.FILE_MODELS))
def test_blind_solver_is_below_fib_and_the_mdp_solution(key):
    model, gamma, mdp, fib, blind, hist = solved(key)
    limit = 1e-3 * gamma / (1 - gamma)
    changes = hist.value_function_changes
    assert 0 < len(changes) < 10000 and changes[-1] < limit and all(c >= limit for c in changes[:-1])
    assert isinstance(blind, ValueFunction) and not blind.is_on_gpu
    rows = blind.alpha_vector_array
    assert rows.shape[1] == model.state_count and len(blind.actions) == rows.shape[0] <= model.action_count
    v_mdp = np.max(mdp.alpha_vector_array, axis=0)
    assert (np.max(rows, axis=0) <= v_mdp + 1e-9).all()
    beliefs = mc.sparse_beliefs(np.random.default_rng(11), 32, model.state_count)
    lower = np.max(beliefs @ rows.T, axis=1)
    upper = np.max(beliefs @ fib.alpha_vector_array.T, axis=1)
    assert (lower <= upper + 1e-9).all(), (key, np.max(lower - upper))


def test_blind_solver_rows_are_the_blind_controller_from_the_pessimistic_start():
    model, gamma, _, _, blind, hist = solved('tiger')
    A, O = model.action_count, len(model.observations)
    na, ns = cc.blind(A, O)
    rows, changes = evaluate_controller(model, na, ns, gamma=gamma, eps=1e-3)
    assert list(changes) == hist.value_function_changes
    want = ValueFunction(model, rows, model.actions)
    assert np.array_equal(blind.alpha_vector_array, want.alpha_vector_array) and np.array_equal(blind.actions, want.actions)
    # listening for ever on tiger.95 is worth -1 / (1 - gamma), not the -1 of its expected-rewards row
    listen = rows[int(np.argmax(rows[:, 0]))]
    np.testing.assert_allclose(listen, -1.0 / (1 - gamma), rtol=0, atol=1e-3 * gamma / (1 - gamma) ** 2)
    per_sweep, hist2 = Blind_Solver(gamma=gamma, eps=1e-3).solve(model, history_tracking_level=2, print_progress=False)
    assert np.array_equal(per_sweep.alpha_vector_array, blind.alpha_vector_array)
    assert hist2.value_function_changes == hist.value_function_changes


def test_names_are_exported():
    for name in ('Blind_Solver', 'controller_numpy', 'evaluate_controller', 'pessimistic_start'):
        assert name in pkg.__all__ and hasattr(pkg, name)
    assert 'pbvi_controller_value_iteration' in eng.EXPORTS


# --------------------------------------------------------------------------- #
# 4. Stopping
# --------------------------------------------------------------------------- #
def test_run_stops_at_the_limit_and_returns_the_last_sweep_that_ran():
    t = fc.structure_case('ragged', 257)
    S, A, O, R = cc.shape(t)
    na, ns = cc.blind(A, O)
    v0 = pessimistic_start(t, 0.9, A)
    rows, changes = controller_numpy(t, na, ns, v0, 0.9, 1e-4, 200)
    assert 70 < len(changes) < 200 and changes[-1] < 1e-4 and (changes[:-1] >= 1e-4).all()
    again, _ = controller_numpy(t, na, ns, v0, 0.9, 0.0, len(changes))     # the same sweeps, none of them the stopping one
    assert np.array_equal(rows, again)
    same, none = controller_numpy(t, na, ns, v0 - 3.0, 0.9, 1e-4, 0)
    assert np.array_equal(same, v0 - 3.0) and none.shape == (0,)
    for horizon in (1, 10, 64, 70):
        cut, cut_changes = controller_numpy(t, na, ns, v0, 0.9, 1e-4, horizon)
        assert cut_changes.shape == (horizon,) and np.array_equal(cut_changes, changes[:horizon])
        assert not np.array_equal(cut, rows)


# --------------------------------------------------------------------------- #
# 5. The entry and its binding refuse bad input before they touch the device
# --------------------------------------------------------------------------- #
def small():
    t = fc.structure_case('hub', 5)
    na, ns = cc.random_controller(3, 2, 2, 0)
    return (t.reachable_states, t.reachable_transitional_observation_table, t.expected_rewards_table, na, ns,
            np.zeros((3, 5)))


def test_binding_refuses_bad_input_without_a_gpu():
    rs, rto, er, na, ns, v0 = small()
    call = eng.controller_value_iteration
    bad = rs.copy()
    bad[3, 1, 0] = 5
    with pytest.raises(ValueError):
        call(bad, rto, er, na, ns, v0, 0.9, 0.0, 3)
    bad[3, 1, 0] = -1
    with pytest.raises(ValueError):
        call(bad, rto, er, na, ns, v0, 0.9, 0.0, 3)
    for bad_action in (2, -1):
        with pytest.raises(ValueError):
            call(rs, rto, er, np.array([0, bad_action, 1]), ns, v0, 0.9, 0.0, 3)
    for bad_succ in (3, -1):
        bad_ns = ns.copy()
        bad_ns[2, 1] = bad_succ
        with pytest.raises(ValueError):
            call(rs, rto, er, na, bad_ns, v0, 0.9, 0.0, 3)
    with pytest.raises(ValueError):
        call(rs, rto[:, :, :, :1], er, na, ns, v0, 0.9, 0.0, 3)
    with pytest.raises(ValueError):
        call(rs, rto, er[:4], na, ns, v0, 0.9, 0.0, 3)
    with pytest.raises(ValueError):
        call(rs, rto, er, na, ns[:, :1], v0, 0.9, 0.0, 3)
    with pytest.raises(ValueError):
        call(rs, rto, er, na, ns, v0.T, 0.9, 0.0, 3)
    with pytest.raises(ValueError):
        call(rs, rto, er, na[:0], ns[:0], v0[:0], 0.9, 0.0, 3)
    with pytest.raises(ValueError):
        call(rs, rto, er, na, ns, v0, 0.9, 0.0, -1)
    # oversize products: the arrays are views with stride 0, nothing of that size exists
    O = 2 ** 31
    one = np.zeros((1, 1, 1), dtype=np.int64)
    with pytest.raises(NotImplementedError):
        call(one, np.broadcast_to(np.ones(1), (1, 1, O, 1)), np.zeros((1, 1)), np.zeros(1, dtype=np.int64),
             np.broadcast_to(np.zeros(1, dtype=np.int64), (1, O)), np.zeros((1, 1)), 0.9, 0.0, 3)
    N = 2 ** 31
    with pytest.raises(NotImplementedError):
        call(one, np.ones((1, 1, 1, 1)), np.zeros((1, 1)), np.broadcast_to(np.zeros(1, dtype=np.int64), (N,)),
             np.broadcast_to(np.zeros(1, dtype=np.int64), (N, 1)), np.broadcast_to(np.zeros(1), (N, 1)), 0.9, 0.0, 3)


def test_entry_point_decides_errors_before_the_device():
    """The same refusals from the C entry itself (codes of include/pbvi_hip.h), and ``horizon = 0`` returning ``v0``: none
    of them needs a device."""
    lib = eng.load_library()
    rs, rto, er, na, ns, v0 = small()
    rs32, na32, ns32 = (np.ascontiguousarray(x, dtype=np.int32) for x in (rs, na, ns))
    v0 = v0 - 2.5
    out = np.full((3, 5), np.nan)
    its = C.c_int32(-1)
    EINVAL, EUNSUPPORTED = -1, -4

    def call(S=5, A=2, O=2, R=2, N=3, rs_=rs32, na_=na32, ns_=ns32, horizon=3):
        p = lambda a, ty: a.ctypes.data_as(C.POINTER(ty))      # noqa: E731
        return lib.pbvi_controller_value_iteration(0, S, A, O, R, p(rs_, C.c_int32), p(rto, C.c_double), p(er, C.c_double),
                                                   N, p(na_, C.c_int32), p(ns_, C.c_int32), p(v0, C.c_double), 0.9, 0.0,
                                                   horizon, p(out, C.c_double), None, C.byref(its))

    assert call(horizon=-1) == EINVAL and b'controller_value_iteration' in lib.pbvi_last_error()
    assert call(N=0) == EINVAL and call(S=0) == EINVAL and call(O=0) == EINVAL
    bad = na32.copy()
    bad[1] = 2
    assert call(na_=bad) == EINVAL and b'node action' in lib.pbvi_last_error()
    bad = ns32.copy()
    bad[2, 0] = 3
    assert call(ns_=bad) == EINVAL and b'successor node' in lib.pbvi_last_error()
    bad = rs32.copy()
    bad[4, 0, 1] = 5
    assert call(rs_=bad) == EINVAL and b'reachable state' in lib.pbvi_last_error()
    # sizes alone decide these, before any table is read (the pointers are the tiny arrays above)
    assert call(S=2 ** 20, A=2 ** 6, O=2 ** 4, R=2) == EUNSUPPORTED and b'S*A*O*R' in lib.pbvi_last_error()
    assert call(S=2 ** 20, A=1, O=1, R=1, N=2 ** 19) == EUNSUPPORTED and b'N*ceil(S/256)' in lib.pbvi_last_error()
    assert call(horizon=0) == 0 and its.value == 0 and np.array_equal(out, v0)


# --------------------------------------------------------------------------- #
# 6. HSVI_Solver(lower_init=...)
# --------------------------------------------------------------------------- #
def test_hsvi_lower_init():
    model, gamma, mdp, _, blind, _ = solved('tiger')

    def run(**kw):
        np.random.seed(0)
        solver = HSVI_Solver(gamma=gamma, eps=1e-3, mdp_solution=mdp, sawtooth='support', **kw)
        out, hist = solver.solve(model, expansions=3, history_tracking_level=2, print_progress=False)
        return solver, out, hist

    with pytest.raises(ValueError):
        HSVI_Solver(lower_init='bogus')
    s_blind, vf_blind, h_blind = run(lower_init='blind')
    first = h_blind.value_functions[0]
    assert np.array_equal(first.alpha_vector_array, blind.alpha_vector_array) and np.array_equal(first.actions, blind.actions)
    assert len(vf_blind) >= 1
    again, _ = s_blind.solve(model, expansions=1, print_progress=False)    # computed once per solver object
    assert s_blind._blind_start is first
    # an initial value function given by the caller wins
    given = ValueFunction(model, blind.alpha_vector_array[:1], blind.actions[:1])
    _, h_given = s_blind.solve(model, expansions=1, initial_value_function=given, history_tracking_level=2, print_progress=False)
    assert h_given.value_functions[0] is given
    # 'rewards' is the default and changes nothing
    _, vf_rewards, h_rewards = run(lower_init='rewards')
    _, vf_def, h_def = run()
    want = ValueFunction(model, model.expected_rewards_table.T, model.actions)
    for h in (h_rewards, h_def):
        assert np.array_equal(h.value_functions[0].alpha_vector_array, want.alpha_vector_array)
        assert np.array_equal(h.value_functions[0].actions, want.actions)
    assert np.array_equal(vf_rewards.alpha_vector_array, vf_def.alpha_vector_array)
    assert np.array_equal(vf_rewards.actions, vf_def.actions)
