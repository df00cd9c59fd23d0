"""Host-side mirror of the reference interface (NumPy path, BASELINE config 0): same tables,
same container semantics, same known answers as the reference."""
import copy
import json
import os
import random

import numpy as np
import pytest

from conftest import GOLDEN, load_npz
from pomdp_pbvi_exploration_amd import (Belief, BeliefSet, FSVI_Solver, Model, PBVI_Solver, ValueFunction,
                                        load_POMDP_file, synth)

EXAMPLES = os.path.join(GOLDEN, 'models')
KAT = json.load(open(os.path.join(GOLDEN, 'kat.json')))


def _two_state(obs_rnd):
    T = np.zeros((2, 2, 2))
    Ob = np.zeros((2, 2, 2))
    Rw = np.zeros((2, 2, 2, 2))
    for s in range(2):
        for a in range(2):
            for sp in range(2):
                T[s, a, sp] = 0.8 if (s + a) % 2 == sp else round(1.0 - 0.8, 1)
                Ob[sp, a, s] = obs_rnd if sp == s else 1.0 - obs_rnd
    for sp in range(2):
        Rw[:, :, sp, :] = [0.2, 0.6][sp]
    return Model(states=['s0', 's1'], actions=['stay', 'move'], observations=['s0', 's1'], transitions=T, rewards=Rw,
                 observation_table=Ob, rewards_are_probabilistic=True)


@pytest.mark.parametrize('fname,tables', [('tiger.95.POMDP', 'tiger_tables.npz'),
                                          ('4x3.95-no_loop_2_grid.POMDP', 'grid4x3_tables.npz')])
def test_pomdp_file_tables_equal_reference(fname, tables):
    model, solver = load_POMDP_file(os.path.join(EXAMPLES, fname))
    t = load_npz(tables)
    assert np.array_equal(model.reachable_states, t['reachable_states'])
    assert np.array_equal(model.reachable_probabilities, t['reachable_probabilities'])
    assert np.array_equal(model.reachable_transitional_observation_table, t['rto'])
    assert np.array_equal(model.expected_rewards_table, t['expected_rewards'])
    assert np.array_equal(model.start_probabilities, t['start'])
    assert solver.gamma == 0.95 and solver.expand_function == 'ssea' and solver.eps == 0.001


def test_kat1_kat2_tiger():
    model, solver = load_POMDP_file(os.path.join(EXAMPLES, 'tiger.95.POMDP'))
    vf0 = ValueFunction(model, model.expected_rewards_table.T, model.actions)
    out = solver.backup(model, BeliefSet(model, [Belief(model)]), vf0, belief_dominance_prune=False)
    assert out.alpha_vector_array.tolist() == KAT['kat1_alpha'] == [[-1.95, -1.95]]
    assert list(out.actions) == [0]
    assert Belief(model).update(0, 0).values.tolist() == KAT['kat2_belief']
    np.testing.assert_allclose(KAT['kat2_belief'], [0.85, 0.15], rtol=1e-15)


def test_kat3_tiger_full_solve_matches_reference():
    model, solver = load_POMDP_file(os.path.join(EXAMPLES, 'tiger.95.POMDP'))
    model.end_actions = [1, 2]
    vf, hist = solver.solve(model, expansions=8, update_passes=8, print_progress=False)
    assert hist.beliefs_counts == KAT['kat3_belief_counts'] == [1, 2, 4, 7, 11, 15, 21, 31, 41]
    assert len(vf) == 5                                                   # tiger_problem_from_file.ipynb cell [22]
    np.testing.assert_allclose(vf.alpha_vector_array, KAT['kat3_alpha'], rtol=1e-12)
    assert list(vf.actions) == KAT['kat3_actions'] == [0, 0, 0, 1, 2]   # reference run; SURVEY 8c lists the last two swapped
    assert hist.alpha_vector_counts == KAT['kat3_alpha_counts']
    # policy thresholds printed by the notebook (tiger_problem_from_file.ipynb:205,388)
    a = vf.alpha_vector_array
    x = (a[2, 1] - a[4, 1]) / ((a[4, 0] - a[4, 1]) - (a[2, 0] - a[2, 1]))
    np.testing.assert_allclose([1 - x, x], [0.041972822899461214, 0.9580271771005388], rtol=1e-9)


def _iterate(model, belief_rows, eps):
    solver = PBVI_Solver(gamma=0.99)
    bs = BeliefSet(model, [Belief(model, np.array(r)) for r in belief_rows])
    vf = copy.deepcopy(ValueFunction(model, model.expected_rewards_table, model.actions))
    limit = eps * (0.99 / (1 - 0.99))
    old, its = None, 1000
    for it in range(1000):
        vf = solver.backup(model, bs, vf)
        cur = np.max(np.matmul(bs.belief_array, vf.alpha_vector_array.T), axis=1)
        if old is not None and np.max(np.abs(cur - old)) < limit:
            its = it
            break
        old = cur
    return float(np.max(vf.alpha_vector_array)), float(np.min(vf.alpha_vector_array)), its, len(vf)


@pytest.mark.parametrize('i,expect', [(0, (39.324873290949945, 38.73374028602384, 368)),
                                      (17, (43.89860938273302, 43.65860938273302, 379)),
                                      (50, (39.3162567916742, 38.725123786748085, 367))])
def test_kat4_repeated_backup_notebook_numbers(i, expect):
    """observation_variation_comparisson.ipynb:238,255,288 (stored cell outputs)."""
    mx, mn, its, _ = _iterate(_two_state(0.7), [[i / 100, 1.0 - (i / 100)], [1.0 - (i / 100), i / 100]], 0.0001)
    assert its == expect[2]
    np.testing.assert_allclose([mx, mn], expect[:2], rtol=1e-12)
    ref = KAT['kat4'][str(i)]
    assert (ref['max'], ref['min'], ref['iters']) == expect


@pytest.mark.parametrize('acc,expect', [(0.5, (30.500954541065976, 29.90982153613987, 138)),
                                        (0.7, (35.201002743439766, 34.77750362678456, 150)),
                                        (1.0, (42.29309361078366, 42.053093610783655, 165))])
def test_kat5_102_beliefs_notebook_numbers(acc, expect):
    """observation_variation_comparisson.ipynb:787,791,797 (stored cell outputs)."""
    rows = []
    for i in range(51):
        rows += [[i / 100, 1.0 - (i / 100)], [1.0 - (i / 100), i / 100]]
    mx, mn, its, n = _iterate(_two_state(acc), rows, 0.001)
    assert its == expect[2] and n == KAT['kat5'][str(acc)]['n']
    np.testing.assert_allclose([mx, mn], expect[:2], rtol=1e-12)


def test_grid4x3_seeded_fsvi_trajectory():
    """G-C2: seeded FSVI on the 4x3 grid reproduces the reference's |V| trajectory and final set."""
    z = load_npz('grid4x3_fsvi.npz')
    model, _ = load_POMDP_file(os.path.join(EXAMPLES, '4x3.95-no_loop_2_grid.POMDP'))
    model.end_states = [3, 6]
    np.random.seed(0)
    random.seed(0)
    vf, hist = FSVI_Solver(gamma=0.95, eps=1e-6).solve(model, expansions=10, max_belief_growth=10, print_progress=False)
    assert hist.alpha_vector_counts == list(z['alpha_counts'])
    last = int(z['n_calls']) - 1
    np.testing.assert_allclose(vf.alpha_vector_array, z[f'c{last}_out_alpha'], rtol=1e-12, atol=1e-13)
    assert np.array_equal(vf.actions, z[f'c{last}_out_actions'])


def _limiter_solve(use_gpu: bool):
    z = load_npz('limiter_fsvi.npz')
    cfg = json.loads(str(z['cfg']))
    m = synth.olfactory_model(H=15, W=40, R=1, f32=False)
    model = Model(states=m.S, actions=m.A, observations=m.O, reachable_states=m.reachable_states,
                  observation_table=m.observation_table, end_states=[m.goal], start_probabilities=list(m.start_belief))
    np.random.seed(0)
    random.seed(0)
    vf, hist = FSVI_Solver(gamma=m.gamma, eps=1e-6).solve(
        model, cfg['expansions'], max_belief_growth=cfg['max_belief_growth'],
        limit_value_function_size=cfg['limit_value_function_size'], print_progress=False, use_gpu=use_gpu)
    return z, vf, hist


def test_value_function_size_limiter_reproduces_the_reference_run():
    """SURVEY 8f-1, second half: the |V| limiter (usefulness scan + weighted random deletion, src/pomdp.py:2347-2365) in
    the reference's seeded FSVI run of the S=600 olfactory model (limiter_fsvi.npz, made by make_golden.py limiter)."""
    z, vf, hist = _limiter_solve(use_gpu=False)
    assert hist.alpha_vector_counts == list(z['alpha_counts']) and hist.beliefs_counts == list(z['belief_counts'])
    assert np.any(np.diff(z['alpha_counts']) < 0)            # the limiter fired
    np.testing.assert_allclose(hist.value_function_changes, z['changes'], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(vf.alpha_vector_array, z['final_alpha'], rtol=1e-12, atol=1e-14)
    assert np.array_equal(vf.actions, z['final_actions'])


def test_alpha_key_has_the_semantics_of_the_row_bytes():
    """ValueFunction keys its dedup dictionary on ``_AlphaKey`` instead of ``values.tobytes()`` (src/mdp.py:667-669): equal
    bytes <=> equal keys; shifted copies, a flipped sign of zero, another dtype are different keys; a known hash (the
    device's) with the same row is the same key; and the container behaves as with bytes keys."""
    from pomdp_pbvi_exploration_amd.mdp import AlphaVector, _AlphaKey
    rng = np.random.default_rng(0)
    r = rng.normal(size=257)
    assert _AlphaKey(r) == _AlphaKey(r.copy()) and hash(_AlphaKey(r)) == hash(_AlphaKey(r.copy()))
    assert _AlphaKey(r) != _AlphaKey(np.roll(r, 1)) and int(_AlphaKey(r)) != int(_AlphaKey(np.roll(r, 1)))   # no collision either
    z = np.zeros(8)
    zn = z.copy()
    zn[3] = -0.0
    assert _AlphaKey(z) != _AlphaKey(zn)
    r32 = r.astype(np.float32)
    assert _AlphaKey(r32) != _AlphaKey(r32.astype(np.float64))
    assert _AlphaKey.from_hash(_AlphaKey.hash_of(r32), r32) == _AlphaKey(r32.copy())
    # the hash is the documented sum (what the device kernel computes)
    bits = r32.view(np.uint32).astype(object)
    assert int(_AlphaKey(r32)) == sum(int(b) * (2 * i + 1) for i, b in enumerate(bits)) % (1 << 64)
    bits = r.view(np.uint64).astype(object)
    assert int(_AlphaKey(r)) == sum(int(b) * (2 * i + 1) for i, b in enumerate(bits)) % (1 << 64)
    # a vector that carries a (device) hash is found equal to a host-hashed copy of its row
    model = _two_state(0.7)
    a = AlphaVector(np.array([1., 2.]), 0)
    a._hash = _AlphaKey.hash_of(a.values)
    vf = ValueFunction(model, [a, AlphaVector(np.array([3., 4.]), 1), AlphaVector(np.array([1., 2.]), 1)])
    assert len(vf) == 2 and list(vf.actions) == [1, 1]                 # first position, last action


def test_value_function_container_semantics():
    model = _two_state(0.7)
    rows = np.array([[1., 2.], [3., 4.], [1., 2.]])
    vf = ValueFunction(model, rows, [0, 1, 1])
    assert vf.alpha_vector_array.tolist() == [[1., 2.], [3., 4.]] and list(vf.actions) == [1, 1]
    new = ValueFunction(model, np.array([[9., 9.], [3., 4.]]), [0, 0])
    new.extend(vf)
    assert new.alpha_vector_array.tolist() == [[9., 9.], [3., 4.], [1., 2.]] and list(new.actions) == [0, 1, 1]
    dom = ValueFunction(model, np.array([[1., 2.], [0., 1.], [2., 0.]]), [0, 1, 0])
    dom.prune(2)
    assert dom.alpha_vector_array.tolist() == [[1., 2.], [2., 0.]] and len(dom) == 2


def test_gpu_request_never_falls_back(monkeypatch):
    """use_gpu=True must raise when the HIP engine cannot be created (no silent CPU path)."""
    from pomdp_pbvi_exploration_amd import engine as eng
    model = _two_state(0.7)
    monkeypatch.setattr(eng, 'LIB_PATH', '/nonexistent/libpbvi_hip.so')
    monkeypatch.setattr(eng, '_lib', None)
    with pytest.raises(eng.EngineUnavailable):
        eng.load_library('/nonexistent/libpbvi_hip.so')
    if eng.device_count.__call__ and not _has_gpu():
        with pytest.raises((eng.EngineUnavailable, RuntimeError)):
            PBVI_Solver().solve(model, expansions=1, use_gpu=True, print_progress=False)


def _has_gpu():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


def test_synth_generator_is_deterministic():
    m1 = synth.olfactory_model(H=15, W=40, R=5)
    m2 = synth.olfactory_model(H=15, W=40, R=5)
    assert synth.checksum(m1.rto, m1.reachable_states) == synth.checksum(m2.rto, m2.reachable_states)
    z = load_npz('olfactory_small_R5.npz')
    assert np.array_equal(m1.reachable_states, z['reachable_states'])
    assert np.array_equal(m1.rto.astype(np.float32), z['rto'])
    a, acts = synth.alpha_set(m1, 48)
    assert np.array_equal(a.astype(np.float32), z['alpha']) and np.array_equal(acts, z['alpha_actions'])
    b = synth.belief_points(m1, 64, max_depth=16)
    assert np.array_equal(b.astype(np.float32), z['beliefs'])
    np.testing.assert_allclose(b.sum(axis=1), 1.0, atol=1e-6)
    # R=5 rows are proper distributions over five distinct successors
    assert all(len(set(row)) == 5 for row in m1.reachable_states.reshape(-1, 5)[:50])


def test_backup_result_rows_for_value_function():
    """engine.BackupResult -> rows handed to ValueFunction: one row per distinct key among the kept beliefs,
    in first-occurrence order (what the reference's byte-dedup dict produces)."""
    from pomdp_pbvi_exploration_amd.engine import BackupResult
    uniq = np.array([[1., 1.], [2., 2.], [3., 3.]])
    index = np.array([0, 1, 0, 2, 1])
    res = BackupResult(uniq, index, np.array([5, 6, 5, 7, 6]), np.zeros((5, 1, 1), dtype=np.int64),
                       np.array([False, True, True, False, True]), {})
    assert res.alpha.tolist() == [[1., 1.], [2., 2.], [1., 1.], [3., 3.], [2., 2.]]
    rows, acts = res.value_function_rows(use_keep=False)
    assert rows.tolist() == [[1., 1.], [2., 2.], [3., 3.]] and acts.tolist() == [5, 6, 7]
    rows, acts = res.value_function_rows(use_keep=True)        # kept beliefs 1,2,4 -> keys 1,0,1
    assert rows.tolist() == [[2., 2.], [1., 1.]] and acts.tolist() == [6, 5]
    res.keep[:] = False
    rows, acts = res.value_function_rows(use_keep=True)
    assert rows.shape == (0, 2) and acts.shape == (0,)


# --------------------------------------------------------------------------- #
# On-disk formats + MDP value iteration
# --------------------------------------------------------------------------- #
def clipped_olfactory_mdp(H=61, W=361):
    """The 61x361 grid of the reference's stored value function: N/E/S/W/stay/stay moves, rows wrap, columns clip,
    reward 1 on landing in the goal (30, 60)."""
    from pomdp_pbvi_exploration_amd.mdp import Model as MDPModel
    S = H * W
    y, x = np.divmod(np.arange(S), W)

    def nb(dy, dx):
        return ((y + dy) % H) * W + np.clip(x + dx, 0, W - 1)

    rs = np.stack([nb(-1, 0), nb(0, 1), nb(1, 0), nb(0, -1), np.arange(S), np.arange(S)], axis=1)[:, :, None]
    return MDPModel(states=S, actions=6, reachable_states=rs, end_states=[(H // 2) * W + 60])


def test_value_iteration_reproduces_reference_csv():
    """KAT: the value function the reference stored (Experiments/Olfactory Navigation/ValueFunctions/
    20231113_182429_value_function.csv, kept gzip-compressed under tests/golden) is the VI solution of the
    clipped 61x361 grid at gamma=0.99, eps=1e-4: 460 sweeps from V0 = ER, max 99.0276 = 100(1 - 0.99^461)."""
    from pomdp_pbvi_exploration_amd.mdp import VI_Solver
    model = clipped_olfactory_mdp()
    ref = ValueFunction.load_from_file(os.path.join(GOLDEN, 'ref_value_function_61x361.csv.gzip'), model)
    assert list(ref.actions) == [0, 1, 2, 3, 5] and ref.alpha_vector_array.shape == (5, 22021)
    vf, hist = VI_Solver(gamma=0.99, eps=1e-4).solve(model, print_progress=False)
    assert len(hist.iteration_times) == 460                      # V0 = ER is the first term of the series
    assert list(vf.actions) == [0, 1, 2, 3, 5]
    np.testing.assert_allclose(vf.alpha_vector_array, ref.alpha_vector_array, rtol=0, atol=1e-12)
    assert abs(float(vf.alpha_vector_array.max()) - 100 * (1 - 0.99 ** 461)) < 1e-10


def test_value_function_file_round_trips(tmp_path):
    model = _two_state(0.7)
    vf = ValueFunction(model, np.array([[0.1, 1 / 3], [2.5, -7.25], [1e-17, 3.0]]), [1, 0, 1])
    d = str(tmp_path / 'vfs')
    vf.save(d, 'a')                                   # '.csv' is appended
    vf.save(d, 'b.csv', compress=True)                # -> b.csv.gzip
    vf.save_parquet(d, 'c')
    assert sorted(os.listdir(d)) == ['a.csv', 'b.csv.gzip', 'c.parquet']
    with open(os.path.join(d, 'a.csv')) as f:
        assert f.readline().strip() == 'action,s0,s1'  # the reference's header: action, then state labels
    for back in (ValueFunction.load_from_file(os.path.join(d, 'a.csv'), model),
                 ValueFunction.load_from_file(os.path.join(d, 'b.csv.gzip'), model),
                 ValueFunction.load_from_parquet(os.path.join(d, 'c.parquet'), model)):
        assert np.array_equal(back.alpha_vector_array, vf.alpha_vector_array)
        assert np.array_equal(back.actions, vf.actions)


# --------------------------------------------------------------------------- #
# Host-side logic of the GPU path, exercised on CPU with a NumPy stand-in for the device calls
# (tests only: the product raises when the HIP library is missing, see test_gpu_request_never_falls_back)
# --------------------------------------------------------------------------- #
class _StubEngine:
    """Stands in for engine.Engine in tests of the host bookkeeping around it: row stores, id tags, the
    max-value cache and the belief walk; device kernels are replaced by NumPy on the stored rows."""

    def __init__(self, model):
        from pomdp_pbvi_exploration_amd.engine import Engine
        self.model = model
        self.S = model.state_count
        self.rows = {'alpha': [], 'belief': []}
        self._store_epoch = {'alpha': 0, 'belief': 0}
        self._vmax_cache, self._vmax_epochs = [], None
        self.serial = next(Engine._serials)                  # residency tags name the engine by serial, not by id()
        self.pairs_scored = 0
        # the real bookkeeping methods, bound to this object
        self.dtype = 'f64'
        for name in ('row_ids', 'max_value_objects', '_max_value_objects', 'belief_tag'):
            setattr(self, name, getattr(Engine, name).__get__(self))
        self._VMAX_ENTRIES, self._BLOCK = Engine._VMAX_ENTRIES, Engine._BLOCK

    def store_rows(self, which, rows):
        first = len(self.rows[which])
        self.rows[which].extend(np.asarray(rows, dtype=np.float64))
        return first

    def reset_store(self, which):
        self.rows[which] = []
        self._store_epoch[which] += 1

    def _vmax_block(self, a_ids, b_ids):
        a = np.array([self.rows['alpha'][i] for i in a_ids])
        b = np.array([self.rows['belief'][i] for i in b_ids])
        self.pairs_scored += len(a_ids) * len(b_ids)
        return np.max(b @ a.T, axis=1)

    def belief_walk(self, b0, actions, observations, restart=None):
        out, b = [], Belief(self.model, np.asarray(b0))
        start = b
        for i, (a, o) in enumerate(zip(actions, observations)):
            if restart is not None and restart[i]:
                b = start
            b = b.update(int(a), int(o))
            out.append(b.values)
        first = self.store_rows('belief', np.array(out))
        return np.array(out), first


def test_max_value_cache_scores_only_new_pairs():
    """compute_change's bookkeeping (Engine.max_value_objects): values equal the from-scratch ones for every query
    order of the solve loop, and only (known beliefs x new alpha rows) + (new beliefs x all alpha rows) are scored."""
    from pomdp_pbvi_exploration_amd.mdp import AlphaVector
    model, _ = load_POMDP_file(os.path.join(EXAMPLES, '4x3.95-no_loop_2_grid.POMDP'))
    rng = np.random.default_rng(3)
    S = model.state_count
    alpha = rng.normal(size=(40, S))
    bel = rng.random((30, S))
    bel /= bel.sum(axis=1, keepdims=True)
    A = [AlphaVector(r, 0) for r in alpha]
    Bl = [Belief(model, r) for r in bel]
    eng = _StubEngine(model)

    def query(na, nb):
        before = eng.pairs_scored
        got = eng.max_value_objects(A[:na], Bl[:nb], lambda v: v.values, lambda x: x.values)
        np.testing.assert_allclose(got, np.max(bel[:nb] @ alpha[:na].T, axis=1), rtol=1e-13)
        return eng.pairs_scored - before

    assert query(10, 12) == 10 * 12                    # cold
    assert query(15, 20) == 5 * 12 + 15 * 8            # 5 new alpha rows on 12 known beliefs + 8 new beliefs on all 15
    assert query(10, 20) == 10 * 8                     # the older alpha set again: only its 8 unseen beliefs
    assert query(10, 20) == 0 and query(15, 20) == 0   # exact hits
    assert query(15, 21) == 15                         # one more belief
    got = eng.max_value_objects(A[20:25], Bl[:5], lambda v: v.values, lambda x: x.values)    # unrelated set
    np.testing.assert_allclose(got, np.max(bel[:5] @ alpha[20:25].T, axis=1), rtol=1e-13)
    eng.reset_store('alpha')                           # ids restart: nothing cached may be reused
    for v in A:
        v.__dict__.pop('_dev', None)
    assert query(12, 6) == 12 * 6


def test_store_ids_travel_with_the_containers():
    """ValueFunction.extend and BeliefSet.union carry the device-store ids of their rows (Engine.row_ids caches them per
    container): a slot taken over on equal bytes keeps its id, new rows bring theirs, and what row_ids would find by
    walking the objects is what the carried array says -- so a solve never walks 10^4 objects per call."""
    from pomdp_pbvi_exploration_amd.mdp import AlphaVector
    model, _ = load_POMDP_file(os.path.join(EXAMPLES, '4x3.95-no_loop_2_grid.POMDP'))
    rng = np.random.default_rng(11)
    S = model.state_count
    eng = _StubEngine(model)
    old = ValueFunction(model, rng.normal(size=(6, S)), [0, 1, 2, 3, 0, 1])
    ids_old = eng.row_ids('alpha', old.alpha_vector_list, lambda v: v.values, owner=old)
    assert list(ids_old) == [0, 1, 2, 3, 4, 5] and old._dev_ids[1] is ids_old
    # a backup's result: two new rows and one that repeats an old row's bytes, every vector tagged with its store id
    rows = np.vstack([rng.normal(size=(2, S)), old.alpha_vector_array[3:4]])
    first = eng.store_rows('alpha', rows)
    tag = (eng.serial, 'alpha', eng._store_epoch['alpha'])
    vecs = []
    for k, r in enumerate(rows):
        v = AlphaVector(r, 2)
        v._dev = (tag, first + k)
        vecs.append(v)
    new = ValueFunction(model, vecs)
    new.extend(old)
    assert len(new) == 8 and new._dev_ids is not None
    walked = [v._dev[1] for v in new.alpha_vector_list]          # the objects' own tags (old object took the repeated slot)
    assert [eng.rows['alpha'][i].tobytes() for i in new._dev_ids[1]] == [v.values.tobytes() for v in new.alpha_vector_list]
    assert sorted(walked) == sorted(set(walked)) and len(set(new._dev_ids[1].tolist())) == 8
    assert list(new._dev_ids[1]) == walked                       # the carried array says what the objects say ...
    assert set(ids_old.tolist()) <= set(new._dev_ids[1].tolist())     # ... and the id set only grows (old id 3 kept, new id 8 unused)
    assert eng.row_ids('alpha', new.alpha_vector_list, lambda v: v.values, owner=new) is new._dev_ids[1]
    new.append(AlphaVector(rng.normal(size=S), 0))               # any other change drops the cache
    assert new._dev_ids is None

    bel = rng.random((5, S))
    bel /= bel.sum(axis=1, keepdims=True)
    mine = BeliefSet(model, [Belief(model, r) for r in bel[:3]])
    eng.row_ids('belief', mine.belief_list, lambda b: b.values, owner=mine)
    theirs = BeliefSet(model, [Belief(model, bel[1].copy()), Belief(model, bel[3]), Belief(model, bel[4])])   # first one repeats
    eng.row_ids('belief', theirs.belief_list, lambda b: b.values, owner=theirs)
    both = mine.union(theirs)
    assert len(both) == 5 and both._dev_ids is not None
    assert [eng.rows['belief'][i].tobytes() for i in both._dev_ids[1]] == [b.values.tobytes() for b in both.belief_list]
    untagged = BeliefSet(model, [Belief(model, rng.dirichlet(np.ones(S)))])
    assert getattr(mine.union(untagged), '_dev_ids', None) is None     # a belief without a store row: walk on demand


def test_device_walk_draws_the_same_trajectory_as_the_host_walk():
    """PBVI_Solver._walk_device simulates the (a, o) trajectory first and updates the beliefs in one batched call; it
    must consume the random streams exactly like the step-by-step host walk (same beliefs, same order)."""
    from pomdp_pbvi_exploration_amd import FSVI_Solver
    from pomdp_pbvi_exploration_amd.mdp import VI_Solver
    model, _ = load_POMDP_file(os.path.join(EXAMPLES, '4x3.95-no_loop_2_grid.POMDP'))
    model.end_states = [3, 6]
    mdp_policy, _ = VI_Solver(gamma=0.95, eps=1e-6).solve(model, print_progress=False)
    solver = FSVI_Solver(gamma=0.95, eps=1e-6)
    for variant in ('fsvi', 'fsvi_eg'):
        seqs = []
        for device in (False, True):
            np.random.seed(4)
            random.seed(4)
            m = model
            if device:                                 # a model that claims GPU residency, backed by the stub
                m = copy.copy(model)
                m.is_on_gpu = True
                m._engine = _StubEngine(model)
            b0 = Belief(m)
            fn = solver.expand_fsvi if variant == 'fsvi' else solver.expand_fsvi_eg
            bs = fn(m, b0, mdp_policy, max_generation=60)
            seqs.append((np.array([b.values for b in bs.belief_list]), np.random.random(), random.random()))
        assert seqs[0][0].shape == seqs[1][0].shape == (60, model.state_count)
        np.testing.assert_array_equal(seqs[0][0], seqs[1][0])
        assert seqs[0][1:] == seqs[1][1:]              # both walks left the generators in the same state


def _example_model_path(name, tmp_path):
    src = os.path.join(EXAMPLES, name)
    if os.path.exists(src):
        return src
    import gzip
    dst = str(tmp_path / name)
    with gzip.open(src + '.gz', 'rb') as z, open(dst, 'wb') as fh:
        fh.write(z.read())
    return dst


def test_pomdp_file_loader_matches_reference_on_every_example_model(tmp_path):
    """All 25 Cassandra files the reference ships, against the tables its own loader built from them
    (tests/golden/pomdp_file_tables.json, sha256 per table): bit-identical wherever the reference's result is a
    proper model; where the reference mis-reads the file (fully specified entries with the value on the next line
    become row assignments and the rows stop summing to 1: hanks, network) this loader must produce a proper
    model instead; files the reference rejects are not constrained."""
    import hashlib
    ref = json.load(open(os.path.join(GOLDEN, 'pomdp_file_tables.json')))
    compared = fixed = 0
    for name, entry in sorted(ref.items()):
        if 'error' in entry:
            continue
        model, solver = load_POMDP_file(_example_model_path(name, tmp_path))
        assert (model.state_count, model.action_count, model.observation_count) == (entry['S'], entry['A'], entry['O']), name
        assert solver.gamma == entry['gamma'], name
        same = True
        for attr, want in entry['tables'].items():
            a = np.ascontiguousarray(getattr(model, attr))
            same &= (list(a.shape) == want['shape'] and str(a.dtype) == want['dtype'] and
                     hashlib.sha256(a.tobytes()).hexdigest() == want['sha256'])
        if entry['stochastic']:
            assert same, name
        if same:
            compared += 1                              # (ejs7's own rows do not sum to 1; both loaders keep them)
        else:
            assert np.allclose(model.transition_table.sum(axis=2), 1.0), name
            assert np.allclose(model.observation_table.sum(axis=2), 1.0), name
            fixed += 1
    assert compared == 20 and fixed == 2               # fixed: hanks.95, network.95


SOLVE_MODELS = ('tiger-grid.POMDP', 'hallway.POMDP', 'cheese.95.POMDP', '4x4.95.POMDP', '4x3.95.POMDP', 'cit.POMDP')


def solve_example(name, tmp_path, use_gpu=False, engine_dtype='f64'):
    """The call make_golden.gen_solve made on the reference, on this package."""
    z = load_npz('example_solves.npz')
    key = name.replace('.POMDP', '').replace('.', '_').replace('-', '_')
    model, solver = load_POMDP_file(_example_model_path(name, tmp_path))
    np.random.seed(0)
    random.seed(0)
    exps, growth = (int(x) for x in z[f'{key}_cfg'])
    vf, hist = FSVI_Solver(gamma=solver.gamma, eps=1e-6).solve(model, expansions=exps, max_belief_growth=growth,
                                                               use_gpu=use_gpu, engine_dtype=engine_dtype, print_progress=False)
    want = {k[len(key) + 1:]: z[k] for k in z if k.startswith(key + '_')}
    return vf, hist, want


@pytest.mark.parametrize('name', SOLVE_MODELS)
def test_fsvi_solves_of_example_models_match_reference_host(name, tmp_path):
    """Models with up to 28 observations and 56 reachable states per (s, a): trajectories and the final alpha set of
    the reference's seeded FSVI solve, reproduced by the host mirror."""
    vf, hist, want = solve_example(name, tmp_path)
    assert hist.beliefs_counts == list(want['beliefs'])
    assert hist.alpha_vector_counts == list(want['alphas'])
    assert np.array_equal(np.asarray(vf.actions), want['actions'])
    np.testing.assert_allclose(vf.alpha_vector_array, want['alpha'], rtol=1e-12, atol=1e-12)


def test_backup_in_belief_chunks_halves_until_one_fits_and_gives_the_block_result():
    """PBVI_Solver._backup_in_chunks (what backup does after the engine's MemoryError): the belief list goes through in chunks,
    halved until one fits, the value function is uploaded again after every failure (the engine forgets everything on OOM),
    the caller's formulation setting comes back, the result is the block's, and a single belief that does not fit re-raises."""
    from types import SimpleNamespace
    model, _ = load_POMDP_file(os.path.join(EXAMPLES, '4x3.95-no_loop_2_grid.POMDP'))
    rng = np.random.default_rng(5)
    S = model.state_count
    vf = ValueFunction(model, rng.normal(size=(9, S)), rng.integers(0, model.action_count, 9))
    bel = rng.random((37, S))
    bel /= bel.sum(axis=1, keepdims=True)
    beliefs = [Belief(model, r) for r in bel]
    solver = PBVI_Solver(gamma=0.95, eps=1e-6)

    class Dev:
        """NumPy stand-in for the engine calls of the chunk loop; `fits` beliefs at most per run."""
        def __init__(self, fits):
            self.fits, self.formulation, self.log, self.alpha, self.block = fits, 'alpha', [], None, None

        def set_formulation(self, which):
            self.formulation = which
            self.log.append(('formulation', which))

        def sync_rows(self, which, objs, values_of, owner=None):
            rows = np.array([values_of(x) for x in objs])
            if which == 'alpha':
                self.alpha = rows
                self.log.append(('alpha', len(rows)))
            else:
                self.block = rows

        def run(self, gamma, prune):
            if len(self.block) > self.fits:
                self.alpha = self.block = None                       # pbvi_engine_after_oom: nothing resident any more
                self.log.append(('oom', None))
                raise MemoryError('stub: block too large')
            assert self.alpha is not None, 'the value function was not uploaded again after the failure'
            assert self.formulation == 'belief'
            self.log.append(('run', len(self.block)))
            return {}

        def fetch(self):
            rows, acts = solver._backup_numpy(model, self.block, self.alpha, False)
            return SimpleNamespace(value_function_rows=lambda use_keep=False: (rows, acts))

    want_rows, want_acts = solver._backup_numpy(model, bel, vf.alpha_vector_array, False)
    want = ValueFunction(model, want_rows, want_acts)
    dev = Dev(fits=6)
    rows, acts = solver._backup_in_chunks(dev, vf, beliefs, False)
    got = ValueFunction(model, rows, acts)
    assert solver._belief_chunk == 5                                 # 19 -> 10 -> 5
    assert [x for x in dev.log if x[0] == 'oom'] == [('oom', None)] * 2
    assert [n for k, n in dev.log if k == 'run'] == [5] * 7 + [2]
    assert sum(1 for k, _ in dev.log if k == 'alpha') == 3          # once per attempt
    assert dev.formulation == 'alpha'                               # the caller's setting
    assert len(got) == len(want)
    key = lambda v: (v.alpha_vector_array[np.lexsort(v.alpha_vector_array.T[::-1])], )
    np.testing.assert_array_equal(key(got)[0], key(want)[0])
    # a later, larger block of the same solve starts at the size that fitted
    dev2 = Dev(fits=6)
    solver._backup_in_chunks(dev2, vf, beliefs, False)
    assert not [x for x in dev2.log if x[0] == 'oom']
    # nothing fits: the error reaches the caller (solve turns it into the partial result)
    solver._belief_chunk = None
    with pytest.raises(MemoryError):
        solver._backup_in_chunks(Dev(fits=0), vf, beliefs, False)


def test_backup_in_belief_chunks_never_exceeds_the_engine_block_limit():
    """A belief list longer than twice the engine's block limit: the first chunk (half the list) would be refused by the
    engine with PBVI_EUNSUPPORTED, which Engine._ck raises as RuntimeError -- not the MemoryError the halving loop catches.
    The chunk is clamped to BELIEF_BLOCK, so the refusal is never provoked, and the union of the chunks' rows is the
    unchunked NumPy result."""
    from types import SimpleNamespace
    model, _ = load_POMDP_file(os.path.join(EXAMPLES, '4x3.95-no_loop_2_grid.POMDP'))
    rng = np.random.default_rng(11)
    S = model.state_count
    vf = ValueFunction(model, rng.normal(size=(9, S)), rng.integers(0, model.action_count, 9))
    bel = rng.random((37, S))
    bel /= bel.sum(axis=1, keepdims=True)
    beliefs = [Belief(model, r) for r in bel]
    solver = PBVI_Solver(gamma=0.95, eps=1e-6)
    LIMIT = 8
    solver.BELIEF_BLOCK = LIMIT
    assert len(beliefs) > 2 * LIMIT

    class Dev:
        """NumPy stand-in for the engine: blocks above `limit` are refused as pbvi_beliefs_select refuses them (status
        PBVI_EUNSUPPORTED -> RuntimeError in Engine._ck), blocks above `fits` run out of memory."""
        def __init__(self, limit, fits):
            self.limit, self.fits, self.formulation, self.runs, self.alpha, self.block = limit, fits, 'auto', [], None, None

        def set_formulation(self, which):
            self.formulation = which

        def sync_rows(self, which, objs, values_of, owner=None):
            rows = np.array([values_of(x) for x in objs])
            if which == 'alpha':
                self.alpha = rows
                return
            if len(rows) > self.limit:
                raise RuntimeError(f'pbvi engine error -4: at most {self.limit} beliefs per block')
            self.block = rows

        def run(self, gamma, prune):
            if len(self.block) > self.fits:
                self.alpha = self.block = None
                raise MemoryError('stub: block too large')
            self.runs.append(len(self.block))
            return {}

        def fetch(self):
            rows, acts = solver._backup_numpy(model, self.block, self.alpha, False)
            return SimpleNamespace(value_function_rows=lambda use_keep=False: (rows, acts))

    want_rows, want_acts = solver._backup_numpy(model, bel, vf.alpha_vector_array, False)
    want = ValueFunction(model, want_rows, want_acts)
    srt = lambda v: v.alpha_vector_array[np.lexsort(v.alpha_vector_array.T[::-1])]
    dev = Dev(limit=LIMIT, fits=LIMIT)
    rows, acts = solver._backup_in_chunks(dev, vf, beliefs, False)
    assert dev.runs == [8, 8, 8, 8, 5] and solver._belief_chunk == LIMIT
    got = ValueFunction(model, rows, acts)
    assert len(got) == len(want)
    np.testing.assert_array_equal(srt(got), srt(want))
    assert dev.formulation == 'auto'
    # the block limit and a memory limit below it together: clamped first, then halved (8 -> 4 -> 2)
    solver._belief_chunk = None
    dev = Dev(limit=LIMIT, fits=3)
    rows, acts = solver._backup_in_chunks(dev, vf, beliefs, False)
    assert solver._belief_chunk == 2 and set(dev.runs) <= {1, 2} and sum(dev.runs) == len(beliefs)
    np.testing.assert_array_equal(srt(ValueFunction(model, rows, acts)), srt(want))
    # a chunk size remembered from a solve with a larger limit is clamped too
    solver._belief_chunk = 3 * LIMIT
    dev = Dev(limit=LIMIT, fits=LIMIT)
    solver._backup_in_chunks(dev, vf, beliefs, False)
    assert max(dev.runs) == LIMIT


def _numpy_exchange_merge(all_meta, per, kw, n_total):
    """The NumPy merge pbvi_exchange_merge replaced: distinct keys in order of first occurrence over the ranks'
    messages, and per belief (global order) the position of its key."""
    world = all_meta.shape[0]
    rows, owner = [], []
    for r in range(world):
        c = int(all_meta[r, 0])
        rows.append(all_meta[r, 1 + 3 * per:1 + 3 * per + c * kw].reshape(c, kw))
        owner.append(np.full(c, r))
    rows = np.concatenate(rows)
    base = np.concatenate([[0], np.cumsum([int(all_meta[r, 0]) for r in range(world)])])
    uniq, first, inv = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind='stable')                 # np.unique sorts: back to first-occurrence order
    rank_of = np.empty(len(order), dtype=np.int64)
    rank_of[order] = np.arange(len(order))
    pos = rank_of[np.asarray(inv).reshape(-1)]
    idx, act, keep = [], [], []
    for r in range(world):
        lo = min(r * per, n_total)
        n = min(lo + per, n_total) - lo
        idx.append(pos[base[r] + all_meta[r, 1:1 + n]])
        act.append(all_meta[r, 1 + per:1 + per + n])
        keep.append(all_meta[r, 1 + 2 * per:1 + 2 * per + n] != 0)
    return rows[np.sort(first)], np.concatenate(idx), np.concatenate(act), np.concatenate(keep)


@pytest.mark.parametrize('key_width', [3, 64, 65, 201])
def test_exchange_merge_of_wide_keys_equals_the_numpy_merge(key_width):
    """pbvi_exchange_merge (host code, no GPU) for key widths 1 + O up to and beyond 64 -- a model with 63, 64 or 200
    observations -- against the NumPy merge it replaced.  Keys repeat within and across ranks and differ only in their LAST
    entry in places, so a comparison that stopped at 64 entries would merge distinct keys."""
    from pomdp_pbvi_exploration_amd.dist import merge_exchange
    rng = np.random.default_rng(100 + key_width)
    world, per, n_total = 3, 23, 3 * 23 - 4
    pool = rng.integers(0, 5, size=(12, key_width)).astype(np.int32)
    pool[1] = pool[0]
    pool[1, -1] += 1                                         # equal up to the last entry
    pool[3] = pool[2]
    pool[3, 0] += 1
    n_meta = 1 + 3 * per + per * key_width
    allm = np.zeros((world, n_meta + 2), dtype=np.int32)     # a trailer may follow the payload
    for r in range(world):
        c = int(rng.integers(3, per + 1))
        keys = pool[rng.integers(0, len(pool), c)]
        n = min(per, n_total - r * per)
        allm[r, 0] = c
        allm[r, 1:1 + n] = rng.integers(0, c, n)
        allm[r, 1 + per:1 + per + n] = rng.integers(0, 4, n)
        allm[r, 1 + 2 * per:1 + 2 * per + n] = rng.integers(0, 2, n)
        allm[r, 1 + 3 * per:1 + 3 * per + c * key_width] = keys.reshape(-1)
    keys, idx, act, keep = merge_exchange(allm, per, key_width, n_total)
    wk, wi, wa, wkeep = _numpy_exchange_merge(allm, per, key_width, n_total)
    np.testing.assert_array_equal(keys, wk)
    np.testing.assert_array_equal(idx, wi)
    np.testing.assert_array_equal(act, wa)
    np.testing.assert_array_equal(keep, wkeep)
    assert len(keys) < sum(int(c) for c in allm[:, 0])       # the case does merge keys


def test_exchange_merge_refuses_what_the_int32_message_cannot_hold():
    """The bounds that replaced ``key_width <= 64``: a key needs at least one entry, and one message -- 1 + per (3 + key_width)
    int32 words, addressed by int32 positions -- must fit the int32 range.  The second call passes every other check (the
    stride is larger than the message, world * per and n_total are small), so only that bound can refuse it; it returns
    before anything is read or allocated."""
    import ctypes as C
    from pomdp_pbvi_exploration_amd.dist import merge_exchange
    from pomdp_pbvi_exploration_amd.engine import load_library
    with pytest.raises(ValueError):
        merge_exchange(np.zeros((1, 8), dtype=np.int32), 1, 0, 1)                     # no key at all
    lib = load_library()
    meta = np.zeros(8, dtype=np.int32)
    out = np.zeros(8, dtype=np.int32)
    per, kw = 2 ** 29, 5                                                               # per * (3 + kw) = 2^32
    rc = lib.pbvi_exchange_merge(meta.ctypes.data, 1, 2 ** 40, per, kw, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                                 out.ctypes.data)
    assert rc == -1 and b'do not fit' in lib.pbvi_last_error()
    per = (2 ** 31 - 1) // (kw + 3) + 1                                                # the first block size past the bound
    rc = lib.pbvi_exchange_merge(meta.ctypes.data, 1, 2 ** 40, per, kw, 1, out.ctypes.data, out.ctypes.data, out.ctypes.data,
                                 out.ctypes.data)
    assert rc == -1 and b'do not fit' in lib.pbvi_last_error()


def test_twin_rows_make_fp32_and_fp64_decisions_disagree_on_the_host():
    """CPU check of the construction behind test_run_fetch_slot_overflow_falls_back_to_the_plain_order (no engine): emulated
    fp32 accumulation, in either order and with or without a fused multiply-add, picks another row than fp64 for a large
    share of the beliefs."""
    from pomdp_pbvi_exploration_amd import synth
    S, rs, rto, er, alpha, b = synth.twin_rows_case()
    B = b.shape[0]
    exact = np.argmax(b @ alpha.T, axis=1)
    assert np.array_equal(exact, 2 * np.arange(B) + 1)       # fp64: always the twin
    a32, b32 = alpha.astype(np.float32), b.astype(np.float32)
    i = np.arange(B)
    for fused in (False, True):
        for order in (0, 1):
            s0, s1 = (2 * i, 2 * i + 1) if order == 0 else (2 * i + 1, 2 * i)
            score = np.empty((B, 2), dtype=np.float32)
            for t in range(2):
                row = 2 * i + t
                first = (b32[i, s0] * a32[row, s0]).astype(np.float32)
                if fused:
                    score[:, t] = (first.astype(np.float64) + b32[i, s1].astype(np.float64) * a32[row, s1].astype(np.float64)).astype(np.float32)
                else:
                    score[:, t] = (first + (b32[i, s1] * a32[row, s1]).astype(np.float32)).astype(np.float32)
            first_max = 2 * i + np.argmax(score, axis=1)
            assert np.count_nonzero(first_max != exact) > B // 4, (fused, order, np.count_nonzero(first_max != exact))
