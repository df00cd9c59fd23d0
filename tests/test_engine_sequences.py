"""Any order of engine calls must equal a fresh engine.

An ``Engine`` lives for thousands of calls and carries a lot from one to the next (dead-triple maps, tile lists, sort orders,
the pre-split belief plane, the primary alpha layout and its magnitude row, the fp32 screen's mirror, zeroed pad rows, the
fused tile map, the belief store's zero maps, the speculation about the refinement, the fetchable result).  The invariant:

    what a call returns is a function of the engine's logical state -- tables, working alpha set, belief block, row stores,
    state weights, the point store of the upper bound, the state policies' table, switches -- and not of the calls that
    produced that state.

``sequence_cases.py`` holds the sequences (scripted ones aimed at one carry-over each, seeded random ones), the shadow of
the logical state and the ``Runner`` that, after every query, compares the engine with (a) the fp64 host statements on the
shadow's arrays and (b) a fresh engine brought to that state by ``set_alpha`` / ``set_beliefs`` / ``set_state_policy``:
indices, actions, masks, unique rows, keys, hashes, ``q``, infotaxis, space-aware infotaxis, the sawtooth bound and its action
values (over a point store the fresh engine receives in ONE append), ``fetch_beliefs`` and rollout trajectories byte for byte,
the state policies' actions, states and votes byte for byte against both (the three rules are defined bit for bit), value
maxima (also through ``max_value_objects``) and, where the score probe is on, ``best_score`` at the bar.  Where the engine's
own output becomes state (``advance_beliefs``, ``belief_walk``, rollout survivors, ``store_unique``) it is checked against the
host statement at the bar and its bits are adopted into the shadow.  ``sweeps_beside`` runs three sweeps of a handle-free
entry (FIB, the blind controller, MDP value iteration) between two calls of the engine, bit-equal to its host statement.

CPU tests: every sequence runs against ``HostEngine`` (the host statements under ``Engine``'s method names) with no entry
skipped as undecidable; seventeen stand-ins with one planted carry-over bug each fail a scripted and a seeded sequence; the
operation lists cover the vocabulary.  GPU tests: the same sequences on the HIP engine, both models, both engine types.
"""
import functools
import json
import os

import numpy as np
import pytest

import sequence_cases as sc

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'engine_sequences.json')
MIB = 1 << 20


@functools.lru_cache(maxsize=None)
def committed():
    """The seeded sequences as committed: ``{'<model>-<dtype>-<seed>': operations}`` (``sc.generate`` reproduces each)."""
    with open(GOLDEN) as f:
        return {k: sc.from_json(v) for k, v in json.load(f).items()}


def seeded_ops(mname, dtype, seed):
    return committed()[f'{mname}-{dtype}-{seed}']


def all_sequences():
    out = [(mname, dtype, sc.SCRIPTED[name][2]) for name, mname, dtype in sc.scripted_cases()]
    return out + [(mname, dtype, seeded_ops(mname, dtype, seed)) for mname, dtype, seed in sc.seeded_cases()]


def host_runner(mname, dtype, cls=sc.HostEngine):
    return sc.Runner(mname, dtype, lambda: cls(mname, dtype))


# --------------------------------------------------------------------------------------------------------------------- #
# the harness itself, on the host
# --------------------------------------------------------------------------------------------------------------------- #
@pytest.mark.parametrize('name,mname,dtype', sc.scripted_cases())
def test_scripted_sequence_on_the_host_engine(name, mname, dtype):
    r = host_runner(mname, dtype).run(sc.SCRIPTED[name][2])
    assert r.entries > 0 and r.skipped == 0, (r.skipped, r.entries)


@pytest.mark.parametrize('mname,dtype,seed', sc.seeded_cases())
def test_seeded_sequence_is_the_generators_and_legal(mname, dtype, seed):
    """``generate`` runs the list it draws through a ``HostEngine`` with every comparison on (and refuses a skipped entry);
    the committed list is that list."""
    ops = sc.generate(mname, dtype, seed)
    assert len(ops) == sc.N_RANDOM_OPS
    assert sc.to_json(ops) == sc.to_json(seeded_ops(mname, dtype, seed))
    n_value = sum(name in sc.VALUE_QUERIES for name, _ in ops)          # (fetch_refused compares no value)
    n_backup = sum(name in sc.BACKUPS for name, _ in ops)
    assert sc.MIN_VALUE_QUERIES <= n_value <= 18 and n_backup >= sc.MIN_BACKUPS, (n_value, n_backup)


def fails(mname, dtype, cls, ops):
    try:
        host_runner(mname, dtype, cls).run(ops)
    except sc.Mismatch:
        return True
    return False


@pytest.mark.parametrize('defect', list(sc.DEFECTS))
def test_a_planted_carry_over_fails_a_scripted_and_a_seeded_sequence(defect):
    cls = sc.DEFECTS[defect]
    name = sc.DEFECT_SCRIPTS[defect]
    models, dtypes, ops = sc.SCRIPTED[name]
    assert any(fails(m, d, cls, ops) for m in models for d in dtypes), f'{defect}: {name} passes'
    assert any(fails(m, d, cls, seeded_ops(m, d, s)) for m, d, s in sc.seeded_cases()), f'{defect}: every seeded sequence passes'


def test_the_sequences_cover_the_vocabulary():
    cov = sc.coverage(all_sequences())
    rare = {k: v for k, v in cov.counts.items() if v < 5}
    assert not rare, rare
    missing = {(m, q) for m in sc.MUTATIONS for q in sc.QUERIES} - sc.NEVER_LEGAL_AFTER_A_RESET - sc.NEVER_LEGAL_BY_CONSTRUCTION - cov.pairs
    assert not missing, sorted(missing)
    for name, values in sc.SWITCH_VALUES.items():                      # every listed value; away from the default and back
        seen = {v for n, v in cov.switch_values if n == name}
        assert seen >= set(values), (name, set(values) - seen)
        assert name in cov.returned, name
    assert cov.envs >= {('table', False), ('table', True), ('frames', False), ('frames', True)}, cov.envs
    assert set(sc.B_EDGES) <= cov.Bs and set(sc.V_EDGES) <= cov.Vs, (cov.Bs, cov.Vs)
    assert cov.hows >= {'small', 'primary', 'all', 'fresh'}
    # the greedy calls: every kind of weights, every window, both objectives with and without terms, in the model's world and
    # against both environments; appends of 0, 1 and several points, supports on both sides of a wavefront, point counts
    # below, at and above one chunk of the sawtooth, hits in blocks on both sides of the sorted-block threshold
    assert cov.kinds >= set(sc.tsa.WEIGHT_KINDS), cov.kinds
    assert cov.windows >= set(sc.WINDOWS) and cov.q_windows >= {(w, e) for w in sc.WINDOWS for e in (False, True)}, (cov.windows, cov.q_windows)
    assert cov.space_aware >= {(o, t) for o in (0, 1) for t in (False, True)}, cov.space_aware
    assert cov.sa_rollouts >= {(o, e) for o in (0, 1) for e in (None, 'table', 'frames')}, cov.sa_rollouts
    assert cov.appends >= {0, 1, 63, 64, 65} and cov.supports >= set(sc.hc.SUPPORTS), (cov.appends, cov.supports)
    assert cov.hit_blocks >= {3, 257, 300}, cov.hit_blocks
    assert cov.mapping >= {(w, a, u) for w in (0, 1) for a, u in ((True, True), (True, False), (False, True))}, cov.mapping
    # the state policies: every kind of table, every rule with hashed uniforms and rule 2 with given ones (uniforms belong to
    # rule 2 only), the long and the short forms, every rule's rollout in the model's world and against both environments, all
    # three handle-free entries beside the engine
    assert cov.table_kinds >= set(sc.POLICY_KINDS), cov.table_kinds
    assert cov.rule_draws >= {(0, 'hashed'), (1, 'hashed'), (2, 'hashed'), (2, 'uniforms')}, cov.rule_draws
    assert cov.want_state == {False, True} and cov.want_votes == {False, True}, (cov.want_state, cov.want_votes)
    assert cov.sp_rollouts >= {(r, e) for r in (0, 1, 2) for e in (None, 'table', 'frames')}, cov.sp_rollouts
    assert cov.sweeps >= set(sc.SWEEP_KINDS), cov.sweeps
    # the four forms a selection of alpha rows takes, named by the shadow's restatement of the engine's bookkeeping, and the
    # blocks a state_policy query has seen (both sorted sizes among them)
    forms, policy_blocks = set(), set()
    for mname, dtype, ops in all_sequences()[:len(sc.scripted_cases())]:
        r = host_runner(mname, dtype).run(ops)
        forms |= set(r.forms)
        policy_blocks |= r.policy_blocks
    assert forms >= {'extend', 'exhaust', 'small', 'primary', 'fresh'}, forms
    assert policy_blocks >= {3, 128, 257, 300}, policy_blocks


def test_the_backup_reference_is_the_oracles():
    """``sc.backup_ref`` (reference (a), with the decidability of every choice) against ``orc.backup_core``,
    ``orc.belief_dominance_mask`` and ``_q_values_numpy`` on inputs without ties."""
    from oracle import pbvi_oracle as orc
    from pomdp_pbvi_exploration_amd.pomdp import _q_values_numpy
    for mname in sc.MODELS:
        m = sc.model(mname)
        alpha = sc.f32r(np.random.default_rng(5).normal(scale=4.0, size=(37, m.S)))
        bel = sc.belief_rows(mname, B=29, seed=5)
        ref = sc.backup_ref(mname, alpha, bel, tol=1e-12)
        rows, act, best = orc.backup_core(alpha, bel, m.rs, m.rto, m.er, sc.GAMMA)
        assert ref.decided.all() and ref.row_ok.all() and ref.keep_ok.all()
        assert np.array_equal(ref.best, best) and np.array_equal(ref.act, act)
        np.testing.assert_allclose(ref.rows, rows, rtol=1e-13, atol=1e-13 * np.abs(rows).max())
        assert np.array_equal(ref.keep, orc.belief_dominance_mask(alpha, bel, rows))
        assert np.array_equal(ref.rows[np.unique(ref.index, return_index=True)[1]], ref.urows)
        np.testing.assert_allclose(ref.q, _q_values_numpy(m.tables, bel, alpha, sc.GAMMA), rtol=1e-12)


def test_a_switch_toggled_back_is_remembered_and_compared():
    """``remember`` / ``same_as`` compare byte for byte: a stand-in that answers differently the second time is caught."""
    class Drifting(sc.HostEngine):
        def max_value_resident(self):
            self.calls = getattr(self, 'calls', 0) + 1
            val, idx = super().max_value_resident()
            return val * (1.0 + 2.0 ** -50 * (self.calls > 1)), idx
    ops = [sc.op('set_alpha', V=5, seed=1), sc.op('set_beliefs', B=3, seed=1), sc.op('vmax_resident'), sc.op('remember', tag='v'),
           sc.op('vmax_resident'), sc.op('same_as', tag='v')]
    host_runner('I', 'f64').run(ops)
    assert fails('I', 'f64', Drifting, ops)


@pytest.mark.parametrize('mname', sc.MODELS)
@pytest.mark.parametrize('dtype', sc.DTYPES)
def test_a_store_window_left_as_the_resident_block_is_caught(mname, dtype):
    """``store_operand_beside_a_sorted_block`` is aimed at a ``max_value_store`` that scores the store's windows through the
    resident block's own fields: a stand-in that leaves the last window there fails it, on every model and engine type."""
    class WindowLeft(sc.HostEngine):
        def max_value_store(self, n=-1):
            out = super().max_value_store(n)
            self.bel = np.stack(self.bstore)[-32768:]
            return out
    ops = sc.SCRIPTED['store_operand_beside_a_sorted_block'][2]
    assert fails(mname, dtype, WindowLeft, ops)


# --------------------------------------------------------------------------------------------------------------------- #
# the HIP engine
# --------------------------------------------------------------------------------------------------------------------- #
def device_runner(mname, dtype):
    from pomdp_pbvi_exploration_amd import engine as em
    m = sc.model(mname)

    def make():
        return em.Engine(m.S, m.A, m.O, m.R, m.rs, m.rto, m.er, dtype=dtype)

    def alloc(shape, dt):
        return em.PinnedBuffer(int(np.prod(shape)) * np.dtype(dt).itemsize + 256).carve(shape, dt)

    def provoke_oom(eng):
        """``store_rows`` under a cap 4 MiB above what the engine holds (tests/test_engine_memory.py), of more rows than
        all it holds plus 8 MiB: however much room the store has left, it has to grow past the cap."""
        row_bytes = -(-m.S // 32) * 32 * (4 if dtype == 'f32' else 8)
        big = np.zeros(((eng.device_bytes + 8 * MIB) // row_bytes + 1, m.S))
        prev = em.debug_alloc_limit(eng.device_bytes // MIB + 4)
        try:
            with pytest.raises(MemoryError):
                eng.store_rows('alpha', big)
        finally:
            em.debug_alloc_limit(prev)

    def sweeps(mname, which):
        """Three sweeps of a handle-free entry on the model's tables (the arguments of ``sc.sweeps_ref``'s host statements)."""
        t, args = m.tables, sc.sweep_inputs(mname, which)
        if which == 'fib':
            return em.fib_value_iteration(t.reachable_states, t.reachable_transitional_observation_table, t.expected_rewards_table,
                                          *args, sc.SWEEP_GAMMA, 0.0, 3)
        if which == 'controller':
            return em.controller_value_iteration(t.reachable_states, t.reachable_transitional_observation_table,
                                                 t.expected_rewards_table, *args, sc.SWEEP_GAMMA, 0.0, 3)
        return em.mdp_value_iteration(*sc.tmd.mdp_tables(t), *args, sc.SWEEP_GAMMA, 0.0, 3)

    return sc.Runner(mname, dtype, make, alloc=alloc, provoke_oom=provoke_oom, sweeps=sweeps)


def run_on_device(mname, dtype, ops):
    r = device_runner(mname, dtype)
    try:
        r.run(ops)
    finally:
        r.close()
    assert r.skipped == 0, (r.skipped, r.entries)
    # value maxima are compared at the bar; on every committed sequence they are also the fresh engine's bits
    assert all(r.vmax_bits), r.vmax_bits
    # ... and so is best_score wherever the probe was on (the largest error seen, in bars, for pytest -s)
    assert all(r.score_bits), r.score_bits
    if r.score_bits:
        print(f'best_score: largest error {r.score_ratio:.3f} of its bar over {len(r.score_bits)} probed backups')
    print(f'value maxima equal to the fresh engine\'s bit for bit in {sum(r.vmax_bits)} of {len(r.vmax_bits)} queries')
    return r


@pytest.mark.gpu
@pytest.mark.parametrize('name,mname,dtype', sc.scripted_cases())
def test_scripted_sequence(name, mname, dtype):
    run_on_device(mname, dtype, sc.SCRIPTED[name][2])


@pytest.mark.gpu
@pytest.mark.parametrize('mname,dtype,seed', sc.seeded_cases())
def test_seeded_sequence(mname, dtype, seed):
    run_on_device(mname, dtype, seeded_ops(mname, dtype, seed))
