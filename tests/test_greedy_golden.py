"""The bits of the greedy successor policies that ``test_successor_golden.py`` and ``test_rollout_golden.py`` do not pin:
``space_aware_resident``, ``rollout_space_aware`` and the two policies interleaved on one engine -- sha256 of every returned
array against tests/golden/greedy_digests.json.

The file was recorded on an MI355X (twice, with the same digests in every case, so none had to be dropped) from the commit
that added space-aware infotaxis as a second copy of infotaxis at every layer (b7d3b39).  The refactor that folded the two
policies into one finish kernel, one launcher, one engine stage with one buffer family and one host loop had to reproduce
it without re-recording.  A later change that alters these bits on purpose must re-record the file
(``python tests/test_greedy_golden.py --record FILE`` on the device) and say why.

Every case is the smallest at which its path can still go wrong; the models, rows and environments are the ones of the two
other golden files:
  * ``space_aware_resident(objective, want_terms=True)``, objectives 0 and 1, on the models of
    ``test_successor_golden.INFOTAXIS``: the ragged model with O = 5 at S = 300 (two observation passes, the second of one),
    the identity model (the ``R == 1`` branch), the ragged model at S = 2100 (two x-blocks); blocks of 6 rows (a full group of
    four beliefs and a ragged group of two) and, at S = 300, of 300 rows (sorted, ``perm`` is read).  The weights hold zeros,
    non-integers and one large entry; the all-zero vector runs on the 6-row O = 5 block.
  * ``rollout_space_aware``, both objectives, on the S = 700 ragged model (three push blocks, the norm summed in block
    order), 1100 rows and T = 6: in the model's world, against the frames (non-zero shifts, ``end_observation`` 1) and
    against the table (``end_observation`` -1) of ``test_rollout_golden``, whose model has the dead fourth observation.
    After each rollout the same call on the first 300 rows of the same engine: buffers reused after shrinking.  The four
    or five arrays, ``eng.B`` and the beliefs left resident.
  * one engine, 6 rows of the O = 5 model: ``infotaxis_resident(True, True)``, ``space_aware_resident(0, True)``,
    ``infotaxis_resident(True, True)``, ``space_aware_resident(1, True)`` -- the two policies work in the same device buffers,
    so each must leave nothing behind that the other reads.  The engine then holds what a fresh engine holds after the
    space-aware calls alone, plus the ``[B]`` entropies that only infotaxis asks for: ``B * 8`` bytes.  (At b7d3b39 each policy
    had buffers of its own and the engine held the partials ``[XB,B,A,O,2]``, ``G [B,A]``, the actions ``[B]`` and
    ``p_obs [B,A,O]`` a second time.)
The host tests pin ``space_aware_numpy``, ``space_aware_terms`` and ``rollout_space_aware_numpy`` on the same inputs to the
doubles they returned at b7d3b39, and hold the cases to this description."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest                                                         # noqa: F401  (puts the repository on sys.path)

import test_rollout_golden as rg
import test_successor_golden as sg
from pomdp_pbvi_exploration_amd.pomdp import (FrameEnvironment, rollout_space_aware_numpy, space_aware_numpy,
                                              space_aware_terms)

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'greedy_digests.json')
DTYPES, CASTS = sg.DTYPES, sg.CASTS
OBJECTIVES = (0, 1)
MODELS = sg.INFOTAXIS                                  # model -> block sizes
ZERO_CASE = ('ragged300_o5', 6)                        # the all-zero weights run here
S_ROLLOUT, N_HOST = 700, 40
WORLDS = {'model': None, 'frames': ('frames', 1), 'table': ('table', -1)}      # world -> (environment kind, end_observation)
TERM_NAMES = ('Z', 'N', 'D', 'M_Z', 'M_N', 'M_D')
ROLLOUT_NAMES = ('states', 'actions', 'observations', 'steps', 'lost')
_CACHE = {}
sha = sg.sha


# --------------------------------------------------------------------------------------------------------------------- #
# cases (seeded, built once)
# --------------------------------------------------------------------------------------------------------------------- #
def weights(S):
    """``w [S]``: about a fifth zeros, non-integers below 10 elsewhere, and one entry of 1e6."""
    if ('w', S) not in _CACHE:
        rng = np.random.default_rng(9400 + S)
        w = rng.random(S) * 10.0
        w[rng.random(S) < 0.2] = 0.0
        w[int(rng.integers(0, S))] = 1.0e6
        _CACHE[('w', S)] = w
    return _CACHE[('w', S)]


def rollout_case(world):
    """``(tables, environment or None)`` of a rollout case: the model has the dead observation where an environment emits it."""
    c = rg.tables(S_ROLLOUT, dead=world != 'model')
    return c, (None if world == 'model' else rg.environment(S_ROLLOUT, *WORLDS[world]))


def host_resident(name, dtype):
    c, out = sg.model(name), {}
    w = weights(c.m.state_count)
    for n in MODELS[name]:
        for objective in OBJECTIVES:
            out[f'n{n}_obj{objective}'] = space_aware_numpy(c.m, c.rows[:n], w, objective, CASTS[dtype])
        out[f'n{n}_terms'] = space_aware_terms(c.m, c.rows[:n], w, CASTS[dtype])
    out['n6_terms_3_at_once'] = space_aware_terms(c.m, c.rows[:6], w, CASTS[dtype], rows_at_once=3)
    if name == ZERO_CASE[0]:
        for objective in OBJECTIVES:
            out[f'n6_obj{objective}_zero'] = space_aware_numpy(c.m, c.rows[:6], np.zeros(c.m.state_count), objective, CASTS[dtype])
    return out


def host_rollout(world, objective):
    key = ('host_rollout', world, objective)
    if key not in _CACHE:
        c, env = rollout_case(world)
        _CACHE[key] = rollout_space_aware_numpy(c.m, c.b0[:N_HOST], c.s0[:N_HOST], weights(S_ROLLOUT), rg.SEED, rg.FIRST_ID,
                                                rg.T_STEPS, objective, env=None if env is None else env.rows(0, N_HOST))
    return _CACHE[key]


def host_digests():
    out = {}
    for dtype in DTYPES:
        for name in MODELS:
            out[f'host_space_aware_{name}/{dtype}'] = {k: [sha(x) for x in v] for k, v in host_resident(name, dtype).items()}
    for world in WORLDS:
        for objective in OBJECTIVES:
            out[f'host_rollout_{world}_obj{objective}'] = [sha(x) for x in host_rollout(world, objective)]
    return out


def golden(key):
    """The recorded digests of ``key``; a key that is missing from the file fails the test (KeyError), it never skips."""
    if 'file' not in _CACHE:
        with open(GOLDEN_FILE) as f:
            _CACHE['file'] = json.load(f)
    return _CACHE['file'][key]


# --------------------------------------------------------------------------------------------------------------------- #
# host (no GPU): the cases are what the description says, and the host restatements return the recorded doubles
# --------------------------------------------------------------------------------------------------------------------- #
def test_cases_are_what_the_description_says():
    assert 'PBVI_NO_BELIEF_SORT' not in os.environ
    per_pass, per_thread, x_block = 4, 4, 8 * 256              # observations per pass, beliefs per thread, states per x-block
    assert {-(-sg.model(name).m.state_count // x_block) for name in MODELS} == {1, 2}                       # both x-block counts
    assert all(6 in v and 6 // per_thread == 1 and 6 % per_thread == 2 for v in MODELS.values())           # a full and a ragged group
    assert max(MODELS['ragged300_o5']) > sg.SORT_ABOVE and ZERO_CASE[1] in MODELS[ZERO_CASE[0]]
    assert sg.model('ragged300_o5').m.observation_count == 5 and 5 % per_pass == 1
    assert sg.model('identity300').m.reachable_state_count == 1
    for S in (300, 2100, S_ROLLOUT):
        w = weights(S)
        assert np.any(w == 0) and np.any(w != np.floor(w)) and w.max() == 1.0e6 and np.all(w >= 0)
    assert (S_ROLLOUT + 255) // 256 == 3 and rg.N_ROWS > 1024 and rg.N_AGAIN > rg.SORT_ABOVE
    frames, table = rollout_case('frames')[1], rollout_case('table')[1]
    assert isinstance(frames, FrameEnvironment) and frames.shifts.max() > 0 and frames.end_observation >= 0
    assert table.end_observation == -1 and rollout_case('table')[0].m.observation_count == rg.DEAD + 1
    c = sg.model(ZERO_CASE[0])
    for objective in OBJECTIVES:                                # the zero weights give D == 0; the expected weight is then 0 too
        F, act, terms = space_aware_numpy(c.m, c.rows[:6], np.zeros(c.m.state_count), objective)
        assert np.all(terms[..., 2] == 0) and np.all(terms[..., 0] > 0) and (objective == 0 or (np.all(F == 0) and np.all(act == 0)))


@pytest.mark.parametrize('objective', OBJECTIVES)
@pytest.mark.parametrize('world', list(WORLDS))
def test_rollout_cases_hold_finished_lost_and_surviving_rows(world, objective):
    """``rollout_space_aware_numpy`` on the device case's inputs, whole and on the second call's 300 rows."""
    c, env = rollout_case(world)
    for n in (rg.N_ROWS, rg.N_AGAIN):
        out = rollout_space_aware_numpy(c.m, c.b0[:n], c.s0[:n], weights(S_ROLLOUT), rg.SEED, rg.FIRST_ID, rg.T_STEPS, objective,
                                        env=None if env is None else env.rows(0, n))
        states, actions, observations, steps = out[:4]
        lost = out[4] if env is not None else np.zeros(n, dtype=np.uint8)
        finished = np.isin(states[steps, np.arange(n)], c.m.end_states)
        assert not np.any(finished & (lost != 0))
        survivors = (steps == rg.T_STEPS) & ~finished & (lost == 0)
        assert finished.sum() >= 1 and survivors.sum() >= 1, (world, n)
        assert len(set(steps[finished].tolist())) > 1, (world, n)
        if env is not None:
            assert lost.sum() >= 1 and np.all(observations[steps[lost != 0] - 1, np.flatnonzero(lost)] == rg.DEAD), (world, n)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(MODELS))
def test_space_aware_numpy_returns_the_recorded_doubles(name, dtype):
    got = host_resident(name, dtype)
    assert all(len(v) == (6 if 'terms' in k else 3) for k, v in got.items())
    assert {k: [sha(x) for x in v] for k, v in got.items()} == golden(f'host_space_aware_{name}/{dtype}')


@pytest.mark.parametrize('objective', OBJECTIVES)
@pytest.mark.parametrize('world', list(WORLDS))
def test_rollout_space_aware_numpy_returns_the_recorded_doubles(world, objective):
    got = host_rollout(world, objective)
    assert len(got) == (4 if world == 'model' else 5)
    assert [sha(x) for x in got] == golden(f'host_rollout_{world}_obj{objective}')


# --------------------------------------------------------------------------------------------------------------------- #
# device
# --------------------------------------------------------------------------------------------------------------------- #
def run_resident(name, dtype):
    c = sg.model(name)
    eng = sg.make_engine(c.m, dtype)
    try:
        out = {}
        eng.set_state_weights(weights(c.m.state_count))
        for n in MODELS[name]:
            eng.set_beliefs(c.rows[:n])
            for objective in OBJECTIVES:
                arrays = eng.space_aware_resident(objective, want_terms=True)
                out[f'n{n}_obj{objective}'] = {k: sha(a) for k, a in zip(('F', 'action', 'terms'), arrays)}
        if name == ZERO_CASE[0]:
            eng.set_state_weights(np.zeros(c.m.state_count))
            eng.set_beliefs(c.rows[:6])
            for objective in OBJECTIVES:
                arrays = eng.space_aware_resident(objective, want_terms=True)
                assert np.all(arrays[2][..., 2] == 0)
                out[f'n6_obj{objective}_zero'] = {k: sha(a) for k, a in zip(('F', 'action', 'terms'), arrays)}
        return out
    finally:
        eng.close()


def run_rollout(world, dtype):
    c, env = rollout_case(world)
    eng = rg.make_engine(c, dtype)
    try:
        if isinstance(env, FrameEnvironment):
            eng.set_environment_frames(env.frames, env.channel_of_action)
        elif env is not None:
            eng.set_environment_table(env.obs_prob)
        eng.set_state_weights(weights(S_ROLLOUT))
        out = {}
        for objective in OBJECTIVES:
            for tag, n in (('first', rg.N_ROWS), ('again', rg.N_AGAIN)):
                eng.set_beliefs(c.b0[:n])
                shifts = env.shifts[:n] if isinstance(env, FrameEnvironment) else None
                arrays = eng.rollout_space_aware(c.s0[:n], rg.end_mask(c.m), rg.SEED, rg.T_STEPS, first_sim_id=rg.FIRST_ID,
                                                 objective=objective, use_env=env is not None, shifts=shifts,
                                                 end_observation=-1 if env is None else env.end_observation)
                d = {k: sha(a) for k, a in zip(ROLLOUT_NAMES, arrays)}
                d['B'] = int(eng.B)
                assert eng.B == int(eng._lib.pbvi_beliefs_count(eng._h))
                d['beliefs'] = sha(eng.fetch_beliefs()) if eng.B else None
                out[f'obj{objective}_{tag}'] = d
        return out
    finally:
        eng.close()


def run_interleaved(name, dtype, held=None):
    """The two policies in turn on one engine; ``held``: a dict that receives ``device_bytes`` of this engine and of a fresh
    one that makes the two space-aware calls alone."""
    c = sg.model(name)
    rows, w = c.rows[:ZERO_CASE[1]], weights(c.m.state_count)
    eng = sg.make_engine(c.m, dtype)
    try:
        eng.set_state_weights(w)
        eng.set_beliefs(rows)
        out = {}
        for i, objective in enumerate(OBJECTIVES):
            arrays = eng.infotaxis_resident(want_p_obs=True, want_entropy=True)
            out[f'infotaxis_{i}'] = {k: sha(a) for k, a in zip(('G', 'action', 'p_obs', 'H'), arrays)}
            arrays = eng.space_aware_resident(objective, want_terms=True)
            out[f'space_aware_obj{objective}'] = {k: sha(a) for k, a in zip(('F', 'action', 'terms'), arrays)}
        if held is not None:
            held['interleaved'] = int(eng.device_bytes)
    finally:
        eng.close()
    if held is not None:
        eng = sg.make_engine(c.m, dtype)
        try:
            eng.set_state_weights(w)
            eng.set_beliefs(rows)
            for objective in OBJECTIVES:
                eng.space_aware_resident(objective, want_terms=True)
            held['space_aware_alone'] = int(eng.device_bytes)
        finally:
            eng.close()
    return out


DEVICE_CASES = {}
for _d in DTYPES:
    for _n in MODELS:
        DEVICE_CASES[f'space_aware_{_n}/{_d}'] = (run_resident, _n, _d)
    for _w in WORLDS:
        DEVICE_CASES[f'rollout_space_aware_{_w}/{_d}'] = (run_rollout, _w, _d)
    DEVICE_CASES[f'interleaved_{ZERO_CASE[0]}/{_d}'] = (run_interleaved, ZERO_CASE[0], _d)


@pytest.mark.gpu
@pytest.mark.parametrize('key', list(DEVICE_CASES))
def test_greedy_policies_equal_the_recorded_bits(key):
    fn, name, kind = DEVICE_CASES[key]
    want = golden(key)
    if fn is run_interleaved:
        held = {}
        got = fn(name, kind, held)
        assert got['infotaxis_0'] == got['infotaxis_1'], key
        assert got['space_aware_obj0'] == golden(f'space_aware_{name}/{kind}')[f'n{ZERO_CASE[1]}_obj0'], key
        # one buffer family: what infotaxis adds to an engine that runs space-aware infotaxis is its [B] entropies alone
        assert held['interleaved'] == held['space_aware_alone'] + ZERO_CASE[1] * 8, (key, held)
    else:
        got = fn(name, kind)
    assert got == want, key


if __name__ == '__main__':
    assert len(sys.argv) == 3 and sys.argv[1] == '--record', 'usage: test_greedy_golden.py --record FILE'
    recorded = host_digests()
    recorded.update({key: fn(name, kind) for key, (fn, name, kind) in DEVICE_CASES.items()})
    with open(sys.argv[2], 'w') as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'recorded {len(recorded)} cases into {sys.argv[2]}')
