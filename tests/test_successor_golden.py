"""The bits of every call that sums the un-normalised Bayes successor over the inverse transition lists and is not pinned by
``test_rollout_golden.py`` already: sha256 of the returned arrays against tests/golden/successor_digests.json.

The file was recorded on an MI355X (twice, with the same digests) from the commit before the successor sum of the device
code became one pair of functions in ``csrc/successor.h`` and the HSVI successors moved onto the Bayes-step launchers
(05e3c78).  That refactor had to reproduce it without re-recording.  A later change that alters these bits on purpose must
re-record the file (``python tests/test_successor_golden.py --record FILE`` on the device) and say why.

Every case is the smallest at which its path can still go wrong (``model_cases`` models, A = 2):
  * successor Q (``upper_q_resident``): the ragged model (O = 3, R = 4) at S = 300 and 700 -- two and three push blocks per
    successor row, the last ragged -- with blocks of 1, 7 and 300 rows (300 rows are sorted inside an engine of either type,
    so ``perm`` is read) over 0 and 65 random points (65: a second sawtooth chunk).  In the ragged model every observation
    is possible after every step, so here observation 2 is made impossible from the first ``BLOCKED`` states (its
    probability moves to observation 0) and row 0 of every block lives on those states: ``p_obs == 0`` exactly, the
    successor's value NaN.  The same call on 40 rows at S = 700 under an allocation cap that leaves room for fewer than 40
    beliefs' successors: the chunks must give the bits of the whole.
  * infotaxis (``infotaxis_resident``): the ragged model with O = 5 at S = 300 (two observation passes, the second of one),
    the identity model (R = 1: the ``R == 1`` branch of the index split), the ragged model at S = 2100 (two x-blocks of
    2048 landing states); blocks of 6 rows (one full group of four beliefs and a ragged group of two), and 300 rows at
    S = 300.
  * belief-side backup (``set_formulation('belief')``): the O = 5 ragged model and the identity model at S = 300, 6 and 300
    beliefs, 40 alpha rows.  An f64 engine projects the beliefs only when B * A * O * V >= 64 * 64 (below that its score
    GEMM is not the MFMA one), so its 6-belief block with 40 alpha rows takes the alpha side; a third block, 6 beliefs
    against 200 alpha rows, brings the ragged group of two to ``k_push_project<double>`` as well.  The projected rows are
    free of atomics; the magnitude row is summed with atomics, but it only scales tie windows that the refinement settles
    exactly.  (Both parent recordings agreed on every one of these cases, so none had to be dropped.)
  * belief walk (``belief_walk``, 41 steps, restarts at steps 0, 13 and 14) on the ragged model at S = 700: the fp64 rows
    and ``belief_walk_keys`` of an f64 engine and of f32 engines with and without the fp64 table -- both table types, and
    both sources of the base row (the start belief, the previous raw row over its mass).
The host tests below hold the cases to that description, and pin ``upper_q_numpy`` / ``infotaxis_numpy`` on the same inputs
to the doubles they returned before they shared ``_successor_rows`` (recorded from the same parent commit)."""
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest

if __name__ == '__main__':
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import conftest                                                         # noqa: F401  (puts the repository on sys.path)

import hsvi_cases as hc
import model_cases as mc
from pomdp_pbvi_exploration_amd.pomdp import infotaxis_numpy, upper_q_numpy

GOLDEN_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'successor_digests.json')
DTYPES = ('f32', 'f64')
CASTS = {'f32': np.float32, 'f64': np.float64}
GAMMA = 0.95
SORT_ABOVE = 256                       # beliefs_finish sorts a block of more rows than this in an f32 engine (f64: 128)
BLOCKED = 20                           # HSVI cases: observation 2 is impossible from the states below this
UQ_BLOCKS, UQ_POINTS, UQ_CHUNK_ROWS = (1, 7, 300), (0, 65), 40
INFOTAXIS = {'ragged300_o5': (6, 300), 'identity300': (6,), 'ragged2100': (6,)}      # model -> block sizes
BACKUP = {'ragged300_o5': ((6, 40), (300, 40), (6, 200)), 'identity300': ((6, 40), (300, 40), (6, 200))}     # (beliefs, alpha rows)
N_ALPHA = 200
WALK_STEPS, WALK_RESTARTS = 41, (0, 13, 14)
WALK_KINDS = ('f64', 'f32_rto64', 'f32_plain')
_CACHE = {}


def sha(x):
    x = np.ascontiguousarray(x)
    return hashlib.sha256(f'{x.dtype.str} {x.shape} '.encode() + x.tobytes()).hexdigest()


# --------------------------------------------------------------------------------------------------------------------- #
# cases (seeded, built once)
# --------------------------------------------------------------------------------------------------------------------- #
BUILDERS = {
    'ragged300': lambda: mc.ragged_model(300, A=2, O=3),
    'ragged700': lambda: mc.ragged_model(700, A=2, O=3),
    'ragged300_o5': lambda: mc.ragged_model(300, A=2, O=5),
    'identity300': lambda: mc.identity_model(300),
    'ragged2100': lambda: mc.ragged_model(2100, A=2, O=3),
}


def model(name, blocked=False):
    """The model under ``Model``'s attribute names with rewards, 300 belief rows (representable in fp32, so that both engine
    types hold the same numbers) and an alpha set; ``blocked``: the HSVI variant, whose row 0 lives on the blocked states."""
    key = (name, blocked)
    if key not in _CACHE:
        rs, rto = BUILDERS[name]()
        S, A, O, R = rto.shape
        rng = np.random.default_rng(9100 + S + O)
        rows = mc.sparse_beliefs(rng, 300, S)
        if blocked:
            rto = rto.copy()
            rto[:BLOCKED, :, 0, :] += rto[:BLOCKED, :, 2, :]
            rto[:BLOCKED, :, 2, :] = 0.0
            rows[0] = 0.0
            rows[0, :BLOCKED] = rng.random(BLOCKED) + 0.1
            rows[0] /= rows[0].sum()
        m = SimpleNamespace(state_count=S, action_count=A, observation_count=O, reachable_state_count=R,
                            reachable_states=rs.astype(np.int64), reachable_transitional_observation_table=rto,
                            expected_rewards_table=rng.normal(size=(S, A)), end_states=[])
        _CACHE[key] = SimpleNamespace(m=m, rows=hc.r32(rows), alpha=rng.normal(size=(N_ALPHA, S)))
    return _CACHE[key]


def point_store(S, P):
    """``(corner, points, values, gaps)`` of a case with P points."""
    rng = np.random.default_rng(9200 + S + P)
    c = hc.corner_values(rng, S)
    return (c,) + hc.make_points(rng, S, P, c)


def walk_inputs(S):
    rng = np.random.default_rng(9300 + S)
    restart = np.zeros(WALK_STEPS, dtype=np.uint8)
    restart[list(WALK_RESTARTS)] = 1
    return rng.integers(0, 2, WALK_STEPS), rng.integers(0, 3, WALK_STEPS), restart


def host_upper_q(name, dtype):
    c = model(name, blocked=True)
    out = {}
    for P in UQ_POINTS:
        corner, pts, values, gaps = point_store(c.m.state_count, P)
        for n in UQ_BLOCKS:
            out[f'P{P}_n{n}'] = upper_q_numpy(c.m, pts, values, gaps, corner, c.rows[:n], GAMMA, table_dtype=CASTS[dtype])
    return out


def host_infotaxis(name, dtype):
    c = model(name)
    return {f'n{n}': infotaxis_numpy(c.m, c.rows[:n], CASTS[dtype]) for n in INFOTAXIS[name]}


def host_digests():
    out = {}
    for dtype in DTYPES:
        for name in ('ragged300', 'ragged700'):
            out[f'host_upper_q_{name}/{dtype}'] = {k: [sha(x) for x in v] for k, v in host_upper_q(name, dtype).items()}
        for name in INFOTAXIS:
            out[f'host_infotaxis_{name}/{dtype}'] = {k: [sha(x) for x in v] for k, v in host_infotaxis(name, dtype).items()}
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
    for name, S in (('ragged300', 300), ('ragged700', 700)):
        m = model(name, blocked=True).m
        assert m.reachable_transitional_observation_table.shape == (S, 2, 3, 4)
        t, t0 = m.reachable_transitional_observation_table, model(name).m.reachable_transitional_observation_table
        assert np.all(t[:BLOCKED, :, 2, :] == 0) and np.allclose(t.sum(axis=2), t0.sum(axis=2), rtol=1e-14, atol=0)
    assert (300 + 255) // 256 == 2 and (700 + 255) // 256 == 3 and 300 % 256 != 0 and 700 % 256 != 0       # push blocks
    assert max(UQ_BLOCKS) > SORT_ABOVE and max(INFOTAXIS['ragged300_o5']) > SORT_ABOVE                      # sorted blocks
    assert max(UQ_POINTS) > 64 and min(UQ_POINTS) == 0                                                      # sawtooth chunks of 64
    per_pass, per_thread, x_block = 4, 4, 8 * 256              # observations per pass, beliefs per thread, states per x-block
    assert model('ragged300_o5').m.observation_count == 5 and 5 > per_pass and 5 % per_pass == 1           # two passes, 4 + 1
    assert model('identity300').m.reachable_state_count == 1 and model('ragged300_o5').m.reachable_state_count == 4
    assert all(6 in v and 6 > per_thread and 6 % per_thread == 2 for v in INFOTAXIS.values())             # a ragged group of two
    assert -(-2100 // x_block) == 2 and -(-300 // x_block) == 1                                             # two x-blocks
    for name, blocks in BACKUP.items():                        # a ragged group of two beliefs reaches k_push_project of either type
        assert all(any(n == 6 and projects_beliefs(model(name).m, d, n, V) for n, V in blocks) for d in DTYPES)
        assert all(any(n > SORT_ABOVE and projects_beliefs(model(name).m, d, n, V) for n, V in blocks) for d in DTYPES)
    restart = walk_inputs(700)[2]
    assert restart[0] == 1 and restart[13] == 1 and restart[14] == 1 and restart.sum() == 3 and restart[12] == 0


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', ['ragged300', 'ragged700'])
def test_upper_q_numpy_returns_the_recorded_doubles(name, dtype):
    got = host_upper_q(name, dtype)
    for k, (Q, act, Z, sval, shit) in got.items():
        assert np.any(Z[0] == 0) and np.all(Z[0, :, :2] > 0), (name, k)          # row 0 cannot see observation 2 ...
        assert np.array_equal(np.isnan(sval), Z == 0) and np.all(Z[1:] > 0), (name, k)      # ... and every other row can
    assert {k: [sha(x) for x in v] for k, v in got.items()} == golden(f'host_upper_q_{name}/{dtype}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name', list(INFOTAXIS))
def test_infotaxis_numpy_returns_the_recorded_doubles(name, dtype):
    got = host_infotaxis(name, dtype)
    for k, (G, act, Z, H) in got.items():
        assert np.all(np.isfinite(G)) and np.all(H > 0), (name, k)
    assert {k: [sha(x) for x in v] for k, v in got.items()} == golden(f'host_infotaxis_{name}/{dtype}')


# --------------------------------------------------------------------------------------------------------------------- #
# device
# --------------------------------------------------------------------------------------------------------------------- #
def make_engine(m, dtype, plain_f32_table=False):
    from pomdp_pbvi_exploration_amd.engine import Engine
    rto = m.reachable_transitional_observation_table
    if plain_f32_table:                                        # an f32 engine given an fp32 table keeps no fp64 copy of it
        rto = rto.astype(np.float32)
    return Engine(m.state_count, m.action_count, m.observation_count, m.reachable_state_count, m.reachable_states, rto,
                  m.expected_rewards_table, dtype=dtype)


UQ_NAMES = ('Q', 'action', 'p_obs', 'succ_value')


def run_upper_q(name, dtype):
    c = model(name, blocked=True)
    eng = make_engine(c.m, dtype)
    try:
        out = {}
        for P in UQ_POINTS:
            corner, pts, values, gaps = point_store(c.m.state_count, P)
            eng.upper_reset(corner)
            if P:
                eng.upper_append(pts, values, gaps)
            for n in UQ_BLOCKS:
                eng.set_beliefs(c.rows[:n])
                arrays = eng.upper_q_resident(GAMMA, want_p_obs=True, want_succ_value=True)
                assert np.any(arrays[2][0] == 0) and np.array_equal(np.isnan(arrays[3]), arrays[2] == 0)
                out[f'P{P}_n{n}'] = {k: sha(a) for k, a in zip(UQ_NAMES, arrays)}
        return out
    finally:
        eng.close()


def run_upper_q_chunked(name, dtype):
    """40 rows under a cap that leaves half of its room too small for 40 beliefs' successors, then without the cap."""
    from pomdp_pbvi_exploration_amd import engine as engine_mod
    c = model(name, blocked=True)
    S, A, O = c.m.state_count, c.m.action_count, c.m.observation_count
    corner, pts, values, gaps = point_store(S, 65)
    per_belief = A * O * S * (8 + np.dtype(CASTS[dtype]).itemsize)      # un-normalised fp64 and normalised successors
    out = {}
    prev = engine_mod.debug_alloc_limit(-1)
    try:
        for tag in ('chunked', 'whole'):
            eng = make_engine(c.m, dtype)
            try:
                eng.upper_reset(corner)
                eng.upper_append(pts, values, gaps)
                eng.set_beliefs(c.rows[:UQ_CHUNK_ROWS])
                if tag == 'chunked':
                    cap = -(-eng.device_bytes // (1 << 20)) + 2
                    assert ((cap << 20) - eng.device_bytes) // 2 < UQ_CHUNK_ROWS * per_belief
                    engine_mod.debug_alloc_limit(cap)
                arrays = eng.upper_q_resident(GAMMA, want_p_obs=True, want_succ_value=True)
                out[tag] = {k: sha(a) for k, a in zip(UQ_NAMES, arrays)}
            finally:
                engine_mod.debug_alloc_limit(-1)
                eng.close()
    finally:
        engine_mod.debug_alloc_limit(prev)
    return out


def run_infotaxis(name, dtype):
    c = model(name)
    eng = make_engine(c.m, dtype)
    try:
        out = {}
        for n in INFOTAXIS[name]:
            eng.set_beliefs(c.rows[:n])
            arrays = eng.infotaxis_resident(want_p_obs=True, want_entropy=True)
            out[f'n{n}'] = {k: sha(a) for k, a in zip(('G', 'action', 'p_obs', 'H'), arrays)}
        return out
    finally:
        eng.close()


def projects_beliefs(m, dtype, n, V):
    """Whether an engine told to project the beliefs can (``EngineT::choose_push``: fp32, or an fp64 score GEMM on MFMAs)."""
    return dtype == 'f32' or n * m.action_count * m.observation_count * V >= 64 * 64


def run_backup(name, dtype):
    c = model(name)
    eng = make_engine(c.m, dtype)
    try:
        eng.set_formulation('belief')
        out = {}
        for n, V in BACKUP[name]:
            eng.set_alpha(c.alpha[:V])
            eng.set_beliefs(c.rows[:n])
            st = eng.run(GAMMA)
            assert st['formulation'] == 2 or not projects_beliefs(c.m, dtype, n, V), (name, dtype, n, V)
            res = eng.fetch()
            out[f'n{n}_V{V}'] = {'rows': sha(res.alpha), 'index': sha(res.best_alpha_ind), 'actions': sha(res.actions)}
        return out
    finally:
        eng.close()


def run_walk(name, kind):
    c = model(name)
    acts, obs, restart = walk_inputs(c.m.state_count)
    eng = make_engine(c.m, kind[:3], plain_f32_table=kind == 'f32_plain')
    try:
        rows, _ = eng.belief_walk(c.rows[1], acts, obs, restart)
        assert rows.dtype == np.float64 and rows.shape == (WALK_STEPS, c.m.state_count) and np.all(np.isfinite(rows))
        return {'rows': sha(rows), 'keys': sha(eng.belief_walk_keys(WALK_STEPS))}
    finally:
        eng.close()


DEVICE_CASES = {}
for _d in DTYPES:
    for _n in ('ragged300', 'ragged700'):
        DEVICE_CASES[f'upper_q_{_n}/{_d}'] = (run_upper_q, _n, _d)
    DEVICE_CASES[f'upper_q_chunked_ragged700/{_d}'] = (run_upper_q_chunked, 'ragged700', _d)
    for _n in INFOTAXIS:
        DEVICE_CASES[f'infotaxis_{_n}/{_d}'] = (run_infotaxis, _n, _d)
    for _n in BACKUP:
        DEVICE_CASES[f'belief_backup_{_n}/{_d}'] = (run_backup, _n, _d)
for _k in WALK_KINDS:
    DEVICE_CASES[f'walk_ragged700/{_k}'] = (run_walk, 'ragged700', _k)


@pytest.mark.gpu
@pytest.mark.parametrize('key', list(DEVICE_CASES))
def test_successor_calls_equal_the_recorded_bits(key):
    fn, name, kind = DEVICE_CASES[key]
    want = golden(key)
    got = fn(name, kind)
    if fn is run_upper_q_chunked:
        assert got['chunked'] == got['whole'], key
    assert got == want, key


if __name__ == '__main__':
    assert len(sys.argv) == 3 and sys.argv[1] == '--record', 'usage: test_successor_golden.py --record FILE'
    recorded = host_digests()
    recorded.update({key: fn(name, kind) for key, (fn, name, kind) in DEVICE_CASES.items()})
    with open(sys.argv[2], 'w') as f:
        json.dump(recorded, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'recorded {len(recorded)} cases into {sys.argv[2]}')
