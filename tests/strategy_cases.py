"""Cases of ``test_strategy_solves.py``: seeded solves of every belief-expansion strategy of ``PBVI_Solver``.

No tests in here.  Every function takes the module that provides ``Model`` / ``PBVI_Solver`` / ... as ``pkg``: the fixture
generator (``golden/make_golden.py strategies``) passes the reference's ``src.pomdp``, the tests pass this package's
``pomdp`` module, so both sides make literally the same calls.

* models: two generated ones (sparse transitions, a strictly positive observation table -- the all-successor strategies
  ``ssea`` and ``ger`` divide by the probability of every observation, so they only run where none is impossible) and three
  example files;
* solver ``PBVI_Solver(gamma=0.9, eps=1e-6, expand_function=f)``, seeds 0 set after the model is built;
* configs ``(update_passes, prune_level, prune_interval)``;
* one direct ``expand_*`` call per strategy on ``gen70``, and ``ssga`` once more with an epsilon that makes it explore;
* the flat layout of ``golden/strategy_solves.npz`` (``pack`` / ``unpack``: one float array, one integer array, one pool of
  distinct rows per row width and a JSON index, because a zip member per array would cost more bytes than the arrays
  hold and the configs of one strategy share most of their alpha rows).
"""
import contextlib
import io
import json
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS_DIR = os.path.join(HERE, 'golden', 'models')
FIXTURE = 'strategy_solves.npz'

STRATEGIES = ('ra', 'ssra', 'ssga', 'ssea', 'ger', 'hsvi', 'fsvi', 'fsvi_eg', 'perseus')
FULL_BACKUP = ('ra', 'ssra', 'ssga', 'ssea', 'ger')          # the strategies solve() backs the whole belief set up for
CONFIGS = ((1, 1, 10), (2, 1, 10), (2, 2, 2))                # (update_passes, prune_level, prune_interval)
GAMMA, EPS = 0.9, 1e-6

GENERATED = {'gen70': (70, 3, 3, 3), 'gen600': (600, 4, 3, 2)}          # S, A, O, R
FILE_MODELS = {'tiger': 'tiger.95.POMDP', 'grid4x3': '4x3.95.POMDP', 'hallway': 'hallway.POMDP'}
MODEL_NAMES = tuple(GENERATED) + tuple(FILE_MODELS)
SIZES = {**{k: (6, 8) for k in GENERATED}, **{k: (5, 6) for k in FILE_MODELS}}     # expansions, max_belief_growth
# an observation of probability 0 at some successor: b.update divides by zero, in the reference and here alike
RAISING = tuple((m, s) for m in ('grid4x3', 'hallway') for s in ('ssea', 'ger'))
RAISING_PREFIX = 'States probabilities in belief must sum to 1 (found: nan'
# GPU-against-host cases that run on another seed of the random streams than 0.  hallway starts from the uniform belief
# over a maze with symmetries: at some beliefs two actions with different alpha rows have the same value up to the last
# bit (host: the einsum of the backup differs by one ulp, an exactly rounded sum by none), the host's pick is its
# summation order's and the fp64 engine's is its own, and from there the two solves hold different rows.  With seed 0
# that happens in these four solves (second update pass of the first expansion for perseus, backup 7 for ssga); each
# runs on the smallest seed at which the HOST solve meets no such tie (test_strategy_solves.action_value_ties).
GPU_STREAM_SEEDS = {('hallway', 'ssga', (2, 1, 10)): 9, ('hallway', 'ssga', (2, 2, 2)): 9,
                    ('hallway', 'perseus', (2, 1, 10)): 1, ('hallway', 'perseus', (2, 2, 2)): 1}
# ssga takes a random action with probability epsilon (default 0.1).  With seeds 0 no draw of the cases above falls under
# 0.1, so that branch never runs in them: one more solve and one more direct call on gen70 pass epsilon = 0.5.
SSGA_EPSILON = 0.5
SSGA_EPSILON_CASE = ('gen70', 'ssga', (1, 1, 10))
PROBE_SEED, PROBES = 9, 8                                   # gen600: rows are stored as 8 projections and their sum


def config_tag(config) -> str:
    return 'u{}l{}i{}'.format(*config)


def case_key(model_name, strategy, config) -> str:
    return f'{model_name}/{strategy}/{config_tag(config)}'


def solve_cases(models=MODEL_NAMES):
    """Every (model, strategy, config) the reference completes."""
    return [(m, s, c) for m in models for s in STRATEGIES for c in CONFIGS if (m, s) not in RAISING]


def positive_obs_tables(S, A, O, R, seed=5):
    rng = np.random.default_rng(seed)
    rs = np.stack([np.stack([rng.choice(S, size=R, replace=False) for _ in range(A)]) for _ in range(S)])
    ob = 0.02 + rng.random((S, A, O)) ** 3
    ob /= ob.sum(axis=2, keepdims=True)
    return rs, ob


def quiet(fn, *a, **k):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*a, **k)


def build_model(pkg, name, seed=5):
    if name in GENERATED:
        S, A, O, R = GENERATED[name]
        rs, ob = positive_obs_tables(S, A, O, R, seed)
        return quiet(pkg.Model, states=S, actions=A, observations=O, reachable_states=rs, observation_table=ob,
                     end_states=[S - 1])
    return quiet(pkg.load_POMDP_file, os.path.join(MODELS_DIR, FILE_MODELS[name]))[0]


def run_solve(pkg, model, model_name, strategy, config, seed=0, expand_params=None, **solve_kw):
    """The one call every case makes.  Returns ``(value_function, history)``."""
    u, l, i = config
    expansions, growth = SIZES[model_name]
    np.random.seed(seed)
    random.seed(seed)
    solver = pkg.PBVI_Solver(gamma=GAMMA, eps=EPS, expand_function=strategy, **(expand_params or {}))
    return quiet(solver.solve, model, expansions=expansions, max_belief_growth=growth, update_passes=u, prune_level=l,
                 prune_interval=i, print_progress=False, **solve_kw)


def probe_vectors(S):
    return np.random.default_rng(PROBE_SEED).random((PROBES, S))


def row_summary(model_name, rows):
    """What the fixture keeps of the final alpha rows: the rows, or for gen600 ``[V, PROBES + 1]`` projections and sums."""
    rows = np.asarray(rows, dtype=np.float64)
    if model_name != 'gen600':
        return rows
    return np.concatenate([rows @ probe_vectors(rows.shape[1]).T, rows.sum(axis=1, keepdims=True)], axis=1)


def record(model_name, vf, hist) -> dict:
    return {'beliefs_counts': np.asarray(hist.beliefs_counts, dtype=np.int64),
            'alpha_vector_counts': np.asarray(hist.alpha_vector_counts, dtype=np.int64),
            'prune_counts': np.asarray(hist.prune_counts, dtype=np.int64),
            'value_function_changes': np.asarray(hist.value_function_changes, dtype=np.float64),
            'actions': np.asarray(vf.actions, dtype=np.int64),
            'rows': row_summary(model_name, vf.alpha_vector_array)}


# --------------------------------------------------------------------------- #
# one direct expand_* call per strategy
# --------------------------------------------------------------------------- #
def single_expansion(pkg, model, strategy, max_generation=6, **expand_kw):
    """``expand_<strategy>`` on the initial belief and its A x O successors with the initial value function (``ER.T``);
    the strategies that walk from one belief start from the initial one, as ``expand()`` makes them.  Returns the belief
    array of the result."""
    b0 = pkg.Belief(model)
    belief_set = pkg.BeliefSet(model, [b0] + b0.generate_successors())
    vf = pkg.ValueFunction(model, model.expected_rewards_table.T, model.actions)
    solver = pkg.PBVI_Solver(gamma=GAMMA, eps=EPS, expand_function=strategy)
    mdp_policy = None
    if strategy in ('hsvi', 'fsvi', 'fsvi_eg'):
        mdp_policy = quiet(pkg.VI_Solver(gamma=GAMMA, eps=EPS).solve, model, print_progress=False)[0]
    np.random.seed(0)
    random.seed(0)
    fn = getattr(solver, 'expand_' + strategy)
    if strategy in ('ra', 'ssra', 'ssea'):
        out = fn(model, belief_set, max_generation=max_generation)
    elif strategy in ('ssga', 'ger'):
        out = fn(model, belief_set, value_function=vf, max_generation=max_generation, **expand_kw)
    elif strategy == 'hsvi':
        out = fn(model, b0, vf, pkg.BeliefValueMapping(model, mdp_policy), max_generation=max_generation)
    elif strategy in ('fsvi', 'fsvi_eg'):
        out = fn(model, b0, mdp_policy, max_generation=max_generation)
    else:
        out = fn(model, b0, max_generation=max_generation)
    return np.asarray(out.belief_array, dtype=np.float64)


# --------------------------------------------------------------------------- #
# fixture layout
# --------------------------------------------------------------------------- #
def pack(entries: dict) -> dict:
    """``{key: array}`` -> ``{'index': json, 'floats': f64 [n], 'ints': i32 [m], 'pool_<S>': f64 [k, S], ...}``.  A 2-D float
    array is kept as row numbers into the pool of its width: the configs of one (model, strategy) share most of their
    alpha rows bit for bit, and each distinct row is stored once."""
    index, floats, ints, pools, seen = {}, [np.zeros(0)], [np.zeros(0, dtype=np.int32)], {}, {}
    n_f = n_i = 0
    for key, a in entries.items():
        a = np.asarray(a)
        if a.dtype.kind == 'f' and a.ndim == 2:
            a = np.ascontiguousarray(a, dtype=np.float64)
            pool = pools.setdefault(a.shape[1], [])
            ids = []
            for row in a:
                k = (a.shape[1], row.tobytes())
                if k not in seen:
                    seen[k] = len(pool)
                    pool.append(row)
                ids.append(seen[k])
            index[key] = ['r', n_i, list(a.shape)]
            ints.append(np.asarray(ids, dtype=np.int32))
            n_i += len(ids)
        elif a.dtype.kind == 'f':
            index[key] = ['f', n_f, list(a.shape)]
            floats.append(a.astype(np.float64).ravel())
            n_f += a.size
        else:
            assert a.size == 0 or np.abs(a).max() < 2 ** 31
            index[key] = ['i', n_i, list(a.shape)]
            ints.append(a.astype(np.int32).ravel())
            n_i += a.size
    out = {'index': np.array(json.dumps(index)), 'floats': np.concatenate(floats), 'ints': np.concatenate(ints)}
    out.update({f'pool_{w}': np.array(rows) for w, rows in pools.items()})
    return out


def unpack(z) -> dict:
    index = json.loads(str(z['index']))
    floats, ints = np.asarray(z['floats']), np.asarray(z['ints']).astype(np.int64)
    out = {}
    for key, (kind, start, shape) in index.items():
        if kind == 'r':
            out[key] = np.asarray(z[f'pool_{shape[1]}'])[ints[start:start + shape[0]]].reshape(shape)
        else:
            flat = floats if kind == 'f' else ints
            out[key] = flat[start:start + int(np.prod(shape, dtype=np.int64))].reshape(shape)
    return out
