"""Host-side mirror of the reference's ``src/pomdp.py`` around the backup path.

Same class names, signatures and container semantics as the reference so its
notebooks' ``from src.pomdp import *`` keeps working (``src/`` at the repo root
re-exports this module).  What differs is the seam the reference implements with
CuPy array-module dispatch (``src/pomdp.py:1482``, ``:2243-2264``): here
``use_gpu=True`` / ``.gpu_model`` / ``.to_gpu()`` bind the objects to a HIP
engine (``engine.Engine``) and ``PBVI_Solver.backup`` then runs on hand-written
gfx950 kernels through the C-ABI of ``include/pbvi_hip.h``.  With
``use_gpu=False`` the NumPy statements of the reference run on the host
(BASELINE config 0).  A GPU request never degrades to the CPU path: if the HIP
library is missing the call raises.
"""
from __future__ import annotations

import copy            # noqa: F401  (notebooks rely on these leaked names)
import random
from datetime import datetime
from typing import Tuple, Union

import numpy as np

from .mdp import AlphaVector, ValueFunction, VI_Solver, log, _log, set_quiet   # noqa: F401
from .mdp import Model as MDP_Model
from .mdp import Solver as MDP_Solver
from .mdp import RewardSet, _RowKey, _draw_index, _run_sweeps            # noqa: F401
from .mdp import SimulationHistory as MDP_SimulationHistory
from .mdp import Simulation as MDP_Simulation
from . import dist as _dist

gpu_support = True


class Model(MDP_Model):
    """POMDP model: MDP tables + observation table, fused ``RTO[s,a,o,r]`` and
    ``expected_rewards_table[s,a]`` (``src/pomdp.py:147-254``)."""

    def __init__(self, states, actions, observations, transitions=None, reachable_states=None, rewards=None,
                 observation_table=None, rewards_are_probabilistic: bool = False, state_grid=None,
                 start_probabilities=None, end_states: list = [], end_actions: list = []):
        super().__init__(states=states, actions=actions, transitions=transitions, reachable_states=reachable_states,
                         rewards=-1, rewards_are_probabilistic=rewards_are_probabilistic, state_grid=state_grid,
                         start_probabilities=start_probabilities, end_states=end_states, end_actions=end_actions)
        S, A = self.state_count, self.action_count
        self.observation_labels = [f'o_{i}' for i in range(observations)] if isinstance(observations, int) else observations
        self.observation_count = len(self.observation_labels)
        self.observations = np.arange(self.observation_count)
        O = self.observation_count

        if observation_table is None:
            rnd = np.random.rand(S, A, O)
            self.observation_table = rnd / np.sum(rnd, axis=2, keepdims=True)
        else:
            self.observation_table = np.array(observation_table)
            assert self.observation_table.shape == (S, A, O), \
                f"Observations table doesnt have the right shape, it should be SxAxO (expected: {(S, A, O)}, received: {self.observation_table.shape})."
        _log(f'POMDP model: {O} observations')

        rs = self.reachable_states
        reach_obs = self.observation_table[rs[:, :, None, :], self.actions[None, :, None, None], self.observations[None, None, :, None]]
        self.reachable_transitional_observation_table = np.einsum('sar,saor->saor', self.reachable_probabilities, reach_obs)

        self.immediate_reward_table = None
        self.immediate_reward_function = None
        if rewards is None:
            if len(self.end_states) > 0 or len(self.end_actions) > 0:
                self.immediate_reward_function = self._end_reward_function
            else:
                self.immediate_reward_table = np.random.rand(S, A, S, O)
        elif callable(rewards):
            self.immediate_reward_function = rewards
        else:
            self.immediate_reward_table = np.array(rewards)
            assert self.immediate_reward_table.shape == (S, A, S, O), \
                f"Rewards table doesnt have the right shape, it should be SxAxSxO (expected: {(S, A, S, O)}, received {self.immediate_reward_table.shape})"

        if self.immediate_reward_table is not None:
            reach_r = self.immediate_reward_table[self.states[:, None, None, None], self.actions[None, :, None, None],
                                                  rs[:, :, :, None], self.observations[None, None, None, :]]
        else:
            reach_r = np.fromfunction(lambda s, a, r, o: self.immediate_reward_function(
                s.astype(int), a.astype(int), rs[s.astype(int), a.astype(int), r.astype(int)], o.astype(int)), (*rs.shape, O))
        self._min_reward = float(np.min(reach_r))
        self._max_reward = float(np.max(reach_r))
        self.expected_rewards_table = np.einsum('saor,saro->sa', self.reachable_transitional_observation_table, reach_r)

    def _end_reward_function(self, s, a, sn, o):
        return (np.isin(sn, self.end_states) | np.isin(a, self.end_actions)).astype(int)

    def reward(self, s: int, a: int, s_p: int, o: int):
        """Reward of ``(s, a, s_p, o)``; a Bernoulli draw when rewards are probabilities (``src/pomdp.py:259-285``)."""
        if self.immediate_reward_table is not None:
            r = float(self.immediate_reward_table[s, a, s_p, o])
        else:
            r = float(self.immediate_reward_function(s, a, s_p, o))
        if self.rewards_are_probabilistic:
            return 1 if random.random() < r else 0
        return r

    def observe(self, s_p: int, a: int) -> int:
        return int(self.observations[_draw_index(self.observation_table[s_p, a])])


class Belief:
    """Probability distribution over states; Bayes update through the
    reachable-state tables (``src/pomdp.py:311-421``)."""

    def __new__(cls, *args, **kwargs):
        inst = super().__new__(cls)
        inst._bytes_repr = None
        inst._key = None
        inst._successors = {}
        return inst

    def __init__(self, model: Model, values: Union[np.ndarray, None] = None):
        assert model is not None
        self.model = model
        if values is not None:
            assert values.shape[0] == model.state_count, "Belief must contain be of dimension |S|"
            total = np.sum(values)
            assert np.round(total, decimals=3) == 1.0, f"States probabilities in belief must sum to 1 (found: {total})"
            self._values = values
        else:
            self._values = model.start_probabilities

    @property
    def values(self) -> np.ndarray:
        return self._values

    @property
    def bytes_repr(self) -> bytes:
        if self._bytes_repr is None:
            self._bytes_repr = self.values.tobytes()
        return self._bytes_repr

    @property
    def key(self) -> _RowKey:
        if self._key is None:
            self._key = _RowKey(self.values)
        return self._key

    def __eq__(self, other) -> bool:
        return self.bytes_repr == other.bytes_repr

    def update(self, a: int, o: int) -> 'Belief':
        key = f'{a}_{o}'
        hit = self._successors.get(key)
        if hit is not None:
            return hit
        m = self.model
        weights = m.reachable_transitional_observation_table[:, a, o, :] * self.values[:, None]
        nxt = np.bincount(m.reachable_states[:, a, :].flatten(), weights=weights.flatten(), minlength=m.state_count)
        nxt /= np.sum(nxt)
        out = self.__new__(self.__class__)
        out.model = m
        out._values = nxt
        self._successors[key] = out
        return out

    def generate_successors(self) -> list:
        return [self.update(a, o) for a in self.model.actions for o in self.model.observations]

    def random_state(self) -> int:
        return int(self.model.states[_draw_index(self._values)])


class BeliefSet:
    """A set of beliefs as a list and as a B x S matrix (``src/pomdp.py:489-659``)."""

    def __init__(self, model: Model, beliefs: Union[list, np.ndarray]) -> None:
        self.model = model
        self._belief_array = None
        self._uniqueness_dict = None
        self._key_dict = None
        self.is_on_gpu = bool(getattr(model, 'is_on_gpu', False))
        if isinstance(beliefs, list):
            assert all(len(b.values) == model.state_count for b in beliefs), \
                f"Beliefs in belief list provided dont all have shape ({model.state_count},)"
            self._belief_list = beliefs
        else:
            assert beliefs.shape[1] == model.state_count, \
                f"Belief array provided doesnt have the right shape (expected (-,{model.state_count}), received {beliefs.shape})"
            self._belief_list = [Belief(model, row) for row in beliefs]

    @property
    def belief_array(self) -> np.ndarray:
        if self._belief_array is None:
            self._belief_array = np.array([b.values for b in self._belief_list])
        return self._belief_array

    @property
    def belief_list(self) -> list:
        if self._belief_list is None:
            self._belief_list = [Belief(self.model, row) for row in self._belief_array]
        return self._belief_list

    def generate_all_successors(self) -> 'BeliefSet':
        succ = []
        for b in self.belief_list:
            succ.extend(b.generate_successors())
        return BeliefSet(self.model, succ)

    @property
    def unique_belief_dict(self) -> dict:
        """Beliefs keyed by their bytes, as the reference exposes them (built on demand)."""
        if self._uniqueness_dict is None:
            self._uniqueness_dict = {b.bytes_repr: b for b in self.belief_list}
        return self._uniqueness_dict

    @property
    def _unique_by_key(self) -> dict:
        if self._key_dict is None:
            self._key_dict = {b.key: b for b in self.belief_list}
        return self._key_dict

    def union(self, other: 'BeliefSet') -> 'BeliefSet':
        """``self.unique_belief_dict | other.unique_belief_dict`` (``src/pomdp.py:585-606``): this set's order, then
        the other's beliefs that are new by bytes; on equal bytes the other's object takes the slot.  Both inputs
        were validated when they were built, so the result is assembled directly; when every belief already lives
        in an engine's belief store (``_dev``), the id array of the result is carried over instead of re-walking
        the objects on the next device call."""
        mine = self._unique_by_key                           # same dedup as the bytes-keyed dictionaries, cheaper keys
        theirs = other._unique_by_key
        added = [b for k, b in theirs.items() if k not in mine]
        merged = dict(mine)
        merged.update(theirs)
        out = BeliefSet.__new__(BeliefSet)
        out.model = self.model
        out._belief_array = None
        out._uniqueness_dict = None
        out._key_dict = merged
        out.is_on_gpu = self.is_on_gpu
        out._belief_list = list(merged.values())
        ids = getattr(self, '_dev_ids', None)
        if ids is not None and len(ids[1]) == len(mine) and len(self._belief_list) == len(mine):
            # a slot the other set's object took over keeps its id: equal bytes, so it names an equal row
            tag = ids[0]
            if all(getattr(b, '_dev', (None,))[0] == tag for b in added):
                out._dev_ids = (tag, np.concatenate([ids[1], np.fromiter((b._dev[1] for b in added), dtype=np.int32,
                                                                          count=len(added))]))
        return out

    def __len__(self) -> int:
        return len(self._belief_list) if self._belief_list is not None else self._belief_array.shape[0]

    def to_gpu(self) -> 'BeliefSet':
        gm = self.model.gpu_model
        out = BeliefSet(gm, [Belief(gm, b.values) for b in self.belief_list])
        return out

    def to_cpu(self) -> 'BeliefSet':
        cm = self.model.cpu_model
        return BeliefSet(cm, [Belief(cm, b.values) for b in self.belief_list])


# --------------------------------------------------------------------------- #
# HSVI upper bound: the support-restricted sawtooth and the bound-greedy action values (what ``pbvi_upper_bound`` and
# ``pbvi_upper_q`` compute on the device)
# --------------------------------------------------------------------------- #
def sawtooth_numpy(points, values, gaps, corner, beliefs, n_visible: Union[int, None] = None, n_hit: Union[int, None] = None):
    """Sawtooth upper bound of every row of ``beliefs [n,S]`` over the points ``points [P,S]`` with values ``values [P]`` and
    gaps ``gaps [P]`` (``= values - points @ corner``, computed once by the caller) above the corner values ``corner [S]``,
    on the host: what ``pbvi_upper_bound`` computes on the device.

        ``v0 = b . corner;  r_i = min_{s: p_i[s] > 0} b[s] / p_i[s];  w_i = v0 + gap_i * r_i``
        ``U = min(v0, min_{i < n_visible} w_i);  point`` = the first ``i`` attaining it, -1 when ``v0 <= `` every ``w_i``
        ``hit`` = the first ``i < n_hit`` with ``p_i == b``, else -1;  ``value = values[hit] if hit >= 0 else U``

    The minimum runs over the SUPPORT of the point: ``BeliefValueMapping.evaluate``'s reference form divides over all states
    and is NaN (0/0) wherever belief and point share a zero; where that form is finite the two agree.  ``n_visible <= n_hit
    <= P`` (defaults: all) restate the reference's stale cache.  A row that holds a NaN gives NaN, -1, -1.
    Returns ``(value [n] f64, point [n], hit [n])``."""
    c = np.asarray(corner, dtype=np.float64)
    S = c.shape[0]
    p = np.asarray(points, dtype=np.float64).reshape(-1, S)
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    g = np.asarray(gaps, dtype=np.float64).reshape(-1)
    b = np.asarray(beliefs, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != S:
        raise ValueError(f'beliefs must be a [*, {S}] array')
    P = p.shape[0]
    n_hit = P if n_hit is None else int(n_hit)
    n_visible = n_hit if n_visible is None else int(n_visible)
    if not 0 <= n_visible <= n_hit <= P or v.shape[0] < n_hit or g.shape[0] < n_hit:
        raise ValueError('need 0 <= n_visible <= n_hit <= P points, each with a value and a gap')
    n = b.shape[0]
    v0 = np.dot(b, c)
    value = v0.copy()
    point = np.full(n, -1, dtype=np.int64)
    hit = np.full(n, -1, dtype=np.int64)
    nnz_b = np.count_nonzero(b, axis=1)
    with np.errstate(divide='ignore', invalid='ignore', over='ignore'):
        for i in range(n_hit):
            s = np.flatnonzero(p[i] > 0)
            cols = b[:, s]
            if i < n_visible:
                r = np.min(cols / p[i, s], axis=1) if s.size else np.full(n, np.inf)
                w = v0 + g[i] * r
                better = w < value                              # strictly: the first point attaining the minimum keeps it
                value[better] = w[better]
                point[better] = i
            same = (hit < 0) & (nnz_b == s.size) & np.all(cols == p[i, s], axis=1)
            hit[same] = i
    bad = np.isnan(b).any(axis=1)
    value = np.where(hit >= 0, v[np.maximum(hit, 0)] if P else value, value)
    value[bad] = np.nan
    point[bad] = -1
    hit[bad] = -1
    return value, point, hit


def upper_q_first_argmax(Q: np.ndarray) -> np.ndarray:
    """The first action whose ``Q`` is strictly larger than every earlier one; a NaN never wins, a row of NaNs gives 0."""
    return np.argmax(np.where(np.isnan(Q), -np.inf, Q), axis=1)


def _successor_rows(b, rs, rto):
    """The un-normalised Bayes successors of the rows of ``b [n,S]`` (fp64), one ``(a, o, u [n,S])`` per action and
    observation in that order: ``u[i,s'] = sum_{(s,r): rs[s,a,r] = s'} b[i,s] rto[s,a,o,r]`` with ``np.bincount``, whose
    accumulation order (ascending ``s * R + r``) is the order of the device's inverse lists.  ``rs [S,A,R]`` int64,
    ``rto [S,A,O,R]`` already cast to the engine's number format and widened."""
    n, S = b.shape
    R = rs.shape[2]
    base = np.arange(n)[:, None] * S
    for a in range(rs.shape[1]):
        idx = (rs[:, a, :].reshape(1, S * R) + base).ravel()                     # entry s * R + r lands on rs[s, a, r]
        for o in range(rto.shape[2]):
            w = (b[:, :, None] * rto[None, :, a, o, :]).reshape(n, S * R)
            yield a, o, np.bincount(idx, weights=w.ravel(), minlength=n * S).reshape(n, S)


def upper_q_numpy(model, points, values, gaps, corner, beliefs, gamma: float, n_visible: Union[int, None] = None,
                  n_hit: Union[int, None] = None, table_dtype=np.float64):
    """The action values the HSVI descent is greedy for, on the host: what ``pbvi_upper_q`` computes on the device.  With
    ``u`` and ``Z = sum_s' u`` as in ``infotaxis_numpy`` (tables cast to ``table_dtype``, the engine's number format, and
    widened) and ``b_ao = (u / Z)`` rounded to ``table_dtype``, the successor as the engine holds it:

        ``Q[b,a] = b . ER[:,a] + gamma * sum_o Z[a,o] * value(b_ao)``   (sequential over ``o``; ``Z == 0`` adds 0)

    ``value`` is ``sawtooth_numpy``'s.  Returns ``(Q [n,A], action [n], p_obs [n,A,O], succ_value [n,A,O], succ_hit
    [n,A,O])``: ``action`` is ``upper_q_first_argmax(Q)``, ``p_obs`` is ``Z``; at an impossible observation the successor's
    value is NaN and its hit -1."""
    m = _rollout_tables(model)
    S, A, O, R = m.state_count, m.action_count, m.observation_count, m.reachable_state_count
    b = np.asarray(beliefs, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != S:
        raise ValueError(f'beliefs must be a [*, {S}] array')
    n = b.shape[0]
    rto = np.ascontiguousarray(m.reachable_transitional_observation_table, dtype=table_dtype).astype(np.float64)
    er = np.ascontiguousarray(m.expected_rewards_table, dtype=table_dtype).astype(np.float64)
    rs = np.asarray(m.reachable_states).astype(np.int64)
    Q = np.dot(b, er)
    Z = np.zeros((n, A, O))
    sval = np.full((n, A, O), np.nan)
    shit = np.full((n, A, O), -1, dtype=np.int64)
    tail = np.zeros((n, A))
    for a, o, u in _successor_rows(b, rs, rto):
        z = np.sum(u, axis=1)
        Z[:, a, o] = z
        ok = z != 0
        if ok.any():
            succ = (u[ok] / z[ok, None]).astype(table_dtype).astype(np.float64)
            sval[ok, a, o], _, shit[ok, a, o] = sawtooth_numpy(points, values, gaps, corner, succ, n_visible, n_hit)
            tail[ok, a] += z[ok] * sval[ok, a, o]
    Q += gamma * tail
    return Q, upper_q_first_argmax(Q), Z, sval, shit


class BeliefValueMapping:
    """Upper bound of the value function as (belief, value) points over the corner values, evaluated with the
    sawtooth interpolation (``src/pomdp.py:786-895``; used by the HSVI expansion only).

    ``sawtooth='reference'`` (the default) is the reference bit for bit, host-side: its minimum over ALL states is NaN (0/0)
    for every belief that shares a zero with a point.  ``sawtooth='support'`` restricts the minimum to the support of the
    point (``sawtooth_numpy``), adds ``evaluate_block`` for many beliefs at once, and can keep its points in an engine's
    device point store (``pbvi_upper_append``): per engine a cursor remembers how many points it already holds, so only the
    new ones travel."""

    def __init__(self, model, corner_belief_values: ValueFunction, sawtooth: str = 'reference') -> None:
        if sawtooth not in ('reference', 'support'):
            raise ValueError("sawtooth must be 'reference' or 'support'")
        self.model = model
        self.corner_belief_values = corner_belief_values
        self.corner_values = np.max(corner_belief_values.alpha_vector_array, axis=0)
        self.sawtooth = sawtooth
        self.beliefs = []
        self.belief_value_mapping = {}
        self._belief_array = None
        self._value_array = None
        # 'support' only: gap_i = v_i - p_i . corner, computed once when the point is added; the points the cached arrays of
        # the reference would hold (its stale cache); the stacked points; per engine serial (store epoch, points appended)
        self.gaps = []
        self._n_visible = None
        self._rows = np.zeros((0, len(self.corner_values)))
        self._cursor = {}

    def add(self, b: Belief, v: float) -> None:
        """Record ``v`` at ``b``; a belief that is already a point keeps its first value."""
        if b.bytes_repr not in self.belief_value_mapping:
            self.beliefs.append(b)
            self.belief_value_mapping[b.bytes_repr] = v
            if self.sawtooth == 'support':
                self.gaps.append(float(v) - float(np.dot(np.asarray(b.values, dtype=np.float64), self.corner_values)))

    def update(self) -> None:
        """Re-stack the cached point arrays (``evaluate`` reads the cache, so points added since the last call
        are not seen until this runs -- the reference's behaviour, ``src/pomdp.py:863-870``)."""
        if self.sawtooth == 'support':                       # (the cache is a count: the stacked points only grow)
            self._n_visible = len(self.beliefs)
            return
        self._belief_array = np.array([b.values for b in self.beliefs])
        self._value_array = np.array(list(self.belief_value_mapping.values()))

    # -- 'support' mode ------------------------------------------------------------------------------------------- #
    def window(self) -> Tuple[int, int]:
        """``(n_visible, n_hit)``: the points the reference's cached arrays would hold at this moment -- those of the last
        ``update()``, or of the first evaluation that found a point -- and the points its dictionary holds (all)."""
        if self._n_visible is None and self.beliefs:
            self._n_visible = len(self.beliefs)
        return (self._n_visible or 0), len(self.beliefs)

    def point_arrays(self):
        """``(points [P,S], values [P], gaps [P])`` of every point, fp64 (the stack is extended, not rebuilt)."""
        if self._rows.shape[0] < len(self.beliefs):
            fresh = [np.asarray(b.values, dtype=np.float64) for b in self.beliefs[self._rows.shape[0]:]]
            self._rows = np.concatenate([self._rows, np.array(fresh)])
        return self._rows, np.array(list(self.belief_value_mapping.values()), dtype=np.float64), np.array(self.gaps)

    def sync_engine(self, eng) -> None:
        """Bring ``eng``'s device point store up to this mapping's points: a reset with the corner values when the store
        is not (or no longer) this mapping's, then only the points added since the last call."""
        if self.sawtooth != 'support':
            raise ValueError("the device point store needs sawtooth='support'")
        epoch, done = self._cursor.get(eng.serial, (None, 0))
        if epoch != eng.upper_epoch or getattr(eng, '_upper_owner', None) is not self or done != eng.upper_count:
            eng.upper_reset(self.corner_values)
            eng._upper_owner = self
            done = 0
        if done < len(self.beliefs):
            rows, values, gaps = self.point_arrays()
            eng.upper_append(rows[done:], values[done:], gaps[done:])
            done = len(self.beliefs)
        self._cursor[eng.serial] = (eng.upper_epoch, done)

    def evaluate_block(self, beliefs, engine=None) -> np.ndarray:
        """``evaluate`` for every row of ``beliefs [n,S]`` (``'support'`` only): through ``engine``'s ``pbvi_upper_bound``
        when one is given, else ``sawtooth_numpy``."""
        if self.sawtooth != 'support':
            raise ValueError("evaluate_block needs sawtooth='support'")
        arr = np.asarray(beliefs, dtype=np.float64)
        n_visible, n_hit = self.window()
        if engine is not None:
            self.sync_engine(engine)
            engine.set_beliefs(arr)
            return engine.upper_bound_resident(n_visible, n_hit)[0]
        rows, values, gaps = self.point_arrays()
        return sawtooth_numpy(rows, values, gaps, self.corner_values, arr, n_visible, n_hit)[0]

    @property
    def belief_array(self) -> np.ndarray:
        if self._belief_array is None:
            self._belief_array = np.array([b.values for b in self.beliefs])
        return self._belief_array

    @property
    def value_array(self) -> np.ndarray:
        if self._value_array is None:
            self._value_array = np.array(list(self.belief_value_mapping.values()))
        return self._value_array

    def evaluate(self, belief: Belief) -> float:
        hit = self.belief_value_mapping.get(belief.bytes_repr)
        if hit is not None:
            return hit
        if self.sawtooth == 'support':
            return float(self.evaluate_block(np.asarray(belief.values)[None, :])[0])
        v0 = np.dot(belief.values, self.corner_values)
        if len(self.beliefs) == 0:
            return float(v0)
        with np.errstate(divide='ignore', invalid='ignore'):
            gap = self.value_array - np.dot(self.belief_array, self.corner_values)
            vb = v0 + gap * np.min(belief.values / self.belief_array, axis=1)
        return float(np.min(np.append(vb, v0)))


class SolverHistory:
    """Times and sizes of a PBVI run (subset of ``src/pomdp.py:898-1117``)."""

    def __init__(self, tracking_level, model, gamma, eps, expand_function, expand_append,
                 initial_value_function, initial_belief_set):
        self.tracking_level = tracking_level
        self.model = model
        self.gamma = gamma
        self.eps = eps
        self.run_ts = datetime.now()
        self.expand_function = expand_function
        self.expand_append = expand_append
        self.expansion_times = []
        self.backup_times = []
        self.pruning_times = []
        self.alpha_vector_counts = []
        self.beliefs_counts = []
        self.value_function_changes = []
        self.prune_counts = []
        self.value_functions = []
        self.belief_sets = []
        if tracking_level >= 1:
            self.alpha_vector_counts.append(len(initial_value_function))
            self.beliefs_counts.append(len(initial_belief_set))
        if tracking_level >= 2:
            self.value_functions.append(initial_value_function)
            self.belief_sets.append(initial_belief_set)

    def add_expand_step(self, expansion_time: float, belief_set: BeliefSet) -> None:
        if self.tracking_level >= 1:
            self.expansion_times.append(float(expansion_time))
            self.beliefs_counts.append(len(belief_set))
        if self.tracking_level >= 2:
            self.belief_sets.append(belief_set)

    def add_backup_step(self, backup_time: float, value_function_change: float, value_function: ValueFunction) -> None:
        if self.tracking_level >= 1:
            self.backup_times.append(float(backup_time))
            self.alpha_vector_counts.append(len(value_function))
            self.value_function_changes.append(float(value_function_change))
        if self.tracking_level >= 2:
            self.value_functions.append(value_function)

    def add_prune_step(self, prune_time: float, alpha_vectors_pruned: int) -> None:
        if self.tracking_level >= 1:
            self.pruning_times.append(prune_time)
            self.prune_counts.append(alpha_vectors_pruned)

    @property
    def solution(self) -> ValueFunction:
        assert self.tracking_level >= 2, "Tracking level is set too low, increase it to 2 if you want to have value function tracking as well."
        return self.value_functions[-1]

    @property
    def explored_beliefs(self) -> BeliefSet:
        assert self.tracking_level >= 2, "Tracking level is set too low, increase it to 2 if you want to have belief sets tracking as well."
        return self.belief_sets[-1]

    @property
    def summary(self) -> str:
        n_b, n_e = len(self.backup_times), len(self.expansion_times)
        s = f'Summary of Point Based Value Iteration run\n'
        s += f'  - Model: {self.model.state_count} state, {self.model.action_count} action, {self.model.observation_count} observations\n'
        s += f'  - Converged or stopped after {n_e} expansion steps and {n_b} backup steps.\n'
        if n_b and n_e:
            s += f'  - Resulting value function has {self.alpha_vector_counts[-1]} alpha vectors.\n'
            s += f'  - Converged in {sum(self.expansion_times) + sum(self.backup_times):.4f}s\n\n'
            s += f'  - Expand function took on average {sum(self.expansion_times) / n_e:.4f}s\n'
            s += f'  - Backup function took on average {sum(self.backup_times) / n_b:.4f}s\n'
        return s


class Solver(MDP_Solver):
    def solve(self, model):
        raise Exception("Method has to be implemented by subclass...")


class PBVI_Solver(Solver):
    """Point-Based Value Iteration (``src/pomdp.py:1301-2413``).

    ``backup`` is the hot path.  On GPU-resident inputs it is one call into the
    HIP engine; on host inputs it is the reference's NumPy statement sequence.
    """

    def __init__(self, gamma: float = 0.99, eps: float = 0.001, expand_function: str = 'ssea', **expand_function_params):
        self.gamma = gamma
        self.eps = eps
        self.expand_function = expand_function
        self.expand_function_params = expand_function_params

    def test_n_simulations(self, model: Model, value_function: ValueFunction, n: int = 1000, horizon: int = 300,
                           print_progress: bool = False):
        """Roll the greedy policy of ``value_function`` out in ``n`` simulations advanced together
        (``src/pomdp.py:1338-1444``).  Unlike ``Agent.run_n_simulations_parallel`` every simulation keeps being
        stepped after it reached an end state (its rewards are masked instead).  Returns ``(start_states,
        done_at_step, rewards, discounted_rewards)`` -- the last two are lists of ``[n]`` arrays, one per step.
        With the value function on the GPU the belief block lives in the HIP engine for the whole run."""
        on_gpu = value_function.is_on_gpu
        model = model.gpu_model if on_gpu else model.cpu_model
        beliefs = np.repeat(Belief(model).values[None, :], n, axis=0)
        sims = SimulationSet(model.cpu_model)
        start_states = sims.initialize_simulations(n)
        block = (_DeviceBeliefBlock if on_gpu else _HostBeliefBlock)(model, value_function, beliefs)
        everyone = np.ones(n, dtype=bool)
        end_states = np.array(model.end_states)
        done_at_step = np.full(n, -1)
        actions_of = np.asarray(value_function.actions)
        discount = self.gamma
        rewards, discounted_rewards = [], []
        for i in range(horizon):
            was_done = sims.is_done.copy()
            best_actions = actions_of[block.best_vectors()]
            step_rewards, observations = sims.run_actions(best_actions)
            block.advance(best_actions, observations, everyone)
            rewards.append(step_rewards)
            discounted_rewards.append(step_rewards * discount)
            are_done = np.isin(sims.agent_states, end_states)
            done_at_step[was_done ^ are_done] = i + 1
            discount *= self.gamma
            if np.all(sims.is_done):
                break
        return start_states, done_at_step, rewards, discounted_rewards

    # ------------------------------------------------------------------ #
    # hot path
    # ------------------------------------------------------------------ #
    BELIEF_BLOCK = 32768      # beliefs per engine call on the GPU path
    shard_beliefs = None      # True: shard `backup` over the ranks of the torch.distributed job; None: dist.enable() / PBVI_SHARD

    def backup(self, model: Model, belief_set: BeliefSet, value_function: ValueFunction,
               append: bool = False, belief_dominance_prune: bool = True) -> ValueFunction:
        """One point-based backup (``src/pomdp.py:1447-1524``): B beliefs x V
        alpha-vectors -> at most B new alpha-vectors (+ union with the old set).

        With ``self.shard_beliefs = True`` (or ``dist.enable()`` / ``PBVI_SHARD=1``) as one rank of a multi-rank
        ``torch.distributed`` job (one process per GPU) the beliefs are sharded over the ranks, one all-gather makes
        every rank hold the whole result and every replica appends the same rows (``dist.sharded_backup``); the return
        value is the single-process one on every rank.  Opt-in: every rank must call with the same model, beliefs and
        value function (checked as far as a message trailer can: ``dist.ReplicaMismatch``)."""
        if _dist.active(solver=self) and len(belief_set) > 0:
            new_vf = _dist.sharded_backup(self, model, belief_set, value_function, belief_dominance_prune)
        elif value_function.is_on_gpu:
            # Residency: every AlphaVector / Belief row is uploaded once into the engine's device stores; the
            # working sets are selected by id in list order (tie-breaks follow the host order), the device
            # runs the backup, and only the distinct new rows come back.
            eng = value_function.model.engine
            beliefs = belief_set.belief_list
            if self.tile_gamma and eng.gamma_tiling[0] == 'off':
                eng.set_gamma_tiling('auto')
            try:
                if self._belief_chunk is not None and len(beliefs) > self._belief_chunk:
                    raise MemoryError('an earlier backup of this solver only fitted in belief chunks')
                alpha_new, actions = self._backup_block(eng, value_function, belief_set, beliefs, belief_dominance_prune)
            except MemoryError as e:
                if len(beliefs) < 2:
                    raise
                if self._belief_chunk is None:
                    log(f'[Warning] Backup of {len(beliefs)} beliefs does not fit the device ({e}); continuing in belief chunks...')
                alpha_new, actions = self._backup_in_chunks(eng, value_function, beliefs, belief_dominance_prune)
            new_vf = (ValueFunction(value_function.model, alpha_new) if isinstance(alpha_new, list)
                      else ValueFunction(value_function.model, alpha_new, actions))
        else:
            alpha_new, actions = self._backup_numpy(model, belief_set.belief_array, value_function.alpha_vector_array,
                                                    belief_dominance_prune)
            new_vf = ValueFunction(model, alpha_new, actions)
        if append:
            new_vf.extend(value_function)
        return new_vf

    # True: the engines this solver backs up on tile Gamma over the alpha set when it does not fit the device
    # (Engine.set_gamma_tiling('auto')): an alpha-side backup is then served by ONE engine call within the memory there is,
    # and the belief chunks below are reached only if that call still raises MemoryError.  False: nothing changes.
    tile_gamma = False
    _belief_chunk = None      # set once a block only fitted the device in pieces: later backups start there

    def _backup_block(self, eng, value_function, belief_set, beliefs, belief_dominance_prune):
        """The device backup of one belief list against the resident value function: rows (``AlphaVector`` objects tagged
        with their device residency, or an array) and actions."""
        eng.sync_rows('alpha', value_function.alpha_vector_list, lambda v: v.values, owner=value_function)
        if len(beliefs) <= self.BELIEF_BLOCK:
            eng.sync_rows('belief', beliefs, lambda b: b.values, owner=belief_set)
            stats = eng.run(self.gamma, belief_dominance_prune)
            if stats['formulation'] == 2:
                # belief-side GEMM: it also multiplied the beliefs themselves by the alpha set; compute_change asks for
                # exactly those maxima next (these beliefs, the value function that was just backed up)
                eng.seed_max_values(value_function.alpha_vector_list, beliefs, lambda v: v.values, lambda b: b.values,
                                    alpha_owner=value_function, belief_owner=belief_set)
            alpha_new, actions, uidx = eng.fetch().value_function_rows(use_keep=belief_dominance_prune, with_index=True)
            if len(uidx):
                # the new rows join the engine's alpha store device to device: the next call selects them by id;
                # their dedup hashes come from the device too (ValueFunction keys its dictionary on them)
                first, tag = eng.store_unique(uidx), eng.store_tag('alpha')
                hashes = eng.fetch_row_hashes()[uidx]
                vectors = []
                for k, (row, act) in enumerate(zip(alpha_new, actions)):
                    v = AlphaVector(row, act)
                    v._dev = (tag, first + k)
                    v._hash = int(hashes[k])
                    vectors.append(v)
                alpha_new = vectors
        else:   # beliefs are independent: larger sets go through the engine in blocks (it takes 65535 at a time)
            parts = []
            for i0 in range(0, len(beliefs), self.BELIEF_BLOCK):
                eng.sync_rows('belief', beliefs[i0:i0 + self.BELIEF_BLOCK], lambda b: b.values)
                eng.run(self.gamma, belief_dominance_prune)
                parts.append(eng.fetch().value_function_rows(use_keep=belief_dominance_prune))
            alpha_new = np.concatenate([p[0] for p in parts])
            actions = np.concatenate([p[1] for p in parts])
        return alpha_new, actions

    def _backup_in_chunks(self, eng, value_function, beliefs, belief_dominance_prune):
        """A backup whose working set did not fit the device (the engine raised ``MemoryError`` and is back in its freshly
        created state), done in belief chunks: beliefs are independent, so the union of the chunks' rows is the block's
        result (the constructor of ``ValueFunction`` drops duplicates as it does for one block).  Chunks project the
        BELIEFS through the model, whose footprint is chunk x A x O rows, instead of Gamma's A x O x V rows -- the array
        the reference's CuPy path dies allocating (``Sea_Robin_Real.ipynb:913``) -- and are halved until one fits; a
        single belief that does not fit re-raises, which ``solve`` turns into the partial result
        (``src/pomdp.py:2399-2401``)."""
        chunk = self._belief_chunk if self._belief_chunk is not None else (len(beliefs) + 1) // 2
        # (never above the block size of one engine call: the engine refuses larger blocks with an error that is not a
        # MemoryError, which the halving below would not catch)
        chunk = max(1, min(chunk, (len(beliefs) + 1) // 2, self.BELIEF_BLOCK))
        setting = eng.formulation
        while True:
            # (not inside the try: a value function that does not fit by itself is not cured by smaller chunks)
            eng.sync_rows('alpha', value_function.alpha_vector_list, lambda v: v.values, owner=value_function)
            try:
                eng.set_formulation('belief' if chunk <= len(value_function) else 'auto')
                parts = []
                for i0 in range(0, len(beliefs), chunk):
                    eng.sync_rows('belief', beliefs[i0:i0 + chunk], lambda b: b.values)
                    eng.run(self.gamma, belief_dominance_prune)
                    parts.append(eng.fetch().value_function_rows(use_keep=belief_dominance_prune))
                self._belief_chunk = chunk
                return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
            except MemoryError:
                if chunk == 1:
                    raise
                chunk = (chunk + 1) // 2
            finally:
                eng.set_formulation(setting)

    def _backup_numpy(self, model, b, alpha, belief_dominance_prune, return_mask: bool = False):
        """Host path: the reference's array statements (``src/pomdp.py:1485-1515``).  ``return_mask``: every belief's
        row and action plus the belief-dominance mask, instead of the filtered rows (the sharded backup exchanges
        per-belief results)."""
        V = alpha.shape[0]
        alpha_r = alpha[np.arange(V)[:, None, None, None], model.reachable_states[None, :, :, :]]
        gamma_aovs = self.gamma * np.einsum('saor,vsar->aovs', model.reachable_transitional_observation_table, alpha_r)
        pick = np.argmax(np.tensordot(b, gamma_aovs, (1, 3)), axis=3)
        per_o = gamma_aovs[model.actions[None, :, None, None], model.observations[None, None, :, None],
                           pick[:, :, :, None], model.states[None, None, None, :]]
        alpha_a = model.expected_rewards_table.T + np.sum(per_o, axis=2)
        acts = np.argmax(np.einsum('bas,bs->ba', alpha_a, b), axis=1)
        rows = np.take_along_axis(alpha_a, acts[:, None, None], axis=1)[:, 0, :]
        better = np.ones(len(acts), dtype=bool)
        if belief_dominance_prune:
            new_val = np.sum(b * rows, axis=1)
            old_val = np.max(np.matmul(b, alpha.T), axis=1)
            better = new_val > old_val
        if return_mask:
            return rows, acts, better
        if belief_dominance_prune:
            rows, acts = rows[better], acts[better]
        return rows, acts

    def q_values(self, model: Model, beliefs, value_function: ValueFunction) -> np.ndarray:
        """One-step lookahead values ``Q[b,a] = b.ER[:,a] + gamma * sum_o max_v b.Gamma[a,o,v]`` (Gamma as in
        ``src/pomdp.py:1485-1491``; the quantity the backup maximises over ``a``, ``:1495-1505``) of a ``BeliefSet``, a
        ``Belief`` or a ``[B,S]`` array, as ``[B,A]`` float64.  With the value function on the GPU the HIP engine
        computes it (``pbvi_q_values``), in blocks of ``_DeviceBeliefBlock.CHUNK`` beliefs; otherwise NumPy does."""
        if isinstance(beliefs, BeliefSet):
            arr = beliefs.belief_array
        elif isinstance(beliefs, Belief):
            arr = beliefs.values[None, :]
        else:
            arr = np.asarray(beliefs)
            arr = arr[None, :] if arr.ndim == 1 else arr
        if value_function.is_on_gpu:
            return _q_values_device(value_function, arr, self.gamma)[0]
        return _q_values_numpy(model.cpu_model if model.is_on_gpu else model, arr, value_function.alpha_vector_array, self.gamma)

    # ------------------------------------------------------------------ #
    # belief expansion (host side; out of the accelerated path)
    # ------------------------------------------------------------------ #
    def expand_ra(self, model, belief_set, max_generation: int = 10) -> BeliefSet:
        n = min(belief_set.belief_array.shape[0], max_generation)
        nb = np.random.random((n, model.state_count))
        nb /= np.sum(nb, axis=1)[:, None]
        return BeliefSet(model, nb)

    def _sim_step(self, model, b: Belief, a: int) -> Belief:
        s = b.random_state()
        s_p = model.transition(s, a)
        return b.update(a, model.observe(s_p, a))

    def expand_ssra(self, model, belief_set, max_generation: int = 10) -> BeliefSet:
        arr = belief_set.belief_array
        n = min(max_generation, arr.shape[0])
        picks = np.random.choice(np.arange(arr.shape[0]), n, replace=False)
        out = np.empty((n, arr.shape[1]))
        for i, row in enumerate(arr[picks]):
            b = Belief(model, row)
            s = b.random_state()
            a = random.choice(model.actions)
            s_p = model.transition(s, a)
            out[i] = b.update(a, model.observe(s_p, a)).values
        return BeliefSet(model, out)

    def expand_ssga(self, model, belief_set, value_function, epsilon: float = 0.1, max_generation: int = 10) -> BeliefSet:
        arr = belief_set.belief_array
        n = min(max_generation, arr.shape[0])
        picks = np.random.choice(np.arange(arr.shape[0]), n, replace=False)
        out = np.empty((n, arr.shape[1]))
        for i, row in enumerate(arr[picks]):
            b = Belief(model, row)
            s = b.random_state()
            if random.random() < epsilon:
                a = random.choice(model.actions)
            else:
                a = value_function.actions[np.argmax(np.dot(value_function.alpha_vector_array, b.values))]
            s_p = model.transition(s, a)
            out[i] = b.update(a, model.observe(s_p, a)).values
        return BeliefSet(model, out)

    def expand_ssea(self, model, belief_set, max_generation: int = 10) -> BeliefSet:
        arr = belief_set.belief_array
        n = min(max_generation, arr.shape[0])
        succ = np.array([[[b.update(a, o).values for o in model.observations] for a in model.actions]
                         for b in belief_set.belief_list])
        diff = arr[:, None, None, None, :] - succ
        dist = np.sqrt(np.einsum('bnaos,bnaos->bnao', diff, diff))
        nearest = np.min(dist, axis=0)
        b_i, a_i, o_i = np.unravel_index(np.argsort(nearest, axis=None)[::-1][:n], succ.shape[:-1])
        return BeliefSet(model, succ[b_i[:, None], a_i[:, None], o_i[:, None], model.states[None, :]])

    def expand_ger(self, model, belief_set, value_function, max_generation: int = 10) -> BeliefSet:
        arr = belief_set.belief_array
        n = min(max_generation, arr.shape[0])
        r_lo = model._min_reward / (1 - self.gamma)
        r_hi = model._max_reward / (1 - self.gamma)
        succ = np.array([[[b.update(a, o).values for o in model.observations] for a in model.actions]
                         for b in belief_set.belief_list])
        va = value_function.alpha_vector_array
        own = va[np.argmax(np.dot(arr, va.T), axis=1)]
        d_b = succ - arr[:, None, None, :]
        d_a = np.where(d_b >= 0, r_hi, r_lo) - own[:, None, None, :]
        err = np.einsum('baos,baos->bao', d_a, d_b)
        p_bao = np.einsum('bs,saor->bao', arr, model.reachable_transitional_observation_table)
        score = np.einsum('bao,bao->ba', p_bao, err)
        b_i, a_i = np.unravel_index(np.argsort(score, axis=None)[::-1][:n], score.shape)
        o_i = np.argmax(p_bao[b_i[:, None], a_i[:, None], model.observations[None, :]]
                        * err[b_i[:, None], a_i[:, None], model.observations[None, :]], axis=1)
        return BeliefSet(model, succ[b_i[:, None], a_i[:, None], o_i[:, None], model.states[None, :]])

    def expand_hsvi(self, model, b: Belief, value_function: ValueFunction, upper_bound_belief_value_map: BeliefValueMapping,
                    conv_term: Union[float, None] = None, max_generation: int = 10, sawtooth: Union[str, None] = None,
                    trace: Union[list, None] = None) -> BeliefSet:
        """HSVI descent (``src/pomdp.py:1768-1868``): from ``b`` take the action that is greedy for the upper bound,
        then the observation with the largest probability-weighted gap between the bounds, until the gap falls under
        ``eps / gamma^depth`` or ``max_generation`` beliefs are out.  The deepest belief comes first in the result.
        The lower bound ``max_v alpha_v . b`` is one small matrix-vector product per observation and stays on the host.

        ``sawtooth`` (default: the mapping's own mode) ``'reference'`` is the reference bit for bit -- on a belief with
        zeros its upper bound is NaN and the chain is the start belief's first successor alone.  ``'support'`` evaluates
        the bound with ``sawtooth_numpy``'s definition, lets an impossible observation add 0 and never chooses one, and
        runs on the engine when the value function is on the GPU (``_expand_hsvi_support``).  ``trace``, a list, receives
        one dict per step of a ``'support'`` descent: the action values, the chosen (action, observation), the
        observations' scores and gaps, and the hits met."""
        mode = upper_bound_belief_value_map.sawtooth if sawtooth is None else sawtooth
        if mode not in ('reference', 'support'):
            raise ValueError("sawtooth must be 'reference' or 'support'")
        if mode != upper_bound_belief_value_map.sawtooth:
            raise ValueError(f"the upper bound mapping was built with sawtooth={upper_bound_belief_value_map.sawtooth!r}")
        if mode == 'support':
            return self._expand_hsvi_support(model, b, value_function, upper_bound_belief_value_map, conv_term, max_generation,
                                             trace)
        rto = model.reachable_transitional_observation_table
        alpha = value_function.alpha_vector_array
        conv = self.eps if conv_term is None else conv_term
        chain = []
        while True:
            conv /= self.gamma
            best_q, best_a = -np.inf, -1
            for a in model.actions:
                p_o = np.einsum('sor,s->o', rto[:, a, :, :], b.values)
                tail = 0
                for o in model.observations:
                    tail += p_o[o] * upper_bound_belief_value_map.evaluate(b.update(a, o))
                q = float(np.dot(model.expected_rewards_table[:, a], b.values) + self.gamma * tail)
                if q > best_q:
                    best_q, best_a = q, a
            p_o = np.einsum('sor,s->o', rto[:, best_a, :, :], b.values)
            top, gap_at_top, nxt = -np.inf, -np.inf, b
            for o in model.observations:
                bao = b.update(best_a, o)
                gap = upper_bound_belief_value_map.evaluate(bao) - np.max(np.dot(alpha, bao.values))
                if p_o[o] * gap > top:
                    top, gap_at_top, nxt = p_o[o] * gap, gap, bao
            chain.append(nxt)
            if gap_at_top < conv or max_generation <= 1:
                break
            upper_bound_belief_value_map.add(b, best_q)
            b = nxt
            max_generation -= 1
        return BeliefSet(model, chain[::-1])

    def _expand_hsvi_support(self, model, b: Belief, value_function: ValueFunction, ub: BeliefValueMapping,
                             conv_term: Union[float, None], max_generation: int, trace: Union[list, None]) -> BeliefSet:
        """``expand_hsvi`` over the support-restricted sawtooth.  Per step: the action values of ``b`` under the upper bound
        (``pbvi_upper_q`` / ``upper_q_numpy``) and their first maximum; the successors of that action under every POSSIBLE
        observation (an impossible one has no successor, adds 0 and is never chosen); their lower bound ``max_v alpha_v .
        b'`` and upper bound; the first largest ``P(o) * gap``.  With the value function on the GPU the three stages are engine
        calls on the resident block (``upper_q``, then ``belief_update`` + ``max_value`` + ``upper_bound`` on the successors) and
        the point store takes only the point each step adds; otherwise they are the NumPy restatements."""
        conv = self.eps if conv_term is None else conv_term
        on_gpu = bool(getattr(value_function, 'is_on_gpu', False))
        if on_gpu:
            eng = model.engine
            eng.sync_rows('alpha', value_function.alpha_vector_list, lambda v: v.values)
        else:
            alpha = value_function.alpha_vector_array
        chain = []
        while True:
            conv /= self.gamma
            n_visible, n_hit = ub.window()
            row = np.asarray(b.values, dtype=np.float64)[None, :]
            if on_gpu:
                ub.sync_engine(eng)
                eng.set_beliefs(row)
                q, act, p_obs = eng.upper_q_resident(self.gamma, n_visible, n_hit, want_p_obs=True)
                hits = 0
            else:
                rows, values, gaps = ub.point_arrays()
                q, act, p_obs, _, succ_hit = upper_q_numpy(model, rows, values, gaps, ub.corner_values, row, self.gamma,
                                                           n_visible, n_hit)
                hits = int(np.sum(succ_hit >= 0))
            best_a = int(act[0])
            best_q = float(q[0, best_a])
            p_o = p_obs[0, best_a]
            obs = np.flatnonzero(p_o > 0)
            if on_gpu:
                succ = eng.belief_update(np.repeat(row, len(obs), axis=0), np.full(len(obs), best_a), obs).astype(np.float64)
                eng.set_beliefs(succ)
                low = eng.max_value_resident()[0]
                up, _, hit = eng.upper_bound_resident(n_visible, n_hit)
                hits += int(np.sum(hit >= 0))
                successors = []
                for k in range(len(obs)):
                    nb = Belief.__new__(Belief)
                    nb.model = b.model
                    nb._values = succ[k]
                    successors.append(nb)
            else:
                successors = [b.update(best_a, int(o)) for o in obs]
                hits += sum(1 for s in successors if s.bytes_repr in ub.belief_value_mapping)
                low = np.array([np.max(np.dot(alpha, s.values)) for s in successors])
                up = np.array([ub.evaluate(s) for s in successors])
            gap = up - low
            score = p_o[obs] * gap
            top, gap_at_top, nxt, chosen = -np.inf, -np.inf, b, -1
            for k in range(len(obs)):
                if score[k] > top:
                    top, gap_at_top, nxt, chosen = score[k], gap[k], successors[k], int(obs[k])
            if trace is not None:
                trace.append(dict(q=np.array(q[0]), action=best_a, observations=obs, scores=score, gaps=gap, observation=chosen,
                                  hits=hits, belief=row[0]))
            chain.append(nxt)
            if gap_at_top < conv or max_generation <= 1:
                break
            ub.add(b, best_q)
            b = nxt
            max_generation -= 1
        return BeliefSet(model, chain[::-1])

    def _walk_device(self, model, b0: Belief, policy_action, max_generation: int) -> BeliefSet:
        """``_walk`` with the beliefs on the device.  The (action, observation) trajectory is simulated in the underlying
        MDP and does not depend on the beliefs, so it is drawn first (same random draws, same order), then the n
        chained Bayes updates run in one C-ABI call (``pbvi_belief_walk``): the new beliefs land in the engine's
        belief store -- the following backup selects them by id, nothing is uploaded -- and their fp64 values come
        back once for the containers' byte-keyed dedup."""
        acts, obs, restart = [], [], []
        s = b0.random_state()
        fresh = True                                   # the belief this step starts from is b0
        for i in range(max_generation - 1):
            a = int(policy_action(i, s))
            s_p = model.transition(s, a)
            acts.append(a)
            obs.append(model.observe(s_p, a))
            restart.append(fresh)
            fresh = False
            s = s_p
            if s in model.end_states:
                s = b0.random_state()
                fresh = True
        if not acts:
            return BeliefSet(model, [b0])
        eng = model.engine
        values, first = eng.belief_walk(b0.values, acts, obs, restart)
        sums = eng.belief_walk_keys(len(acts)).tolist() if hasattr(eng, 'belief_walk_keys') else None
        tag = eng.belief_tag()
        seq = [b0]
        for i in range(len(acts)):
            nb = Belief.__new__(Belief)
            nb.model = b0.model
            nb._values = values[i]
            nb._dev = (tag, first + i)
            if sums is not None:                       # the dedup key's hash comes from the device: no host pass over the row
                nb._key = _RowKey.from_sum(sums[i], values[i])
            seq.append(nb)
        return BeliefSet(model, seq)

    def _walk(self, model, b0: Belief, policy_action, max_generation: int) -> BeliefSet:
        if getattr(model, 'is_on_gpu', False):
            return self._walk_device(model, b0, policy_action, max_generation)
        seq = [b0]
        s = b0.random_state()
        b = b0
        for i in range(max_generation - 1):
            a = policy_action(i, s)
            s_p = model.transition(s, a)
            b = b.update(a, model.observe(s_p, a))
            seq.append(b)
            s = s_p
            if s in model.end_states:
                s = b0.random_state()
                b = b0
        return BeliefSet(model, seq)

    def expand_fsvi(self, model, b0: Belief, mdp_policy: ValueFunction, max_generation: int = 10) -> BeliefSet:
        q = mdp_policy.alpha_vector_array
        return self._walk(model, b0, lambda i, s: np.argmax(q[:, s]), max_generation)

    def expand_fsvi_eg(self, model, b0, mdp_policy, eps_greedy=None, max_generation: int = 10) -> BeliefSet:
        q = mdp_policy.alpha_vector_array
        eg = eps_greedy if eps_greedy is not None else (lambda t: 0.2)
        return self._walk(model, b0, lambda i, s: int(random.choice(model.actions)) if random.random() < eg(i)
                          else np.argmax(q[:, s]), max_generation)

    def expand_perseus(self, model, b: Belief, max_generation: int = 10) -> BeliefSet:
        seq = []
        for _ in range(max_generation):
            a = int(np.random.choice(model.actions, size=1)[0])
            p_o = np.einsum('sor,s->o', model.reachable_transitional_observation_table[:, a, :, :], b.values)
            o = int(np.random.choice(model.observations, size=1, p=p_o)[0])
            b = b.update(a, o)
            seq.append(b)
        return BeliefSet(model, seq)

    def expand(self, model, belief_set, max_generation: int, **params) -> BeliefSet:
        """Dispatch by substring exactly like ``src/pomdp.py:2088-2136``: ``self.expand_function`` is one of ``ra``,
        ``ssra``, ``ssga``, ``ssea``, ``ger``, ``hsvi``, ``fsvi``, ``fsvi_eg``, ``perseus``, with or without the
        ``expand_`` prefix; the order of the tests matters (``'ra'`` is also a substring of ``'expand_ssra'``, ``'fsvi'``
        of ``'expand_fsvi_eg'``).

        ``ssea`` and ``ger`` update every belief with every (action, observation), so they cannot run on a model with
        an impossible observation -- one of probability 0 at every successor some belief reaches, as in 4x3.95,
        cheese.95 and hallway: ``Belief.update`` divides by zero and the belief's check raises ``AssertionError: States
        probabilities in belief must sum to 1 (found: nan)``.  They run on tiger and on any model whose observation
        table is strictly positive.  This matches the reference, which raises the same way on the same models."""
        f = self.expand_function
        if f in 'expand_ra':
            return self.expand_ra(model, belief_set, max_generation)
        if f in 'expand_ssra':
            return self.expand_ssra(model, belief_set, max_generation)
        if f in 'expand_ssga':
            kw = {k: params[k] for k in ('value_function', 'epsilon') if k in params}
            return self.expand_ssga(model, belief_set, max_generation=max_generation, **kw)
        if f in 'expand_ssea':
            return self.expand_ssea(model, belief_set, max_generation)
        if f in 'expand_ger':
            return self.expand_ger(model, belief_set, params['value_function'], max_generation)
        if f in 'expand_hsvi':
            if not hasattr(self, '_upper_bound'):          # kept on the solver across calls, like src/pomdp.py:2112-2115
                self._upper_bound = BeliefValueMapping(model, params['mdp_policy'], sawtooth=params.get('sawtooth', 'reference'))
            else:
                self._upper_bound.update()
            return self.expand_hsvi(model, belief_set.belief_list[0], params['value_function'], self._upper_bound,
                                    max_generation=max_generation)
        if f in 'expand_fsvi':
            return self.expand_fsvi(model, belief_set.belief_list[0], params['mdp_policy'], max_generation)
        if f in 'expand_fsvi_eg':
            return self.expand_fsvi_eg(model, belief_set.belief_list[0], params['mdp_policy'],
                                       params.get('eps_greedy'), max_generation)
        if f in 'expand_perseus':
            return self.expand_perseus(model, belief_set.belief_list[0], max_generation)
        raise Exception('Not implemented')

    def compute_change(self, value_function: ValueFunction, new_value_function: ValueFunction, belief_set: BeliefSet) -> float:
        """Largest change of ``max_v b.alpha_v`` over the belief set (``src/pomdp.py:2141-2169``)."""
        if value_function.is_on_gpu:
            # the belief set and the alpha set only grow between calls: the engine wrapper scores just the new
            # (belief, alpha) pairs and keeps the rest (Engine.max_value_objects)
            eng = value_function.model.engine
            beliefs = belief_set.belief_list
            # smaller alpha set first: in the solve loop it is the previous value function, a subset of the other one,
            # so the larger set then only needs (all beliefs x its additional rows)
            pair = sorted((value_function, new_value_function), key=len)
            # only max|new - old| of the values is used, against eps * gamma / (1 - gamma): an f32 engine returns its
            # GEMM's maxima as they are (exact=False); f64 engines are exact either way
            vals = {id(vf): eng.max_value_objects(vf.alpha_vector_list, beliefs, lambda v: v.values, lambda x: x.values,
                                                  alpha_owner=vf, belief_owner=belief_set, exact=False) for vf in pair}
            old, new = vals[id(value_function)], vals[id(new_value_function)]
        else:
            b = belief_set.belief_array
            old = np.max(np.matmul(b, value_function.alpha_vector_array.T), axis=1)
            new = np.max(np.matmul(b, new_value_function.alpha_vector_array.T), axis=1)
        return float(np.max(np.abs(new - old)))

    def _limit_value_function(self, model, value_function: ValueFunction, belief_set: BeliefSet,
                              max_belief_growth: int) -> ValueFunction:
        """The |V| limiter of the solve loop (``src/pomdp.py:2347-2365``): alpha-vectors that are the best one for no
        belief of the set are "unuseful"; ``max_belief_growth`` of them, drawn with replacement and weights falling
        linearly with their position, are deleted.  The usefulness scan -- ``argmax_v`` of the V x B_total score matrix --
        runs on the engine when the value function is on the GPU (``pbvi_value_max_store`` over the belief store in
        place, first maximum, exact indices); the draw stays ``np.random.choice`` on the host, as in the reference."""
        n = len(value_function)
        if value_function.is_on_gpu:
            eng = value_function.model.engine
            beliefs = belief_set.belief_list
            eng.sync_rows('alpha', value_function.alpha_vector_list, lambda v: v.values, owner=value_function)
            b_ids = eng.row_ids('belief', beliefs, lambda b: b.values, owner=belief_set)
            best = eng.best_alpha_of_store_rows(b_ids)
        else:
            best = np.argmax(np.matmul(value_function.alpha_vector_array, belief_set.belief_array.T), axis=0)
        useful = np.unique(best)
        useless = np.delete(np.arange(n), useful)
        w = np.arange(len(useless))[::-1]
        drop = np.random.choice(useless, size=max_belief_growth, p=w / np.sum(w))
        self._last_useful_count = int(useful.shape[0])
        if value_function.is_on_gpu:
            # on the objects: the surviving vectors keep their rows in the device store, nothing is re-stacked
            gone = set(int(i) for i in drop)
            limited = ValueFunction(value_function.model, [v for i, v in enumerate(value_function.alpha_vector_list) if i not in gone])
            for i in gone:
                value_function.alpha_vector_list[i].__dict__.pop('_l2', None)
            limited._take_prune_flags(value_function)       # a subset of a domination-free set is domination-free
            return limited
        limited = ValueFunction(model, np.delete(value_function.alpha_vector_array, drop, axis=0),
                                np.delete(value_function.actions, drop))
        limited._take_prune_flags(value_function, index=np.delete(np.arange(n), drop))
        return limited

    def solve(self, model: Model, expansions: int, full_backup: Union[bool, None] = None, update_passes: int = 1,
              max_belief_growth: int = 10, initial_belief=None, initial_value_function=None, prune_level: int = 1,
              prune_interval: int = 10, limit_value_function_size: int = -1, use_gpu: bool = False,
              history_tracking_level: int = 1, print_progress: bool = True, engine_dtype: str = 'f64'):
        """Expand / backup loop (``src/pomdp.py:2172-2413``).  ``engine_dtype``
        ('f64' or 'f32') is the one added keyword: the arithmetic type of the HIP
        engine when ``use_gpu=True``.  ``prune_level=2, prune_interval=1`` is cheap: after the first level-2 prune only
        the pairs that involve the rows a backup added are tested (``ValueFunction.prune``), with the same result."""
        if use_gpu:
            model = model.to_gpu(engine_dtype) if not model.is_on_gpu else model

        if initial_belief is None:
            belief_set = BeliefSet(model, [Belief(model)])
        elif isinstance(initial_belief, BeliefSet):
            belief_set = initial_belief.to_gpu() if use_gpu else initial_belief
        else:
            belief_set = BeliefSet(model, [Belief(model, np.array(initial_belief.values))])

        if initial_value_function is None:
            value_function = ValueFunction(model, model.expected_rewards_table.T, model.actions)
        else:
            value_function = initial_value_function.to_gpu() if use_gpu else initial_value_function

        if full_backup is None:
            full_backup = any(self.expand_function in f for f in
                              ['expand_ra', 'expand_ssra', 'expand_ssga', 'expand_ssea', 'expand_ger'])

        if ('fsvi' in self.expand_function or 'hsvi' in self.expand_function) and \
                self.expand_function_params.get('mdp_policy') is None:
            log('[Warning] MDP solution not provided, running value iteration on the problem to retrieve it...')
            # Device sweeps are bit-identical to the NumPy loop for R = 1 only; with several reachable states the sum
            # over r may associate differently, and FSVI breaks exact Q-value ties (symmetric grids) by argmax --
            # keep the reference's arithmetic there so seeded runs follow the reference's trajectory.
            mdp_solution, _ = VI_Solver(gamma=self.gamma, eps=self.eps).solve(
                model, use_gpu=use_gpu and model.reachable_state_count == 1, print_progress=False)
            self.expand_function_params['mdp_policy'] = mdp_solution

        max_allowed_change = self.eps * (self.gamma / (1 - self.gamma))
        history = SolverHistory(history_tracking_level, model, self.gamma, self.eps, self.expand_function,
                                full_backup, value_function, belief_set)

        iteration = 0
        expand_value_function = value_function
        old_value_function = value_function
        self._belief_chunk = None              # (backup: the chunk size an earlier solve settled on says nothing about this one)
        try:
            for expansion_i in range(expansions):
                t0 = datetime.now()
                new_belief_set = self.expand(model=model, belief_set=belief_set, value_function=value_function,
                                             max_generation=max_belief_growth, **self.expand_function_params)
                belief_set = belief_set.union(new_belief_set)
                history.add_expand_step((datetime.now() - t0).total_seconds(), belief_set)

                for _ in range(update_passes):
                    t0 = datetime.now()
                    value_function = self.backup(model, belief_set if full_backup else new_belief_set, value_function,
                                                 append=(not full_backup), belief_dominance_prune=False)
                    backup_time = (datetime.now() - t0).total_seconds()

                    if (iteration % prune_interval) == 0 and iteration > 0:
                        t0 = datetime.now()
                        before = len(value_function)
                        value_function.prune(prune_level)
                        history.add_prune_step((datetime.now() - t0).total_seconds(), len(value_function) - before)

                    if limit_value_function_size >= 0 and len(value_function) > limit_value_function_size:
                        value_function = self._limit_value_function(model, value_function, belief_set, max_belief_growth)

                    max_change = self.compute_change(value_function, old_value_function, belief_set)
                    history.add_backup_step(backup_time, max_change, value_function)
                    if max_change < max_allowed_change:
                        break
                    old_value_function = value_function
                    iteration += 1

                if self.compute_change(expand_value_function, value_function, belief_set) < max_allowed_change:
                    print('Converged!')
                    break
                expand_value_function = value_function
        except MemoryError as e:
            print(f'Memory full: {e}')
            print('Returning value function and history as is...\n')

        t0 = datetime.now()
        before = len(value_function)
        value_function.prune(prune_level)
        history.add_prune_step((datetime.now() - t0).total_seconds(), len(value_function) - before)
        return value_function, history


class FSVI_Solver(PBVI_Solver):
    """Forward Search Value Iteration preset (``src/pomdp.py:2470-2544``)."""

    def __init__(self, gamma: float = 0.99, eps: float = 0.001, mdp_policy: Union[ValueFunction, None] = None):
        super().__init__(gamma, eps, 'fsvi', mdp_policy=mdp_policy)

    def solve(self, model, expansions, update_passes: int = 1, max_belief_growth: int = 10, initial_belief=None,
              initial_value_function=None, prune_level: int = 1, prune_interval: int = 10,
              limit_value_function_size: int = -1, use_gpu: bool = False, history_tracking_level: int = 1,
              print_progress: bool = True, engine_dtype: str = 'f64'):
        """``PBVI_Solver.solve`` with ``full_backup=False``.  ``prune_level=2, prune_interval=1`` is cheap: a level-2
        prune after the first tests only the pairs that involve the rows the backup added."""
        return super().solve(model=model, expansions=expansions, full_backup=False, update_passes=update_passes,
                             max_belief_growth=max_belief_growth, initial_belief=initial_belief,
                             initial_value_function=initial_value_function, prune_level=prune_level,
                             prune_interval=prune_interval, limit_value_function_size=limit_value_function_size,
                             use_gpu=use_gpu, history_tracking_level=history_tracking_level,
                             print_progress=print_progress, engine_dtype=engine_dtype)


class FSVI_EG_Solver(FSVI_Solver):
    """Epsilon-greedy FSVI preset (``src/pomdp.py:2547-2578``)."""

    def __init__(self, gamma: float = 0.99, eps: float = 0.001, mdp_policy=None, eps_greedy=None):
        PBVI_Solver.__init__(self, gamma, eps, 'fsvi_eg', mdp_policy=mdp_policy, eps_greedy=eps_greedy)


class HSVI_Solver(PBVI_Solver):
    """Heuristic Search Value Iteration preset (``src/pomdp.py:2416-2478``).  ``sawtooth='reference'`` (the default) keeps
    the reference's upper bound bit for bit, NaN on sparse beliefs included; ``sawtooth='support'`` evaluates it over the
    support of each point (``sawtooth_numpy``), on the engine when the solve runs on the GPU (``expand_hsvi``)."""

    def __init__(self, gamma: float = 0.99, eps: float = 0.001, mdp_solution: Union[ValueFunction, None] = None,
                 sawtooth: str = 'reference', upper_init: str = 'mdp', lower_init: str = 'rewards'):
        if sawtooth not in ('reference', 'support'):
            raise ValueError("sawtooth must be 'reference' or 'support'")
        if upper_init not in ('mdp', 'fib'):
            raise ValueError("upper_init must be 'mdp' or 'fib'")
        if lower_init not in ('rewards', 'blind'):
            raise ValueError("lower_init must be 'rewards' or 'blind'")
        extra = {} if sawtooth == 'reference' else {'sawtooth': sawtooth}
        super().__init__(gamma, eps, 'hsvi', mdp_policy=mdp_solution, **extra)
        self.upper_init = upper_init
        self._fib_tightened = False
        self.lower_init = lower_init
        self._blind_start = None

    def solve(self, model, expansions, max_belief_growth: int = 10, initial_belief=None, initial_value_function=None,
              prune_level: int = 1, prune_interval: int = 10, limit_value_function_size: int = -1, use_gpu: bool = False,
              history_tracking_level: int = 1, print_progress: bool = True, engine_dtype: str = 'f64'):
        """``PBVI_Solver.solve`` with ``full_backup=False`` and one update pass.  ``prune_level=2, prune_interval=1`` is
        cheap: a level-2 prune after the first tests only the pairs that involve the rows the backup added.

        ``upper_init='fib'``: the MDP solution (the given one, or the one ``PBVI_Solver.solve`` would compute) passes
        through ``FIB_Solver`` once, on the device when ``use_gpu``, before it becomes the corner value function of the
        upper bound: corner values that are never above the MDP's.

        ``lower_init='blind'``: when no ``initial_value_function`` is given the loop starts from ``Blind_Solver``'s rows
        (computed once per solver object, on the device when ``use_gpu``) instead of the expected-rewards rows, which are a
        lower bound only where no reward is negative."""
        if self.lower_init == 'blind' and initial_value_function is None:
            if self._blind_start is None:
                self._blind_start, _ = Blind_Solver(gamma=self.gamma, eps=self.eps).solve(
                    model, use_gpu=use_gpu, print_progress=False)
            initial_value_function = self._blind_start
        if self.upper_init == 'fib' and not self._fib_tightened:
            mdp_solution = self.expand_function_params.get('mdp_policy')
            if mdp_solution is None:
                log('[Warning] MDP solution not provided, running value iteration on the problem to retrieve it...')
                mdp_solution, _ = VI_Solver(gamma=self.gamma, eps=self.eps).solve(
                    model, use_gpu=use_gpu and model.reachable_state_count == 1, print_progress=False)
            self.expand_function_params['mdp_policy'], _ = FIB_Solver(gamma=self.gamma, eps=self.eps).solve(
                model, mdp_solution=mdp_solution, use_gpu=use_gpu, print_progress=False)
            self._fib_tightened = True
        return super().solve(model=model, expansions=expansions, full_backup=False, update_passes=1,
                             max_belief_growth=max_belief_growth, initial_belief=initial_belief,
                             initial_value_function=initial_value_function, prune_level=prune_level,
                             prune_interval=prune_interval, limit_value_function_size=limit_value_function_size,
                             use_gpu=use_gpu, history_tracking_level=history_tracking_level,
                             print_progress=print_progress, engine_dtype=engine_dtype)


# --------------------------------------------------------------------------- #
# Fast Informed Bound (Hauskrecht 2000): the definition ``pbvi_fib_value_iteration`` implements, restated with NumPy
# --------------------------------------------------------------------------- #
def _fib_tables(model):
    """``(reachable_states [S,A,R], rto [S,A,O,R], expected_rewards [S,A])`` of a ``Model``, of any object with ``Model``'s
    attribute names, or of a ``synth.SynthModel``."""
    if hasattr(model, 'reachable_transitional_observation_table'):
        m = model.cpu_model if getattr(model, 'is_on_gpu', False) else model
        return (np.asarray(m.reachable_states), np.asarray(m.reachable_transitional_observation_table, dtype=np.float64),
                np.asarray(m.expected_rewards_table, dtype=np.float64))
    return (np.asarray(model.reachable_states), np.asarray(model.rto, dtype=np.float64),
            np.asarray(model.expected_rewards, dtype=np.float64))


def fib_numpy(model, q0, gamma: float, max_change_limit: float, horizon: int):
    """Fast Informed Bound sweeps from ``q0 [A,S]``:

        Q'(s,a) = ER[s,a] + gamma * sum_o max_a' sum_r RTO[s,a,o,r] * Q(rs[s,a,r], a')

    until ``max_{s,a} |Q' - Q| < max_change_limit`` or ``horizon`` sweeps; returns ``(rows [A,S], changes)``, the rows of
    the last sweep that ran (``q0`` for ``horizon = 0``).  The loops over o and r are explicit so that every sum associates
    as the device kernel's does -- ``acc = t_0``, then ``acc = acc + t_r``; ``tot = m_0``, then ``tot = tot + m_o`` -- and
    the two agree bit for bit on finite inputs.  Working memory: S * A * A doubles per observation.

    From the same start a sweep is never above the MDP sweep (``sum_o RTO = P``, and ``max_a' sum_r RTO Q(., a')`` is at most
    ``sum_r RTO max_a' Q(., a')``), it stays an upper bound of the POMDP value, and with one successor per (s, a) the maximum
    moves inside the sum over o and the sweep IS the MDP sweep."""
    rs, rto, er = _fib_tables(model)
    S, A, O, R = rto.shape
    Q = np.ascontiguousarray(np.asarray(q0, dtype=np.float64).T)           # [S,A]: a successor's action values are one row
    if Q.shape != (S, A) or rs.shape != (S, A, R) or er.shape != (S, A):
        raise ValueError('fib_numpy: table shapes do not agree')
    changes = []
    for _ in range(int(horizon)):
        tot = None
        for o in range(O):
            acc = None
            for r in range(R):
                t = rto[:, :, o, r][:, :, None] * Q[rs[:, :, r]]         # [S,A,A']
                acc = t if acc is None else acc + t
            m = np.max(acc, axis=2)
            tot = m if tot is None else tot + m
        new = er + gamma * tot
        change = float(np.max(np.abs(new - Q)))
        Q = new
        changes.append(change)
        if change < max_change_limit:
            break
    return np.ascontiguousarray(Q.T), np.array(changes, dtype=np.float64)


class FIB_Solver(Solver):
    """The Fast Informed Bound as a solver: ``solve`` returns A action-labelled rows of length S, the shape of a policy, so
    the result runs through ``ValueFunction``, ``Agent``, rollouts, ``FSVI_Solver(mdp_policy=...)`` and
    ``HSVI_Solver(mdp_solution=...)`` like the MDP solution does -- as a tighter upper bound wherever moves are
    stochastic, and as the same rows where every (s, a) has one successor."""

    def __init__(self, horizon: int = 10000, gamma: float = 0.99, eps: float = 0.001):
        self.horizon = horizon
        self.gamma = gamma
        self.eps = eps

    def solve(self, model: Model, mdp_solution: Union[ValueFunction, None] = None, use_gpu: bool = False,
              history_tracking_level: int = 1, print_progress: bool = True):
        """Sweeps from ``q0[a] = max over the rows of mdp_solution`` for every a (``VI_Solver`` runs when none is given):
        the first sweep then reproduces the MDP rows and every later one can only lower them.  The start reads the
        maximum over the rows, so it does not depend on how ``ValueFunction`` folded equal rows.  The change limit is
        ``eps * gamma / (1 - gamma)`` as in ``VI_Solver``.  ``use_gpu=True`` runs ``pbvi_fib_value_iteration`` and raises when
        the HIP library or the GPU is missing."""
        from .mdp import SolverHistory as MDP_SolverHistory
        host = model.cpu_model
        if mdp_solution is None:
            # (device VI sweeps are bit-identical to the host's for R = 1 only, PBVI_Solver.solve: keep one start for both)
            mdp_solution, _ = VI_Solver(horizon=self.horizon, gamma=self.gamma, eps=self.eps).solve(
                model, use_gpu=use_gpu and host.reachable_state_count == 1, print_progress=False)
        mdp_rows = (mdp_solution.to_cpu() if mdp_solution.is_on_gpu else mdp_solution).alpha_vector_array
        rows = np.tile(np.max(np.asarray(mdp_rows, dtype=np.float64), axis=0), (host.action_count, 1))
        V = ValueFunction(host, rows, host.actions)
        hist = MDP_SolverHistory(history_tracking_level, host, self.gamma, self.eps, V)
        limit = self.eps * (self.gamma / (1 - self.gamma))
        if use_gpu:
            from .engine import fib_value_iteration          # raises if the HIP library is missing
            rs, rto, er = _fib_tables(host)

            def run(q, n):
                return fib_value_iteration(rs, rto, er, q, self.gamma, limit, n)
        else:
            def run(q, n):
                return fib_numpy(host, q, self.gamma, limit, n)
        return _run_sweeps(run, host, V, rows, self.horizon, limit, hist), hist


# --------------------------------------------------------------------------- #
# Finite-state controllers (policy graphs) and the blind-policy lower bound (Hauskrecht 1997): the definition
# ``pbvi_controller_value_iteration`` implements, restated with NumPy
# --------------------------------------------------------------------------- #
def controller_numpy(model, node_action, node_succ, v0, gamma: float, max_change_limit: float, horizon: int):
    """Jacobi sweeps of the value of a finite-state controller from ``v0 [N,S]``.  Node n takes action
    ``a = node_action[n]`` and moves to node ``node_succ[n][o]`` on observation o:

        V'[n][s] = ER[s,a] + gamma * sum_o sum_r RTO[s,a,o,r] * V[node_succ[n][o]][rs[s,a,r]]

    All of V' is computed from the old V, until ``max_{n,s} |V' - V| < max_change_limit`` or ``horizon`` sweeps; returns
    ``(rows [N,S], changes)``, the rows of the last sweep that ran (``v0`` for ``horizon = 0``).  The loops over o and r are
    explicit so that every sum associates as the device kernel's does -- ``acc = t_0``, then ``acc = acc + t_r``;
    ``tot = acc_0``, then ``tot = tot + acc_o`` -- and the two agree bit for bit on finite inputs.  The tables are read per
    node through the action-major layout the kernel reads; working memory is a few ``[N,S]`` planes."""
    rs, rto, er = _fib_tables(model)
    S, A, O, R = rto.shape
    na = np.asarray(node_action, dtype=np.int64)
    ns = np.asarray(node_succ, dtype=np.int64)
    V = np.array(v0, dtype=np.float64, order='C')
    if rs.shape != (S, A, R) or er.shape != (S, A):
        raise ValueError('controller_numpy: table shapes do not agree')
    N = na.shape[0] if na.ndim == 1 else -1
    if N <= 0 or ns.shape != (N, O) or V.shape != (N, S):
        raise ValueError('controller_numpy: node_action must be [N], node_succ [N,O] and v0 [N,S]')
    if na.min() < 0 or na.max() >= A or ns.min() < 0 or ns.max() >= N:
        raise ValueError('controller_numpy: node action or successor node out of range')
    rs_t = np.ascontiguousarray(rs.transpose(1, 2, 0))                     # [A,R,S]
    rto_t = np.ascontiguousarray(rto.transpose(1, 2, 3, 0))                # [A,O,R,S]
    er_n = np.ascontiguousarray(er.T)[na]                                  # [N,S]
    to = [rs_t[na, r] for r in range(R)]                                   # [N,S] each: the landing state of (n, s, r)
    changes = []
    for _ in range(int(horizon)):
        tot = None
        for o in range(O):
            succ = ns[:, o][:, None]                                       # [N,1]
            acc = None
            for r in range(R):
                t = rto_t[na, o, r] * V[succ, to[r]]                       # [N,S]
                acc = t if acc is None else acc + t
            tot = acc if tot is None else tot + acc
        new = er_n + gamma * tot
        change = float(np.max(np.abs(new - V)))
        V = new
        changes.append(change)
        if change < max_change_limit:
            break
    return V, np.array(changes, dtype=np.float64)


def pessimistic_start(model, gamma: float, n_nodes: int):
    """The constant ``min(ER) / (1 - gamma)`` as ``[n_nodes, S]``: what the worst reward for ever is worth, below the value
    of every controller.  From it the sweeps of ``controller_numpy`` rise monotonically (the sweep is monotone and the first
    one does not go down), so a run stopped anywhere is still below the controller's true value: a valid lower bound at
    any horizon.  The mirror image of ``FIB_Solver``'s start from the MDP solution, from which the sweeps fall."""
    _, _, er = _fib_tables(model)
    return np.full((int(n_nodes), er.shape[0]), float(er.min()) / (1.0 - gamma), dtype=np.float64)


def evaluate_controller(model, node_action, node_succ, gamma: float = 0.99, eps: float = 0.001, horizon: int = 10000,
                        v0=None, use_gpu: bool = False):
    """The value of a finite-state controller: ``(rows [N,S], changes)``, row n the value of starting the controller in
    node n, every row a valid alpha-vector.  Sweeps from ``v0`` (``pessimistic_start`` when none is given) until the change
    is below ``eps * gamma / (1 - gamma)``, as in ``VI_Solver`` and ``FIB_Solver``, or ``horizon`` sweeps; on the device
    (``pbvi_controller_value_iteration``) when ``use_gpu``, which raises when the HIP library or the GPU is missing, else
    with ``controller_numpy`` -- the same rows bit for bit.  The rows come back raw, not as a ``ValueFunction``: that would
    fold byte-equal rows and lose which node a row belongs to."""
    node_action = np.asarray(node_action)
    if v0 is None:
        v0 = pessimistic_start(model, gamma, node_action.shape[0])
    limit = eps * (gamma / (1 - gamma))
    if use_gpu:
        from .engine import controller_value_iteration          # raises if the HIP library is missing
        rs, rto, er = _fib_tables(model)
        return controller_value_iteration(rs, rto, er, node_action, node_succ, v0, gamma, limit, horizon)
    return controller_numpy(model, node_action, node_succ, v0, gamma, limit, horizon)


class Blind_Solver(Solver):
    """The blind-policy lower bound (Hauskrecht 1997) as a solver: row a is the value of taking action a for ever, the
    controller with one node per action that is its own successor under every observation.  Each row is the value of a
    policy that can be run, so the A action-labelled rows are a valid lower bound of the POMDP value whatever the sign of
    the rewards -- the initial value function HSVI and SARSOP start from (``HSVI_Solver(lower_init='blind')``) -- and run
    through ``ValueFunction``, ``Agent`` and rollouts like any solution."""

    def __init__(self, horizon: int = 10000, gamma: float = 0.99, eps: float = 0.001):
        self.horizon = horizon
        self.gamma = gamma
        self.eps = eps

    def solve(self, model: Model, use_gpu: bool = False, history_tracking_level: int = 1, print_progress: bool = True):
        """Sweeps from ``pessimistic_start``, so the rows rise and are below the blind policies' values wherever the run
        stops.  The change limit is ``eps * gamma / (1 - gamma)`` as in ``VI_Solver``.  ``use_gpu=True`` runs
        ``pbvi_controller_value_iteration`` and raises when the HIP library or the GPU is missing."""
        from .mdp import SolverHistory as MDP_SolverHistory
        host = model.cpu_model
        A = host.action_count
        node_action = np.arange(A)
        node_succ = np.tile(np.arange(A)[:, None], (1, len(host.observations)))
        rows = pessimistic_start(host, self.gamma, A)
        V = ValueFunction(host, rows, host.actions)
        hist = MDP_SolverHistory(history_tracking_level, host, self.gamma, self.eps, V)
        limit = self.eps * (self.gamma / (1 - self.gamma))

        def run(rows, n):
            return evaluate_controller(host, node_action, node_succ, gamma=self.gamma, eps=self.eps, horizon=n, v0=rows,
                                       use_gpu=use_gpu)
        return _run_sweeps(run, host, V, rows, self.horizon, limit, hist), hist


# --------------------------------------------------------------------------- #
# Policy evaluation: simulators and the agent
# --------------------------------------------------------------------------- #
class SimulationHistory(MDP_SimulationHistory):
    """Episode record with observations and beliefs (``src/pomdp.py:2581-2662``).  The belief sequence is rebuilt
    on demand from the (action, observation) pairs when it was not recorded step by step."""

    def __init__(self, model: Model, start_state: int, start_belief: Belief):
        super().__init__(model, start_state)
        self._beliefs = [start_belief]
        self.observations = []
        self.lost = False          # run against an environment: stopped at an observation the model gives probability 0

    @property
    def beliefs(self) -> list:
        if len(self._beliefs) < len(self):
            b = self._beliefs[0]
            self._beliefs = [b]
            for a, o in zip(self.actions, self.observations):
                b = b.update(int(a), int(o))
                self._beliefs.append(b)
        return self._beliefs

    def add(self, action: int, reward, next_state: int, next_belief: Belief, observation: int) -> None:
        super().add(action, reward, next_state)
        self._beliefs.append(next_belief)
        self.observations.append(observation)

    def to_dataframe(self, include_beliefs: bool = False):
        """The MDP columns plus ``Observations`` and, on request, one ``B_<state>`` column per state
        (``src/pomdp.py:2664-2686``)."""
        import pandas as pd
        df = super().to_dataframe()
        df['Observations'] = list(self.observations) + [None]
        if include_beliefs:
            rows = np.array([b.values.tolist() for b in self.beliefs])
            df = pd.concat([df, pd.DataFrame(rows, columns=[f'B_{sl}' for sl in self.model.state_labels])], axis=1)
        return df

    def save(self, path: str = './Simulations', file_name: Union[str, None] = None, include_beliefs: bool = False) -> None:
        target = self._csv_target(path, file_name)
        if not include_beliefs:
            print('[Warning] Beliefs not saved with simulation history but the belief sequence can be recreated from '
                  'the actions and observations.')
        self.to_dataframe(include_beliefs=include_beliefs).to_csv(target, index=False)
        print(f'Saved to: {target}')


class Simulation(MDP_Simulation):
    """One hidden-state walk with observations (``src/pomdp.py:2756-2815``)."""

    def __init__(self, model: Model) -> None:
        super().__init__(model)
        self.model = model

    def run_action(self, a: int) -> Tuple[Union[int, float], int]:
        assert not self.is_done, "Action run when simulation is done."
        s = self.agent_state
        s_p = self.model.transition(s, a)
        o = self.model.observe(s_p, a)
        r = self.model.reward(s, a, s_p, o)
        self.agent_state = s_p
        self._mark_done(s_p, a)
        return r, o


class SimulationSet:
    """n hidden-state walks advanced together (``src/pomdp.py:2818-2945``).  The random draws are NumPy's global
    stream in the reference's call order (start states: one ``choice``; per step: one ``choice`` per
    simulation when R > 1, then one ``random(n)``), so a seeded run reproduces the reference's trajectories.

    ``reference_indexing``: for R > 1 the reference picks the successor with ``potentials[chosen][:, 0, 0]``
    (``:2928``), i.e. row ``chosen[i]`` column 0 rather than row ``i`` column ``chosen[i]``.  The default keeps
    that behaviour for parity; set it to False to sample ``rs[s_i, a_i, chosen_i]``.
    """

    reference_indexing = True

    def __init__(self, model: Model):
        self.model = model
        self.n = -1
        self.agent_states = [-1]
        self.simulations = []
        self.is_done = [True]

    def initialize_simulations(self, n: int = 1, start_state: Union[list, int, None] = None) -> np.ndarray:
        if isinstance(start_state, int):
            states = (np.ones(n) * start_state).astype(int)
        elif isinstance(start_state, list):
            rep = np.repeat(np.array(start_state), int(np.ceil(n / len(start_state))))
            states = np.resize(rep, n)
        else:
            states = np.random.choice(self.model.states, size=n, p=self.model.start_probabilities).astype(int)
        self.n = n
        self.agent_states = states
        self.simulations = np.arange(n)
        self.is_done = np.zeros(n, dtype=bool)
        return self.agent_states

    def _step_rewards(self, s, a, s_p, o) -> np.ndarray:
        m = self.model
        if m.immediate_reward_table is not None:
            return np.asarray(m.immediate_reward_table[s, a, s_p, o])
        fn = m.immediate_reward_function
        if getattr(fn, '__func__', None) is Model._end_reward_function:      # element-wise by construction
            return np.asarray(fn(s, a, s_p, o))
        return np.array([fn(int(w), int(x), int(y), int(z)) for w, x, y, z in zip(s, a, s_p, o)])

    def run_actions(self, actions: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        m = self.model
        actions = np.asarray(actions)
        potentials = m.reachable_states[self.agent_states, actions]                 # [n, R]
        if m.reachable_state_count == 1:
            next_states = potentials[:, 0]
        else:
            probs = m.reachable_probabilities[self.agent_states, actions]            # [n, R]
            chosen = np.apply_along_axis(lambda x: np.random.choice(len(x), size=1, p=x), axis=1, arr=probs)
            if self.reference_indexing:
                next_states = potentials[chosen][:, 0, 0]
            else:
                next_states = potentials[np.arange(self.n), chosen[:, 0]]
        obs_p = m.observation_table[next_states, actions]                            # [n, O]
        observations = np.sum(np.random.random(self.n)[:, None] > np.cumsum(obs_p[:, :-1], axis=1), axis=1)
        step_rewards = self._step_rewards(self.agent_states, actions, next_states, observations)
        rewards = np.where(~self.is_done, step_rewards, 0)
        self.is_done |= np.isin(next_states, np.array(m.end_states))
        self.agent_states = next_states
        return rewards, observations


def _q_values_numpy(model: Model, b: np.ndarray, alpha: np.ndarray, gamma: float) -> np.ndarray:
    """``Q[b,a] = b.ER[:,a] + gamma * sum_o max_v b.Gamma[a,o,v]`` in the array statements of the host backup."""
    V = alpha.shape[0]
    alpha_r = alpha[np.arange(V)[:, None, None, None], model.reachable_states[None, :, :, :]]
    gamma_aovs = gamma * np.einsum('saor,vsar->aovs', model.reachable_transitional_observation_table, alpha_r)
    scores = np.tensordot(b, gamma_aovs, (1, 3))                                   # [B,A,O,V]
    return np.matmul(b, model.expected_rewards_table) + np.sum(np.max(scores, axis=3), axis=2)


def _q_values_device(value_function: ValueFunction, arr: np.ndarray, gamma: float):
    """``(Q [B,A], argmax_a Q [B])`` from the HIP engine, ``_DeviceBeliefBlock.CHUNK`` beliefs at a time."""
    eng = value_function.model.engine
    eng.sync_rows('alpha', value_function.alpha_vector_list, lambda v: v.values)
    qs, acts = [], []
    for i0 in range(0, arr.shape[0], _DeviceBeliefBlock.CHUNK):
        eng.set_beliefs(arr[i0:i0 + _DeviceBeliefBlock.CHUNK])
        q, a = eng.q_values_resident(gamma)
        qs.append(q)
        acts.append(a)
    if len(qs) == 1:
        return qs[0], acts[0]
    A = value_function.model.action_count
    return (np.concatenate(qs) if qs else np.zeros((0, A))), (np.concatenate(acts) if acts else np.zeros(0, dtype=np.int64))


# --------------------------------------------------------------------------- #
# Counter-based rollouts: the definition ``pbvi_rollout`` implements on the device, restated with NumPy
# --------------------------------------------------------------------------- #
def _rollout_tables(model):
    """The tables a rollout reads under ``Model``'s attribute names, from a ``Model`` or a ``synth.SynthModel`` (whose one
    end state is its goal)."""
    from types import SimpleNamespace
    if hasattr(model, 'reachable_transitional_observation_table'):
        m = model.cpu_model if getattr(model, 'is_on_gpu', False) else model
        return SimpleNamespace(state_count=m.state_count, action_count=m.action_count, observation_count=m.observation_count,
                               reachable_state_count=m.reachable_state_count, reachable_states=np.asarray(m.reachable_states),
                               reachable_transitional_observation_table=np.asarray(m.reachable_transitional_observation_table),
                               expected_rewards_table=np.asarray(m.expected_rewards_table),
                               end_states=np.asarray(m.end_states, dtype=np.int64))
    return SimpleNamespace(state_count=model.S, action_count=model.A, observation_count=model.O, reachable_state_count=model.R,
                           reachable_states=np.asarray(model.reachable_states),
                           reachable_transitional_observation_table=np.asarray(model.rto),
                           expected_rewards_table=np.asarray(model.expected_rewards),
                           end_states=np.asarray(getattr(model, 'end_states', [model.goal]), dtype=np.int64))


def rollout_uniform(seed: int, sim_ids, t) -> np.ndarray:
    """``u(i, t) = uniform01(splitmix64(seed, i), t)``: the one uniform of simulation ``i`` (global id) at step ``t``."""
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError('seed must fit an unsigned 64-bit integer')
    from . import synth
    return synth.uniform01(synth.splitmix64(int(seed), sim_ids), t)


def rollout_draw(rows: np.ndarray, u: np.ndarray) -> np.ndarray:
    """Index ``k`` drawn from each ``[O*R]`` row of weights with its uniform: the first ``k`` with ``u * c[-1] < c[k]``,
    ``c`` the sequential fp64 prefix sums; where rounding leaves none, the last ``k`` with a positive weight."""
    rows = np.asarray(rows, dtype=np.float64)
    c = np.cumsum(rows, axis=1)
    if not np.all(c[:, -1] > 0):
        raise ValueError('a row of RTO[s, a, :, :] sums to 0: nothing can follow that state-action pair')
    hit = (np.asarray(u, dtype=np.float64) * c[:, -1])[:, None] < c
    k = np.argmax(hit, axis=1)
    none = ~hit.any(axis=1)
    if none.any():
        k[none] = rows.shape[1] - 1 - np.argmax(rows[none, ::-1] > 0, axis=1)
    return k


def _rollout_inputs(model, beliefs, start_states, T: int, alpha=None, alpha_actions=None, one_message: bool = False):
    """The inputs every host rollout takes, validated: ``(tables, T, beliefs [n,S] fp64 (a copy), start states [n] int64, alpha
    [V,S] fp64, alpha_actions [V] int64)``, the last two ``None`` when no alpha set is given.  ``one_message``:
    ``rollout_numpy``'s wording for a wrong shape of ``beliefs`` or ``alpha``."""
    m = _rollout_tables(model)
    S, A = m.state_count, m.action_count
    T = int(T)
    if T < 1:
        raise ValueError('T must be at least 1')
    b = np.array(beliefs, dtype=np.float64)
    s = np.asarray(start_states).astype(np.int64)
    acts = None
    if alpha is not None:
        alpha = np.asarray(alpha, dtype=np.float64)
        acts = np.asarray(alpha_actions).astype(np.int64)
    n = b.shape[0]
    bad_b = b.ndim != 2 or b.shape[1] != S
    bad_alpha = alpha is not None and (alpha.ndim != 2 or alpha.shape[1] != S)
    if one_message and (bad_b or bad_alpha):
        raise ValueError(f'beliefs and alpha must be [*, {S}] arrays')
    if bad_b:
        raise ValueError(f'beliefs must be a [*, {S}] array')
    if s.shape != (n,) or (n and (s.min() < 0 or s.max() >= S)):
        raise ValueError('start_states must be [n] with entries in [0, S)')
    if bad_alpha:
        raise ValueError(f'alpha must be a [*, {S}] array')
    if alpha is not None and (acts.shape != (alpha.shape[0],) or acts.min() < 0 or acts.max() >= A):
        raise ValueError('alpha_actions must be [V] with entries in [0, A)')
    return m, T, b, s, alpha, acts


def rollout_numpy(model, alpha, alpha_actions, beliefs, start_states, seed: int, first_sim_id: int, T: int,
                  lookahead: int = 0, gamma: float = 0.99, table_dtype=np.float64, return_beliefs: bool = False):
    """``T`` lock-step simulation steps with counter-based draws, on the host: what ``pbvi_rollout`` computes on the device.

    Row ``b`` of ``beliefs`` is simulation ``first_sim_id + b``.  Per step and running simulation: the action
    (``alpha_actions[argmax_v b.alpha_v]``, or ``argmax_a Q(b,a)`` for ``lookahead=1``), one uniform
    ``rollout_uniform(seed, id, t)``, the ``(observation, successor)`` pair drawn from ``RTO[s, a, :, :]`` -- cast to
    ``table_dtype``, the engine's arithmetic type, and widened -- by ``rollout_draw``, the Bayes update
    (``_HostBeliefBlock.advance``) and the done-filter.  Returns ``(states [T+1,n], actions [T,n], observations [T,n],
    steps [n])`` as int32 arrays, ``-1`` behind a finished simulation's last step; with ``return_beliefs`` also the
    ``[n_running, S]`` beliefs of the simulations still running, in order.  A trajectory depends on its own row and id
    only, so a run cut into chunks (``first_sim_id`` advanced by the rows before) returns the same rows."""
    from types import SimpleNamespace
    if lookahead not in (0, 1):
        raise ValueError(f'lookahead must be 0 or 1, not {lookahead!r}')
    m, T, b, s, alpha, acts = _rollout_inputs(model, beliefs, start_states, T, alpha, alpha_actions, one_message=True)
    block = _HostBeliefBlock(m, SimpleNamespace(alpha_vector_array=alpha), b)
    choose = (lambda: block.best_actions(gamma)) if lookahead == 1 else (lambda: acts[block.best_vectors()])
    return _rollout_loop(m, block, choose, s, seed, first_sim_id, T, table_dtype, return_beliefs)


def _rollout_loop(m, block, choose, s, seed: int, first_sim_id: int, T: int, table_dtype, return_beliefs: bool,
                  observe=None, choose_draws: bool = False):
    """The step loop of the counter-based rollouts (``rollout_numpy``, ``rollout_infotaxis_numpy``, ``rollout_env_numpy``):
    ``choose()`` gives the actions of the beliefs ``block`` holds; the uniform, the done-filter and the Bayes step are the
    same for every policy.  ``m``: ``_rollout_tables``' tables, ``s``: the validated start states.  ``choose_draws``: the
    policy draws itself (Thompson) and is called as ``choose(t, ids)`` with the step and the running simulations' global ids.

    ``observe=None``: the ``(observation, successor)`` pair comes from the model's joint row ``RTO[s, a, :, :]`` and a belief
    is always normalised -- ``pbvi_rollout``'s step.  ``observe(t, rows, ids, a, sn, done)``: ``pbvi_rollout_env``'s step --
    the successor from the marginal ``w[r] = sum_o RTO[s, a, o, r]`` (``o`` ascending, sequential adds), the observation of
    the running simulations ``rows`` (global ids ``ids``) from the hook, and the lost rule (``advance_or_lose``); the
    return value then ends with ``lost [n]`` uint8."""
    S, A, O, R = m.state_count, m.action_count, m.observation_count, m.reachable_state_count
    n = s.shape[0]
    rto = np.ascontiguousarray(m.reachable_transitional_observation_table, dtype=table_dtype).astype(np.float64).reshape(S, A, O * R)
    if not np.all(np.cumsum(rto, axis=2)[:, :, -1] > 0):
        raise ValueError('a row of RTO[s, a, :, :] sums to 0: nothing can follow that state-action pair')
    if observe is not None:
        marginal = np.zeros((S, A, R))
        for o in range(O):
            marginal += rto[:, :, o * R:(o + 1) * R]
    end = np.zeros(S, dtype=bool)
    end[m.end_states] = True
    with np.errstate(over='ignore'):
        ids = np.uint64(int(first_sim_id)) + np.arange(n, dtype=np.uint64)
    states = np.full((T + 1, n), -1, dtype=np.int32)
    actions = np.full((T, n), -1, dtype=np.int32)
    observations = np.full((T, n), -1, dtype=np.int32)
    steps = np.full(n, T, dtype=np.int32)
    lost = np.zeros(n, dtype=np.uint8)
    states[0] = s
    alive = np.arange(n)
    for t in range(T):
        if alive.size == 0:
            break
        a = choose(t, ids[alive]) if choose_draws else choose()
        if observe is None:
            k = rollout_draw(rto[s, a], rollout_uniform(seed, ids[alive], t))
            o, sn = k // R, m.reachable_states[s, a, k % R]
            done = end[sn]
        else:
            sn = m.reachable_states[s, a, rollout_draw(marginal[s, a], rollout_uniform(seed, ids[alive], t))]
            done = end[sn]
            o = observe(t, alive, ids[alive], a, sn, done)
        states[t + 1, alive], actions[t, alive], observations[t, alive] = sn, a, o
        steps[alive[done]] = t + 1
        go = ~done
        if observe is None:
            block.advance(a, o, go)
        else:
            gone = block.advance_or_lose(a, o, go)
            steps[alive[gone]] = t + 1
            lost[alive[gone]] = 1
            go = go & ~gone
        alive, s = alive[go], sn[go]
    out = (states, actions, observations, steps)
    if return_beliefs:
        out += (block.b if alive.size else np.zeros((0, S)),)
    return out + (lost,) if observe is not None else out


# --------------------------------------------------------------------------- #
# Environments: the observation source of ``rollout_env_numpy`` / ``pbvi_rollout_env``
# --------------------------------------------------------------------------- #
class FrameEnvironment:
    """Recorded observations: ``frames[f, c, s]`` (uint8 ``[F, C, S]``) is the observation id emitted in frame ``f``, channel
    ``c``, at state ``s``; action ``a`` reads channel ``channel_of_action[a]``.  Simulation ``b`` reads frame
    ``shifts[b] + t`` at step ``t`` (``shifts``: one integer for all, or one per simulation).  ``end_observation >= 0``:
    the observation on landing in an end state, whatever the frame says.  A plain data holder: the reference's plume
    movies (``RealSimulationSetAlt``: nose and ground data, ``C = 2``) in the form the engine takes.  The frames are taken
    as immutable once the holder is built: they are scanned once, here (``largest``), a contiguous uint8 array is kept
    without a copy, and an engine that holds them does not upload them again -- build a new holder for edited frames."""

    def __init__(self, frames, channel_of_action, shifts=0, end_observation: int = -1):
        raw = np.asarray(frames)
        if raw.ndim != 3 or raw.shape[0] < 1 or raw.shape[1] < 1:
            raise ValueError('frames must be a [F, C, S] array with F, C >= 1')
        if raw.dtype != np.uint8 and (raw.min() < 0 or raw.max() > 255):
            raise ValueError('frame entries must fit one byte')
        self.frames = np.ascontiguousarray(raw, dtype=np.uint8)
        self.channel_of_action = np.ascontiguousarray(channel_of_action, dtype=np.int32)
        self.shifts = np.asarray(shifts, dtype=np.int64)
        self.end_observation = int(end_observation)
        self.largest = int(self.frames.max())                  # scanned once: check() is called per rollout
        C = self.frames.shape[1]
        if self.channel_of_action.ndim != 1 or self.channel_of_action.min() < 0 or self.channel_of_action.max() >= C:
            raise ValueError('channel_of_action must be [A] with entries in [0, C)')
        if self.shifts.ndim > 1 or (self.shifts.size and self.shifts.min() < 0):
            raise ValueError('shifts must be one non-negative integer or a [n] array of them')

    def check(self, S: int, A: int, O: int, n: int, T: int) -> np.ndarray:
        """Raises ``ValueError`` where ``pbvi_env_set_frames`` / ``pbvi_rollout_env`` refuse; returns the ``[n]`` shifts."""
        if O > 255:
            raise ValueError('frames hold one byte per observation, so O must be at most 255')
        if self.frames.shape[2] != S or self.channel_of_action.shape != (A,):
            raise ValueError(f'frames must be [F, C, {S}] and channel_of_action [{A}]')
        if self.largest >= O or self.end_observation >= O:
            raise ValueError(f'a frame entry (or end_observation) is not an observation in [0, {O})')
        if self.shifts.ndim == 1 and self.shifts.shape != (n,):
            raise ValueError(f'shifts must be one integer or [{n}]')
        sh = np.broadcast_to(self.shifts, (n,))
        if (int(sh.max()) if n else 0) + T > self.frames.shape[0]:
            raise ValueError(f'max(shift) + T exceeds the {self.frames.shape[0]} frames of the environment')
        return sh

    def rows(self, lo: int, hi: int) -> 'FrameEnvironment':
        """The environment of simulations ``lo:hi`` (the frames are shared, per-simulation shifts are sliced)."""
        import copy
        part = copy.copy(self)                                  # (no second scan of the frames)
        part.shifts = self.shifts[lo:hi] if self.shifts.ndim else self.shifts
        return part


class TableEnvironment:
    """Another observation law: ``obs_prob[s', a, :]`` (``[S, A, O]``, non-negative, every row with mass) is the law of the
    observation after landing in ``s'`` with action ``a`` -- the reference's ``SimulationSetAltProb``.
    ``end_observation >= 0``: the observation on landing in an end state."""

    def __init__(self, obs_prob, end_observation: int = -1):
        self.obs_prob = np.ascontiguousarray(obs_prob, dtype=np.float64)
        self.end_observation = int(end_observation)
        if self.obs_prob.ndim != 3:
            raise ValueError('obs_prob must be a [S, A, O] array')
        if not np.all(np.isfinite(self.obs_prob)) or self.obs_prob.min() < 0:
            raise ValueError('obs_prob has a negative or non-finite entry')
        if not np.all(np.cumsum(self.obs_prob, axis=2)[:, :, -1] > 0):
            raise ValueError('a row obs_prob[s, a, :] sums to 0')

    def check(self, S: int, A: int, O: int, n: int, T: int) -> None:
        if self.obs_prob.shape != (S, A, O):
            raise ValueError(f'obs_prob must be [{S}, {A}, {O}]')
        if self.end_observation >= O:
            raise ValueError(f'end_observation is not an observation in [0, {O})')

    def rows(self, lo: int, hi: int) -> 'TableEnvironment':
        return self


def record_frames(obs_table, F: int, seed: int) -> np.ndarray:
    """``F`` frames drawn from an observation table ``[S, A, O]``: uint8 ``[F, A, S]`` (one channel per action, so
    ``channel_of_action = arange(A)``) with ``frames[f, a, s]`` drawn from ``obs_table[s, a, :]`` by ``rollout_draw``'s prefix
    rule with the uniform ``synth.uniform01(seed, (f * A + a) * S + s)``.  A deterministic stand-in for an intermittent plume
    movie whose law is the model's own."""
    from . import synth
    tab = np.asarray(obs_table, dtype=np.float64)
    if tab.ndim != 3 or tab.shape[2] > 255:
        raise ValueError('obs_table must be [S, A, O] with O <= 255')
    F = int(F)
    if F < 1:
        raise ValueError('F must be at least 1')
    if not 0 <= int(seed) < 1 << 64:
        raise ValueError('seed must fit an unsigned 64-bit integer')
    S, A, O = tab.shape
    rows = np.ascontiguousarray(tab.transpose(1, 0, 2)).reshape(A * S, O)          # row a * S + s
    c = np.cumsum(rows, axis=1)
    if not np.all(c[:, -1] > 0):
        raise ValueError('a row obs_table[s, a, :] sums to 0')
    last_pos = O - 1 - np.argmax(rows[:, ::-1] > 0, axis=1)
    cell = np.arange(A * S, dtype=np.uint64)
    frames = np.empty((F, A, S), dtype=np.uint8)
    for f in range(F):
        u = synth.uniform01(int(seed), np.uint64(f * A * S) + cell)
        hit = (u * c[:, -1])[:, None] < c
        frames[f] = np.where(hit.any(axis=1), np.argmax(hit, axis=1), last_pos).reshape(A, S)
    return frames


ENV_POLICY_INFOTAXIS = 2               # ``rollout_env`` / ``pbvi_rollout_env`` number the policies: 0 value-max, 1 Q, 2 infotaxis


def rollout_env_numpy(model, env, policy: int, alpha, alpha_actions, beliefs, start_states, seed: int, first_sim_id: int,
                      T: int, gamma: float = 0.99, table_dtype=np.float64, return_beliefs: bool = False):
    """``T`` lock-step steps against an environment, on the host: what ``pbvi_rollout_env`` computes on the device.

    ``policy``: 0 ``alpha_actions[argmax_v b.alpha_v]``, 1 ``argmax_a Q(b, a)``, 2 infotaxis (``alpha`` and ``alpha_actions``
    may be ``None``).  Per step ``t`` and running simulation ``i`` in state ``s`` with action ``a``: the successor ``s'`` is
    drawn from ``w[r] = sum_o RTO[s, a, o, r]`` with ``u1 = rollout_uniform(seed, i, t)``; the observation is
    ``env.end_observation`` on landing in an end state when that is ``>= 0``, else ``frames[shift_i + t, channel[a], s']``
    (``FrameEnvironment``) or drawn from ``obs_prob[s', a, :]`` with the second uniform ``u2 = rollout_uniform(seed, i,
    2**32 + t)`` (``TableEnvironment``); an end state finishes the simulation; otherwise a Bayes step whose un-normalised
    mass is 0 or not finite -- an observation impossible under the model -- stops it as LOST at this step (``steps = t + 1``,
    recorded ``a``, ``o``, ``s'``, no NaN belief), and any other is normalised.  ``env.shifts`` belong to the rows given.
    Returns ``rollout_numpy``'s arrays and then ``lost [n]`` uint8."""
    from types import SimpleNamespace
    if policy not in (0, 1, ENV_POLICY_INFOTAXIS):
        raise ValueError(f'policy must be 0 (value-max), 1 (Q) or 2 (infotaxis), not {policy!r}')
    if not isinstance(env, (FrameEnvironment, TableEnvironment)):
        raise ValueError('env must be a FrameEnvironment or a TableEnvironment')
    if int(T) >= 1 << 31:
        raise ValueError('T must be below 2**31')
    infotaxis = policy == ENV_POLICY_INFOTAXIS
    m, T, b, s, alpha, acts = _rollout_inputs(model, beliefs, start_states, T,
                                              None if infotaxis else np.asarray(alpha, dtype=np.float64), alpha_actions)
    if infotaxis:
        block = _HostBeliefBlock(m, None, b)
        choose = lambda: block.infotaxis_actions(table_dtype)
    else:
        block = _HostBeliefBlock(m, SimpleNamespace(alpha_vector_array=alpha), b)
        choose = (lambda: block.best_actions(gamma)) if policy == 1 else (lambda: acts[block.best_vectors()])
    return _rollout_env_loop(m, env, block, choose, s, seed, first_sim_id, T, table_dtype, return_beliefs)


def _rollout_env_loop(m, env, block, choose, s, seed: int, first_sim_id: int, T: int, table_dtype, return_beliefs: bool,
                      choose_draws: bool = False):
    """``_rollout_loop`` against ``env``, for whatever policy ``choose`` is (``rollout_env_numpy``,
    ``rollout_space_aware_numpy``): the environment's checks, then the observation hook -- the frame of the simulation's
    shift, or a draw from the table's row with the second uniform; ``env.end_observation`` on landing in an end state."""
    shifts = env.check(m.state_count, m.action_count, m.observation_count, s.shape[0], T)
    end_obs = env.end_observation

    def observe(t, rows, ids, a, sn, done):
        if isinstance(env, FrameEnvironment):
            o = env.frames[shifts[rows] + t, env.channel_of_action[a], sn].astype(np.int64)
        else:
            o = rollout_draw(env.obs_prob[sn, a], rollout_uniform(seed, ids, (1 << 32) + t))
        return np.where(done, end_obs, o) if end_obs >= 0 else o

    return _rollout_loop(m, block, choose, s, seed, first_sim_id, T, table_dtype, return_beliefs, observe, choose_draws)


# --------------------------------------------------------------------------- #
# Infotaxis: the action with the smallest expected entropy of the next belief (what ``pbvi_infotaxis`` computes)
# --------------------------------------------------------------------------- #
def _xlogx(x: np.ndarray) -> np.ndarray:
    """``x * ln x`` element by element, 0 where ``x == 0``."""
    out = np.zeros_like(x, dtype=np.float64)
    nz = x != 0
    with np.errstate(invalid='ignore', divide='ignore'):
        out[nz] = x[nz] * np.log(x[nz])
    return out


def _successor_terms(model, beliefs, weights=None, table_dtype=np.float64, rows_at_once: Union[int, None] = None):
    """The sums over the un-normalised successor ``u`` (``_successor_rows``: ``np.bincount``'s order; the table cast to
    ``table_dtype``, the engine's number format, and widened) that the greedy successor policies are made of, and the checks of
    their arguments: ``(b [n,S] fp64, Z, N, M_N, D)``, the last four ``[n,A,O]``:

        ``Z = sum_s' u``,   ``N = sum_s' u ln u``,   ``M_N = sum_s' |u ln u|``,   ``D = sum_s' u w``     (``u == 0`` adds 0)

    ``D`` is ``None`` without ``weights``.  ``rows_at_once`` beliefs are expanded at a time (by default ~32 MiB of products)."""
    m = _rollout_tables(model)
    S, A, O, R = m.state_count, m.action_count, m.observation_count, m.reachable_state_count
    b = np.asarray(beliefs, dtype=np.float64)
    if b.ndim != 2 or b.shape[1] != S:
        raise ValueError(f'beliefs must be a [*, {S}] array')
    w = None if weights is None else _state_weights(S, weights)
    n = b.shape[0]
    rto = np.ascontiguousarray(m.reachable_transitional_observation_table, dtype=table_dtype).astype(np.float64)
    rs = np.asarray(m.reachable_states).astype(np.int64)
    Z, N, MN = (np.zeros((n, A, O)) for _ in range(3))
    D = None if w is None else np.zeros((n, A, O))
    step = max(1, (1 << 22) // (S * R)) if rows_at_once is None else int(rows_at_once)
    for i0 in range(0, n, step):
        i1 = min(i0 + step, n)
        for a, o, u in _successor_rows(b[i0:i1], rs, rto):
            ulu = _xlogx(u)
            Z[i0:i1, a, o] = np.sum(u, axis=1)
            N[i0:i1, a, o] = np.sum(ulu, axis=1)
            MN[i0:i1, a, o] = np.sum(np.abs(ulu), axis=1)
            if w is not None:
                D[i0:i1, a, o] = np.sum(u * w[None, :], axis=1)
    return b, Z, N, MN, D


def _infotaxis_terms(model, beliefs, table_dtype=np.float64, rows_at_once: Union[int, None] = None):
    """The sums of ``infotaxis_numpy`` and the magnitudes of their terms: ``(G [n,A], Z [n,A,O], H [n], M_G [n,A], M_H [n])``
    with ``M_G = sum_o (|Z ln Z| + sum_s' |u ln u|)`` and ``M_H = sum_s |b ln b|`` (what a rounding-error bound for a
    re-ordered evaluation of ``G`` and ``H`` scales with).  ``G`` and ``M_G`` start from zero and take one term per observation,
    in the order of the observations."""
    b, Z, N, MN, _ = _successor_terms(model, beliefs, None, table_dtype, rows_at_once)
    G, MG = np.zeros(Z.shape[:2]), np.zeros(Z.shape[:2])
    for o in range(Z.shape[2]):
        zlz = _xlogx(Z[:, :, o])
        G += zlz - N[:, :, o]
        MG += np.abs(zlz) + MN[:, :, o]
    blb = _xlogx(b)
    return G, Z, -np.sum(blb, axis=1), MG, np.sum(np.abs(blb), axis=1)


def infotaxis_first_argmin(G: np.ndarray) -> np.ndarray:
    """The first action whose ``G`` is strictly smaller than every earlier one; a NaN never wins, a row of NaNs gives 0."""
    return np.argmin(np.where(np.isnan(G), np.inf, G), axis=1)


def infotaxis_numpy(model, beliefs, table_dtype=np.float64):
    """Expected entropy of the next belief for every row of ``beliefs [n,S]`` and every action, on the host: what
    ``pbvi_infotaxis`` computes on the device.  With ``u[s'] = sum_{(s,r): rs[s,a,r] = s'} b[s] RTO[s,a,o,r]`` (``np.bincount``,
    the un-normalised ``Belief.update``; the table cast to ``table_dtype``, the engine's number format, and widened),
    ``Z[a,o] = sum_s' u`` and ``N[a,o] = sum_s' u ln u``:

        ``G[b,a] = sum_o (Z ln Z - N) = sum_o P(o|b,a) H(update(b,a,o))``   (nats; zero terms add 0)

    Returns ``(G [n,A], action [n], p_obs [n,A,O], entropy [n])``: ``action`` is ``infotaxis_first_argmin(G)``, ``p_obs`` is
    ``Z`` and ``entropy[b] = -sum_s b[s] ln b[s]``, the entropy of the belief itself."""
    G, Z, H, _, _ = _infotaxis_terms(model, beliefs, table_dtype)
    return G, infotaxis_first_argmin(G), Z, H


def rollout_infotaxis_numpy(model, beliefs, start_states, seed: int, first_sim_id: int, T: int, table_dtype=np.float64,
                            return_beliefs: bool = False):
    """``rollout_numpy`` with the infotaxis policy, on the host: what ``pbvi_rollout_infotaxis`` computes on the device.
    Per step and running simulation the action is ``infotaxis_numpy(model, b, table_dtype)``'s; the uniform, the draw, the
    Bayes update, the done-filter and the return value are ``rollout_numpy``'s."""
    m, T, b, s, _, _ = _rollout_inputs(model, beliefs, start_states, T)
    block = _HostBeliefBlock(m, None, b)
    return _rollout_loop(m, block, lambda: block.infotaxis_actions(table_dtype), s, seed, first_sim_id, T, table_dtype,
                         return_beliefs)


# --------------------------------------------------------------------------- #
# Space-aware infotaxis (Loisy & Eloy 2022): greedy for J = log2(D + 2^(H-1) - 1/2) of the next belief, D its expected
# distance to the source and H its entropy in bits (what ``pbvi_space_aware`` computes)
# --------------------------------------------------------------------------- #
SPACE_AWARE_OBJECTIVES = {'space_aware': 0, 'expected_weight': 1}


def _state_weights(S: int, weights) -> np.ndarray:
    """``weights`` as the engine takes them: ``[S]`` fp64, every entry finite and ``>= 0``."""
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (S,):
        raise ValueError(f'weights must be [{S}]')
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError('weights must be finite and >= 0')
    return w


def _space_aware_objective(objective) -> int:
    objective = SPACE_AWARE_OBJECTIVES.get(objective, objective)
    if isinstance(objective, bool) or objective not in (0, 1):
        raise ValueError(f"objective must be 0 / 'space_aware' or 1 / 'expected_weight', not {objective!r}")
    return int(objective)


def manhattan_to_end_states(model) -> np.ndarray:
    """``w [S]``: for every state the smallest ``|d row| + |d col|`` on ``model.state_grid`` to any end state -- the distance
    space-aware infotaxis uses.  Wrap-around is ignored: on a grid whose moves wrap, the distance is still measured inside
    the rectangle.  ``ValueError`` without end states, or with a state that is not on the grid."""
    m = model.cpu_model if getattr(model, 'is_on_gpu', False) else model
    S = int(m.state_count)
    ends = np.asarray(m.end_states, dtype=np.int64).ravel()
    if ends.size == 0:
        raise ValueError('the model has no end states: there is nothing to measure a distance to')
    grid = np.asarray(m.state_grid)
    pos = np.full((S, 2), -1, dtype=np.int64)
    rows, cols = np.indices(grid.shape)
    on = (grid >= 0) & (grid < S)
    pos[grid[on], 0], pos[grid[on], 1] = rows[on], cols[on]
    if np.any(pos < 0):
        raise ValueError('every state must have a cell on state_grid')
    best = np.full(S, np.iinfo(np.int64).max, dtype=np.int64)
    step = max(1, (1 << 22) // S)                                 # [S, step] int64 at a time: ~32 MiB
    for i0 in range(0, ends.size, step):
        e = pos[ends[i0:i0 + step]]
        dist = np.abs(pos[:, None, 0] - e[None, :, 0]) + np.abs(pos[:, None, 1] - e[None, :, 1])
        best = np.minimum(best, dist.min(axis=1))
    return best.astype(np.float64)


def space_aware_terms(model, beliefs, weights, table_dtype=np.float64, rows_at_once: Union[int, None] = None):
    """The three sums ``pbvi_space_aware`` forms per (belief, action, observation), on the host, and the magnitudes of their
    terms: ``(Z, N, D, M_Z, M_N, M_D)``, each ``[n,A,O]``.  With ``u`` the un-normalised successor of ``infotaxis_numpy``
    (``_successor_rows``: ``np.bincount``'s order; the table cast to ``table_dtype`` and widened):

        ``Z = sum_s' u``,   ``N = sum_s' u ln u``,   ``D = sum_s' u w``        (``u == 0`` adds 0)

    ``M_Z = Z``, ``M_N = sum_s' |u ln u|`` and ``M_D = D`` (the terms of ``Z`` and ``D`` are non-negative) are what a
    rounding-error bound for a re-ordered evaluation of each sum scales with."""
    # (``None`` is no weight vector here: as an array it has no shape ``[S]``, and is refused as one)
    _, Z, N, MN, D = _successor_terms(model, beliefs, np.asarray(weights, dtype=np.float64), table_dtype, rows_at_once)
    return Z, N, D, Z, MN, D


def space_aware_j(Z, N, D) -> np.ndarray:
    """``J = log2(max(1, D/Z + (exp(H) - 1)/2))`` with ``H = max(0, ln Z - N/Z)``, element by element; 0 where ``Z == 0``.
    Both clamps are part of the definition (``max`` as C's ``fmax``): rounding can leave ``ln Z - N/Z`` slightly negative,
    and a successor known to sit on the source has ``J = 0``."""
    Z, N, D = (np.asarray(x, dtype=np.float64) for x in (Z, N, D))
    ok = Z != 0
    J = np.zeros(Z.shape)
    with np.errstate(all='ignore'):
        z, nn, d = Z[ok], N[ok], D[ok]
        H = np.fmax(0.0, np.log(z) - nn / z)
        J[ok] = np.log2(np.fmax(1.0, d / z + (np.exp(H) - 1.0) * 0.5))
    return J


def space_aware_from_terms(Z, N, D, objective=0) -> np.ndarray:
    """``F [..., A]`` from the terms ``[..., A, O]``: objective 0 ``sum_o Z J`` (``space_aware_j``), objective 1 ``sum_o D``;
    both sums sequential over ``o``, an observation with ``Z == 0`` adds 0."""
    objective = _space_aware_objective(objective)
    Z, D = np.asarray(Z, dtype=np.float64), np.asarray(D, dtype=np.float64)
    with np.errstate(all='ignore'):
        terms = np.where(Z != 0, D if objective == 1 else Z * space_aware_j(Z, N, D), 0.0)
    F = np.zeros(Z.shape[:-1])
    for o in range(Z.shape[-1]):
        F = F + terms[..., o]
    return F


def space_aware_numpy(model, beliefs, weights, objective=0, table_dtype=np.float64):
    """Space-aware infotaxis for every row of ``beliefs [n,S]`` and every action, on the host: what ``pbvi_space_aware``
    computes on the device.  ``weights [S]``: finite, ``>= 0`` -- the distance of every state to the source.  Per (a, o), with
    ``space_aware_terms``' sums, ``H = max(0, ln Z - N/Z)`` is the entropy of the successor belief (nats) and ``D/Z`` its
    expected weight;

        objective 0 / ``'space_aware'``:      ``F[b,a] = sum_o Z log2(max(1, D/Z + (exp(H) - 1)/2))``
        objective 1 / ``'expected_weight'``:  ``F[b,a] = sum_o D``

    Returns ``(F [n,A], action [n], terms [n,A,O,3])``: ``action`` is ``infotaxis_first_argmin(F)``, ``terms`` holds
    ``(Z, N, D)``."""
    Z, N, D, _, _, _ = space_aware_terms(model, beliefs, weights, table_dtype)
    F = space_aware_from_terms(Z, N, D, objective)
    return F, infotaxis_first_argmin(F), np.stack([Z, N, D], axis=-1)


def rollout_space_aware_numpy(model, beliefs, start_states, weights, seed: int, first_sim_id: int, T: int, objective=0,
                              table_dtype=np.float64, return_beliefs: bool = False, env=None):
    """``rollout_numpy`` with the space-aware policy, on the host: what ``pbvi_rollout_space_aware`` computes on the device.
    Per step and running simulation the action is ``space_aware_numpy(model, b, weights, objective, table_dtype)``'s.
    ``env=None``: the model's world -- the uniform, the draw, the Bayes update, the done-filter and the return value are
    ``rollout_numpy``'s.  ``env`` (a ``FrameEnvironment`` or ``TableEnvironment``): the successor draw, the observation, the
    lost rule and the return value (``lost [n]`` last) are ``rollout_env_numpy``'s."""
    objective = _space_aware_objective(objective)
    if env is not None:
        if not isinstance(env, (FrameEnvironment, TableEnvironment)):
            raise ValueError('env must be a FrameEnvironment or a TableEnvironment')
        if int(T) >= 1 << 31:
            raise ValueError('T must be below 2**31')
    m, T, b, s, _, _ = _rollout_inputs(model, beliefs, start_states, T)
    w = _state_weights(m.state_count, weights)
    block = _HostBeliefBlock(m, None, b)
    choose = lambda: block.space_aware_actions(w, objective, table_dtype)
    if env is None:
        return _rollout_loop(m, block, choose, s, seed, first_sim_id, T, table_dtype, return_beliefs)
    return _rollout_env_loop(m, env, block, choose, s, seed, first_sim_id, T, table_dtype, return_beliefs)


# --------------------------------------------------------------------------- #
# State policies: most likely state, action voting, Thompson sampling (what ``pbvi_state_policy`` computes).  All three act
# through a policy of the underlying MDP, ``state_actions [S]``.  The sums are sequential fp64 walks over chunks of 256
# states, combined in chunk order (``include/pbvi_hip.h``), so host and device agree bit for bit.
# --------------------------------------------------------------------------- #
STATE_POLICY_RULES = {'mls': 0, 'voting': 1, 'thompson': 2}
STATE_POLICY_CHUNK = 256
THOMPSON_STREAM = 1 << 33                # Thompson's counter is 2^33 + t: beside the draws' t and 2^32 + t


def _state_policy_rule(rule) -> int:
    r = STATE_POLICY_RULES.get(rule, rule) if isinstance(rule, str) else rule
    if isinstance(r, bool) or r not in (0, 1, 2):
        raise ValueError(f"rule must be 0 / 'mls', 1 / 'voting' or 2 / 'thompson', not {rule!r}")
    return int(r)


def _state_actions(S: int, A: int, state_actions) -> np.ndarray:
    sa = np.asarray(state_actions)
    if sa.shape != (S,) or not np.issubdtype(sa.dtype, np.integer) or (S and (sa.min() < 0 or sa.max() >= A)):
        raise ValueError('state_actions must be [S] integers in [0, A)')
    return sa.astype(np.int64)


def state_actions_from(value_function) -> np.ndarray:
    """The state policy of an action-labelled solution (``VI_Solver`` or ``FIB_Solver``): ``actions[first argmax_v
    alpha_v[s]]`` for every state ``s``, ``[S]`` int64."""
    vf = value_function.to_cpu() if getattr(value_function, 'is_on_gpu', False) else value_function
    alpha = np.asarray(vf.alpha_vector_array, dtype=np.float64)
    return np.asarray(vf.actions, dtype=np.int64)[np.argmax(alpha, axis=0)]


def _chunked(beliefs: np.ndarray) -> np.ndarray:
    """``beliefs [n,S]`` as ``[n, C, 256]`` fp64, the last chunk filled with ``+0.0`` (which adds nothing to a sum)."""
    b = np.asarray(beliefs, dtype=np.float64)
    n, S = b.shape
    C = -(-S // STATE_POLICY_CHUNK)
    out = np.zeros((n, C * STATE_POLICY_CHUNK))
    out[:, :S] = b
    return out.reshape(n, C, STATE_POLICY_CHUNK)


def _first_greater(x: np.ndarray) -> np.ndarray:
    """The first index of each row whose entry is strictly greater than every earlier one; a NaN never wins."""
    return np.argmax(np.where(np.isnan(x), -np.inf, x), axis=1)


def thompson_state_numpy(beliefs, u) -> np.ndarray:
    """The state Thompson sampling draws from each row of ``beliefs [n,S]`` with its uniform ``u [n]`` in ``[0, 1]``: with
    ``q_c`` the sequential prefix sums of ``b`` inside chunk ``c`` (256 states), ``m_c = q_c[last]``, ``P_c = P_{c-1} + m_c``
    and ``target = u * P_{C-1}``: the chunk ``c*`` is the first with ``target < P_c`` (else the last with ``m_c > 0``), and the
    state the first ``j`` of it with ``target - P_{c*-1} < q_{c*}[j]`` (else its last with ``b > 0``).  The drawn state has
    positive mass."""
    q = np.cumsum(_chunked(beliefs), axis=2)                    # (np.cumsum adds sequentially)
    n, C, _ = q.shape
    u = np.asarray(u, dtype=np.float64)
    if u.shape != (n,) or not np.all((u >= 0.0) & (u <= 1.0)):
        raise ValueError('u must be [n] with entries in [0, 1]')
    rows = np.arange(n)
    m = q[:, :, -1]
    P = np.cumsum(m, axis=1)
    target = u * P[:, -1]
    hit = target[:, None] < P
    c = np.argmax(hit, axis=1)
    none = ~hit.any(axis=1)
    if none.any():
        pos = m[none] > 0
        c[none] = np.where(pos.any(axis=1), C - 1 - np.argmax(pos[:, ::-1], axis=1), 0)
    r = target - np.where(c > 0, P[rows, np.maximum(c - 1, 0)], 0.0)
    qc = q[rows, c]
    hit = r[:, None] < qc
    j = np.argmax(hit, axis=1)
    none = ~hit.any(axis=1)
    if none.any():
        bc = _chunked(beliefs)[rows[none], c[none]] > 0
        j[none] = np.where(bc.any(axis=1), STATE_POLICY_CHUNK - 1 - np.argmax(bc[:, ::-1], axis=1), 0)
    return c * STATE_POLICY_CHUNK + j


def state_policy_votes(beliefs, state_actions, A: int) -> np.ndarray:
    """``W [n,A]``: ``W_c[a]`` = the sequential sum over chunk ``c`` (256 states, ascending) of ``b[s]`` where
    ``state_actions[s] == a``; ``W[a]`` = the ``W_c[a]`` added in chunk order."""
    bc = _chunked(beliefs)
    n, C, L = bc.shape
    sa = np.full(C * L, -1, dtype=np.int64)
    sa[:state_actions.shape[0]] = state_actions
    sa = sa.reshape(C, L)
    W = np.zeros((n, A))
    for a in range(A):
        Wc = np.cumsum(np.where(sa[None] == a, bc, 0.0), axis=2)[:, :, -1]     # (+0.0 leaves the bits of a sum >= +0.0)
        W[:, a] = np.cumsum(Wc, axis=1)[:, -1]
    return W


def state_policy_numpy(beliefs, state_actions, rule, u=None, table_dtype=np.float64, action_count=None):
    """The state policy ``rule`` for every row of ``beliefs [n,S]``, on the host: what ``pbvi_state_policy`` computes on the
    device, bit for bit.  ``beliefs`` are cast to ``table_dtype``, the engine's number format, and widened.  Returns
    ``(action [n], state [n], votes)``:
        rule 0 / ``'mls'``:       the table's action in the first maximum of ``b``; ``state`` = that state; ``votes`` ``None``
        rule 1 / ``'voting'``:    the first maximum of ``votes = state_policy_votes(...)`` ``[n,A]``; ``state`` = -1
        rule 2 / ``'thompson'``:  the table's action in ``thompson_state_numpy(b, u)``; ``state`` = that state
    ``action_count``: the model's ``A``, the width of ``votes`` (default ``max(state_actions) + 1``)."""
    return _state_policy(beliefs, state_actions, action_count, rule, u, table_dtype)


def _state_policy(beliefs, state_actions, A, rule, u, table_dtype):
    rule = _state_policy_rule(rule)
    b = np.asarray(beliefs, dtype=table_dtype).astype(np.float64)
    if b.ndim != 2:
        raise ValueError('beliefs must be [n, S]')
    sa = np.asarray(state_actions)
    A = int(A) if A is not None else (int(sa.max()) + 1 if sa.size else 1)
    sa = _state_actions(b.shape[1], A, sa)
    if u is not None and rule != 2:
        raise ValueError('u belongs to rule 2 (Thompson)')
    if rule == 0:
        s = _first_greater(b)
        return sa[s], s, None
    if rule == 1:
        W = state_policy_votes(b, sa, A)
        return _first_greater(W), np.full(b.shape[0], -1, dtype=np.int64), W
    if u is None:
        raise ValueError('Thompson sampling needs its uniforms u [n]')
    s = thompson_state_numpy(b, u)
    return sa[s], s, None


def thompson_uniform(seed: int, sim_ids, t) -> np.ndarray:
    """Thompson sampling's uniform of simulation ``i`` at step ``t``: ``rollout_uniform(seed, i, 2**33 + t)``, a third
    stream beside the simulator's ``t`` and ``2**32 + t`` (``t < 2**31``)."""
    return rollout_uniform(seed, sim_ids, THOMPSON_STREAM + int(t))


def rollout_state_policy_numpy(model, beliefs, start_states, state_actions, rule, seed: int, first_sim_id: int, T: int,
                               table_dtype=np.float64, return_beliefs: bool = False, env=None):
    """``rollout_numpy`` with a state policy, on the host: what ``pbvi_rollout_state_policy`` computes on the device.  Per
    step and running simulation the action is ``state_policy_numpy(b, state_actions, rule, u, table_dtype)``'s, Thompson
    with ``u = thompson_uniform(seed, id, t)``; the beliefs are held in ``table_dtype`` between the steps, as the engine
    holds them.  ``env=None``: the model's world, with ``rollout_numpy``'s return value; ``env``: the draw, the observation,
    the lost rule and the return value (``lost [n]`` last) of ``rollout_env_numpy``."""
    rule = _state_policy_rule(rule)
    if int(T) >= 1 << 31:
        raise ValueError('T must be below 2**31')
    if env is not None and not isinstance(env, (FrameEnvironment, TableEnvironment)):
        raise ValueError('env must be a FrameEnvironment or a TableEnvironment')
    m, T, b, s, _, _ = _rollout_inputs(model, beliefs, start_states, T)
    sa = _state_actions(m.state_count, m.action_count, state_actions)
    block = _HostBeliefBlock(m, None, b, store_dtype=table_dtype)

    def choose(t, ids):
        u = thompson_uniform(seed, ids, t) if rule == 2 else None
        return block.state_policy_actions(sa, rule, u, table_dtype)

    if env is None:
        return _rollout_loop(m, block, choose, s, seed, first_sim_id, T, table_dtype, return_beliefs, choose_draws=True)
    return _rollout_env_loop(m, env, block, choose, s, seed, first_sim_id, T, table_dtype, return_beliefs, choose_draws=True)


class _HostBeliefBlock:
    """Belief block of the parallel simulator held in NumPy (reference CPU statements, ``:3029``, ``:3306-3311``).
    ``store_dtype``: the beliefs are rounded to that format after every step, as an engine of that format stores them."""

    def __init__(self, model: Model, value_function: ValueFunction, beliefs: np.ndarray, store_dtype=None):
        self.m, self.b = model, beliefs
        self.alpha = None if value_function is None else value_function.alpha_vector_array      # (infotaxis has none)
        self.store_dtype = None if store_dtype is None or np.dtype(store_dtype) == np.float64 else np.dtype(store_dtype)
        self._stored()

    def _stored(self) -> None:
        if self.store_dtype is not None:
            self.b = self.b.astype(self.store_dtype).astype(np.float64)

    def count(self) -> int:
        return self.b.shape[0]

    def state_policy_actions(self, state_actions, rule: int = 0, u=None, table_dtype=np.float64) -> np.ndarray:
        """The state policy ``rule`` (``state_policy_numpy``) of every belief of the block; ``u``: Thompson's uniforms."""
        return _state_policy(self.b, state_actions, self.m.action_count, rule, u, table_dtype)[0]

    def best_vectors(self) -> np.ndarray:
        return np.argmax(np.matmul(self.b, self.alpha.T), axis=1)

    def best_actions(self, gamma: float) -> np.ndarray:
        """One-step lookahead: ``argmax_a Q(b,a)`` of every belief of the block."""
        return np.argmax(_q_values_numpy(self.m, self.b, self.alpha, gamma), axis=1)

    def infotaxis_actions(self, table_dtype=np.float64) -> np.ndarray:
        """Infotaxis: the first ``argmin_a`` of the expected successor entropy of every belief of the block."""
        return infotaxis_numpy(self.m, self.b, table_dtype)[1]

    def space_aware_actions(self, weights, objective: int = 0, table_dtype=np.float64) -> np.ndarray:
        """Space-aware infotaxis: the first ``argmin_a`` of ``space_aware_numpy``'s ``F`` of every belief of the block."""
        return space_aware_numpy(self.m, self.b, weights, objective, table_dtype)[1]

    def _push(self, actions: np.ndarray, observations: np.ndarray) -> np.ndarray:
        """The un-normalised Bayes step of every row: ``u[b, s'] = sum_{(s,r): rs[s,a,r] = s'} b[s] RTO[s,a,o,r]``."""
        m, n = self.m, self.b.shape[0]
        S = m.state_count
        w = m.reachable_transitional_observation_table[:, actions, observations, :] * self.b.T[:, :, None]   # [S,n,R]
        tgt = m.reachable_states[:, actions, :]                                                             # [S,n,R]
        flat = (n, S * m.reachable_state_count)
        idx = tgt.swapaxes(0, 1).reshape(flat) + (np.arange(n)[:, None] * S)
        return np.bincount(idx.ravel(), weights=w.swapaxes(0, 1).reshape(flat).ravel(), minlength=n * S).reshape((-1, S))

    def advance(self, actions: np.ndarray, observations: np.ndarray, keep: np.ndarray) -> None:
        nb = self._push(actions, observations)
        nb /= np.sum(nb, axis=1)[:, None]
        self.b = nb[keep]
        self._stored()

    def advance_or_lose(self, actions: np.ndarray, observations: np.ndarray, keep: np.ndarray) -> np.ndarray:
        """``advance`` with the lost rule of ``rollout_env_numpy``: a kept row whose un-normalised mass ``Z`` is 0 or not
        finite (an observation the model gives no probability) is dropped too, before any division.  Returns the ``[n]``
        mask of the rows lost."""
        nb = self._push(actions, observations)
        z = np.sum(nb, axis=1)
        lost = keep & ((z == 0) | ~np.isfinite(z))
        go = keep & ~lost
        self.b = nb[go] / z[go][:, None]
        self._stored()
        return lost


class _DeviceBeliefBlock:
    """Belief block resident in the HIP engine: ``pbvi_value_max`` + ``pbvi_beliefs_advance``.

    The engine holds one block of at most 65535 beliefs.  Larger simulations (the reference takes any ``n``) run in
    chunks of ``CHUNK`` rows that live on the host between steps and pass through the engine one after the other --
    correct, but every step then moves the beliefs over PCIe; the resident path is the one that is fast."""

    CHUNK = 32768

    def __init__(self, model: Model, value_function: ValueFunction, beliefs: np.ndarray, resident_rows: int = 65535):
        """``resident_rows``: the largest block that is set as one (``get_best_action`` chunks above ``CHUNK`` already)."""
        self.eng = model.engine
        if value_function is not None:                          # (infotaxis has none)
            self.eng.sync_rows('alpha', value_function.alpha_vector_list, lambda v: v.values)
        self.chunks = None
        if beliefs.shape[0] <= resident_rows:
            self.eng.set_beliefs(beliefs)
        else:
            self.chunks = [np.ascontiguousarray(beliefs[i:i + self.CHUNK]) for i in range(0, beliefs.shape[0], self.CHUNK)]

    def each(self, call) -> np.ndarray:
        """``call()`` -- an engine call that returns one entry per belief of the resident block, which stays on the device --
        for every belief of this block: once if it is resident, else on each chunk made resident in turn, joined."""
        if self.chunks is None:
            return call()
        out = []
        for c in self.chunks:
            self.eng.set_beliefs(c)
            out.append(call())
        return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)

    def best_vectors(self) -> np.ndarray:
        return self.each(lambda: self.eng.max_value_resident()[1])

    def best_actions(self, gamma: float) -> np.ndarray:
        """One-step lookahead: ``argmax_a Q(b,a)`` of every belief of the block (``pbvi_q_values``)."""
        return self.each(lambda: self.eng.q_values_resident(gamma)[1])

    def infotaxis_actions(self) -> np.ndarray:
        """Infotaxis: the first ``argmin_a`` of the expected successor entropy of every belief of the block
        (``pbvi_infotaxis``)."""
        return self.each(lambda: self.eng.infotaxis_resident()[1])

    def space_aware_actions(self, weights, objective: int = 0) -> np.ndarray:
        """Space-aware infotaxis: the first ``argmin_a`` of ``pbvi_space_aware``'s ``F`` of every belief of the block (the
        weights are uploaded once per block)."""
        if getattr(self, '_weights', None) is not weights:
            self.eng.set_state_weights(weights)
            self._weights = weights
        return self.each(lambda: self.eng.space_aware_resident(objective)[1])

    def count(self) -> int:
        return self.eng.B if self.chunks is None else sum(c.shape[0] for c in self.chunks)

    def state_policy_actions(self, state_actions, rule: int = 0, u=None) -> np.ndarray:
        """The state policy ``rule`` (``pbvi_state_policy``) of every belief of the block; ``u``: Thompson's uniforms, one
        per belief.  The table is uploaded once per block."""
        if getattr(self, '_state_actions', None) is not state_actions:
            self.eng.set_state_policy(state_actions)
            self._state_actions = state_actions
        if self.chunks is None:
            return self.eng.state_policy_resident(rule, uniforms=u)
        out, i0 = [], 0
        for c in self.chunks:
            self.eng.set_beliefs(c)
            out.append(self.eng.state_policy_resident(rule, uniforms=None if u is None else u[i0:i0 + c.shape[0]]))
            i0 += c.shape[0]
        return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)

    def advance(self, actions: np.ndarray, observations: np.ndarray, keep: np.ndarray) -> None:
        if self.chunks is None:
            self.eng.advance_beliefs(actions, observations, keep)
            return
        nxt, i0 = [], 0
        for c in self.chunks:
            n = c.shape[0]
            self.eng.set_beliefs(c)
            if self.eng.advance_beliefs(actions[i0:i0 + n], observations[i0:i0 + n], keep[i0:i0 + n]) > 0:
                nxt.append(self.eng.fetch_beliefs())
            i0 += n
        self.chunks = nxt
        if sum(c.shape[0] for c in nxt) <= 65535 and nxt:       # few enough simulations left: stay on the device from here on
            self.eng.set_beliefs(np.concatenate(nxt))
            self.chunks = None


class Agent:
    """Greedy agent over a value function (``src/pomdp.py:2948-3380``): best action for a belief, single
    simulations, and n simulations advanced together with the belief block on the host or in the HIP engine.

    ``lookahead=0``: the reference's policy, ``actions[argmax_v b.alpha_v]``.  ``lookahead=1``: the one-step lookahead
    policy ``argmax_a Q(b,a)``, ``Q(b,a) = b.ER[:,a] + gamma * sum_o max_v b.Gamma[a,o,v]`` (``PBVI_Solver.q_values``),
    with discount ``gamma``."""

    def __init__(self, model: Model, value_function: Union[ValueFunction, None] = None, lookahead: int = 0,
                 gamma: float = 0.99) -> None:
        if lookahead not in (0, 1):
            raise ValueError(f'lookahead must be 0 or 1, not {lookahead!r}')
        self.model = model
        self.value_function = value_function
        self.lookahead = lookahead
        self.gamma = gamma

    def train(self, solver: PBVI_Solver, expansions: int, horizon: int) -> SolverHistory:
        self.value_function, hist = solver.solve(self.model, expansions, horizon)
        return hist

    def _on_gpu(self) -> bool:
        """Whether this agent's policy is evaluated in the HIP engine."""
        assert self.value_function is not None, "No value function, training probably has to be run..."
        return self.value_function.is_on_gpu

    def _block_actions(self, block) -> np.ndarray:
        """The policy's actions for the beliefs of a belief block of the parallel simulator."""
        if self.lookahead == 1:
            return block.best_actions(self.gamma)
        return self.value_function.actions[block.best_vectors()]

    def get_best_action(self, belief):
        """This agent's action -- ``Agent``: ``actions[argmax_v b.alpha_v]`` (``:3005-3034``), or ``argmax_a Q(b,a)`` with
        ``lookahead=1`` -- for one ``Belief`` (returns int) or a ``[n,S]`` array: ``_block_actions`` of the array as a belief
        block, in the HIP engine (``_DeviceBeliefBlock.CHUNK`` beliefs at a time) when the agent is on the GPU."""
        on_gpu, vf = self._on_gpu(), self.value_function
        single = isinstance(belief, Belief)
        arr = belief.values[None, :] if single else belief
        model = self.model if vf is None else vf.model
        if on_gpu:
            block = _DeviceBeliefBlock(model, vf, arr, resident_rows=_DeviceBeliefBlock.CHUNK)
        else:
            block = _HostBeliefBlock(model, vf, arr)
        acts = self._block_actions(block)
        return int(acts[0]) if single else acts

    def simulate(self, simulator: Union[Simulation, None] = None, max_steps: int = 1000,
                 start_state: Union[int, None] = None, initial_belief: Union[Belief, None] = None,
                 print_progress: bool = True, print_stats: bool = True) -> SimulationHistory:
        self.model = self.model.gpu_model if self._on_gpu() else self.model.cpu_model
        simulator = Simulation(self.model) if simulator is None else simulator
        s = simulator.initialize_simulation(start_state=start_state)
        belief = Belief(self.model) if initial_belief is None else initial_belief
        history = SimulationHistory(self.model, start_state=s, start_belief=belief)
        t0 = datetime.now()
        for _ in range(max_steps):
            a = self.get_best_action(belief)
            r, o = simulator.run_action(a)
            belief = belief.update(a, o)
            history.add(action=a, next_state=simulator.agent_state, next_belief=belief, reward=r, observation=o)
            if simulator.is_done:
                break
        if print_stats:
            print('Simulation done:')
            print(f'\t- Runtime (s): {(datetime.now() - t0).total_seconds()}')
            print(f'\t- Steps: {len(history.states)}')
            print(f'\t- Total rewards: {sum(history.rewards)}')
            print(f'\t- End state: {self.model.state_labels[history.states[-1]]}')
        return history

    def run_n_simulations(self, simulator: Union[Simulation, None] = None, n: int = 1000, max_steps: int = 1000,
                          start_states: Union[list, int, None] = None, initial_beliefs=None,
                          reward_discount: float = 0.99, print_progress: bool = True, print_stats: bool = True):
        simulator = Simulation(self.model) if simulator is None else simulator
        assert (not isinstance(start_states, list)) or (len(start_states) == n), 'The size of the list of start states has to match n'
        assert (not isinstance(initial_beliefs, list)) or (len(initial_beliefs) == n), 'The size of the list of initial beliefs has to match n'
        t0 = datetime.now()
        histories, totals, discounted, done = [], RewardSet(), [], 0
        for i in range(n):
            h = self.simulate(simulator=simulator, max_steps=max_steps,
                              start_state=(start_states[i] if isinstance(start_states, list) else start_states),
                              initial_belief=(initial_beliefs[i] if isinstance(initial_beliefs, list) else initial_beliefs),
                              print_progress=False, print_stats=False)
            done += int(simulator.is_done)
            histories.append(h)
            totals.append(np.sum(h.rewards))
            discounted.append(h.rewards.get_total_discounted_reward(reward_discount))
        if print_stats:
            print(f'All {n} simulations done:')
            print(f'\t- Average runtime (s): {(datetime.now() - t0).total_seconds() / n}')
            print(f'\t- Simulations reached goal: {done}/{n} ({n - done} failures)')
            print(f'\t- Average step count: {sum(len(h) for h in histories) / n}')
            print(f'\t- Average total rewards: {sum(totals) / n}')
            print(f'\t- Average discounted rewards (ADR): {sum(discounted) / n}')
        return totals, histories

    def run_n_simulations_parallel(self, n: int = 1000, simulator_set: Union[SimulationSet, None] = None,
                                   max_steps: int = 1000, start_states: Union[list, int, None] = None,
                                   initial_beliefs=None, reward_discount: float = 0.99,
                                   print_progress: bool = True, print_stats: bool = True,
                                   device_rng_seed: Union[int, None] = None, environment=None):
        """n simulations advanced in lock-step (``src/pomdp.py:3203-3380``).  Per step: best α per belief
        (GEMM + first-max), host simulator draw, Bayes update of every belief, done-filter.  With the value
        function on the GPU the belief block lives in the HIP engine for the whole run; only the ``[n]`` index,
        action and observation vectors cross the boundary each step.

        ``device_rng_seed=None`` (default): the draws are NumPy's global stream in the reference's call order, so a seeded
        run reproduces the reference's trajectories.  An integer: the counter-based rollout instead (``rollout_numpy``'s
        definition; simulation ``i`` draws ``rollout_uniform(seed, i, t)`` at step ``t``) -- the whole step loop runs in
        the HIP engine (``pbvi_rollout``) when the value function is on the GPU, on the host otherwise, and the
        trajectories do not depend on which, up to exact ties between actions.  Only the start states, when none are
        given, still come from NumPy's stream.

        ``environment`` (a ``FrameEnvironment`` or ``TableEnvironment``; needs ``device_rng_seed``): the observations come
        from it instead of the model (``rollout_env_numpy``'s definition, ``pbvi_rollout_env`` on the GPU), per-simulation
        shifts are ``[n]``, and every returned ``SimulationHistory`` says in ``lost`` whether it stopped at an observation the
        model gives probability 0."""
        if environment is not None and device_rng_seed is None:
            raise ValueError('environment needs device_rng_seed: the NumPy-stream path simulates the model itself')
        on_gpu = self._on_gpu()
        vf = self.value_function
        model = self.model.gpu_model if on_gpu else self.model.cpu_model
        assert (not isinstance(start_states, list)) or (len(start_states) == n), 'The size of the list of start states has to match n'
        assert (not isinstance(initial_beliefs, list)) or (len(initial_beliefs) == n), 'The size of the list of initial beliefs has to match n'

        if initial_beliefs is None:
            b0 = np.repeat(Belief(model).values[None, :], n, axis=0)
        elif isinstance(initial_beliefs, Belief):
            b0 = np.repeat(initial_beliefs.values[None, :], n, axis=0)
        else:
            b0 = np.array([b.values for b in initial_beliefs])

        simulator_set = SimulationSet(model) if simulator_set is None else simulator_set
        start_state_array = simulator_set.initialize_simulations(n, start_states)
        if device_rng_seed is not None:
            return self._run_counter_rollouts(model, simulator_set, b0, np.asarray(start_state_array), int(device_rng_seed),
                                              max_steps, reward_discount, print_stats, environment)
        block = (_DeviceBeliefBlock if on_gpu else _HostBeliefBlock)(model, vf, b0)

        done_at_step = np.full(n, -1, dtype=int)
        alive = np.arange(n)
        discount = reward_discount
        rewards_history = np.zeros((max_steps, n))
        discounted_history = np.zeros((max_steps, n))
        states_history = np.empty((max_steps + 1, n))
        states_history[0] = start_state_array
        actions_history = np.empty((max_steps, n))
        observations_history = np.empty((max_steps, n))

        t0 = datetime.now()
        for i in range(max_steps):
            best_actions = self._block_actions(block)
            rewards, observations = simulator_set.run_actions(best_actions)
            finished = simulator_set.is_done
            block.advance(best_actions, observations, ~finished)

            rewards_history[i, alive] = rewards
            discounted_history[i, alive] = rewards * discount
            states_history[i + 1, alive] = simulator_set.agent_states
            actions_history[i, alive] = best_actions
            observations_history[i, alive] = observations
            done_at_step[alive[finished]] = i

            alive = alive[~finished]
            simulator_set.n = len(alive)
            simulator_set.agent_states = simulator_set.agent_states[~finished]
            simulator_set.simulations = simulator_set.simulations[~finished]
            simulator_set.is_done = finished[~finished]
            discount *= reward_discount
            if len(alive) == 0:
                break

        histories, steps_sum = [], 0
        b_start = Belief(model)
        for i, s0 in enumerate(start_state_array):
            h = SimulationHistory(self.model, int(s0), b_start)
            last = int(done_at_step[i]) if done_at_step[i] >= 0 else max_steps
            steps_sum += last
            h.states = states_history[:last + 1, i].tolist()
            h.actions = actions_history[:last, i].tolist()
            h.observations = observations_history[:last, i].tolist()
            h.rewards = rewards_history[:last, i].tolist()
            histories.append(h)
        n_done = int(np.sum(done_at_step >= 0))
        if print_stats:
            print(f'All {n} simulations done in {(datetime.now() - t0).total_seconds():.3f}s:')
            print(f'\t- Simulations reached goal: {n_done}/{n} ({n - n_done} failures)')
            print(f'\t- Average step count: {steps_sum / n}')
            print(f'\t- Average total rewards: {np.sum(rewards_history) / n}')
            print(f'\t- Average discounted rewards (ADR): {np.sum(discounted_history) / n}')
        return RewardSet(np.sum(rewards_history, axis=0).tolist()), histories

    ROLLOUT_CHUNK = 65535            # simulations per ``pbvi_rollout`` call: the engine's belief block limit

    @staticmethod
    def _end_mask(model: Model) -> np.ndarray:
        mask = np.zeros(model.state_count, dtype=np.uint8)
        mask[np.asarray(model.end_states, dtype=np.int64)] = 1
        return mask

    def _rollout_chunks(self, eng, b0: np.ndarray, start_states: np.ndarray, shifts, call):
        """The chunk loop of the device rollouts: ``ROLLOUT_CHUNK`` simulations at a time become the engine's belief block and
        ``call(start_states, first_sim_id, shifts)`` -- their rows of both, ``shifts`` may be ``None`` -- runs them; the 4 or 5
        arrays of the chunks, joined along the simulations."""
        parts = []
        for i0 in range(0, b0.shape[0], self.ROLLOUT_CHUNK):
            i1 = i0 + self.ROLLOUT_CHUNK
            eng.set_beliefs(b0[i0:i1])
            parts.append(call(start_states[i0:i1], i0, None if shifts is None else shifts[i0:i1]))
        return tuple(np.concatenate([p[k] for p in parts], axis=-1) for k in range(len(parts[0])))

    # What the counter-based rollouts need to know of the policy, beside ``_block_actions``: three hooks.
    def _upload(self, eng) -> None:
        """What the engine needs resident before this policy's device rollout: the alpha rows."""
        eng.sync_rows('alpha', self.value_function.alpha_vector_list, lambda v: v.values)

    def _host_rollout(self, model: Model, b0: np.ndarray, start_states: np.ndarray, seed: int, T: int, env):
        vf = self.value_function
        if env is not None:
            return rollout_env_numpy(model, env, self.lookahead, vf.alpha_vector_array, vf.actions, b0, start_states, seed, 0, T,
                                     self.gamma)
        return rollout_numpy(model, vf.alpha_vector_array, vf.actions, b0, start_states, seed, 0, T, self.lookahead, self.gamma)

    def _device_rollout(self, eng, end_mask: np.ndarray, seed: int, T: int, env):
        """``call(start_states, first_sim_id, shifts)`` of ``_rollout_chunks``: this policy's rollout of the resident block."""
        acts = self.value_function.actions
        if env is not None:
            return lambda s0, first, sh: eng.rollout_env(self.lookahead, acts, s0, end_mask, seed, T, first_sim_id=first,
                                                         gamma=self.gamma, shifts=sh, end_observation=env.end_observation)
        return lambda s0, first, sh: eng.rollout(acts, s0, end_mask, seed, T, first_sim_id=first, lookahead=self.lookahead,
                                                 gamma=self.gamma)

    def _counter_trajectories(self, model: Model, b0: np.ndarray, start_states: np.ndarray, seed: int, T: int, env=None):
        """``(states, actions, observations, steps)`` of the counter-based rollout of this agent's policy, against ``env`` with
        ``lost`` behind them: on the device when the agent is (what the policy needs uploaded first, then the environment,
        once: later calls with the same arrays find it there), else on the host."""
        if not self._on_gpu():
            return self._host_rollout(model, b0, start_states, seed, T, env)
        shifts = None
        if env is not None:
            shifts = env.check(model.state_count, model.action_count, model.observation_count, b0.shape[0], T)
        eng = model.engine
        self._upload(eng)
        if env is not None:
            eng.hold_environment(env)
        out = self._rollout_chunks(eng, b0, start_states, shifts, self._device_rollout(eng, self._end_mask(model), seed, T, env))
        return out if env is not None else out[:4]

    def _run_counter_rollouts(self, model: Model, simulator_set: SimulationSet, b0: np.ndarray, start_states: np.ndarray,
                              seed: int, max_steps: int, reward_discount: float, print_stats: bool, environment=None):
        """``run_n_simulations_parallel(device_rng_seed=seed)``: the trajectories from ``pbvi_rollout`` (value function on
        the GPU; more than ``ROLLOUT_CHUNK`` simulations in chunks with ``first_sim_id`` advanced) or ``rollout_numpy``,
        the rewards from the recorded ``(s, a, s', o)`` afterwards, the result in ``run_n_simulations_parallel``'s form."""
        n, T = b0.shape[0], int(max_steps)
        t0 = datetime.now()
        out = self._counter_trajectories(model, b0, start_states, seed, T, environment)
        states, actions, observations, steps = out[:4]
        lost = out[4] if environment is not None else np.zeros(n, dtype=np.uint8)
        ran = actions >= 0                                       # [T, n] steps that were taken
        rewards_history = np.zeros((T, n))
        if ran.any():
            rewards_history[ran] = simulator_set._step_rewards(states[:-1][ran].astype(np.int64), actions[ran].astype(np.int64),
                                                               states[1:][ran].astype(np.int64), observations[ran].astype(np.int64))
        discounted_history = rewards_history * (reward_discount ** np.arange(1, T + 1))[:, None]
        histories = []
        b_start = Belief(model)
        for i in range(n):
            h = SimulationHistory(self.model, int(start_states[i]), b_start)
            last = int(steps[i])
            h.states = states[:last + 1, i].tolist()
            h.actions = actions[:last, i].tolist()
            h.observations = observations[:last, i].tolist()
            h.rewards = rewards_history[:last, i].tolist()
            h.lost = bool(lost[i])
            histories.append(h)
        n_done = int(np.sum(np.isin(states[steps, np.arange(n)], model.end_states)))
        if print_stats:
            print(f'All {n} simulations done in {(datetime.now() - t0).total_seconds():.3f}s:')
            print(f'\t- Simulations reached goal: {n_done}/{n} ({n - n_done} failures)')
            print(f'\t- Average step count: {int(np.sum(steps)) / n}')
            print(f'\t- Average total rewards: {np.sum(rewards_history) / n}')
            print(f'\t- Average discounted rewards (ADR): {np.sum(discounted_history) / n}')
        return RewardSet(np.sum(rewards_history, axis=0).tolist()), histories


class Infotaxis_Agent(Agent):
    """Infotaxis: the greedy policy that takes the action with the smallest expected entropy of the next belief,
    ``argmin_a sum_o P(o|b,a) H(update(b,a,o))`` (``infotaxis_numpy``) -- the baseline a solved olfactory-search policy is
    judged against.  It takes no value function; a model on the GPU (``model.to_gpu()``) has the HIP engine evaluate it
    (``pbvi_infotaxis``, ``pbvi_rollout_infotaxis``).  ``simulate``, ``run_n_simulations`` and
    ``run_n_simulations_parallel(..., device_rng_seed=None)`` are ``Agent``'s with this policy."""

    def __init__(self, model: Model) -> None:
        super().__init__(model, None)

    def _on_gpu(self) -> bool:
        return bool(self.model.is_on_gpu)

    def _block_actions(self, block) -> np.ndarray:
        return block.infotaxis_actions()

    def _upload(self, eng) -> None:
        pass

    def _host_rollout(self, model: Model, b0: np.ndarray, start_states: np.ndarray, seed: int, T: int, env):
        if env is not None:
            return rollout_env_numpy(model, env, ENV_POLICY_INFOTAXIS, None, None, b0, start_states, seed, 0, T, self.gamma)
        return rollout_infotaxis_numpy(model, b0, start_states, seed, 0, T)

    def _device_rollout(self, eng, end_mask: np.ndarray, seed: int, T: int, env):
        if env is not None:
            return lambda s0, first, sh: eng.rollout_env(ENV_POLICY_INFOTAXIS, None, s0, end_mask, seed, T, first_sim_id=first,
                                                         gamma=self.gamma, shifts=sh, end_observation=env.end_observation)
        return lambda s0, first, sh: eng.rollout_infotaxis(s0, end_mask, seed, T, first_sim_id=first)


class SpaceAware_Agent(Agent):
    """Space-aware infotaxis (Loisy & Eloy 2022): the greedy policy for ``J(b) = log2(D(b) + 2^(H(b) - 1) - 1/2)`` of the next
    belief, ``D`` its expected distance to the source and ``H`` its entropy in bits (``space_aware_numpy``) -- the baseline
    that beats infotaxis and comes close to solved policies.  ``weights [S]``: the distance of every state to the source,
    by default ``manhattan_to_end_states(model)``.  ``objective='expected_weight'``: greedy for the expected weight of the
    next belief alone (greedy distance; with ``weights = max(V_MDP) - V_MDP`` a QMDP-style policy).  It takes no value
    function; a model on the GPU (``model.to_gpu()``) has the HIP engine evaluate it (``pbvi_space_aware``,
    ``pbvi_rollout_space_aware``).  ``simulate``, ``run_n_simulations`` and ``run_n_simulations_parallel(...,
    device_rng_seed=, environment=)`` are ``Agent``'s with this policy."""

    def __init__(self, model: Model, weights=None, objective='space_aware') -> None:
        super().__init__(model, None)
        self.objective = _space_aware_objective(objective)
        self.weights = _state_weights(model.state_count, manhattan_to_end_states(model) if weights is None else weights)

    def _on_gpu(self) -> bool:
        return bool(self.model.is_on_gpu)

    def _block_actions(self, block) -> np.ndarray:
        return block.space_aware_actions(self.weights, self.objective)

    def _upload(self, eng) -> None:
        eng.set_state_weights(self.weights)

    def _host_rollout(self, model: Model, b0: np.ndarray, start_states: np.ndarray, seed: int, T: int, env):
        return rollout_space_aware_numpy(model, b0, start_states, self.weights, seed, 0, T, self.objective, env=env)

    def _device_rollout(self, eng, end_mask: np.ndarray, seed: int, T: int, env):
        end_obs = -1 if env is None else env.end_observation
        return lambda s0, first, sh: eng.rollout_space_aware(s0, end_mask, seed, T, first_sim_id=first, objective=self.objective,
                                                             use_env=env is not None, shifts=sh, end_observation=end_obs)


class StatePolicy_Agent(Agent):
    """The heuristics that act through a policy ``pi(s)`` of the underlying MDP: ``rule='mls'`` plays ``pi`` of the most
    likely state, ``'voting'`` the action with the largest vote ``sum_{s: pi(s) = a} b(s)``, ``'thompson'`` ``pi`` of a state
    drawn from the belief (``state_policy_numpy``) -- the baselines tabulated beside infotaxis and QMDP.  ``policy``: the
    table ``[S]`` itself, or an action-labelled ``ValueFunction`` (a ``VI_Solver`` or ``FIB_Solver`` solution), read with
    ``state_actions_from``.  A model on the GPU (``model.to_gpu()``) has the HIP engine evaluate it (``pbvi_state_policy``,
    ``pbvi_rollout_state_policy``).  ``simulate``, ``run_n_simulations`` and ``run_n_simulations_parallel(...,
    device_rng_seed=, environment=)`` are ``Agent``'s with this policy.

    Thompson sampling is reproducible exactly with ``device_rng_seed`` only: simulation ``i`` then draws with
    ``thompson_uniform(seed, i, t)`` on the host and on the device alike.  In the paths that use NumPy's global stream (no
    ``device_rng_seed``; ``get_best_action``, ``simulate``) it takes ``np.random.random(n)`` for the ``n`` beliefs of the
    step, before the simulator's draws of that step."""

    def __init__(self, model: Model, policy, rule='mls') -> None:
        super().__init__(model, None)
        self.rule = _state_policy_rule(rule)
        table = state_actions_from(policy) if isinstance(policy, ValueFunction) else policy
        self.state_actions = _state_actions(model.state_count, model.action_count, table)

    def _on_gpu(self) -> bool:
        return bool(self.model.is_on_gpu)

    def _block_actions(self, block) -> np.ndarray:
        u = np.random.random(block.count()) if self.rule == 2 else None
        return block.state_policy_actions(self.state_actions, self.rule, u)

    def _upload(self, eng) -> None:
        eng.set_state_policy(self.state_actions)

    def _host_rollout(self, model: Model, b0: np.ndarray, start_states: np.ndarray, seed: int, T: int, env):
        return rollout_state_policy_numpy(model, b0, start_states, self.state_actions, self.rule, seed, 0, T, env=env)

    def _device_rollout(self, eng, end_mask: np.ndarray, seed: int, T: int, env):
        end_obs = -1 if env is None else env.end_observation
        return lambda s0, first, sh: eng.rollout_state_policy(s0, end_mask, seed, T, first_sim_id=first, rule=self.rule,
                                                              use_env=env is not None, shifts=sh, end_observation=end_obs)


# --------------------------------------------------------------------------- #
# Cassandra .POMDP files (inputs of BASELINE configs 0-1)
# --------------------------------------------------------------------------- #
def load_POMDP_file(file_name: str) -> Tuple[Model, PBVI_Solver]:
    """Parse a Cassandra ``.POMDP`` file into ``(Model, PBVI_Solver(gamma))``.

    Covers the constructs the reference's loader handles (``src/pomdp.py:3383-3737``):
    ``discount/values/states/actions/observations/start`` headers and ``T``, ``O``,
    ``R`` entries given as single values, rows, or matrices with ``uniform`` /
    ``identity`` shortcuts and ``*`` wildcards.  Rewards land in ``R[s,a,s',o]``.

    Bit-identical tables to the reference's loader on 20 of the 25 example models it ships
    (``tests/golden/pomdp_file_tables.json``).  The other five: three it rejects itself; ``hanks.95`` and
    ``network.95`` write fully specified entries with the value on the next line (``T: a : s : s'`` / ``0.1``),
    which the reference reads as a row assignment (its tables stop being stochastic) and this loader reads as the
    file format defines it, one entry.
    """
    with open(file_name) as fh:
        lines = [ln.split('#')[0].strip() for ln in fh]
    lines = [ln for ln in lines if ln]

    gamma = 1.0
    names = {'states': None, 'actions': None, 'observations': None}
    start = None
    T = Ob = Rw = None

    def counts():
        return len(names['states']), len(names['actions']), len(names['observations'])

    def ensure_tables():
        nonlocal T, Ob, Rw
        if T is None and all(v is not None for v in names.values()):
            S, A, O = counts()
            T = np.zeros((S, A, S))
            Ob = np.zeros((S, A, O))
            Rw = np.zeros((S, A, S, O))

    def sel(kind: str, tok: str):
        n = len(names[kind])
        if tok == '*':
            return list(range(n))
        if tok.isnumeric():
            return [int(tok)]
        return [names[kind].index(tok)]

    def is_number(tok: str) -> bool:
        try:
            float(tok)
            return True
        except ValueError:
            return False

    i = 0
    while i < len(lines):
        ln = lines[i]
        i += 1
        head, _, rest = ln.partition(':')
        head = head.strip()
        if head == 'discount':
            gamma = float(rest)
        elif head == 'values':
            pass
        elif head in names:
            toks = rest.split()
            if len(toks) == 1 and toks[0].isnumeric():
                prefix = {'states': 's', 'actions': 'a', 'observations': 'o'}[head]
                names[head] = [f'{prefix}{k}' for k in range(int(toks[0]))]
            else:
                names[head] = toks
            ensure_tables()
        elif head == 'start':
            toks = rest.split()
            if not toks:
                toks = lines[i].split()
                i += 1
            assert len(toks) == len(names['states']), 'Not enough states in initial belief'
            start = np.array([float(t) for t in toks])
        elif head in ('T', 'O', 'R'):
            S, A, O = counts()
            fields = [f.strip() for f in rest.split(':')]
            value = None
            last = fields[-1].split()
            if len(last) > 1:                       # "... : x value"
                fields[-1] = last[0]
                value = float(last[1])
            keys = [f for f in fields if f != '']
            full = {'T': 3, 'O': 3, 'R': 4}[head]
            if value is None and len(keys) == full + 1 and is_number(keys[-1]):
                value = float(keys.pop())
            if value is None and len(keys) == full:   # fully specified entry, its single value on the next line
                value = float(lines[i].split()[0])
                i += 1
            acts = sel('actions', keys[0])
            if head == 'T':
                if len(keys) == 3:
                    for a in acts:
                        for s in sel('states', keys[1]):
                            for sp in sel('states', keys[2]):
                                T[s, a, sp] = value
                elif len(keys) == 2:
                    row = lines[i].split()
                    i += 1
                    for a in acts:
                        for s in sel('states', keys[1]):
                            T[s, a, :] = (np.ones(S) / S) if row[0] == 'uniform' else [float(t) for t in row]
                else:
                    first = lines[i].split()
                    if first[0] in ('uniform', 'identity'):
                        i += 1
                        for a in acts:
                            T[:, a, :] = (np.ones((S, S)) / S) if first[0] == 'uniform' else np.eye(S)
                    else:
                        mat = np.array([[float(t) for t in lines[i + k].split()] for k in range(S)])
                        i += S
                        for a in acts:
                            T[:, a, :] = mat
            elif head == 'O':
                if len(keys) == 3:
                    for a in acts:
                        for sp in sel('states', keys[1]):
                            for o in sel('observations', keys[2]):
                                Ob[sp, a, o] = value
                elif len(keys) == 2:
                    row = lines[i].split()
                    i += 1
                    for a in acts:
                        for sp in sel('states', keys[1]):
                            Ob[sp, a, :] = (np.ones(O) / O) if row[0] == 'uniform' else [float(t) for t in row]
                else:
                    first = lines[i].split()
                    if first[0] == 'uniform':
                        i += 1
                        for a in acts:
                            Ob[:, a, :] = np.ones((S, O)) / O
                    else:
                        mat = np.array([[float(t) for t in lines[i + k].split()] for k in range(S)])
                        i += S
                        for a in acts:
                            Ob[:, a, :] = mat
            else:  # R
                if len(keys) == 4:
                    for a in acts:
                        for s in sel('states', keys[1]):
                            for sp in sel('states', keys[2]):
                                for o in sel('observations', keys[3]):
                                    Rw[s, a, sp, o] = value
                elif len(keys) == 3:
                    row = [float(t) for t in lines[i].split()]
                    i += 1
                    for a in acts:
                        for s in sel('states', keys[1]):
                            for sp in sel('states', keys[2]):
                                Rw[s, a, sp, :] = row
                elif len(keys) == 2:
                    mat = np.array([[float(t) for t in lines[i + k].split()] for k in range(S)])
                    i += S
                    for a in acts:
                        for s in sel('states', keys[1]):
                            Rw[s, a, :, :] = mat
                else:
                    raise Exception('Need more than 1 parameter for rewards')

    params = dict(states=names['states'], actions=names['actions'], observations=names['observations'],
                  transitions=T, observation_table=Ob, rewards=Rw)
    if start is not None:
        params['start_probabilities'] = start
    return Model(**params), PBVI_Solver(gamma=gamma)
