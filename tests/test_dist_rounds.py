"""The round protocol of ``dist.sharded_backup``: every message carries a status, the ranks agree on an out-of-memory
and redo the round with half the chunk, a shard above the engine's block limit takes several rounds, and whatever
the rounds were the result is the single-process value function (rows bit for bit, row order, actions).

CPU tests: gloo ranks in fresh child processes over a NumPy stand-in for the engine calls of the sharded path (its
backup is the host mirror's statements, so the single-process reference is ``PBVI_Solver._backup_numpy``).  GPU tests:
two ranks with one HIP engine each on the one GPU (``tests/dist_rounds_check.py`` holds their code).  Every wait has a
time limit: a hang shows as a failure, never as a stuck suite."""
import ctypes
import datetime
import os
import socket
import subprocess
import sys
import time

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import REPO

GRID = os.path.join(REPO, 'tests', 'golden', 'models', '4x3.95-no_loop_2_grid.POMDP')
WORLD_LIMIT_S = 30            # per world; the collectives' own time limit is the same
GAMMA = 0.95
N_ALPHA = 9


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


# --------------------------------------------------------------------------- #
# inputs (rebuilt from seeds in every process) and the single-process reference
# --------------------------------------------------------------------------- #
def _inputs(n_total, dup=(), extra_alpha=0):
    """The 4x3 grid, ``N_ALPHA (+ extra_alpha)`` random alpha rows and ``n_total`` random beliefs; ``dup``: pairs
    ``(dst, src)``, belief ``dst`` becomes a copy of belief ``src``."""
    from pomdp_pbvi_exploration_amd import load_POMDP_file
    model, _ = load_POMDP_file(GRID)
    rng = np.random.default_rng(5)
    S = model.state_count
    alpha = rng.normal(size=(N_ALPHA + 3, S))[:N_ALPHA + extra_alpha]
    acts = rng.integers(0, model.action_count, N_ALPHA + 3)[:N_ALPHA + extra_alpha]
    bel = rng.random((max(n_total, 1), S))[:n_total]
    bel /= bel.sum(axis=1, keepdims=True)
    for dst, src in dup:
        bel[dst] = bel[src]
    return model, alpha, acts, bel


_REFERENCE = {}


def _reference(n_total, prune=False, dup=()):
    """(rows, actions) of the single-process backup; computed once per input and shared."""
    key = (n_total, prune, tuple(dup))
    if key not in _REFERENCE:
        from pomdp_pbvi_exploration_amd import PBVI_Solver, ValueFunction
        model, alpha, acts, bel = _inputs(n_total, dup)
        rows, a = PBVI_Solver(gamma=GAMMA)._backup_numpy(model, bel, alpha, prune)
        vf = ValueFunction(model, rows, a)
        out = (np.array(vf.alpha_vector_array), np.array(vf.actions))
        for x in out:
            x.setflags(write=False)
        _REFERENCE[key] = out
    return _REFERENCE[key]


# --------------------------------------------------------------------------- #
# NumPy stand-in for the engine calls of the sharded path
# --------------------------------------------------------------------------- #
class StandInEngine:
    """What ``dist.sharded_backup`` and ``dist.EngineShard`` call on an ``Engine``, on NumPy: the backup is the host
    mirror's statements (``PBVI_Solver._backup_numpy``), the exchange message has the engine's layout, rows are rebuilt
    from keys against the resident alpha set.  ``fits``: a run of more beliefs raises ``MemoryError`` after dropping
    everything resident, as the engine does."""
    device, dtype = 0, 'f64'

    def __init__(self, model, fits=None):
        self.model, self.S, self.O = model, model.state_count, model.observation_count
        self.fits = fits
        self.formulation = 'auto'
        self.alpha = self.block = self.result = None
        self.B = 0
        self._resident = {'alpha': None, 'belief': None}
        self.epoch, self.stored = 0, 0
        self.log = []

    # residency
    def sync_rows(self, which, objects, values_of, owner=None):
        rows = np.array([values_of(o) for o in objects])
        if which == 'alpha':
            self.alpha = rows
        else:
            self.block, self.B = rows, len(rows)

    @property
    def alpha_count(self):
        return 0 if self.alpha is None else len(self.alpha)

    def set_formulation(self, which):
        self.formulation = which

    def after_oom(self):
        self.alpha = self.block = self.result = None
        self.B = 0
        self.epoch += 1
        self.stored = 0
        self.log.append(('reset', None))

    def store_tag(self, which):
        return (id(self), which, self.epoch)

    # backup
    def _gamma(self, gamma):
        m, V = self.model, len(self.alpha)
        alpha_r = self.alpha[np.arange(V)[:, None, None, None], m.reachable_states[None, :, :, :]]
        return gamma * np.einsum('saor,vsar->aovs', m.reachable_transitional_observation_table, alpha_r)

    def run(self, gamma, prune=False):
        if self.fits is not None and self.B > self.fits:
            self.log.append(('oom', self.B))
            self.after_oom()
            raise MemoryError(f'stand-in: a block of {self.B or "too many"} beliefs does not fit')
        assert self.alpha is not None, 'the value function was not uploaded again after the failure'
        m, b, g = self.model, self.block, self._gamma(gamma)
        pick = np.argmax(np.tensordot(b, g, (1, 3)), axis=3)
        per_o = g[m.actions[None, :, None, None], m.observations[None, None, :, None], pick[:, :, :, None],
                  m.states[None, None, None, :]]
        alpha_a = m.expected_rewards_table.T + np.sum(per_o, axis=2)
        acts = np.argmax(np.einsum('bas,bs->ba', alpha_a, b), axis=1)
        keep = np.ones(len(acts), dtype=bool)
        if prune:
            rows = np.take_along_axis(alpha_a, acts[:, None, None], axis=1)[:, 0, :]
            keep = np.sum(b * rows, axis=1) > np.max(np.matmul(b, self.alpha.T), axis=1)
        keys = np.concatenate([acts[:, None], pick[np.arange(len(acts)), acts, :]], axis=1).astype(np.int32)
        seen, index = {}, []
        for k in map(tuple, keys):
            index.append(seen.setdefault(k, len(seen)))
        self.result = (np.array(list(seen), dtype=np.int32).reshape(len(seen), 1 + self.O), np.array(index), acts, keep)
        self.log.append(('run', self.B, self.formulation))
        return {}

    def exchange_size(self, per):
        return 1 + 3 * per + per * (1 + self.O)

    def fetch_exchange_into(self, ptr, per=None):
        per = self.B if per is None else per
        keys, index, acts, keep = self.result
        n = self.exchange_size(per)
        out = np.ctypeslib.as_array((ctypes.c_int32 * n).from_address(ptr))
        out[:] = 0
        out[0] = len(keys)
        out[1:1 + self.B] = index
        out[1 + per:1 + per + self.B] = acts
        out[1 + 2 * per:1 + 2 * per + self.B] = keep
        out[1 + 3 * per:1 + 3 * per + keys.size] = keys.reshape(-1)

    def assemble_rows_store(self, keys, gamma, want_rows=True):
        m, g = self.model, self._gamma(gamma)
        a = keys[:, 0]
        per_o = g[a[:, None, None], m.observations[None, :, None], keys[:, 1:, None], m.states[None, None, :]]
        rows = m.expected_rewards_table.T[a] + np.sum(per_o, axis=1)
        first, self.stored = self.stored, self.stored + len(rows)
        self.log.append(('store', len(rows)))
        return rows, first


# --------------------------------------------------------------------------- #
# the ranks
# --------------------------------------------------------------------------- #
def _run_case(case, rank, world, pdist):
    """One sharded ``PBVI_Solver.backup`` of this rank as ``case`` says; returns what the parent compares."""
    import copy
    from pomdp_pbvi_exploration_amd import Belief, BeliefSet, PBVI_Solver, ValueFunction
    model, alpha, acts, bel = _inputs(case['n_total'], case.get('dup', ()),
                                      extra_alpha=1 if case.get('diverged') == rank else 0)
    gm = copy.copy(model)                                   # a model that claims GPU residency, backed by the stand-in
    gm.is_on_gpu = True
    eng = gm._engine = StandInEngine(model, fits=case.get('fits', {}).get(rank))
    solver = PBVI_Solver(gamma=GAMMA)
    solver._belief_chunk = case.get('chunk')
    pdist.SHARD_BLOCK_LIMIT = case.get('limit', 65535)
    bs = BeliefSet(gm, [Belief(gm, r) for r in bel])
    vf = ValueFunction(gm, alpha, acts)
    out = {'error': '', 'round': -1, 'rows': np.zeros((0, model.state_count)), 'actions': np.zeros(0, dtype=np.int64)}
    try:
        got = solver.backup(gm, bs, vf, append=False, belief_dominance_prune=case.get('prune', False))
        out['rows'], out['actions'] = np.array(got.alpha_vector_array), np.array(got.actions)
        assert all(v._dev[0] == eng.store_tag('alpha') for v in got.alpha_vector_list)
        assert [v._dev[1] for v in got.alpha_vector_list] == list(range(len(got)))      # stored once, after the last round
    except MemoryError as e:
        out['error'], out['round'] = 'MemoryError', getattr(e, 'shard_round', -1)
    except pdist.ReplicaMismatch as e:
        out['error'] = 'ReplicaMismatch: ' + str(e)
    except NotImplementedError as e:
        out['error'] = 'NotImplementedError: ' + str(e)
    out['chunk'] = -1 if solver._belief_chunk is None else solver._belief_chunk
    kept = eng.log[max([i for i, x in enumerate(eng.log) if x[0] == 'reset'], default=-1) + 1:]
    out['runs'] = np.array([x[1] for x in kept if x[0] == 'run'], dtype=np.int64)    # (rounds before a reset were dropped)
    out['ooms'] = sum(1 for x in eng.log if x[0] == 'oom')
    out['stores'] = sum(1 for x in eng.log if x[0] == 'store')
    out['formulation'] = eng.formulation
    dist.barrier()                                          # the ranks are still in step, whatever the case did
    return out


def _worker(rank, world, port, out_dir, cases):
    sys.path.insert(0, REPO)
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world, timeout=datetime.timedelta(seconds=WORLD_LIMIT_S))
    try:
        from pomdp_pbvi_exploration_amd import dist as pdist
        from pomdp_pbvi_exploration_amd import set_quiet
        set_quiet(True)
        pdist.enable(True)
        for i, case in enumerate(cases):
            np.savez(os.path.join(out_dir, f'case{i}_rank{rank}.npz'), **_run_case(case, rank, world, pdist))
    finally:
        dist.destroy_process_group()


def _run_world(world, cases, tmp_path):
    """Run ``cases`` one after the other on ``world`` fresh gloo ranks; ``[case][rank] -> result``.  Children that are
    not done within the time limit are killed and the test fails."""
    ctx = mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), cases), nprocs=world, join=False)
    deadline = time.monotonic() + WORLD_LIMIT_S
    try:
        while not ctx.join(timeout=max(0.1, deadline - time.monotonic())):      # raises when a child failed
            if time.monotonic() >= deadline:
                pytest.fail(f'the {world} ranks were not done within {WORLD_LIMIT_S} s: they wait for one another')
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
            p.join(5)
    return [[dict(np.load(os.path.join(tmp_path, f'case{i}_rank{r}.npz'))) for r in range(world)] for i in range(len(cases))]


def _assert_equals_reference(results, case):
    want_rows, want_acts = _reference(case['n_total'], case.get('prune', False), case.get('dup', ()))
    for r, got in enumerate(results):
        assert str(got['error']) == '', (case, r, str(got['error']))
        assert got['rows'].shape == want_rows.shape, (case, r, got['rows'].shape, want_rows.shape)
        assert np.array_equal(got['rows'], want_rows), (case, r)                   # bit for bit, in order
        assert np.array_equal(got['actions'], want_acts), (case, r)
        assert got['stores'] == (1 if len(want_rows) else 0), (case, r)            # rows assembled once, not per round


# --------------------------------------------------------------------------- #
# CPU tests
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('world', [2, 3])
def test_one_rank_out_of_memory_ranks_agree_and_retry(tmp_path, world):
    """One rank's engine raises ``MemoryError`` for more than n beliefs, n chosen for exactly one and exactly two
    halvings (per = 12: 12 -> 6, 12 -> 6 -> 3).  Every rank returns the single-process value function within the time
    limit, all ranks settle on the same chunk, only the limited rank saw a failure, and everybody's value function was
    uploaded again after it.

    FAILS ON THE PARENT COMMIT: there the failing rank leaves ``sharded_backup`` with its ``MemoryError`` before the
    collective and the others wait for it until the backend's time limit."""
    n_total = 12 * world - (1 if world == 3 else 0)          # world 3: ragged, the limited (last) rank holds 11
    last = world - 1
    cases = [{'n_total': n_total, 'fits': {last: 6}}, {'n_total': n_total, 'fits': {last: 4}},
             {'n_total': n_total, 'fits': {0: 4}, 'prune': True}]
    res = _run_world(world, cases, tmp_path)
    for case, results, chunk, ooms in zip(cases, res, (6, 3, 3), (1, 2, 2)):
        _assert_equals_reference(results, case)
        limited = next(iter(case['fits']))
        for r, got in enumerate(results):
            assert got['chunk'] == chunk, (case, r, got['chunk'])
            assert got['ooms'] == (ooms if r == limited else 0)
            assert got['runs'].max() <= chunk and got['runs'].sum() == min(12, n_total - 12 * r)
            assert str(got['formulation']) == 'auto'                               # the caller's setting is back


def test_out_of_memory_at_chunk_one_raises_on_every_rank_from_the_same_round(tmp_path):
    """One rank never fits anything: 3 -> 2 -> 1, and the round that fails at one belief per rank (the third, index 2)
    raises ``MemoryError`` on every rank.  The barrier behind it completes: the ranks are still in step.  A later
    backup of the same group works."""
    cases = [{'n_total': 6, 'fits': {1: 0}}, {'n_total': 6}]
    res = _run_world(2, cases, tmp_path)                     # (_run_case ends with dist.barrier(): done means in step)
    assert [str(g['error']) for g in res[0]] == ['MemoryError'] * 2
    assert [int(g['round']) for g in res[0]] == [2, 2]
    assert [int(g['ooms']) for g in res[0]] == [0, 3]
    _assert_equals_reference(res[1], cases[1])


@pytest.mark.parametrize('world', [2, 3])
def test_rounds_equal_one_round(tmp_path, world):
    """No failure, the chunk forced to 1, 2 and ``per``: every result is the single-process one, so they equal one
    another.  13 beliefs split raggedly (7 + 6, 5 + 5 + 3); with fewer beliefs than ranks the last rank has none."""
    cases = []
    for n_total in (13, world - 1):
        per = -(-n_total // world)
        for chunk in sorted({1, 2, per}):
            cases.append({'n_total': n_total, 'chunk': chunk})
    cases.append({'n_total': 13, 'chunk': 2, 'prune': True})
    cases.append({'n_total': 13})                           # one round, as before
    res = _run_world(world, cases, tmp_path)
    for case, results in zip(cases, res):
        _assert_equals_reference(results, case)
        for r, got in enumerate(results):
            have = max(0, min(case['n_total'] - r * -(-case['n_total'] // world), -(-case['n_total'] // world)))
            assert got['runs'].sum() == have and got['ooms'] == 0
            if 'chunk' in case and have:
                assert got['runs'].max() <= case['chunk']
    assert len(res[-1][0]['runs']) == 1 and len(res[0][0]['runs']) == -(-13 // world)    # one round; a round per belief


def test_shard_above_the_block_limit_takes_several_rounds(tmp_path):
    """The engine's block limit, patched to 5 in the ranks: 12 beliefs per rank go through in rounds of 5, 5 and 2 --
    no ``NotImplementedError`` -- and the chunk is not remembered as a memory limit."""
    cases = [{'n_total': 24, 'limit': 5}, {'n_total': 23, 'limit': 5, 'prune': True}]
    res = _run_world(2, cases, tmp_path)
    for case, results in zip(cases, res):
        _assert_equals_reference(results, case)
        assert all(g['chunk'] == -1 for g in results)
    assert res[0][0]['runs'].tolist() == [5, 5, 2] and res[0][1]['runs'].tolist() == [5, 5, 2]
    assert res[1][1]['runs'].tolist() == [5, 5, 1]
    import inspect
    from pomdp_pbvi_exploration_amd import dist as pdist
    assert 'NotImplementedError' not in inspect.getsource(pdist.sharded_backup)


def test_status_difference_is_not_a_replica_mismatch(tmp_path):
    """The trailer check: ranks whose statuses differ hold the same problem; an out-of-memory rank, whose engine holds
    no alpha set any more, is excused from (|V|, fingerprint) and excuses the others; a different n_total, |V| or
    fingerprint, or a first word that is no status, is named as before.  Then on two ranks: a value function with one
    more row on rank 1 raises ``ReplicaMismatch`` on both, each naming the other; a rank that reports out of memory (case
    two) does not."""
    from pomdp_pbvi_exploration_amd import dist as pdist
    tv = pdist.trailer_values
    mine = tv(40, 9, 77)
    assert mine.tolist() == [0x50425649, 40, 9, 77] and len(mine) == pdist.TRAILER     # all fine: the message of before

    def check(mine, *others):
        pdist.check_trailers(np.stack([mine, *others]), 0, mine)

    check(mine, tv(40, 9, 77, pdist.STATUS_MORE), tv(40, 0, 0, pdist.STATUS_OOM))
    check(tv(40, 0, 0, pdist.STATUS_OOM), tv(40, 9, 77), tv(40, 9, 77, pdist.STATUS_MORE))
    assert pdist.trailer_statuses(np.stack([mine, tv(40, 0, 0, pdist.STATUS_OOM)]), 0).tolist() == [0, 1]
    for bad in (tv(40, 10, 77), tv(41, 9, 77), tv(40, 9, 78), tv(40, 10, 77, pdist.STATUS_MORE),
                tv(41, 0, 0, pdist.STATUS_OOM), tv(40, 9, 77, 3), tv(40, 9, 77, -1)):
        with pytest.raises(pdist.ReplicaMismatch, match='rank 1 sent'):
            check(mine, bad)
    with pytest.raises(pdist.ReplicaMismatch, match='rank 0 sent'):
        pdist.check_trailers(np.stack([tv(41, 9, 77), tv(40, 0, 0, pdist.STATUS_OOM)]), 0, tv(40, 0, 0, pdist.STATUS_OOM))

    cases = [{'n_total': 8, 'diverged': 1}, {'n_total': 8, 'fits': {1: 2}}]
    res = _run_world(2, cases, tmp_path)
    for r, got in enumerate(res[0]):
        assert str(got['error']).startswith(f'ReplicaMismatch: sharded backup: rank {1 - r} sent'), str(got['error'])
    _assert_equals_reference(res[1], cases[1])
    assert [int(g['ooms']) for g in res[1]] == [0, 1]


def test_equal_keys_of_different_rounds_and_ranks_are_one_row(tmp_path):
    """12 beliefs on two ranks in chunks of 3.  Belief 4 copies belief 0 (same rank, next round), belief 9 copies
    belief 1 (other rank, later round), belief 6 copies belief 5 (across the shard boundary): each key is one row, at
    the position of its first occurrence in global belief order."""
    from pomdp_pbvi_exploration_amd import PBVI_Solver
    dup = ((4, 0), (9, 1), (6, 5))
    case = {'n_total': 12, 'chunk': 3, 'dup': dup}
    res = _run_world(2, [case], tmp_path)[0]
    _assert_equals_reference(res, case)
    # the expectation spelled out: per-belief rows of the whole set, distinct ones in order of first occurrence
    model, alpha, _, bel = _inputs(12, dup)
    rows, acts, _ = PBVI_Solver(gamma=GAMMA)._backup_numpy(model, bel, alpha, False, return_mask=True)
    order, seen = [], set()
    for i, row in enumerate(rows):
        if row.tobytes() not in seen:
            seen.add(row.tobytes())
            order.append(i)
    assert not {4, 9, 6} & set(order) and len(order) <= 9
    for got in res:
        assert np.array_equal(got['rows'], rows[order]) and np.array_equal(got['actions'], acts[order])
        assert got['runs'].tolist() == [3, 3]


# --------------------------------------------------------------------------- #
# GPU tests: two ranks, one HIP engine each, on the one GPU (gloo carries the exchange)
# --------------------------------------------------------------------------- #
CHILD_LIMIT_S = 120


def _run_gpu_ranks(mode, tmp_path):
    """Start the two ranks of ``tests/dist_rounds_check.py`` as fresh processes, each under its own time limit.  A child
    that ends with a fault, an abort or at its time limit fails the test at once: the other one is killed and nothing
    else is started."""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'dist_rounds_check.py')
    port = _free_port()
    procs, logs = [], []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE='2')
        logs.append(open(tmp_path / f'rank{rank}.log', 'w+'))
        procs.append(subprocess.Popen([sys.executable, script, mode, str(tmp_path)], env=env, stdout=logs[-1],
                                      stderr=subprocess.STDOUT))
    deadline = time.monotonic() + CHILD_LIMIT_S
    codes = [None, None]
    try:
        while any(c is None for c in codes):
            for r, p in enumerate(procs):
                if codes[r] is None:
                    try:
                        codes[r] = p.wait(timeout=0.2)
                    except subprocess.TimeoutExpired:
                        if time.monotonic() >= deadline:
                            codes[r] = 'time limit'
            if any(c not in (None, 0) for c in codes):
                break
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait(10)
    text = []
    for r, f in enumerate(logs):
        f.seek(0)
        text.append(f'--- rank {r} (exit {codes[r]}) ---\n' + f.read()[-4000:])
        f.close()
    text = '\n'.join(text)
    print(text)
    assert codes == [0, 0], text
    return text


@pytest.mark.gpu
def test_engine_rank_under_a_memory_cap_retries_in_smaller_rounds(tmp_path):
    """S = 600 olfactory model (H = 15, W = 40, R = 1), fp64 engines, 37 alpha-vectors, 40 beliefs on two ranks.  Rank 1
    runs under a cap of its engine's device bytes (``pbvi_debug_alloc_limit``: refused by the engine's own bookkeeping,
    before any allocation) under which its 20-belief block fails and a 10-belief one fits; the cap lies strictly
    between the footprints the child measured without a cap just before (both and the cap are in its log; if they fall
    into the same MiB the child doubles B -- see ``dist_rounds_check.py``).  Both ranks return the alpha set of the
    single-process backup on the same GPU, rows bit for bit, same actions, having agreed on the smaller chunk."""
    text = _run_gpu_ranks('cap', tmp_path)
    assert text.count('sharded rounds ok') == 2
    assert 'footprint' in text and 'cap ' in text


@pytest.mark.gpu
def test_engine_rounds_of_seven_equal_one_round(tmp_path):
    """The same model and inputs, no cap, the chunk forced to 7 on both ranks (rounds of 7, 7, 6): identical to the
    one-round sharded result."""
    text = _run_gpu_ranks('chunk7', tmp_path)
    assert text.count('sharded rounds ok') == 2
