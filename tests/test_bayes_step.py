"""The Bayes-step entry points and the belief-side projection on irregular models.

``pbvi_belief_update``, ``pbvi_beliefs_advance``, ``pbvi_belief_walk`` / ``pbvi_belief_walk_keys`` and the belief-side
formulation of the backup (``k_push_project``) all pull through the inverse transition lists of
``engine.hip::build_inverse_lists``.  The older tests run them on the olfactory grid, where every list has the same
handful of entries.  Here: the 60 random models of ``test_random_models_against_the_oracle`` (lists of 0 to 132 entries)
and hand-built structures with one list of S entries beside empty ones (hub), probability-0 padding (ragged), the same
source state twice in one list (duplicate) and R = 1 identity transitions -- each against ``orc.belief_update`` (fp64
``np.bincount``), chained on the host for walks and advances.  f32 engines: model tables and beliefs rounded to f32 first.

Bounds (the ones the older tests of these entry points use): update / advance rtol 1e-12 (f64 engines) and 2e-6 (f32
engines), atol 1e-12; walk rows 1e-13 and 1e-6.
"""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch            # noqa: F401  torch first: its HIP runtime has to be the one that opens the device (device-pointer test)

from conftest import REPO
from model_cases import (N_RANDOM_CASES, STRUCTURES, assert_backup_matches_oracle, f32_round, first_possible_observation,
                         hub_model, in_degrees, ragged_model, random_case, sparse_beliefs, update_longdouble)
from oracle import pbvi_oracle as orc
from pomdp_pbvi_exploration_amd.engine import Engine
from pomdp_pbvi_exploration_amd.mdp import _RowKey

gpu = pytest.mark.gpu

UPDATE_RTOL = {'f64': 1e-12, 'f32': 2e-6}
UPDATE_ATOL = 1e-12
WALK_TOL = {'f64': 1e-13, 'f32': 1e-6}

SIZES_S = [2, 31, 33, 255, 256, 257, 600]
SIZES_B = [1, 3, 257]
WALK_LENGTHS = [1, 7, 8, 9, 41]          # 8 = first length copied out in four overlapped chunks; 9 and 41: n % 4 != 0
RESTARTS = ['none', 'all', 'last', 'two']
WALK_SEEDS = [0, 1, 2]
ENGINE_KINDS = ['f64', 'f32_rto64', 'f32_plain']


# --------------------------------------------------------------------------- #
# Helpers
# --------------------------------------------------------------------------- #
def update_actions(seed, A, B):
    return np.random.default_rng(1000 + seed).integers(0, A, B)


def update_reference(b, acts, rs, rto):
    """``(obs [B], ref [B,S])``: per row the lowest observation with a finite oracle result (-1: none) and that result."""
    obs = np.empty(len(b), dtype=np.int64)
    ref = np.zeros_like(b)
    for i in range(len(b)):
        obs[i], nb = first_possible_observation(b[i], acts[i], rs, rto)
        if nb is not None:
            ref[i] = nb
    return obs, ref


def assert_update_matches(out, ref, dtype, tag):
    """Values, row sums and the zero pattern of a batch of updated beliefs."""
    out = np.asarray(out, dtype=np.float64)
    np.testing.assert_allclose(out, ref, rtol=UPDATE_RTOL[dtype], atol=UPDATE_ATOL, err_msg=str(tag))
    # the rows are sums of S non-negative terms rounded once to the engine's type: |sum - 1| <= S * ulp/2 at worst
    eps = 2.0 ** -53 if dtype == 'f64' else 2.0 ** -24
    np.testing.assert_allclose(out.sum(axis=1), 1.0, rtol=0, atol=UPDATE_RTOL[dtype] + out.shape[1] * eps, err_msg=str(tag))
    # states without a predecessor, or with weightless ones only, hold exact zeros
    if dtype == 'f64':
        assert np.array_equal(out == 0, ref == 0), tag
    else:
        assert np.all(out[ref == 0] == 0), tag


def structure_case(name, S, dtype):
    """``(rs, rto, er, A, O, R)`` of a hand-built structure, tables as an engine of ``dtype`` holds them."""
    rs, rto = STRUCTURES[name](S)
    if dtype == 'f32':
        rto = f32_round(rto)
    _, A, O, R = rto.shape
    return rs, rto, np.zeros((S, A)), A, O, R


def restart_pattern(kind, n):
    r = np.zeros(n, dtype=bool)
    if kind == 'all':
        r[:] = True
    elif kind == 'last':
        r[n - 1] = True
    elif kind == 'two':                  # two consecutive restarts mid-walk (n = 41: steps 20 and 21, across a chunk end)
        r[n // 2] = True
        r[min(n // 2 + 1, n - 1)] = True
    return r


def host_walk(rs, rto, b0, acts, restart):
    """The reference chain: ``(acts, obs, rows [n,S])`` with every step through the lowest possible observation; an
    action that admits none (a zero-mass step) is replaced by the next one that does."""
    A = rto.shape[1]
    acts = np.array(acts, dtype=np.int64)
    obs = np.zeros(len(acts), dtype=np.int64)
    rows, b = [], b0
    for i in range(len(acts)):
        base = b0 if restart[i] else b
        for k in range(A):
            a = (acts[i] + k) % A
            o, nb = first_possible_observation(base, a, rs, rto)
            if o >= 0:
                break
        assert o >= 0, 'no possible (action, observation) from this belief'
        acts[i], obs[i], b = a, o, nb
        rows.append(nb)
    return acts, obs, np.array(rows)


_WALK_MODELS = {}


def walk_model(case):
    """``(S, A, O, R, rs, rto, er, b0)`` of a walk case: a random seed or ``'ragged'``."""
    if case not in _WALK_MODELS:
        if case == 'ragged':
            S = 257
            rs, rto = ragged_model(S)
            _, A, O, R = rto.shape
            er = np.zeros((S, A))
            b0 = sparse_beliefs(np.random.default_rng(5), 1, S)[0]
        else:
            S, A, O, R, rs, rto, er, _, b, _ = random_case(case)
            b0 = b[0]
        _WALK_MODELS[case] = (S, A, O, R, rs, rto, er, b0)
    return _WALK_MODELS[case]


_WALK_REFS = {}


def walk_reference(case, rounded, n, kind):
    """Host chain of a walk case, computed once per (case, table precision, length, restart pattern)."""
    key = (case, rounded, n, kind)
    if key not in _WALK_REFS:
        S, A, O, R, rs, rto, er, b0 = walk_model(case)
        if rounded:
            rto = f32_round(rto)
        acts = np.random.default_rng(4000 + n).integers(0, A, n)
        _WALK_REFS[key] = host_walk(rs, rto, b0, acts, restart_pattern(kind, n))
    return _WALK_REFS[key]


def walk_engine(kind, case):
    """f64 engine; f32 engine holding the fp64 table for the walk (``pbvi_engine_set_rto_f64``, what ``Engine`` does when
    it is given an fp64 table); f32 engine without it (given an f32 table)."""
    S, A, O, R, rs, rto, er, _ = walk_model(case)
    if kind == 'f64':
        return Engine(S, A, O, R, rs, rto, er, dtype='f64')
    if kind == 'f32_rto64':
        return Engine(S, A, O, R, rs, rto, er, dtype='f32')
    return Engine(S, A, O, R, rs, rto.astype(np.float32), er, dtype='f32')


def walk_bound(kind):
    return WALK_TOL['f64' if kind == 'f64' else 'f32']


def rows_digest(rows):
    return hashlib.sha256(np.ascontiguousarray(rows, dtype=np.float64).tobytes()).hexdigest()


def hash_walk_digests():
    """sha256 of the rows of the n = 41 walk of seed 0 (restart pattern 'two') per engine kind: what the parent compares with
    a child process that runs the two-kernel chain."""
    out = []
    for kind in ENGINE_KINDS:
        acts, obs, _ = walk_reference(0, kind == 'f32_plain', 41, 'two')
        eng = walk_engine(kind, 0)
        got, _ = eng.belief_walk(walk_model(0)[7], acts, obs, restart_pattern('two', 41))
        out.append(rows_digest(got))
        eng.close()
    return out


ADVANCE_SEEDS = [0, 2, 3]                 # random cases with B = 334, 405, 320: blocks the engine sorts internally


# --------------------------------------------------------------------------- #
# CPU: the input conditions the GPU tests rely on
# --------------------------------------------------------------------------- #
@pytest.mark.parametrize('rounded', [False, True])
def test_every_random_pair_has_a_possible_observation(rounded):
    """All 16 619 (belief, action) pairs of the 60 random cases have an observation whose update is finite, with the tables
    in fp64 and rounded to f32: the GPU tests leave no row out."""
    pairs = 0
    for seed in range(N_RANDOM_CASES):
        S, A, O, R, rs, rto, er, alpha, b, gamma = random_case(seed)
        if rounded:
            rto, b = f32_round(rto, b)
        obs, _ = update_reference(b, update_actions(seed, A, len(b)), rs, rto)
        assert (obs >= 0).all(), seed
        pairs += len(b)
    assert pairs == 16619


def test_random_cases_hold_long_and_empty_inverse_lists():
    """What makes the random cases worth running: lists far longer than the grid's five entries, and states that no
    state reaches under some action."""
    longest, empty, total = 0, 0, 0
    for seed in range(N_RANDOM_CASES):
        deg = in_degrees(random_case(seed)[4])
        longest = max(longest, int(deg.max()))
        empty += int((deg == 0).sum())
        total += deg.size
    assert longest == 132
    assert 0.03 < empty / total < 0.08
    assert [random_case(s)[8].shape[0] for s in ADVANCE_SEEDS] == [334, 405, 320]     # > 256: sorted in either engine type


@pytest.mark.parametrize('S', SIZES_S)
def test_hand_built_structures_are_what_they_claim(S):
    rs, rto = hub_model(S)
    deg = in_degrees(rs)
    assert (deg[:, S - 1] >= S).all()
    if S > 4:
        assert (deg == 0).any()
    rs, rto = ragged_model(S)
    if S > 4:
        assert (rto.sum(axis=2) == 0).any() and (rto.sum(axis=2) > 0).any()        # padded entries: probability 0
    for a in range(rs.shape[1]):
        for s in range(0, S, max(1, S // 7)):
            assert len(set(rs[s, a])) == rs.shape[2]                                # padding never repeats a successor
    rs, rto = STRUCTURES['duplicate'](S)
    assert np.array_equal(rs[:, :, 0], rs[:, :, 1]) and (rto > 0).all()
    rs, rto = STRUCTURES['identity'](S)
    assert rs.shape[2] == 1 and np.array_equal(rs[:, 0, 0], np.arange(S))
    for name in STRUCTURES:
        rs, rto = STRUCTURES[name](S)
        np.testing.assert_allclose(rto.sum(axis=(2, 3)), 1.0, atol=1e-12)


def test_walk_references_are_finite_and_restart_where_asked():
    """Every walk case has a host chain without a zero-mass step; a restarted step is the update of b0."""
    for case in WALK_SEEDS + ['ragged']:
        S, A, O, R, rs, rto, er, b0 = walk_model(case)
        for rounded in (False, True):
            t = f32_round(rto) if rounded else rto
            for n in WALK_LENGTHS:
                for kind in RESTARTS:
                    acts, obs, rows = walk_reference(case, rounded, n, kind)
                    assert rows.shape == (n, S) and np.isfinite(rows).all()
                    for i in np.flatnonzero(restart_pattern(kind, n)):
                        assert np.array_equal(rows[i], orc.belief_update(b0, int(acts[i]), int(obs[i]), rs, t))
    assert restart_pattern('two', 41).nonzero()[0].tolist() == [20, 21]
    assert restart_pattern('two', 1).tolist() == [True] and restart_pattern('last', 9).nonzero()[0].tolist() == [8]


def test_longdouble_restatement_agrees_with_the_oracle():
    """The yardstick a widened bound would have to come from: ``orc.belief_update`` is within a few ulp of the same update
    accumulated in ``np.longdouble``."""
    worst = 0.0
    for seed in (0, 1, 2):
        S, A, O, R, rs, rto, er, alpha, b, gamma = random_case(seed)
        acts = update_actions(seed, A, len(b))
        for i in range(min(len(b), 20)):
            o, nb = first_possible_observation(b[i], acts[i], rs, rto)
            ld = update_longdouble(b[i], int(acts[i]), o, rs, rto)
            nz = nb > 0
            assert np.array_equal(nz, ld > 0)
            worst = max(worst, float(np.max(np.abs(nb[nz] - ld[nz]) / ld[nz])))
    assert worst < 1e-14


# --------------------------------------------------------------------------- #
# 1. pbvi_belief_update on the random models
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_belief_update_on_random_models(dtype):
    """Every belief of the 60 random cases through one Bayes step (random action, lowest possible observation): values,
    row sums and exact zeros against the oracle."""
    for seed in range(N_RANDOM_CASES):
        S, A, O, R, rs, rto, er, alpha, b, gamma = random_case(seed)
        if dtype == 'f32':
            rto, b = f32_round(rto, b)
        acts = update_actions(seed, A, len(b))
        obs, ref = update_reference(b, acts, rs, rto)
        assert (obs >= 0).all(), seed
        eng = Engine(S, A, O, R, rs, rto, er, dtype=dtype)
        out = eng.belief_update(b, acts, obs)
        eng.close()
        assert_update_matches(out, ref, dtype, seed)


# --------------------------------------------------------------------------- #
# 2. hand-built structures
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('S', SIZES_S)
@pytest.mark.parametrize('name', list(STRUCTURES))
def test_belief_update_on_hand_built_structures(name, S, dtype):
    rs, rto, er, A, O, R = structure_case(name, S, dtype)
    eng = Engine(S, A, O, R, rs, rto, er, dtype=dtype)
    for B in SIZES_B:
        rng = np.random.default_rng(100 * S + B)
        b = sparse_beliefs(rng, B, S)
        if dtype == 'f32':
            b = f32_round(b)
        acts = rng.integers(0, A, B)
        obs = rng.integers(0, O, B)                        # every observation is possible in these models
        ref = np.stack([orc.belief_update(b[i], int(acts[i]), int(obs[i]), rs, rto) for i in range(B)])
        assert np.isfinite(ref).all()
        assert_update_matches(eng.belief_update(b, acts, obs), ref, dtype, (name, S, B))
    eng.close()


@gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_impossible_observation_gives_a_nan_row(dtype):
    """Observation 2 never follows action 0: those rows are NaN from end to end, exactly where the oracle's are, and their
    neighbours in the batch are untouched."""
    S = 257
    rs, rto = hub_model(S, A=2, O=3)
    rto[:, 0, 2, :] = 0.0
    if dtype == 'f32':
        rto = f32_round(rto)
    rng = np.random.default_rng(11)
    b = sparse_beliefs(rng, 6, S)
    if dtype == 'f32':
        b = f32_round(b)
    acts = np.array([0, 1, 0, 0, 1, 0])
    obs = np.array([2, 2, 0, 2, 1, 1])
    with np.errstate(invalid='ignore', divide='ignore'):
        ref = np.stack([orc.belief_update(b[i], int(acts[i]), int(obs[i]), rs, rto) for i in range(6)])
    assert np.isnan(ref).all(axis=1).tolist() == [True, False, False, True, False, False]
    eng = Engine(S, 2, 3, 2, rs, rto, np.zeros((S, 2)), dtype=dtype)
    out = eng.belief_update(b, acts, obs).astype(np.float64)
    eng.close()
    assert np.array_equal(np.isnan(out), np.isnan(ref))
    ok = ~np.isnan(ref).any(axis=1)
    assert_update_matches(out[ok], ref[ok], dtype, 'possible rows')


# --------------------------------------------------------------------------- #
# 3. pbvi_beliefs_advance
# --------------------------------------------------------------------------- #
def keep_mask(kind, B):
    k = np.zeros(B, dtype=bool)
    if kind == 'all':
        k[:] = True
    elif kind == 'alternating':
        k[::2] = True
    elif kind == 'first':
        k[0] = True
    elif kind == 'last':
        k[B - 1] = True
    return k


def advance_case(case, dtype):
    if case == 'hub':
        S, B = 600, 257
        rs, rto, er, A, O, R = structure_case('hub', S, dtype)
        rng = np.random.default_rng(21)
        er = rng.normal(size=(S, A))
        b, alpha, gamma = sparse_beliefs(rng, B, S), rng.normal(size=(37, S)), 0.9
    else:
        S, A, O, R, rs, rto, er, alpha, b, gamma = random_case(case)
    if dtype == 'f32':
        rto, er, alpha, b = f32_round(rto, er, alpha, b)
    return S, A, O, R, rs, rto, er, alpha, b, gamma


@gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('mask', ['all', 'alternating', 'first', 'last', 'none'])
@pytest.mark.parametrize('case', ADVANCE_SEEDS + ['hub'])
def test_advance_three_steps_then_value_max_and_backup(case, mask, dtype):
    """Three chained simulator steps on a block that starts internally sorted (B >= 256), each against the oracle applied
    to the block the engine held before the step: survivor order, values, zeros.  Then ``pbvi_value_max`` and one backup
    of the advanced block against the oracle on ``fetch_beliefs()``: zero maps and tile lists belong to the compacted
    block.  'none' drops every row at the third step (after two alternating ones): no block is resident afterwards."""
    S, A, O, R, rs, rto, er, alpha, b, gamma = advance_case(case, dtype)
    eng = Engine(S, A, O, R, rs, rto, er, dtype=dtype)
    eng.set_beliefs(b)
    prev = eng.fetch_beliefs().astype(np.float64)
    assert np.array_equal(prev, b)
    rng = np.random.default_rng(31)
    for step in range(3):
        B = len(prev)
        acts = rng.integers(0, A, B)
        obs, ref = update_reference(prev, acts, rs, rto)
        assert (obs >= 0).all()
        kind = mask if mask != 'none' else ('alternating' if step < 2 else 'none')
        keep = keep_mask(kind, B)
        nb = eng.advance_beliefs(acts, obs, None if (kind == 'all' and step == 1) else keep)
        assert nb == int(keep.sum()) == eng.B
        if nb == 0:
            with pytest.raises(ValueError):
                eng.max_value_resident()
            eng.close()
            return
        got = eng.fetch_beliefs().astype(np.float64)
        assert_update_matches(got, ref[keep], dtype, (case, mask, step))
        prev = got
    eng.set_alpha(alpha)
    val, idx = eng.max_value_resident()
    scores = prev @ alpha.T
    # exact maxima in fp64 whatever the engine's type; a dot product over S terms with sum |b| = 1 is good to
    # S * 2^-53 * max|alpha| in any order, on either side
    np.testing.assert_allclose(val, scores.max(axis=1), rtol=1e-12, atol=2 * S * 2.0 ** -53 * np.abs(alpha).max())
    np.testing.assert_allclose(scores[np.arange(len(prev)), idx], scores.max(axis=1), rtol=1e-12,
                               atol=2 * S * 2.0 ** -53 * np.abs(alpha).max())
    stats = eng.run(gamma)
    res = eng.fetch()
    assert stats['n_pairs'] == len(prev) * A * O
    want_rows, want_a, want_v = orc.backup_core(alpha, prev, rs, rto, er, gamma)
    assert_backup_matches_oracle(res, alpha, want_rows, want_a, want_v, dtype, (case, mask))
    eng.close()


# --------------------------------------------------------------------------- #
# 4. pbvi_belief_walk / pbvi_belief_walk_keys
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize('case', WALK_SEEDS + ['ragged'])
@pytest.mark.parametrize('kind', ENGINE_KINDS)
def test_walk_lengths_and_restarts(kind, case):
    """Walks of 1, 7, 8, 9 and 41 steps (8 switches to the four-chunk overlapped copy-out; 9 and 41 are no multiple of 4)
    with no restart, a restart at every step, at the last step only and at two consecutive steps: rows against the host
    chain, keys against ``_RowKey`` of the returned rows, store ids consecutive."""
    S, A, O, R, rs, rto, er, b0 = walk_model(case)
    eng = walk_engine(kind, case)
    tol = walk_bound(kind)
    expect_first = 0
    for n in WALK_LENGTHS:
        for pattern in RESTARTS:
            acts, obs, want = walk_reference(case, kind == 'f32_plain', n, pattern)
            restart = restart_pattern(pattern, n)
            got, first = eng.belief_walk(b0, acts, obs, None if pattern == 'none' else restart)
            tag = (kind, case, n, pattern)
            assert first == expect_first, tag
            expect_first += n
            np.testing.assert_allclose(got, want, rtol=tol, atol=tol * 1e-3, err_msg=str(tag))
            np.testing.assert_allclose(got.sum(axis=1), 1.0, rtol=0, atol=1e-12, err_msg=str(tag))
            keys = eng.belief_walk_keys(n)
            assert [int(k) for k in keys] == [int(_RowKey(r)) for r in got], tag
    eng.close()


@gpu
@pytest.mark.parametrize('kind', ENGINE_KINDS)
def test_walk_rows_survive_the_growth_of_the_store(kind):
    """A 7-step walk, then a 41-step one: the belief store is reallocated for the second.  The first walk's ids still
    select the first walk's rows, bit for bit in the engine's type."""
    case = 1
    b0 = walk_model(case)[7]
    eng = walk_engine(kind, case)
    a1, o1, _ = walk_reference(case, kind == 'f32_plain', 7, 'two')
    rows1, first1 = eng.belief_walk(b0, a1, o1, restart_pattern('two', 7))
    rows1 = rows1.copy()
    bytes1 = eng.device_bytes
    a2, o2, _ = walk_reference(case, kind == 'f32_plain', 41, 'none')
    rows2, first2 = eng.belief_walk(b0, a2, o2, None)
    assert first2 == first1 + 7 and eng.device_bytes > bytes1
    eng.select_beliefs(np.arange(first1, first1 + 7))
    assert np.array_equal(eng.fetch_beliefs(), rows1.astype(eng.np_dtype))
    eng.select_beliefs(np.arange(first2, first2 + 41))
    assert np.array_equal(eng.fetch_beliefs(), rows2.astype(eng.np_dtype))
    eng.close()


def _hip_runtimes_mapped():
    with open('/proc/self/maps') as f:
        return {line.split()[-1] for line in f if 'libamdhip64' in line}


@gpu
@pytest.mark.parametrize('n', [7, 41])
@pytest.mark.parametrize('kind', ENGINE_KINDS)
def test_walk_into_device_memory_equals_walk_into_host_memory(kind, n):
    """``out_beliefs`` in device memory (a torch tensor): one device-to-device copy instead of the staged (n < 8) or
    chunked (n >= 8) host delivery.  Same rows bit for bit, same keys."""
    case = 2
    S, A, O, R, rs, rto, er, b0 = walk_model(case)
    acts, obs, _ = walk_reference(case, kind == 'f32_plain', n, 'two')
    restart = restart_pattern('two', n).astype(np.uint8)
    eng = walk_engine(kind, case)
    host, first = eng.belief_walk(b0, acts, obs, restart)
    host_keys = eng.belief_walk_keys(n)
    # one HIP runtime in the process: a pointer of torch's allocator means the same to the engine
    assert len(_hip_runtimes_mapped()) == 1, _hip_runtimes_mapped()
    dev = torch.full((n, S), -1.0, dtype=torch.float64, device='cuda:0')
    torch.cuda.synchronize()
    a32, o32 = np.ascontiguousarray(acts, dtype=np.int32), np.ascontiguousarray(obs, dtype=np.int32)
    start = np.ascontiguousarray(b0, dtype=np.float64)
    f64p, i32p = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    first2 = eng._lib.pbvi_belief_walk(eng._h, start.ctypes.data_as(f64p), n, a32.ctypes.data_as(i32p), o32.ctypes.data_as(i32p),
                                       restart.ctypes.data_as(C.POINTER(C.c_uint8)), C.cast(dev.data_ptr(), f64p))
    assert first2 == first + n
    assert np.array_equal(dev.cpu().numpy(), host)
    assert np.array_equal(eng.belief_walk_keys(n), host_keys)
    eng.close()


@gpu
def test_fused_chain_gives_the_doubles_of_the_two_kernel_chain():
    """The comments at ``k_walk_fused`` promise the doubles of ``k_walk_push`` + ``k_walk_norm``.  ``PBVI_WALK_TWO_KERNELS``
    is read once per process, so the other chain runs in a fresh child: same 41-step walk on each kind of engine, sha256
    of the rows."""
    env = dict(os.environ)
    if 'PBVI_WALK_TWO_KERNELS' in env:       # this process runs the two-kernel chain: the child runs the fused one
        del env['PBVI_WALK_TWO_KERNELS']
    else:
        env['PBVI_WALK_TWO_KERNELS'] = '1'
    mine = hash_walk_digests()
    child = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'walk_hash_check.py')], env=env, cwd=REPO,
                           stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stdout + child.stderr
    theirs = [line.split()[1] for line in child.stdout.splitlines() if line.startswith('walk-sha256 ')]
    assert len(theirs) == len(ENGINE_KINDS), child.stdout + child.stderr
    assert theirs == mine


# --------------------------------------------------------------------------- #
# 5. belief-side formulation on irregular models
# --------------------------------------------------------------------------- #
def _belief_side_backup(S, A, O, R, rs, rto, er, alpha, b, gamma, dtype, tag):
    """One backup with the beliefs projected (``k_push_project``) against ``orc.backup_core``, and the value maxima it
    offers against ``orc.max_value_per_belief``."""
    if dtype == 'f32':
        rto, er, alpha, b = f32_round(rto, er, alpha, b)
    want_rows, want_a, want_v = orc.backup_core(alpha, b, rs, rto, er, gamma)
    eng = Engine(S, A, O, R, rs, rto, er, dtype=dtype)
    eng.set_formulation('belief')
    eng.set_alpha(alpha)
    eng.set_beliefs(b)
    st = eng.run(gamma)
    assert st['formulation'] == 2, tag
    res = eng.fetch()
    assert_backup_matches_oracle(res, alpha, want_rows, want_a, want_v, dtype, tag)
    out = np.empty(len(b), dtype=np.float64)
    rc = eng._lib.pbvi_backup_fetch_value_max(eng._h, out.ctypes.data_as(C.POINTER(C.c_double)))
    eng.close()
    if st['screened']:     # (PBVI_F64_SCREEN=always) a screened backup's GEMM rows are fp32: it offers no exact maxima
        assert rc == -4, tag
        return
    assert rc == 0, tag
    np.testing.assert_allclose(out, orc.max_value_per_belief(alpha, b), rtol=1e-12 if dtype == 'f64' else 1e-6, err_msg=str(tag))


@gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_belief_side_formulation_on_random_models(dtype):
    """The 60 random cases with the beliefs pushed through the inverse lists instead of the alpha-vectors pulled through
    the forward ones: the acceptance rule of ``test_random_models_against_the_oracle``, and the maxima that ride along."""
    if dtype == 'f64' and os.environ.get('PBVI_F64_SIMPLE'):
        pytest.skip('debug mode: the plain fp64 GEMM has no belief-side formulation')
    for seed in range(N_RANDOM_CASES):
        _belief_side_backup(*random_case(seed), dtype, seed)


@gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('name,S,B', [('hub', 600, 7), ('ragged', 257, 5)])
def test_belief_side_formulation_on_hand_built_structures(name, S, B, dtype):
    """B no multiple of 4 (beliefs per thread of ``k_push_project``) and S no multiple of 2048 (states per block).  160
    alpha-vectors: an f64 engine has a belief side only where its score GEMM is the MFMA one, B*A*O*V >= 4096."""
    if dtype == 'f64' and os.environ.get('PBVI_F64_SIMPLE'):
        pytest.skip('debug mode: the plain fp64 GEMM has no belief-side formulation')
    rs, rto, er, A, O, R = structure_case(name, S, 'f64')
    rng = np.random.default_rng(41)
    er = rng.normal(size=(S, A))
    _belief_side_backup(S, A, O, R, rs, rto, er, rng.normal(size=(160, S)), sparse_beliefs(rng, B, S), 0.95, dtype, name)
