"""The bits of every fp32 score-GEMM route, pinned: sha256 of the raw slab buffer (pbvi_debug_slabs) and of the backup's
outputs, plus the counters that tell which route ran, against tests/golden/score_slabs.json.

The file was recorded from the commit before the stream-K share walk, the kernel table and the launch arguments of
gemm.hip were refactored (2b34c47), on an MI355X with 256 CUs -- the stream-K shares, and with them the slab buffer's
size and the partial sums in it, depend on the number of persistent blocks.  The refactor had to reproduce it without
re-recording.  A later change that alters these bits on purpose must re-record the file and say why.

Each case is the smallest at which its kernel's walk meets a continuation tile and more than one m-tile (a-i), lists of
two entries (j), the non-persistent scheduler on a score GEMM (k: PBVI_GEMM_NO_STREAMK is read once per process, so a
child process) and the batched single-chunk launch of the dense projection (l: results only, its product buffer is not
exposed)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from pomdp_pbvi_exploration_amd.engine import Engine, debug_split_schedule
from score_cases import beliefs, random_model, shifted_model

pytestmark = pytest.mark.gpu

FILL = 0xA5
COUNTERS = ('score_tiles_run', 'score_split', 'fused_projection')
GOLDEN_FILE = os.path.join(GOLDEN, 'score_slabs.json')
CHILD_TAG = 'score-slabs-json '

REGULAR = (4097, 3, 1, 300, 300)
# case -> (kind, shape, settings)
CASES = {
    'a': ('r1', REGULAR, dict(regular=True, split='off', fused=False)),
    'b': ('r1', REGULAR, dict(regular=True, split='off', fused=True)),
    'c': ('r1', REGULAR, dict(regular=True, split='always', fused=True, schedule='parent')),
    'd': ('r1', REGULAR, dict(regular=True, split='always', fused=False, schedule='parent')),
    'e': ('r1', REGULAR, dict(regular=True, split='always', fused=True, schedule='pipelined')),
    'f': ('r1', REGULAR, dict(regular=True, split='always', fused=False, schedule='pipelined')),
    'g': ('r1', (1000, 2, 2, 512, 70), dict(regular=False, split='always', fused=True)),
    'h': ('rn', (4100, 2, 2, 2, 512, 70), {}),
    'i': ('rn', (9000, 1, 3, 5, 777, 40), {}),
    'j': ('short', (100, 2), {}),
    'k': ('child', REGULAR, {}),
    'l': ('dense', (520, 2, 2, 40, 70), {}),
}


def sha(x):
    x = np.ascontiguousarray(x)
    return hashlib.sha256(f'{x.dtype.str} {x.shape} '.encode() + x.tobytes()).hexdigest()


def digest(res, slabs=None):
    out = {k: sha(getattr(res, k)) for k in ('alpha', 'actions', 'best_alpha_ind', 'keep')}
    out.update({k: int(res.stats[k]) for k in COUNTERS})
    if slabs is not None:
        out['slabs'] = sha(slabs)
        out['slab_bytes'] = int(slabs.size)
    return out


def slab_run(eng, alpha, b, gamma, schedule='parent'):
    """test_split_schedule.run_both's method for one run: the buffer at its final size, every byte FILL, then the backup
    (no dominance stage: its GEMM would re-use the slab buffer)."""
    prev = debug_split_schedule(schedule)
    try:
        eng.backup_full(alpha, b, gamma)
        eng.debug_slabs_fill(FILL)
        res = eng.backup_full(alpha, b, gamma)
        return digest(res, eng.debug_slabs())
    finally:
        debug_split_schedule(prev)


def case_r1(shape, regular, split, fused, schedule='parent'):
    S, A, O, V, B = shape
    rng = np.random.default_rng(S + V)
    rs, rto, er = random_model(rng, S, A, O, regular)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    try:
        eng.set_formulation('alpha')
        eng.set_score_split(split)
        eng.set_fused_projection(fused)
        return slab_run(eng, alpha, b, 0.9, schedule)
    finally:
        eng.close()


def case_rn(shape):
    S, A, O, R, V, B = shape
    rng = np.random.default_rng(S + V + R)
    rs, rto, er = shifted_model(rng, S, A, O, R)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S)
    eng = Engine(S, A, O, R, rs, rto, er, dtype='f32')
    try:
        eng.set_formulation('alpha')
        eng.set_score_split('off')
        eng.set_fused_projection(2)
        return slab_run(eng, alpha, b, 0.9)
    finally:
        eng.close()


def case_short(shape):
    """test_split_schedule.test_short_segments: every tile list has k_tiles entries"""
    S, k_tiles = shape
    A, O, V, B = 2, 2, 13000, 40
    rng = np.random.default_rng(100 * S + k_tiles)
    rs, rto, er = random_model(rng, S, A, O, True)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S, density=0.5, support=min(S, 32 * k_tiles))
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32')
    try:
        eng.set_formulation('alpha')
        eng.set_score_split('always')
        eng.set_fused_projection(True)
        return slab_run(eng, alpha, b, 0.9)
    finally:
        eng.close()


def case_child(shape):
    """Case a in a fresh process with the stream-K scheduler switched off: one block per (pair, chunk of the list)."""
    env = dict(os.environ)
    env['PBVI_GEMM_NO_STREAMK'] = '1'
    child = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'score_slabs_child.py')], env=env, cwd=REPO,
                           stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stdout + child.stderr
    lines = [ln for ln in child.stdout.splitlines() if ln.startswith(CHILD_TAG)]
    assert len(lines) == 1, child.stdout + child.stderr
    return json.loads(lines[0][len(CHILD_TAG):])


def case_dense(shape):
    S, A, O, V, B = shape
    rng = np.random.default_rng(S + V)
    rs, rto, er = random_model(rng, S, A, O, False)
    alpha = rng.normal(scale=4.0, size=(V, S)).astype(np.float32).astype(np.float64)
    b = beliefs(rng, B, S)
    eng = Engine(S, A, O, 1, rs, rto, er, dtype='f32', mode='dense')
    try:
        return digest(eng.backup_full(alpha, b, 0.9))
    finally:
        eng.close()


KINDS = {'r1': case_r1, 'rn': case_rn, 'short': case_short, 'child': case_child, 'dense': case_dense}


def run_case(name):
    kind, shape, settings = CASES[name]
    out = KINDS[kind](shape, **settings)
    out['blocks'] = 256                                     # persistent blocks of the recording device (see above)
    return out


@pytest.mark.parametrize('name', list(CASES))
def test_score_slabs_equal_the_recorded_bits(name):
    with open(GOLDEN_FILE) as f:
        want = json.load(f)[name]
    assert run_case(name) == want
