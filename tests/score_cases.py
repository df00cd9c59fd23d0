"""Seeded random models and belief sets shared by the score-GEMM tests (test_split_schedule.py, test_score_split.py,
test_score_slabs_golden.py, test_gpu_parity.py).  Every value is fp32-representable, so an fp32 engine holds them exactly."""
import numpy as np


def random_model(rng, S, A, O, regular):
    """One successor per (s, a): a shift per action (``regular``: 16-byte alpha loads) or random (gathers)."""
    if regular:
        rs = ((np.arange(S)[:, None] + rng.integers(-5, 6, size=A)[None, :]) % S)[:, :, None].astype(np.int64)
    else:
        rs = rng.integers(0, S, size=(S, A, 1))
    p = rng.random((S, A, O))
    p[rng.random((S, A, O)) < 0.3] = 0.0
    p[:, :, 0] += 1e-3
    rto = (p / p.sum(axis=2, keepdims=True))[:, :, :, None].astype(np.float32).astype(np.float64)
    er = rng.normal(size=(S, A)).astype(np.float32).astype(np.float64)
    return rs, rto, er


def shifted_model(rng, S, A, O, R):
    """R successors per (s, a): shifts per (action, slot) with a sprinkle of random successors -- K tiles with such a chunk
    are projected and read, so generated and read K steps alternate inside one tile list -- and zero-probability pad slots
    as the reference's Model pads them (src/mdp.py:308-335)."""
    shifts = rng.integers(-40, 41, size=(A, R))
    rs = (np.arange(S)[:, None, None] + shifts[None]) % S
    odd = rng.random((S // 4 + 1, A, R)) < 0.003                      # some 4-state chunks lose their regularity
    odd = np.repeat(odd, 4, axis=0)[:S]
    rs = np.where(odd, rng.integers(0, S, size=(S, A, R)), rs).astype(np.int64)
    p = rng.random((S, A, O, R))
    p[rng.random((S, A, O, R)) < 0.3] = 0.0
    p[:, :, 0, 0] += 1e-3
    pad = rng.random((S, A)) < 0.1                                      # (s, a) with fewer than R successors
    p[pad, :, R - 1] = 0.0
    rs[pad, R - 1] = 0
    rto = (p / p.sum(axis=(2, 3), keepdims=True)).astype(np.float32).astype(np.float64)
    er = rng.normal(size=(S, A)).astype(np.float32).astype(np.float64)
    return rs, rto, er


def beliefs(rng, B, S, density=0.2, support=None):
    """Random sparse beliefs; support: only the first `support` states may be non-zero."""
    n = S if support is None else support
    b = np.zeros((B, S))
    b[:, :n] = rng.random((B, n)) * (rng.random((B, n)) < density)
    b[np.arange(B), rng.integers(0, n, size=B)] += 1e-3
    return (b / b.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float64)
