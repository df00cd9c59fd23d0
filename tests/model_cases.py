"""Model builders and acceptance rules shared by the GPU test modules (no tests here).

``random_case`` is the random-model generator of ``test_random_models_against_the_oracle``; the hand-built structures
below are the smallest models in which an inverse transition list (``engine.hip::build_inverse_lists``) is very long,
empty, padded with probability-0 entries, or holds the same source state twice.
"""
import numpy as np

from oracle import pbvi_oracle as orc

N_RANDOM_CASES = 60


def random_case(seed):
    """A random model and shapes: successors random / grid-like / mixed, sparse RTO, localized or scattered belief supports,
    an alpha set with exact and near duplicates."""
    rng = np.random.default_rng(seed)
    S = int(rng.integers(33, 900)); A = int(rng.integers(1, 6)); O = int(rng.integers(1, 6)); R = int(rng.integers(1, 7))
    V = int(rng.integers(2, 400)); B = int(rng.integers(1, 400))
    if rng.random() < 0.3:
        B = int(rng.integers(257, 700))                         # more than one row block: the sorted path
    style = rng.integers(0, 3)
    if style == 0:
        rs = rng.integers(0, S, (S, A, R))
    else:
        off = rng.integers(-40, 41, (1, A, R)) if style == 1 else rng.integers(-5, 6, (1, A, R))
        rs = np.clip(np.arange(S)[:, None, None] + off, 0, S - 1)      # consecutive successors: the 16-byte gathers
        if style == 2:
            rs = np.where(rng.random((S, A, R)) < 0.1, rng.integers(0, S, (S, A, R)), rs)
    rto = rng.random((S, A, O, R)) * (rng.random((S, A, O, R)) < rng.uniform(0.2, 1.0))
    rto /= np.maximum(rto.sum(axis=(2, 3), keepdims=True), 1e-9)
    er = rng.normal(size=(S, A))
    b = rng.random((B, S)) * (rng.random((B, S)) < rng.uniform(0.02, 1.0))
    if rng.random() < 0.5:
        w = max(1, int(S * rng.uniform(0.05, 0.5)))
        for i in range(B):
            s0 = int(rng.integers(0, S - w + 1))
            b[i, :s0] = 0
            b[i, s0 + w:] = 0
    b[np.arange(B), rng.integers(0, S, B)] += 1e-3
    b /= b.sum(axis=1, keepdims=True)
    alpha = rng.normal(size=(V, S))
    if rng.random() < 0.4 and V > 4:
        k = int(rng.integers(1, max(2, V // 2)))
        src, dst = rng.integers(0, V, k), rng.integers(0, V, k)
        alpha[dst] = alpha[src]
        if rng.random() < 0.5:
            alpha[dst[: k // 2]] += rng.normal(size=(len(dst[: k // 2]), S)) * 1e-7
    return S, A, O, R, rs.astype(np.int64), rto, er, alpha, b, float(rng.uniform(0.5, 0.99))


def f32_round(*arrays):
    """The arrays as an f32 engine holds them, back in fp64 for the oracle."""
    out = tuple(np.asarray(a).astype(np.float32).astype(np.float64) for a in arrays)
    return out[0] if len(out) == 1 else out


def assert_backup_matches_oracle(res, alpha, want_rows, want_a, want_v, dtype, tag):
    """Acceptance rule of the random-model tests: indices, actions and rows against ``orc.backup_core``.  Between EXACT
    duplicates of an alpha row the engine returns the first (the tied scores are equal in exact arithmetic); NumPy's BLAS
    may round the later column's dot product one ulp higher and pick that one -- the reference never holds duplicates
    (``ValueFunction`` drops them), so such entries are compared by row content."""
    diff = np.argwhere(res.best_alpha_ind != want_v)
    for bi, a, o in diff:
        v1, v2 = res.best_alpha_ind[bi, a, o], want_v[bi, a, o]
        assert v1 < v2 and np.array_equal(alpha[v1], alpha[v2]), (tag, bi, a, o, v1, v2)
    assert np.array_equal(res.actions, want_a), tag
    tol = 1e-6 if dtype == 'f32' else 1e-12
    np.testing.assert_allclose(res.alpha, want_rows, rtol=tol, atol=tol * (np.abs(want_rows).max() + 1e-30), err_msg=str(tag))


# --------------------------------------------------------------------------- #
# Hand-built transition structures
# --------------------------------------------------------------------------- #
def _observation_table(rng, S, A, O):
    """O[s', a, o] > 0 everywhere: every observation is possible after every step."""
    t = rng.random((S, A, O)) + 0.05
    return t / t.sum(axis=2, keepdims=True)


def hub_model(S, A=2, O=2, seed=0):
    """Every (s, a, r=0) lands on state S-1; r=1 lands in the lower half.  The inverse list of the hub holds at least S
    entries, the lists of the lower half one or two, and the upper half (but the hub) has no predecessor at all."""
    rng = np.random.default_rng(7000 + seed + S)
    rs = np.empty((S, A, 2), dtype=np.int64)
    rs[:, :, 0] = S - 1
    rs[:, :, 1] = np.minimum((np.arange(S)[:, None] + np.arange(A)[None, :]) // 2, S - 1)
    rp = rng.uniform(0.2, 0.8, (S, A, 2))
    rp[:, :, 1] = 1.0 - rp[:, :, 0]
    return rs, orc.rto_table(rs, rp, _observation_table(rng, S, A, O))


def ragged_model(S, A=2, O=3, seed=0, max_succ=4):
    """Dense random T with one to ``max_succ`` successors per (s, a), through ``orc.reachable_from_dense``: short lists
    are padded with the lowest free state indices at probability 0, so the low states' inverse lists are long and
    mostly weightless."""
    rng = np.random.default_rng(8000 + seed + S)
    T = np.zeros((S, A, S))
    for s in range(S):
        for a in range(A):
            k = int(rng.integers(1, min(max_succ, S) + 1))
            to = rng.choice(S, size=k, replace=False)
            p = rng.random(k) + 0.1
            T[s, a, to] = p / p.sum()
    rs, rp = orc.reachable_from_dense(T)
    return rs, orc.rto_table(rs, rp, _observation_table(rng, S, A, O))


def duplicate_successor_model(S, A=2, O=2, seed=0):
    """rs[s,a,0] == rs[s,a,1] with both weights non-zero: one source state twice in the same inverse list."""
    rng = np.random.default_rng(9000 + seed + S)
    to = rng.integers(0, S, (S, A))
    rs = np.stack([to, to], axis=2).astype(np.int64)
    rp = rng.uniform(0.2, 0.8, (S, A, 2))
    rp[:, :, 1] = 1.0 - rp[:, :, 0]
    return rs, orc.rto_table(rs, rp, _observation_table(rng, S, A, O))


def identity_model(S, A=2, O=2, seed=0):
    """R = 1, every state stays where it is: every inverse list holds exactly its own state."""
    rng = np.random.default_rng(10000 + seed + S)
    rs = np.broadcast_to(np.arange(S, dtype=np.int64)[:, None, None], (S, A, 1)).copy()
    return rs, orc.rto_table(rs, np.ones((S, A, 1)), _observation_table(rng, S, A, O))


STRUCTURES = {'hub': hub_model, 'ragged': ragged_model, 'duplicate': duplicate_successor_model, 'identity': identity_model}


def sparse_beliefs(rng, B, S, density=0.3):
    """[B,S] normalised rows with exact zeros (at least one non-zero each)."""
    b = rng.random((B, S)) * (rng.random((B, S)) < density)
    b[np.arange(B), rng.integers(0, S, B)] += 0.25
    return b / b.sum(axis=1, keepdims=True)


def in_degrees(rs):
    """[A,S]: length of the inverse list of every (action, landing state)."""
    S, A, _ = rs.shape
    return np.stack([np.bincount(rs[:, a, :].ravel(), minlength=S) for a in range(A)])


def update_longdouble(belief, a, o, rs, rto):
    """``orc.belief_update`` restated in ``np.longdouble`` (sequential accumulation): the yardstick for how far the
    oracle's own fp64 sums are from the exact update."""
    S = belief.shape[0]
    w = (rto[:, a, o, :].astype(np.longdouble) * belief.astype(np.longdouble)[:, None]).ravel()
    nb = np.zeros(S, dtype=np.longdouble)
    np.add.at(nb, rs[:, a, :].ravel(), w)
    return nb / nb.sum()


def first_possible_observation(belief, a, rs, rto):
    """``(o, b')`` for the lowest observation whose ``orc.belief_update`` is finite, or ``(-1, None)``."""
    with np.errstate(invalid='ignore', divide='ignore'):
        for o in range(rto.shape[2]):
            nb = orc.belief_update(belief, int(a), o, rs, rto)
            if np.isfinite(nb).all():
                return o, nb
    return -1, None
