"""Shared inputs and plain-Python statements of the state policies (``test_state_policy``, ``test_state_policy_device``):
belief rows that exercise the chunk edges, per-state action tables, and the definition of include/pbvi_hip.h written as
loops, one add at a time -- what ``pomdp.state_policy_numpy`` and ``pbvi_state_policy`` are compared with bit for bit."""
import numpy as np

CHUNK = 256
SIZES = [2, 11, 255, 256, 257, 513, 600]
UNIFORMS = [0.0, 0.5, float(np.nextafter(0.5, 0.0)), 1.0 - 2.0 ** -53, 1.0]
ACTION_COUNTS = [1, 4, 9, 17]


def r32(a):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64)


def belief_rows(S, seed=0):
    """``[n, S]`` fp64 rows whose values are fp32 numbers (so that engines of both formats hold them exactly): dense random,
    sparse (about 2 % non-zero, at least one), one-hot at the first / a middle / the last state, all mass in the last
    (ragged) chunk, exact ties between states, and a leading run of zeros."""
    rng = np.random.default_rng(1000 + S + seed)
    rows = []
    for _ in range(3):
        b = rng.random(S)
        rows.append(b / b.sum())
    for _ in range(3):
        b = rng.random(S) * (rng.random(S) < 0.02)
        b[rng.integers(S)] += rng.random() + 0.1
        rows.append(b / b.sum())
    for s in sorted({0, S // 2, S - 1}):
        b = np.zeros(S)
        b[s] = 1.0
        rows.append(b)
    last = (S - 1) // CHUNK * CHUNK                              # first state of the last chunk
    b = np.zeros(S)
    b[last:] = rng.random(S - last) + 0.01
    rows.append(b / b.sum())
    b = np.zeros(S)                                              # exact ties: equal masses, the first must win
    b[rng.choice(S, size=min(S, 4), replace=False)] = 0.25
    rows.append(b)
    b = rng.random(S)
    b[:S // 2] = 0.0
    rows.append(b / b.sum())
    return r32(np.array(rows))


def action_table(S, A, seed=0):
    """``[S]`` int64 in ``[0, A)``; every action below ``min(A, S)`` occurs."""
    rng = np.random.default_rng(77 + 13 * S + A + seed)
    sa = rng.integers(0, A, S)
    k = min(A, S)
    sa[rng.choice(S, size=k, replace=False)] = np.arange(k)
    return sa.astype(np.int64)


def thompson_loop(b, u):
    """The definition of rule 2 for one row, as a loop: ``(state, took the chunk fallback, took the state fallback)``."""
    b = [float(x) for x in b]
    S = len(b)
    C = -(-S // CHUNK)
    q, m, P = [], [], []
    run = 0.0
    for c in range(C):
        acc, qc = 0.0, []
        for s in range(CHUNK * c, min(CHUNK * c + CHUNK, S)):
            acc = acc + b[s]
            qc.append(acc)
        q.append(qc)
        m.append(acc)
        run = run + acc
        P.append(run)
    target = float(u) * P[-1]
    cs = next((c for c in range(C) if target < P[c]), None)
    chunk_fallback = cs is None
    if chunk_fallback:
        cs = max([c for c in range(C) if m[c] > 0], default=0)
    r = target - (P[cs - 1] if cs > 0 else 0.0)
    j = next((j for j in range(len(q[cs])) if r < q[cs][j]), None)
    state_fallback = j is None
    if state_fallback:
        j = max([j for j in range(len(q[cs])) if b[CHUNK * cs + j] > 0], default=0)
    return CHUNK * cs + j, chunk_fallback, state_fallback


def votes_loop(b, sa, A):
    """The definition of rule 1's ``W [A]`` for one row, as a loop."""
    S = len(b)
    W = [0.0] * A
    for c in range(-(-S // CHUNK)):
        Wc = [0.0] * A
        for s in range(CHUNK * c, min(CHUNK * c + CHUNK, S)):
            Wc[int(sa[s])] = Wc[int(sa[s])] + float(b[s])
        for a in range(A):
            W[a] = W[a] + Wc[a]
    return np.array(W)


def first_greater_loop(x):
    """The first index whose entry is strictly greater than every earlier one; a NaN counts as -inf, so it never wins
    against a number and a row of NaNs gives 0."""
    best, at = None, 0
    for i, v in enumerate(x):
        v = float(v)
        if v != v:
            v = -np.inf
        if best is None or v > best:
            best, at = v, i
    return at
