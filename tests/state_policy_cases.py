"""Shared inputs and plain-Python statements of the state policies (``test_state_policy``, ``test_state_policy_device``):
belief rows that exercise the chunk edges, the seam between two chunk groups and the MLS lane stride, per-state action tables, a
model that is sparse at any S, and the definition of include/pbvi_hip.h written as
loops, one add at a time -- what ``pomdp.state_policy_numpy`` and ``pbvi_state_policy`` are compared with bit for bit."""
import numpy as np

CHUNK = 256
SIZES = [2, 11, 255, 256, 257, 513, 600]
UNIFORMS = [0.0, 0.5, float(np.nextafter(0.5, 0.0)), 1.0 - 2.0 ** -53, 1.0]
ACTION_COUNTS = [1, 4, 9, 17]
# The voting and Thompson walks of k_state_policy take the chunks in groups of 128 (one per thread of the row's block); the
# definition knows no groups, so the statements below are an independent reference for everything that depends on the group.
GROUP = 128 * CHUNK
SEAM_SIZES = (32767, 32768, 32769, 33000, 65537)    # 128 chunks, the last ragged | one full group | two groups, the second one
                                                    # state | the 75 x 440 olfactory grid: a ragged chunk in group 1 | three groups
MLS_WRAP_SIZES = (1023, 1024, 1025, 1281)           # an fp32 engine's MLS lanes (256, 4 states a load) wrap above 1024 states
SEAM_UNIFORMS = (0.0, 0.25, float(np.nextafter(0.25, 0.0)), 0.5, float(np.nextafter(0.5, 0.0)), 0.75, 1.0 - 2.0 ** -53, 1.0)


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


def seam_marks(S):
    """The states of the exact boundary row: the first and the last state of the last chunk of group 0, the first state of
    group 1 and the last state (``S > GROUP``); else the first and last state of the last two chunks.  Needs ``S > CHUNK``."""
    if S > GROUP:
        return [GROUP - CHUNK, GROUP - 1, GROUP, S - 1]
    last = (S - 1) // CHUNK * CHUNK
    return [last - CHUNK, last - 1, last, S - 1]


def seam_tie_states(S):
    """``(lower, upper)``: the states of the vote-tie row.  The first four lie in group 0 only (two chunks, two states each),
    the last one in group >= 1 only (``S > GROUP``; else: in the chunk before the last, and in the last)."""
    edge = GROUP if S > GROUP else (S - 1) // CHUNK * CHUNK
    return [edge - 2 * CHUNK + 7, edge - CHUNK - 1, edge - CHUNK, edge - 1], [edge]


def seam_rows(S, seed=0):
    """``{name: [S] row}``, fp64 rows whose values are fp32 numbers, around the seam between two chunk groups:
        dense         random mass everywhere: 128 or more chunk partials behind every vote and every Thompson prefix
        behind, front (``S > GROUP``) all mass in ``[GROUP, S)`` / in ``[0, GROUP)``
        boundary      0.25 on each of ``seam_marks(S)`` (coinciding states add up): every partial sum is exact, so u = 0.25,
                      0.5, 0.75 put Thompson's target ON a cumulative sum and ``nextafter(u, 0)`` one ulp below it; the
                      equal maxima are MLS's tie across the seam
        one_hot_<s>   at the last state of group 0, the first of group 1 and the last state
        vote_tie      0.0625 on four states of group 0, 0.25 on one state of group 1 (``seam_tie_states``): under
                      ``seam_tie_table`` two actions get the same votes, one from either side of the seam"""
    rng = np.random.default_rng(4000 + S + seed)
    rows = {}
    b = rng.random(S)
    rows['dense'] = b / b.sum()
    if S > GROUP:
        b = np.zeros(S)
        b[GROUP:] = rng.random(S - GROUP) + 0.01
        rows['behind'] = b / b.sum()
        b = np.zeros(S)
        b[:GROUP] = rng.random(GROUP)
        rows['front'] = b / b.sum()
    b = np.zeros(S)
    np.add.at(b, seam_marks(S), 0.25)
    rows['boundary'] = b
    for s in sorted(set(seam_marks(S)[1:])):
        b = np.zeros(S)
        b[s] = 1.0
        rows[f'one_hot_{s}'] = b
    lower, upper = seam_tie_states(S)
    b = np.zeros(S)
    b[lower] = 0.0625
    b[upper] = 0.25
    rows['vote_tie'] = b
    return {name: r32(row) for name, row in rows.items()}


def seam_tie_table(S, A, seed=0):
    """``action_table`` with the lower states of ``seam_tie_states`` on action 1 and the upper one on action ``A - 1``: on
    the ``vote_tie`` row both get exactly 0.25, every other action +0.0, and action 1 must win.  ``A >= 3``."""
    sa = action_table(S, A, seed)
    lower, upper = seam_tie_states(S)
    sa[lower] = 1
    sa[upper] = A - 1
    return sa


def lane_tie_rows(S):
    """Rows whose equal maxima lie 512 and (``S > 1024``) 1024 states apart: the stride of one MLS lane on an fp64 / fp32
    engine, so that one lane compares the two: the lower state must win.  In the last row of either stride the later state
    holds more, and must win.  Needs ``S > 512``."""
    rows = []
    for d in (512, 1024):
        if S <= d:
            continue
        for lo in sorted({0, S - 1 - d}):
            b = np.zeros(S)
            b[[lo, lo + d]] = 0.5
            rows.append(b)
        b = np.zeros(S)
        b[0], b[d] = 0.25, 0.75
        rows.append(b)
    return np.array(rows)


def bare_model(S, A):
    """``(rs [S,A,1], rto [S,A,1,1])`` of a deterministic model with one observation: ``rs[s, a, 0] = (s + a + 1) % S``.  Nothing
    of it is dense in S x S, so it can be built at any S."""
    rs = ((np.arange(S, dtype=np.int64)[:, None] + np.arange(A, dtype=np.int64)[None, :] + 1) % S)[:, :, None]
    return rs, np.ones((S, A, 1, 1))


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
