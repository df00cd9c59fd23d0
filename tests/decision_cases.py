"""Input families and host references of tests/test_decision_paths.py (shared with its child process,
tests/decision_paths_child.py).  Test infrastructure: plain NumPy, no engine calls but ``Problem.engine``.

Family E  exact arithmetic: rto in {0.25, 0.75}, gamma = 0.5, beliefs in multiples of 1/64, small-integer ER and alpha
          rows (one dyadic step on one state of one row).  Every fp64 sum is exact in any order, so the reference is
          exact, ties are ties, and alpha' rows can be compared byte for byte.
Family N  the inexact near-ties of test_gpu_parity.py::test_adversarial_near_ties, rounded to fp32 for fp32 engines and
          left in fp64 (gaps 1e-7 .. 1e-11) for fp64 engines; reference in np.longdouble.
Both come with planted action structure (``actions=``): action 2 a copy of action 0, or a copy but for a tiny change of
its rewards.
"""
import functools
import hashlib

import numpy as np

from test_score_window import U24, f32r, ref_magnitude, ref_scores, sparse_rto, successors

E_GAMMA = 0.5
N_GAMMA = 0.9375                                             # exact in fp32
E_S, E_V, E_B = 310, 700, 40                                # S no multiple of 32; three 256-column chunks of V
E_KS = (2, 3, 8, 9, 32, 33, 300)
E_VARIANTS = ('copies', 'l1_gap', 'window_gap')             # (i), (ii), (iii)


class Problem:
    """One backup's inputs as the engine holds them, and its reference (computed once, on first use)."""

    def __init__(self, rs, rto, er, alpha, b, gamma, exact, **extra):
        self.rs, self.rto, self.er, self.alpha, self.b, self.gamma, self.exact = rs, rto, er, alpha, b, gamma, exact
        self.S, self.A, self.O, self.R = rto.shape
        self.V, self.B = alpha.shape[0], b.shape[0]
        self.__dict__.update(extra)

    def engine(self, dtype, mode='sparse'):
        from pomdp_pbvi_exploration_amd.engine import Engine
        return Engine(self.S, self.A, self.O, self.R, self.rs, self.rto, self.er, dtype=dtype, mode=mode)

    def with_alpha(self, alpha):
        return Problem(self.rs, self.rto, self.er, alpha, self.b, self.gamma, self.exact)

    @functools.cached_property
    def ref(self):
        return ref_backup(self.alpha, self.b, self.rs, self.rto, self.er, self.gamma,
                          np.float64 if self.exact else np.longdouble)

    @functools.cached_property
    def mag(self):
        return ref_magnitude(self.alpha, self.b, self.rs, self.rto, self.gamma)


def ref_rows(alpha, rs, rto, er, gamma, act, best):
    """alpha'[b, s] = ER[s, a*] + sum_o gamma sum_r rto[s, a*, o, r] alpha[v*[b, a*, o], rs[s, a*, r]] in float64, the
    observations added in order (k_assemble's association)."""
    B = len(act)
    S, A, O, R = rto.shape
    out = np.empty((B, S))
    for i in range(B):
        a = int(act[i])
        total = np.zeros(S)
        for o in range(O):
            g = np.zeros(S)
            for r in range(R):
                g = g + rto[:, a, o, r] * alpha[int(best[i, a, o]), rs[:, a, r]]
            total = gamma * g if o == 0 else total + gamma * g
        out[i] = er[:, a] + total
    return out


def ref_backup(alpha, b, rs, rto, er, gamma, dtype=np.longdouble):
    """The whole decision in ``dtype``: scores [B, G, V], v* = first maximum per (b, a, o), action values
    b . ER[:, a] + sum_o max_v score (reward first, then the observations in order), a* = first maximum; rows in float64."""
    S, A, O, R = rto.shape
    B = b.shape[0]
    sc = ref_scores(alpha, b, rs, rto, gamma, dtype)
    best = np.argmax(sc, axis=2).reshape(B, A, O)
    top = sc.max(axis=2).reshape(B, A, O)
    val = np.einsum('bs,sa->ba', b.astype(dtype), er.astype(dtype))
    for o in range(O):
        val = val + top[:, :, o]
    act = np.argmax(val, axis=1)
    return {'scores': sc, 'best': best, 'values': val, 'actions': act,
            'rows': ref_rows(alpha, rs, rto, er, gamma, act, best)}


def digest(best, actions, rows):
    """sha256 over (indices, actions, row bytes) of a result in caller order."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(best, dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(actions, dtype=np.int64).tobytes())
    h.update(np.ascontiguousarray(rows).tobytes())
    return h.hexdigest()


# --------------------------------------------------------------------------- #
# Family E
# --------------------------------------------------------------------------- #
def planted_positions(k, late=False):
    """k indices of the copies of the top row in [1, E_V): never 0, always 255 | 256 (the first chunk boundary of
    k_refine's candidate scan); from k = 3 on the last column, from k = 8 on also 254, 257, 511 | 512 and column 3.
    Per 256-column chunk: k = 9 -> 3 / 3 / 3 (no chunk above the deferral threshold of 8), k = 32 -> 12 / 10 / 10,
    k = 33 -> 12 / 10 / 11, k = 300 -> 100 / 100 / 100.  late: k = 33 as 3 / 19 / 11 -- the first chunk stays in the
    entry's own block, the rest is deferred, and the two results are merged."""
    fixed = {2: [255, 256], 3: [255, 256, 699], 8: [3, 254, 255, 256, 257, 511, 512, 699]}
    if k in fixed:
        return fixed[k]
    pos = set(fixed[8]) | {600}                              # 3 / 3 / 3
    per = {9: (3, 3, 3), 32: (12, 10, 10), 33: (3, 19, 11) if late else (12, 10, 11), 300: (100, 100, 100)}[k]
    lo = (1, 256, 512)
    hi = (256, 512, E_V)
    for c in range(3):
        step = max(1, (hi[c] - lo[c]) // (per[c] + 1))
        v = lo[c] + 7                                        # 64-column wave boundaries of the scan fall in between
        while sum(lo[c] <= p < hi[c] for p in pos) < per[c]:
            if v not in pos and v < hi[c]:
                pos.add(v)
            v += step
            if v >= hi[c]:
                v = lo[c] + 1 + (v % 5)
    out = sorted(pos)
    assert len(out) == k and [sum(lo[c] <= p < hi[c] for p in out) for c in range(3)] == list(per)
    return out


def chunk_counts(pos):
    return [sum(256 * c <= p < 256 * (c + 1) for p in pos) for c in range((E_V + 255) // 256)]


@functools.lru_cache(maxsize=None)
def e_model(R, regular, actions=None):
    """Model of family E: A = 2 (3 with planted actions), O = 2.  State T = 200 is where variants (ii) and (iii) raise one
    alpha row; its only predecessor is P0 = T - 1, through successor slot 0 of every action, with rto[P0, :, :, 0] = 0.25
    (irregular: successors that hit T are moved to T + 1; regular: shifts, slot 0 by +1, the others away from the
    beliefs' support around T)."""
    rng = np.random.default_rng(900 + 10 * R + int(regular))
    S, A, O, T = E_S, 2, 2, 200
    if regular:
        off = np.array([[1, 7, -6], [1, -9, 12]])[:, :R]
        rs = ((np.arange(S)[:, None, None] + off[None]) % S).astype(np.int64)
    else:
        rs = rng.integers(0, S, size=(S, A, R)).astype(np.int64)
        rs[rs == T] = T + 1
        rs[T - 1, :, 0] = T
    rto = np.where(rng.random((S, A, 1, R)) < 0.5, 0.25, 0.75) * np.ones((1, 1, O, 1))
    rto[:, :, 1, :] = 1.0 - rto[:, :, 0, :]
    rto[T - 1, :, :, 0] = 0.25
    er = rng.integers(-4, 5, size=(S, A)).astype(np.float64)
    if actions is not None:                                  # action 2: a copy of action 0; the pair boosted on some states
        boost = np.zeros(S)
        boost[rng.choice(S, size=S // 3, replace=False)] = 6.0
        er[:, 0] += boost
        rs = np.concatenate([rs, rs[:, :1]], axis=1)
        rto = np.concatenate([rto, rto[:, :1]], axis=1)
        er = np.concatenate([er, er[:, :1]], axis=1)
        if actions == 'raised':                              # ... but for one dyadic step on one state's reward
            er[E_ER_STATE, 2] += 2.0 ** -20
    return rs, rto, er, T


E_ER_STATE = 77


@functools.lru_cache(maxsize=None)
def e_beliefs(R, regular, actions=None):
    """B = 40 beliefs of 64 atoms of 1/64.  Even rows ("touching") hold 2/64 on P0 = T - 1 and nothing on any other
    predecessor of T; odd rows hold nothing on any predecessor.  Rows 1, 5, 9, ... hold 1/64 on T itself (for the
    value maxima, which score b . alpha).  With planted actions every third row holds weight on E_ER_STATE."""
    rs, rto, er, T = e_model(R, regular, actions)
    rng = np.random.default_rng(31 + R)
    S = E_S
    pred = np.unique(np.nonzero((rs == T).any(axis=(1, 2)))[0])
    free = np.setdiff1d(np.arange(S), np.concatenate([pred, [T, E_ER_STATE]]))
    b = np.zeros((E_B, S))
    for i in range(E_B):
        n = 64
        if i % 2 == 0:
            b[i, T - 1] += 2.0 / 64.0
            n -= 2
        if i % 4 == 1:
            b[i, T] += 1.0 / 64.0
            n -= 1
        if actions is not None and i % 3 == 0:
            b[i, E_ER_STATE] += 4.0 / 64.0
            n -= 4
        np.add.at(b[i], rng.choice(free, size=n), 1.0 / 64.0)
    assert np.all(b.sum(axis=1) == 1.0) and np.all(b[1::2][:, pred] == 0) and np.all(b[0::2][:, np.setdiff1d(pred, [T - 1])] == 0)
    return b


def e_alpha(R, regular, positions, step, actions=None):
    """V = 700 rows: the top row (integers in [-8, 8]) at `positions`, the LAST of them raised by `step` on state T
    (step = 0: a plain copy); every other row is the top row minus 2 or 3 minus 0 / 1 / 2 per state (distinct rows)."""
    T = e_model(R, regular, actions)[3]
    rng = np.random.default_rng(5 + R)
    top = rng.integers(-8, 9, size=E_S).astype(np.float64)
    alpha = top[None, :] - rng.integers(2, 4, size=(E_V, 1)) - rng.integers(0, 3, size=(E_V, E_S))
    alpha[positions] = top
    alpha[positions[-1], T] += step
    return alpha


def e_gain_units(R, regular, positions, step, actions=None):
    """[B][G]: (score of the raised row - score of a plain copy) / (2^-24 magnitude), exact."""
    rs, rto, er, T = e_model(R, regular, actions)
    b = e_beliefs(R, regular, actions)
    alpha = e_alpha(R, regular, positions, step, actions)
    sc = ref_scores(alpha[[positions[0], positions[-1]]], b, rs, rto, E_GAMMA)
    return (sc[:, :, 1] - sc[:, :, 0]) / (U24 * ref_magnitude(alpha, b, rs, rto, E_GAMMA))


def e_step(R, regular, variant, positions, actions=None):
    """The dyadic step of a variant.  (ii): the largest power of two whose gain stays below HALF the level-1 screen's width
    2 (R + 4) 2^-24 mag for every entry; (iii): the smallest one whose gain exceeds TWICE that width for every touching
    entry -- so the screen separates the raised row whatever its own rounding does -- and it must stay below twice the
    narrowest score window, 8 2^-24 (sqrt(32) + 1) mag."""
    if variant == 'copies':
        return 0.0
    unit = e_gain_units(R, regular, positions, 1.0, actions)             # gain per unit step (mag barely moves with the step)
    live = unit > 0
    l1 = 2.0 * (R + 4)
    if variant == 'l1_gap':
        e = np.floor(np.log2(0.5 * l1 / unit[live].max()))
    else:
        e = np.ceil(np.log2(2.0 * l1 / unit[live].min()))
    assert -19 <= e <= -8, e                                 # |integer| <= 8 plus the step: 4 + 19 bits, an fp32 number
    return float(2.0 ** e)


@functools.lru_cache(maxsize=None)
def e_problem(R, regular, k, variant, late=False, actions=None):
    pos = planted_positions(k, late)
    rs, rto, er, T = e_model(R, regular, actions)
    step = e_step(R, regular, variant, pos, actions)
    alpha = e_alpha(R, regular, pos, step, actions)
    return Problem(rs, rto, er, alpha, e_beliefs(R, regular, actions), E_GAMMA, True, positions=pos, step=step, k=k,
                   variant=variant, T=T)


def e_plain_alpha(R, regular, actions=None):
    """An alpha set of family E without any tie: one top row at index 5."""
    return e_alpha(R, regular, [5], 0.0, actions)


# --------------------------------------------------------------------------- #
# Family N
# --------------------------------------------------------------------------- #
N_S, N_B = 1000, 70
# model variant (test_score_window.VARIANTS): successors per (s, a), consecutive successors, alpha rows
N_VARIANTS = {'proj': (2, False, 96), 'fused1': (1, True, 300), 'fused3': (3, True, 96)}


@functools.lru_cache(maxsize=None)
def n_problem(variant, f32, actions=None, eps=0.0, seed=42, A=3, O=2, S=N_S, V=None, B=N_B, plain=False):
    """test_adversarial_near_ties' construction: alpha rows base (1 + 10^-(5 + v mod 5) noise) (fp64 engines: 10^-(7 + v mod 5),
    operands not fp32-representable), alpha[7] = alpha[3], sparse beliefs.  actions = 'copy': A is tiled cyclically from a
    3-action base whose action 2 is a copy of action 0, the pair boosted; 'eps': ER[:, 2] = ER[:, 0] (1 + eps noise).
    plain: alpha rows 20 % apart instead -- hardly an entry is a near-tie, so the action stage meets scores that still carry
    their window."""
    R, regular, V0 = N_VARIANTS[variant]
    V = V or V0
    rng = np.random.default_rng(seed)
    A0 = 3 if actions else A
    rs = successors(rng, S, A0, R, regular)
    rto = sparse_rto(rng, S, A0, O, R)
    er = rng.normal(size=(S, A0))
    if not f32:
        rto = rto * (1.0 + 1e-9 * rng.standard_normal(rto.shape))       # not fp32-representable
    if actions:
        er[:, 0] += 0.5 * (rng.random(S) < 0.3)
        rs[:, 2], rto[:, 2], er[:, 2] = rs[:, 0], rto[:, 0], er[:, 0]
        if actions == 'eps':
            er[:, 2] = er[:, 0] * (1.0 + eps * rng.standard_normal(S))
        cyc = np.arange(A) % 3
        rs, rto, er = rs[:, cyc], rto[:, cyc], er[:, cyc]
    base = rng.random(S) * 10.0 + 1.0
    alpha = np.empty((V, S))
    for v in range(V):
        alpha[v] = base * (1.0 + (0.2 if plain else 10.0 ** -((5 if f32 else 7) + v % 5)) * rng.standard_normal(S))
    if V > 7:
        alpha[7] = alpha[3]
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.05)
    b[:, 0] += 1e-3
    b = b / b.sum(axis=1, keepdims=True)
    if f32:
        rto, er, alpha, b = f32r(rto), f32r(er), f32r(alpha), f32r(b)
    return Problem(np.ascontiguousarray(rs), np.ascontiguousarray(rto), np.ascontiguousarray(er), alpha, b, N_GAMMA, False)


def undecidable(p):
    """Entries whose longdouble top-2 gap is non-zero and below 64 S R 2^-53 of the magnitude."""
    sc = p.ref['scores']
    top2 = np.sort(sc, axis=2)[:, :, -2:]
    gap = (top2[:, :, 1] - top2[:, :, 0]).astype(np.float64)
    return (gap != 0) & (gap < 64.0 * p.S * p.R * 2.0 ** -53 * p.mag), gap
