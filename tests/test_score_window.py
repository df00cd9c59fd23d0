"""The scores and tie windows behind every argmax, against a high-precision reference.

Every decision of a backup rests on one claim: a score read from the GEMM slabs lies within the window E of the true
score, so a (belief, group) whose runner-up is closer than 2E is queued for exact refinement and every other one is
already right.  The score probe (``Engine.debug_score_probe``) captures, at the end of the scoring stage and before any
refinement, what ``k_argmax`` read (scores, magnitudes, through its own slab view) and wrote (windows, first maxima,
queue).  For every pipeline and input family below:

0. dead map   the probe's dead triples are supp(b) n supp(RTO[:, a, o, :]) = {} on the inputs as the engine holds them
              (``mask_cases.dead_ref``), before anything below is restricted to the live ones;
1. values     |score_dev - score_ref| <= E_dev  (pure fp64: <= (n + 2) 2^-53 mag_ref, n = non-zero products of the dot);
2. window     E_dev is the documented formula applied to the reference's magnitude, within its own relative width;
3. argmax     from score_dev and E_dev alone, ``ref_argmax`` reproduces best_v and best_score bit for bit and the set of
              queued entries exactly; dead rows are (0, 0.0, 0.0) and not queued;
4. safety     every row that is neither queued nor dead already holds the first argmax of score_ref;
5. headroom   the largest |err| / E is printed (``pytest -s``); DESIGN.md section 5e keeps the measured table.

References are plain NumPy on the same rounded inputs the engine gets: float64 accumulation for fp32 scoring (its own
error, ~S 2^-53 of the magnitude, is 2^-29 of the narrowest window 8 2^-24), ``np.longdouble`` for pure fp64 scoring.
"""
import functools

import numpy as np
import pytest

from mask_cases import dead_ref
from oracle import pbvi_oracle as orc

U24 = 2.0 ** -24
GAMMA = 0.9375                      # exact in fp32: the engine's (float) gamma is the reference's


# --------------------------------------------------------------------------- #
# Host references
# --------------------------------------------------------------------------- #
def ref_scores(alpha, b, rs, rto, gamma, dtype=np.float64):
    """[B][G][V], g = a * O + o:  b . Gamma[a,o,v,:],  Gamma[a,o,v,s] = gamma sum_r rto[s,a,o,r] alpha[v, rs[s,a,r]],
    accumulated in ``dtype``."""
    S, A, O, R = rto.shape
    al, bb, rt = alpha.astype(dtype), b.astype(dtype), rto.astype(dtype)
    out = np.zeros((b.shape[0], A * O, alpha.shape[0]), dtype=dtype)
    for a in range(A):
        alpha_r = al[:, rs[:, a, :]]                                     # V,S,R
        for o in range(O):
            gam = dtype(gamma) * (rt[None, :, a, o, :] * alpha_r).sum(axis=2)      # V,S
            # (c_einsum, not BLAS: one summation order for every column, so equal alpha rows get equal scores)
            out[:, a * O + o, :] = np.einsum('bs,vs->bv', bb, gam)
    return out


def ref_magnitude(alpha, b, rs, rto, gamma):
    """[B][G]: the magnitude column as the code defines it -- the row max_v |alpha_v| (k_col_absmax: column-wise, over
    the alpha rows) carried through the same projection and dot as an alpha row (k_project's row V; the belief side's
    aux_mag is the same sum re-associated: sum_s' |bp[g,b,s']| amax[s'])."""
    amax = np.abs(alpha).max(axis=0)
    return ref_scores(amax[None, :], np.abs(b), rs, np.abs(rto), abs(gamma))[:, :, 0]


def ref_products(alpha, b, rs, rto):
    """[B][G][V]: number of non-zero products b[s] rto[s,a,o,r] alpha[v, rs[s,a,r]] in each score's dot."""
    S, A, O, R = rto.shape
    nzb = (b != 0).astype(np.float64)
    out = np.zeros((b.shape[0], A * O, alpha.shape[0]))
    for a in range(A):
        nza = alpha[:, rs[:, a, :]] != 0                                 # V,S,R
        for o in range(O):
            cnt = (nza & (rto[None, :, a, o, :] != 0)).sum(axis=2).astype(np.float64)
            out[:, a * O + o, :] = np.einsum('bs,vs->bv', nzb, cnt)
    return out


def ref_argmax(scores, E):
    """One pass per (b, g) over scores [..., V] with windows E [...]: the first maximum m and its index, m2 = the
    largest of the OTHER entries (a later entry equal to m counts; -inf when V = 1) and flag = (m2 >= m - 2E) in
    float64, as k_argmax evaluates it."""
    scores = np.asarray(scores, dtype=np.float64)
    idx = np.argmax(scores, axis=-1)                                     # first maximum
    m = np.take_along_axis(scores, idx[..., None], axis=-1)[..., 0]
    rest = scores.copy()
    np.put_along_axis(rest, idx[..., None], -np.inf, axis=-1)
    m2 = rest.max(axis=-1)
    flag = m2 >= m - 2.0 * np.asarray(E, dtype=np.float64)
    return m, idx, m2, flag


def host_window(p):
    """The documented relative window (backup_kernels.hip: score_window, k_argmax; engine.hip: tie_window) from the
    probe's scalars.  fp32 GEMM: 8 2^-24 (sqrt(chain) + 1), chain = 32 chain_steps fma's (3x as many for the split);
    split: + 3.1 2^-16, the whole times 1 + 2^-11; belief side: + 2 2^-24.  tol_extra is added by the caller."""
    if p['tol_rel'] < 0.0:
        assert p['chain_steps'] >= 1, p['chain_steps']
        tr = 8.0 * U24 * (np.sqrt(p['chain_steps'] * 32.0 * (3.0 if p['split'] else 1.0)) + 1.0)
    else:                                                                # a chunk length known on the host
        tr = p['tol_rel']
        k = (tr / (8.0 * U24) - 1.0) ** 2
        assert abs(k - round(k)) < 1e-6 and round(k) >= 1, (tr, k)
    if p['split']:
        tr = (tr + 3.1 * 2.0 ** -16) * (1.0 + 2.0 ** -11)
    if p['push']:
        tr += 2.0 * U24
    return tr


# --------------------------------------------------------------------------- #
# Input families (all seeded)
# --------------------------------------------------------------------------- #
def f32r(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32).astype(np.float64)


def successors(rng, S, A, R, regular, step=1):
    if regular:                                              # consecutive successors (16-byte gathers, fused tiles)
        off = rng.integers(-5, 6, size=(1, A, R)) * step
        return ((np.arange(S)[:, None, None] + off) % S).astype(np.int64)
    return rng.integers(0, S, size=(S, A, R)).astype(np.int64)


def sparse_rto(rng, S, A, O, R, zero=0.3):
    p = rng.random((S, A, O, R)) * (rng.random((S, A, O, R)) >= zero)
    p[:, :, 0, 0] += 1e-3
    return p / p.sum(axis=(2, 3), keepdims=True)


def fam_mixed(rng, R, regular, V):
    """1. the baseline of the existing tests: mixed-sign alpha, sparse beliefs."""
    S, A, O, B = 1000, 2, 2, 70
    rs, rto = successors(rng, S, A, R, regular), sparse_rto(rng, S, A, O, R)
    alpha = rng.normal(scale=4.0, size=(V or 150, S))
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.2)
    b[np.arange(B), rng.integers(0, S, B)] += 1e-3
    return rs, rto, alpha, b / b.sum(axis=1, keepdims=True)


def fam_same_sign(rng, R, regular, V):
    """2. same-sign long chains: dense positive beliefs and RTO, alpha in [1, 2), S = 8193 -- every product has the same
    sign, the case a sqrt(chain) error model has least room for."""
    S, A, O, B = 8193, 1, 2, 40
    rs = successors(rng, S, A, R, regular)
    rto = rng.random((S, A, O, R)) + 0.1
    rto /= rto.sum(axis=(2, 3), keepdims=True)
    alpha = 1.0 + rng.random((V or 150, S))
    b = rng.random((B, S)) + 0.05
    return rs, rto, alpha, b / b.sum(axis=1, keepdims=True)


def fam_cancel(rng, R, regular, V):
    """3. cancellation: neighbouring states (2j, 2j + 1) carry +c and -c (1 + 1e-3 noise) under equal belief mass and equal
    RTO, and successors keep the pairing (even offsets), so |score| << magnitude.  The error is judged against the
    magnitude, as the window does."""
    S, A, O, B = 2000, 2, 2, 64
    V = V or 128
    rs = successors(rng, S, A, R, True, step=2)
    rto = np.repeat(sparse_rto(rng, S // 2, A, O, R), 2, axis=0)
    c = rng.uniform(0.5, 4.0, size=(V, S // 2)) * rng.choice([-1.0, 1.0], size=(V, S // 2))
    alpha = np.repeat(c, 2, axis=1) * np.tile([1.0, -1.0], S // 2)[None, :] * (1.0 + 1e-3 * rng.normal(size=(V, S)))
    h = rng.random((B, S // 2)) * (rng.random((B, S // 2)) < 0.3)
    h[np.arange(B), rng.integers(0, S // 2, B)] += 1e-2
    b = np.repeat(h, 2, axis=1)
    return rs, rto, alpha, b / b.sum(axis=1, keepdims=True)


def fam_range(rng, R, regular, V):
    """4. dynamic range: belief entries over 2^-40 .. 1 (not normalised), alpha over +-2^-30 .. 2^30; every score finite."""
    S, A, O, B = 600, 2, 3, 50
    V = V or 97
    rs, rto = successors(rng, S, A, R, regular), sparse_rto(rng, S, A, O, R)
    alpha = rng.choice([-1.0, 1.0], size=(V, S)) * 2.0 ** rng.uniform(-30, 30, size=(V, S))
    b = 2.0 ** -rng.uniform(0, 40, size=(B, S)) * (rng.random((B, S)) < 0.3)
    b[np.arange(B), rng.integers(0, S, B)] = 1.0
    return rs, rto, alpha, b


def fam_edges(S, B):
    def make(rng, R, regular, V):
        """5. tile edges: supports of 7 states that straddle a 32-column boundary (most K tiles skipped), every fifth
        belief with mass in the last -- partly filled -- K tile only, one all-zero Gamma group (a dead pair for every
        belief), B around the 256-row tile edge."""
        A, O = 2, 2
        rs, rto = successors(rng, S, A, R, regular), sparse_rto(rng, S, A, O, R, zero=0.1)
        rto[:, 1, 1, :] = 0.0                                # (a, o) = (1, 1) never happens: dead for every belief
        rto /= rto.sum(axis=(2, 3), keepdims=True)
        alpha = rng.normal(scale=2.0, size=(V or 130, S))
        b = np.zeros((B, S))
        last0 = 32 * ((S - 1) // 32)
        for i in range(B):
            if i % 5 == 4:
                b[i, last0:] = rng.random(S - last0) + 0.1
            else:
                edge = 32 * int(rng.integers(1, max(2, (S + 31) // 32)))
                lo, hi = max(0, min(edge, S) - 3), min(S, edge + 4)
                b[i, lo:hi] = rng.random(hi - lo) + 0.1
        return rs, rto, alpha, b / b.sum(axis=1, keepdims=True)
    return make


FAMILIES = {'mixed': fam_mixed, 'same_sign': fam_same_sign, 'cancel': fam_cancel, 'range': fam_range}
for _S in (31, 32, 33, 4097):                                # K tiles: one short, one full, one + 1 state, 128 + 1 state
    for _B in (1, 255, 256, 257):                            # row tiles: tiles_m 1 -> 2 between 256 and 257
        FAMILIES[f'edges_S{_S}_B{_B}'] = fam_edges(_S, _B)

# what a pipeline asks of the model: (successors per (s, a), consecutive successors, alpha rows or 0 = the family's)
VARIANTS = {'proj': (2, False, 0), 'fused1': (1, True, 300), 'fused3': (3, True, 0)}


class Case:
    """Inputs as the engine holds them (rounded to fp32 for fp32 engines), and their references in caller order."""

    def __init__(self, rs, rto, alpha, b, f32, longdouble=False):
        S, A, O, R = rto.shape
        if f32:
            rto, alpha, b = f32r(rto), f32r(alpha), f32r(b)
        self.S, self.A, self.O, self.R, self.V, self.B = S, A, O, R, alpha.shape[0], b.shape[0]
        self.rs, self.rto, self.alpha, self.b = rs, rto, alpha, b
        self.er = f32r(np.random.default_rng(S + A).normal(size=(S, A)))
        self.scores = ref_scores(alpha, b, rs, rto, GAMMA, np.longdouble if longdouble else np.float64)
        self.mag = ref_magnitude(alpha, b, rs, rto, GAMMA)
        self.dead = dead_ref(b, rto)                         # [B][G]: the dead-triple map from its definition
        assert np.isfinite(self.scores.astype(np.float64)).all()

    def engine(self, dtype, mode='sparse'):
        from pomdp_pbvi_exploration_amd.engine import Engine
        return Engine(self.S, self.A, self.O, self.R, self.rs, self.rto, self.er, dtype=dtype, mode=mode)


def seed_of(*key):
    return sum((i + 1) * ord(c) for i, c in enumerate('/'.join(str(k) for k in key)))


@functools.lru_cache(maxsize=None)
def family_case(family, variant, f32):
    """One reference per (family, variant, precision of the inputs), shared by the pipelines that use it."""
    R, regular, V = VARIANTS[variant]
    rng = np.random.default_rng(seed_of(family, variant))
    return Case(*FAMILIES[family](rng, R, regular, V), f32=f32)


def magnitude_is_valid(case):
    """ref_magnitude >= max_v |ref_scores| (up to the float64 rounding of the two sums: S 2^-52 relative)."""
    top = np.abs(case.scores.astype(np.float64)).max(axis=2)
    return bool(np.all(case.mag * (1.0 + case.S * 2.0 ** -52) >= top))


# --------------------------------------------------------------------------- #
# The planted ties of family 6
# --------------------------------------------------------------------------- #
ARGMAX_V = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1028, 1029)
PLANTS = ('same_lane_same_step', 'same_lane_next_step', 'other_lane', 'last_column', 'column_0')


def argmax_slot(v, vec4):
    """(lane, step) of column v in k_argmax.  vec4 reader (fp32 slabs, V % 4 == 0 or belief side): a lane takes 4
    consecutive columns, 256 columns per load group, four groups (1024 columns) per step.  Scalar reader: lane = v % 64,
    four columns 64 apart per step of 256."""
    return ((v % 256) // 4, v // 1024) if vec4 else (v % 64, v // 256)


def plant_position(V, p, plant, vec4):
    """Column of the duplicate of best column p, or None when V has no such column."""
    lane, step = argmax_slot(p, vec4)
    if plant == 'last_column':
        d = V - 1
    elif plant == 'column_0':
        d = 0
    else:
        want = {'same_lane_same_step': lambda l, s: l == lane and s == step,
                'same_lane_next_step': lambda l, s: l == lane and s == step + 1,
                'other_lane': lambda l, s: l != lane}[plant]
        d = next((v for v in range(V) if v != p and want(*argmax_slot(v, vec4))), None)
    return None if d is None or d == p else d


def planted_case(V, p, d, S=24):
    """A * O = 2, one K tile (S <= 32: equal rows give bit-equal scores whatever the schedule).  Row p is the constant 3,
    every other row lies in [-1, 1], so p wins every (belief, group); row d (if any) is an exact copy of it."""
    rng = np.random.default_rng(1000 * V + p)
    rs = np.arange(S, dtype=np.int64)[:, None, None].repeat(1, axis=1)
    rto = np.full((S, 1, 2, 1), 0.5)
    alpha = rng.uniform(-1.0, 1.0, size=(V, S))
    alpha[p] = 3.0
    if d is not None:
        alpha[d] = alpha[p]
    b = rng.random((6, S)) + 0.1
    return Case(rs, rto, alpha, b / b.sum(axis=1, keepdims=True), f32=True)


def gap_case(V, p, q, gap_out):
    """Row q = row p but for state 0, lower by 8 * gap_out (a power of two).  Belief 0 holds 1/4 of its mass there and
    belief 1 holds 1/8; gamma RTO = 1/2 (GAMMA is replaced by 1 in this case's runs), so the runner-up sits exactly
    gap_out below the winner for belief 0 and gap_out / 2 below it for belief 1.  Every value is a small multiple of a
    power of two: products and sums are exact in fp32."""
    S = 24
    rs = np.arange(S, dtype=np.int64)[:, None, None].repeat(1, axis=1)
    rto = np.full((S, 1, 2, 1), 0.5)
    alpha = np.zeros((V, S))
    alpha[:, 1] = -1.0
    alpha[p] = 3.0
    alpha[q] = 3.0
    alpha[q, 0] = 3.0 - 8.0 * gap_out
    b = np.zeros((2, S))
    b[0, :3] = (0.25, 0.5, 0.25)
    b[1, :3] = (0.125, 0.5, 0.375)
    return rs, rto, alpha, b


# --------------------------------------------------------------------------- #
# CPU-only tests of the references
# --------------------------------------------------------------------------- #
def test_ref_scores_reproduce_the_oracles_indices():
    rng = np.random.default_rng(5)
    S, A, O, R, V, B = 60, 3, 2, 2, 17, 9
    rs, rto = successors(rng, S, A, R, False), sparse_rto(rng, S, A, O, R)
    alpha, b = rng.normal(size=(V, S)), rng.random((B, S))
    b /= b.sum(axis=1, keepdims=True)
    er = rng.normal(size=(S, A))
    _, _, best = orc.backup_core(alpha, b, rs, rto, er, 0.9)
    sc = ref_scores(alpha, b, rs, rto, 0.9)
    assert np.array_equal(np.argmax(sc, axis=2).reshape(B, A, O), best)
    gam = orc.gamma_projection(alpha, rs, rto, 0.9)                     # A,O,V,S
    np.testing.assert_allclose(sc.reshape(B, A, O, V), np.einsum('bs,aovs->baov', b, gam), rtol=1e-12, atol=1e-13)
    ld = ref_scores(alpha, b, rs, rto, 0.9, np.longdouble)
    assert ld.dtype == np.longdouble
    np.testing.assert_allclose(ld.astype(np.float64), sc, rtol=1e-12, atol=1e-13)
    n = ref_products(alpha, b, rs, rto)
    assert n.max() <= S * R and n.min() >= 1


def test_ref_argmax_on_hand_written_rows():
    inf = np.inf
    rows = np.array([[1.0, 3.0, 2.0, 3.0],                   # a tie at a later index
                     [5.0, 5.0, 5.0, 5.0],                   # all entries equal
                     [0.0, 1.0, 2.0, 4.0],                   # the maximum in the last column
                     [4.0, 1.0, 3.0, -2.0]])
    m, idx, m2, flag = ref_argmax(rows, np.array([0.0, 0.0, 0.5, 0.5]))
    assert idx.tolist() == [1, 0, 3, 0] and m.tolist() == [3.0, 5.0, 4.0, 4.0]
    assert m2.tolist() == [3.0, 5.0, 2.0, 3.0]
    assert flag.tolist() == [True, True, False, True]        # 2 >= 4 - 1 is false; 3 >= 4 - 1 holds (the edge counts)
    m, idx, m2, flag = ref_argmax(np.array([[7.0]]), np.array([1e9]))   # V = 1: nothing to tie with
    assert (m[0], idx[0], m2[0], bool(flag[0])) == (7.0, 0, -inf, False)
    m, idx, m2, flag = ref_argmax(np.array([[-0.0, 0.0]]), np.array([0.0]))
    assert idx[0] == 0 and bool(flag[0])                     # -0.0 == 0.0: the first one stays


@pytest.mark.parametrize('family', ['mixed', 'cancel', 'range', 'edges_S33_B255'])
def test_ref_magnitude_bounds_every_score(family):
    case = family_case(family, 'proj', True)
    assert magnitude_is_valid(case)
    if family == 'cancel':                                   # the family does what it says: |score| << magnitude
        assert np.median(np.abs(case.scores).max(axis=2) / case.mag) < 0.02
    if family.startswith('edges'):                           # ... and so does this one: a dead group, last-tile beliefs
        assert np.all(case.scores[:, 3, :] == 0) and np.all(case.mag[:, 3] == 0)
        assert np.all(case.b[4, :32] == 0) and case.b[4, 32] > 0


@pytest.mark.parametrize('vec4', [False, True])
@pytest.mark.parametrize('V', ARGMAX_V)
def test_planted_ties_sit_where_they_say(V, vec4):
    for plant in PLANTS:
        for p in {0, V // 2, V - 1}:
            d = plant_position(V, p, plant, vec4)
            if d is None:
                continue
            assert 0 <= d < V and d != p
            (lp, sp), (ld, sd) = argmax_slot(p, vec4), argmax_slot(d, vec4)
            if plant == 'same_lane_same_step':
                assert (lp, sp) == (ld, sd)
            elif plant == 'same_lane_next_step':
                assert lp == ld and sd == sp + 1
            elif plant == 'other_lane':
                assert lp != ld
            case = planted_case(V, p, d)
            assert np.array_equal(case.alpha[p], case.alpha[d]) and np.all(case.alpha[p] == 3.0)
            others = np.delete(case.alpha, [p, d], axis=0)
            assert others.size == 0 or np.abs(others).max() <= 1.0
            m, idx, m2, flag = ref_argmax(case.scores, np.zeros((case.B, 2)))
            assert np.all(idx == min(p, d)) and np.all(m2 == m) and flag.all()
    # every plant exists somewhere in the set, in both readers
    for plant in PLANTS:
        assert any(plant_position(v, p, plant, vec4) is not None for v in ARGMAX_V for p in (0, v - 1)), plant


def test_gap_case_is_exact():
    rs, rto, alpha, b = gap_case(5, 3, 1, 2.0 ** -16)
    sc = ref_scores(alpha, b, rs, rto, 1.0)
    assert np.all(sc[:, :, 3] == 1.5)
    assert np.all(sc[0, :, 3] - sc[0, :, 1] == 2.0 ** -16) and np.all(sc[1, :, 3] - sc[1, :, 1] == 2.0 ** -17)
    assert np.array_equal(sc, f32r(sc))                      # representable in fp32: the device sums are these
    assert np.all(ref_magnitude(alpha, b, rs, rto, 1.0) == 1.5)


# --------------------------------------------------------------------------- #
# The checks of one captured stage
# --------------------------------------------------------------------------- #
def check_capture(p, case, tag, pure_f64=False, gamma=GAMMA):
    """Assertions 1-5 of the module docstring on one probe capture `p` (engine order) of `case` (caller order)."""
    B, G, V = case.B, case.A * case.O, case.V
    assert p['score'].shape == (B, G, V), tag
    perm = p['perm'].astype(np.int64)
    assert np.array_equal(np.sort(perm), np.arange(B)), tag
    ref = case.scores[perm] if gamma == GAMMA else ref_scores(case.alpha, case.b, case.rs, case.rto, gamma)[perm]
    mag_ref = case.mag[perm] if gamma == GAMMA else ref_magnitude(case.alpha, case.b, case.rs, case.rto, gamma)[perm]
    dev, E, dead = p['score'], p['E'], p['dead'].astype(bool)
    if not pure_f64:                                         # the map is checked, not trusted: everything below runs on `live`
        wrong = np.argwhere(dead != case.dead[perm])
        assert wrong.size == 0, (tag, 'dead map differs at (engine row, group)', wrong[:10].tolist())
    live = ~dead
    assert np.isfinite(dev).all() and np.isfinite(E).all(), tag
    err = np.abs((dev.astype(ref.dtype) - ref)).astype(np.float64)
    top = np.abs(ref.astype(np.float64)).max(axis=2)
    assert np.all(mag_ref * (1.0 + case.S * 2.0 ** -52) >= top), tag          # the restated magnitude is a magnitude

    # 1. values
    if pure_f64:
        assert np.all(E == 0.0) and p['qcount'] == 0 and not dead.any(), tag
        bound = (ref_products(case.alpha, case.b, case.rs, case.rto)[perm] + 2.0) * 2.0 ** -53 * mag_ref[:, :, None]
        ratio = np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)
        print(f'\n[score-window] {tag}: max |err| / ((n + 2) 2^-53 mag) = {ratio.max():.4f}')
        assert np.all(err <= bound), (tag, float(ratio.max()))
    else:
        Eb = np.broadcast_to(E[:, :, None], err.shape)
        ratio = np.divide(err, Eb, out=np.where(err > 0, np.inf, 0.0), where=Eb > 0)[live]
        rel = (err / np.maximum(mag_ref, 1e-300)[:, :, None])[live]
        print(f'\n[score-window] {tag}: max |err| / E = {ratio.max() if ratio.size else 0.0:.4f}   '
              f'(max |err| / mag = {rel.max() if rel.size else 0.0:.3e}, window {host_window(p) + p["tol_extra"]:.3e}, '
              f'chain_steps {p["chain_steps"]}, queued {p["qcount"]} of {int(live.sum())})')
        assert np.all(err[live] <= Eb[live]), (tag, float(ratio.max()))

    # 2. the window is the documented one
    if not pure_f64:
        w = host_window(p) + p['tol_extra']
        m_ref = ref.astype(np.float64).max(axis=2)
        E_host = w * np.maximum(np.abs(m_ref), mag_ref)
        assert np.all(E[live] >= E_host[live] * (1.0 - w)) and np.all(E[live] <= E_host[live] * (1.0 + w)), \
            (tag, float(np.min(E[live] / E_host[live])), float(np.max(E[live] / E_host[live])))

    # 3. the argmax kernel, from what it read alone
    m, idx, m2, flag = ref_argmax(dev, E)
    assert np.array_equal(p['best_v'][live], idx[live].astype(np.int32)), tag
    assert np.array_equal(p['best_score'][live].view(np.int64), m[live].view(np.int64)), tag
    assert np.all(p['best_v'][dead] == 0) and np.all(p['best_score'][dead] == 0.0) and np.all(E[dead] == 0.0), tag
    queue = np.sort(p['queue'].astype(np.int64))
    if not pure_f64:
        assert np.array_equal(queue, np.flatnonzero((flag & live).ravel())), tag
        assert p['qcount'] == int((flag & live).sum()), tag

    # 4. safety: what is not re-decided is already right
    settled = live if pure_f64 else live & ~flag
    first = np.argmax(ref.astype(np.float64), axis=2)
    if pure_f64:                                             # (exact arithmetic has no window: away from fp64 near-ties)
        r_m, _, r_m2, _ = ref_argmax(ref.astype(np.float64), 0.0)
        settled = live & (r_m - r_m2 > 2.0 * (case.S * case.R + 2.0) * 2.0 ** -53 * mag_ref)
    assert np.array_equal(p['best_v'][settled], first[settled].astype(np.int32)), tag
    return float(ratio.max()) if ratio.size else 0.0


# --------------------------------------------------------------------------- #
# Pipelines
# --------------------------------------------------------------------------- #
def ragged_chunk_rows(V):
    """Chunk size (a multiple of 4) that cuts V rows into 3 chunks, the last one shorter."""
    cr = max(4, (2 * V // 5) // 4 * 4)
    assert 2 * cr < V < 3 * cr, (V, cr)
    return cr


# name -> (engine dtype, model variant, Engine mode)
PIPELINES = {
    'f32_projected': ('f32', 'proj', 'sparse'),
    'f32_fused_r1': ('f32', 'fused1', 'sparse'),
    'f32_fused_r3': ('f32', 'fused3', 'sparse'),
    'f32_dense': ('f32', 'proj', 'dense'),
    'split_fused_parent': ('f32', 'fused1', 'sparse'),
    'split_fused_pipelined': ('f32', 'fused1', 'sparse'),
    'split_projected_parent': ('f32', 'proj', 'sparse'),
    'split_projected_pipelined': ('f32', 'proj', 'sparse'),
    'f32_belief_side': ('f32', 'proj', 'sparse'),
    'tiled': ('f32', 'proj', 'sparse'),
    'tiled_split': ('f32', 'proj', 'sparse'),
    'f64_screen_alpha': ('f64', 'proj', 'sparse'),
    'f64_screen_belief': ('f64', 'proj', 'sparse'),
}


def r_gt1_fusion_allowed(rs):
    """The engine's rule for fusing the projection of a model with R > 1 (engine.hip, init: irr_frac_): at most 30 % of
    the (action, 32-state K tile) cells may hold a 4-state chunk whose successors are not consecutive.  The pad states
    behind S count (successor 0), so a model of one or two K tiles whose S is no multiple of 4 never fuses and the
    engine projects instead -- the same scores by the other route."""
    S, A, R = rs.shape
    S_pad = -(-S // 32) * 32
    q = np.zeros((S_pad, A, R), dtype=np.int64)
    q[:S] = rs
    q = q.reshape(S_pad // 4, 4, A, R)
    bad = (q[:, 1] != q[:, 0] + 1) | (q[:, 2] != q[:, 0] + 2) | (q[:, 3] != q[:, 0] + 3)      # chunk, A, R
    cell = bad.any(axis=2).reshape(S_pad // 32, 8, A).any(axis=1)                             # tile, A
    return float(cell.mean()) <= 0.30


def configure(eng, name, case):
    """Route the engine as `name` says; returns the assertions on (stats, probe) that the route ran."""
    checks = []
    split = name.startswith('split') or name == 'tiled_split'
    if eng.dtype == 'f32':
        eng.set_score_split('always' if split else 'off')
        eng.set_formulation('belief' if name == 'f32_belief_side' else 'alpha')
        checks.append(lambda st, p: p['split'] == int(split) and st['score_split'] == int(split))
        checks.append(lambda st, p: p['push'] == int(name == 'f32_belief_side'))
    if name in ('f32_projected', 'split_projected_parent', 'split_projected_pipelined', 'tiled', 'tiled_split'):
        eng.set_fused_projection(False)
        checks.append(lambda st, p: st['fused_projection'] == 0)
    if name in ('f32_fused_r1', 'split_fused_parent', 'split_fused_pipelined'):
        assert case.R == 1 and case.V % 256 != 0 and case.V > 256          # generated tiles AND tiles that straddle groups
        eng.set_fused_projection(True)
        checks.append(lambda st, p: st['fused_projection'] == 1)
    if name == 'f32_fused_r3':
        assert case.R == 3
        eng.set_fused_projection(2)
        fuses = r_gt1_fusion_allowed(case.rs)
        assert fuses or case.S < 64                          # every family but the one- and two-tile models takes the route
        checks.append(lambda st, p: st['fused_projection'] == int(fuses))
    if name.startswith('tiled'):
        eng.set_gamma_tiling('always', ragged_chunk_rows(case.V))
        checks.append(lambda st, p: p['chunks'] == 3 and st['gamma_chunks'] == 3)
    elif name != 'f32_belief_side' and not name.startswith('f64_screen_belief'):
        checks.append(lambda st, p: p['chunks'] == 1)
    if name.startswith('f64_screen'):
        eng.set_f64_screen('always')
        eng.set_formulation('belief' if name.endswith('belief') else 'alpha')
        checks.append(lambda st, p: st['screened'] == 1 and p['push'] == int(name.endswith('belief')))
        checks.append(lambda st, p: p['tol_extra'] == 4.0 * U24 and p['split'] == 0)
    return checks


def run_probe(eng, case, gamma=GAMMA):
    eng.debug_score_probe(True)
    eng.set_alpha(case.alpha)
    eng.set_beliefs(case.b)
    stats = eng.run(gamma)
    return stats, eng.debug_score_probe_fetch()


@pytest.mark.gpu
@pytest.mark.parametrize('family', list(FAMILIES))
@pytest.mark.parametrize('name', list(PIPELINES))
def test_scores_lie_inside_their_windows(name, family):
    from pomdp_pbvi_exploration_amd.engine import debug_split_schedule
    dtype, variant, mode = PIPELINES[name]
    case = family_case(family, variant, dtype == 'f32')      # an fp64 engine gets (and is judged on) the fp64 inputs
    eng = case.engine(dtype, mode)
    prev = debug_split_schedule('pipelined' if name.endswith('pipelined') else 'parent')
    try:
        checks = configure(eng, name, case)
        stats, p = run_probe(eng, case)
    finally:
        debug_split_schedule(prev)
        eng.close()
    for i, ok in enumerate(checks):
        assert ok(stats, p), (name, family, i, {k: v for k, v in p.items() if np.isscalar(v)}, stats)
    check_capture(p, case, f'{name} / {family}')


# Pure fp64 scoring (screen off).  engine.hip f64_uses_mfma: the MFMA GEMM from B * N >= 64 * 64 on (N = Gamma rows);
# gemm_f64.hip gemm_f64_split: one K part once the 128 x 128 tile pairs reach 384, else up to k_tiles / 8 parts.
# R = 1: Gamma's own rounding is the "+ 2" of the bound.
PURE_F64 = {
    # name: (S, A, O, V, B, family of the values, (plain kernel?, K parts == 1?))
    'plain_mixed': (300, 1, 2, 5, 3, 'mixed', (True, True)),
    'mfma_one_part_mixed': (40, 2, 2, 4100, 300, 'mixed', (False, True)),
    'mfma_k_parts_mixed': (8200, 2, 2, 50, 20, 'mixed', (False, False)),
    'mfma_k_parts_same_sign': (8193, 2, 2, 50, 20, 'same_sign', (False, False)),
    'mfma_k_parts_cancel': (8200, 2, 2, 50, 20, 'cancel', (False, False)),
    'mfma_k_parts_range': (8200, 2, 2, 50, 20, 'range', (False, False)),
}


def pure_inputs(rng, S, A, O, V, B, kind):
    rs = successors(rng, S, A, 1, True, step=2)
    rto = sparse_rto(rng, S, A, O, 1, zero=0.0 if kind == 'same_sign' else 0.3)
    b = rng.random((B, S)) * (rng.random((B, S)) < (1.0 if kind == 'same_sign' else 0.2))
    b[np.arange(B), rng.integers(0, S, B)] += 1e-3
    alpha = rng.normal(scale=4.0, size=(V, S))
    if kind == 'same_sign':
        alpha = 1.0 + rng.random((V, S))
    elif kind == 'cancel':
        S2 = S // 2
        rto = np.repeat(rto[:S2], 2, axis=0)
        b = np.repeat(b[:, :S2], 2, axis=1)
        alpha = np.repeat(rng.uniform(0.5, 4.0, size=(V, S2)), 2, axis=1) * np.tile([1.0, -1.0], S2) * (1.0 + 1e-3 * rng.normal(size=(V, S)))
    elif kind == 'range':
        alpha = rng.choice([-1.0, 1.0], size=(V, S)) * 2.0 ** rng.uniform(-30, 30, size=(V, S))
        b = b * 2.0 ** -rng.uniform(0, 40, size=(B, S))
        b[np.arange(B), rng.integers(0, S, B)] = 1.0
        return rs, rto, alpha, b
    return rs, rto, alpha, b / b.sum(axis=1, keepdims=True)


@pytest.mark.gpu
@pytest.mark.parametrize('name', list(PURE_F64))
def test_pure_f64_scores_meet_the_dot_product_bound(name):
    if np.finfo(np.longdouble).nmant < 63:
        pytest.skip('np.longdouble is no wider than float64 here: no reference for fp64 scores')
    S, A, O, V, B, kind, (plain, one_part) = PURE_F64[name]
    case = Case(*pure_inputs(np.random.default_rng(seed_of(name)), S, A, O, V, B, kind), f32=False, longdouble=True)
    eng = case.engine('f64')
    try:
        eng.set_f64_screen('off')
        eng.set_formulation('alpha')
        stats, p = run_probe(eng, case)
    finally:
        eng.close()
    assert stats['screened'] == 0 and p['push'] == 0 and p['split'] == 0 and p['chain_steps'] == -1, (stats, p['chain_steps'])
    assert (p['f64_pairs'] == 0) == plain, p['f64_pairs']
    assert (p['f64_split'] == 1) == one_part, p['f64_split']
    if not plain and one_part:
        assert p['f64_pairs'] >= 384, p['f64_pairs']         # one part because the pairs fill the chip
    check_capture(p, case, f'pure f64 / {name}', pure_f64=True)


# --------------------------------------------------------------------------- #
# Family 6: the argmax's edges
# --------------------------------------------------------------------------- #
def argmax_engine(case, side):
    eng = case.engine('f32')
    eng.set_score_split('off')
    eng.set_formulation(side)
    eng.set_fused_projection(False)
    return eng


@pytest.mark.gpu
@pytest.mark.parametrize('side', ['alpha', 'belief'])
@pytest.mark.parametrize('V', ARGMAX_V)
def test_argmax_edges(V, side):
    """Exact duplicates of the best row at every position the wave merge treats differently, then a runner-up exactly
    one power of two inside 2E and one exactly outside it."""
    vec4 = side == 'belief' or V % 4 == 0                    # k_argmax: fp32 slabs with a pair table, groups 4-aligned
    ran = 0
    for plant in PLANTS:
        for best in sorted({0, V // 2, V - 1}):
            d = plant_position(V, best, plant, vec4)
            if d is None:
                continue
            case = planted_case(V, best, d)
            eng = argmax_engine(case, side)
            try:
                stats, p = run_probe(eng, case)
            finally:
                eng.close()
            assert p['push'] == int(side == 'belief')
            tag = f'argmax V={V} {side} {plant} best={best} dup={d}'
            check_capture(p, case, tag)
            assert np.all(p['score'][:, :, best] == p['score'][:, :, d]), tag       # one K tile: the copies score alike
            assert np.all(p['best_v'] == min(best, d)) and p['qcount'] == case.B * 2, tag
            ran += 1
    assert ran > 0 or V == 1
    # no duplicate: a lone maximum, far from everything else (V = 1: -inf runner-up)
    case = planted_case(V, V // 2, None)
    eng = argmax_engine(case, side)
    try:
        stats, p = run_probe(eng, case)
    finally:
        eng.close()
    check_capture(p, case, f'argmax V={V} {side} lone')
    assert np.all(p['best_v'] == V // 2) and p['qcount'] == 0
    if V < 2:
        return
    # a runner-up just inside 2E (belief 1) and just outside it (belief 0): E is the same for both (m = mag = 1.5)
    E = float(p['E'][0, 0] / p['best_score'][0, 0] * 1.5)
    gap_out = 2.0 ** np.ceil(np.log2(2.0 * E))               # the power of two >= 2E ...
    if gap_out == 2.0 * E:
        gap_out *= 2.0                                       # ... and strictly outside
    assert gap_out / 2.0 <= 2.0 * E < gap_out and gap_out < 2.0 ** -10
    best, q = V // 2, (V // 2 + max(1, V // 3)) % V
    case = Case(*gap_case(V, best, q, gap_out), f32=True)
    eng = argmax_engine(case, side)
    try:
        stats, p = run_probe(eng, case, gamma=1.0)
    finally:
        eng.close()
    tag = f'argmax V={V} {side} gaps'
    check_capture(p, case, tag, gamma=1.0)
    row = {int(c): i for i, c in enumerate(p['perm'])}       # engine row of caller row c
    assert np.all(p['E'] == p['E'][0, 0]) and abs(p['E'][0, 0] - E) <= 1e-6 * E, tag
    assert np.all(p['score'][:, :, best] == 1.5), tag
    assert np.all(p['score'][row[0], :, q] == 1.5 - gap_out) and np.all(p['score'][row[1], :, q] == 1.5 - gap_out / 2.0), tag
    assert sorted(p['queue'].tolist()) == [row[1] * 2, row[1] * 2 + 1], (tag, p['queue'])


# --------------------------------------------------------------------------- #
# The probe's own contract
# --------------------------------------------------------------------------- #
@pytest.mark.gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_probe_changes_nothing_and_is_counted(dtype):
    """Off, on, off again: the same results bit for bit; nothing to fetch before a capture or after switching off; the
    capture's buffers are engine memory like any other and are gone when the probe is switched off.  The live-byte count
    is process-wide: it is compared as its difference from a base taken, after a ``gc.collect()``, before this test's
    engine exists, so engines that other tests of the process left alive do not matter (tests/test_engine_memory.py)."""
    import gc
    from pomdp_pbvi_exploration_amd.engine import load_library
    case = family_case('mixed', 'proj', dtype == 'f32')
    lib = load_library()
    gc.collect()
    base = lib.pbvi_debug_live_bytes()
    eng = case.engine(dtype)
    try:
        if dtype == 'f64':
            eng.set_f64_screen('always')
        with pytest.raises(ValueError, match='nothing captured'):
            eng.debug_score_probe_fetch()
        off = eng.backup_full(case.alpha, case.b, GAMMA)
        held = eng.device_bytes
        eng.debug_score_probe(True)
        with pytest.raises(ValueError, match='nothing captured'):
            eng.debug_score_probe_fetch()
        on = eng.backup_full(case.alpha, case.b, GAMMA)
        p = eng.debug_score_probe_fetch()
        assert p['score'].shape == (case.B, case.A * case.O, case.V)
        grown = eng.device_bytes
        assert grown >= held + p['score'].nbytes and lib.pbvi_debug_live_bytes() - base == grown
        eng.debug_score_probe(False)
        assert eng.device_bytes == held and lib.pbvi_debug_live_bytes() - base == held
        with pytest.raises(ValueError, match='nothing captured'):
            eng.debug_score_probe_fetch()
        again = eng.backup_full(case.alpha, case.b, GAMMA)
        for res in (on, again):
            assert np.array_equal(res.alpha, off.alpha) and np.array_equal(res.actions, off.actions)
            assert np.array_equal(res.best_alpha_ind, off.best_alpha_ind)
            assert res.stats['n_refined'] == off.stats['n_refined']
        # the refinement ran behind the capture: what the probe holds is the argmax's, what the engine returns is final
        assert off.stats['n_refined'] == p['qcount']
    finally:
        eng.close()
    assert lib.pbvi_debug_live_bytes() == base


@pytest.mark.gpu
def test_probe_refuses_a_workload():
    """B * G * V > 2^24: PBVI_EINVAL with a text, and the engine goes on working."""
    S, A, O, V, B = 8, 2, 2, 14000, 300                    # 16.8 M scores
    rng = np.random.default_rng(3)
    case = Case(successors(rng, S, A, 1, True), sparse_rto(rng, S, A, O, 1), rng.normal(size=(V, S)),
                rng.random((B, S)) + 0.1, f32=True)
    eng = case.engine('f32')
    try:
        eng.debug_score_probe(True)
        eng.backup_full(case.alpha, case.b[:10], GAMMA)      # 0.56 M scores: captured
        assert eng.debug_score_probe_fetch()['score'].shape == (10, A * O, V)
        with pytest.raises(ValueError, match='exceeds 2\\^24'):
            eng.backup_full(case.alpha, case.b, GAMMA)
        with pytest.raises(ValueError, match='nothing captured'):    # ... and the earlier capture is not passed off as this run's
            eng.debug_score_probe_fetch()
        eng.debug_score_probe(False)
        res = eng.backup_full(case.alpha, case.b, GAMMA)
        assert np.array_equal(res.best_alpha_ind.reshape(B, A * O), np.argmax(case.scores, axis=2))
    finally:
        eng.close()
