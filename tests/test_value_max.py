"""``max_v b . alpha_v`` (value-max) on every route of the engine, values and indices against exact references.

Routes (engine.hip value_max_device, value_max_store; pbvi_debug_value_max_route says which one a call took):

  f32_skinny      fp32 sparse engine, V <= 64: the fp64 tile engine on fp32 operands (column tiles of 16 / 32 / 48 / 64),
                  K lists from the belief block's zero map alone, K parts folded, k_argmax<double> without a window
  f32_wide_exact  fp32 engine, V > 64 or dense mode: the fp32 stream-K score GEMM, k_argmax with flag_all, k_refine
                  re-scoring every belief in fp64
  f32_wide_fast   the same GEMM after set_value_max_exact(False): its maxima as they are
  f64_mfma/plain  fp64 engine: the MFMA GEMM with its K split from 64 x 64 scores on, else the plain kernel
  store in place  max_value_store on any of them, on 32768-row windows of the belief store
  extras          pbvi_backup_fetch_value_max after a belief-side backup (k_extra_rowmax over the GEMM's extra rows)

Families and references: tests/value_max_cases.py.  Bounds (none is a measurement):

  exact family              array_equal on values and indices, every route, the fast mode included
  near ties, fp32 engines   index == first maximiser of the exact scores for every belief (the family holds no undecided
                            belief: test_near_tie_family_has_no_undecided_belief); |val - exact| <= S 2^-53 M_b[idx]
                            (fp32 products are exact in fp64, the sums are fp64), M_b[v] = sum_s |b_s| |alpha_vs|
  near ties, fp64 engines   the same index; |val - exact| <= (S + 2) 2^-53 M_b[idx] (test_score_window.check_capture)
  fast mode                 |fast - exact| <= tr max(|fast|, mag_b), tr = 8 2^-24 (sqrt(S_pad) + 1), mag_b = sum_s |b_s|
                            max_v |alpha_vs|; its index is a maximiser within 2 tr mag_b of the exact maximum
  extras, fp32              the fast-mode bound with tr + 2 2^-24 (the projected beliefs are rounded once to fp32)
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from model_cases import hub_model
from test_score_window import ARGMAX_V, PLANTS, f32r, host_window
from value_max_cases import (EXACT_B, EXACT_S, EXACT_V, EXTRAS_SHAPE, F64_WIDTHS, KINDS, NEAR_SHAPES, SKINNY_MAX, STORE_WINDOW,
                             U24, U53, ZERO_ROWS, digest, exact_alpha, exact_beliefs, exact_bound_ok, exact_scores_f32,
                             fast_window, first_argmax, k_tiles, longdouble_is_wide, longdouble_scores, make_engine, near_case,
                             planted_alpha, planted_pairs, s_pad, store_beliefs)

gpu = pytest.mark.gpu

ENGINE_KINDS = {'f32_sparse': ('f32', 'sparse'), 'f32_dense': ('f32', 'dense'), 'f64': ('f64', 'sparse')}


def expected_route(dtype, mode, V, B, exact=True):
    """engine.hip: vmax_skinny, f64_uses_mfma (the fp64 GEMM has V + 1 rows: the magnitude row rides along)."""
    if dtype == 'f64':
        return 'f64_mfma' if B * (V + 1) >= 64 * 64 else 'f64_plain'
    if mode == 'sparse' and V <= SKINNY_MAX:
        return 'f32_skinny'
    return 'f32_wide_exact' if exact else 'f32_wide_fast'


def f64_bn(N):
    """gemm_f64.hip gemm_f64_bn."""
    return 16 if N <= 16 else 32 if N <= 32 else 48 if N <= 48 else 64 if N <= 64 else 128


def f64_split(M, N, kt32):
    """gemm_f64.hip gemm_f64_split."""
    pairs = -(-M // 128) * -(-N // f64_bn(N))
    if pairs >= 384:
        return 1
    z = min(-(-2048 // pairs), max(1, kt32 // 8), max(1, (64 << 20) // (M * N * 8)))
    return min(z, 32)


# --------------------------------------------------------------------------- #
# 1. CPU: the references and the families do what they say
# --------------------------------------------------------------------------- #
def test_first_argmax_on_hand_written_rows():
    rows = np.array([[1.0, 3.0, 2.0, 3.0],                   # the first maximum among equal values
                     [4.0, 1.0, 3.0, -2.0],                  # the maximum in column 0
                     [0.0, 1.0, 2.0, 4.0],                   # the maximum in the last column
                     [0.0, 0.0, 0.0, 0.0]])                  # what an all-zero belief scores
    val, idx = first_argmax(rows)
    assert idx.tolist() == [1, 0, 3, 0] and val.tolist() == [3.0, 4.0, 4.0, 0.0]
    alpha = np.array([[1.0, -2.0], [3.0, 5.0], [3.0, 5.0]])
    b = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, -1.0]])
    val, idx = first_argmax(b @ alpha.T)
    assert idx.tolist() == [0, 1, 0] and val.tolist() == [0.0, 3.0, 2.0]
    val, idx = first_argmax(exact_scores_f32(alpha, b))
    assert idx.tolist() == [0, 1, 0] and val.tolist() == [0.0, 3.0, 2.0]


def test_exact_sum_reference_is_correctly_rounded():
    """1 + 2^-30 - 1 over three fp32-valued products: a float64 running sum in the wrong order loses the middle term,
    fsum does not; and longdouble agrees on a random case to its own precision."""
    alpha = f32r(np.array([[1.0, 2.0 ** -60, -1.0], [1.0, 0.0, -1.0]]))
    b = np.ones((1, 3))
    assert exact_scores_f32(alpha, b).tolist() == [[2.0 ** -60, 0.0]]
    rng = np.random.default_rng(1)
    alpha, b = f32r(rng.normal(size=(9, 300))), f32r(rng.random((4, 300)))
    ex = exact_scores_f32(alpha, b)
    if longdouble_is_wide():
        M = np.abs(b) @ np.abs(alpha).T
        assert np.all(np.abs(longdouble_scores(alpha, b) - ex) <= 300 * 2.0 ** -63 * M)


@pytest.mark.parametrize('S', EXACT_S)
def test_exact_family_is_exact_in_every_format(S):
    assert exact_bound_ok(S)
    V = 130
    alpha = exact_alpha(S, V)
    for k in (1, 2, 3):
        b = exact_beliefs(S, k)
        for x, lim in ((alpha, 15), (b, 7)):
            assert np.array_equal(x, np.rint(x)) and np.abs(x).max() <= lim
        # representable in bf16 (8 significant bits), hence in fp32 and fp64
        assert np.array_equal(alpha, (alpha.astype(np.float32).view(np.uint32) & 0xffff0000).view(np.float32).astype(np.float64))
        assert (np.abs(b) @ np.abs(alpha).T).max() < 2 ** 24
        sc = b @ alpha.T
        assert np.array_equal(sc, b.astype(np.int64) @ alpha.astype(np.int64).T)          # the integer reference
        assert np.array_equal(sc, (b.astype(np.float32) @ alpha.astype(np.float32).T).astype(np.float64))
        # rows 0 .. 255 share one support of min(k, tiles) K tiles; the rows behind differ; zero rows are zero
        tiles = lambda row: set((np.flatnonzero(row) // 32).tolist())
        shared = set().union(*(tiles(r) for r in b[:256]))
        assert len(shared) == min(k, k_tiles(S))
        assert all(len(tiles(r)) <= 3 for r in b[256:])
        if k_tiles(S) > 3:
            assert len(set().union(*(tiles(r) for r in b[256:]))) > 3
        assert all(not b[z].any() for z in ZERO_ROWS) and b[0].any()
        # ties are common: the first maximiser is asked for, not just a maximiser
        val, idx = first_argmax(sc)
        assert ((sc == val[:, None]).sum(axis=1) > 1).sum() > len(ZERO_ROWS)


def test_planted_maxima_sit_where_they_say():
    for V in EXACT_V:
        pairs = planted_pairs(V)
        assert (V // 2, None) in pairs
        b = exact_beliefs(33, 2, B=20, signed=False, zero_rows=())
        assert b.min() >= 0 and np.all(b.sum(axis=1) > 0)
        for p, d in pairs:
            alpha = planted_alpha(33, V, p, d)
            val, idx = first_argmax(b @ alpha.T)
            assert np.all(idx == (p if d is None else min(p, d))) and np.all(val == 15.0 * b.sum(axis=1))
        dups = [(p, d) for p, d in pairs if d is not None]
        assert dups or V == 1
        if V > 128:
            assert any(p // 128 != d // 128 for p, d in dups)                      # in another 128-column tile
        if V > 64:
            assert (63, 64) in dups                                                # across the 64 | 65 boundary
        assert any(d == V - 1 or p == V - 1 for p, d in dups) or V == 1            # last column
        assert any(d == 0 or p == 0 for p, d in dups) or V == 1                    # column 0
    assert set(ARGMAX_V) | set(F64_WIDTHS) == set(EXACT_V) and {64, 65} <= set(EXACT_V) and len(PLANTS) == 5


def near_tie_cases():
    """Every (kind, shape, precision of the operands) the GPU tests of the near-tie family use."""
    out = []
    for kind in KINDS:
        for name, (S, B, V, dtype, mode, route) in NEAR_SHAPES.items():
            out.append((kind, S, B, V, dtype == 'f32'))
        S, B, V = EXTRAS_SHAPE
        out += [(kind, S, B, V, True), (kind, S, B, V, False)]
    return sorted(set(out))


@pytest.mark.parametrize('kind,S,B,V,f32', near_tie_cases())
def test_near_tie_family_has_no_undecided_belief(kind, S, B, V, f32):
    """The two conditions the GPU tests rest on: no belief's top two distinct exact scores are closer than
    2 (S + 2) 2^-53 max_v M_b[v] (so every route must return the reference's index for EVERY belief), and in at least a
    quarter of the beliefs they are closer than the fp32 window 8 2^-24 mag_b (so an fp32 GEMM alone cannot)."""
    if not f32 and not longdouble_is_wide():
        pytest.skip('np.longdouble is no wider than float64 here: no reference for fp64 operands')
    c = near_case(kind, S, B, V, f32)
    assert np.array_equal(c.alpha, f32r(c.alpha)) == f32
    if V > 7:
        assert np.array_equal(c.alpha[7], c.alpha[3])
    nnz = (c.b != 0).sum(axis=1)
    assert nnz.min() >= 1 and nnz.mean() <= 0.07 * S and np.allclose(c.b.sum(axis=1), 1.0, atol=1e-6)
    assert not c.undecided().any()
    share = float(c.inside_f32_window().mean())
    print(f'\n[value-max] {kind} S={S} B={B} V={V} f32={f32}: inside the fp32 window {share:.3f}, '
          f'smallest gap {float((c.gaps() / c.mag).min()):.3e} mag')
    assert share >= 0.25
    assert not np.any(c.idx == 7) or V <= 7
    if kind == 'cancel':                                     # the magnitude is well above the value
        assert np.median(np.abs(c.val) / c.mag) < 0.5
    else:
        assert np.median(np.abs(c.val) / c.mag) > 0.99


# --------------------------------------------------------------------------- #
# 2. GPU: the exact family on every route and edge
# --------------------------------------------------------------------------- #
def all_entry_points(eng, alpha, b, tag, dtype, mode):
    """max_value, max_value_resident, max_value_store and (fp32) the fast mode on one alpha set and belief block; the
    route each one reported."""
    want_val, want_idx = first_argmax(b @ alpha.T)
    B, V = b.shape[0], alpha.shape[0]
    routes = []

    def same(got, what):
        val, idx = got
        assert np.array_equal(idx, want_idx), (tag, what, np.flatnonzero(idx != want_idx)[:8])
        assert np.array_equal(val, want_val), (tag, what, np.flatnonzero(val != want_val)[:8])
        routes.append(eng.debug_value_max_route())

    same(eng.max_value(alpha, b), 'max_value')
    calls = routes[-1]['calls']
    same(eng.max_value_resident(), 'resident')
    assert routes[-1]['calls'] == calls + 1, tag
    eng.reset_store('belief')
    eng.store_rows('belief', b)
    same(eng.max_value_store(), 'store')
    if dtype == 'f32':
        eng.set_value_max_exact(False)
        try:
            same(eng.max_value_resident(), 'fast resident')
            fast_route = routes[-1]['route']
            same(eng.max_value_store(), 'fast store')
        finally:
            eng.set_value_max_exact(True)
        assert fast_route == expected_route(dtype, mode, V, B, exact=False), (tag, fast_route)
    for r in routes[:3]:
        assert r['route'] == expected_route(dtype, mode, V, B), (tag, r)
        assert r['rows'] == B and r['alpha_rows'] == V, (tag, r)
    return routes[1]


@gpu
@pytest.mark.parametrize('S', EXACT_S)
@pytest.mark.parametrize('kind', list(ENGINE_KINDS))
def test_exact_family_on_every_route(kind, S):
    dtype, mode = ENGINE_KINDS[kind]
    beliefs = {k: exact_beliefs(S, k) for k in (1, 2, 3)}
    seen, k_parts = set(), set()
    eng = make_engine(S, dtype, mode)
    try:
        for iv, V in enumerate(EXACT_V):
            alpha = exact_alpha(S, V)
            for ib, B in enumerate(EXACT_B):
                b = beliefs[1 + (iv + ib) % 3][:B]
                r = all_entry_points(eng, alpha, b, (kind, S, V, B), dtype, mode)
                seen.add((r['route'], r['bn']))
                if B == max(EXACT_B):
                    k_parts.add(r['k_parts'])
                if r['route'] == 'f32_skinny':
                    assert r['bn'] == f64_bn(V) and r['k_parts'] == f64_split(B, V, k_tiles(S)), (kind, S, V, B, r)
                elif r['route'] == 'f64_mfma':
                    assert r['bn'] == f64_bn(V + 1) and r['k_parts'] == f64_split(B, V + 1, k_tiles(S)), (kind, S, V, B, r)
    finally:
        eng.close()
    routes = {r for r, _ in seen}
    if kind == 'f32_sparse':                                 # V = 64 and V = 65 took different routes, every width ran
        assert routes == {'f32_skinny', 'f32_wide_exact'}
        assert {bn for r, bn in seen if r == 'f32_skinny'} == {16, 32, 48, 64}
    elif kind == 'f32_dense':
        assert routes == {'f32_wide_exact'}
    else:
        assert routes == {'f64_mfma', 'f64_plain'}
        # (16 never: the GEMM has V + 1 rows and B (V + 1) >= 4096 with B <= 333 needs V >= 12 ... of EXACT_V, V >= 16)
        assert {bn for r, bn in seen if r == 'f64_mfma'} == {32, 48, 64, 128}
    if kind != 'f32_dense':                                  # S = 1056: 33 K tiles, four K parts; S = 33: one
        assert max(k_parts) == {33: 1, 600: 2, 1056: 4}[S], k_parts


@gpu
@pytest.mark.parametrize('S', EXACT_S)
@pytest.mark.parametrize('kind', list(ENGINE_KINDS))
def test_planted_maxima_on_every_route(kind, S):
    """The winning row and an exact copy of it at the positions k_argmax's wave merge, the 128-column tiles and the
    skinny / wide switch treat differently: the lower index of the two, the value 15 sum(b), bit for bit."""
    dtype, mode = ENGINE_KINDS[kind]
    b = exact_beliefs(S, 3, B=130, signed=False, zero_rows=(64,))
    eng = make_engine(S, dtype, mode)
    try:
        eng.set_beliefs(b)
        eng.store_rows('belief', b)
        for V in EXACT_V:
            for p, d in planted_pairs(V):
                alpha = planted_alpha(S, V, p, d)
                want_val, want_idx = first_argmax(b @ alpha.T)
                first = p if d is None else min(p, d)
                assert np.all(np.delete(want_idx, 64) == first) and want_idx[64] == 0
                eng.set_alpha(alpha)
                got = [eng.max_value_resident(), eng.max_value_store()]
                if dtype == 'f32':
                    eng.set_value_max_exact(False)
                    got.append(eng.max_value_resident())
                    eng.set_value_max_exact(True)
                for val, idx in got:
                    assert np.array_equal(idx, want_idx) and np.array_equal(val, want_val), (kind, S, V, p, d)
                assert eng.debug_value_max_route()['route'] == expected_route(dtype, mode, V, 130, exact=False), (V, p, d)
    finally:
        eng.close()


@gpu
@pytest.mark.parametrize('S', EXACT_S)
@pytest.mark.parametrize('kind', list(ENGINE_KINDS))
def test_zero_blocks_still_run_the_route(kind, S):
    """A block of all-zero beliefs has an empty K list: the GEMM writes its zeros, the argmax answers (0.0, 0) -- and the
    route is the one the shape asks for, not a shortcut.  Then the same behind 256 live rows (rows 256 .. 383: one 128-row
    tile of the fp64 engine, one empty 256-row block of the zero map)."""
    dtype, mode = ENGINE_KINDS[kind]
    eng = make_engine(S, dtype, mode)
    try:
        for V in (40, 96):
            alpha = exact_alpha(S, V)
            zero = np.zeros((128, S))
            before = None
            for what, b in (('all zero', zero), ('zero tail', np.concatenate([exact_beliefs(S, 2, B=256), zero]))):
                want_val, want_idx = first_argmax(b @ alpha.T)
                assert np.all(want_val[-128:] == 0.0) and np.all(want_idx[-128:] == 0)
                eng.reset_store('belief')
                eng.store_rows('belief', b)
                for entry in ('max_value', 'store'):
                    val, idx = eng.max_value(alpha, b) if entry == 'max_value' else eng.max_value_store()
                    assert np.array_equal(idx, want_idx) and np.array_equal(val, want_val), (kind, S, V, what, entry)
                    r = eng.debug_value_max_route()
                    assert r['route'] == expected_route(dtype, mode, V, len(b)) and r['rows'] == len(b), (kind, S, V, what, r)
                    assert before is None or r['calls'] == before + 1, (kind, S, V, what, r)
                    before = r['calls']
    finally:
        eng.close()


# --------------------------------------------------------------------------- #
# 3. GPU: the near-tie family
# --------------------------------------------------------------------------- #
def check_near(c, val, idx, dtype, tag):
    assert np.array_equal(idx, c.idx), (tag, np.flatnonzero(idx != c.idx)[:8])
    assert not np.any(idx == 7) or c.V <= 7, tag
    n = c.S if dtype == 'f32' else c.S + 2
    bound = n * U53 * c.M[np.arange(c.B), c.idx]
    err = np.abs(val - c.val)
    ratio = float(np.max(np.divide(err, bound, out=np.zeros_like(err), where=bound > 0)))
    print(f'\n[value-max] {tag}: max |err| / bound = {ratio:.4f}')
    assert np.all(err <= bound), (tag, ratio)


def check_fast(c, val, idx, tr, tag):
    scale = np.maximum(np.abs(val), c.mag)
    err = np.abs(val - c.val)
    ratio = float(np.max(err / (tr * scale)))
    print(f'\n[value-max] {tag}: max |fast - exact| / (tr max(|fast|, mag)) = {ratio:.4f}')
    assert np.all(err <= tr * scale), (tag, ratio)
    if idx is not None:
        assert np.all(c.exact[np.arange(c.B), idx] >= c.val - 2.0 * tr * c.mag), tag


@gpu
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('name', list(NEAR_SHAPES))
def test_near_ties_on_every_route(name, kind):
    S, B, V, dtype, mode, route = NEAR_SHAPES[name]
    if dtype == 'f64' and not longdouble_is_wide():
        pytest.skip('np.longdouble is no wider than float64 here: no reference for fp64 operands')
    c = near_case(kind, S, B, V, dtype == 'f32')
    eng = make_engine(S, dtype, mode)
    try:
        val_r, idx_r = eng.max_value(c.alpha, c.b)
        r = eng.debug_value_max_route()
        assert r['route'] == route and r['rows'] == B and r['alpha_rows'] == V, r
        if route == 'f32_wide_exact':
            # The re-scoring pass ran on this call's queue.  A belief takes a slot of the grid-wide passes when more than
            # defer_min of its scores lie inside the window, else its own block settles it: with the window derived on the
            # device from the stream-K share the count is not the host's to know ...
            rc = eng.debug_refine_counts()
            assert 0 < rc['slots'] <= B and rc['q2'] == 0, rc
            # ... with the window at its documented upper limit it is: more than defer_min rows of every belief lie
            # within HALF of it (the other half covers the GEMM's own error), so the pass reserved one slot per belief
            tr = fast_window(S)
            scale = np.maximum(np.abs(c.val), c.mag)
            inside = (c.exact >= (c.val - tr * scale)[:, None]).sum(axis=1)
            assert inside.min() > rc['defer_min'] >= 0, (int(inside.min()), rc)
            eng.set_tie_window(tr)
            try:
                val_w, idx_w = eng.max_value_resident()
                rc = eng.debug_refine_counts()
            finally:
                eng.set_tie_window(-1.0)
            assert rc['slots'] == B, rc
            check_near(c, val_w, idx_w, dtype, f'{name} / {kind} resident, window at its upper limit')
        if route == 'f64_mfma':
            assert B * V >= 4096 and r['k_parts'] > 1 and r['bn'] == 128, r
        if route == 'f32_skinny':
            assert r['k_parts'] > 1 and r['bn'] == 48, r
        check_near(c, val_r, idx_r, dtype, f'{name} / {kind} resident')
        eng.store_rows('belief', c.b)
        val_s, idx_s = eng.max_value_store()
        assert eng.debug_value_max_route()['route'] == route
        check_near(c, val_s, idx_s, dtype, f'{name} / {kind} store')
        if route == 'f32_wide_exact':                        # the store call and the resident call stay bit-identical
            assert np.array_equal(val_s, val_r)
        if dtype == 'f32':
            tr = fast_window(S)
            assert tr == host_window({'tol_rel': -1.0, 'chain_steps': s_pad(S) // 32, 'split': 0, 'push': 0})
            eng.set_value_max_exact(False)
            try:
                fast_r, fidx_r = eng.max_value_resident()
                rf = eng.debug_value_max_route()['route']
                fast_s, fidx_s = eng.max_value_store()
            finally:
                eng.set_value_max_exact(True)
            assert rf == ('f32_skinny' if route == 'f32_skinny' else 'f32_wide_fast'), rf
            check_fast(c, fast_r, fidx_r, tr, f'{name} / {kind} fast resident')
            check_fast(c, fast_s, fidx_s, tr, f'{name} / {kind} fast store')
            if route == 'f32_skinny':                        # no window, nothing to switch off
                assert np.array_equal(fast_r, val_r) and np.array_equal(fidx_r, idx_r)
            elif kind == 'cancel':                           # it really is the un-rescored value
                assert not np.array_equal(fast_r, val_r)
            again, idx_again = eng.max_value_resident()
            assert np.array_equal(again, val_r) and np.array_equal(idx_again, idx_r)
    finally:
        eng.close()


# --------------------------------------------------------------------------- #
# 4. GPU: store windows
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_store_past_one_window(dtype):
    """A store of 32768 + 513 rows (then + 300), appended in pieces that leave partial 256-row blocks, scored in place
    against V = 5 (skinny) and V = 70 (wide exact): every prefix equals the integer reference bit for bit."""
    S = 40
    n0, extra = STORE_WINDOW + 513, 300
    b = store_beliefs(S, n0 + extra)
    alphas = {V: exact_alpha(S, V) for V in (5, 70)}
    want = {V: first_argmax(b @ a.T) for V, a in alphas.items()}
    assert not b[STORE_WINDOW:STORE_WINDOW + 256].any() and b[STORE_WINDOW + 256:n0].any()
    eng = make_engine(S, dtype)

    def check(V, n, tag):
        before = eng.debug_value_max_route()['calls']
        val, idx = eng.max_value_store(n)
        assert np.array_equal(idx, want[V][1][:n]), (tag, V, n, np.flatnonzero(idx != want[V][1][:n])[:8])
        assert np.array_equal(val, want[V][0][:n]), (tag, V, n, np.flatnonzero(val != want[V][0][:n])[:8])
        r = eng.debug_value_max_route()
        windows = -(-n // STORE_WINDOW)
        assert r['calls'] == before + windows and r['rows'] == n - (windows - 1) * STORE_WINDOW, (tag, V, n, r)
        last = r['rows']
        assert r['route'] == expected_route(dtype, 'sparse', V, last), (tag, V, n, r)

    try:
        eng.set_alpha(alphas[5])
        eng.set_beliefs(b[:3])                               # (a resident block: the store call must leave it alone)
        eng.max_value_resident()
        at = 0
        for piece in (100, 7001):                            # 7101 rows: the map's last block is partial
            eng.store_rows('belief', b[at:at + piece])
            at += piece
        check(5, at, 'first pieces')
        for piece in (25667, n0 - 100 - 7001 - 25667):
            eng.store_rows('belief', b[at:at + piece])
            at += piece
        assert at == n0
        for V in (5, 70):
            eng.set_alpha(alphas[V])
            for n in (1, 255, 256, 257, STORE_WINDOW - 1, STORE_WINDOW, STORE_WINDOW + 1, n0):
                check(V, n, 'prefix')
            ids = np.arange(0, n0, 2)
            assert np.array_equal(eng.best_alpha_of_store_rows(ids), want[V][1][ids]), V
        # 300 more rows: the maps and lists of the rows seen before are reused, the last window's end moves inside a block
        eng.store_rows('belief', b[n0:])
        for V in (70, 5):
            eng.set_alpha(alphas[V])
            check(V, n0 + extra, 'after the second append')
            check(V, n0, 'old prefix after the second append')
        val, idx = eng.max_value_resident()                  # the resident block is still the three rows
        assert np.array_equal(idx, want[5][1][:3]) and np.array_equal(val, want[5][0][:3])
    finally:
        eng.close()


# --------------------------------------------------------------------------- #
# 5. GPU: the belief-side backup's extra rows
# --------------------------------------------------------------------------- #
@gpu
@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_belief_side_extras_under_cancellation(dtype):
    from pomdp_pbvi_exploration_amd.engine import Engine
    if dtype == 'f64' and not longdouble_is_wide():
        pytest.skip('np.longdouble is no wider than float64 here: no reference for fp64 operands')
    S, B, V = EXTRAS_SHAPE
    c = near_case('cancel', S, B, V, dtype == 'f32')
    rs, rto = hub_model(S)
    er = np.zeros((S, 2))
    eng = Engine(S, 2, 2, 2, rs, rto, er, dtype=dtype)
    try:
        eng.set_formulation('belief')
        if dtype == 'f64':
            eng.set_f64_screen('off')
        eng.debug_score_probe(True)
        eng.set_alpha(c.alpha)
        eng.set_beliefs(c.b)
        st = eng.run(0.9375)
        assert st['formulation'] == 2 and st['screened'] == 0, st
        perm = eng.debug_score_probe_fetch()['perm']
        assert sorted(perm.tolist()) == list(range(B)) and not np.array_equal(perm, np.arange(B))     # a sorted block
        out = np.empty(B, dtype=np.float64)
        assert eng._lib.pbvi_backup_fetch_value_max(eng._h, out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    finally:
        eng.close()
    if dtype == 'f32':
        check_fast(c, out, None, fast_window(S) + 2.0 * U24, 'extras f32')
    else:
        bound = (S + 2) * U53 * c.M[np.arange(B), c.idx]
        assert np.all(np.abs(out - c.val) <= bound), float(np.max(np.abs(out - c.val) / bound))
    # caller order: against the engine's order the values would miss by far more than the bound
    wrong = np.abs(c.val[perm] - c.val)
    assert np.median(wrong) > 1e3 * fast_window(S) * np.median(c.mag)


# --------------------------------------------------------------------------- #
# 6. PBVI_NO_SKINNY: V <= 64 through the wide route, in one child process
# --------------------------------------------------------------------------- #
CHILD_EXACT = (600, (1, 5, 16, 33, 63, 64), 257)             # S, V values, B


def run_child_cases():
    """What tests/value_max_child.py prints, and what the parent computes in its own process: one line per case with
    the route and digests of the answers (exact family: values and indices; near ties: indices)."""
    lines = []
    S, Vs, B = CHILD_EXACT
    eng = make_engine(S, 'f32')
    try:
        b = exact_beliefs(S, 2)[:B]
        eng.store_rows('belief', b)
        for V in Vs:
            alpha = exact_alpha(S, V)
            want_val, want_idx = first_argmax(b @ alpha.T)
            val, idx = eng.max_value(alpha, b)
            route = eng.debug_value_max_route()['route']
            sval, sidx = eng.max_value_store()
            assert np.array_equal(idx, want_idx) and np.array_equal(val, want_val), V
            assert np.array_equal(sidx, want_idx) and np.array_equal(sval, want_val), V
            lines.append(f'value-max-sha256 exact{V} {route} {digest(val, idx.astype(np.int64))}')
    finally:
        eng.close()
    for kind in KINDS:
        S, B, V = NEAR_SHAPES['f32_skinny'][:3]
        c = near_case(kind, S, B, V, True)
        eng = make_engine(S, 'f32')
        try:
            val, idx = eng.max_value(c.alpha, c.b)
            route = eng.debug_value_max_route()['route']
            check_near(c, val, idx, 'f32', f'child {kind}')
            lines.append(f'value-max-sha256 near_{kind} {route} {digest(idx.astype(np.int64))}')
        finally:
            eng.close()
    return lines


@gpu
def test_small_alpha_sets_on_the_wide_route_in_a_child():
    """``PBVI_NO_SKINNY`` is read once per process: one fresh child runs V <= 64 through the fp32 score GEMM and the
    refinement on the same data; bit-identical answers in the exact family, identical indices on the near ties."""
    mine = [ln.split() for ln in run_child_cases()]
    assert all(ln[2] == 'f32_skinny' for ln in mine), mine
    env = dict(os.environ)
    env['PBVI_NO_SKINNY'] = '1'
    child = subprocess.run([sys.executable, os.path.join(REPO, 'tests', 'value_max_child.py')], env=env, cwd=REPO,
                           stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)
    assert child.returncode == 0, child.stdout + child.stderr
    theirs = [ln.split() for ln in child.stdout.splitlines() if ln.startswith('value-max-sha256 ')]
    assert len(theirs) == len(mine), child.stdout + child.stderr
    for m, t in zip(mine, theirs):
        assert t[1] == m[1] and t[2] == 'f32_wide_exact' and t[3] == m[3], (m, t)
