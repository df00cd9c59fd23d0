"""Every entry point that hands a result to the caller, with its destination in each kind of memory the engine tells
apart -- pageable host memory (through the pinned staging buffer), page-locked host memory (the DMA writes it) and device
memory (device to device): the three results must be the same bytes.  The other suites pin the values of these calls into
one kind of memory each; this one pins that the route does not matter, that the fetches agree with each other exactly,
that a belief walk (which uses the staging buffer as raw pinned memory, on the side stream) leaves the next delivery
intact, and that a fetch without a resident result raises and leaves its destination alone.

Model: random padded-ELL, S = 70 (S_pad = 96 > S), A = 3, O = 4, R = 2, V = 20.  B = 40 is an unsorted block, B = 300 more
than one 256-row block: sorted, the one case where rows come back through the caller-order scatter."""
import ctypes as C

import numpy as np
import pytest
import torch                 # before the engine's library is loaded: torch finds no GPU once another HIP runtime is up

from pomdp_pbvi_exploration_amd.engine import Engine, PinnedBuffer
from test_limits_and_delivery import r32, random_model

pytestmark = pytest.mark.gpu

S, A, O, R, V = 70, 3, 4, 2, 20
GAMMA = 0.95
SENTINEL = 0xA5
KINDS = ('pageable', 'pinned', 'device')
HOST_KINDS = KINDS[:2]
I32, U8, F64 = np.int32, np.uint8, np.float64


class Dst:
    """A destination of ``shape`` / ``dtype`` in one kind of memory, every byte SENTINEL."""

    def __init__(self, kind, shape, dtype, pinned):
        self.shape, self.dtype = tuple(int(x) for x in shape), np.dtype(dtype)
        nbytes = max(int(np.prod(self.shape)) * self.dtype.itemsize, 1)
        if kind == 'device':
            self.t = torch.full((nbytes,), SENTINEL, dtype=torch.uint8, device='cuda')
            torch.cuda.synchronize()                         # (the engine copies on a stream of its own)
            self.ptr = self.t.data_ptr()
        else:
            self.a = np.empty(nbytes, U8) if kind == 'pageable' else pinned.carve((nbytes,), U8)
            self.a[:] = SENTINEL
            self.ptr = self.a.ctypes.data

    def p(self, ctype=None):
        return C.c_void_p(self.ptr) if ctype is None else C.cast(self.ptr, C.POINTER(ctype))

    def read(self):
        raw = self.t.cpu().numpy() if hasattr(self, 't') else np.array(self.a)
        return raw[:int(np.prod(self.shape)) * self.dtype.itemsize].view(self.dtype).reshape(self.shape)


def host_step(b, a, rs, rto):
    """The likeliest observation after action ``a`` in belief ``b`` and the belief it leads to."""
    o = int(np.argmax(b @ rto[:, a].sum(axis=2)))
    nb = np.zeros(S)
    np.add.at(nb, rs[:, a, :], b[:, None] * rto[:, a, o, :])
    return o, nb / nb.sum()


def make_beliefs(rng, B):
    """Beliefs whose first 32-state tile with mass (the engine's sort key) varies from row to row, in shuffled order."""
    b = rng.random((B, S)) * (rng.random((B, S)) < 0.5)
    first = rng.integers(0, 3, B) * 32
    b[np.arange(S)[None, :] < first[:, None]] = 0.0
    b[np.arange(B), first] += 0.1
    return r32(b / b.sum(axis=1, keepdims=True))


# name -> (kinds, outputs as (shape, dtype) with B / U / T / N (message length) / P (its block size) by name, the call)
def _entries():
    i32, u8, f64 = C.c_int32, C.c_uint8, C.c_double
    return {
        'fetch': (KINDS, [('B S', 'T'), ('B', I32), ('B A O', I32), ('B', U8)],
                  lambda sc, d: sc.lib.pbvi_backup_fetch(sc.h, d[0].p(), d[1].p(i32), d[2].p(i32), d[3].p(u8))),
        'fetch_unique': (KINDS, [('U S', 'T'), ('B', I32)],
                         lambda sc, d: sc.lib.pbvi_backup_fetch_unique(sc.h, d[0].p(), d[1].p(i32))),
        'fetch_compact': (KINDS, [('U S', 'T'), ('B', I32), ('B', I32), ('B A O', I32), ('B', U8)],
                          lambda sc, d: sc.lib.pbvi_backup_fetch_compact(sc.h, d[0].p(), d[1].p(i32), d[2].p(i32), d[3].p(i32),
                                                                         d[4].p(u8))),
        'fetch_unique_keys': (KINDS, [('U K', I32)], lambda sc, d: sc.lib.pbvi_backup_fetch_unique_keys(sc.h, d[0].p())),
        'fetch_exchange': (KINDS, [('N', I32)], lambda sc, d: sc.lib.pbvi_backup_fetch_exchange(sc.h, d[0].p())),
        'fetch_exchange_padded': (KINDS, [('NP', I32)],
                                  lambda sc, d: sc.lib.pbvi_backup_fetch_exchange_padded(sc.h, sc.dims['P'], d[0].p())),
        'assemble_rows': (KINDS, [('U S', 'T')],
                          lambda sc, d: sc.lib.pbvi_assemble_rows(sc.h, GAMMA, sc.dims['U'], sc.keys.ctypes.data_as(C.c_void_p), d[0].p())),
        'assemble_rows_store': (KINDS, [('U S', 'T')], lambda sc, d: sc.assemble_store(d[0])),
        'beliefs_fetch': (KINDS, [('B S', 'T')], lambda sc, d: sc.lib.pbvi_beliefs_fetch(sc.h, d[0].p())),
        'belief_update': (KINDS, [('B S', 'T')],
                          lambda sc, d: sc.lib.pbvi_belief_update(sc.h, sc.act.ctypes.data_as(C.POINTER(i32)),
                                                                  sc.obs.ctypes.data_as(C.POINTER(i32)), d[0].p())),
        'value_max': (HOST_KINDS, [('B', F64), ('B', I32)], lambda sc, d: sc.lib.pbvi_value_max(sc.h, d[0].p(f64), d[1].p(i32))),
        'infotaxis': (HOST_KINDS, [('B A', F64), ('B', I32), ('B A O', F64), ('B', F64)],
                      lambda sc, d: sc.lib.pbvi_infotaxis(sc.h, d[0].p(f64), d[1].p(i32), d[2].p(f64), d[3].p(f64))),
        # (overwrites the backup's stage buffers and drops its result: the scene runs the backup again behind it)
        'q_values': (HOST_KINDS, [('B A', F64), ('B', I32), ('B A O', I32)],
                     lambda sc, d: sc.q_values(d)),
    }


ENTRIES = _entries()
NEED_RESULT = {'fetch': 'backup_fetch: no backup result resident (call pbvi_backup_run first)',
               'fetch_unique': 'backup_fetch_unique: no backup result resident',
               'fetch_compact': 'backup_fetch_compact: no backup result resident',
               'fetch_unique_keys': 'backup_fetch_unique_keys: no backup result resident',
               'fetch_exchange': 'backup_fetch_exchange: no backup result resident',
               'fetch_exchange_padded': 'backup_fetch_exchange: no backup result resident'}


class Scene:
    """One engine after one backup; every entry delivered into every kind of memory before and after a belief walk."""

    def __init__(self, dtype, B):
        rng = np.random.default_rng(1000 + B)
        self.rs, self.rto, self.er = random_model(rng, S, A, O, R)
        self.alpha, self.beliefs = r32(rng.normal(size=(V, S))), make_beliefs(rng, B)
        self.eng = eng = Engine(S, A, O, R, self.rs, self.rto, self.er, dtype=dtype)
        self.lib, self.h, self.T = eng._lib, eng._h, eng.np_dtype
        self.pinned = PinnedBuffer(16 << 20)
        eng.set_alpha(self.alpha)
        eng.set_beliefs(self.beliefs)
        eng.debug_score_probe(True)
        eng.run(GAMMA)
        self.perm = eng.debug_score_probe_fetch()['perm']
        eng.debug_score_probe(False)
        U = eng.unique_count
        self.dims = dict(B=B, S=S, A=A, O=O, U=U, K=1 + O, P=B + 7, N=eng.exchange_size(B), NP=eng.exchange_size(B + 7))
        self.keys = eng.fetch_unique_keys()
        self.act = (np.arange(B) % A).astype(I32)
        self.obs = np.array([host_step(b, a, self.rs, self.rto)[0] for b, a in zip(self.beliefs, self.act)], dtype=I32)
        self.store_firsts = []
        self.before = self.deliver_all()
        b, walk_obs = self.beliefs[0], []
        for _ in range(8):                                   # 8 steps: the quarters leave through the raw staging buffer
            o, b = host_step(b, 0, self.rs, self.rto)
            walk_obs.append(o)
        self.walk, _ = eng.belief_walk(self.beliefs[0], np.zeros(8, I32), walk_obs)
        self.walk_end = b
        self.after = self.deliver_all()

    def shape(self, spec):
        return tuple(self.dims[k] for k in spec.split())

    def deliver(self, name, kind):
        _, outs, call = ENTRIES[name]
        dsts = [Dst(kind, self.shape(s), self.T if t == 'T' else t, self.pinned) for s, t in outs]
        self.eng._ck(min(int(call(self, dsts)), 0))
        return [d.read() for d in dsts]

    def deliver_all(self):
        return {name: {kind: self.deliver(name, kind) for kind in kinds} for name, (kinds, _, _) in ENTRIES.items()}

    def assemble_store(self, dst):
        first = int(self.lib.pbvi_assemble_rows_store(self.h, GAMMA, self.dims['U'], self.keys.ctypes.data_as(C.c_void_p), dst.p()))
        self.store_firsts.append(first)
        return first

    def q_values(self, d):
        rc = self.lib.pbvi_q_values(self.h, GAMMA, d[0].p(C.c_double), d[1].p(C.c_int32), d[2].p(C.c_int32))
        self.eng.run(GAMMA)
        return rc


    def close(self):
        self.before = self.after = None
        self.eng.close()
        self.pinned.close()


@pytest.fixture(scope='module', params=[(d, B) for d in ('f32', 'f64') for B in (40, 300)], ids=lambda p: f'{p[0]}-B{p[1]}')
def sc(request):
    """One scene per engine type and block size, shared by the tests of this file (which run scene by scene) and closed
    behind the last of them."""
    scene = Scene(*request.param)
    yield scene
    scene.close()


def untouched(a):
    """How many elements of ``a`` still are the sentinel fill."""
    return int(np.all(np.ascontiguousarray(a).view(U8).reshape(-1, a.dtype.itemsize) == SENTINEL, axis=1).sum())


def same(x, y):
    return all(a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes() for a, b in zip(x, y)) and len(x) == len(y)


def test_block_of_300_is_sorted_and_block_of_40_is_not(sc):
    B = sc.dims['B']
    assert sorted(sc.perm.tolist()) == list(range(B))
    assert np.array_equal(sc.perm, np.arange(B)) == (B == 40)


@pytest.mark.parametrize('name', list(ENTRIES))
def test_destination_kinds_receive_the_same_bytes(sc, name):
    got = sc.before[name]
    for arrays in got.values():
        assert all(a.size and untouched(a) == 0 for a in arrays)      # nothing of the sentinel fill is left
    for kind in ENTRIES[name][0][1:]:
        assert same(got[kind], got['pageable']), f'{name}: {kind} differs from pageable'


@pytest.mark.parametrize('name', list(ENTRIES))
def test_delivery_after_a_belief_walk_is_the_same(sc, name):
    for kind in ENTRIES[name][0]:
        assert same(sc.after[name][kind], sc.before[name][kind]), f'{name} into {kind} memory changed behind the walk'
    # ... and the walk itself delivered its rows: the chain's last belief, recomputed on the host
    np.testing.assert_allclose(sc.walk[-1], sc.walk_end, rtol=1e-9, atol=1e-300)


def test_keys_are_the_first_belief_of_each_distinct_row(sc):
    rows, index, actions, best, keep = sc.before['fetch_compact']['pageable']
    (keys,) = sc.before['fetch_unique_keys']['pageable']
    first = np.array([np.flatnonzero(index == u)[0] for u in range(sc.dims['U'])])
    assert np.array_equal(keys, np.column_stack([actions[first], best[first, actions[first]]]))
    assert np.array_equal(keys, sc.keys)
    # the other fetches of the same result agree with fetch_compact
    alpha, f_actions, f_best, f_keep = sc.before['fetch']['pageable']
    u_rows, u_index = sc.before['fetch_unique']['pageable']
    assert same([u_rows, u_index, f_actions, f_best, f_keep], [rows, index, actions, best, keep])
    assert alpha.tobytes() == rows[index].tobytes()


@pytest.mark.parametrize('name', ['fetch_exchange', 'fetch_exchange_padded'])
def test_exchange_message_is_composed_of_the_other_fetches(sc, name):
    _, index, actions, _, keep = sc.before['fetch_compact']['pageable']
    B, U = sc.dims['B'], sc.dims['U']
    per = B if name == 'fetch_exchange' else sc.dims['P']
    sections = np.zeros((3, per), I32)
    sections[:, :B] = index, actions, keep
    keys = np.zeros((per, 1 + O), I32)
    keys[:U] = sc.keys
    want = np.concatenate([[U], sections.reshape(-1), keys.reshape(-1)]).astype(I32)
    assert np.array_equal(sc.before[name]['pageable'][0], want)


def test_assembled_rows_are_the_fetched_rows(sc):
    (rows,) = sc.before['fetch_unique']['pageable'][:1]
    for name in ('assemble_rows', 'assemble_rows_store'):
        assert sc.before[name]['pageable'][0].tobytes() == rows.tobytes(), name


def test_beliefs_come_back_in_caller_order(sc):
    assert np.array_equal(sc.before['beliefs_fetch']['pageable'][0], sc.beliefs.astype(sc.T))


def test_value_max_is_in_caller_order(sc):
    val, idx = sc.before['value_max']['pageable']
    scores = sc.beliefs @ sc.alpha.T
    assert np.array_equal(idx, np.argmax(scores, axis=1))    # (random rows: no near-ties)
    np.testing.assert_allclose(val, scores.max(axis=1), rtol=1e-6 if sc.eng.dtype == 'f32' else 1e-12)


def test_assemble_rows_store_commits_its_rows(sc):
    """The last test that uses a scene, because it selects another alpha set.  Every assemble_rows_store call appended U rows, and a set selected from
    one call's ids is the rows it returned."""
    eng, U = sc.eng, sc.dims['U']
    assert len(sc.store_firsts) == 2 * len(KINDS) and np.array_equal(np.diff(sc.store_firsts), np.full(len(sc.store_firsts) - 1, U))
    assert int(sc.lib.pbvi_alpha_store_count(sc.h)) == sc.store_firsts[-1] + U
    rows = sc.before['assemble_rows_store']['pageable'][0]
    want = eng.prune_dominated(np.asarray(rows, dtype=F64))      # the same rows uploaded
    eng.select_alpha(np.arange(sc.store_firsts[0], sc.store_firsts[0] + U))
    keep = np.empty(U, U8)
    eng._ck(sc.lib.pbvi_prune_dominated(sc.h, keep.ctypes.data_as(C.POINTER(C.c_uint8))))
    assert np.array_equal(keep.astype(bool), want)
    val, _ = eng.max_value_resident()                            # ... and they score like the uploaded rows
    ref = (sc.beliefs @ np.asarray(rows, dtype=F64).T).max(axis=1)
    np.testing.assert_allclose(val, ref, rtol=1e-6 if eng.dtype == 'f32' else 1e-12)


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_prune_dominated_equals_the_masked_prune_with_every_row_new(dtype):
    rng = np.random.default_rng(7)
    rs, rto, er = random_model(rng, S, A, O, R)
    alpha = r32(rng.normal(size=(20, S)))
    alpha[5] = alpha[2] - 0.5                                # dominated by row 2
    alpha[11] = alpha[8]                                     # a duplicate pair
    alpha[14, 3] = np.nan
    eng = Engine(S, A, O, R, rs, rto, er, dtype=dtype)
    full = eng.prune_dominated(alpha)
    masked = eng.prune_dominated_masked(alpha, np.ones(20, bool))
    assert np.array_equal(full, masked)
    assert not full[5] and full[2] and full[[0, 1, 3, 4]].all()
    eng.close()


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
def test_fetch_without_a_result_raises_and_leaves_the_destination_alone(dtype):
    sc = Scene.__new__(Scene)
    rng = np.random.default_rng(3)
    rs, rto, er = random_model(rng, S, A, O, R)
    sc.eng = Engine(S, A, O, R, rs, rto, er, dtype=dtype)
    sc.lib, sc.h, sc.T, sc.pinned = sc.eng._lib, sc.eng._h, sc.eng.np_dtype, PinnedBuffer(1 << 20)
    sc.eng.set_alpha(r32(rng.normal(size=(V, S))))
    sc.eng.set_beliefs(make_beliefs(rng, 40))
    sc.dims = dict(B=40, S=S, A=A, O=O, U=5, K=1 + O, P=47, N=sc.eng.exchange_size(40), NP=sc.eng.exchange_size(47))
    for name, text in NEED_RESULT.items():
        for kind in KINDS:
            _, outs, call = ENTRIES[name]
            dsts = [Dst(kind, sc.shape(s), sc.T if t == 'T' else t, sc.pinned) for s, t in outs]
            with pytest.raises(ValueError) as e:
                sc.eng._ck(call(sc, dsts))
            assert str(e.value) == text
            assert all(untouched(d.read()) == d.read().size for d in dsts), (name, kind)
    # the guards of the entries that have no destination kinds to vary
    lib, h, vp = sc.lib, sc.h, C.c_void_p
    idx, hashes, val = np.zeros(1, I32), Dst('pageable', (5,), np.uint64, None), Dst('pageable', (40,), F64, None)
    ptrs = [vp(), vp(), vp()]
    for exc, text, call in [
            (ValueError, 'backup_store_unique: no backup result resident',
             lambda: lib.pbvi_backup_store_unique(h, idx.ctypes.data_as(C.POINTER(C.c_int32)), 1)),
            (ValueError, 'backup_fetch_row_hashes: no backup result resident',
             lambda: lib.pbvi_backup_fetch_row_hashes(h, hashes.p(C.c_uint64))),
            (ValueError, 'no backup result resident', lambda: lib.pbvi_backup_device_results(h, *(C.byref(p) for p in ptrs))),
            (NotImplementedError, 'backup_fetch_value_max: the last backup did not run in the belief-side formulation',
             lambda: lib.pbvi_backup_fetch_value_max(h, val.p(C.c_double)))]:
        with pytest.raises(exc) as e:
            sc.eng._ck(min(int(call()), 0))
        assert str(e.value) == text
    assert untouched(hashes.read()) == 5 and untouched(val.read()) == 40 and all(p.value is None for p in ptrs)
    sc.eng.close()
