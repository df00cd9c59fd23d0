"""Hand-built inputs for the two byte masks of a backup (test_backup_masks.py, test_score_window.py).  No tests here.

``keep_case``  an identity-style model on which the belief-dominance margin ``b.alpha'[b] - max_v b.alpha_v`` is exactly
               ``+-2^-(23+j)`` or 0 and every product and partial sum of the backup fits in 53 bits: float64 arithmetic on
               these inputs is exact in any order, so the keep mask has one right answer.
``dead_ref``   the dead-triple map from its definition, on the inputs as the engine holds them.
``DeadCase``   beliefs and RTO supports placed tile by tile, so that each case walks a named branch of ``k_dead``
               (backup_kernels.hip); ``DEAD_CASES`` lists them.
"""
import functools

import numpy as np

TILE = 32                              # states per K tile (GEMM_BK)
WORD = 64                              # tiles per bit word of k_dead

# --------------------------------------------------------------------------- #
# 1. keep at fp64 resolution
# --------------------------------------------------------------------------- #
KEEP_GAMMA = 0.5
LADDER = tuple(range(1, 11))           # b[s0] = 2^-j
D = 2.0 ** -23                         # |d_b|


class KeepCase:
    """R = 1, rs[s, a, 0] = s, O = 1, rto = 1, A = 2, gamma = 1/2, S = 32 B.  Belief i lives on the 32 states of block
    ``block_of[i]`` (a seeded permutation: the caller's order is not the sorted one), entries multiples of 2^-10 that sum to
    1, ``b[s0] = 2^-j``.  Alpha entries are multiples of 2^-8: [1, 1.25] everywhere, but row ``w(i)`` holds [1.75, 2) on
    belief i's block, so it wins there by >= 1/2 per unit of mass.  ``er[:, 0] = alpha_w / 2 + d e_s0`` on that block,
    d = sgn 2^-23, and ``er[:, 1] = er[:, 0] - 1``: action 0 wins by 1, alpha'[i] = alpha_w + d e_s0 on the block and

        nv - old = b.(alpha_w + d e_s0) - b.alpha_w = sgn 2^-(23 + j).

    One alpha entry per belief leaves the 2^-8 grid: ``alpha_w[s0]`` carries ``low 2^-22`` (low = +-1, seeded) as well, so
    that old = b.alpha_w has a bit at 2^-(22 + j) and, from j = 2 on, is NOT an fp32 number -- a K5 that rounded its
    maxima to fp32 on the way, however exactly it had computed them, moves old by at least the margin.  Every entry of
    every alpha' row stays a multiple of 2^-23 in [1, 2): an fp32 number.

    Products are multiples of 2^-33 below 2, sums stay below 4: 36 bits.  ``scale`` (a power of two) multiplies the alpha
    set and er; nothing else changes."""

    def __init__(self, B, V, scale=1.0, seed=0):
        rng = np.random.default_rng([seed, B, V])
        S, A = TILE * B, 2
        self.S, self.A, self.O, self.R, self.B, self.V, self.scale, self.gamma = S, A, 1, 1, B, V, scale, KEEP_GAMMA
        self.rs = np.arange(S, dtype=np.int64)[:, None, None].repeat(A, axis=1)
        self.rto = np.ones((S, A, 1, 1))
        self.block_of = rng.permutation(B)
        combos = [(j, sgn) for j in LADDER for sgn in (1, -1, 0)]
        assert B >= len(combos)
        extra = [combos[i] for i in rng.integers(0, len(combos), B - len(combos))]
        picks = [(combos + extra)[i] for i in rng.permutation(B)]
        self.j = np.array([p[0] for p in picks])
        self.sgn = np.array([p[1] for p in picks])
        self.winner = rng.integers(0, V, B)
        self.low = rng.choice([-1, 1], B)
        alpha = 1.0 + rng.integers(0, 65, (V, S)) / 256.0
        b = np.zeros((B, S))
        er0 = np.zeros(S)
        self.s0 = np.zeros(B, dtype=np.int64)
        for i in range(B):
            lo = TILE * int(self.block_of[i])
            alpha[self.winner[i], lo:lo + TILE] = 1.75 + rng.integers(0, 64, TILE) / 256.0
            s0 = lo + int(rng.integers(0, TILE))
            self.s0[i] = s0
            alpha[self.winner[i], s0] += self.low[i] * 2.0 * D
            units = 1024 - 2 ** (10 - int(self.j[i]))                     # what is left of 1024 units of 2^-10
            rest = rng.multinomial(units, np.full(TILE - 1, 1.0 / (TILE - 1)))
            others = np.array([s for s in range(lo, lo + TILE) if s != s0])
            b[i, others] = rest / 1024.0
            b[i, s0] = 2.0 ** -int(self.j[i])
            er0[lo:lo + TILE] = 0.5 * alpha[self.winner[i], lo:lo + TILE]
            er0[s0] += self.sgn[i] * D
        self.alpha = alpha * scale
        self.b = b
        self.er = np.stack([er0, er0 - 1.0], axis=1) * scale
        self.margin = self.sgn * 2.0 ** -(23.0 + self.j) * scale         # nv - old, exactly
        self.mask = self.margin > 0
        # what the backup must return
        self.rows = np.zeros((B, S))
        for i in range(B):
            self.rows[i] = 0.5 * self.alpha[self.winner[i]] + self.er[:, 0]
        self.best = self.winner.reshape(B, 1, 1).repeat(A, axis=1)
        self.actions = np.zeros(B, dtype=np.int64)

    def sort_perm(self):
        """perm[engine row] = caller row of a block sorted (stably) by the first non-zero K tile, as k_rank_sort leaves it."""
        return np.argsort(self.block_of, kind='stable')


@functools.lru_cache(maxsize=None)
def keep_case(B, V, scale=1.0):
    return KeepCase(B, V, scale)


def keep_chunk_rows(V):
    """Gamma chunk (a multiple of 4) that cuts V alpha rows into three chunks, the last one shorter."""
    cr = {48: 20, 80: 32}[V]
    assert 2 * cr < V < 3 * cr
    return cr


# --------------------------------------------------------------------------- #
# 2. the dead-triple map
# --------------------------------------------------------------------------- #
def dead_ref(b, rto):
    """[B][A * O] bool: supp(b) and supp(RTO[:, a, o, :]) share no state."""
    S, A, O, R = rto.shape
    sup = (rto != 0).any(axis=3).reshape(S, A * O)                        # S, G
    return ~((b != 0).astype(np.int64) @ sup.astype(np.int64) > 0)


def first_tile_perm(b):
    """perm[engine row] = caller row after the engine's stable sort by first non-zero K tile (an empty row sorts last)."""
    B, S = b.shape
    k_tiles = -(-S // TILE)
    nz = b != 0
    key = np.where(nz.any(axis=1), np.argmax(nz, axis=1) // TILE, k_tiles)
    return np.argsort(key, kind='stable')


def tile_structure(b, rto):
    """What k_dead sees of (belief i, group g): ``n_cand`` [B][G] candidate tiles (belief mass AND support in the tile),
    ``first`` [B][G] the position among the candidates, in ascending tile order, of the first one that holds a common
    state (-1: none -- the triple is dead), ``first_tile`` [B][G] that tile (-1: none)."""
    S, A, O, R = rto.shape
    k_tiles = -(-S // TILE)
    pad = k_tiles * TILE - S
    sup = np.pad((rto != 0).any(axis=3).reshape(S, A * O), ((0, pad), (0, 0))).T.reshape(A * O, k_tiles, TILE)
    nzb = np.pad(b != 0, ((0, 0), (0, pad))).reshape(b.shape[0], k_tiles, TILE)
    cand = nzb.any(axis=2)[:, None, :] & sup.any(axis=2)[None, :, :]                      # B, G, k_tiles
    hit = np.einsum('bts,gts->bgt', nzb.astype(np.int64), sup.astype(np.int64)) > 0      # B, G, k_tiles
    n_cand = cand.sum(axis=2)
    first_tile = np.where(hit.any(axis=2), np.argmax(hit, axis=2), -1)
    rank = np.cumsum(cand, axis=2) - 1                                                  # position of tile t among the candidates
    first = np.where(first_tile >= 0, np.take_along_axis(rank, np.maximum(first_tile, 0)[:, :, None], axis=2)[:, :, 0], -1)
    return n_cand, first, first_tile


EVEN = np.arange(0, TILE, 2)
ODD = np.arange(1, TILE, 2)


class DeadCase:
    """R successors per (s, a) with rs[s, a, 0] = s (slots r > 0: probability 0, successor ``pad_to``), A actions, O
    observations; ``sup[g]`` = states where RTO[s, a, o, 0] = 1/2, ``bel[i]`` = states of belief i, each with weight
    2^-10 k (seeded k).  gamma = 1/2.  Alpha row 0 is the constant 1, rows 1 .. V-1 are multiples of 1/4 in [2, 3]: on a
    live triple every other row beats row 0 by a factor of two, so a triple that is wrongly flagged dead (best_v = 0) also
    shows in ``best_alpha_ind``.  Every value is a small multiple of a power of two: the scores are exact in fp32 and
    fp64, ties are exact ties, and the engine's first-maximum rule is np.argmax's."""

    def __init__(self, name, S, A, O, bel, sup, V=5, R=1, pad_to=0, branch='', claims=()):
        rng = np.random.default_rng(sum((i + 1) * ord(c) for i, c in enumerate(name)))
        self.name, self.branch = name, branch
        self.S, self.A, self.O, self.R, self.V, self.B, self.gamma = S, A, O, R, V, len(bel), 0.5
        self.rs = np.full((S, A, R), pad_to, dtype=np.int64)
        self.rs[:, :, 0] = np.arange(S)[:, None]
        self.rto = np.zeros((S, A, O, R))
        for g, states in sup.items():
            states = np.asarray(states, dtype=np.int64)
            self.rto[states[states < S], g // O, g % O, 0] = 0.5          # (a partly filled last tile: what lies behind S is dropped)
        self.b = np.zeros((len(bel), S))
        for i, states in enumerate(bel):
            states = np.asarray(states, dtype=np.int64)
            states = states[states < S]
            self.b[i, states] = rng.integers(1, 9, states.size) / 1024.0
        self.alpha = np.concatenate([np.ones((1, S)), 2.0 + rng.integers(0, 5, (V - 1, S)) / 4.0])
        self.er = rng.integers(-8, 9, (S, A)) / 8.0
        self.dead = dead_ref(self.b, self.rto)
        self.claims = list(claims)           # (belief, group, candidate tiles, position of the first overlapping one or -1, its tile or -1)

    @property
    def k_tiles(self):
        return -(-self.S // TILE)


def tiles(ts, which):
    """States ``which`` (offsets inside a tile) of every tile in ``ts``."""
    ts = np.atleast_1d(np.asarray(ts, dtype=np.int64))
    return (ts[:, None] * TILE + np.asarray(which)[None, :]).ravel()


def _five(shared, far_tile):
    """The five beliefs of a fresh block over the candidate tiles ``shared``:
    0  even states of the shared tiles                     (against an odd support: candidates, no common state)
    1  nothing at all                                      (every triple dead)
    2  odd states of the shared tiles                      (live from the first candidate on)
    3  one tile that no support touches                    (no candidate)
    4  like 0                                              (the block holds two rows of the pattern under test)"""
    return [tiles(shared, EVEN), np.zeros(0, dtype=np.int64), tiles(shared, ODD), tiles(far_tile, EVEN), tiles(shared, EVEN)]


def _groups(shared, hit_tile):
    """A = 1, O = 4.  g0: odd states of the shared tiles (belief 0: candidates but disjoint).  g1: the same plus ONE even
    state in ``hit_tile`` (belief 0: the only overlap is there).  g2: no support (dead for every belief).  g3: g0's
    support again (the last group of the block's four waves)."""
    odd = tiles(shared, ODD)
    g1 = np.concatenate([odd, [hit_tile * TILE + 6]])
    return {0: odd, 1: g1, 2: np.zeros(0, dtype=np.int64), 3: odd}


def _shared_case(name, k_tiles, shared, hit_pos, branch, S=None):
    """Candidates ``shared`` (ascending tiles); the only common state of (belief 0, g1) is in candidate ``hit_pos``."""
    S = S or k_tiles * TILE
    shared = list(shared)
    far = next(t for t in range(k_tiles - 1, -1, -1) if t not in shared) if len(shared) < k_tiles else shared[0]
    n = len(shared)
    claims = [(0, 0, n, -1, -1), (0, 1, n, hit_pos, shared[hit_pos]), (2, 0, n, 0, shared[0]), (1, 0, 0, -1, -1), (0, 2, 0, -1, -1)]
    return DeadCase(name, S, 1, 4, _five(shared, far), _groups(shared, shared[hit_pos]), branch=branch,
                    claims=claims)


def _build_dead_cases():
    c = {}
    # candidate but disjoint: 1, 2, 3 and 64 + 1 shared tiles, the overlap (g1) in the last candidate
    for n in (1, 2, 3, 65):
        kt = max(4, n + 3)
        shared = list(range(1, n + 1))
        c[f'disjoint_{n}'] = _shared_case(f'disjoint_{n}', kt, shared, n - 1,
                                          f'{n} candidate tile(s) with interleaved even / odd states: dead at element level only; '
                                          f'g1 overlaps in the last candidate')
    # overlap in t1: second tile of the first pair; the odd last candidate (t1 = -1); the last candidate of a word
    c['t1_second_of_pair'] = _shared_case('t1_second_of_pair', 12, [2, 5, 7, 9], 1, 'the only overlap is in t1 of the first pair')
    c['t1_second_pair'] = _shared_case('t1_second_pair', 12, [2, 5, 7, 9], 3, 'the only overlap is in t1 of the second pair')
    c['odd_last_candidate'] = _shared_case('odd_last_candidate', 12, [2, 5, 7], 2, 'three candidates: the overlap is in the odd last one (t1 = -1)')
    c['last_of_word'] = _shared_case('last_of_word', 70, [3, 10, 40, 63, 66], 3,
                                     'four candidates in word 0, the overlap in the last of them (bit 63, as t1); word 1 has one more')
    # bit positions of the overlap tile inside a word: alone in word 0; in word 1 behind a candidate of word 0
    for bit in (0, 31, 32, 63):
        c[f'bit_{bit}'] = _shared_case(f'bit_{bit}', 64, [bit], 0, f'the only candidate, with the overlap, at bit {bit} of word 0')
        shared1 = [5, WORD + bit]
        c[f'word1_bit_{bit}'] = _shared_case(f'word1_bit_{bit}', 129, shared1, 1, f'overlap tile at bit {bit} of word 1')
    # word positions for k_tiles in {1, 63, 64, 65, 129}: the overlap in word 0, word 1, the last word
    for kt in (1, 63, 64, 65, 129):
        last_word = (kt - 1) // WORD
        for w in sorted({0, min(1, last_word), last_word}):
            t = min(kt - 1, w * WORD + (WORD - 1 if w < last_word else (kt - 1) % WORD))
            shared = sorted({0, t}) if kt > 1 else [0]
            c[f'kt{kt}_word{w}'] = _shared_case(f'kt{kt}_word{w}', kt, shared, len(shared) - 1,
                                                f'k_tiles = {kt}: the overlap in tile {t} (word {w})', S=kt * TILE - (5 if kt > 1 else 9))
    # the last state: the only overlap at S - 1 for S % 32 in {1, 31, 0}; a zero-probability pad slot (R = 2) whose
    # successor lies in the belief's support must not count
    for rem in (1, 31, 0):
        S = 4 * TILE + rem if rem else 5 * TILE
        kt = -(-S // TILE)
        lastt = kt - 1
        bel = [np.array([2, S - 1]), np.zeros(0, dtype=np.int64), np.array([3, TILE + 3]), np.array([S - 1]), np.array([2, 40])]
        sup = {0: np.array([3, S - 1]), 1: np.array([3, TILE + 1]), 2: np.zeros(0, dtype=np.int64), 3: np.array([S - 1])}
        c[f'last_state_rem{rem}'] = DeadCase(f'last_state_rem{rem}', S, 1, 4, bel, sup, R=2, pad_to=2,
                                             branch=f'S % 32 = {rem}: beliefs 0 and 3 meet g0 and g3 at state S - 1 (tile {lastt}) only',
                                             claims=[(0, 0, 2, 1, lastt), (3, 3, 1, 0, lastt), (0, 1, 1, -1, -1), (4, 0, 1, -1, -1)])
    return c


DEAD_CASES = _build_dead_cases()


@functools.lru_cache(maxsize=None)
def sorted_dead_case(B=300):
    """B = 300 (more than one row block: the engine sorts, k_dead reads the row flags through perm).  Every belief takes
    one of the five roles of ``_five`` on its own pair of tiles, in seeded order, so the caller's order is not the sorted
    one and the pattern of dead triples changes under the sort."""
    rng = np.random.default_rng(300)
    kt = 70
    S = kt * TILE - 3
    shared = list(range(0, kt - 2, 2))                       # supports on every second tile; the odd ones are empty
    odd = tiles(shared, ODD)
    sup = {0: odd, 1: np.concatenate([odd, tiles(shared, [6])]), 2: np.zeros(0, dtype=np.int64), 3: tiles(shared[::3], EVEN)}
    bel = []
    for i in range(B):
        role, t = int(rng.integers(0, 5)), int(rng.choice(shared))
        bel.append([tiles([t], EVEN), np.zeros(0, dtype=np.int64), tiles([t], ODD), tiles([t + 1], EVEN),
                    np.concatenate([tiles([t], [0, 2, 4]), tiles([t + 1], ODD)])][role])
    return DeadCase('sorted_block', S, 1, 4, bel, sup, branch='B = 300: row flags through perm')


@functools.lru_cache(maxsize=None)
def big_dead_case():
    """S = 131072 + 64 + 5: k_tiles = 4099, 65 bit words -- the second iteration of k_dead's 64-word loop.  A = 1, O = 2,
    B = 4, V = 4.  Beliefs 0 and 1 share tiles of words 0, 17 and 63 with the supports without sharing a state; the only
    common states lie in tiles 4097 (g0) and 4098 (g1: state S - 1), both in word 64."""
    S = 131072 + 64 + 5
    lo = [3, 17 * WORD + 9, 63 * WORD + 63]
    sup = {0: np.concatenate([tiles(lo, ODD), tiles([4097], [6])]), 1: np.concatenate([tiles(lo, ODD), [S - 1]])}
    bel = [np.concatenate([tiles(lo, EVEN), tiles([4097], EVEN)]),            # live on g0 through tile 4097, dead on g1
           np.concatenate([tiles(lo, EVEN), [S - 1]]),                       # dead on g0, live on g1 through state S - 1
           tiles(lo, EVEN),                                                  # candidates in the first 64 words only: dead, dead
           np.concatenate([tiles([4096], EVEN), tiles(lo[:1], ODD)])]        # live on both in word 0
    return DeadCase('second_w0_iteration', S, 1, 2, bel, sup, V=4, branch='k_tiles = 4099: the overlap in a tile of word 64',
                    claims=[(0, 0, 4, 3, 4097), (1, 1, 4, 3, 4098), (0, 1, 3, -1, -1), (1, 0, 3, -1, -1), (2, 0, 3, -1, -1), (3, 0, 1, 0, 3)])


class TinyCase:
    """A screened fp64 engine with values that fp32 cannot hold.  S = 96, A = 1, O = 3, R = 1, identity successors.
    g0 has support on tile 0, g1 on tile 1, g2 on tile 2.
      belief 0: ordinary mass on tile 0 and 2^-160 at one state of tile 1      -> (0, g1) is live in fp64, its fp32 copy is 0
      belief 1: ordinary mass on tiles 0 and 2; RTO[s, 0, g2, 0] = 2^-160 there -> (1, g2) is live through a tiny RTO entry
      belief 2: ordinary mass on tile 0 only                                  -> g1, g2 dead
    Alpha row 0 is the constant 1; the other rows are multiples of 1/4 in [2, 3] and row V - 1 is 4 on tiles 1 and 2."""

    def __init__(self):
        rng = np.random.default_rng(160)
        S, A, O, V = 96, 1, 3, 6
        tiny = 2.0 ** -160
        self.S, self.A, self.O, self.R, self.V, self.B, self.gamma = S, A, O, 1, V, 3, 0.5
        self.rs = np.arange(S, dtype=np.int64)[:, None, None]
        self.rto = np.zeros((S, A, O, 1))
        self.rto[0:32, 0, 0, 0] = 0.5
        self.rto[32:64, 0, 1, 0] = 0.5
        self.rto[64:96, 0, 2, 0] = tiny
        self.b = np.zeros((3, S))
        self.b[:, 0:32] = rng.integers(1, 9, (3, 32)) / 1024.0
        self.b[0, 40] = tiny
        self.b[1, 64:96] = rng.integers(1, 9, 32) / 1024.0
        self.alpha = np.concatenate([np.ones((1, S)), 2.0 + rng.integers(0, 5, (V - 1, S)) / 4.0])
        self.alpha[V - 1, 32:] = 4.0
        self.er = rng.integers(-8, 9, (S, A)) / 8.0
        self.dead = dead_ref(self.b, self.rto)
        self.tiny_triples = [(0, 1), (1, 2)]                 # (belief, group)
