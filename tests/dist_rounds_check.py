"""Child ranks of the GPU tests of tests/test_dist_rounds.py: two processes (``RANK`` / ``WORLD_SIZE`` in the
environment), one HIP engine each on GPU 0, gloo carrying the exchange -- everything else is the product path
(``PBVI_Solver.backup`` taking the sharded route by itself).  ``argv[1]``:

* ``cap``: rank 1 backs up under a cap of its engine's device bytes under which its block of the first round fails and
  half of it fits; both ranks must end with the single-process result.
* ``chunk7``: the chunk forced to 7 on both ranks, no cap; the result must be the one-round sharded one.
"""
import datetime
import os
import sys

import numpy as np
import torch                                    # noqa: F401  torch first: its HIP runtime has to be the one that opens the device
import torch.distributed as dist

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..'))
sys.path.insert(0, REPO)

MIB = 1 << 20


def main():
    mode = sys.argv[1]
    dist.init_process_group('gloo', timeout=datetime.timedelta(seconds=60))
    rank, world = dist.get_rank(), dist.get_world_size()
    from pomdp_pbvi_exploration_amd import Belief, BeliefSet, Model, PBVI_Solver, ValueFunction, set_quiet, synth
    from pomdp_pbvi_exploration_amd import dist as pdist
    from pomdp_pbvi_exploration_amd.engine import debug_alloc_limit
    set_quiet(True)
    pdist.enable(True)
    assert pdist.active() and world == 2

    m = synth.olfactory_model(H=15, W=40, R=1, f32=True)                # S = 600
    alpha, acts = synth.alpha_set(m, 37)
    om = Model(states=m.S, actions=m.A, observations=m.O, reachable_states=m.reachable_states,
               observation_table=m.observation_table, end_states=[m.goal], start_probabilities=list(m.start_belief))
    gm = om.to_gpu('f64')
    eng = gm.engine
    solver = PBVI_Solver(gamma=m.gamma)

    at_gather = []                                                       # the engine's device bytes when a round is sent
    gather_round = pdist.gather_round

    def probe(*args, **kwargs):
        at_gather.append(eng.device_bytes)
        return gather_round(*args, **kwargs)

    pdist.gather_round = probe

    def backup(rows, sharded, chunk=None):
        """One backup of ``rows`` against the 37 alpha-vectors on an engine in its fresh state (both ranks alike)."""
        if sharded:
            os.environ.pop('PBVI_NO_SHARD', None)
        else:
            os.environ['PBVI_NO_SHARD'] = '1'
        eng.after_oom()
        solver._belief_chunk = chunk
        del at_gather[:]
        try:
            bs = BeliefSet(gm, [Belief(gm, r) for r in rows])
            return solver.backup(gm, bs, ValueFunction(gm, alpha, acts), append=False, belief_dominance_prune=False)
        finally:
            os.environ.pop('PBVI_NO_SHARD', None)

    def same(a, b):
        return (len(a) == len(b) and np.array_equal(a.actions, b.actions) and
                np.array_equal(np.asarray(a.alpha_vector_array), np.asarray(b.alpha_vector_array)))    # bit for bit

    if mode == 'chunk7':
        rows = synth.belief_points(m, 40, max_depth=16)
        one = backup(rows, sharded=True)
        assert len(at_gather) == 1 and solver._belief_chunk is None
        seven = backup(rows, sharded=True, chunk=7)
        assert len(at_gather) == 3 and solver._belief_chunk == 7         # 20 per rank: 7 + 7 + 6
        assert len(one) > 1 and same(seven, one), (len(one), len(seven))
        assert same(backup(rows, sharded=False), one)
    else:
        # The cap: strictly between what this engine holds after an uncapped backup in half blocks (per / 2 beliefs per
        # round, everything included) and what it holds when the whole block (per beliefs) is ready to be sent, both
        # measured here on the same inputs, in MiB (the unit of pbvi_debug_alloc_limit): the whole MiB nearest to their
        # midpoint.  Not the lowest one: the engine's recovery keeps a few small work lists at the size of the block that
        # failed, so the retry holds somewhat more than the fresh engine measured here.  B = 40 is what the test is
        # about; if no whole MiB lies strictly between the two there, B is doubled until one does.  Rank 1 decides for both.
        for B in (40, 80, 160, 320, 640):
            rows = synth.belief_points(m, B, max_depth=16)
            per = B // 2
            backup(rows, sharded=True)
            whole = at_gather[-1]
            backup(rows, sharded=True, chunk=per // 2)
            halves = eng.device_bytes
            lowest, highest = halves // MIB + 1, (whole - 1) // MIB
            cap = min(max((halves + whole + MIB) // (2 * MIB), lowest), highest)
            print(f'rank {rank}: B = {B}: footprint {whole} bytes with a {per}-belief block, {halves} bytes in '
                  f'{per // 2}-belief rounds; cap {cap} MiB', flush=True)
            verdict = torch.tensor([int(lowest <= highest and halves < cap * MIB < whole), cap], dtype=torch.int64)
            dist.broadcast(verdict, src=1)
            if int(verdict[0]):
                break
        else:
            raise AssertionError('no B at which a whole block and half blocks differ by a MiB')
        cap = int(verdict[1])
        want = backup(rows, sharded=False)                               # the single-process backup on this GPU
        assert len(want) > 1
        prev = debug_alloc_limit(cap) if rank == 1 else None
        try:
            got = backup(rows, sharded=True)
        finally:
            if rank == 1:
                debug_alloc_limit(prev)
        print(f'rank {rank}: {len(at_gather)} rounds, chunk {solver._belief_chunk}, device bytes at the gathers {at_gather}',
              flush=True)
        assert solver._belief_chunk is not None and solver._belief_chunk < per, solver._belief_chunk
        assert same(got, want), (len(got), len(want))
    dist.barrier()
    dist.destroy_process_group()
    print('sharded rounds ok', flush=True)


if __name__ == '__main__':
    main()
