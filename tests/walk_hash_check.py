"""Child process of test_bayes_step.py::test_fused_chain_gives_the_doubles_of_the_two_kernel_chain: the same 41-step walks
in a process of its own (``PBVI_WALK_TWO_KERNELS`` is read once per process), one ``walk-sha256 <kind> <digest>`` line per
engine kind.  Test infrastructure: uses oracle/."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

from test_bayes_step import ENGINE_KINDS, hash_walk_digests             # noqa: E402

if __name__ == '__main__':
    from pomdp_pbvi_exploration_amd import set_quiet
    set_quiet(True)
    for kind, digest in zip(ENGINE_KINDS, hash_walk_digests()):
        print('walk-sha256', digest, kind, flush=True)
