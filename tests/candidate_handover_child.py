"""Child process of test_candidate_handover.py: one group of its cases in a process of its own, started with
``PBVI_NO_CAND_HANDOVER=1`` (read once per process), one ``handover-sha256 <label> ...`` line per case.  Test
infrastructure."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

from test_candidate_handover import GROUPS, edge_lines, run_case          # noqa: E402

if __name__ == '__main__':
    from pomdp_pbvi_exploration_amd import set_quiet
    set_quiet(True)
    group = sys.argv[1]
    lines = edge_lines() if group == 'edge' else [run_case(label)[0] for label in GROUPS[group]]
    for line in lines:
        print(line, flush=True)
