"""Child process of test_score_slabs_golden.py, case k: case a's backup in a process of its own (``PBVI_GEMM_NO_STREAMK``
is read once per process), one ``score-slabs-json <digests and counters>`` line.  Test infrastructure."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

from test_score_slabs_golden import CASES, CHILD_TAG, case_r1            # noqa: E402

if __name__ == '__main__':
    from pomdp_pbvi_exploration_amd import set_quiet
    set_quiet(True)
    _, shape, settings = CASES['a']
    print(CHILD_TAG + json.dumps(case_r1(shape, **settings)), flush=True)
