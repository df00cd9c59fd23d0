"""Child process of test_decision_paths.py::test_once_per_process_switches_in_a_child: family E at k = 3 and 33 and
family N on the projected fp32 route in a process of its own (``PBVI_REFINE_INBLOCK`` and ``PBVI_NO_L1_SCREEN`` are read
once per process), one ``decision-sha256 <label> <digest> <counts>`` line per case.  Test infrastructure: uses oracle/."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

from test_decision_paths import run_child_cases                          # noqa: E402

if __name__ == '__main__':
    from pomdp_pbvi_exploration_amd import set_quiet
    set_quiet(True)
    for line in run_child_cases():
        print(line, flush=True)
