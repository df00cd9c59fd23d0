"""Child process of test_value_max.py::test_small_alpha_sets_on_the_wide_route_in_a_child: the exact family at V <= 64 and
the near-tie family at V = 40 on an fp32 sparse engine in a process of its own (``PBVI_NO_SKINNY`` is read once per
process), one ``value-max-sha256 <label> <route> <digest>`` line per case.  Test infrastructure: uses oracle/."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]

from test_value_max import run_child_cases                               # noqa: E402

if __name__ == '__main__':
    from pomdp_pbvi_exploration_amd import set_quiet
    set_quiet(True)
    for line in run_child_cases():
        print(line, flush=True)
