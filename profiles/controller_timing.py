"""Timing of the controller-evaluation entry (profiles/controller.md): one shape per process, one JSON line per shape.

    python profiles/controller_timing.py --shape olfactory_r1 --nodes blind   # 75 x 400 synthetic plume, S = 30000, A = 6, O = 3, R = 1
    python profiles/controller_timing.py --shape olfactory_r5 --nodes blind   # the same with stochastic moves, R = 5
    python profiles/controller_timing.py --shape olfactory_r1 --nodes 256     # a seeded random controller of 256 nodes
    python profiles/controller_timing.py --shape olfactory_r5 --nodes 256

Per shape, in the same process: the device's time per sweep for pbvi_controller_value_iteration and for
pbvi_fib_value_iteration (the nearest kernel: the same tables, a maximum over a' where the controller has a successor
node), controller_numpy's time per sweep on the host, and -- with --nodes blind -- one whole Blind_Solver solve on the
device and on the host (--host-solve runs the host solve to the end; without it the host figure is sweeps x ms per sweep).

A call uploads and re-tiles the tables before its first sweep, so the time per sweep is the difference of two calls with
different horizons (limit 0: no sweep stops early) divided by the difference of their sweep counts; every figure is the
median of --repeats calls after one warm-up call.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pomdp_pbvi_exploration_amd import Blind_Solver, Model, controller_numpy, pessimistic_start, set_quiet, synth   # noqa: E402
from pomdp_pbvi_exploration_amd.engine import controller_value_iteration, fib_value_iteration                     # noqa: E402
from pomdp_pbvi_exploration_amd.pomdp import _fib_tables                                                           # noqa: E402

SHORT, LONG = 64, 512                       # horizons of the two calls whose difference is the sweeps alone


def median_s(fn, repeats):
    fn()                                                          # warm-up: library loaded, kernels resident
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return statistics.median(times)


def per_sweep_us(call, repeats):
    """``(us per sweep, ms of a SHORT call, ms of a LONG call)``."""
    short, long_ = median_s(lambda: call(SHORT), repeats), median_s(lambda: call(LONG), repeats)
    return 1e6 * (long_ - short) / (LONG - SHORT), 1e3 * short, 1e3 * long_


def olfactory(R):
    """The synthetic model and the ``Model`` built from it the way ``examples/policy_eval.py`` does."""
    m = synth.olfactory_model(H=75, W=400, R=R, f32=False)
    model = Model(states=m.S, actions=m.A, observations=m.O, reachable_states=m.reachable_states,
                  observation_table=m.observation_table, end_states=[m.goal], start_probabilities=list(m.start_belief))
    if R > 1:
        model.reachable_probabilities = m.reachable_probabilities
        model.reachable_transitional_observation_table = m.rto
        model.expected_rewards_table = m.expected_rewards
    return m, model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', required=True, choices=['olfactory_r1', 'olfactory_r5'])
    ap.add_argument('--nodes', default='blind', help="'blind' (N = A, every node its own successor) or a node count")
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-sweeps', type=int, default=3)
    ap.add_argument('--eps', type=float, default=1e-3)
    ap.add_argument('--host-solve', action='store_true', help='run the host Blind_Solver solve to the end')
    args = ap.parse_args()
    set_quiet(True)
    m, model = olfactory(1 if args.shape == 'olfactory_r1' else 5)
    rs, rto, er = _fib_tables(model)
    gamma = m.gamma
    S, A, O, R = rto.shape
    if args.nodes == 'blind':
        na, ns = np.arange(A), np.tile(np.arange(A)[:, None], (1, O))
    else:
        rng = np.random.default_rng(args.seed)
        na, ns = rng.integers(0, A, int(args.nodes)), rng.integers(0, int(args.nodes), (int(args.nodes), O))
    N = len(na)
    v0 = pessimistic_start(model, gamma, N)
    q0 = np.ascontiguousarray(er.T)

    ctl_us, ctl_short, ctl_long = per_sweep_us(lambda n: controller_value_iteration(rs, rto, er, na, ns, v0, gamma, 0.0, n),
                                               args.repeats)
    again_us, _, _ = per_sweep_us(lambda n: controller_value_iteration(rs, rto, er, na, ns, v0, gamma, 0.0, n), args.repeats)
    fib_us, fib_short, fib_long = per_sweep_us(lambda n: fib_value_iteration(rs, rto, er, q0, gamma, 0.0, n), args.repeats)
    out = {}
    if args.host_sweeps > 0:                                      # (--host-sweeps 0: device figures only, for A/B runs)
        host_s = median_s(lambda: controller_numpy(model, na, ns, v0, gamma, 0.0, args.host_sweeps),
                          max(2, args.repeats // 2)) / args.host_sweeps
        host3, host3_changes = controller_numpy(model, na, ns, v0, gamma, 0.0, 3)
        dev3, dev3_changes = controller_value_iteration(rs, rto, er, na, ns, v0, gamma, 0.0, 3)
        out = {'controller_host_ms_per_sweep': round(1e3 * host_s, 2), 'host_over_device_per_sweep': round(1e6 * host_s / ctl_us, 1),
               'three_sweeps_bit_equal_to_host': bool(np.array_equal(host3, dev3) and np.array_equal(host3_changes, dev3_changes))}
    out = {
        **out, 'shape': args.shape, 'S': S, 'A': A, 'O': O, 'R': R, 'N': N, 'nodes': args.nodes, 'gamma': gamma,
        'repeats': args.repeats, 'library': os.environ.get('PBVI_LIB_PATH', 'default'),
        'controller_device_us_per_sweep': round(ctl_us, 2), 'controller_device_us_per_sweep_again': round(again_us, 2),
        'controller_device_ms_call': {str(SHORT): round(ctl_short, 3), str(LONG): round(ctl_long, 3)},
        'fib_device_us_per_sweep': round(fib_us, 2), 'fib_device_ms_call': {str(SHORT): round(fib_short, 3), str(LONG): round(fib_long, 3)},
        'controller_over_fib_time': round(ctl_us / fib_us, 2),
    }
    if args.nodes == 'blind' and args.host_sweeps > 0:
        res = {}
        solver = Blind_Solver(gamma=gamma, eps=args.eps)
        dev_s = median_s(lambda: res.__setitem__('dev', solver.solve(model, use_gpu=True, print_progress=False)), args.repeats)
        sweeps = len(res['dev'][1].value_function_changes)
        solve = {'sweeps': sweeps, 'device_s': round(dev_s, 4), 'host_s_estimated_from_per_sweep': round(host_s * sweeps, 2)}
        if args.host_solve:
            t0 = time.perf_counter()
            host_vf, host_hist = solver.solve(model, use_gpu=False, print_progress=False)
            solve['host_s'] = round(time.perf_counter() - t0, 2)
            solve['identical_rows'] = bool(np.array_equal(host_vf.alpha_vector_array, res['dev'][0].alpha_vector_array)
                                           and host_hist.value_function_changes == res['dev'][1].value_function_changes)
        rows = res['dev'][0].alpha_vector_array
        solve['rows'] = int(rows.shape[0])
        solve['blind_value_at_start_belief'] = float(np.max(rows @ np.asarray(model.start_probabilities, dtype=np.float64)))
        out['blind_solver_solve'] = solve
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
