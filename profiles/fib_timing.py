"""Timing of the Fast Informed Bound entry (profiles/fib.md): one shape per process, one JSON line per shape.

    python profiles/fib_timing.py --shape olfactory_r1     # 75 x 400 synthetic plume, S = 30000, A = 6, O = 3, R = 1
    python profiles/fib_timing.py --shape olfactory_r5     # the same with stochastic moves, R = 5
    python profiles/fib_timing.py --shape sea_robin        # S = 61875, A = 16, O = 2, R = 1

Per shape, in the same process: the device's time per sweep for pbvi_fib_value_iteration and for
pbvi_mdp_value_iteration (the nearest kernel: the same loop without the observation), fib_numpy's time per sweep on the
host, and whole device solves from the rewards and from the MDP solution (the start FIB_Solver uses).

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
from pomdp_pbvi_exploration_amd import fib_numpy, set_quiet, synth                         # noqa: E402
from pomdp_pbvi_exploration_amd.engine import fib_value_iteration, mdp_value_iteration     # noqa: E402
from pomdp_pbvi_exploration_amd.pomdp import _fib_tables                                   # noqa: E402

SHORT, LONG = 64, 512                       # horizons of the two calls whose difference is the sweeps alone


def tables(shape):
    if shape == 'sea_robin':
        S, A, O, rs, rto, er, _, _ = synth.sea_robin_like(V=1, B=1)
        return rs, rto, er, 0.99
    m = synth.olfactory_model(H=75, W=400, R=1 if shape == 'olfactory_r1' else 5, f32=False)
    return (*_fib_tables(m), m.gamma)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', required=True, choices=['olfactory_r1', 'olfactory_r5', 'sea_robin'])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--host-sweeps', type=int, default=3)
    ap.add_argument('--eps', type=float, default=1e-3)
    args = ap.parse_args()
    set_quiet(True)
    rs, rto, er, gamma = tables(args.shape)
    S, A, O, R = rto.shape
    prob = rto.sum(axis=2)
    limit = args.eps * gamma / (1 - gamma)
    from types import SimpleNamespace
    t = SimpleNamespace(reachable_states=rs, reachable_transitional_observation_table=rto, expected_rewards_table=er)
    q_rewards = np.ascontiguousarray(er.T)

    fib_us, fib_short, fib_long = per_sweep_us(lambda n: fib_value_iteration(rs, rto, er, q_rewards, gamma, 0.0, n), args.repeats)
    vi_us, vi_short, vi_long = per_sweep_us(lambda n: mdp_value_iteration(rs, prob, er, q_rewards.max(axis=0), gamma, 0.0, n),
                                            args.repeats)
    host_s = median_s(lambda: fib_numpy(t, q_rewards, gamma, 0.0, args.host_sweeps), max(2, args.repeats // 2)) / args.host_sweeps

    # whole solves on the device: from the rewards, and from the (device) MDP solution as FIB_Solver starts
    out = {}
    solve_cold = median_s(lambda: out.__setitem__('cold', fib_value_iteration(rs, rto, er, q_rewards, gamma, limit, 10000)), args.repeats)
    mdp_rows, mdp_changes = mdp_value_iteration(rs, prob, er, q_rewards.max(axis=0), gamma, limit, 10000)
    q_mdp = np.tile(mdp_rows.max(axis=0), (A, 1))
    solve_warm = median_s(lambda: out.__setitem__('warm', fib_value_iteration(rs, rto, er, q_mdp, gamma, limit, 10000)), args.repeats)
    rows_cold, rows_warm = out['cold'][0], out['warm'][0]
    host3, host3_changes = fib_numpy(t, q_rewards, gamma, 0.0, 3)
    dev3, dev3_changes = fib_value_iteration(rs, rto, er, q_rewards, gamma, 0.0, 3)

    print(json.dumps({
        'shape': args.shape, 'S': S, 'A': A, 'O': O, 'R': R, 'gamma': gamma, 'limit': limit, 'repeats': args.repeats,
        'fib_device_us_per_sweep': round(fib_us, 2), 'fib_device_ms_call': {str(SHORT): round(fib_short, 3), str(LONG): round(fib_long, 3)},
        'vi_device_us_per_sweep': round(vi_us, 2), 'vi_device_ms_call': {str(SHORT): round(vi_short, 3), str(LONG): round(vi_long, 3)},
        'fib_over_vi_time': round(fib_us / vi_us, 2), 'fib_over_vi_multiply_adds': O * A,
        'fib_host_ms_per_sweep': round(1e3 * host_s, 2), 'host_over_device_per_sweep': round(1e6 * host_s / fib_us, 1),
        'solve_from_rewards': {'sweeps': len(out['cold'][1]), 'device_s': round(solve_cold, 4),
                               'host_s_estimated_from_per_sweep': round(host_s * len(out['cold'][1]), 2)},
        'solve_from_mdp': {'mdp_sweeps': len(mdp_changes), 'sweeps': len(out['warm'][1]), 'device_s': round(solve_warm, 4)},
        # how much tighter than the MDP rows (0 at R = 1 up to rounding), and how far the two starts end from each other
        'mdp_rows_minus_fib_rows_max_min': [float(np.max(mdp_rows - rows_warm)), float(np.min(mdp_rows - rows_warm))],
        'mdp_value_minus_fib_value_max': float(np.max(mdp_rows.max(axis=0) - rows_warm.max(axis=0))),
        'from_rewards_minus_from_mdp_max_abs': float(np.max(np.abs(rows_cold - rows_warm))),
        'three_sweeps_bit_equal_to_host': bool(np.array_equal(host3, dev3) and np.array_equal(host3_changes, dev3_changes)),
    }), flush=True)


if __name__ == '__main__':
    main()
