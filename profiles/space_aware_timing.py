"""Timing and a first quality table for space-aware infotaxis (profiles/space_aware.md).

    python profiles/space_aware_timing.py --part call      # pbvi_space_aware against pbvi_infotaxis on the same block
    python profiles/space_aware_timing.py --part rollout   # pbvi_rollout_space_aware against pbvi_rollout_infotaxis, per step
    python profiles/space_aware_timing.py --part quality   # mean steps / success of FSVI, infotaxis, space-aware, expected-distance

Every part prints one JSON line per measurement.  75 x 400 synthetic plume (S = 30000, A = 6, O = 3), R = 1 and 5.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pomdp_pbvi_exploration_amd import FSVI_Solver, Model, set_quiet, synth   # noqa: E402
from pomdp_pbvi_exploration_amd.engine import Engine                          # noqa: E402
from pomdp_pbvi_exploration_amd.mdp import VI_Solver                          # noqa: E402
from pomdp_pbvi_exploration_amd.pomdp import Agent, Infotaxis_Agent, SpaceAware_Agent   # noqa: E402

H, W = 75, 400


def distance(m):
    cell = np.arange(m.S)
    return (np.abs(cell // W - m.goal // W) + np.abs(cell % W - m.goal % W)).astype(np.float64)


def median_ms(fn, repeats):
    fn()                                                          # warm-up: buffers sized, kernels loaded
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), min(times), max(times)


def part_call(args):
    for R in (1, 5):
        m = synth.olfactory_model(H=H, W=W, R=R, f32=False)
        b = synth.belief_points(m, args.B, max_depth=64, f32=False)
        w = distance(m)
        for dtype in ('f32', 'f64'):
            eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype=dtype, device=0)
            eng.set_beliefs(b)
            eng.set_state_weights(w)
            rows = {'infotaxis': median_ms(lambda: eng.infotaxis_resident(), args.repeats),
                    'space_aware': median_ms(lambda: eng.space_aware_resident(0), args.repeats),
                    'expected_weight': median_ms(lambda: eng.space_aware_resident(1), args.repeats),
                    'infotaxis_again': median_ms(lambda: eng.infotaxis_resident(), args.repeats)}
            eng.close()
            print(json.dumps({'part': 'call', 'R': R, 'dtype': dtype, 'B': args.B, 'repeats': args.repeats,
                              'ms_median_min_max': {k: [round(x, 4) for x in v] for k, v in rows.items()}}), flush=True)


def build_model(R):
    m = synth.olfactory_model(H=H, W=W, R=R, f32=False)
    model = Model(states=m.S, actions=m.A, observations=m.O, reachable_states=m.reachable_states,
                  observation_table=m.observation_table, end_states=[m.goal], start_probabilities=list(m.start_belief))
    if R > 1:
        model.reachable_probabilities = m.reachable_probabilities
        model.reachable_transitional_observation_table = m.rto
        model.expected_rewards_table = m.expected_rewards
    return m, model


def evaluate(agent, n, T, seed, repeats):
    walls = []
    for _ in range(repeats):
        np.random.seed(1)
        t0 = time.perf_counter()
        _, hists = agent.run_n_simulations_parallel(n=n, max_steps=T, print_progress=False, print_stats=False, device_rng_seed=seed)
        walls.append(time.perf_counter() - t0)
    steps = np.array([len(h.actions) for h in hists])
    goal = agent.model.cpu_model.end_states[0]
    found = np.array([h.states[-1] == goal for h in hists])
    return {'wall_s': [round(x, 4) for x in walls], 'lock_steps': int(steps.max()),
            'ms_per_lock_step_median_of_all_but_first': round(1e3 * statistics.median(walls[1:] or walls) / int(steps.max()), 4),
            'mean_steps': float(steps.mean()), 'mean_steps_of_the_found': float(steps[found].mean()) if found.any() else None,
            'success_rate': float(found.mean())}


def part_rollout(args):
    for R in (1, 5):
        m, model = build_model(R)
        for dtype in ('f32', 'f64'):
            gm = model.to_gpu(dtype)
            for name, agent in (('infotaxis', Infotaxis_Agent(gm)),
                                ('space_aware', SpaceAware_Agent(gm, distance(m), 'space_aware')),
                                ('expected_weight', SpaceAware_Agent(gm, distance(m), 'expected_weight'))):
                out = evaluate(agent, args.n, args.max_steps, 7, args.repeats)
                print(json.dumps({'part': 'rollout', 'R': R, 'dtype': dtype, 'policy': name, 'n': args.n, 'T': args.max_steps, **out}),
                      flush=True)


def part_quality(args):
    for R in (1, 5):
        m, model = build_model(R)
        mdp, _ = VI_Solver(gamma=m.gamma, eps=1e-6).solve(model, use_gpu=True, print_progress=False)
        np.random.seed(0)
        random.seed(0)
        vf, hist = FSVI_Solver(gamma=m.gamma, eps=1e-6, mdp_policy=mdp).solve(model, expansions=args.expansions, max_belief_growth=100,
                                                                              use_gpu=True, engine_dtype='f32', print_progress=False)
        gm = vf.model
        agents = (('fsvi', Agent(gm, vf, lookahead=0, gamma=m.gamma)), ('infotaxis', Infotaxis_Agent(gm)),
                  ('space_aware', SpaceAware_Agent(gm, distance(m), 'space_aware')),
                  ('expected_distance', SpaceAware_Agent(gm, distance(m), 'expected_weight')))
        for name, agent in agents:
            out = evaluate(agent, args.n, args.max_steps, 7, 1)
            print(json.dumps({'part': 'quality', 'R': R, 'policy': name, 'alpha_vectors': len(vf), 'n': args.n, 'T': args.max_steps,
                              **out}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', required=True, choices=['call', 'rollout', 'quality'])
    ap.add_argument('--B', type=int, default=1000)
    ap.add_argument('--n', type=int, default=1000)
    ap.add_argument('--max-steps', type=int, default=300)
    ap.add_argument('--repeats', type=int, default=9)
    ap.add_argument('--expansions', type=int, default=40)
    args = ap.parse_args()
    set_quiet(True)
    {'call': part_call, 'rollout': part_rollout, 'quality': part_quality}[args.part](args)


if __name__ == '__main__':
    main()
