"""Timing of the state policies -- most likely state, voting, Thompson -- (profiles/state_policy.md).

    python profiles/state_policy_timing.py --part call      # pbvi_state_policy per rule on one block, with the read floor
    python profiles/state_policy_timing.py --part rollout   # pbvi_rollout_state_policy against pbvi_rollout_infotaxis, per step
    python profiles/state_policy_timing.py --part seam      # the same policies computed on the host from the device's block

Every part prints one JSON line per measurement.  75 x 400 synthetic plume (S = 30000, A = 6, O = 3), R = 1 and 5.  The
kernel's own time comes from a kernel trace of ``--part call`` (k_state_policy<T, RULE>), taken in a run of its own.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pomdp_pbvi_exploration_amd import Model, set_quiet, synth                # noqa: E402
from pomdp_pbvi_exploration_amd.engine import Engine                          # noqa: E402
from pomdp_pbvi_exploration_amd.mdp import VI_Solver                          # noqa: E402
from pomdp_pbvi_exploration_amd.pomdp import (Infotaxis_Agent, StatePolicy_Agent, state_actions_from,   # noqa: E402
                                              state_policy_numpy)

H, W = 75, 400
HBM_ACHIEVABLE = 6.3e12                       # bytes / s, the achievable rate of the MI355X's HBM3E (8.0e12 is the specification)
RULES = ('mls', 'voting', 'thompson')


def median_ms(fn, repeats):
    fn()                                                          # warm-up: buffers sized, kernels loaded
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times), min(times), max(times)


def build_model(R):
    m = synth.olfactory_model(H=H, W=W, R=R, f32=False)
    model = Model(states=m.S, actions=m.A, observations=m.O, reachable_states=m.reachable_states,
                  observation_table=m.observation_table, end_states=[m.goal], start_probabilities=list(m.start_belief))
    if R > 1:
        model.reachable_probabilities = m.reachable_probabilities
        model.reachable_transitional_observation_table = m.rto
        model.expected_rewards_table = m.expected_rewards
    return m, model


def mdp_policy(m, model):
    vf, _ = VI_Solver(gamma=m.gamma, eps=1e-6).solve(model, use_gpu=True, print_progress=False)
    return state_actions_from(vf)


def part_call(args):
    for R in (1, 5):
        m, model = build_model(R)
        sa = mdp_policy(m, model)
        b = synth.belief_points(m, args.B, max_depth=64, f32=False)
        for dtype in ('f32', 'f64'):
            eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype=dtype, device=0)
            eng.set_beliefs(b)
            eng.set_state_policy(sa)
            floor_bytes = args.B * m.S * (4 if dtype == 'f32' else 8)           # one read of the block
            rows = {rule: median_ms(lambda k=k: eng.state_policy_resident(k, seed=7), args.repeats) for k, rule in enumerate(RULES)}
            rows['infotaxis'] = median_ms(lambda: eng.infotaxis_resident(), args.repeats)
            eng.close()
            print(json.dumps({'part': 'call', 'R': R, 'dtype': dtype, 'B': args.B, 'S': m.S, 'A': m.A, 'repeats': args.repeats,
                              'floor_bytes': floor_bytes, 'floor_us_at_achievable_hbm': round(1e6 * floor_bytes / HBM_ACHIEVABLE, 2),
                              'call_ms_median_min_max': {k: [round(x, 4) for x in v] for k, v in rows.items()}}), flush=True)


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
            'mean_steps': float(steps.mean()), 'success_rate': float(found.mean())}


def part_rollout(args):
    for R in (1, 5):
        m, model = build_model(R)
        sa = mdp_policy(m, model)
        for dtype in ('f32', 'f64'):
            gm = model.to_gpu(dtype)
            agents = [('infotaxis', Infotaxis_Agent(gm))] + [(rule, StatePolicy_Agent(gm, sa, rule)) for rule in RULES]
            for name, agent in agents:
                out = evaluate(agent, args.n, args.max_steps, 7, args.repeats)
                print(json.dumps({'part': 'rollout', 'R': R, 'dtype': dtype, 'policy': name, 'n': args.n, 'T': args.max_steps, **out}),
                      flush=True)


class HostSeamAgent(StatePolicy_Agent):
    """The policy written on the host against the device's block: the beliefs cross the boundary every step."""

    def _block_actions(self, block):
        b = block.eng.fetch_beliefs()
        u = np.random.random(b.shape[0]) if self.rule == 2 else None
        return state_policy_numpy(b, self.state_actions, self.rule, u, action_count=self.model.action_count)[0]


def part_seam(args):
    for R in (1, 5):
        m, model = build_model(R)
        sa = mdp_policy(m, model)
        for dtype in ('f32', 'f64'):
            gm = model.to_gpu(dtype)
            for rule in RULES:
                agent = HostSeamAgent(gm, sa, rule)
                walls = []
                for _ in range(2):
                    np.random.seed(1)
                    t0 = time.perf_counter()
                    _, hists = agent.run_n_simulations_parallel(n=args.n, max_steps=args.seam_steps, print_progress=False, print_stats=False)
                    walls.append(time.perf_counter() - t0)
                lock = max(len(h.actions) for h in hists)
                print(json.dumps({'part': 'seam', 'R': R, 'dtype': dtype, 'policy': rule, 'n': args.n, 'lock_steps': lock,
                                  'ms_per_lock_step_second_run': round(1e3 * walls[1] / lock, 2)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--part', required=True, choices=['call', 'rollout', 'seam'])
    ap.add_argument('--B', type=int, default=1000)
    ap.add_argument('--n', type=int, default=1000)
    ap.add_argument('--max-steps', type=int, default=300)
    ap.add_argument('--seam-steps', type=int, default=5)
    ap.add_argument('--repeats', type=int, default=9)
    args = ap.parse_args()
    set_quiet(True)
    {'call': part_call, 'rollout': part_rollout, 'seam': part_seam}[args.part](args)


if __name__ == '__main__':
    main()
