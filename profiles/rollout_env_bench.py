"""Timings behind profiles/rollout_env.md: policy evaluation against recorded frames on the S = 30000 olfactory model.

    python profiles/rollout_env_bench.py --reach 5 --dtype f32 [--expansions 40 --n 1000 --max-steps 300 --repeat 4]

After one MDP value iteration and one FSVI solve (examples/policy_eval.py's, same seeds) it times, in this process, the
whole ``Agent.run_n_simulations_parallel`` call -- host bookkeeping included -- ``--repeat`` times each (the first is the
warm-up and is dropped, the median of the rest is reported with all of them in brackets):

  env     device_rng_seed=7, environment=frames   (pbvi_rollout_env; the warm-up call uploads the frames, the timed calls find them resident)
  model   device_rng_seed=7                       (pbvi_rollout, the model's own observations)
  seam    the host seam: a SimulationSet subclass whose run_actions reads the same frames, belief block resident,
          successors from NumPy's stream (what an evaluation against recorded data had to use before)

One JSON line per variant on stdout.
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
from pomdp_pbvi_exploration_amd import FSVI_Solver, Model, set_quiet, synth              # noqa: E402
from pomdp_pbvi_exploration_amd.mdp import VI_Solver                                      # noqa: E402
from pomdp_pbvi_exploration_amd.pomdp import Agent, FrameEnvironment, SimulationSet, record_frames   # noqa: E402


class FrameSimulationSet(SimulationSet):
    """``SimulationSet`` with the observation of step ``t`` read from ``env.frames[shift + t, channel[a], s']``."""

    reference_indexing = False

    def __init__(self, model, env, n):
        super().__init__(model)
        self.env, self.t = env, 0
        self.shift = np.broadcast_to(env.shifts, (n,))

    def initialize_simulations(self, n=1, start_state=None):
        self.t = 0
        return super().initialize_simulations(n, start_state)

    def run_actions(self, actions):
        m = self.model
        actions = np.asarray(actions)
        potentials = m.reachable_states[self.agent_states, actions]
        if m.reachable_state_count == 1:
            next_states = potentials[:, 0]
        else:
            probs = m.reachable_probabilities[self.agent_states, actions]
            chosen = np.apply_along_axis(lambda x: np.random.choice(len(x), size=1, p=x), axis=1, arr=probs)
            next_states = potentials[np.arange(self.n), chosen[:, 0]]
        observations = self.env.frames[self.shift[self.simulations] + self.t, self.env.channel_of_action[actions], next_states].astype(int)
        self.t += 1
        step_rewards = self._step_rewards(self.agent_states, actions, next_states, observations)
        rewards = np.where(~self.is_done, step_rewards, 0)
        self.is_done |= np.isin(next_states, np.array(m.end_states))
        self.agent_states = next_states
        return rewards, observations


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--expansions', type=int, default=40)
    ap.add_argument('--growth', type=int, default=100)
    ap.add_argument('--n', type=int, default=1000)
    ap.add_argument('--max-steps', type=int, default=300)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'f64'])
    ap.add_argument('--grid', default='75x400')
    ap.add_argument('--reach', type=int, default=1, choices=[1, 5])
    ap.add_argument('--repeat', type=int, default=4)
    ap.add_argument('--variants', default='env,model,seam')
    args = ap.parse_args()
    set_quiet(True)
    H, W = (int(x) for x in args.grid.split('x'))
    m = synth.olfactory_model(H=H, W=W, R=args.reach, f32=False)
    model = Model(states=m.S, actions=m.A, observations=m.O, reachable_states=m.reachable_states,
                  observation_table=m.observation_table, end_states=[m.goal], start_probabilities=list(m.start_belief))
    if args.reach > 1:
        model.reachable_probabilities = m.reachable_probabilities
        model.reachable_transitional_observation_table = m.rto
        model.expected_rewards_table = m.expected_rewards
    mdp_dev, _ = VI_Solver(gamma=m.gamma, eps=1e-6).solve(model, use_gpu=True, print_progress=False)
    np.random.seed(0)
    random.seed(0)
    vf, hist = FSVI_Solver(gamma=m.gamma, eps=1e-6, mdp_policy=mdp_dev).solve(model, expansions=args.expansions,
                                                                              max_belief_growth=args.growth, use_gpu=True,
                                                                              engine_dtype=args.dtype, print_progress=False)
    agent = Agent(vf.model, vf, gamma=m.gamma)
    t0 = time.perf_counter()
    frames = record_frames(m.observation_table, args.max_steps + 100, 7)
    env = FrameEnvironment(frames, np.arange(m.A), shifts=np.arange(args.n) % 101)
    t_rec = time.perf_counter() - t0
    base = dict(S=m.S, R=args.reach, dtype=args.dtype, V=len(vf), n=args.n, max_steps=args.max_steps,
                frames=list(frames.shape), frame_bytes=int(frames.nbytes), record_frames_s=round(t_rec, 3))
    for variant in args.variants.split(','):
        walls, steps, lost = [], 0, 0
        for _ in range(args.repeat):
            np.random.seed(1)
            kw = dict(n=args.n, max_steps=args.max_steps, print_progress=False, print_stats=False)
            if variant == 'env':
                kw.update(device_rng_seed=7, environment=env)
            elif variant == 'model':
                kw.update(device_rng_seed=7)
            else:
                kw.update(simulator_set=FrameSimulationSet(vf.model, env, args.n))
            t0 = time.perf_counter()
            _, hists = agent.run_n_simulations_parallel(**kw)
            walls.append(time.perf_counter() - t0)
            steps = sum(len(h.actions) for h in hists)
            lock_steps = max(len(h.actions) for h in hists)
            lost = sum(bool(h.lost) for h in hists)
        timed = walls[1:] if len(walls) > 1 else walls
        med = statistics.median(timed)
        print(json.dumps(dict(base, variant=variant, wall_median_s=round(med, 4), walls_s=[round(w, 4) for w in timed],
                              warmup_s=round(walls[0], 4), lock_steps=lock_steps, ms_per_lock_step=round(1e3 * med / lock_steps, 4),
                              belief_steps=steps, lost=lost)), flush=True)


if __name__ == '__main__':
    main()
