"""Policy evaluation on the HIP engine: solve the synthetic olfactory model with FSVI, then run
`Agent.run_n_simulations_parallel` with the belief block resident on the GPU.

The reference publishes one timing for this step (sim_runtime_test.ipynb:223): 1000 simulations x
300 steps in 41.8 s on its CuPy path (S=22021, unnamed GPU).  This script runs the same call shape.

    python examples/policy_eval.py --expansions 60 --n 1000 --max-steps 300
    python examples/policy_eval.py --reach 5 --device-sim 7      # stochastic moves, simulator on the device too
    python examples/policy_eval.py --policy infotaxis --device-sim 7   # the infotaxis baseline (no solve), on the device
    python examples/policy_eval.py --policy space-aware --device-sim 7   # space-aware infotaxis (pbvi_rollout_space_aware)
    python examples/policy_eval.py --policy expected-distance --device-sim 7   # greedy for the expected distance to the source
    python examples/policy_eval.py --policy fib --reach 5 --device-sim 7   # follow the Fast Informed Bound's rows (no FSVI solve)
    python examples/policy_eval.py --policy qmdp --reach 5 --device-sim 7  # ... or the MDP solution's (QMDP)
    python examples/policy_eval.py --policy blind --device-sim 7   # follow the blind-policy lower bound's rows (no solve)
    python examples/policy_eval.py --policy thompson --device-sim 7   # MDP heuristics: mls, voting, thompson (pbvi_state_policy)
    python examples/policy_eval.py --device-sim 1 --environment frames    # observations from recorded frames (pbvi_rollout_env)
    python examples/policy_eval.py --device-sim 1 --environment table --env-flip 0.1   # a sensor that errs 10 % more often
"""
import argparse
import os
import random
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from pomdp_pbvi_exploration_amd import Blind_Solver, FIB_Solver, FSVI_Solver, Model, set_quiet, synth   # noqa: E402
from pomdp_pbvi_exploration_amd.pomdp import (Agent, FrameEnvironment, Infotaxis_Agent, SpaceAware_Agent,   # noqa: E402
                                              StatePolicy_Agent, TableEnvironment, record_frames, state_actions_from)
from pomdp_pbvi_exploration_amd.mdp import VI_Solver                         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--expansions', type=int, default=60)
    ap.add_argument('--growth', type=int, default=100)
    ap.add_argument('--n', type=int, default=1000)
    ap.add_argument('--max-steps', type=int, default=300)
    ap.add_argument('--dtype', default='f32', choices=['f32', 'f64'])
    ap.add_argument('--grid', default='75x400')
    ap.add_argument('--lookahead', type=int, default=0, choices=[0, 1],
                    help='0: actions[argmax_v b.alpha_v] (the reference policy); 1: one-step lookahead argmax_a Q(b,a)')
    ap.add_argument('--cpu-steps', type=int, default=0, help='also time this many steps of the host NumPy path')
    ap.add_argument('--reach', type=int, default=1, choices=[1, 5],
                    help='reachable states per (state, action): 1 = deterministic moves, 5 = the intended move with 0.8')
    ap.add_argument('--device-sim', type=int, default=None, metavar='SEED',
                    help='counter-based simulator draws with this seed: the whole step loop runs in the engine '
                         '(pbvi_rollout) instead of drawing on the host from NumPy\'s stream')
    ap.add_argument('--policy', default='value', choices=['value', 'infotaxis', 'space-aware', 'expected-distance', 'qmdp', 'fib',
                                                         'blind', 'mls', 'voting', 'thompson'],
                    help='value: solve with FSVI and follow the value function; qmdp / fib: no FSVI solve, follow the A rows of '
                         'MDP value iteration / of the Fast Informed Bound (pbvi_fib_value_iteration); blind: no solve, follow the A rows of '
                         'the blind-policy lower bound, "always take action a" (pbvi_controller_value_iteration); infotaxis: no solve, every step takes the '
                         'action with the smallest expected entropy of the next belief (pbvi_infotaxis); space-aware: no '
                         'solve, greedy for log2(D + 2^(H-1) - 1/2) of the next belief, D its expected Manhattan distance to '
                         'the source and H its entropy in bits (pbvi_space_aware); expected-distance: greedy for D alone; mls / '
                         'voting / thompson: solve the MDP as qmdp does and act through its policy pi(s) -- in the most likely '
                         'state, by the votes of all states weighted with the belief, or in a state drawn from the belief '
                         '(pbvi_state_policy)')
    ap.add_argument('--environment', default=None, choices=['frames', 'table'],
                    help='where the observations come from (needs --device-sim): frames = a recorded movie, max-steps + 100 '
                         'frames drawn from the observation table by record_frames, every simulation starting at its own '
                         'frame; table = the observation table itself as a second law')
    ap.add_argument('--env-flip', type=float, default=0.0, metavar='P',
                    help='perturb the environment\'s table: each row becomes (1 - P) * row + P * (row reversed over the '
                         'observations), a sensor that reports the opposite reading with probability P')
    ap.add_argument('--repeat', type=int, default=1, help='run the evaluation this many times (the first one warms up)')
    args = ap.parse_args()
    set_quiet(True)
    H, W = (int(x) for x in args.grid.split('x'))
    m = synth.olfactory_model(H=H, W=W, R=args.reach, f32=False)
    model = Model(states=m.S, actions=m.A, observations=m.O, reachable_states=m.reachable_states,
                  observation_table=m.observation_table, end_states=[m.goal], start_probabilities=list(m.start_belief))
    if args.reach > 1:                                 # the tables of the stochastic-move model, as the tests' mirror builds them
        model.reachable_probabilities = m.reachable_probabilities
        model.reachable_transitional_observation_table = m.rto
        model.expected_rewards_table = m.expected_rewards
    if args.policy == 'infotaxis':
        agent = Infotaxis_Agent(model.to_gpu(args.dtype))
        policy = 'infotaxis'
    elif args.policy in ('space-aware', 'expected-distance'):
        cell = np.arange(m.S)                                  # state = row * W + column; the distance ignores wrap-around
        distance = (np.abs(cell // W - m.goal // W) + np.abs(cell % W - m.goal % W)).astype(np.float64)
        agent = SpaceAware_Agent(model.to_gpu(args.dtype), weights=distance,
                                 objective='space_aware' if args.policy == 'space-aware' else 'expected_weight')
        policy = args.policy
    elif args.policy in ('mls', 'voting', 'thompson'):
        t0 = time.perf_counter()
        vf, h = VI_Solver(gamma=m.gamma, eps=1e-6).solve(model, use_gpu=True, print_progress=False)
        policy = f'{args.policy} over the MDP policy ({len(h.iteration_times)} sweeps)'
        print(f'{policy}: solved in {time.perf_counter() - t0:.3f}s', flush=True)
        agent = StatePolicy_Agent(model.to_gpu(args.dtype), state_actions_from(vf), rule=args.policy)
    elif args.policy == 'blind':
        t0 = time.perf_counter()
        vf, h = Blind_Solver(gamma=m.gamma, eps=1e-6).solve(model, use_gpu=True, print_progress=False)
        policy = f'blind ({len(h.iteration_times)} sweeps)'
        print(f'{policy}: {len(vf)} rows in {time.perf_counter() - t0:.3f}s', flush=True)
        model.to_gpu(args.dtype)
        vf = vf.to_gpu()
        agent = Agent(vf.model, vf, lookahead=args.lookahead, gamma=m.gamma)
    elif args.policy in ('qmdp', 'fib'):
        t0 = time.perf_counter()
        vf, h = VI_Solver(gamma=m.gamma, eps=1e-6).solve(model, use_gpu=True, print_progress=False)
        policy = f'qmdp ({len(h.iteration_times)} sweeps)'
        if args.policy == 'fib':
            vf, h = FIB_Solver(gamma=m.gamma, eps=1e-6).solve(model, mdp_solution=vf, use_gpu=True, print_progress=False)
            policy += f' + fib ({len(h.iteration_times)} sweeps)'
        print(f'{policy}: {len(vf)} rows in {time.perf_counter() - t0:.3f}s', flush=True)
        model.to_gpu(args.dtype)
        vf = vf.to_gpu()
        agent = Agent(vf.model, vf, lookahead=args.lookahead, gamma=m.gamma)
    else:
        # MDP value iteration that seeds FSVI: device sweeps vs the host NumPy loop (same result, see tests)
        t0 = time.perf_counter()
        mdp_dev, h_dev = VI_Solver(gamma=m.gamma, eps=1e-6).solve(model, use_gpu=True, print_progress=False)
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        mdp_host, h_host = VI_Solver(gamma=m.gamma, eps=1e-6).solve(model, use_gpu=False, print_progress=False)
        t_host = time.perf_counter() - t0
        print(f'value iteration: {len(h_dev.iteration_times)} sweeps  device {t_dev:.3f}s  host NumPy {t_host:.3f}s  '
              f'identical rows: {np.array_equal(mdp_dev.alpha_vector_array, mdp_host.alpha_vector_array)}', flush=True)

        # the Fast Informed Bound from that solution: the device entry against its NumPy restatement (the same rows for
        # R = 1, where FIB is the MDP solution again after a sweep or two; a tighter bound with --reach 5)
        t0 = time.perf_counter()
        fib_dev, f_dev = FIB_Solver(gamma=m.gamma, eps=1e-6).solve(model, mdp_solution=mdp_dev, use_gpu=True, print_progress=False)
        t_dev = time.perf_counter() - t0
        t0 = time.perf_counter()
        fib_host, _ = FIB_Solver(gamma=m.gamma, eps=1e-6).solve(model, mdp_solution=mdp_dev, use_gpu=False, print_progress=False)
        t_host = time.perf_counter() - t0
        print(f'fast informed bound: {len(f_dev.iteration_times)} sweeps  device {t_dev:.3f}s  host NumPy {t_host:.3f}s  '
              f'identical rows: {np.array_equal(fib_dev.alpha_vector_array, fib_host.alpha_vector_array)}', flush=True)

        np.random.seed(0)
        random.seed(0)
        t0 = time.perf_counter()
        vf, hist = FSVI_Solver(gamma=m.gamma, eps=1e-6, mdp_policy=mdp_dev).solve(model, expansions=args.expansions, max_belief_growth=args.growth,
                                                              use_gpu=True, engine_dtype=args.dtype, print_progress=False)
        print(f'solve: S={m.S} expansions={len(hist.expansion_times)} |V|={len(vf)} in {time.perf_counter() - t0:.2f}s', flush=True)

        agent = Agent(vf.model, vf, lookahead=args.lookahead, gamma=m.gamma)
        policy = f'|V|={len(vf)}'
    sim = 'host simulator' if args.device_sim is None else f'device simulator, seed {args.device_sim}'
    env = None
    if args.environment is not None:
        if args.device_sim is None:
            ap.error('--environment needs --device-sim SEED')
        table = (1.0 - args.env_flip) * m.observation_table + args.env_flip * m.observation_table[:, :, ::-1]
        if args.environment == 'frames':
            frames = record_frames(table, args.max_steps + 100, args.device_sim)
            env = FrameEnvironment(frames, np.arange(m.A), shifts=np.arange(args.n) % 101)
            sim += f', {frames.shape[0]} recorded frames ({frames.nbytes / 2 ** 20:.1f} MiB)'
        else:
            env = TableEnvironment(table)
            sim += ', observation table environment'
        if args.env_flip:
            sim += f', flipped with P = {args.env_flip}'
    for rep in range(args.repeat):
        np.random.seed(1)
        t0 = time.perf_counter()
        totals, hists = agent.run_n_simulations_parallel(n=args.n, max_steps=args.max_steps, print_progress=False,
                                                         print_stats=rep == args.repeat - 1, device_rng_seed=args.device_sim,
                                                         **({} if env is None else {'environment': env}))
        wall = time.perf_counter() - t0
        steps = sum(len(h.actions) for h in hists)
        lock_steps = max(len(h.actions) for h in hists)
        print(f'gpu ({args.dtype}, R={args.reach}, {sim}): n={args.n} max_steps={args.max_steps} {policy} wall={wall:.3f}s '
              f'lock-steps={lock_steps} ({1e3 * wall / lock_steps:.3f} ms/step) belief-steps={steps} '
              f'({steps / wall:.0f} belief-steps/s)  reference CuPy: 41.8 s for 1000 x 300', flush=True)
        if env is not None:
            print(f'lost (met an observation the model gives probability 0): {sum(h.lost for h in hists)} of {args.n}', flush=True)

    if args.cpu_steps > 0:
        if args.policy == 'infotaxis':
            host_agent = Infotaxis_Agent(model)
        elif args.policy in ('space-aware', 'expected-distance'):
            host_agent = SpaceAware_Agent(model, weights=agent.weights, objective=agent.objective)
        elif args.policy in ('mls', 'voting', 'thompson'):
            host_agent = StatePolicy_Agent(model, agent.state_actions, rule=agent.rule)
        else:
            host_agent = Agent(model, vf.to_cpu(), lookahead=args.lookahead, gamma=m.gamma)   # (value, qmdp, fib, blind)
        np.random.seed(1)
        t0 = time.perf_counter()
        _, hh = host_agent.run_n_simulations_parallel(n=args.n, max_steps=args.cpu_steps, print_progress=False,
                                                      print_stats=False)
        wall_c = time.perf_counter() - t0
        steps_c = sum(len(h.actions) for h in hh)
        same = all(h.actions[:args.cpu_steps] == g.actions[:args.cpu_steps] for h, g in zip(hh, hists))
        print(f'host NumPy: {args.cpu_steps} steps wall={wall_c:.2f}s ({steps_c / wall_c:.0f} belief-steps/s); '
              f'same actions as the GPU run over those steps: {same}', flush=True)


if __name__ == '__main__':
    main()
