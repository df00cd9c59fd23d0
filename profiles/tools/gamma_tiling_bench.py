"""Cost and benefit of Gamma tiling (pbvi_set_gamma_tiling), one process on the GPU:

  python profiles/tools/gamma_tiling_bench.py [--only c4|capped|large] [--chunks 2,4,8] [--reps 7] [--out FILE]

  c4      olfactory-30000 R = 5, V = B = 1024 (bench.py --reach 5's shape), device-resident step (pbvi_backup_run on
          resident operands): mode off against 'always' with the given chunk counts.  Per-stage medians from pbvi_stats_t;
          in a tiled call ms_project / ms_score are sums over the chunks and ms_argmax includes the fold passes.
  capped  olfactory 30 x 80 R = 5, V = 6000, B = 256 under a cap of (held + 1600 MiB): the tiled alpha side (mode auto)
          against what the untiled engine does under the same cap (formulation auto: belief side).
  large   olfactory 165 x 375 (|S| = 61875) R = 5, V = 8192, B = 1024 under a cap of (held + 16 GiB), same comparison.

Warm-up calls first, then the median of --reps synchronised calls (each call ends synchronised).  The output is stamped
with a sha256 over csrc/*.  For the fold kernel's own time run the c4 case under `rocprofv3 --kernel-trace --stats`."""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), '..', '..'))
sys.path.insert(0, REPO)
from pomdp_pbvi_exploration_amd import synth                                  # noqa: E402
from pomdp_pbvi_exploration_amd.engine import Engine, debug_alloc_limit      # noqa: E402

STAGES = ('ms_total', 'ms_project', 'ms_score', 'ms_argmax', 'ms_refine', 'ms_action', 'ms_assemble')


def csrc_sha():
    h = hashlib.sha256()
    d = os.path.join(REPO, 'pomdp_pbvi_exploration_amd', 'csrc')
    for name in sorted(os.listdir(d)):
        h.update(name.encode())
        h.update(open(os.path.join(d, name), 'rb').read())
    return h.hexdigest()


def timed(eng, gamma, reps, warmup=3):
    for _ in range(warmup):
        eng.run(gamma, False)
    rows, wall = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        st = eng.run(gamma, False)
        wall.append((time.perf_counter() - t0) * 1e3)
        rows.append(st)
    out = {k: round(statistics.median(r[k] for r in rows), 4) for k in STAGES}
    out['wall_ms'] = round(statistics.median(wall), 4)
    out['wall_ms_min_max'] = [round(min(wall), 4), round(max(wall), 4)]
    for k in ('formulation', 'gamma_chunks', 'score_split', 'n_refined', 'n_refine_candidates'):
        out[k] = rows[-1][k]
    out['device_mib'] = eng.device_bytes >> 20
    return out


def engine_for(H, W, V, B):
    m = synth.olfactory_model(H=H, W=W, R=5)
    alpha, _ = synth.alpha_set(m, V)
    beliefs = synth.belief_points(m, B)
    eng = Engine(m.S, m.A, m.O, m.R, m.reachable_states, m.rto, m.expected_rewards, dtype='f32')
    return m, alpha, beliefs, eng


def case_c4(args):
    m, alpha, beliefs, eng = engine_for(75, 400, 1024, 1024)
    eng.set_formulation('alpha')
    eng.set_alpha(alpha)
    eng.set_beliefs(beliefs)
    res = {'shape': f'S={m.S} A={m.A} O={m.O} R={m.R} V=1024 B=1024'}
    eng.set_gamma_tiling('off')
    res['off'] = timed(eng, m.gamma, args.reps)
    for n in args.chunks:
        eng.set_gamma_tiling('always', -(-1024 // n))
        res[f'always_{n}'] = timed(eng, m.gamma, args.reps)
    eng.set_gamma_tiling('off')
    res['off_again'] = timed(eng, m.gamma, args.reps)          # alternated: drift of the box between the two 'off' rows
    eng.close()
    return res


def case_capped(args, H, W, V, B, extra_mib):
    m, alpha, beliefs, eng = engine_for(H, W, V, B)
    res = {'shape': f'S={m.S} A={m.A} O={m.O} R={m.R} V={V} B={B}', 'cap_extra_mib': extra_mib}
    prev = debug_alloc_limit((eng.device_bytes >> 20) + extra_mib)
    try:
        for label, mode, form in (('tiled_alpha_side', 'auto', 'auto'), ('untiled_under_cap', 'off', 'auto')):
            eng.set_gamma_tiling(mode)
            eng.set_formulation(form)
            eng.set_alpha(alpha)
            eng.set_beliefs(beliefs)
            try:
                res[label] = timed(eng, m.gamma, args.reps)
            except MemoryError as e:
                res[label] = {'MemoryError': str(e)[:200]}
    finally:
        debug_alloc_limit(prev)
    eng.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--only', default='c4,capped')
    ap.add_argument('--chunks', default='2,4,8')
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    args.chunks = [int(x) for x in args.chunks.split(',') if x]
    out = {'csrc_sha256': csrc_sha(), 'reps': args.reps}
    for name in args.only.split(','):
        if name == 'c4':
            out['c4_r5'] = case_c4(args)
        elif name == 'capped':
            out['capped_30x80'] = case_capped(args, 30, 80, 6000, 256, 1600)
        elif name == 'large':
            out['large_165x375'] = case_capped(args, 165, 375, 8192, 1024, 16384)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
