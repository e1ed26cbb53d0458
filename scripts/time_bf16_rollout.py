#!/usr/bin/env python3
"""Plan time and rollout-launch time of the three precisions of ONE build — fp32, bf16x3 (fp32-grade split products) and bf16 (reduced
precision: csrc/cem_rollout_bf16.h) — at B1 .. B4 and the two shipped shapes.  Three handles per shape, captured graphs, early stop off;
the legs alternate inside a round (one machine, one warm clock); medians of --rounds rounds x --plans plans of host wall time around
the plan call.  Then the rollout launch by HIP events (cem_planner_set_timing) and, for bf16, the launch as a fraction of the bf16 dense
matrix peak (16 x the 157.3 TFLOP/s fp32 matrix peak the other tables use).
`bf16_beats_bf16x3`: every round median of bf16 lies below every round median of bf16x3 — faster by more than the rounds' own spread.
usage: time_bf16_rollout.py [--plans 40] [--rounds 3] [--shapes B1,B2,...] > profiles/bf16_rollout.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, synthetic  # noqa: E402

# name -> (obs, act, the PlannerConfig fields)
SHAPES = {'B1': (60, 2, dict(variant='cem', ensemble_size=5, particles=5, n_samples=500, horizon=25, n_elite=50, iterations=5)),
          'B2': (60, 2, dict(variant='cem', ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)),
          'B3': (60, 2, dict(variant='cem', ensemble_size=16, particles=16, n_samples=8192, horizon=30, n_elite=819, iterations=5)),
          'B4': (100, 12, dict(variant='cem', ensemble_size=8, particles=8, n_samples=4096, horizon=50, n_elite=409, iterations=5)),
          'cem_mpc': (60, 2, dict(variant='cem', ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10)),
          'safe_cem_mpc': (60, 2, dict(variant='safe', ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9))}
LEGS = ('fp32', 'bf16x3', 'bf16')
BF16_PEAK = 16 * 157.3e12


def planner(shape, precision):
    obs, act, sh = SHAPES[shape]
    pb = synthetic.problem(obs, act, sh['ensemble_size'])
    cfg = PlannerConfig(obs_dim=obs, act_dim=act, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=True, precision=precision, **sh)
    pl = CemPlanner(cfg)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl, np.asarray(pb['state'], np.float32).copy()


def main():
    plans = int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 40
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 3
    shapes = sys.argv[sys.argv.index('--shapes') + 1].split(',') if '--shapes' in sys.argv else list(SHAPES)
    out = {}
    for shape in shapes:
        obs, act, sh = SHAPES[shape]
        handles = {leg: planner(shape, leg) for leg in LEGS}
        call = 0
        for leg in LEGS:                                      # clocks and the captured graph
            for _ in range(15):
                handles[leg][0].plan(handles[leg][1], seed=1, call=call); call += 1
        ms = {leg: [] for leg in LEGS}
        for r in range(rounds):
            for leg in LEGS:
                pl, st = handles[leg]
                row = []
                for _ in range(plans):
                    t0 = time.perf_counter()
                    pl.plan(st, seed=1, call=call); call += 1
                    row.append(1e3 * (time.perf_counter() - t0))
                ms[leg].append(row)
        res = {}
        for leg in LEGS:
            pl, st = handles[leg]
            pl.set_timing(True)
            rms, rn = 0.0, 0
            for i in range(3):
                pl.plan(st, seed=2, call=i); tm = pl.last_timing(); rms += tm['rollout_ms']; rn += tm['rollout_launches']
            pl.set_timing(False)
            rc, tiles = pl.tiles()
            round_medians = [float(np.median(r)) for r in ms[leg]]
            res[leg] = dict(plan_ms_median=float(np.median([x for r in ms[leg] for x in r])), round_medians=round_medians,
                            plans_per_s=1e3 / float(np.median([x for r in ms[leg] for x in r])), rollout_launch_ms=rms / rn,
                            chunks_per_tile=rc, workgroups=len(tiles), graph=pl.graph_status(), rollout_path=pl.rollout_path())
            pl.close()
        flops = synthetic.flops_per_row_step(obs, act) * sh['particles'] * sh['n_samples'] * sh['horizon']
        res['bf16']['frac_of_bf16_dense_peak'] = flops / (res['bf16']['rollout_launch_ms'] * 1e-3) / BF16_PEAK
        res['bf16_over_bf16x3_plan'] = res['bf16']['plan_ms_median'] / res['bf16x3']['plan_ms_median']
        res['bf16_over_fp32_plan'] = res['bf16']['plan_ms_median'] / res['fp32']['plan_ms_median']
        res['bf16_over_bf16x3_launch'] = res['bf16']['rollout_launch_ms'] / res['bf16x3']['rollout_launch_ms']
        res['bf16_beats_bf16x3'] = bool(max(res['bf16']['round_medians']) < min(res['bf16x3']['round_medians']))
        out[shape] = res
        sys.stderr.write('%s: %s\n' % (shape, ' | '.join('%s %.3f ms (launch %.4f)' % (l, res[l]['plan_ms_median'], res[l]['rollout_launch_ms']) for l in LEGS)))
    print(json.dumps(dict(plans=plans, rounds=rounds, shapes=out), indent=1))


if __name__ == '__main__':
    main()
