#!/usr/bin/env python3
"""Per-plan wall time of a plan with time-correlated action noise (cem_planner_set_action_noise, CEM_NOISE_MIXED; PlannerConfig.action_noise)
beside the WHITE plan of the same build on the same handle shape (captured graph, early stop off): the shipped cem_mpc and safe_cem_mpc
shapes and B2.  A mixed plan launches cem_mix_action_noise_kernel once, reads its samples from the mixed tensor and runs the generic
rollout kernels; a white plan runs the lean ones where the handle is eligible.  Each shape is therefore measured twice:
  white / mixed                    handles created as usual: the white leg takes the lean path where it is eligible (`rollout_path` says)
  white_generic / mixed_generic    handles created under CEM_FORCE_ROLLOUT=generic: both legs on the generic kernels
so that the price of losing the lean path (white_generic - white) and the price of the mix and the tensor read (mixed_generic -
white_generic) are told apart.  Medians of --rounds rounds x --plans plans, the legs alternating inside a round; host wall time around
the plan call (result poll included).
With --kernel-stats the mix kernel's mean device time comes from a `rocprofv3 --kernel-trace --stats` run of its own (a fresh child
process running --child: 20 mixed plans of every shape), not from the timed legs.
With --scores the file also records, for information only, the mean best score of --score-plans plans from different states of the
synthetic model at equal sample budget with white, beta = 1 and beta = 2 noise at B2's shape.  The synthetic model is not an environment:
nothing is claimed from these numbers.
usage: time_colored_noise.py [--plans 40] [--rounds 3] [--kernel-stats] [--scores] > profiles/colored_noise.json"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, synthetic  # noqa: E402

SHAPES = {'cem_mpc': dict(variant='cem', ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10),
          'safe_cem_mpc': dict(variant='safe', ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9),
          'B2': dict(variant='cem', ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)}
# leg -> (action_noise, force the generic rollout at create)
LEGS = {'white': ('white', False), 'mixed': ('powerlaw', False), 'white_generic': ('white', True), 'mixed_generic': ('powerlaw', True)}
BETA = 2.0
KERNEL = 'cem_mix_action_noise_kernel'


def planner(shape, noise, generic, beta=BETA):
    sh = dict(SHAPES[shape])
    pb = synthetic.problem(60, 2, sh['ensemble_size'])
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=True, action_noise=noise,
                        action_noise_param=beta if noise != 'white' else 0.0, **sh)
    before = os.environ.get('CEM_FORCE_ROLLOUT')
    if generic:
        os.environ['CEM_FORCE_ROLLOUT'] = 'generic'               # read once, when the handle is created
    try:
        pl = CemPlanner(cfg)
    finally:
        if generic:
            if before is None:
                del os.environ['CEM_FORCE_ROLLOUT']
            else:
                os.environ['CEM_FORCE_ROLLOUT'] = before
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl, np.asarray(pb['state'], np.float32).copy()


def leg(shape, noise, generic, plans, seed):
    pl, st = planner(shape, noise, generic)
    rng = np.random.default_rng(seed)
    ms = []
    for i in range(plans + 15):
        t0 = time.perf_counter()
        pl.plan(st, seed=seed, call=i)
        if i >= 15:
            ms.append(1e3 * (time.perf_counter() - t0))
        st = st + rng.normal(0, 0.02, st.shape).astype(np.float32)
    out = dict(ms=[round(x, 4) for x in ms], ms_median=float(np.median(ms)), graph=pl.graph_status(), rollout_path=pl.rollout_path(),
               launches_per_iteration=pl.launches_per_iteration(), action_noise=pl.action_noise()[0], noise_floats=pl.action_noise_floats())
    pl.close()
    return out


def child():
    """What the profiled process runs: 20 mixed plans of every shape."""
    for shape in SHAPES:
        pl, st = planner(shape, 'powerlaw', False)
        for i in range(20):
            pl.plan(st, seed=1, call=i)
        pl.close()


def kernel_stats():
    """[{name, mean us, calls}] of the mix kernel from a rocprofv3 --kernel-trace --stats run of --child."""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'mix', '--', sys.executable, os.path.abspath(__file__), '--child'],
                           capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            return dict(error=r.stderr[-500:])
        rows = []
        for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(f)):
                if KERNEL in row.get('Name', ''):
                    rows.append(dict(name=row['Name'][:80], mean_us=float(row['AverageNs']) / 1e3, calls=int(row['Calls']),
                                     note='all three shapes together: 20 plans each'))
        return rows


def scores(n_plans):
    """Mean best score of n_plans plans at B2's shape from perturbed states, the same states and seeds for every noise: information only."""
    out = {}
    for name, noise, beta in (('white', 'white', 0.0), ('beta_1', 'powerlaw', 1.0), ('beta_2', 'powerlaw', 2.0)):
        pl, st = planner('B2', noise, False, beta)
        rng = np.random.default_rng(7)
        best = []
        for i in range(n_plans):
            best.append(pl.plan(st, seed=3, call=i)[1])
            st = st + rng.normal(0, 0.02, st.shape).astype(np.float32)
        pl.close()
        out[name] = dict(mean_best_score=float(np.mean(best)), std=float(np.std(best)), plans=n_plans)
    return out


def main():
    if '--child' in sys.argv:
        return child()
    plans = int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 40
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 3
    legs = []
    for shape in SHAPES:
        for r in range(rounds):                               # the legs alternate inside a round: one machine, one warm clock
            for name, (noise, generic) in LEGS.items():
                legs.append(dict(shape=shape, leg=name, round=r, **leg(shape, noise, generic, plans, 1)))
    summary = {}
    for s in SHAPES:
        summary[s] = {n: float(np.median([x for l in legs if l['shape'] == s and l['leg'] == n for x in l['ms']])) for n in LEGS}
        summary[s]['round_medians'] = {n: [l['ms_median'] for l in legs if l['shape'] == s and l['leg'] == n] for n in LEGS}
        summary[s]['mixed_minus_white'] = summary[s]['mixed'] - summary[s]['white']
        summary[s]['white_generic_minus_white'] = summary[s]['white_generic'] - summary[s]['white']
        summary[s]['mixed_generic_minus_white_generic'] = summary[s]['mixed_generic'] - summary[s]['white_generic']
        summary[s]['rollout_path'] = {n: next(l['rollout_path'] for l in legs if l['shape'] == s and l['leg'] == n) for n in LEGS}
        summary[s]['launches_per_iteration'] = {n: next(l['launches_per_iteration'] for l in legs if l['shape'] == s and l['leg'] == n) for n in LEGS}
    doc = dict(plans=plans, rounds=rounds, beta=BETA, ms_median_of_all_plans=summary, legs=legs)
    if '--kernel-stats' in sys.argv:
        doc['mix_kernel_us'] = kernel_stats()
    if '--scores' in sys.argv:
        n = int(sys.argv[sys.argv.index('--score-plans') + 1]) if '--score-plans' in sys.argv else 50
        doc['mean_best_score_information_only'] = scores(n)
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
