#!/usr/bin/env python3
"""Per-plan wall time of a plan on the lower-tail particle objective (cem_planner_set_particle_objective, CEM_PARTICLES_LOWER_TAIL;
PlannerConfig.worst_particles) beside the MEAN plan of the same build on the same handle shape (captured graph, early stop off): the
shipped cem_mpc and safe_cem_mpc shapes and B2, m = 1 and m = ceil(P / 5).  All legs launch the same rollout; the tail plan's reduce
(cem_constraint_tail_kernel) replaces cem_reduce_kernel on SafeCemMpc handles and is an EXTRA launch on CemMpc handles, whose mean the
select folds.  Medians of --rounds rounds x --plans plans, the legs alternating inside a round; host wall time around the plan call
(result poll included).
With --kernel-stats the two reduce kernels' mean device time comes from a `rocprofv3 --kernel-trace --stats` run of its own (a fresh
child process running --child at the shipped safe_cem_mpc shape), not from the timed legs.
usage: time_risk_objective.py [--plans 40] [--rounds 3] [--kernel-stats] > profiles/risk_objective.json"""
import csv
import glob
import json
import math
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, synthetic  # noqa: E402

SHAPES = {'cem_mpc': dict(variant='cem', ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10),
          'safe_cem_mpc': dict(variant='safe', ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9),
          'B2': dict(variant='cem', ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)}
KERNELS = ('cem_constraint_tail_kernel', 'cem_reduce_kernel')


def worst_of(shape):
    """{leg name: worst_particles}: the mean, the worst particle, a fifth of the particles."""
    P = SHAPES[shape]['particles']
    return {'mean': 0, 'm1': 1, 'm_fifth': int(math.ceil(P / 5))}


def planner(shape, worst):
    pb = synthetic.problem(60, 2, SHAPES[shape]['ensemble_size'])
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=True, worst_particles=worst, **SHAPES[shape])
    pl = CemPlanner(cfg)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl, np.asarray(pb['state'], np.float32).copy()


def leg(shape, worst, plans, seed):
    pl, st = planner(shape, worst)
    rng = np.random.default_rng(seed)
    ms, scores = [], []
    for i in range(plans + 15):
        t0 = time.perf_counter()
        _, s, it = pl.plan(st, seed=seed, call=i)
        if i >= 15:
            ms.append(1e3 * (time.perf_counter() - t0)); scores.append(float(s))
        st = st + rng.normal(0, 0.02, st.shape).astype(np.float32)
    out = dict(ms=[round(x, 4) for x in ms], ms_median=float(np.median(ms)), score_mean=float(np.mean(scores)), graph=pl.graph_status(),
               launches_per_iteration=pl.launches_per_iteration(), particle_objective=list(pl.particle_objective()))
    pl.close()
    return out


def child():
    """What the profiled process runs: 20 plans of the mean and of either tail at the shipped safe_cem_mpc shape."""
    for worst in worst_of('safe_cem_mpc').values():
        pl, st = planner('safe_cem_mpc', worst)
        for i in range(20):
            pl.plan(st, seed=1, call=i)
        pl.close()


def kernel_stats():
    """{kernel: mean us, calls} of the two reduce kernels from a rocprofv3 --kernel-trace --stats run of --child; None where absent."""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'risk', '--', sys.executable, os.path.abspath(__file__), '--child'],
                           capture_output=True, text=True, timeout=300)
        out = {k: None for k in KERNELS}
        if r.returncode != 0:
            return dict(error=r.stderr[-500:], **out)
        for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(f)):
                for k in KERNELS:
                    if row.get('Name', '').startswith(k):
                        out[k] = dict(mean_us=float(row['AverageNs']) / 1e3, calls=int(row['Calls']))
        return out


def main():
    if '--child' in sys.argv:
        return child()
    plans = int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 40
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 3
    legs = []
    for shape in SHAPES:
        for r in range(rounds):                               # the legs alternate inside a round: one machine, one warm clock
            for name, worst in worst_of(shape).items():
                legs.append(dict(shape=shape, leg=name, worst_particles=worst, round=r, **leg(shape, worst, plans, 1)))
    summary = {s: {n: float(np.median([x for l in legs if l['shape'] == s and l['leg'] == n for x in l['ms']])) for n in worst_of(s)} for s in SHAPES}
    for s in SHAPES:                                          # what the tail costs over the mean plan of the same build, as measured
        summary[s]['m1_minus_mean'] = summary[s]['m1'] - summary[s]['mean']
        summary[s]['m_fifth_minus_mean'] = summary[s]['m_fifth'] - summary[s]['mean']
        summary[s]['launches_per_iteration'] = {n: next(l['launches_per_iteration'] for l in legs if l['shape'] == s and l['leg'] == n) for n in worst_of(s)}
    doc = dict(plans=plans, rounds=rounds, ms_median_of_all_plans=summary, legs=legs)
    if '--kernel-stats' in sys.argv:
        doc['reduce_kernels_us'] = kernel_stats()
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
