#!/usr/bin/env python3
"""Per-plan wall time of a budget-constrained plan (cem_planner_set_constraint, CEM_CONSTRAINT_BUDGET; PlannerConfig.constraint) beside
the BETA plan of the same build on the same handle shape (captured graph, early stop off): the shipped safe_cem_mpc shape and B2 as a
SafeCemMpc handle, the cost statistic on the particle mean (`mean`) and on m_c = ceil(P / 5) worst particles (`tail`).  All legs launch
the same rollout and select; the constrained plan's reduce (cem_constrained_budget_kernel) replaces cem_reduce_kernel.  Each budget is
the median cost statistic of the handle's first iteration, so about half of the first iteration's candidates are infeasible.  Medians of
--rounds rounds x --plans plans, the legs alternating inside a round; host wall time around the plan call (result poll included).
With --kernel-stats the two reduce kernels' mean device time comes from a `rocprofv3 --kernel-trace --stats` run of its own (a fresh
child process running --child at the shipped safe_cem_mpc shape), not from the timed legs.
usage: time_cost_budget.py [--plans 40] [--rounds 3] [--kernel-stats] > profiles/cost_budget.json"""
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

SHAPES = {'safe_cem_mpc': dict(ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9),
          'B2': dict(ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)}
KERNELS = ('cem_constrained_budget_kernel', 'cem_reduce_kernel')


def legs_of(shape):
    """{leg name: (constraint, worst_cost_particles)}."""
    P = SHAPES[shape]['particles']
    return {'beta': ('beta', 0), 'mean': ('budget', 0), 'tail': ('budget', int(math.ceil(P / 5)))}


def planner(shape, constraint, worst_cost):
    pb = synthetic.problem(60, 2, SHAPES[shape]['ensemble_size'])
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3, variant='safe',
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=True, constraint=constraint,
                        worst_cost_particles=worst_cost, **SHAPES[shape])
    pl = CemPlanner(cfg)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    st = np.asarray(pb['state'], np.float32).copy()
    budget = None
    if constraint == 'budget':                                # the median cost statistic of the first iteration of plan (seed 1, call 0)
        pl.plan_begin(st, seed=1, call=0)
        pl.plan_rollout(0)
        budget = float(np.median(pl.constraint_costs()))
        for it in range(cfg.iterations):
            if it:
                pl.plan_rollout(it)
            pl.plan_select(it)
        pl.plan_end()
        pl.set_cost_budget(budget)
    return pl, st, budget


def leg(shape, constraint, worst_cost, plans, seed):
    pl, st, budget = planner(shape, constraint, worst_cost)
    rng = np.random.default_rng(seed)
    ms, feasible = [], 0
    for i in range(plans + 15):
        t0 = time.perf_counter()
        _, s, it = pl.plan(st, seed=seed, call=i)
        if i >= 15:
            ms.append(1e3 * (time.perf_counter() - t0)); feasible += int(s > -2.0 ** 100)
        st = st + rng.normal(0, 0.02, st.shape).astype(np.float32)
    out = dict(ms=[round(x, 4) for x in ms], ms_median=float(np.median(ms)), budget=budget, plans_with_a_feasible_best=feasible, graph=pl.graph_status(),
               launches_per_iteration=pl.launches_per_iteration(), constraint=list(pl.constraint()))
    pl.close()
    return out


def child():
    """What the profiled process runs: 20 plans of every leg at the shipped safe_cem_mpc shape."""
    for constraint, worst_cost in legs_of('safe_cem_mpc').values():
        pl, st, _ = planner('safe_cem_mpc', constraint, worst_cost)
        for i in range(20):
            pl.plan(st, seed=1, call=i)
        pl.close()


def kernel_stats():
    """{kernel: mean us, calls} of the two reduce kernels from a rocprofv3 --kernel-trace --stats run of --child; None where absent."""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'budget', '--', sys.executable, os.path.abspath(__file__), '--child'],
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
            for name, (constraint, worst_cost) in legs_of(shape).items():
                legs.append(dict(shape=shape, leg=name, round=r, **leg(shape, constraint, worst_cost, plans, 1)))
    summary = {}
    for s in SHAPES:
        summary[s] = {n: float(np.median([x for l in legs if l['shape'] == s and l['leg'] == n for x in l['ms']])) for n in legs_of(s)}
        # the spread: every round's own median, per leg
        summary[s]['round_medians'] = {n: [l['ms_median'] for l in legs if l['shape'] == s and l['leg'] == n] for n in legs_of(s)}
        summary[s]['mean_minus_beta'] = summary[s]['mean'] - summary[s]['beta']
        summary[s]['tail_minus_beta'] = summary[s]['tail'] - summary[s]['beta']
        summary[s]['launches_per_iteration'] = {n: next(l['launches_per_iteration'] for l in legs if l['shape'] == s and l['leg'] == n) for n in legs_of(s)}
    doc = dict(plans=plans, rounds=rounds, ms_median_of_all_plans=summary, legs=legs)
    if '--kernel-stats' in sys.argv:
        doc['reduce_kernels_us'] = kernel_stats()
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
