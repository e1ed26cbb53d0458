#!/usr/bin/env python3
"""Per-plan wall time of a plan with a task scorer (cem_planner_set_task; PlannerConfig.task) beside the Safety-Gym plan of the same
build on the same handle shape (captured graph, early stop off): the shipped cem_mpc and safe_cem_mpc shapes and B2, on precision fp32
and bf16.  A task plan launches the sampler, the handle's MODE 1 rollout kernel (which writes every row's state trajectory) and
cem_task_score_kernel; it has no lean form, no folded sampler and no floating segments.  The Safety-Gym plan is therefore measured
twice: as create chooses its rollout (`gym`), and with CEM_FORCE_ROLLOUT=generic (`gym_generic`: what the task plan gives up apart from
the trajectory traffic).  The task leg is measured under both settings too (`task`, `task_generic`): they launch the same kernels.
The new kernel's time per launch comes from eager timed plans (cem_planner_set_timing: events around every launch), as the difference of
the reduce time of a task plan and of the Safety-Gym plan, per iteration.
Medians of --rounds rounds x --plans plans, the legs alternating inside a round; host wall time around the plan call (result poll
included).
usage: time_task_scorer.py [--plans 40] [--rounds 3] > profiles/task_scorer.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, QuadraticTask, synthetic  # noqa: E402

SHAPES = {'cem_mpc': dict(variant='cem', ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10),
          'safe_cem_mpc': dict(variant='safe', ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9),
          'B2': dict(variant='cem', ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)}
PRECISIONS = ('fp32', 'bf16')
LEGS = {'gym': (False, None), 'task': (True, None), 'gym_generic': (False, 'generic'), 'task_generic': (True, 'generic')}


def planner(shape, precision, task_on, force, use_graph=True):
    sh = dict(SHAPES[shape])
    pb = synthetic.problem(60, 2, sh['ensemble_size'])
    st = np.asarray(pb['state'], np.float32).copy()
    task = QuadraticTask(q=1.0, g=st, c=0.01, goal_mask=1.0, lo=st - 0.5, hi=st + 0.5, rho=0.1, goal_radius=0.05, reward_goal=1.0) if task_on else None
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=use_graph, precision=precision, task=task, **sh)
    if force:
        os.environ['CEM_FORCE_ROLLOUT'] = force                # read at create
    else:
        os.environ.pop('CEM_FORCE_ROLLOUT', None)
    try:
        pl = CemPlanner(cfg)
    finally:
        os.environ.pop('CEM_FORCE_ROLLOUT', None)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl, st


def leg(shape, precision, task_on, force, plans, seed):
    pl, st = planner(shape, precision, task_on, force)
    rng = np.random.default_rng(seed)
    ms = []
    for i in range(plans + 15):
        t0 = time.perf_counter()
        pl.plan(st, seed=seed, call=i)
        t1 = time.perf_counter()
        if i >= 15:
            ms.append(1e3 * (t1 - t0))
        st = st + rng.normal(0, 0.02, st.shape).astype(np.float32)
    out = dict(ms=[round(x, 4) for x in ms], ms_median=float(np.median(ms)), graph=pl.graph_status(), graph_nodes=pl.graph_nodes(),
               rollout_path=pl.rollout_path(), rollout_form=pl.rollout_form(0), launches_per_iteration=pl.launches_per_iteration())
    pl.close()
    return out


def kernel_us(shape, precision, plans=20):
    """us per launch of cem_task_score_kernel: eager timed plans, the reduce time (events around the score launches) of a task plan less
    that of the Safety-Gym plan, per iteration."""
    red = {}
    for task_on in (False, True):
        pl, st = planner(shape, precision, task_on, 'generic', use_graph=False)
        pl.set_timing(True)
        vals = []
        for i in range(plans + 5):
            _, _, iters = pl.plan(st, seed=1, call=i)
            pl.synchronize()
            if i >= 5:
                vals.append(pl.last_timing()['reduce_ms'] / max(iters, 1))
        red[task_on] = float(np.median(vals))
        pl.close()
    return dict(reduce_ms_per_iteration_gym=red[False], reduce_ms_per_iteration_task=red[True], task_kernel_us=1e3 * (red[True] - red[False]))


def main():
    plans = int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 40
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 3
    legs, summary = [], {}
    for shape in SHAPES:
        for prec in PRECISIONS:
            for r in range(rounds):                           # the legs alternate inside a round: one machine, one warm clock
                for name, (task_on, force) in LEGS.items():
                    legs.append(dict(shape=shape, precision=prec, leg=name, round=r, **leg(shape, prec, task_on, force, plans, 1)))
            mine = [l for l in legs if l['shape'] == shape and l['precision'] == prec]
            d = {n: float(np.median([x for l in mine if l['leg'] == n for x in l['ms']])) for n in LEGS}
            d['round_medians'] = {n: [l['ms_median'] for l in mine if l['leg'] == n] for n in LEGS}
            d['task_minus_gym'] = d['task'] - d['gym']
            d['task_minus_gym_generic'] = d['task_generic'] - d['gym_generic']
            for key in ('rollout_path', 'rollout_form', 'launches_per_iteration', 'graph_nodes', 'graph'):
                d[key] = {n: next(l[key] for l in mine if l['leg'] == n) for n in LEGS}
            d['kernel'] = kernel_us(shape, prec)
            sh = SHAPES[shape]
            d['trajectory_bytes_per_iteration'] = sh['particles'] * sh['n_samples'] * (sh['horizon'] + 1) * 60 * 4
            summary['%s/%s' % (shape, prec)] = d
    print(json.dumps(dict(plans=plans, rounds=rounds, ms_median_of_all_plans=summary, legs=legs)))


if __name__ == '__main__':
    main()
