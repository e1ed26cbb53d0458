#!/usr/bin/env python3
"""Per-plan wall time of a plan with a tracking task (cem_planner_set_task_tracking; PlannerConfig.task = TrackingTask) beside a plan
with a quadratic task of the same build on the same handle shape (captured graph, early stop off, fp32): the shipped cem_mpc shape and
B2.  Both launch the sampler, the handle's MODE 1 rollout kernel and ONE scoring kernel per iteration — cem_task_reference_kernel or
cem_task_score_kernel; the tracking leg also moves its clock before every plan, as CemMpc does (cem_planner_set_task_clock: a
stream-ordered copy of 256 bytes), so its wall time includes that call.  The reference has 256 rows and the clock runs through it.
The kernels' time per launch comes from eager timed plans (cem_planner_set_timing: events around every launch), as the difference of the
reduce time of a task plan and of the Safety-Gym plan on the generic rollout, per iteration.
Medians of --rounds rounds x --plans plans, the legs alternating inside a round; host wall time around the plan call (result poll
included).
usage: time_tracking_task.py [--plans 40] [--rounds 3] > profiles/tracking_task.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, QuadraticTask, TrackingTask, synthetic  # noqa: E402

SHAPES = {'cem_mpc': dict(variant='cem', ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10),
          'B2': dict(variant='cem', ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)}
LEGS = ('quadratic', 'tracking')
REF_STEPS = 256


def tasks(st):
    common = dict(q=1.0, c=0.01, goal_mask=1.0, lo=st - 0.5, hi=st + 0.5, rho=0.1, goal_radius=0.05, reward_goal=1.0)
    drift = np.linspace(0.0, 0.2, REF_STEPS, dtype=np.float32)[:, None]
    return dict(quadratic=QuadraticTask(g=st, **common),
                tracking=TrackingTask(reference=(st[None] + drift).astype(np.float32), terminal_weights=4.0, action_rate=0.05, **common))


def planner(shape, kind, use_graph=True, force=None):
    sh = dict(SHAPES[shape])
    pb = synthetic.problem(60, 2, sh['ensemble_size'])
    st = np.asarray(pb['state'], np.float32).copy()
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=use_graph, task=tasks(st).get(kind), **sh)
    if force:
        os.environ['CEM_FORCE_ROLLOUT'] = force                # read at create
    try:
        pl = CemPlanner(cfg)
    finally:
        os.environ.pop('CEM_FORCE_ROLLOUT', None)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl, st


def leg(shape, kind, plans, seed):
    pl, st = planner(shape, kind)
    rng = np.random.default_rng(seed)
    ms, action = [], np.zeros(2, np.float32)
    for i in range(plans + 15):
        t0 = time.perf_counter()
        if kind == 'tracking':
            pl.set_task_clock(i, action)
        action, _, _ = pl.plan(st, seed=seed, call=i)
        t1 = time.perf_counter()
        if i >= 15:
            ms.append(1e3 * (t1 - t0))
        st = st + rng.normal(0, 0.02, st.shape).astype(np.float32)
    out = dict(ms=[round(x, 4) for x in ms], ms_median=float(np.median(ms)), graph=pl.graph_status(), graph_nodes=pl.graph_nodes(),
               rollout_path=pl.rollout_path(), launches_per_iteration=pl.launches_per_iteration())
    pl.close()
    return out


def kernel_us(shape, plans=20):
    """us per launch of the two scoring kernels: eager timed plans, the reduce time (events around the score launches) of a task plan
    less that of the Safety-Gym plan on the generic rollout, per iteration."""
    red = {}
    for kind in (None,) + LEGS:
        pl, st = planner(shape, kind, use_graph=False, force='generic')
        pl.set_timing(True)
        vals = []
        for i in range(plans + 5):
            if kind == 'tracking':
                pl.set_task_clock(i)
            _, _, iters = pl.plan(st, seed=1, call=i)
            pl.synchronize()
            if i >= 5:
                vals.append(pl.last_timing()['reduce_ms'] / max(iters, 1))
        red[kind] = float(np.median(vals))
        pl.close()
    return dict(reduce_ms_per_iteration_gym=red[None], reduce_ms_per_iteration_quadratic=red['quadratic'],
                reduce_ms_per_iteration_tracking=red['tracking'], task_score_kernel_us=1e3 * (red['quadratic'] - red[None]),
                task_reference_kernel_us=1e3 * (red['tracking'] - red[None]))


def main():
    plans = int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 40
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 3
    legs, summary = [], {}
    for shape in SHAPES:
        for r in range(rounds):                               # the legs alternate inside a round: one machine, one warm clock
            for name in LEGS:
                legs.append(dict(shape=shape, leg=name, round=r, **leg(shape, name, plans, 1)))
        mine = [l for l in legs if l['shape'] == shape]
        d = {n: float(np.median([x for l in mine if l['leg'] == n for x in l['ms']])) for n in LEGS}
        d['round_medians'] = {n: [l['ms_median'] for l in mine if l['leg'] == n] for n in LEGS}
        d['tracking_minus_quadratic'] = d['tracking'] - d['quadratic']
        for key in ('rollout_path', 'launches_per_iteration', 'graph_nodes', 'graph'):
            d[key] = {n: next(l[key] for l in mine if l['leg'] == n) for n in LEGS}
        d['kernel'] = kernel_us(shape)
        summary[shape] = d
    print(json.dumps(dict(plans=plans, rounds=rounds, reference_steps=REF_STEPS, ms_median_of_all_plans=summary, legs=legs)))


if __name__ == '__main__':
    main()
