#!/usr/bin/env python3
"""Per-plan wall time of a tracking plan with four zones and 0, 1, 4 and 16 linear outputs (cem_planner_set_task_outputs;
TrackingTask.outputs = TaskOutputs) of the same build on the same handle shape (captured graph, early stop off, fp32): the shipped
cem_mpc shape and B2.  Every leg launches the sampler, the handle's MODE 1 rollout kernel and ONE scoring kernel per iteration —
cem_task_zones_kernel without outputs, cem_task_outputs_kernel with — and moves its clock before every plan, as CemMpc does.  The
outputs are random combinations of the state with a weight, a target and a bound each, so that every term is live.
The kernels' time per launch comes from eager timed plans (cem_planner_set_timing: events around every launch), as the difference of the
reduce time of a task plan and of the Safety-Gym plan on the generic rollout, per iteration.
Medians of --rounds rounds x --plans plans, the legs alternating inside a round; host wall time around the plan call (result poll
included).
usage: time_task_outputs.py [--plans 40] [--rounds 3] > profiles/task_outputs.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, StateZones, TaskOutputs, TrackingTask, synthetic  # noqa: E402

SHAPES = {'cem_mpc': dict(variant='cem', ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10),
          'B2': dict(variant='cem', ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)}
OUTPUTS = (0, 1, 4, 16)
LEGS = tuple('outputs_%d' % m for m in OUTPUTS)
REF_STEPS = 256
N_ZONES = 4


def task(st, n_outputs):
    drift = np.linspace(0.0, 0.2, REF_STEPS, dtype=np.float32)[:, None]
    z = np.arange(N_ZONES)
    feats = np.stack([2 + 3 * z, 3 + 3 * z], axis=1)                           # pairs of features below 60
    zones = StateZones(axes=feats, centre=st[feats] + 0.3, radius=0.2, margin=0.2, penalty=1.0)
    outputs = None
    if n_outputs:
        C = np.random.default_rng(n_outputs).uniform(-1.0, 1.0, (n_outputs, st.shape[0])).astype(np.float32)
        y = C @ st
        outputs = TaskOutputs(matrix=C, weights=0.1, target=y + 0.1, linear=0.01, near=0.001, lo=y - 2.0, hi=y + 2.0, terminal_weights=0.4)
    return TrackingTask(reference=(st[None] + drift).astype(np.float32), q=1.0, c=0.01, goal_mask=1.0, lo=st - 0.5, hi=st + 0.5, rho=0.1,
                        goal_radius=0.05, reward_goal=1.0, terminal_weights=4.0, action_rate=0.05, outputs=outputs, zones=zones)


def planner(shape, n_outputs, use_graph=True, force=None):
    sh = dict(SHAPES[shape])
    pb = synthetic.problem(60, 2, sh['ensemble_size'])
    st = np.asarray(pb['state'], np.float32).copy()
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=use_graph,
                        task=None if n_outputs is None else task(st, n_outputs), **sh)
    if force:
        os.environ['CEM_FORCE_ROLLOUT'] = force                # read at create
    try:
        pl = CemPlanner(cfg)
    finally:
        os.environ.pop('CEM_FORCE_ROLLOUT', None)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl, st


def leg(shape, n_outputs, plans, seed):
    pl, st = planner(shape, n_outputs)
    rng = np.random.default_rng(seed)
    ms, action = [], np.zeros(2, np.float32)
    for i in range(plans + 15):
        t0 = time.perf_counter()
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
    """us per launch of the scoring kernel of every leg: eager timed plans, the reduce time (events around the score launches) of a task
    plan less that of the Safety-Gym plan on the generic rollout, per iteration."""
    red = {}
    for m in (None,) + OUTPUTS:
        pl, st = planner(shape, m, use_graph=False, force='generic')
        pl.set_timing(True)
        vals = []
        for i in range(plans + 5):
            if m is not None:
                pl.set_task_clock(i)
            _, _, iters = pl.plan(st, seed=1, call=i)
            pl.synchronize()
            if i >= 5:
                vals.append(pl.last_timing()['reduce_ms'] / max(iters, 1))
        red[m] = float(np.median(vals))
        pl.close()
    sh = SHAPES[shape]
    traj_bytes = sh['particles'] * sh['n_samples'] * (sh['horizon'] + 1) * 60 * 4
    out = dict(reduce_ms_per_iteration_gym=red[None], traj_bytes=traj_bytes)
    for m in OUTPUTS:
        us = 1e3 * (red[m] - red[None])
        name = 'task_zones_kernel' if m == 0 else 'task_outputs_kernel_%d_outputs' % m
        out[name + '_us'] = us
        out[name + '_traj_GBps'] = traj_bytes / (us * 1e-6) / 1e9 if us > 0 else None
    return out


def main():
    plans = int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 40
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 3
    legs, summary = [], {}
    for shape in SHAPES:
        for r in range(rounds):                               # the legs alternate inside a round: one machine, one warm clock
            for name, m in zip(LEGS, OUTPUTS):
                legs.append(dict(shape=shape, leg=name, round=r, **leg(shape, m, plans, 1)))
        mine = [l for l in legs if l['shape'] == shape]
        d = {n: float(np.median([x for l in mine if l['leg'] == n for x in l['ms']])) for n in LEGS}
        d['round_medians'] = {n: [l['ms_median'] for l in mine if l['leg'] == n] for n in LEGS}
        for n in LEGS[1:]:
            d[n + '_minus_outputs_0'] = d[n] - d['outputs_0']
        for key in ('rollout_path', 'launches_per_iteration', 'graph_nodes', 'graph'):
            d[key] = {n: next(l[key] for l in mine if l['leg'] == n) for n in LEGS}
        d['kernel'] = kernel_us(shape)
        summary[shape] = d
    print(json.dumps(dict(plans=plans, rounds=rounds, reference_steps=REF_STEPS, zones=N_ZONES, ms_median_of_all_plans=summary, legs=legs)))


if __name__ == '__main__':
    main()
