#!/usr/bin/env python3
"""Per-plan wall time of a plan with the plan read-out (cem_planner_set_plan_readout; PlannerConfig.plan_readout) beside the plan without
it of the same build on the same handle shape (captured graph, early stop off): the shipped cem_mpc and safe_cem_mpc shapes and B2.  The
read-out adds one launch per iteration, cem_plan_track_kernel behind the select, and changes no other: the rollout path and form are
reported for both legs.  Each shape is measured two ways,
  off   a handle created as usual
  on    plan_readout = True; the leg also reads the block after every plan (CemPlanner.plan_readout: a stream drain and four small copies),
        timed apart as `read_ms`
and from the two the cost of a DECISION under replan_every = r is derived, not measured again: a plan every r-th decision, nothing on
the GPU in between (noise_stddev = 0), i.e. plans per decision 1 / r and (on + read) / r milliseconds per decision.  Medians of --rounds
rounds x --plans plans, the legs alternating inside a round; host wall time around the plan call (result poll included).
With --trace DIR the script instead runs 20 plans of the `on` leg of every shape and exits, for a kernel trace taken around it (the
tracker's share of the plan's kernel time).
usage: time_plan_readout.py [--plans 40] [--rounds 3] > profiles/plan_readout.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, synthetic  # noqa: E402

SHAPES = {'cem_mpc': dict(variant='cem', ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10),
          'safe_cem_mpc': dict(variant='safe', ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9),
          'B2': dict(variant='cem', ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)}
LEGS = {'off': False, 'on': True}
REPLAN = (2, 3)


def planner(shape, on):
    sh = dict(SHAPES[shape])
    pb = synthetic.problem(60, 2, sh['ensemble_size'])
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=True, plan_readout=on, **sh)
    pl = CemPlanner(cfg)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl, np.asarray(pb['state'], np.float32).copy()


def leg(shape, on, plans, seed):
    pl, st = planner(shape, on)
    rng = np.random.default_rng(seed)
    ms, read = [], []
    for i in range(plans + 15):
        t0 = time.perf_counter()
        pl.plan(st, seed=seed, call=i)
        t1 = time.perf_counter()
        if on:
            blk = pl.plan_readout()
            assert blk.flags == 0 and blk.candidate >= 0
        t2 = time.perf_counter()
        if i >= 15:
            ms.append(1e3 * (t1 - t0))
            read.append(1e3 * (t2 - t1))
        st = st + rng.normal(0, 0.02, st.shape).astype(np.float32)
    out = dict(ms=[round(x, 4) for x in ms], ms_median=float(np.median(ms)), graph=pl.graph_status(), graph_nodes=pl.graph_nodes(),
               rollout_path=pl.rollout_path(), rollout_form=pl.rollout_form(0), launches_per_iteration=pl.launches_per_iteration())
    if on:
        out.update(read_ms=[round(x, 4) for x in read], read_ms_median=float(np.median(read)))
    pl.close()
    return out


def trace_run():
    for shape in SHAPES:
        pl, st = planner(shape, True)
        for i in range(20):
            pl.plan(st, seed=1, call=i)
        pl.plan_readout()
        pl.close()


def main():
    if '--trace' in sys.argv:
        return trace_run()
    plans = int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 40
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 3
    legs = []
    for shape in SHAPES:
        for r in range(rounds):                               # the legs alternate inside a round: one machine, one warm clock
            for name, on in LEGS.items():
                legs.append(dict(shape=shape, leg=name, round=r, **leg(shape, on, plans, 1)))
    summary = {}
    for s in SHAPES:
        d = {n: float(np.median([x for l in legs if l['shape'] == s and l['leg'] == n for x in l['ms']])) for n in LEGS}
        d['round_medians'] = {n: [l['ms_median'] for l in legs if l['shape'] == s and l['leg'] == n] for n in LEGS}
        d['read_ms'] = float(np.median([x for l in legs if l['shape'] == s and l['leg'] == 'on' for x in l['read_ms']]))
        d['on_minus_off'] = d['on'] - d['off']
        d['per_decision'] = {'off_replan_1': dict(plans_per_decision=1.0, ms=d['off']), 'on_replan_1': dict(plans_per_decision=1.0, ms=d['on'] + d['read_ms'])}
        for r in REPLAN:
            d['per_decision']['on_replan_%d' % r] = dict(plans_per_decision=1.0 / r, ms=(d['on'] + d['read_ms']) / r)
        for key in ('rollout_path', 'rollout_form', 'launches_per_iteration', 'graph_nodes'):
            d[key] = {n: next(l[key] for l in legs if l['shape'] == s and l['leg'] == n) for n in LEGS}
        summary[s] = d
    print(json.dumps(dict(plans=plans, rounds=rounds, replan_every=list(REPLAN), ms_median_of_all_plans=summary, legs=legs)))


if __name__ == '__main__':
    main()
