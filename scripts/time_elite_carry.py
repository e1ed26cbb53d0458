#!/usr/bin/env python3
"""Per-plan wall time of a plan with elite carry-over (cem_planner_set_elite_carry; PlannerConfig.keep_elites) beside the plan without it
of the same build on the same handle shape (captured graph, early stop off): the shipped cem_mpc and safe_cem_mpc shapes and B2.  A plan
that carries elites samples in a launch of its own (cem_sample_kernel), runs the generic rollout kernels and launches the inject and the
keep in every iteration; a plan that does not folds the sampler into the rollout launch and runs the lean kernels where the handle is
eligible.  Each shape is therefore measured four ways:
  off            a handle created as usual (`rollout_path`, `launches_per_iteration` say what it runs)
  off_forced     created under CEM_FORCE_SAMPLER=kernel and CEM_FORCE_ROLLOUT=generic: the sampler launch and the generic rollout, no carry
  keep           keep_elites = max(1, floor(0.3 n_elite)), inside plans only
  keep_across    the same, and the first iteration of every plan takes the previous plan's store shifted by one step
so that the price of giving up the lean path and the folded sampler (off_forced - off) and the price of the two new launches
(keep - off_forced; the inject of iteration 0: keep_across - keep) are told apart.  Medians of --rounds rounds x --plans plans, the
legs alternating inside a round; host wall time around the plan call (result poll included).
usage: time_elite_carry.py [--plans 40] [--rounds 3] > profiles/elite_carry.json"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, synthetic  # noqa: E402
from ethz_safe_learning_amd.planner import elite_keep_count  # noqa: E402

SHAPES = {'cem_mpc': dict(variant='cem', ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10),
          'safe_cem_mpc': dict(variant='safe', ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9),
          'B2': dict(variant='cem', ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)}
# leg -> (keep elites, across plans, force the sampler launch and the generic rollout at create)
LEGS = {'off': (False, False, False), 'off_forced': (False, False, True), 'keep': (True, False, False), 'keep_across': (True, True, False)}
FRACTION = 0.3
FORCED = {'CEM_FORCE_SAMPLER': 'kernel', 'CEM_FORCE_ROLLOUT': 'generic'}


def planner(shape, keep, across, forced):
    sh = dict(SHAPES[shape])
    pb = synthetic.problem(60, 2, sh['ensemble_size'])
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=True,
                        keep_elites=elite_keep_count(FRACTION, sh['n_elite']) if keep else 0, shift_elites=across, **sh)
    before = {k: os.environ.get(k) for k in FORCED}
    if forced:
        os.environ.update(FORCED)                                   # read once, when the handle is created
    try:
        pl = CemPlanner(cfg)
    finally:
        if forced:
            for k, v in before.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl, np.asarray(pb['state'], np.float32).copy()


def leg(shape, keep, across, forced, plans, seed):
    pl, st = planner(shape, keep, across, forced)
    rng = np.random.default_rng(seed)
    ms = []
    for i in range(plans + 15):
        t0 = time.perf_counter()
        pl.plan(st, seed=seed, call=i)
        if i >= 15:
            ms.append(1e3 * (time.perf_counter() - t0))
        st = st + rng.normal(0, 0.02, st.shape).astype(np.float32)
    out = dict(ms=[round(x, 4) for x in ms], ms_median=float(np.median(ms)), graph=pl.graph_status(), rollout_path=pl.rollout_path(),
               launches_per_iteration=pl.launches_per_iteration(), elite_carry=list(pl.elite_carry()))
    pl.close()
    return out


def main():
    plans = int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 40
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 3
    legs = []
    for shape in SHAPES:
        for r in range(rounds):                               # the legs alternate inside a round: one machine, one warm clock
            for name, (keep, across, forced) in LEGS.items():
                legs.append(dict(shape=shape, leg=name, round=r, **leg(shape, keep, across, forced, plans, 1)))
    summary = {}
    for s in SHAPES:
        summary[s] = {n: float(np.median([x for l in legs if l['shape'] == s and l['leg'] == n for x in l['ms']])) for n in LEGS}
        summary[s]['round_medians'] = {n: [l['ms_median'] for l in legs if l['shape'] == s and l['leg'] == n] for n in LEGS}
        summary[s]['off_forced_minus_off'] = summary[s]['off_forced'] - summary[s]['off']
        summary[s]['keep_minus_off_forced'] = summary[s]['keep'] - summary[s]['off_forced']
        summary[s]['keep_across_minus_keep'] = summary[s]['keep_across'] - summary[s]['keep']
        summary[s]['keep_minus_off'] = summary[s]['keep'] - summary[s]['off']
        summary[s]['rollout_path'] = {n: next(l['rollout_path'] for l in legs if l['shape'] == s and l['leg'] == n) for n in LEGS}
        summary[s]['launches_per_iteration'] = {n: next(l['launches_per_iteration'] for l in legs if l['shape'] == s and l['leg'] == n) for n in LEGS}
    print(json.dumps(dict(plans=plans, rounds=rounds, keep_fraction=FRACTION, ms_median_of_all_plans=summary, legs=legs)))


if __name__ == '__main__':
    main()
