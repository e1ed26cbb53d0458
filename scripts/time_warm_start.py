#!/usr/bin/env python3
"""Per-plan wall time of cold and warm-started plans on one build (captured graph): B2 and the shipped cem_mpc / safe_cem_mpc shapes.
Early stop off measures the cost of the first kernel at equal work (COLD against SHIFT: same iteration count); with the shipped
threshold 0.25 and sigma 'keep' it shows the iterations a warm start saves on a drifting observation.  Prints one JSON document with
the raw per-plan times.  Times are host wall time around the plan call (result poll included).
usage: time_warm_start.py [--plans 40] [--rounds 3] > profiles/warm_start.json"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, synthetic  # noqa: E402

SHAPES = {'B2': dict(ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5),
          'cem_mpc': dict(ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10),
          'safe_cem_mpc': dict(ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9)}


def leg(shape, variant, thr, mode, plans, seed):
    pb = synthetic.problem(60, 2, SHAPES[shape]['ensemble_size'])
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3, variant=variant,
                        posterior_mean_threashold=0.3, stddev_threshold=thr, **SHAPES[shape])
    pl = CemPlanner(cfg)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    if mode != 'cold':
        pl.set_warm_start(shift=1, tail='repeat', sigma=mode, floor_frac=0.25)
        pl.set_init_mode('shift')
    rng = np.random.default_rng(seed)
    st = np.asarray(pb['state'], np.float32).copy()
    ms, its, scores = [], [], []
    for i in range(plans + 15):
        t0 = time.perf_counter()
        _, s, it = pl.plan(st, seed=seed, call=i)
        if i >= 15:
            ms.append(1e3 * (time.perf_counter() - t0)); its.append(int(it)); scores.append(float(s))
        st = st + rng.normal(0, 0.02, st.shape).astype(np.float32)
    pl.close()
    return dict(ms=[round(x, 4) for x in ms], ms_median=float(np.median(ms)), iterations_mean=float(np.mean(its)), score_mean=float(np.mean(scores)))


def main():
    plans = int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 40
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 3
    out = []
    for shape, variant in (('B2', 'cem'), ('B2', 'safe'), ('cem_mpc', 'cem'), ('safe_cem_mpc', 'safe')):
        for thr in ((-1.0,) if shape == 'B2' else (-1.0, 0.25)):
            for r in range(rounds):                       # the legs alternate inside a round: one machine, one warm clock
                for mode in ('cold', 'reset', 'keep'):
                    out.append(dict(shape=shape, variant=variant, stddev_threshold=thr, mode=mode, round=r, **leg(shape, variant, thr, mode, plans, 1)))
    print(json.dumps(dict(plans=plans, rounds=rounds, legs=out)))


if __name__ == '__main__':
    main()
