#!/usr/bin/env python3
"""Cost of a COLD plan on one build, for a same-machine A/B of two builds (the tree to measure comes first on PYTHONPATH; only calls
that exist on both sides of the warm-start change are used).  Shipped cem_mpc and safe_cem_mpc shapes on a single-state handle and the
shipped cem_mpc shape on a batch handle with 8 problems; captured graph, early stop off.  Host wall time around the plan call (its
result poll included).  Prints one JSON line: {leg: {ms_median, ms: [...]}}.  --profile: a short run for a kernel trace instead."""
import json
import os
import sys
import time

import numpy as np

if os.environ.get('AB_TREE'):
    sys.path.insert(0, os.environ['AB_TREE'])
else:
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ethz_safe_learning_amd import BatchCemPlanner, CemPlanner, PlannerConfig, synthetic  # noqa: E402

SHAPES = {'cem_mpc': ('cem', dict(ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10)),
          'safe_cem_mpc': ('safe', dict(ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9))}


def make(shape, batch=0):
    variant, s = SHAPES[shape]
    pb = synthetic.problem(60, 2, s['ensemble_size'])
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3, variant=variant,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, **s)
    pl = BatchCemPlanner(cfg, batch) if batch else CemPlanner(cfg)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl, np.asarray(pb['state'], np.float32)


def leg(shape, batch, plans, warmup=20):
    pl, st = make(shape, batch)
    states = np.repeat(st[None], batch, 0) if batch else None
    ms = []
    for i in range(warmup + plans):
        t0 = time.perf_counter()
        if batch:
            pl.plan_batch(states, seed=1, calls=np.arange(batch, dtype=np.uint64) + 8 * i)
        else:
            pl.plan(st, seed=1, call=i)
        if i >= warmup:
            ms.append(1e3 * (time.perf_counter() - t0))
    pl.close()
    return dict(ms_median=float(np.median(ms)), ms=[round(x, 4) for x in ms])


def main():
    plans = 10 if '--profile' in sys.argv else (int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 200)
    out = {'cem_mpc': leg('cem_mpc', 0, plans), 'safe_cem_mpc': leg('safe_cem_mpc', 0, plans), 'cem_mpc_batch8': leg('cem_mpc', 8, plans)}
    print(json.dumps(out))


if __name__ == '__main__':
    main()
