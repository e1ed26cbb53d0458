#!/usr/bin/env python3
"""us per select launch (HIP events, set_timing) for forms 0 and 1 of the same build at B2, B1 and the shipped cem_mpc shape."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, synthetic

SHAPES = [('B2', dict(E=5, P=5, N=2000, H=30, k=200, I=5)), ('B1', dict(E=5, P=5, N=500, H=25, k=50, I=5)),
          ('shipped_cem_mpc', dict(E=15, P=5, N=150, H=8, k=15, I=10))]
for name, s in SHAPES:
    pb = synthetic.problem(60, 2, s['E'])
    for rnd in range(2):
        for form in (0, 1):
            if form == 0:
                os.environ['CEM_FORCE_SELECT'] = 'bucket'
            else:
                os.environ.pop('CEM_FORCE_SELECT', None)
            cfg = PlannerConfig(obs_dim=60, act_dim=2, ensemble_size=s['E'], particles=s['P'], n_samples=s['N'], horizon=s['H'], n_elite=s['k'],
                                iterations=s['I'], scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3, use_graph=False)
            pl = CemPlanner(cfg); pl.set_weights(pb['weights']); pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
            assert pl.select_form(0) == form and pl.select_mode() == 1
            for i in range(5):
                pl.plan(pb['state'], seed=1, call=i)
            pl.set_timing(True)
            per = []
            for i in range(40):
                pl.plan(pb['state'], seed=2, call=i); tm = pl.last_timing(); per.append(1e3 * tm['select_ms'] / tm['rollout_launches'])
            per = np.array(per)
            print('%-16s round %d form %d  select us/launch: median %.2f  mean %.2f  min %.2f  max %.2f' % (name, rnd, form, np.median(per), per.mean(), per.min(), per.max()), flush=True)
            pl.close()
