"""Time the weight sync of a planner handle after a fit, on its two routes:

  host    CemTrainer.get_weights (device -> host -> Python lists) + CemPlanner.set_weights (flatten, the host packers of cem_capi.hip on
          one thread, four or five uploads, a stream synchronise) — the only route before cem_planner_set_weights_dev existed
  device  CemPlanner.set_weights_from(trainer): the pack kernels of csrc/cem_pack.h read the trainer's workspace (the wall time includes
          a stream synchronise here, which the route itself does not need)

per handle at the shipped cem_mpc / safe_cem_mpc shapes (E = 15), B2 (E = 5; fp32 and bf16x3) and a 256-unit wide model; the pack
kernels' own device time from HIP events around the call on the planner's stream; and the weight sync of all 36 handles of the
scripts/tune_cem_policy.py grid, both ways.  Recorded, not gated: profiles/weight_handover.json.

    python scripts/time_weight_handover.py [--out profiles/weight_handover.json]"""
import argparse
import itertools
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {
    # name: (planner overrides, model (units, layers, activation))
    'cem_mpc': (dict(ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10), (128, 4, 'relu')),
    'safe_cem_mpc': (dict(ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9, variant='safe'), (128, 4, 'relu')),
    'B2': (dict(ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5), (128, 4, 'relu')),
    'B2_bf16x3': (dict(ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5, precision='bf16x3'), (128, 4, 'relu')),
    'wide_256': (dict(ensemble_size=5, particles=5, n_samples=500, horizon=8, n_elite=20, iterations=5), (256, 4, 'relu')),
}
O, A = 60, 2


def planner_config(over, units, layers, activation):
    from ethz_safe_learning_amd import PlannerConfig, ScorerConfig
    return PlannerConfig(obs_dim=O, act_dim=A, units=units, n_layers=layers, activation=activation,
                         scorer=ScorerConfig(goal_slice=(3, 19), cost_kinds=[(22, 38, 0.2)]), act_low=[-1.0] * A, act_high=[1.0] * A, **over)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'weight_handover.json'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    import torch
    from ethz_safe_learning_amd import CemPlanner
    from ethz_safe_learning_amd.trainer import CemTrainer, unflatten_weights

    def trainer(E, units, layers, activation):
        tr = CemTrainer(O + A, O, units, layers, E, activation=activation)
        n = tr.weights_dev().numel()
        tr.set_state(unflatten_weights(np.random.default_rng(0).normal(0, 0.05, n).astype(np.float32), *tr.dims))
        return tr

    def wall(fn):
        ts = []
        for i in range(args.warmup + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append((time.perf_counter() - t0) * 1e6)
        return dict(median=float(np.median(ts)), min=float(np.min(ts)))

    def events(stream, fn):
        ts = []
        for i in range(args.warmup + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(stream)
            fn()
            e1.record(stream)
            torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(e0.elapsed_time(e1) * 1e3)
        return dict(median=float(np.median(ts)), min=float(np.min(ts)))

    out = dict(device=torch.cuda.get_device_name(0), reps=args.reps, warmup=args.warmup, unit='us', handles=[])
    for name, (over, (units, layers, act)) in SHAPES.items():
        tr = trainer(over['ensemble_size'], units, layers, act)
        pl = CemPlanner(planner_config(over, units, layers, act))
        rec = dict(shape=name, ensemble_size=over['ensemble_size'], blob_floats=tr.weights_dev().numel(),
                   host_route_wall_us=wall(lambda: pl.set_weights(tr.get_weights())),
                   host_get_weights_wall_us=wall(tr.get_weights),
                   device_route_wall_us=wall(lambda: pl.set_weights_from(tr)),
                   pack_kernels_device_us=events(pl.stream, lambda: pl.set_weights_from(tr)))
        out['handles'].append(rec)
        print(json.dumps(rec))
        pl.close(); tr.close()

    # the 36 shapes scripts/tune_cem_policy.py walks (its horizons x (proposals, iterations) x elite ratios), one handle each, synced once
    # (15 particles: every proposal count then splits over the 15 members)
    over0, (units, layers, act) = SHAPES['cem_mpc']
    tr = trainer(over0['ensemble_size'], units, layers, act)
    grid = list(itertools.product((8, 10, 12, 15), ((100, 15), (150, 10), (300, 5)), (0.05, 0.1, 0.2)))     # HORIZONS x PROPOSALS_WITH_ITERATIONS x ELITE_RATIOS
    handles = [CemPlanner(planner_config(dict(over0, particles=15, horizon=h, iterations=i, n_samples=n, n_elite=round(f * n)), units, layers, act))
               for h, (n, i), f in grid]

    def sync_all(device):
        ws = None if device else tr.get_weights()               # the host route fetches the weights once for all handles, as the model does
        for pl in handles:
            pl.set_weights_from(tr) if device else pl.set_weights(ws)
    out['tune_grid'] = dict(handles=len(handles), host_route_wall_us=wall(lambda: sync_all(False)), device_route_wall_us=wall(lambda: sync_all(True)))
    print(json.dumps(out['tune_grid']))
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
