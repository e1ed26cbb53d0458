#!/usr/bin/env python3
"""Batched planning throughput: plans/s and states/s of cem_planner_plan_batch for B in {1, 2, 4, 8, 16, 32, 64} at the shipped
`cem_mpc` shape, the shipped `safe_cem_mpc` shape and BASELINE B2, against the single-state handle of the same shape in the same
process.  Captured-graph plans on the Philox path (what a policy runs), device-synchronised wall time per window; after a warm-up of
every handle, timed windows alternate single / batch, R rounds, and the median window is reported.

  python scripts/time_batch_plans.py --out profiles/batch_states_per_s.json
  python scripts/time_batch_plans.py --shape cem_mpc --batch 8 --plans 50 --rounds 1      # one workload (e.g. under rocprofv3)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {          # E, P, N, H, k, I, variant, stddev_threshold (config.py's shipped policies; BASELINE B2)
    'cem_mpc': dict(E=15, P=5, N=150, H=8, k=15, I=10, variant='cem', thr=0.25),
    'safe_cem_mpc': dict(E=15, P=45, N=500, H=8, k=20, I=9, variant='safe', thr=0.25),
    'B2': dict(E=5, P=5, N=2000, H=30, k=200, I=5, variant='cem', thr=-1.0),
}
BATCHES = (1, 2, 4, 8, 16, 32, 64)


def window(fn, n, torch):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main(argv=None):
    import torch
    from tests import helpers as hp
    from ethz_safe_learning_amd import BatchCemPlanner
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', choices=sorted(SHAPES), action='append')
    ap.add_argument('--batch', type=int, action='append')
    ap.add_argument('--plans', type=int, default=30, help='plan calls per timed window')
    ap.add_argument('--rounds', type=int, default=5, help='alternating single / batch window pairs')
    ap.add_argument('--out', default=None)
    args = ap.parse_args(argv)
    shapes, batches = args.shape or sorted(SHAPES), args.batch or list(BATCHES)
    rows = []
    for name in shapes:
        s = SHAPES[name]
        # stddev_threshold -1: every plan runs all I iterations, so that states/s compares equal work (an early stop would make the
        # batch wait for its slowest problem and the single plan not)
        pb = hp.make_problem(60, 2, s['E'], 4, seed=1234)
        _, pcfg = hp.configs(pb, N=s['N'], H=s['H'], P=s['P'], E=s['E'], k=s['k'], I=s['I'], variant=s['variant'], thr=-1.0,
                             noise=1e-3, post=0.2, use_graph=True)
        single = hp.make_planner(pb, pcfg)
        rng = np.random.default_rng(0)
        states = (pb['state'][None] + rng.normal(0, 0.05, (max(batches), pb['state'].shape[0]))).astype(np.float32)
        for _ in range(5):
            single.plan(states[0], seed=1)
        for B in batches:
            pl = BatchCemPlanner(pcfg, B)
            pl.set_weights(pb['weights'])
            pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
            st = states[:B]
            for _ in range(5):                             # warm-up: capture + replays
                pl.plan_batch(st, seed=1)
                single.plan(st[0], seed=1)
            assert pl.graph_status() == 'graph' and single.graph_status() == 'graph'
            t_single, t_batch = [], []
            for _ in range(args.rounds):
                t_single.append(window(lambda: single.plan(st[0], seed=1), args.plans, torch) / args.plans)
                t_batch.append(window(lambda: pl.plan_batch(st, seed=1), args.plans, torch) / args.plans)
            ms1, msb = 1e3 * float(np.median(t_single)), 1e3 * float(np.median(t_batch))
            row = dict(shape=name, B=B, single_ms=ms1, batch_ms=msb, single_states_per_s=1e3 / ms1, batch_plans_per_s=1e3 / msb,
                       batch_states_per_s=B * 1e3 / msb, gain_states_per_s=(B * 1e3 / msb) / (1e3 / ms1),
                       single_ms_windows=[1e3 * x for x in t_single], batch_ms_windows=[1e3 * x for x in t_batch],
                       launches_per_iteration=pl.launches_per_iteration(), single_launches_per_iteration=single.launches_per_iteration(),
                       chunks_per_tile_single=single.tiles()[0])
            rows.append(row)
            print('%-13s B=%-3d single %.3f ms (%.0f states/s)  batch %.3f ms (%.0f plans/s, %.0f states/s)  gain %.2fx'
                  % (name, B, ms1, 1e3 / ms1, msb, 1e3 / msb, B * 1e3 / msb, row['gain_states_per_s']), flush=True)
            pl.close()
        single.close()
    if args.out:
        import bench
        rec = dict(what='batched planning throughput (scripts/time_batch_plans.py): captured-graph Philox plans, all I iterations '
                        '(stddev_threshold -1), median of %d alternating single / batch windows of %d plan calls each, '
                        'device-synchronised wall time' % (args.rounds, args.plans),
                   device=torch.cuda.get_device_name(0), date=time.strftime('%Y-%m-%d'), source_sha16=bench.source_sha16(), rows=rows)
        with open(args.out, 'w') as fh:
            json.dump(rec, fh, indent=1)
    return rows


if __name__ == '__main__':
    main()
