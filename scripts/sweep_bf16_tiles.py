#!/usr/bin/env python3
"""Diagnostic: the bf16 rollout (precision 'bf16', csrc/cem_rollout_bf16.h) over population sizes and tile sizes (K = P members, H = 30,
I = 5): plan time with 1 / 2 / 3 / 4 chunks per tile and with the library's own choice, per input family (obs 60 act 2 K 5: one input
block per wave; obs 100 act 12 K 8: two).  The last column is the load auto_chunks_chunked keys its table on: row-chunks per CU at
one-chunk tiles.  usage: python scripts/sweep_bf16_tiles.py [--family 60|100] [N ...] > profiles/bf16_tile_sizes.txt"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, synthetic

FAMILIES = {60: (60, 2, 5, [500, 800, 1200, 1600, 2000, 2400, 3200, 4000, 8000]), 100: (100, 12, 8, [512, 768, 1024, 1536, 2048, 3072, 4096])}
args = sys.argv[1:]
only = None
if '--family' in args:
    only = int(args[args.index('--family') + 1]); del args[args.index('--family'):args.index('--family') + 2]
H, I = 30, 5
cus = torch.cuda.get_device_properties(0).multi_processor_count
print("# bf16 rollout (precision 'bf16', csrc/cem_rollout_bf16.h): plan ms (captured graph, %d iterations, H = %d) at 1 / 2 / 3 / 4 chunks per tile" % (I, H))
print('# and at the size auto_chunks_chunked picks (its table, kBf16Step, holds the m-co-resident-tiles figures of the rc columns); %d CUs' % cus, flush=True)
for fam, (obs, act, K, sizes) in FAMILIES.items():
    if only and fam != only:
        continue
    pb = synthetic.problem(obs, act, K)
    for N in [int(a) for a in args] or sizes:
        row = []
        for rc in (1, 2, 3, 4, 0):
            cfg = PlannerConfig(obs_dim=obs, act_dim=act, ensemble_size=K, particles=K, n_samples=N, horizon=H, n_elite=max(1, N // 10), iterations=I,
                                scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3, use_graph=True, chunks_per_tile=rc,
                                precision='bf16')
            pl = CemPlanner(cfg); pl.set_weights(pb['weights']); pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
            for i in range(8):
                pl.plan(pb['state'], seed=1, call=i)
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(12):
                pl.plan(pb['state'], seed=1, call=10 + i)
            torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / 12
            row.append('%s%d: %.3f ms' % ('auto->' if rc == 0 else 'rc ', pl.tiles()[0], dt * 1e3))
            pl.close()
        chunks = K * ((N + 15) // 16)
        print('obs %3d N %5d (%5d chunks, load %.2f per CU)  %s' % (obs, N, chunks, chunks / cus, '   '.join(row)), flush=True)
