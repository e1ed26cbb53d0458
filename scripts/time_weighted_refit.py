#!/usr/bin/env python3
"""Per-plan wall time of a plan with the score-weighted refit (cem_planner_set_refit, CEM_REFIT_SOFTMAX; PlannerConfig.refit) beside the
UNIFORM plan of the same build on the same handle shape (captured graph, early stop off): the shipped cem_mpc and safe_cem_mpc shapes and
B2.  Legs: `uniform`; `softmax` at the shape's own n_elite; `softmax_kN` with n_elite = n_samples (MPPI), beside `uniform_kN`, the
uniform plan of that elite count.  A weighted plan launches the unchanged select plus cem_constraint_refit_kernel an iteration, and ends
with the final kernel.  Medians of --rounds rounds x --plans plans, the legs alternating inside a round; host wall time around the plan
call (result poll included).
With --kernel-stats the new kernel's mean device time beside cem_select_kernel's comes from a `rocprofv3 --kernel-trace --stats` run of
its own (a fresh child process running --child: 20 plans of every leg of every shape), not from the timed legs.
With --accuracy the file also records the largest error of one weighted select against the float64 restatement of
tests/weighted_cases.py, as a fraction of the tests' bars, over that file's cases (a development aid: it imports from tests/).
usage: time_weighted_refit.py [--plans 40] [--rounds 3] [--kernel-stats] [--accuracy] > profiles/weighted_refit.json"""
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, synthetic  # noqa: E402

SHAPES = {'cem_mpc': dict(variant='cem', ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10),
          'safe_cem_mpc': dict(variant='safe', ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9),
          'B2': dict(variant='cem', ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)}
LEGS = {'uniform': ('uniform', False), 'softmax': ('softmax', False), 'uniform_kN': ('uniform', True), 'softmax_kN': ('softmax', True)}
KERNELS = ('cem_constraint_refit_kernel', 'cem_select_kernel')
TEMPERATURE = 0.5


def planner(shape, refit, all_elite):
    sh = dict(SHAPES[shape])
    if all_elite:
        sh['n_elite'] = sh['n_samples']
    pb = synthetic.problem(60, 2, sh['ensemble_size'])
    cfg = PlannerConfig(obs_dim=60, act_dim=2, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=1e-3,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=True, refit=refit,
                        refit_temperature=TEMPERATURE if refit == 'softmax' else 0.0, **sh)
    pl = CemPlanner(cfg)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl, np.asarray(pb['state'], np.float32).copy()


def leg(shape, refit, all_elite, plans, seed):
    pl, st = planner(shape, refit, all_elite)
    rng = np.random.default_rng(seed)
    ms = []
    for i in range(plans + 15):
        t0 = time.perf_counter()
        pl.plan(st, seed=seed, call=i)
        if i >= 15:
            ms.append(1e3 * (time.perf_counter() - t0))
        st = st + rng.normal(0, 0.02, st.shape).astype(np.float32)
    out = dict(ms=[round(x, 4) for x in ms], ms_median=float(np.median(ms)), graph=pl.graph_status(),
               launches_per_iteration=pl.launches_per_iteration(), refit=list(pl.refit()), n_elite=pl.cfg.n_elite)
    if refit == 'softmax':
        out['ess_last_plan'] = [round(float(x), 3) for x in pl.refit_stats(0)]
    pl.close()
    return out


def child():
    """What the profiled process runs: 20 plans of every leg of every shape."""
    for shape in SHAPES:
        for refit, all_elite in LEGS.values():
            pl, st = planner(shape, refit, all_elite)
            for i in range(20):
                pl.plan(st, seed=1, call=i)
            pl.close()


def kernel_stats():
    """{kernel: [{name, mean us, calls}]} from a rocprofv3 --kernel-trace --stats run of --child (every instantiation of the select)."""
    with tempfile.TemporaryDirectory() as d:
        r = subprocess.run(['rocprofv3', '--kernel-trace', '--stats', '--output-format', 'csv', '-d', d, '-o', 'refit', '--', sys.executable, os.path.abspath(__file__), '--child'],
                           capture_output=True, text=True, timeout=400)
        out = {k: [] for k in KERNELS}
        if r.returncode != 0:
            return dict(error=r.stderr[-500:], **out)
        for f in glob.glob(os.path.join(d, '**', '*kernel_stats.csv'), recursive=True):
            for row in csv.DictReader(open(f)):
                for k in KERNELS:
                    if k in row.get('Name', ''):
                        out[k].append(dict(name=row['Name'][:80], mean_us=float(row['AverageNs']) / 1e3, calls=int(row['Calls'])))
        return out


def accuracy():
    """Largest |device - float64| over the bar, for mu and sigma, over the cases of tests/weighted_cases.py on CemMpc handles."""
    import torch
    from tests import helpers as hp
    from tests import weighted_cases as wc
    worst = dict(mu=0.0, sigma=0.0, mu_case=None, sigma_case=None)
    pbs = {}
    for case in wc.CASES:
        pb = pbs.setdefault(case.A, hp.make_problem(seed=42, act_dim=case.A))
        _, pcfg = hp.configs(pb, N=case.N, H=case.H, P=5, E=5, k=case.k, I=1, smoothing=0.25)
        pcfg.refit, pcfg.refit_temperature = 'softmax', case.tau
        pl = hp.make_planner(pb, pcfg)
        ea, em, _ = hp.noise(1, case.N, case.H, case.A, 5, 60, seed=1)
        pl.plan_begin(pb['state'], eps_act=ea, eps_model=em)
        pl.plan_rollout(0)
        actions, ms0 = pl.actions().cpu().numpy().copy(), pl.mu_sigma().cpu().numpy().copy()
        pl.scores_global().copy_(torch.from_numpy(case.scores))
        torch.cuda.synchronize()
        pl.plan_select(0)
        ms1, elite = pl.mu_sigma().cpu().numpy().copy(), np.sort(pl.elite_idx().cpu().numpy())
        pl.plan_end()
        pl.close()
        mu64, sg64, _, _, _ = wc.refit64(case.scores, elite, actions, ms0[0], ms0[1], 0.25, case.tau)
        e_mu = float((np.abs(ms1[0] - mu64) / (wc.MU_ATOL + wc.MU_RTOL * np.abs(mu64))).max())
        e_sg = float((np.abs(ms1[1] - sg64) / (wc.SG_ATOL + wc.SG_RTOL * np.abs(sg64))).max())
        if e_mu > worst['mu']:
            worst['mu'], worst['mu_case'] = e_mu, case.name
        if e_sg > worst['sigma']:
            worst['sigma'], worst['sigma_case'] = e_sg, case.name
    return dict(fraction_of_bar=worst, bars=dict(mu=[wc.MU_RTOL, wc.MU_ATOL], sigma=[wc.SG_RTOL, wc.SG_ATOL]), cases=len(wc.CASES))


def main():
    if '--child' in sys.argv:
        return child()
    plans = int(sys.argv[sys.argv.index('--plans') + 1]) if '--plans' in sys.argv else 40
    rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 3
    legs = []
    for shape in SHAPES:
        for r in range(rounds):                               # the legs alternate inside a round: one machine, one warm clock
            for name, (refit, all_elite) in LEGS.items():
                legs.append(dict(shape=shape, leg=name, round=r, **leg(shape, refit, all_elite, plans, 1)))
    summary = {}
    for s in SHAPES:
        summary[s] = {n: float(np.median([x for l in legs if l['shape'] == s and l['leg'] == n for x in l['ms']])) for n in LEGS}
        summary[s]['round_medians'] = {n: [l['ms_median'] for l in legs if l['shape'] == s and l['leg'] == n] for n in LEGS}
        summary[s]['softmax_minus_uniform'] = summary[s]['softmax'] - summary[s]['uniform']
        summary[s]['softmax_kN_minus_uniform_kN'] = summary[s]['softmax_kN'] - summary[s]['uniform_kN']
        summary[s]['launches_per_iteration'] = {n: next(l['launches_per_iteration'] for l in legs if l['shape'] == s and l['leg'] == n) for n in LEGS}
    doc = dict(plans=plans, rounds=rounds, temperature=TEMPERATURE, ms_median_of_all_plans=summary, legs=legs)
    if '--kernel-stats' in sys.argv:
        doc['kernels_us'] = kernel_stats()
    if '--accuracy' in sys.argv:
        doc['max_error_vs_float64'] = accuracy()
    print(json.dumps(doc))


if __name__ == '__main__':
    main()
