#!/usr/bin/env python3
"""Same-box A/B of library builds: MI355X devices differ by up to ~12 % in wall time, so variants are only comparable
inside one run on one device.  usage: ab_bench.py lib1.so lib2.so ... [--rounds R] [--chunks C]
A variant may also be a DIRECTORY: a checkout of another commit with its own built library (e.g. `git archive` of the parent under
build_ab/), whose bench.py is run there with its own binding — what a build needs whose exported symbols differ from this tree's."""
import json, os, subprocess, sys
libs = [a for a in sys.argv[1:] if a.endswith('.so') or os.path.isfile(os.path.join(a, 'bench.py'))]
rounds = int(sys.argv[sys.argv.index('--rounds') + 1]) if '--rounds' in sys.argv else 2
chunks = sys.argv[sys.argv.index('--chunks') + 1] if '--chunks' in sys.argv else '0'
steps = sys.argv[sys.argv.index('--steps') + 1] if '--steps' in sys.argv else '100'
res = {l: [] for l in libs}
for r in range(rounds):
    for l in libs:
        tree = os.path.isdir(l)
        env = dict(os.environ) if tree else dict(os.environ, CEM_MPC_LIB=os.path.abspath(l))
        if tree:
            env.pop('CEM_MPC_LIB', None)
        out = subprocess.run([sys.executable, 'bench.py', '--steps', steps, '--warmup', '15', '--full', '--no-cpu-baseline', '--no-split-leg', '--no-configs', '--chunks', chunks],
                             env=env, cwd=l if tree else None, capture_output=True, text=True).stdout.strip().splitlines()
        d = json.loads(out[-1])
        res[l].append((d['roofline']['avg_launch_ms'], d['value'], d['ms_per_step_median']))
for l in libs:
    print('%-40s rollout ms %s   plans/s %s   median plan ms %s' % (os.path.basename(os.path.normpath(l)), ' '.join('%.4f' % a for a, _, _ in res[l]), ' '.join('%.1f' % b for _, b, _ in res[l]),
                                                                       ' '.join('%.4f' % c for _, _, c in res[l])), flush=True)
