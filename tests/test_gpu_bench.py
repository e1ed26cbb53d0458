"""bench.py's contract on an MI355X: the plain single-process line and its --dump-outputs, the --full line with every extra,
and the multi-rank leg (process group over RCCL, stepwise plan with the score all-gather, barrier + max-over-ranks timing) rehearsed
with one rank under torch.distributed.run — the only rehearsal a single GPU allows (CEM_BENCH_FORCE_DIST=1)."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {'metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype',
        'data', 'config'}
# what only --full measures: a plain run carries none of it
FULL_ONLY = {'roofline', 'configs', 'split_bf16x3', 'cpu_baseline', 'per_rank_single_gpu_b2_plans_per_s', 'b2_strong', 'b5', 'b5_split_bf16x3'}


def _json_line(out):
    lines = [l for l in out.splitlines() if l.startswith('{') and '"metric"' in l]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def _check(r, steps, warmup, full=True):
    assert KEYS <= set(r)
    assert r['metric'] == 'planning steps/sec (CEM-MPC, N=2000 K=5 H=30)' and r['unit'] == 'plans/s' and r['n_gpus'] == 1
    assert r['steps'] == steps and r['warmup'] == warmup and r['higher_is_better'] is True and r['scaling'] == 'weak'
    assert r['dtype'] == 'f32' and r['vs_baseline'] is None and r['data'] == 'synthetic' and 'workload' in r['config']
    assert abs(r['value'] * r['ms_per_step'] / 1e3 - 1.0) < 1e-6 and r['value'] > 100
    if not full:
        assert not FULL_ONLY & set(r), FULL_ONLY & set(r)
        return
    rf = r['roofline']
    assert rf['bound'] == 'mfma' and rf['unit'] == 'TFLOP/s' and abs(rf['frac'] - rf['achieved'] / rf['peak']) < 1e-9
    assert 0.3 < rf['frac'] < 1.0


def test_plain_bench_line_and_outputs(tmp_path):
    """A plain run times exactly the steps asked for and nothing else; --dump-outputs writes what the last timed plan returned, and
    the same arguments give the same outputs bit for bit (seeded inputs, deterministic plan)."""
    dumps = []
    for run in range(2):
        d = str(tmp_path / ('out%d' % run))
        out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '7', '--warmup', '2', '--dump-outputs', d],
                             cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        r = _json_line(out.stdout)
        _check(r, 7, 2, full=False)
        assert len(r['ms_per_step_each']) == 7 and abs(sum(r['ms_per_step_each']) / 7 - r['ms_per_step']) < 0.02 * r['ms_per_step']
        assert r['order'].startswith('headline first') and r['config']['hip_graph'] is True
        got = {n: np.load(os.path.join(d, n + '.npy')) for n in ('action', 'score', 'iterations')}
        assert sorted(os.listdir(d)) == ['action.npy', 'iterations.npy', 'score.npy']
        assert got['action'].dtype == np.float32 and got['action'].shape == (2,) and np.isfinite(got['action']).all()
        assert got['score'].dtype == np.float32 and got['score'].shape == (1,) and np.isfinite(got['score']).all()
        assert got['iterations'].dtype == np.float64 and got['iterations'].tolist() == [5.0]
        dumps.append(got)
    for n in dumps[0]:
        np.testing.assert_array_equal(dumps[0][n], dumps[1][n], err_msg=n)


def test_default_bench_line():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '5', '--warmup', '2', '--no-cpu-baseline', '--full'],
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = _json_line(out.stdout)
    _check(r, 5, 2)
    assert r['config']['hip_graph'] is True and r['config']['launches_per_iteration'] == 2       # rollout + select per CEM iteration at B2
    # the other BASELINE configs ride along as labelled extras (value stays B2): B1, B3, B4 whole plans + one rank of B5's eight
    cf = r['configs']
    policy = {'B2_safe', 'shipped_safe_cem_mpc', 'shipped_safe_cem_mpc_early_stop', 'shipped_cem_mpc', 'shipped_cem_mpc_early_stop'}
    assert set(cf) == {'B1', 'B3', 'B4', 'B5_rank'} | policy and not any('error' in v for v in cf.values()), cf
    # the reference's default policy (config/agents.yaml:11) and its shipped shapes, timed by the driver's own run
    for name in policy:
        c = cf[name]
        assert c['workload'].startswith(name + ':') and c['hip_graph'] is True and abs(c['plans_per_s'] * c['ms_per_plan'] / 1e3 - 1.0) < 1e-6
        assert 0.0 < c['rollout_share_of_plan'] < 1.0 and c['select_us_per_iteration'] > 1.0
        safe = 'safe' in name
        # SafeCemMpc keeps the reduce kernel (Beta filter): 3 launches per iteration, its time reported; CemMpc folds it into the select
        assert c['launches_per_iteration'] == (3 if safe else 2), (name, c['launches_per_iteration'])
        assert (c['reduce_us_per_iteration'] > 0.5) == safe, (name, c['reduce_us_per_iteration'])
        full = {'B2_safe': 5, 'shipped_safe_cem_mpc': 9, 'shipped_cem_mpc': 10}
        if name in full:
            assert c['iterations_run_mean'] == full[name]
        else:
            assert 1 <= c['iterations_run_mean'] <= (9 if safe else 10)
    assert cf['B2_safe']['ms_per_plan'] < 1.25 * r['ms_per_step'], 'SafeCemMpc at the headline shape costs more than 25 % over CemMpc'
    assert r['weak_plans_per_s'] == r['value'] and r['weak_candidates_per_plan'] == 2000 and 'extras_timed_out' not in r
    # the other legs run in front of the headline (sustained clock); every timed step is listed, and none of them is a cold-start outlier
    assert r['order'].startswith('the other legs first') and len(r['ms_per_step_each']) == 5
    assert abs(sum(r['ms_per_step_each']) / 5 - r['ms_per_step']) < 0.02 * r['ms_per_step']        # (the listed steps ARE the timed interval; what they show on a cold / warm GPU: profiles/r05_cold_start_steps.txt)
    rows = {'B1': 5 * 500, 'B3': 16 * 8192, 'B4': 8 * 4096}
    for name in ('B1', 'B3', 'B4'):
        c = cf[name]
        assert c['workload'].startswith(name + ':') and c['hip_graph'] is True and c['tiles'] * c['chunks_per_tile'] * 16 >= rows[name]
        assert abs(c['plans_per_s'] * c['ms_per_plan'] / 1e3 - 1.0) < 1e-6 and c['kernel'].startswith('void cem_rollout_')
        assert abs(c['frac_of_fp32_mfma_peak'] - c['algorithmic_flops_per_launch'] / (c['rollout_ms_per_launch'] * 1e-3) / 157.3e12) < 1e-9
        assert (0.25 if name == 'B1' else 0.5) < c['frac_of_fp32_mfma_peak'] < 1.0 and c['plan_frac_of_fp32_mfma_peak'] < c['frac_of_fp32_mfma_peak']
        assert c['launches_per_iteration'] == (2 if name == 'B1' else 3)      # (B3 / B4: tiles queue for slots — the sampler is a launch of its own)
    assert cf['B5_rank']['candidates_per_rank'] == 8192 and 0.5 < cf['B5_rank']['rollout_frac_of_fp32_mfma_peak_per_rank'] < 1.0


def test_distributed_leg_with_one_rank_over_rccl():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, CEM_BENCH_FORCE_DIST='1')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr',
                          '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '5',
                          '--warmup', '2', '--no-cpu-baseline', '--full'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = _json_line(out.stdout)
    _check(r, 5, 2)
    # the multi-rank leg is the library's own: RCCL all-gather inside the captured per-rank graph
    assert r['config']['hip_graph'] is True and 'ncclAllGather' in r['config']['exchange']


def test_distributed_leg_host_stepped_fallback():
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, CEM_BENCH_FORCE_DIST='1', CEM_BENCH_PYTHON_EXCHANGE='1')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr',
                          '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '5',
                          '--warmup', '2', '--no-cpu-baseline', '--full'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    r = _json_line(out.stdout)
    _check(r, 5, 2)
    assert r['config']['hip_graph'] is False and 'torch.distributed' in r['config']['exchange']


def test_b5_leg_rehearsed_as_one_rank_of_eight():
    """BASELINE config 5 in bench.py's multi-GPU leg (N = 65536, k = 6554, 65536/G candidates per rank), rehearsed on one GPU:
    the process plays rank 0 of 8 (8192 candidates, the replicated sample and select over all 65536 scores, the all-gather
    replaced by a device copy of its shard) under torch.distributed.run with the headline's distributed leg alongside."""
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, CEM_BENCH_FORCE_DIST='1', CEM_BENCH_B5_REHEARSAL='8')
    out = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '1', '--master-addr',
                          '127.0.0.1', '--master-port', str(port), os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '5',
                          '--warmup', '2', '--no-cpu-baseline', '--full'], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    r = _json_line(out.stdout)
    _check(r, 5, 2)
    # the literal metric, strong-scaled: N = 2000 candidates in total, 250 on this rank of eight, plain plans/s
    b2s = r['b2_strong']
    assert b2s['n_ranks'] == 8 and b2s['candidates_per_rank'] == 250 and b2s['scaling'] == 'strong' and b2s['unit'] == 'plans/s' and 'N=2000' in b2s['workload']
    assert abs(b2s['plans_per_s'] * b2s['ms_per_plan'] / 1e3 - 1.0) < 1e-6 and b2s['plans_per_s'] > 200
    b5 = r['b5']
    assert b5['n_ranks'] == 8 and b5['candidates_per_rank'] == 8192 and b5['scaling'] == 'strong' and 'N=65536' in b5['workload']
    assert b5['tiles'] * b5['chunks_per_tile'] * 16 == 5 * 8192 and 'rehearsal' in b5['exchange']
    assert abs(b5['plans_per_s'] * b5['ms_per_plan'] / 1e3 - 1.0) < 1e-6 and b5['plans_per_s'] > 50
    assert 0.5 < b5['rollout_frac_of_fp32_mfma_peak_per_rank'] < 1.0 and 20 < b5['select_us_per_iteration'] < 400
    assert b5['rollout_kernel'].startswith('void cem_rollout_')
