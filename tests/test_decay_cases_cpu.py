"""Population schedule and mean candidate on the host: planner.population_schedule's known answers and refusals, planner.mean_candidate
on hand-made inputs, and tests/decay_cases.py itself — every schedule admissible, every iteration's tile plan a partition of its rows
with the member map of the n[it]-wide configuration, the oracle seeds' gaps recomputed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from ethz_safe_learning_amd.planner import mean_candidate, population_schedule
from tests import decay_cases as dc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, U = np.float32, np.uint32


def test_population_schedule_known_answers():
    assert population_schedule(2000, 200, 5, 1.25, 5, 5) == [2000, 1600, 1280, 1024, 820]
    assert population_schedule(150, 15, 10, 1.25, 5, 5) == [150, 120, 96, 77, 62, 50, 40, 32, 30, 30]
    assert population_schedule(66, 8, 3, 1.5, 2, 3) == [66, 45, 30]
    assert population_schedule(64, 8, 4, 1.0, 5, 5) == [64] * 4                           # decay 1: off
    assert population_schedule(64, 8, 4, 2.0, 5, 5, min_population=8) == [64, 32, 16, 8]
    assert population_schedule(64, 8, 4, 2.0, 5, 5, min_population=3) == [64, 32, 16, 8]  # never below n_elite
    assert population_schedule(64, 40, 3, 2.0, 5, 5) == [64, 64, 64]                      # the floor 2 k is capped at n_samples
    for args in [(2000, 200, 5, 1.25, 5, 5), (150, 15, 10, 1.25, 5, 5), (66, 8, 3, 1.5, 2, 3), (500, 20, 6, 1.3, 45, 15), (102, 7, 8, 3.0, 4, 6)]:
        N, k, I, g, P, E = args
        s = population_schedule(*args)
        assert len(s) == I and s[0] == N and all(k <= n <= N and (P * n) % E == 0 for n in s), (args, s)
        assert all(a >= b for a, b in zip(s, s[1:])), (args, s)


@pytest.mark.parametrize('decay', [0.99, 0.0, -1.25, float('nan'), float('inf')])
def test_population_schedule_refuses_a_decay_below_one_or_not_finite(decay):
    with pytest.raises(ValueError):
        population_schedule(64, 8, 3, decay, 5, 5)


def test_population_schedule_refuses_shapes_that_are_none():
    for args in [(8, 9, 3, 1.25, 5, 5), (64, 8, 0, 1.25, 5, 5), (64, 0, 3, 1.25, 5, 5)]:
        with pytest.raises(ValueError):
            population_schedule(*args)
    with pytest.raises(ValueError):
        population_schedule(64, 8, 3, 1.25, 5, 5, min_population=0)


def test_mean_candidate_on_hand_made_inputs():
    acts = np.arange(3 * 2 * 3, dtype=F).reshape(3, 2, 3) / F(7)
    mu = np.array([[-2.0, 0.25, 3.0], [0.5, -0.75, -0.0]], F)                           # outside the box below and above, inside, a signed zero
    lb, ub = np.array([-1.0, -0.5, -1.0], F), np.array([1.0, 0.5, 2.5], F)
    out = mean_candidate(acts, mu, lb, ub)
    assert out.dtype == F and out is not acts
    np.testing.assert_array_equal(out[:2].view(U), acts[:2].view(U))                      # every other row is the sampler's, bit for bit
    np.testing.assert_array_equal(out[2], np.array([[-1.0, 0.25, 2.5], [0.5, -0.5, -0.0]], F))
    assert np.signbit(out[2, 1, 2])
    np.testing.assert_array_equal(acts, np.arange(18, dtype=F).reshape(3, 2, 3) / F(7))   # the input is left alone
    one = mean_candidate(acts[:1], mu, lb, ub)                                            # a population of one: the row IS the mean
    np.testing.assert_array_equal(one[0], out[2])


def test_every_case_is_admissible_and_named_once():
    assert [c.name for c in dc.CASES] == ['lean', 'ragged', 'to_k', 'grow', 'split_members', 'segments', 'two_blocks_safe', 'cost', 'wide256',
                                          'bf16x3']
    for c in dc.CASES:
        assert dc.admissible(c), c.name
        assert any(n != c.N for n in c.schedule), c.name                                  # (all-N would be OFF)
    assert dc.BY_NAME['ragged'].schedule == (64, 37, 21) and all(n % 16 for n in dc.BY_NAME['ragged'].schedule[1:])
    assert dc.BY_NAME['to_k'].schedule[-1] == dc.BY_NAME['to_k'].k
    g = dc.BY_NAME['grow'].schedule
    assert g[0] < g[1] > g[2]
    assert population_schedule(66, 8, 3, 1.5, 2, 3) == list(dc.BY_NAME['split_members'].schedule)


_TILE_CODE = r'''
import json, sys
sys.path.insert(0, %r)
from tests import decay_cases as dc, helpers as hp
from ethz_safe_learning_amd.planner import plan_tiles, plan_segments
out = {}
for c in dc.CASES:
    pb = dc.problem(c)
    rows = []
    for n in c.schedule:
        _, pcfg = hp.configs(pb, **dc.config_kwargs(c, N=n))
        rc, tiles = plan_tiles(pcfg)
        rows.append(dict(n=n, rc=rc, tiles=tiles.tolist(), segments=plan_segments(pcfg)[0]))
    out[c.name] = rows
print(json.dumps(out))
'''


@pytest.fixture(scope='module')
def tile_plans(built_lib):
    """{case: [per iteration dict(n, rc, tiles, segments)]} from cem_plan_tiles_host on the configuration with n_samples = n[it], priced
    for 256 CUs whatever this host has (CEM_ASSUME_CUS is read once per process: a child process)."""
    r = subprocess.run([sys.executable, '-c', _TILE_CODE % ROOT], env=dict(os.environ, CEM_ASSUME_CUS='256'), capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize('case', dc.CASES, ids=[c.name for c in dc.CASES])
def test_every_iteration_has_the_tile_plan_of_its_own_population(case, tile_plans):
    """Each iteration's tiles partition the P n[it] rows; a tile lies inside ONE member of the n[it]-wide map (p n + j) / (P n / E), holds
    at most 16 rc rows, and names the global row its model noise is keyed on."""
    plans = tile_plans[case.name]
    assert [p['n'] for p in plans] == list(case.schedule)
    for p in plans:
        n, rc = p['n'], p['rc']
        chunk = case.P * n // case.E
        seen = np.zeros(case.P * n, np.int32)
        assert 1 <= rc <= 4 and (case.rc == 0 or rc == case.rc) and (case.units <= 128 or rc == 1)
        for row_base, cnt, member, cand, grow, _ in p['tiles']:
            assert 1 <= cnt <= 16 * rc
            part, j = divmod(row_base, n)
            assert cand == j and grow == part * n + j == row_base and j + cnt <= n           # one rank: local row == global row
            assert grow // chunk == member == (grow + cnt - 1) // chunk, (case.name, n, row_base)
            seen[row_base:row_base + cnt] += 1
        assert (seen == 1).all(), (case.name, n)
        if case.segments:
            assert p['segments'] == case.segments
    if case.name == 'split_members':
        # the member boundaries fall inside particles, at another candidate index for every population
        cuts = [sorted({t[3] for t in p['tiles'] if t[3] != 0}) for p in plans]
        assert all(cuts) and len({tuple(c) for c in cuts}) == len(cuts), cuts
    if case.name == 'lean':
        assert all(p['rc'] == 1 for p in plans)


@pytest.mark.parametrize('case,seed', dc.ORACLE_CASES, ids=['%s_%d' % (c.name, s) for c, s in dc.ORACLE_CASES])
def test_oracle_seeds_have_a_clear_cut_in_every_iteration(case, seed):
    for with_mean in (False, True):
        _, score, iters, trace = dc.oracle_plan(case, seed, with_mean=with_mean)
        assert iters == dc.I and np.isfinite(score)
        assert [t['scores'].shape[0] for t in trace] == list(case.schedule)
        gaps = dc.oracle_gaps(trace, case.k)
        assert min(gaps) > dc.ORACLE_GAP, (case.name, seed, with_mean, gaps)


def test_the_cases_cover_what_they_are_for():
    assert {c.name for c, _ in dc.ORACLE_CASES} >= {'lean', 'ragged', 'to_k', 'grow', 'split_members', 'segments', 'two_blocks_safe'}
    assert dc.BY_NAME['lean'].lean and dc.BY_NAME['lean'].obs % 4 == 0 and dc.BY_NAME['lean'].rc == 1
    assert dc.BY_NAME['two_blocks_safe'].obs + dc.BY_NAME['two_blocks_safe'].act > 64 and dc.BY_NAME['two_blocks_safe'].variant == 'safe'
    assert dc.BY_NAME['wide256'].units == 256 and dc.BY_NAME['bf16x3'].precision == 'bf16x3' and dc.BY_NAME['cost'].variant == 'cost'
    c = dc.BY_NAME['ragged']
    ea = np.arange(dc.I * c.N * c.H * c.act, dtype=F).reshape(dc.I, c.N, c.H, c.act)
    em = np.arange(dc.I * c.H * c.P * c.N * c.obs, dtype=F).reshape(dc.I, c.H, c.P * c.N, c.obs)
    a, m = dc.cut_noise(c, ea, em, 1)
    n = c.schedule[1]
    assert a.shape == (n, c.H, c.act) and m.shape == (c.H, c.P * n, c.obs)
    assert a[0, 0, 0] == ea[1, 0, 0, 0] and m[0, 0, 0] == em[1, 0, 0, 0]
    # the model noise is the LEADING floats of the slab re-read with the narrower row count, not the leading rows of every step
    assert m[1, 0, 0] == em[1].reshape(-1)[c.P * n * c.obs] and m[1, 0, 0] != em[1, 1, 0, 0]
