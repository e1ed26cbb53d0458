"""Shared by tests/test_bf16_fuzz_cpu.py and tests/test_gpu_bf16_fuzz.py: random shapes for the precision='bf16' rollout — the recipe of
tests/test_gpu_fuzz.py restricted to what the kernel takes (units <= 128, relu, no floating segments), on seed bases of its own so that
no existing case changes — their references, and the COMMITTED TABLES of seeds the GPU tests run.

Why tables and not whatever the generator yields: the bars of tests/bf16_cases.py compare the kernel with the emulation in units of the
emulation's own distance to the fp64 oracle, and on a small population one candidate whose score a bf16 tie moved can put the
fp32-accumulating stand-in itself over RATIO (about 2 % of random cases).  tests/test_bf16_fuzz_cpu.py admits a seed only if
  * cem_plan_tiles_host accepts its configuration,
  * at most NEAR_CAP of its candidates sit on a threshold and at least Y_MIN are flip-free,
  * the stand-in passes every bar under ALL 24 visiting orders of the four chunks, and under the fine-grained sums of bf16_cases.FINE,
    with every ratio at most RATIO / 2 (the device's ties fall yet another way: the factor of two is its headroom), and
  * every mutant of bf16_cases.MUTANTS fails (scores: all but the variance-head one),
and asserts that the tables cover every depth, tile size, input width class and option the kernel has a path for.
A screened seed that fails on the GPU is a finding about the kernel.  A seed is dropped only if a CPU summation order reproduces the
excess; dropped seeds and the reason are recorded in DROPPED."""
import functools

import numpy as np

from oracle import cem_oracle as o
from tests import bf16_cases as bc
from tests import helpers as hp

F32 = np.float32
UNITS = [16, 17, 32, 33, 48, 64, 100, 127, 128]
OBS = [5, 9, 17, 26, 28, 31, 40, 58, 60, 62, 63, 70, 97, 110, 122]   # with A in 1..6: obs + act at 32, 33, 64, 65, 128 and in between

SCORE_SEEDS = (2, 9, 12, 18, 24, 29, 36, 40, 44, 52, 57, 58, 60, 65, 67, 74, 76, 79, 83, 84, 91, 100, 121, 143, 146, 148, 149, 155, 158, 160, 161, 169)
UNFOLD_SEEDS = (3, 6, 11, 13, 17, 21, 22, 26, 30, 31, 34, 36, 38, 46, 48, 52)
CUT_SEEDS = (0, 2, 4, 5, 10, 13, 14, 15, 19, 24, 29, 291)      # (5 and 291: a shard with a one-row tile)
DROPPED = {                                                   # (table, seed) -> reason (see the module docstring)
    ('unfold', 12): 'O 63, A 2, E 5, L 3, B 170, H 6, units 32: on the device mu sat at 0.056 of the yardstick at step 3 (RMS(kernel - emulation) '
                    '2.16e-6 against 3.84e-5; 3e-10 at steps 0 - 2, 3.5e-10 at step 4, 1.3e-6 at step 5) — ONE hidden activation of one row on the '
                    'other side of a bf16 tie, in a 32-unit network where one unit moves every output.  None of the 24 chunk orders puts it '
                    'there (the seed was admitted under them at RATIO / 2); a float32 rounding after every product does (emu32 group = 1), '
                    'with the same figures step for step, k descending 2.2e-6 and 1.3e-6 as on the device '
                    '(test_the_dropped_seed_is_reproduced_by_a_cpu_summation_order).  The FINE stand-ins joined the screening for it.',
}


# ---- D.1 scores ----------------------------------------------------------------------------------------------------------------------
def score_params(seed):
    rng = np.random.default_rng(21000 + seed)
    A = int(rng.integers(1, 7))
    O = min(int(rng.choice(OBS)), 128 - A)
    E = int(rng.integers(1, 7))
    per = int(rng.integers(1, 4))                             # particles per member, or members per particle
    if rng.random() < 0.5:
        P, N = E * per, int(rng.integers(24, 160))            # whole particles per member
    else:
        P = int(rng.integers(1, 5))                           # members split particles: P * N must divide by E
        N = E * max(int(rng.integers(5, 40)), -(-24 // E))       # (at least 24 candidates: a quantile over fewer means little)
    if rng.random() < 0.35:                                   # the next population, if there is one, with P N / E = 1 (mod 16)
        for n in range(max(N, 24), max(N, 24) + 16 * E + 1):
            if (P * n) % E == 0 and (P * n // E) % 16 == 1:
                N = n
                break
    c = dict(O=O, A=A, E=E, P=P, N=N, H=int(rng.integers(1, 11)), L=int(rng.integers(1, 6)), units=int(rng.choice(UNITS)),
             variant=str(rng.choice(['cem', 'safe'])), rc=int(rng.integers(0, 5)), sampling=bool(rng.random() < 0.8), scale=bool(rng.random() < 0.8),
             post=float(rng.choice([0.15, 0.3, 0.5])))
    c['box'], c['low'], c['high'] = hp.random_action_bounds(rng, A)
    return c


def score_configs(seed):
    """(case dict, problem, oracle config, planner config) of a score seed"""
    c = score_params(seed)
    pb = hp.with_action_bounds(hp.make_problem(c['O'], c['A'], c['E'], c['L'], seed=700 + seed, units=c['units']), c['low'], c['high'])
    ocfg, pcfg = hp.configs(pb, N=c['N'], H=c['H'], P=c['P'], E=c['E'], k=max(1, c['N'] // 10), I=1, variant=c['variant'], post=c['post'],
                            sampling=c['sampling'], scale=c['scale'], chunks_per_tile=c['rc'], precision='bf16')
    return c, pb, ocfg, pcfg


@functools.lru_cache(maxsize=None)
def score_case(seed):
    """bf16_cases.score_case's dict for a score seed, with the case dict (`c`) and the planner configuration (`pcfg`)"""
    c, pb, ocfg, pcfg = score_configs(seed)
    ea, em, _ = hp.noise(1, c['N'], c['H'], c['A'], c['P'], c['O'], seed=seed)
    return dict(bc._score_case(pb, ea, em, ocfg), c=c, pcfg=pcfg)


def tiles_of(pcfg):
    """(status, tile size, rows of every tile) from cem_plan_tiles_host — no device needed"""
    import ctypes as C
    from ethz_safe_learning_amd import _capi, planner
    lib = _capi.load()
    cc = planner.to_c_config(pcfg)
    rc, nt = C.c_int32(), C.c_int32()
    st = lib.cem_plan_tiles_host(C.byref(cc), C.byref(rc), C.byref(nt), None, 0)
    if st:
        return st, 0, np.zeros(0, np.int32)
    rc, tiles = planner.plan_tiles(pcfg)
    return 0, rc, tiles[:, 1]


def screen_score(seed):
    """The admission conditions of a score seed (module docstring), asserted.  Returns the facts the coverage check reads and the
    largest ratios seen: dict(c, rc, one_row_tail, worst = (RMS, median, 90th percentile ratio over the 24 orders), caught = {mutant: bar})"""
    c, pb, ocfg, pcfg = score_configs(seed)
    what = 'score seed %d %s' % (seed, {k: v for k, v in c.items() if k not in ('low', 'high')})
    st, rc, cnt = tiles_of(pcfg)
    assert st == 0, '%s: cem_plan_tiles_host status %d' % (what, st)
    ref = score_case(seed)
    worst = np.zeros(3)
    for name, forward in bc.stand_ins().items():
        r = bc.check_scores(bc.scores_under(ref, forward), ref, '%s %s' % (what, name), bc.RATIO / 2)
        worst = np.maximum(worst, (r[0], r[2], r[3]))
    caught = {}
    for kind in bc.MUTANTS:
        if kind not in bc.SCORE_BLIND:
            caught[kind] = bc.failed_score_bars(bc.scores_under(ref, bc.mutant(kind)), ref)
            assert caught[kind], '%s: the %s mutant passes every bar of the score check' % (what, kind)
    return dict(c=c, rc=rc, one_row_tail=bool((cnt == 1).any()), worst=tuple(worst), caught=caught)


# ---- D.2 unfold with moments ------------------------------------------------------------------------------------------------------------
def unfold_params(seed):
    rng = np.random.default_rng(27000 + seed)
    A = int(rng.integers(1, 9))
    O = min(int(rng.choice(OBS)), 128 - A)
    E = int(rng.integers(1, 7))
    return dict(O=O, A=A, E=E, L=int(rng.integers(1, 6)), B=E * int(rng.integers(1, 41)), H=int(rng.integers(1, 9)), units=int(rng.choice(UNITS)),
                sampling=bool(rng.random() < 0.8), scale=bool(rng.random() < 0.8))


@functools.lru_cache(maxsize=None)
def unfold_case(seed):
    """dict(c, pb, pcfg, s0, acts, eps, emu = (traj, mu, sd) under the emulation, ref64 = the same of the fp64 oracle)"""
    c = unfold_params(seed)
    O, A, E, B, H = c['O'], c['A'], c['E'], c['B'], c['H']
    pb = hp.make_problem(O, A, E, c['L'], seed=800 + seed, units=c['units'])
    _, pcfg = hp.configs(pb, N=max(B // E, 1), H=H, P=E, E=E, k=1, I=1, sampling=c['sampling'], scale=c['scale'], precision='bf16')
    rng = np.random.default_rng(seed)
    s0 = (pb['state'][None, :] + 0.05 * rng.standard_normal((B, O))).astype(F32)
    acts = rng.uniform(-1, 1, (B, H, A)).astype(F32)
    eps = rng.standard_normal((H, B, O)).astype(F32)
    args = (s0.astype(np.float64), acts.astype(np.float64), o.cast_weights(pb['weights'], np.float64), o.member_of_rows(B, E), pb['inputs_min'], pb['inputs_max'],
            eps.astype(np.float64), c['scale'], c['sampling'])
    ref64 = bc.unfold_with_moments(*args)
    with bc.emulating(bc.emu64):
        emu = bc.unfold_with_moments(*args)
    return dict(c=c, pb=pb, pcfg=pcfg, s0=s0, acts=acts, eps=eps, emu=emu, ref64=ref64)


def unfold_under(u, forward):
    """(traj, mu, sd) `forward` gives in the kernel's place: float32 throughout"""
    c, pb = u['c'], u['pb']
    with bc.emulating(forward):
        return bc.unfold_with_moments(u['s0'], u['acts'], pb['weights'], o.member_of_rows(c['B'], c['E']), pb['inputs_min'], pb['inputs_max'], u['eps'],
                                      c['scale'], c['sampling'])


def check_unfold(got, u, what, ratio=bc.RATIO):
    """The rounding model on the trajectory and on the heads' moments, and the start states handed through untouched.  Returns the
    largest RMS ratio of each of the three."""
    traj, mu, sd = (np.asarray(x) for x in got)
    np.testing.assert_array_equal(traj[:, 0], u['s0'], err_msg=what)
    return tuple(max(bc.check_rounding_model(g, e, r, '%s %s' % (what, name), ratio))
                 for name, g, e, r in zip(('trajectory', 'mu', 'sd'), (traj, mu, sd), u['emu'], u['ref64']))


def screen_unfold(seed):
    """The admission conditions of an unfold seed: the configuration accepted, the stand-in within RATIO / 2 under all 24 orders on
    trajectory, mu and sd, and EVERY mutant caught (the variance-head one by sd).  Returns dict(c, worst = (trajectory, mu, sd ratio),
    caught = {mutant: which of trajectory / mu / sd})"""
    u = unfold_case(seed)
    what = 'unfold seed %d %s' % (seed, u['c'])
    st, _, _ = tiles_of(u['pcfg'])
    assert st == 0, '%s: cem_plan_tiles_host status %d' % (what, st)
    worst = np.zeros(3)
    for name, forward in bc.stand_ins().items():
        worst = np.maximum(worst, check_unfold(unfold_under(u, forward), u, '%s %s' % (what, name), bc.RATIO / 2))
    caught = {}
    for kind in bc.MUTANTS:
        try:
            check_unfold(unfold_under(u, bc.mutant(kind)), u, what)
            caught[kind] = ''
        except AssertionError as e:
            caught[kind] = next((n for n in ('trajectory', 'mu', 'sd') if (what + ' ' + n) in str(e)), 'other')
        assert caught[kind], '%s: the %s mutant passes the rounding model on trajectory, mu and sd' % (what, kind)
    return dict(c=u['c'], worst=tuple(worst), caught=caught)


# ---- D.3 cutting invariance --------------------------------------------------------------------------------------------------------------
def cut_params(seed):
    rng = np.random.default_rng(33000 + seed)
    W = int(rng.choice([2, 3, 4]))
    E = int(rng.integers(1, 6))
    P = E * int(rng.integers(1, 3)) if rng.random() < 0.6 else int(rng.integers(1, 5))
    per = int(rng.integers(1, 60))
    N = W * per
    if (P * N) % E:
        N = W * per * E
    A = int(rng.integers(1, 4))
    O = int(rng.choice([9, 28, 40, 60, 62, 100]))
    rc_full = int(rng.integers(0, 5))
    c = dict(W=W, E=E, P=P, N=N, O=O, A=A, H=int(rng.integers(1, 9)), L=int(rng.integers(1, 6)), variant=str(rng.choice(['cem', 'safe'])),
             rc_full=rc_full, rc_shard=(rc_full + int(rng.integers(1, 5))) % 5, units=int(rng.choice(UNITS)))
    c['box'], c['low'], c['high'] = hp.random_action_bounds(rng, A)
    return c


def cut_configs(seed):
    """(case dict, problem, {(world, rank): planner config}) — the single rank at rc_full, and every rank of the world of W at rc_shard"""
    c = cut_params(seed)
    pb = hp.with_action_bounds(hp.make_problem(c['O'], c['A'], c['E'], c['L'], seed=900 + seed, units=c['units']), c['low'], c['high'])
    cfgs = {}
    for world, rank, rc in [(1, 0, c['rc_full'])] + [(c['W'], r, c['rc_shard']) for r in range(c['W'])]:
        cfgs[world, rank] = hp.configs(pb, N=c['N'], H=c['H'], P=c['P'], E=c['E'], k=max(1, c['N'] // 10), I=1, variant=c['variant'], post=0.3,
                                       world_size=world, rank=rank, chunks_per_tile=rc, precision='bf16')[1]
    return c, pb, cfgs
