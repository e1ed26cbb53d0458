"""Option combinations of a planner handle: the generated case table tests/test_gpu_option_fuzz.py runs on the device and
tests/test_composed_cases_cpu.py checks on the host, the rules a combination must meet, and ONE composed restatement of a plan with any
admitted set of options on.  Plain data and NumPy; importable without a GPU or torch.

The ten options: tail (lower-tail objective), budget (cost budget), softmax (weighted refit), mixed (time-correlated action noise), carry
(elite carry-over, inside a plan and across plans), sched (population schedule), mean (the mean candidate), track (plan read-out), task (a
task scorer), warm (warm start).  Each has a restatement of its own in ethz_safe_learning_amd.planner or a *_cases.py file; `Reference`
only CALLS those, in the order the host path launches the kernels:
    sample -> inject -> mean row -> rollout -> task score -> score -> select -> refit -> keep -> track
Every stage function takes the inputs of that stage, so the device test can hand in the device's OWN values (teacher forcing) and a near-tie
never excuses a mismatch; `replay` chains the same stages on the fp32 oracle's values.

case_for(seed): seeds 0 .. 43 force one of the 44 option pairs (all pairs but tail x budget, which admit() refuses) and draw every other
option with probability 0.3; seeds 44 .. 47 switch on everything that can be on at once, on a cem handle (tail), a safe handle (budget), a
cost handle and a bf16 handle.  Shapes are the smallest at which the code paths still differ: N 24 .. 96 with ragged schedules (no multiple of
the 16-row chunk) and schedules that end at n = k, H 2 .. 6, I 2 .. 4, A 1 .. 6 (one and two action quads), O in 9 / 12 / 31 / 60 / 70, E 1 .. 4,
P <= 6, units 32 / 64 (160, the wide family, on a few seeds), rollout_segments 0 / 2, and every fourth seed the lean-eligible shape (obs 12 /
act 2, depth 4, one chunk per tile: the handle leaves the lean path for the options that rewrite the sample and comes back)."""
import collections
import dataclasses
import itertools

import numpy as np

from ethz_safe_learning_amd.planner import (empty_readout, inject_elites, keep_elites, mean_candidate, mix_noise, mixing_matrix,
                                            shift_distribution, softmax_refit, task_objective, track_best, warm_sigma_floor)
from tests import constrained_cases as kc
from tests import cost_cases
from tests import elite_cases as ec
from tests import helpers as hp
from tests import readout_cases as rdc
from tests import risk_cases as rk
from tests import task_cases as tc
from tests import weighted_cases as wc

F, U = np.float32, np.uint32
OPTIONS = ('tail', 'budget', 'softmax', 'mixed', 'carry', 'sched', 'mean', 'track', 'task', 'warm')
PAIRS = [p for p in itertools.combinations(OPTIONS, 2) if p != ('tail', 'budget')]
assert len(PAIRS) == 44
N_SEEDS = len(PAIRS) + 4
EVERYTHING = ('cem', 'safe', 'cost', 'bf16')          # seeds 44 .. 47
POST = 0.3
PLAN_SEED, PLAN_CALL = 5, 3
# the kernel capacities admit() reads (csrc/cem_plan_options.h HandleFacts), by the names the other case files give them
TAIL_MAX_P = rdc.MAX_P                                # csrc/cem_score.h CEM_TAIL_MAX_P = CEM_BUDGET_MAX_TAIL_P = CEM_READOUT_MAX_P
ELITE_MAX_K = ec.ELITE_MAX_K
READOUT_MAX_P = rdc.MAX_P
MIX_MAX_H = 128                                       # csrc/cem_noise_mix.h CEM_MIX_MAX_H
MAX_COST_KINDS = 4                                    # include/cem_mpc.h CEM_MAX_COST_KINDS
BUDGET_TOTAL_LIMIT = kc.TWO23                         # csrc/cem_capi.hip kBudgetTotalLimit

Keep = collections.namedtuple('Keep', 'm across shift')
Warm = collections.namedtuple('Warm', 'shift tail sigma floor_frac')
Options = collections.namedtuple('Options', 'tail_m cost_m budget tau noise keep schedule mean readout task warm')
NOTHING = Options(0, 0, float('inf'), 0.0, None, None, None, False, False, None, None)
_Case = collections.namedtuple('_Case', 'name O A H N P E k I units depth variant precision smoothing thr out_noise box low high segments rc '
                                        'pseed opt')


class Case(_Case):
    """One handle and its options.  low / high None: the synthetic problem's own action Box."""
    __slots__ = ()
    obs = property(lambda s: s.O)                     # (the names the other case tables use: helpers.Arrays reads them)
    act = property(lambda s: s.A)


def on(case):
    """The names of the options the case switches on."""
    o = case.opt
    flags = dict(tail=o.tail_m != 0, budget=o.cost_m != 0, softmax=o.tau > 0, mixed=o.noise is not None, carry=o.keep is not None,
                 sched=o.schedule is not None, mean=bool(o.mean), track=bool(o.readout), task=o.task is not None, warm=o.warm is not None)
    return frozenset(k for k, v in flags.items() if v)


def populations(case):
    """n[it] of every iteration."""
    return tuple(case.opt.schedule) if case.opt.schedule is not None else (case.N,) * case.I


def lean_eligible(case):
    """Whether a handle of the shape, with nothing on, rolls out on the lean kernels (cem_capi.hip lean_eligible): the one-chunk fp32 kernel
    of the obs + act <= 64 family, four layers, every feature quad all-observation or all-action."""
    return (case.precision == 'fp32' and case.units <= 128 and case.rc == 1 and case.O + case.A <= 64 and case.depth == 4 and case.O % 4 == 0)


def generic_forced(case, it):
    """Whether iteration `it` must report the generic rollout path (cem_capi.hip recipe_of): carry, the mean candidate in the iteration it
    is written in, mixed noise or a task rewrite or replace the sample the lean kernels would draw in place."""
    o = case.opt
    return o.keep is not None or (o.mean and it == case.I - 1) or o.noise is not None or o.task is not None


def admitted(case):
    """admit() of csrc/cem_plan_options.h as far as a single-rank, single-state handle on the one-workgroup select can reach it, together
    with the setters' own argument checks (include/cem_mpc.h)."""
    o, n = case.opt, populations(case)
    if len(n) != case.I or (case.P * case.N) % case.E or not 1 <= case.k <= case.N:
        return False
    if any(not case.k <= x <= case.N or (case.P * x) % case.E for x in n):
        return False
    if o.schedule is not None and all(x == case.N for x in n):
        return False                                                      # (all N: the setter takes it as "off")
    if o.tail_m and o.cost_m:
        return False                                                      # ONE m
    if o.cost_m and case.variant != 'safe':
        return False
    if o.tail_m and case.variant == 'cost':
        return False
    if o.tail_m and (not 1 <= o.tail_m <= case.P or case.P > TAIL_MAX_P):
        return False
    if o.cost_m and (not 1 <= o.cost_m <= case.P or (o.cost_m < case.P and case.P > TAIL_MAX_P)
                     or case.H * o.cost_m * MAX_COST_KINDS >= BUDGET_TOTAL_LIMIT):
        return False
    if o.noise is not None and case.H > MIX_MAX_H:
        return False
    if o.readout and case.P > READOUT_MAX_P:
        return False
    if o.keep is not None:
        m, across, shift = o.keep
        if not 1 <= m <= case.k or case.k > ELITE_MAX_K or any(x <= m for x in n):
            return False
        if o.mean and m >= n[-1] - 1:
            return False
        if across and (case.H < 2 or not 1 <= shift < case.H):
            return False
    if o.warm is not None and (case.H < 2 or not 1 <= o.warm.shift < case.H):
        return False
    return True


# ---- the generator --------------------------------------------------------------------------------------------------------------------
def _schedule(rng, kind, N, k, I, q, floor):
    """I sizes in max(k, floor) .. N, each a multiple of q (so that P n splits among the members).  kind 'ragged': at least one is no
    multiple of 16; 'to_k': the last one is k; 'grow': not monotone; 'plain': whatever comes."""
    lo = max(k, floor)

    def snap(x):
        return min(N, max(-(-lo // q) * q, -(-int(x) // q) * q))
    out = [N] + [snap(rng.integers(lo, N + 1)) for _ in range(I - 1)]
    if kind != 'grow':
        out = sorted(out, reverse=True)
    else:
        out[0], out[1] = snap(lo + (N - lo) // 3), N
    if kind == 'to_k':
        out[-1] = k
    if kind == 'ragged':
        ragged = [x for x in range(lo, N) if x % q == 0 and x % 16]
        if ragged:
            out[-1] = int(rng.choice(ragged))
    return tuple(int(x) for x in out)


def _draw(seed, rng, forced, everything):
    lean = everything is None and seed % 4 == 0
    wide = everything is None and seed % 11 == 5 and not lean
    A = 2 if lean else int(rng.integers(1, 7))
    O = 12 if lean else int(rng.choice([9, 12, 31, 60, 70]))
    E = int(rng.integers(1, 5))
    if rng.random() < 0.6:
        P, q = E * int(rng.integers(1, max(1, 6 // E) + 1)), 1                  # whole particles per member
    else:
        P = int(rng.integers(1, 5))                                             # members split particles: P n must divide by E
        q = E // int(np.gcd(P, E))
    N = -(-int(rng.integers(24, 97)) // q) * q
    if lean:
        N = min(96, -(-N // (16 * q)) * 16 * q) if 16 * q <= 96 else N
    N = min(N, 96 // q * q)
    k = int(rng.choice([2, 3, max(2, N // 10), max(2, N // 4)]))
    k = min(N, -(-k // q) * q)
    H, I = int(rng.integers(2, 7)), int(rng.integers(2, 5))
    units = 160 if wide else int(rng.choice([32, 64]))
    depth = 4 if lean else int(rng.integers(2, 5))
    variant = everything if everything in ('cem', 'safe', 'cost') else ('cem' if everything == 'bf16' else ('cem', 'safe', 'cost')[seed % 3])
    if 'budget' in forced:
        variant = 'safe'
    elif 'tail' in forced and variant == 'cost':
        variant = 'cem'
    precision = 'bf16' if everything == 'bf16' else 'fp32' if (lean or wide or everything) else ('fp32', 'bf16x3', 'fp32', 'bf16', 'bf16x3')[seed % 5]
    segments = 0 if lean else int(rng.choice([0, 0, 2]))
    rc = 1 if lean else int(rng.choice([0, 0, 1, 2]))
    box, low, high = hp.random_action_bounds(rng, A)

    def want(name):
        if name in forced:
            return True
        if name == 'budget' and (variant != 'safe' or 'tail' in chosen):
            return False
        if name == 'tail' and (variant == 'cost' or everything == 'safe'):
            return False                                                        # (the safe "everything" handle takes the budget instead)
        return bool(rng.random() < (1.0 if everything else 0.3))
    chosen = set()
    for name in OPTIONS:
        if want(name):
            chosen.add(name)
    tail_m = int(rng.integers(1, P + 1)) if 'tail' in chosen else 0
    cost_m = int(rng.integers(1, P + 1)) if 'budget' in chosen else 0
    budget = float(rng.choice([0.0, 0.5, 1.0, 2.0])) if cost_m else float('inf')
    tau = float(rng.choice([0.1, 0.5, 2.0])) if 'softmax' in chosen else 0.0
    noise = (('powerlaw', float(rng.choice([0.5, 2.0]))) if rng.random() < 0.5 else ('ar1', float(rng.choice([0.5, 0.9])))) if 'mixed' in chosen else None
    keep = Keep(int(rng.integers(1, min(k, 4) + 1)), bool(rng.random() < 0.6 or everything), int(rng.integers(1, H))) if 'carry' in chosen else None
    schedule = None
    if 'sched' in chosen:
        kind = ('ragged', 'to_k', 'plain', 'grow')[seed % 4] if not lean else ('plain', 'ragged')[(seed // 4) % 2]
        if kind == 'to_k' and keep is not None:
            keep = keep._replace(m=max(1, min(keep.m, k - 2)))
        schedule = _schedule(rng, kind, N, k, I, q, (keep.m + 2) if keep is not None else 0)
    task = tc.task_for(O, A, seed, bool(rng.random() < 0.5)) if 'task' in chosen else None
    warm = Warm(int(rng.integers(1, H)), str(rng.choice(['box', 'repeat'])), str(rng.choice(['reset', 'keep'])), float(rng.choice([0.0, 0.25]))) if 'warm' in chosen else None
    opt = Options(tail_m, cost_m, budget, tau, noise, keep, schedule, 'mean' in chosen, 'track' in chosen, task, warm)
    smoothing = float(rng.choice([0.0, 0.1, 0.5]))
    # the stop threshold on the scale of the Box (sigma0 is its half width, 100 when it is unbounded): a fixed value would stop most
    # narrow boxes in their first iteration.  The "everything" handles run all their iterations
    frac = float(rng.choice([-1.0, -1.0, 0.1, 0.3]))
    thr = -1.0 if (frac < 0 or everything) else float(F(frac * float(np.mean(hp.o.sampling_params(low, high)[3]))))
    return Case('seed%d' % seed, O, A, H, N, P, E, k, I, units, depth, variant, precision, smoothing, thr, float(rng.choice([0.0, 0.05])), box,
                low, high, segments, rc, 400 + seed, opt)


def case_for(seed):
    """The case of a seed: deterministic, drawn again until `admitted` holds and the forced options are on."""
    seed = int(seed)
    j = seed % N_SEEDS                                                    # (CEM_FUZZ_SCALE: later rounds force the same pairs on other shapes)
    forced = frozenset(PAIRS[j]) if j < len(PAIRS) else frozenset()
    everything = EVERYTHING[j - len(PAIRS)] if j >= len(PAIRS) else None
    rng = np.random.default_rng(70000 + seed)
    for _ in range(1000):
        case = _draw(seed, rng, forced, everything)
        if admitted(case) and forced <= on(case) and (everything is None or len(on(case)) == (8 if everything == 'cost' else 9)):
            return case
    raise AssertionError('no admitted case for seed %d' % seed)


# ---- the problem and the handle -------------------------------------------------------------------------------------------------------
_PROBLEMS = {}


def problem(case):
    """The case's synthetic problem (cached: weights and state are never written to)."""
    key = (case.O, case.A, case.E, case.depth, case.units, case.pseed, None if case.low is None else (case.low.tobytes(), case.high.tobytes()))
    if key not in _PROBLEMS:
        pb = hp.make_problem(case.O, case.A, case.E, case.depth, seed=case.pseed, units=case.units)
        _PROBLEMS[key] = pb if case.low is None else hp.with_action_bounds(pb, case.low, case.high)
    return _PROBLEMS[key]


def config_kwargs(case, **over):
    """What hp.configs takes for the case."""
    kw = dict(N=case.N, H=case.H, P=case.P, E=case.E, k=case.k, I=case.I, variant=case.variant, thr=case.thr, noise=case.out_noise, post=POST,
              smoothing=case.smoothing, chunks_per_tile=case.rc, rollout_segments=case.segments, precision=case.precision)
    kw.update(over)
    return kw


def apply_options(pl, case):
    """The case's options through the CemPlanner setters, in the order of OPTIONS (a refusal raises _capi.CemError)."""
    o = case.opt
    if o.tail_m:
        pl.set_particle_objective('lower_tail', o.tail_m)
    if o.cost_m:
        pl.set_constraint('budget', 0 if o.cost_m == case.P else o.cost_m)
        pl.set_cost_budget(o.budget)
    if o.tau > 0:
        pl.set_refit('softmax', o.tau)
    if o.noise is not None:
        pl.set_action_noise(*o.noise)
    if o.keep is not None:
        pl.set_elite_carry(o.keep.m, o.keep.across, o.keep.shift)
    if o.schedule is not None:
        pl.set_population_schedule(list(o.schedule))
    if o.mean:
        pl.set_mean_candidate(True)
    if o.readout:
        pl.set_plan_readout(True)
    if o.task is not None:
        pl.set_task(o.task)
    if o.warm is not None:
        pl.set_warm_start(shift=o.warm.shift, tail=o.warm.tail, sigma=o.warm.sigma, floor_frac=o.warm.floor_frac)
        pl.set_init_mode('shift')


def cut_model_noise(case, em_it, n):
    """What an iteration of n candidates reads of slab `it` of a caller's eps_model [H, P N, O]: the LEADING H P n O floats as [H, P n, O]
    (cem_mpc.h; tests/decay_cases.cut_noise)."""
    return np.ascontiguousarray(em_it.reshape(-1)[:case.H * case.P * n * case.O].reshape(case.H, case.P * n, case.O))


# ---- the composed restatement ---------------------------------------------------------------------------------------------------------
class Reference:
    """The stages of a plan of `case`, each on the inputs handed to it.  No arithmetic of its own: every line calls an existing restatement."""

    def __init__(self, case):
        from oracle import cem_oracle as o
        self.o, self.case, self.opt = o, case, case.opt
        self.pb = problem(case)
        self.ocfg, self.pcfg = hp.configs(self.pb, **config_kwargs(case))
        self.lb, self.ub, self.mu0, self.sg0 = o.sampling_params(self.pb['low'], self.pb['high'])
        self.n = populations(case)
        self.M = mixing_matrix(case.opt.noise[0], case.opt.noise[1], case.H) if case.opt.noise is not None else None
        self.has_costs = case.variant != 'cem'

    def cfg_it(self, it):
        return dataclasses.replace(self.ocfg, n_samples=self.n[it])

    def cold(self):
        c = self.case
        return (np.broadcast_to(self.mu0, (c.H, c.A)).astype(F).copy(), np.broadcast_to(self.sg0, (c.H, c.A)).astype(F).copy())

    def empty_block(self):
        return empty_readout(self.case.H, self.case.A, self.case.P, self.has_costs)

    def action_noise(self, xi):
        """eps [I, N, H, A] the sampler multiplies by sigma, from the white streams xi."""
        return xi if self.M is None else mix_noise(self.M, xi)

    def init(self, plan_index, carry, store):
        """(mu, sigma) iteration 0 samples from and the elite store its inject reads (None: no inject there).  carry: (mu, sigma, valid) of
        the handle; store: the previous plan's last kept elites."""
        w = self.opt.warm
        mu, sigma = self.cold()
        if w is not None and plan_index > 0 and carry[2]:
            mu, sigma = shift_distribution(carry[0], carry[1], self.mu0, self.sg0, w.shift, 1 if w.tail == 'repeat' else 0,
                                           1 if w.sigma == 'keep' else 0, warm_sigma_floor(self.pcfg, w.floor_frac))
        k = self.opt.keep
        return mu, sigma, (store if (k is not None and k.across and plan_index > 0) else None)

    def candidates(self, it, mu, sigma, eps_it, store, plan_index):
        """The sample of iteration `it`: the sampler on the leading n[it] rows of the slab, the inject, the mean row."""
        n, k = self.n[it], self.opt.keep
        acts = self.o.sample_actions(mu, sigma, self.lb, self.ub, np.asarray(eps_it, F)[:n]).astype(F)
        if k is not None and store is not None:
            if it > 0:
                acts = inject_elites(acts, store, k.m, 0)
            elif plan_index > 0 and k.across:
                acts = inject_elites(acts, store, k.m, k.shift)
        if self.opt.mean and it == self.case.I - 1:
            acts = mean_candidate(acts, mu, self.lb, self.ub)
        return acts

    def scores(self, it, ret, costs):
        """The scores of the handle's objective on returns [P, n] and cost bytes [H, P, n] (None on 'cem')."""
        c, n = self.case, self.n[it]
        ret = np.asarray(ret, F).reshape(c.P, n)
        cb = None if costs is None else np.asarray(costs, np.uint8).reshape(c.H, c.P, n)
        if c.variant == 'cost':
            return cost_cases.scores_from_bytes(cb, c.P, n)
        if self.opt.tail_m:
            return rk.scores(ret, self.opt.tail_m, cb if c.variant == 'safe' else None, POST)
        if self.opt.cost_m:
            return kc.scores(ret, cb, c.P, n, self.opt.cost_m, self.opt.budget)
        mean = kc.mean_returns(ret)
        if c.variant == 'safe':
            mean = mean - np.where(rk.unsafe_flags(cb, c.P, POST), F(1.0), F(0.0)) * F(100.0)
        return mean

    def select(self, it, scores, actions, mu, sigma, best, best_score):
        """-> (mu, sigma, best, best_score, elite, stop, mean sigma the stop rule compared)."""
        scores, actions = np.asarray(scores, F), np.asarray(actions, F)
        mu_n, sg_n, best, best_score, elite, stop = self.o.select_and_refit(scores, actions, mu, sigma, best, best_score, self.cfg_it(it))
        mean_sigma = float(sg_n.mean(dtype=F))
        if self.opt.tau > 0:
            mu_n, sg_n = softmax_refit(scores, elite, actions, mu, sigma, self.case.smoothing, self.opt.tau)[:2]
            stop, mean_sigma = wc.stops(sg_n, self.case.thr)
            mean_sigma = float(mean_sigma)
        return mu_n, sg_n, best, best_score, elite, stop, mean_sigma

    def keep(self, scores, elite, actions):
        return keep_elites(scores, elite, actions, self.opt.keep.m)

    def track(self, block, it, iters, best_score, scores, elite, actions, ret, costs):
        return track_best(block, it, iters, best_score, scores, elite, actions, ret, costs if self.has_costs else None, n=self.n[it])

    def finish(self, best, eps_out):
        return best + np.asarray(eps_out, F) * F(self.ocfg.noise_stddev)

    # -- the fp32 oracle's rollout, for `replay`
    def oracle_rollout(self, it, actions, em_it):
        """(scores, ret [P, n], cost bytes [H, P, n] or None) of the fp32 oracle on the sample: o.candidate_scores, or task_objective on
        o.unfold_sequences with a task on; the other objectives through `scores` on the oracle's own returns and cost bytes."""
        o, c, pb, n = self.o, self.case, self.pb, self.n[it]
        cfg = self.cfg_it(it)
        if self.opt.task is not None:
            s0 = np.broadcast_to(pb['state'].astype(F), (c.P * n, c.O)).copy()
            traj = o.unfold_sequences(s0, np.tile(actions, (c.P, 1, 1)), pb['weights'], o.member_of_rows(c.P * n, c.E), pb['inputs_min'],
                                      pb['inputs_max'], em_it.astype(F), cfg.scale_features, cfg.sampling_propagation)
            ret, costs = task_objective(traj, actions, self.opt.task, c.variant)
            ret, costs = ret.reshape(c.P, n), (None if costs is None else costs.reshape(c.H, c.P, n))
            return self.scores(it, ret, costs), ret, costs
        sc, traj = o.candidate_scores(pb['state'], actions, pb['weights'], pb['inputs_min'], pb['inputs_max'], em_it, cfg, pb['scorer'],
                                      return_traj=True)
        ret, costs = rdc.oracle_evidence(traj, c.P, n, pb['scorer'], c.variant)
        if c.variant == 'cost':
            costs = cost_cases.cost_bytes(traj, pb['scorer']).reshape(c.H, c.P, n)
        cb = (costs != 0).astype(np.uint8) if self.has_costs else None
        if c.variant == 'cost' or self.opt.tail_m or self.opt.cost_m:
            sc = self.scores(it, ret, cb)
        return sc, ret, cb


def replay(case, noises, ref=None):
    """Consecutive plans of the case on the fp32 oracle's own values: `noises` holds one (eps_act [I, N, H, A], eps_model [I, H, P N, O],
    eps_out [A]) per plan (white streams: mixed noise is mixed from them).  -> one dict per plan: action, score, iters, trace, block, mu,
    sigma, store; a trace entry holds actions, scores, elite, mu, sigma, store, before, ret, costs."""
    ref = Reference(case) if ref is None else ref
    c, out = case, []
    carry, store = (np.zeros((c.H, c.A), F), np.zeros((c.H, c.A), F), False), None
    for plan_index, (ea, em, eo) in enumerate(noises):
        mu, sigma, st = ref.init(plan_index, carry, store)
        eps = ref.action_noise(np.asarray(ea, F))
        best, best_score = np.zeros(c.A, F), F(-np.inf)
        block, trace = ref.empty_block(), []
        for it in range(c.I):
            actions = ref.candidates(it, mu, sigma, eps[it], st, plan_index)
            scores, ret, costs = ref.oracle_rollout(it, actions, cut_model_noise(c, em[it], ref.n[it]))
            before = best_score
            mu, sigma, best, best_score, elite, stop, _ = ref.select(it, scores, actions, mu, sigma, best, best_score)
            if c.opt.keep is not None:
                st = ref.keep(scores, elite, actions)
            if c.opt.readout:
                block = ref.track(block, it, it + 1, best_score, scores, elite, actions, ret, costs)
            trace.append(dict(actions=actions, scores=scores, elite=elite, mu=mu.copy(), sigma=sigma.copy(), store=st, before=before, ret=ret,
                              costs=costs))
            if stop:
                break
        carry, store = (mu, sigma, True), st
        out.append(dict(action=ref.finish(best, eo), score=best_score, iters=len(trace), trace=trace, block=block, mu=mu, sigma=sigma, store=st))
    return out


def noise_for(case, seed, plans=2):
    """hp.noise for `plans` consecutive plans of the case."""
    return [hp.noise(case.I, case.N, case.H, case.A, case.P, case.O, seed=seed + 1000 * j) for j in range(plans)]


# ---- the per-option case tables as composed cases (tests/test_composed_cases_cpu.py ties `replay` to their oracle_plan) ----------------
def _from(c, P, I, out_noise, opt, H=None):
    return Case(c.name, c.obs, c.act, c.H if H is None else H, c.N, P, c.E, c.k, I, c.units, c.depth, c.variant, c.precision, 0.0, -1.0, out_noise,
                'problem', None, None, c.segments, c.rc, 77, opt)


def from_elite(c, m=None):
    return _from(c, c.E, ec.I, 0.01, NOTHING._replace(keep=Keep(c.m if m is None else m, False, c.shift)))


def from_decay(c, with_mean=False):
    from tests import decay_cases as dc
    return _from(c, c.P, dc.I, 0.01, NOTHING._replace(schedule=tuple(c.schedule), mean=with_mean))


def from_readout(c):
    return _from(c, c.P, rdc.I, 0.0, NOTHING._replace(readout=True))
