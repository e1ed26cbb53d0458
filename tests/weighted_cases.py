"""The score-weighted refit (cem_mpc.h: cem_planner_set_refit, CEM_REFIT_SOFTMAX) restated in NumPy, and the score
vectors its tests share.  The reference has no such update (MPPI; the refit of TD-MPC / PlaNet-style planners): the definition in
cem_mpc.h is the contract, for one problem and one iteration:
  s_j = scores[elite[j]], s_max = max s_j; beta = fl32(1 / tau); w_j = 1 where s_j == s_max, else exp((s_j - s_max) * beta);
  W = sum w_j; mean = sum w_j a_j / W; var = sum w_j (a_j - mean)^2 / W (two-pass); sd = sqrt(var);
  mu <- s mu + fl32(1 - s) mean; sigma <- s sigma + fl32(1 - s) sd; stop iff mean(sigma) <= threshold; ESS = W^2 / sum w_j^2.
refit64 is that in float64 (the fp32 inputs and the two fp32 constants taken as they are): what the device is held to by tolerance.
refit32 is the same in float32 with NumPy's pairwise sums — another summation order than the kernel's — and shows how much of the
tolerance a correct fp32 implementation uses (tests/test_weighted_cases_cpu.py: at most a quarter).
A case is (name, N, k, tau, scores float32[N], H, A).  NaN scores are outside the contract.  Importable without a GPU or torch."""
import collections

import numpy as np

F = np.float32
D = np.float64

# the bars of a select (tests/test_gpu_select_paths.py:78-79), which the weighted refit keeps
MU_RTOL, MU_ATOL = 1e-5, 1e-6
SG_RTOL, SG_ATOL = 2e-5, 1e-6

# The kernel's depths, in elites k, for a column block of ncol columns served by tpc parts (tpc = the largest power of two with
# tpc * ncol <= 1024; H A = 6: 128; a full block of 1024 columns: 1):
#   tpc            up to tpc elites every part holds at most one row
#   KEEP * tpc     rows a thread gathers once and keeps in registers for both phases (CEM_REFIT_KEEP = 4)
#   + BATCH * tpc  every further trip of the re-gathering loop (CEM_REFIT_BATCH = 4)
#   1024           elites per trip of the weight loop (one per thread)
KEEP, BATCH, THREADS = 4, 4, 1024

Case = collections.namedtuple('Case', 'name N k tau scores H A')


def beta_of(tau):
    """fl32(1 / tau): one fp32 division on the host."""
    t = F(tau)
    assert np.isfinite(t) and t > 0
    with np.errstate(over='ignore'):
        return F(1.0) / t


def weights64(s, tau):
    s = np.asarray(s, F).astype(D)
    smax = s.max()
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        return np.where(s == smax, 1.0, np.exp((s - smax) * D(beta_of(tau))))


def refit64(scores, elite, actions, mu, sigma, smoothing, tau):
    """-> (mu_new, sigma_new, ess, mean, sd), float64.  actions [N, ...], mu / sigma of the trailing shape."""
    e = np.asarray(elite, np.int64)
    w = weights64(np.asarray(scores, F)[e], tau)
    a = np.asarray(actions, F)[e].astype(D)
    wb = w.reshape((-1,) + (1,) * (a.ndim - 1))
    W = w.sum()
    mean = (wb * a).sum(axis=0) / W
    var = (wb * (a - mean) ** 2).sum(axis=0) / W
    sd = np.sqrt(var)
    s, oms = D(F(smoothing)), D(F(1.0 - float(smoothing)))
    return s * np.asarray(mu, F).astype(D) + oms * mean, s * np.asarray(sigma, F).astype(D) + oms * sd, W * W / (w * w).sum(), mean, sd


def _psum(x):
    """fp32 sum over axis 0 with NumPy's pairwise order (the reduced axis made contiguous)."""
    x = np.asarray(x, F)
    return np.add.reduce(np.ascontiguousarray(np.moveaxis(x, 0, -1)), axis=-1, dtype=F)


def refit32(scores, elite, actions, mu, sigma, smoothing, tau):
    """The contract in float32, operation for operation, sums in NumPy's pairwise order -> (mu_new, sigma_new, ess, mean, sd)."""
    e = np.asarray(elite, np.int64)
    s = np.asarray(scores, F)[e]
    smax = s.max()
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        w = np.where(s == smax, F(1.0), np.exp(((s - smax).astype(F) * beta_of(tau)).astype(F)).astype(F)).astype(F)
    a = np.asarray(actions, F)[e]
    wb = w.reshape((-1,) + (1,) * (a.ndim - 1))
    W = _psum(w)
    mean = (_psum(wb * a) / W).astype(F)
    d = (a - mean).astype(F)
    sd = np.sqrt((_psum(wb * (d * d)) / W).astype(F)).astype(F)
    sm, oms = F(smoothing), F(1.0 - float(smoothing))
    return ((sm * np.asarray(mu, F) + oms * mean).astype(F), (sm * np.asarray(sigma, F) + oms * sd).astype(F), F(W * W / _psum(w * w)), mean, sd)


def stops(sigma_new, threshold):
    """cem_mpc.py:66-67 with the select's sum: sigma added in index order in fp32 from 0, divided once by the count."""
    ssum = F(0.0)
    for v in np.asarray(sigma_new, F).ravel():
        ssum = F(ssum + v)
    return bool(F(ssum / F(np.asarray(sigma_new).size)) <= F(threshold)), F(ssum / F(np.asarray(sigma_new).size))


def reference_top_k(scores, k):
    """The k largest by value, ties -> lower index, -0.0 == +0.0; ascending indices (tests/select_cases.py without NaN)."""
    s = np.asarray(scores, F).astype(D)
    return np.sort(np.lexsort((np.arange(s.shape[0]), -s))[:k])


def synthetic_actions(case, seed=7):
    """A stand-in for the handle's action tensor where there is no device: clip(eps, -1, 1) [N, H, A], fp32."""
    rng = np.random.default_rng(seed + case.N)
    return np.clip(rng.standard_normal((case.N, case.H, case.A)), -1.0, 1.0).astype(F)


def encode_infeasible(total):
    """cem_f32_encode_infeasible (cem_mpc.h): -(float)(2^23 + T) * 2^77."""
    return -((np.asarray(total, np.int64) + (1 << 23)).astype(F)) * F(2.0 ** 77)


def _cases():
    out = []

    def add(name, N, k, tau, sc, H=3, A=2):
        sc = np.ascontiguousarray(sc, F)
        assert sc.shape == (N,) and 1 <= k <= N and not np.isnan(sc).any()
        out.append(Case(name, N, int(k), float(tau), sc, H, A))

    rng = np.random.default_rng(2026)
    spread = lambda n: rng.standard_normal(n).astype(F)
    # ---- the temperature: small (a few elites carry the weight), moderate, and so large that every weight rounds to 1
    sc = spread(301)
    add('tau_small', 301, 37, 0.05, sc)                  # k % 4 == 1
    add('tau_moderate', 301, 37, 1.0, sc)
    add('tau_1e30', 301, 37, 1e30, sc)
    # ---- k edges
    add('k1', 64, 1, 0.5, spread(64))
    add('kN', 101, 101, 0.5, spread(101))                # MPPI: every candidate
    add('k_not_multiple_of_4', 257, 30, 0.3, spread(257))
    # ---- both sides of every depth at H A = 6 (tpc = 128): one row per part | KEEP rows in registers | the weight loop's trip
    sc = spread(600)
    for k in (127, 128, 129, KEEP * 128 - 1, KEEP * 128, KEEP * 128 + 1):
        add('depth_k%d' % k, 600, k, 0.7, sc)
    # (beyond N = 600: the only sizes at which the second trip of the re-gathering loop and of the weight loop run at H A = 6)
    sc = spread(1100)
    for k in ((KEEP + BATCH) * 128, (KEEP + BATCH) * 128 + 1, 1100):
        add('depth_k%d' % k, 1100, k, 0.7, sc)
    # ---- ties at the maximum: five elites share it
    sc = spread(257)
    sc[[3, 77, 130, 131, 256]] = F(4.5)
    add('ties_at_max', 257, 40, 0.2, sc)
    # ---- infinities
    sc = spread(64)
    sc[rng.permutation(64)[:34]] = -np.inf
    add('neg_inf_among_elites', 64, 40, 0.5, sc)         # 30 finite, 10 of the 34 -inf (the lowest indices) are elite: weight 0
    add('neg_inf_all', 64, 9, 0.5, np.full(64, -np.inf, F))
    sc = spread(64)
    sc[41] = np.inf
    add('pos_inf_one', 64, 12, 0.5, sc)
    # ---- SafeCemMpc's crowd: unsafe candidates at return - 100, a tenth safe; more elites than safe candidates
    sc = (F(-100.0) + rng.uniform(0.0, 2.0, 400).astype(F)).astype(F)
    safe = rng.permutation(400)[:40]
    sc[safe] = rng.uniform(-3.0, 3.0, 40).astype(F)
    add('safe_crowd', 400, 90, 1.0, sc)
    add('safe_crowd_all_unsafe', 400, 90, 1.0, (F(-100.0) + rng.uniform(0.0, 2.0, 400).astype(F)).astype(F))
    # ---- the budget encoding: infeasible candidates at -(2^23 + T) 2^77, mixed with feasible returns and alone
    sc = encode_infeasible(rng.integers(1, 200, 300))
    feas = rng.permutation(300)[:25]
    sc[feas] = rng.uniform(-2.0, 6.0, 25).astype(F)
    add('budget_mixed', 300, 60, 0.5, sc)
    tot = rng.integers(5, 200, 300)
    tot[[17, 200]] = 3                                   # the two cheapest tie: both weigh 1, the rest 0
    add('budget_all_infeasible', 300, 60, 0.5, encode_infeasible(tot))
    # ---- signed zeros: both zeros are the maximum, the rest negative
    sc = (-rng.uniform(0.1, 5.0, 99)).astype(F)
    sc[0::9] = F(-0.0)
    sc[4::9] = F(0.0)
    add('signed_zeros', 99, 50, 0.8, sc)
    # ---- one dominant score: every other weight underflows to exactly 0 (DOMINANT_AT is its candidate index)
    sc = spread(128)
    sc[DOMINANT_AT] = F(2000.0)
    add('dominant', 128, 20, 1.0, sc)
    # ---- H A = 1030 > 1024: two column blocks — 1024 columns on one part each (tpc = 1: depths KEEP, KEEP + BATCH), then 6 on 128 parts
    sc = spread(32)
    for k in (KEEP - 1, KEEP, KEEP + 1, KEEP + BATCH, KEEP + BATCH + 1, 32):
        add('wide_k%d' % k, 32, k, 0.6, sc, H=103, A=10)
    return out


DOMINANT_AT = 71
CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
