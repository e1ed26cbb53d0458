"""Shapes, weights and the NumPy restatement of the weight images for the device weight hand-over tests
(tests/test_weight_handover_cpu.py, tests/test_gpu_weight_handover.py).

The restatement is destination driven like the kernels of csrc/cem_pack.h, but shares no code with them or with the host packers of
cem_capi.hip: ``units_*`` lists which matrix block every unit of a member's image holds, ``image_*`` gathers the words."""
import numpy as np

from ethz_safe_learning_amd import PlannerConfig, ScorerConfig

# name -> overrides of BASE: every index branch of the three packers at the smallest shapes that reach it
BASE = dict(obs_dim=60, act_dim=2, units=128, n_layers=4, ensemble_size=5, particles=5, n_samples=32, horizon=3, n_elite=4, iterations=2,
            activation='relu', precision='fp32')
TUNED = {
    'tuned_nfw1': dict(),
    'obs63_act1': dict(obs_dim=63, act_dim=1),                       # O not a multiple of 4 or 16
    'nfw2_obs100_act12': dict(obs_dim=100, act_dim=12),              # obs + act over 64: two layer-0 blocks per wave
    'u16_l1': dict(units=16, n_layers=1), 'u16_l6': dict(units=16, n_layers=6),      # narrow, zero-padded hidden layers
    'u48_l1': dict(units=48, n_layers=1), 'u48_l6': dict(units=48, n_layers=6),
    'split_members': dict(ensemble_size=15, particles=5, n_samples=150, n_elite=15),
}
SPLIT = {
    'bf16x3_nfw1': dict(precision='bf16x3'),
    'bf16x3_nfw2': dict(precision='bf16x3', obs_dim=100, act_dim=12),
    'bf16x3_u48_obs63': dict(precision='bf16x3', units=48, n_layers=2, obs_dim=63, act_dim=1),
}
WIDE = {
    'wide_u200_relu': dict(units=200, n_layers=2),
    'wide_u256_tanh': dict(units=256, n_layers=2, activation='tanh'),
    'wide_u128_tanh': dict(units=128, n_layers=3, activation='tanh'),
    'wide_obs100_act12': dict(units=144, n_layers=2, obs_dim=100, act_dim=12),
}
CASES = dict(**TUNED, **SPLIT, **WIDE)


def config(case, **kw):
    c = dict(BASE)
    c.update(CASES[case] if isinstance(case, str) else case)
    c.update(kw)
    A = c['act_dim']
    return PlannerConfig(scorer=ScorerConfig(goal_slice=(3, 19), cost_kinds=[(22, 38, 0.2)]), act_low=[-1.0] * A, act_high=[1.0] * A, **c)


# exact values planted among the random weights: the edges of the three-way bf16 split
F32 = np.float32
SPECIAL = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 2.0 ** -126, -2.0 ** -126, 1.5, -0.375,          # +-0, denormals, 2^-126, bf16-exact
                    1.0 + 2.0 ** -10, -(1.0 + 2.0 ** -10), 1.0 + 2.0 ** -9 + 2.0 ** -18,                             # third piece zero; three pieces
                    0.0, 0.0], F32)
SPECIAL[-2:] = np.array([0x7F7EFFFF, 0xFF7EFFFF], np.uint32).view(F32)                                               # just below the largest bf16


def weights(cfg, seed=0, special=False, scale=None):
    """Per-member Keras-layout dicts of random normals (every bias too); special=True plants SPECIAL at random places of every array
    (images only: a plan with 3e38 among its weights is all NaN)."""
    rng = np.random.default_rng(seed)
    D, O, U, L = cfg.obs_dim + cfg.act_dim, cfg.obs_dim, cfg.units, cfg.n_layers

    def arr(*shape):
        s = scale if scale is not None else 1.0 / np.sqrt(shape[0])
        a = rng.normal(0, s, shape).astype(F32)
        if special:
            flat = a.reshape(-1)
            at = rng.choice(flat.size, size=min(flat.size, SPECIAL.size), replace=False)
            flat[at] = SPECIAL[:at.size]
        return a
    out = []
    for _ in range(cfg.ensemble_size):
        Ws, bs, fi = [], [], D
        for _ in range(L):
            Ws.append(arr(fi, U)); bs.append(arr(U)); fi = U
        out.append(dict(W=Ws, b=bs, W_mu=arr(U, O), b_mu=arr(O), W_var=arr(U, O), b_var=arr(O)))
    return out


# ---- the maps ---------------------------------------------------------------------------------------------------------------
def perm_hidden(w, phi):
    """input block a wave visits at position phi of a hidden / heads stage: its own two first, the rest ascending"""
    return ([2 * w, 2 * w + 1] + [b for b in range(8) if b // 2 != w])[phi]


def perm_l0(w, nfw, phi):
    """... of layer 0: its own blocks w, w + 4, ... first, the rest ascending"""
    return ([w + 4 * i for i in range(nfw)] + [b for b in range(4 * nfw) if b % 4 != w])[phi]


def split_perm(w, phi):
    return ([w] + [c for c in range(4) if c != w])[phi]


def _dims(cfg):
    D, O = cfg.obs_dim + cfg.act_dim, cfg.obs_dim
    kb_in, kb_obs = -(-D // 16), -(-O // 16)
    return D, O, kb_in, kb_obs, -(-kb_in // 4)


def units_fp32(cfg):
    """[(matrix, k block, output block)] of a member's stream, matrix = ('W', l) | 'W_mu' | 'W_var'; a 2 KB group is two units"""
    _, _, _, kb_obs, nfw = _dims(cfg)
    out = []
    for w in range(4):
        for P in range(4 * nfw):
            F = perm_l0(w, nfw, P)
            out += [(('W', 0), F, 2 * w), (('W', 0), F, 2 * w + 1)]
        swap = lambda P: P ^ 1 if P < 2 else P                                       # the second accumulator takes the own blocks swapped
        for l in range(1, cfg.n_layers):
            for P in range(8):
                out += [(('W', l), perm_hidden(w, P), 2 * w), (('W', l), perm_hidden(w, swap(P)), 2 * w + 1)]
        for Fo in range(w, min(4 * nfw, kb_obs), 4):
            for P in range(8):
                out += [('W_mu', perm_hidden(w, P), Fo), ('W_var', perm_hidden(w, swap(P)), Fo)]
    return out


def units_split(cfg):
    """... of the split stream: the k block is a K = 32 chunk; a 6 KB group is two units (a, b)"""
    _, _, _, kb_obs, nfw = _dims(cfg)
    out = []
    for w in range(4):
        for P in range(max(2 * nfw, 2)):
            out += [(('W', 0), P, 2 * w), (('W', 0), P, 2 * w + 1)]
        for l in range(1, cfg.n_layers):
            for P in range(4):
                out += [(('W', l), split_perm(w, P), 2 * w), (('W', l), split_perm(w, P), 2 * w + 1)]
        for Fo in range(w, min(4 * nfw, kb_obs), 4):
            for P in range(4):
                out += [('W_mu', split_perm(w, P), Fo), ('W_var', split_perm(w, P), Fo)]
    return out


def units_wide(cfg):
    _, _, kb_in, kb_obs, _ = _dims(cfg)
    nbu = -(-cfg.units // 16)
    out = []
    for l in range(cfg.n_layers):
        out += [(('W', l), kb, ob) for kb in range(kb_in if l == 0 else nbu) for ob in range(nbu)]
    for name in ('W_mu', 'W_var'):
        out += [(name, kb, ob) for kb in range(nbu) for ob in range(kb_obs)]
    return out


def _matrix(w, name):
    return w['W'][name[1]] if isinstance(name, tuple) else w[name]


def _gather(W, k, o):
    """W[k, o] with zeros outside the matrix (k, o broadcastable index arrays)"""
    k, o = np.broadcast_arrays(k, o)
    ok = (k < W.shape[0]) & (o < W.shape[1])
    out = np.zeros(k.shape, F32)
    out[ok] = W[k[ok], o[ok]]
    return out


LANE = np.arange(64)
Q, I16 = (LANE >> 4)[:, None], (LANE & 15)[:, None]


def image_fp32(cfg, w, units=None):
    """uint32 words of one member's image: units of [lane(64)][r(4)], then 4 KB of zeros (tuned stream only)"""
    tuned = units is None
    r = np.arange(4)[None, :]
    parts = [_gather(_matrix(w, name), 16 * kb + 4 * Q + r, 16 * ob + I16).reshape(-1) for name, kb, ob in (units_fp32(cfg) if tuned else units)]
    if tuned:
        parts.append(np.zeros(1024, F32))
    return np.concatenate(parts).view(np.uint32)


def image_wide(cfg, w):
    return image_fp32(cfg, w, units_wide(cfg))


def rn_bf16(x):
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32)


def split3(x):
    """exact three-way bf16 split of fp32 values -> three uint16 arrays (round to nearest even, two exact subtractions)"""
    x = np.ascontiguousarray(x, F32)
    with np.errstate(over='ignore', invalid='ignore'):
        a0 = rn_bf16(x)
        r1 = (x - a0.view(F32)).astype(F32)
        a1 = rn_bf16(r1)
        r2 = (r1 - a1.view(F32)).astype(F32)
    return [(a >> 16).astype(np.uint16) for a in (a0, a1, r2.view(np.uint32))]


def image_split(cfg, w):
    """uint32 words of one member's split image: units of [plane(3)][lane(64)][s(8)] bf16, then 4 KB of zeros"""
    s = np.arange(8)[None, :]
    parts = []
    for name, kb, ob in units_split(cfg):
        v = _gather(_matrix(w, name), 16 * (2 * kb + (s >> 2)) + 4 * Q + (s & 3), 16 * ob + I16)
        parts += [p.reshape(-1) for p in split3(v)]
    parts.append(np.zeros(2048, np.uint16))
    return np.ascontiguousarray(np.concatenate(parts)).view(np.uint32)
