"""Shared inputs of the variance-regime tests (tests/test_variance_cases_cpu.py, tests/test_gpu_variance_regimes.py): models whose
variance-head bias walks a LADDER of pre-softplus values, so that var = softplus(v) + 1e-4 (mlp_ensemble.py:33-34,59-61) is evaluated on
the floor (v <= -40: var is fl32(1e-4)), on both tail branches of Eigen's softplus and across its two switch points (+-13.942384), around
zero, where softplus is ~v, and beyond |v| = 88, where expf(-v) overflows and exp2 underflows.  With the variance on its floor the
gradient (mu - y) / var is 1e4 (mu - y): Adam's element-wise clip (clipvalue, mlp_ensemble.py:113-117) is live on the mean head while
the variance head's own gradients stay below it.  Importable without a GPU; everything here is NumPy and the oracle."""
import numpy as np

from oracle import cem_oracle as o
from tests import helpers as hp

SWITCH = 13.942384                      # -(log(fp32 eps) + 2): Eigen's softplus switches branches at +-SWITCH (oracle.softplus_tf)
LADDER = [-104, -90, -40, -20, -14.5, -SWITCH, -13.5, -8, -2, 0, 2, 13.5, SWITCH, 14.5, 20, 40, 90]
NR = len(LADDER)
SWITCH_RUNGS = (LADDER.index(-SWITCH), LADDER.index(SWITCH))
SPREAD = 0.30                           # |v - b_var| stays below this on every shape below (asserted on the CPU)
BAND = 1e-3                             # elements with ||g| - clip| < BAND * clip may land on either side of the clip in fp32

# (O, A, E, L, units[, precision]) of the rollout heads: one and two input blocks per wave (tuned fp32), a narrow odd shape, the wide
# kernel; and the split-product rollout
ROLLOUT_CASES = [(60, 2, 5, 4, 128, 'fp32'), (100, 12, 8, 4, 128, 'fp32'), (23, 3, 2, 2, 48, 'fp32'), (20, 3, 2, 3, 200, 'fp32'),
                 (60, 2, 5, 4, 128, 'bf16x3')]
ROLLOUT_FAMILY = {(60, 128): 'tuned fp32, one input block', (100, 128): 'tuned fp32, two input blocks', (23, 48): 'tuned fp32, 48 units',
                  (20, 200): 'wide'}

# (E, D, O, L, bt, units, activation, batch_size, clipvalue, kernels) of the training steps.  bt 600 on batch_size 600: 32 row parts of
# two 16-row passes each (the last ones ragged), partial gradients summed before the clip
TRAIN_CASES = [
    (2, 20, 17, 2, 37, 48, 'relu', 64, 1.0, ('tile', 'gemm')),
    (3, 62, 60, 4, 64, 128, 'relu', 64, 1.0, ('tile', 'gemm')),
    (2, 62, 60, 3, 600, 128, 'relu', 600, 1.0, ('tile', 'gemm')),
    (2, 62, 60, 3, 64, 256, 'relu', 64, 1.0, ('gemm',)),
    (1, 30, 28, 7, 20, 64, 'relu', 64, 1.0, ('gemm',)),
    (2, 62, 60, 3, 64, 128, 'tf.nn.swish', 64, 1.0, ('gemm',)),
    (3, 62, 60, 4, 64, 128, 'relu', 64, 0.05, ('tile', 'gemm')),          # the clip live in the hidden layers' tensors too
    (3, 62, 60, 4, 64, 128, 'relu', 64, 1e30, ('tile', 'gemm')),          # "no clip": raw gradients of up to ~30 come through
]
# (E, D, O, L, units, activation, kernels) of validation_loss / forward: the tile form's two shapes, and the generic form's
EVAL_CASES = [
    (2, 20, 17, 2, 48, 'relu', ('tile', 'gemm')),
    (3, 62, 60, 4, 128, 'relu', ('tile', 'gemm')),
    (2, 62, 60, 3, 256, 'relu', ('gemm',)),
    (1, 30, 28, 7, 64, 'relu', ('gemm',)),
    (2, 62, 60, 3, 128, 'tf.nn.swish', ('gemm',)),
]
EVAL_ROWS = 83                          # one 64-row chunk and a ragged second one (19 rows: a full 16-row part and 3 rows)

LR = 0.00025
F = np.float32
BETA1, BETA2, EPSILON = F(0.9), F(0.999), F(1e-5)       # the device's copies of Adam's constants (cem_train_config_t holds floats)
OB1, OB2 = F(1) - BETA1, F(1) - BETA2                   # cem_adam_kernel's 1 - beta, in fp32


def rungs(O, member):
    """Index into LADDER of every output column of one member: the ladder shifts by one column per member."""
    return (np.arange(O) + member) % NR


def ladder_problem(O, A, E, L, units, activation='relu', seed=0):
    """hp.make_problem (Glorot weights, non-zero biases, heads x 0.3) with b_var[c] = LADDER[(c + member) % 17]."""
    pb = hp.make_problem(O, A, E, L, seed=seed, bias_noise=0.05, head_scale=0.3, var_bias=0.0, units=units, activation=activation)
    for m, w in enumerate(pb['weights']):
        w['b_var'][:] = np.asarray(LADDER, np.float32)[rungs(O, m)]
    return pb


def training_data(D, O, n, seed=3):
    """X ~ N(0, 0.5), Y = 0.1 X[:, :O] + 0.05 N(0, 1), as tests/test_gpu_training.py draws them; and the generator, for the permutations."""
    rng = np.random.default_rng(seed)
    X = rng.normal(0, 0.5, (n, D)).astype(np.float32)
    Y = (0.1 * X[:, :O] + 0.05 * rng.normal(0, 1, (n, O))).astype(np.float32)
    return X, Y, rng


def train_inputs(E, D, O, bt, steps=2):
    """(X, Y, [perm of step 1, perm of step 2], offsets): bt + 64 rows; step t takes rows perm_t[m, 7 t : 7 t + bt] for member m."""
    X, Y, rng = training_data(D, O, bt + 64)
    perms = [np.stack([rng.permutation(X.shape[0]) for _ in range(E)]).astype(np.int32) for _ in range(steps)]
    return X, Y, perms, [7 * (t + 1) for t in range(steps)]


def rollout_inputs(pb, E, seed=5):
    """(s0 [B, O], actions [B, 1, A], eps [1, B, O]) with B = 16 E, as test_unfold_sequences_matches_oracle draws them."""
    O, A, B = pb['state'].shape[0], pb['low'].shape[0], 16 * E
    rng = np.random.default_rng(seed)
    s0 = (pb['state'][None, :] + 0.05 * rng.standard_normal((B, O))).astype(np.float32)
    acts = rng.uniform(-1, 1, (B, 1, A)).astype(np.float32)
    eps = rng.standard_normal((1, B, O)).astype(np.float32)
    return s0, acts, eps


def rollout_reference(pb, E, s0, acts, dtype=np.float64):
    """(mu, var, pre-softplus v) of the first step in ``dtype``: the scaled inputs through o.ensemble_forward."""
    x0 = o.scale(np.concatenate([s0, acts[:, 0]], 1).astype(dtype), pb['inputs_min'], pb['inputs_max'], True)
    w = o.cast_weights(pb['weights'], dtype)
    members = o.member_of_rows(s0.shape[0], E)
    mu, var = o.ensemble_forward(x0, w, members)
    return mu, var, pre_softplus(x0, w, members)


def pre_softplus(x, weights, members):
    """The variance head's pre-activation v [rows, O] (o.gaussian_dist_mlp up to the softplus)."""
    out = np.empty((x.shape[0], weights[0]['W_var'].shape[1]), x.dtype)
    for m in np.unique(members):
        w, sel = weights[int(m)], members == m
        f, _ = o.activation_and_grad(w.get('activation', 'relu'))
        h = x[sel]
        for W, b in zip(w['W'], w['b']):
            h = f(h @ W + b)
        out[sel] = h @ w['W_var'] + w['b_var']
    return out


def check_ladder(v, b_var_rungs, straddle=True):
    """v [rows, O] of one member against its rungs: every value within SPREAD of its rung; every rung but the two switch rungs wholly on
    its intended side of +-SWITCH; with ``straddle``, each switch rung with values on both sides of its switch point (over the rows and
    the columns that hold the rung).  The rollouts' softplus has no branches, so their inputs are not asked to straddle."""
    lad = np.asarray(LADDER, np.float64)[b_var_rungs]
    assert np.abs(v - lad[None, :]).max() <= SPREAD, float(np.abs(v - lad[None, :]).max())
    for r in range(NR):
        cols = v[:, b_var_rungs == r]
        for s in (-SWITCH, SWITCH):
            below = cols < s
            if LADDER[r] == s:
                assert not straddle or (below.any() and (~below).any()), 'rung %g does not straddle its switch point' % s
            else:
                assert below.all() if LADDER[r] < s else not below.any(), (r, s)


# ---- the training step's reference ---------------------------------------------------------------------------------------------------
NAMES = lambda L: ['W%d' % l for l in range(L)] + ['b%d' % l for l in range(L)] + ['W_mu', 'b_mu', 'W_var', 'b_var']


def flat(ws):
    """{tensor name: [E, ...]} of a list of per-member dicts (weights, moments or gradients): a tensor is pooled over the members."""
    L = len(ws[0]['W'])
    return {n: np.stack([o._flat_params(w)[i] for w in ws]) for i, n in enumerate(NAMES(L))}


def grads(weights, X, Y, idx, dtype):
    """(total loss, [per-member gradient dicts]) of one training_step in ``dtype`` (no Adam)."""
    E = len(weights)
    w = o.cast_weights(weights, dtype)
    out, total = [], dtype(0)
    for m in range(E):
        loss, g = o.member_loss_and_grads(w[m], X[idx[m]].astype(dtype), Y[idx[m]].astype(dtype), E)
        total += loss
        out.append(g)
    return total, out


def adam64(w, g, m, v, lr, t, clip):
    """o.adam_apply in fp64 on the device's fp32 constants, tensor by tensor of flat() dicts -> (w, m, v)."""
    out = ({}, {}, {})
    for n in w:
        r = o.adam_apply(w[n].astype(np.float64), g[n].astype(np.float64), m[n].astype(np.float64), v[n].astype(np.float64), lr, t,
                         beta1=float(BETA1), beta2=float(BETA2), epsilon=float(EPSILON), clipvalue=float(F(clip)))
        for d, a in zip(out, r):
            d[n] = a
    return out


def lr_t(lr, t):
    """CemTrainer.lr_t: Keras' bias-corrected step size in fp32."""
    return F(F(lr) * F(np.sqrt(1.0 - 0.999 ** t)) / F(1.0 - 0.9 ** t))


def adam32_clipped(w, m, v, sign, lr_t32, clip):
    """cem_adam_kernel's update of elements whose gradient is clipped to sign * clip, operation by operation in fp32."""
    g = (sign * F(clip)).astype(F)
    m2 = (m + ((g - m) * OB1).astype(F)).astype(F)
    v2 = (v + (((g * g).astype(F) - v) * OB2).astype(F)).astype(F)
    w2 = (w - ((lr_t32 * m2).astype(F) / (np.sqrt(v2).astype(F) + EPSILON).astype(F)).astype(F)).astype(F)
    return w2, m2, v2


def clip_masks(g64, clip):
    """(clipped, free): elements surely beyond the clip and surely inside it; the band between belongs to neither."""
    a = np.abs(g64)
    return a > clip * (1 + BAND), a < clip * (1 - BAND)


def gradient_bounds(g64, g32):
    """Per tensor (pooled over the members): (the fp32 NumPy oracle's own max |g32 - g64|, the bound the device is held to:
    max(8 x that, 1e-6 max |g64|)).  Two fp32 evaluations of one expression with different summation orders (BLAS; 4-wide MFMA k-chains
    plus per-part partials) have errors of one order, and the worst of ~1e4 elements varies by a few times.  Both maxima run over the
    WHOLE tensor, clipped elements included: a gradient's error follows the size of the terms summed, not of the sum, and an element
    inside the clip can be a cancelling sum of terms as large as a clipped element's.  The consequence: an element inside the clip is
    held to an absolute bound set by the tensor's largest raw gradient — for b_mu, whose raw gradients reach 4 to 30 here, at least
    4e-6 to 3e-5 whatever the element's own size."""
    out = {}
    for n in g64:
        own = float(np.abs(g32[n].astype(np.float64) - g64[n]).max())
        out[n] = (own, max(8.0 * own, 1e-6 * float(np.abs(g64[n]).max())))
    return out


def compare_step(name, got, prev, ref, g64, bounds, lr_t32, clip, report=None):
    """One Adam step of the device against the oracle.  got / prev: (w, m, v) flat() dicts read from the device after / before the step
    (fp32); ref: adam64 of prev and the fp64 gradient g64.
      * an element clipped for sure: m, v and w are cem_adam_kernel's fp32 arithmetic on +-clip bit for bit (from zero moments that is
        m == +-clip ob1, v == clip^2 ob2);
      * an element inside the clip: m within ob1 x bound of the reference (from zero moments: m / ob1 is the gradient within the bound),
        v within ob2 (2 |g| bound + bound^2) — the bound carried through g^2 — each plus the fp32 rounding of the moment update itself,
        2^-22 (|previous moment| + |its increment|), which vanishes from zero moments against the bound's floor;
      * every weight within 2e-5.
    Returns {tensor: worst (device gradient error) / (NumPy fp32 error)} and fills report[name]."""
    ratios = {}
    for n in g64:
        clipped, free = clip_masks(g64[n], clip)
        own, bound = bounds[n]
        (w1, m1, v1), (w0, m0, v0), (wr, mr, vr) = [[d[n] for d in s] for s in (got, prev, ref)]
        if clipped.any():
            w2, m2, v2 = adam32_clipped(w0[clipped], m0[clipped], v0[clipped], np.sign(g64[n][clipped]).astype(F), lr_t32, clip)
            for what, a, b in (('m', m1[clipped], m2), ('v', v1[clipped], v2), ('w', w1[clipped], w2)):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), '%s %s: %s of %d of %d clipped elements differs from the fp32 update on +-clip' % (
                    name, n, what, int((a != b).sum()), a.size)
        g, e_m, e_v = g64[n][free], np.abs(m1.astype(np.float64) - mr)[free], np.abs(v1.astype(np.float64) - vr)[free]
        tol_m = float(OB1) * bound + 2.0 ** -22 * (np.abs(m0[free]) + float(OB1) * np.abs(g))
        tol_v = float(OB2) * (2 * np.abs(g) * bound + bound ** 2) + 2.0 ** -22 * (np.abs(v0[free]) + float(OB2) * g * g)
        gerr = float((e_m / float(OB1)).max()) if free.any() else 0.0
        ratios[n] = gerr / own if own > 0 else 0.0
        print('%s %-6s clipped %5d free %6d  max|g| %.3g  gpu err %.3g  numpy32 err %.3g  ratio %.2f  bound %.3g' % (
            name, n, int(clipped.sum()), int(free.sum()), float(np.abs(g).max()) if free.any() else 0.0, gerr, own, ratios[n], bound))
        assert (e_m <= tol_m).all(), '%s %s: first moment off by %.3g x its bound (gradient error %.3g, NumPy fp32 %.3g)' % (name, n, float((e_m / tol_m).max()), gerr, own)
        assert (e_v <= tol_v).all(), '%s %s: second moment off by %.3g x its bound' % (name, n, float((e_v / tol_v).max()))
        werr = float(np.abs(w1.astype(np.float64) - wr).max())
        assert werr <= 2e-5, '%s %s: weights off by %.3g' % (name, n, werr)
    if report is not None:
        report[name] = ratios
    return ratios


def nll64(y, mu, var):
    return float(o.negative_log_likelihood(y.astype(np.float64), mu.astype(np.float64), var.astype(np.float64)))
