"""Mixing matrices and shapes shared by the CPU and GPU tests of time-correlated action noise (cem_planner_set_action_noise,
CEM_NOISE_MIXED).

A transposed index, or a swap of t and u, is invisible to a symmetric M — which every power-law matrix is.  Hence the lower-triangular
AR(1) matrices, the time-reversal permutation and a seeded dense matrix with negative entries and one all-zero row.

Every non-zero entry has |M| >= 2^-60: a white draw is never below 2^-30 or so in magnitude where it is not zero, so no product is
subnormal and a flush-to-zero mode on either side cannot matter."""
import numpy as np

from ethz_safe_learning_amd.planner import ar1_mixing, powerlaw_mixing

F = np.float32
TINY = 2.0 ** -60

# (N, H, A, I) of the kernel-alone test
BASE_SHAPE = (37, 8, 2, 3)               # every matrix; N = 37 leaves a partial last group of sequences (256 / 8 = 32 per workgroup pass)
EXTRA_SHAPES = [
    (64, 1, 1, 1),                       # H = 1: M is one number
    (33, 3, 5, 2),                       # two action quads, the second partial; 256 / 3 = 85 sequences per pass, the last pass partial
    (16, 30, 12, 1),                     # three full quads; 256 / 30 = 8 sequences per pass and 16 idle threads
    (16, 128, 2, 1),                     # the H limit: two sequences per pass, 64 KB of M in LDS
]
MATRIX_NAMES = ('identity', 'ar1_0.5', 'ar1_0.9', 'powerlaw_0.5', 'powerlaw_2', 'powerlaw_4', 'reversal', 'dense')


def dense_matrix(H, seed=20):
    """Seeded, dense, both signs, entries of magnitude 1 / sqrt(H) or so, one all-zero row (H > 1: row H // 2)."""
    rng = np.random.default_rng(seed + H)
    M = (rng.standard_normal((H, H)) / np.sqrt(H)).astype(F)
    M[np.abs(M) < 1e-3] = F(0.25)                         # (nothing anywhere near 2^-60)
    if H > 1:
        M[H // 2] = 0
    return M


def matrix(name, H):
    """The named matrix at horizon H, float32, entries below 2^-60 in magnitude (an ifft's rounding residue) set to zero."""
    if name == 'identity':
        M = np.eye(H, dtype=F)
    elif name.startswith('ar1_'):
        M = ar1_mixing(H, float(name[4:]))
    elif name.startswith('powerlaw_'):
        M = powerlaw_mixing(H, float(name[9:]))
    elif name == 'reversal':
        M = np.eye(H, dtype=F)[::-1].copy()
    elif name == 'dense':
        M = dense_matrix(H)
    else:
        raise KeyError(name)
    M = np.ascontiguousarray(M, F)
    M[np.abs(M) < TINY] = 0
    return M


def mix_noise_scalar(M, xi):
    """The contract as a scalar Python loop over float32 values: the reference mix_noise is held to, bit for bit."""
    M, xi = np.asarray(M, F), np.asarray(xi, F)
    H = M.shape[0]
    flat = xi.reshape(-1, H, xi.shape[-1])
    out = np.zeros_like(flat)
    for s in range(flat.shape[0]):
        for a in range(flat.shape[2]):
            for t in range(H):
                acc = F(0.0)
                for u in range(H):
                    acc = F(acc + F(M[t, u] * flat[s, u, a]))
                out[s, t, a] = acc
    return out.reshape(xi.shape)
