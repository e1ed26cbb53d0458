"""The inputs of tests/variance_cases.py do what they claim, and the fp32 NumPy oracle on them stays inside every bound that
tests/test_gpu_variance_regimes.py applies to the device.  No GPU."""
import numpy as np
import pytest

from oracle import cem_oracle as o
from tests import variance_cases as vc

F = np.float32
FLOOR = F(1e-4)


def test_ladder_holds_every_regime():
    lad = np.asarray(vc.LADDER)
    assert len(lad) == 17 and (np.diff(lad) > 0).all()
    assert abs(-vc.SWITCH - (np.log(float(np.finfo(F).eps)) + 2.0)) < 2e-6   # Eigen's fp32 threshold log(eps) + 2 (oracle.softplus_tf)
    assert (np.abs(lad) > 88).sum() == 3 and 0 in lad                          # expf(-v) overflows / exp2 underflows; v ~ 0
    var = o.softplus_tf(lad.astype(np.float64)) + 1e-4
    # exp(v) is below half an ulp of fl32(1e-4) (3.6e-12) from v = -26.4 down: the rungs <= -40 sit exactly on the floor, -20 does not
    # (exp(-20) = 2.1e-9 is 283 ulps of 1e-4)
    assert (var.astype(F)[lad <= -40] == FLOOR).all() and var.astype(F)[lad == -20][0] > FLOOR
    assert var.max() > 90


@pytest.mark.parametrize('O,A,E,L,units,precision', vc.ROLLOUT_CASES)
def test_rollout_inputs_reach_their_rungs(O, A, E, L, units, precision):
    pb = vc.ladder_problem(O, A, E, L, units)
    s0, acts, eps = vc.rollout_inputs(pb, E)
    mu, var, v = vc.rollout_reference(pb, E, s0, acts)
    members = o.member_of_rows(s0.shape[0], E)
    for m in range(E):
        vc.check_ladder(v[members == m], vc.rungs(O, m), straddle=False)
    assert var.min() < 1.0001e-4 and var.max() > 89.5
    # the fp32 NumPy oracle inside the device's bounds
    mu32, var32, _ = vc.rollout_reference(pb, E, s0, acts, np.float32)
    np.testing.assert_allclose(mu32, mu, atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(np.sqrt(var32), np.sqrt(var), atol=2e-6, rtol=1e-5)
    # half of var's 5e-7 plus one rounding of the square root
    assert (np.abs(np.sqrt(var32).astype(np.float64) / np.sqrt(var) - 1) <= 3.2e-7).all()


def _train_case(E, D, O, L, bt, units, act):
    pb = vc.ladder_problem(O, D - O, E, L, units, act)
    X, Y, perms, offs = vc.train_inputs(E, D, O, bt)
    idx = perms[0][:, offs[0]:offs[0] + bt]
    return pb, X, Y, idx


SHAPES = sorted(set(c[:7] for c in vc.TRAIN_CASES))


@pytest.mark.parametrize('E,D,O,L,bt,units,act', SHAPES)
def test_training_inputs_reach_their_rungs_and_the_clip(E, D, O, L, bt, units, act):
    pb, X, Y, idx = _train_case(E, D, O, L, bt, units, act)
    w64 = o.cast_weights(pb['weights'], np.float64)
    for m in range(E):
        v = vc.pre_softplus(X[idx[m]].astype(np.float64), w64, np.full(bt, m))
        vc.check_ladder(v, vc.rungs(O, m))
    loss64, g = vc.grads(pb['weights'], X, Y, idx, np.float64)
    loss32, g32 = vc.grads(pb['weights'], X, Y, idx, np.float32)
    g, g32 = vc.flat(g), vc.flat(g32)
    # the clip is live in b_mu in both signs, and not at all in the variance head: clipped and unclipped tensors side by side
    assert (g['b_mu'] > 1).mean() >= 0.05 and (g['b_mu'] < -1).mean() >= 0.05, ((g['b_mu'] > 1).mean(), (g['b_mu'] < -1).mean())
    assert np.abs(g['W_var']).max() <= 1 and np.abs(g['b_var']).max() <= 1
    allg = np.concatenate([np.abs(a).ravel() for a in g.values()])
    assert (np.abs(allg - 1) < vc.BAND).mean() <= 1e-3
    # the fp32 NumPy oracle: the loss within the device's bound, its own gradient error (the yardstick of the device's) small
    assert abs(float(loss32) - loss64) <= 1e-5 * abs(loss64)
    for n in g:
        own = np.abs(g32[n].astype(np.float64) - g[n]).max()
        print('%-6s max|g| %.3g  max|numpy32 - f64| %.3g (%.2g max|g|)' % (n, np.abs(g[n]).max(), own, own / np.abs(g[n]).max()))
        assert own <= 1e-6 * np.abs(g[n]).max(), (n, own, np.abs(g[n]).max())     # (measured: up to 6.1e-7, at 600 rows)
    # ... and through one Adam step it passes compare_step, second moment included: the device stood in for by the fp32 gradient
    # through Adam in fp64 on the device's constants (rounded to fp32), its clipped elements by cem_adam_kernel's fp32 arithmetic
    for clip in sorted(set(c[8] for c in vc.TRAIN_CASES if c[:7] == (E, D, O, L, bt, units, act))):
        w0 = vc.flat(pb['weights'])
        zero = {n: np.zeros_like(a) for n, a in w0.items()}
        prev = (w0, zero, zero)
        ref = vc.adam64(w0, g, zero, zero, vc.LR, 1, clip)
        got = tuple({n: a.astype(F) for n, a in d.items()} for d in vc.adam64(w0, g32, zero, zero, vc.LR, 1, clip))
        for n in g:
            clipped, _ = vc.clip_masks(g[n], clip)
            upd = vc.adam32_clipped(w0[n][clipped], zero[n][clipped], zero[n][clipped], np.sign(g[n][clipped]).astype(F), vc.lr_t(vc.LR, 1), clip)
            for d, a in zip(got, upd):
                d[n][clipped] = a
        vc.compare_step('numpy32 clip %g' % clip, got, prev, ref, g, vc.gradient_bounds(g, g32), vc.lr_t(vc.LR, 1), clip)


def test_a_small_clipvalue_is_live_in_the_hidden_layers():
    E, D, O, L, bt, units, act = 3, 62, 60, 4, 64, 128, 'relu'
    pb, X, Y, idx = _train_case(E, D, O, L, bt, units, act)
    g = vc.flat(vc.grads(pb['weights'], X, Y, idx, np.float64)[1])
    for l in range(L):
        for n in ('W%d' % l, 'b%d' % l):
            count = int((np.abs(g[n]) > 0.05 * (1 + vc.BAND)).sum())              # (measured: 0.2 % of W0 ... 61 % of b3)
            assert count >= 10 and (np.abs(g[n]) <= 1).all(), (n, count)           # ... and clipvalue=1.0 leaves them all alone
    assert max(np.abs(a).max() for a in g.values()) > 3                          # what clipvalue=1e30 lets through


@pytest.mark.parametrize('E,D,O,L,units,act,kernels', vc.EVAL_CASES)
def test_eval_inputs_reach_their_rungs(E, D, O, L, units, act, kernels):
    pb = vc.ladder_problem(O, D - O, E, L, units, act)
    X, Y, _ = vc.training_data(D, O, vc.EVAL_ROWS)
    w64, w32 = o.cast_weights(pb['weights'], np.float64), o.cast_weights(pb['weights'], np.float32)
    for m in range(E):
        members = np.full(vc.EVAL_ROWS, m)
        vc.check_ladder(vc.pre_softplus(X.astype(np.float64), w64, members), vc.rungs(O, m))
        mu, var = o.ensemble_forward(X.astype(np.float64), w64, members)
        mu32, var32 = o.ensemble_forward(X, w32, members)
        assert (np.abs(var32.astype(np.float64) - var) <= 5e-7 * var).all()
        assert (np.abs(np.sqrt(var32).astype(np.float64) - np.sqrt(var)) <= 3.2e-7 * np.sqrt(var)).all()
        floor = vc.rungs(O, m) <= vc.LADDER.index(-40)
        assert (var32[:, floor] == FLOOR).all() and (var32[:, ~floor] > FLOOR).all()
    ref = o.validation_loss(w64, X.astype(np.float64), Y.astype(np.float64))
    assert abs(float(o.validation_loss(w32, X, Y)) - ref) <= 1e-5 * abs(ref)
