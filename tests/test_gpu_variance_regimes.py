"""The variance head var = softplus(v) + 1e-4 over its whole range, and Adam's gradient clip, on the device — against the fp64 oracle on
the ladder models of tests/variance_cases.py (whose claims tests/test_variance_cases_cpu.py checks without a GPU).

  a. the heads of every rollout family (cem_softplus4: hardware exp2 / rcp and a degree-4 polynomial) at H = 1;
  b. one training step from zero moments and a second one from the moments it left, on both training kernels (train_softplus, the
     NLL's gradients with the variance on its floor, cem_adam_kernel's clip), at clipvalue 1, 0.05 and 1e30;
  c. validation_loss and forward on both forms, var held to a RELATIVE bound (at the 1e-4 floor an absolute 5e-6 is a 5 % error bar).

The gradient bound of (b) is not a fixed number: vc.gradient_bounds builds it from the fp32 NumPy oracle's own error on the same inputs.
Setting CEM_VARIANCE_REPORT to a path makes the module write the worst values it measured there (scripts/variance_regimes_report.py)."""
import json
import os

import numpy as np
import pytest

from oracle import cem_oracle as o
from tests import helpers as hp
from tests import variance_cases as vc

pytestmark = pytest.mark.gpu

F = np.float32
FLOOR = F(1e-4)
REPORT = {'rollout_sd_rel_err_per_rung': {}, 'forward_var_rel_err_per_rung': {}, 'gradient_err_over_numpy32_err': {}}


@pytest.fixture(scope='module', autouse=True)
def _write_report():
    yield
    path = os.environ.get('CEM_VARIANCE_REPORT')
    if path:
        out = dict(ladder=[float(x) for x in vc.LADDER], **REPORT)
        with open(path, 'w') as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write('\n')


def _kernel(monkeypatch, kernel):
    # cem_trainer_create (training, validation) and cem_trainer_forward read the switch
    if kernel == 'gemm':
        monkeypatch.setenv('CEM_TRAIN_GEMM_KERNEL', '1')
    else:
        monkeypatch.delenv('CEM_TRAIN_GEMM_KERNEL', raising=False)


def _per_rung(rel, E, rows_of_member):
    """Worst of rel [rows, O] per rung; rows_of_member(m) selects member m's rows."""
    worst = np.zeros(vc.NR)
    for m in range(E):
        r = rel[rows_of_member(m)].max(axis=0)
        np.maximum.at(worst, vc.rungs(rel.shape[1], m), r)
    return worst


def _print_rungs(what, worst):
    print('%s, worst relative error per rung:' % what)
    print('   ' + '  '.join('%g: %.2g' % (v, e) for v, e in zip(vc.LADDER, worst)))


# ---- a. the rollouts' heads ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('O,A,E,L,units,precision', vc.ROLLOUT_CASES)
def test_rollout_heads_over_the_ladder(O, A, E, L, units, precision):
    import torch
    pb = vc.ladder_problem(O, A, E, L, units)
    _, pcfg = hp.configs(pb, N=16 * E, H=2, P=E, E=E, k=4, precision=precision)
    assert pcfg.precision == precision
    pl = hp.make_planner(pb, pcfg)
    s0, acts, eps = vc.rollout_inputs(pb, E)
    traj, mu, sd = pl.unfold_sequences(s0, acts, eps_model=eps, return_moments=True)
    torch.cuda.synchronize()
    traj, mu, sd = traj.cpu().numpy(), mu.cpu().numpy()[:, 0], sd.cpu().numpy()[:, 0]
    pl.close()
    m64, v64, _ = vc.rollout_reference(pb, E, s0, acts)
    sd64 = np.sqrt(v64)
    members = o.member_of_rows(s0.shape[0], E)
    worst = _per_rung(np.abs(sd - sd64) / sd64, E, lambda m: members == m)
    name = '%s (O %d, %d units)' % (precision if precision != 'fp32' else vc.ROLLOUT_FAMILY[(O, units)], O, units)
    _print_rungs('sd of the %s rollout' % name, worst)
    REPORT['rollout_sd_rel_err_per_rung'][name] = [float('%.3g' % x) for x in worst]
    np.testing.assert_array_equal(traj[:, 0], s0)
    np.testing.assert_allclose(mu, m64, atol=2e-6, rtol=1e-5)
    np.testing.assert_allclose(sd, sd64, atol=2e-6, rtol=1e-5)
    # s_1 = s_0 + mu + sd eps: the project's ATOL plus sd's relative allowance carried through mu + sd eps
    e64 = eps[0].astype(np.float64)
    ref1 = s0.astype(np.float64) + m64 + sd64 * e64
    err = np.abs(traj[:, 1] - ref1)
    allow = 5e-6 + 1e-5 * (np.abs(m64) + np.abs(sd64 * e64))
    print('s_1: max |gpu - f64| / allowance = %.3g' % (err / allow).max())
    assert (err <= allow).all(), float((err / allow).max())


# ---- b. the training step ----------------------------------------------------------------------------------------------------------------
def _train_params():
    for c in vc.TRAIN_CASES:
        for k in c[9]:
            yield pytest.param(*c[:9], k, id='%s-E%d-D%d-O%d-L%d-bt%d-u%d-%s-clip%g' % (k, c[0], c[1], c[2], c[3], c[4], c[5], c[6].split('.')[-1], c[8]))


@pytest.mark.parametrize('E,D,O,L,bt,units,act,batch_size,clip,kernel', list(_train_params()))
def test_training_steps_over_the_ladder(E, D, O, L, bt, units, act, batch_size, clip, kernel, monkeypatch):
    import torch
    from ethz_safe_learning_amd.trainer import CemTrainer
    _kernel(monkeypatch, kernel)
    pb = vc.ladder_problem(O, D - O, E, L, units, act)
    X, Y, perms, offs = vc.train_inputs(E, D, O, bt)
    tr = CemTrainer(D, O, units, L, E, batch_size=batch_size, activation=act, clipvalue=clip)
    tr.set_state(pb['weights'])
    x_dev, y_dev = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    weights = pb['weights']
    w0 = vc.flat(weights)
    prev = (w0, {n: np.zeros_like(a) for n, a in w0.items()}, {n: np.zeros_like(a) for n, a in w0.items()})
    case = '%s E%d D%d O%d L%d bt%d u%d %s clip%g' % (kernel, E, D, O, L, bt, units, act.split('.')[-1], clip)
    for t in (1, 2):                                    # from zero moments; then from the moments and weights the device holds
        off = offs[t - 1]
        idx = perms[t - 1][:, off:off + bt]
        loss_dev = torch.zeros(E, device='cuda')
        tr.step(x_dev, y_dev, torch.from_numpy(perms[t - 1]).cuda(), off, bt, vc.LR, loss_dev)
        tr.synchronize()
        loss64, g64 = vc.grads(weights, X, Y, idx, np.float64)
        _, g32 = vc.grads(weights, X, Y, idx, np.float32)
        g64, g32 = vc.flat(g64), vc.flat(g32)
        got_loss = float(loss_dev.sum().item())
        print('%s step %d: loss gpu %.9g f64 %.9g' % (case, t, got_loss, loss64))
        assert abs(got_loss - loss64) <= 1e-5 * abs(loss64), (t, got_loss, loss64)
        weights = tr.get_weights()
        if act != 'relu':
            for w in weights:
                w['activation'] = act
        gm, gv = tr.get_moments()
        got = (vc.flat(weights), vc.flat(gm), vc.flat(gv))
        if t == 1 and clip == 1.0:
            # every element beyond the clip holds m == +-(1 - beta1), v == 1 - beta2 bit for bit; and the clip is live
            n_clipped = 0
            for n in g64:
                clipped, _ = vc.clip_masks(g64[n], clip)
                n_clipped += int(clipped.sum())
                assert np.array_equal(got[1][n][clipped], (np.sign(g64[n][clipped]) * vc.OB1).astype(F)), n
                assert (got[2][n][clipped] == vc.OB2).all(), n
            assert (np.abs(g64['b_mu']) > 1).mean() >= 0.1 and n_clipped >= 20
        bounds = vc.gradient_bounds(g64, g32)
        ref = vc.adam64(prev[0], g64, prev[1], prev[2], vc.LR, t, clip)
        vc.compare_step('%s step %d' % (case, t), got, prev, ref, g64, bounds, vc.lr_t(vc.LR, t), clip, REPORT['gradient_err_over_numpy32_err'])
        prev = got
    if clip == 1e30:                                    # nothing was clipped: the raw gradient came through
        assert max(float(np.abs(a).max()) for a in g64.values()) > 1
        assert max(float(np.abs(a).max()) for a in got[1].values()) > float(vc.OB1) * 1.5
    tr.close()


# ---- c. validation_loss and forward ------------------------------------------------------------------------------------------------------
def _eval_params():
    for c in vc.EVAL_CASES:
        for k in c[6]:
            yield pytest.param(*c[:6], k, id='%s-E%d-D%d-O%d-L%d-u%d-%s' % (k, c[0], c[1], c[2], c[3], c[4], c[5].split('.')[-1]))


@pytest.mark.parametrize('E,D,O,L,units,act,kernel', list(_eval_params()))
def test_validation_loss_and_forward_over_the_ladder(E, D, O, L, units, act, kernel, monkeypatch):
    import torch
    from ethz_safe_learning_amd.trainer import CemTrainer
    _kernel(monkeypatch, kernel)
    pb = vc.ladder_problem(O, D - O, E, L, units, act)
    n = vc.EVAL_ROWS
    X, Y, _ = vc.training_data(D, O, n)
    tr = CemTrainer(D, O, units, L, E, batch_size=64, activation=act)
    tr.set_state(pb['weights'])
    x_dev, y_dev = torch.from_numpy(X).cuda(), torch.from_numpy(Y).cuda()
    w64 = o.cast_weights(pb['weights'], np.float64)
    vl = tr.validation_loss(x_dev, y_dev)
    ref_vl = float(o.validation_loss(w64, X.astype(np.float64), Y.astype(np.float64)))
    print('validation loss gpu %.9g f64 %.9g' % (vl, ref_vl))
    assert abs(vl - ref_vl) <= 1e-5 * abs(ref_vl), (vl, ref_vl)
    mu, var, sd = (t.cpu().numpy() for t in tr.forward(x_dev, map='all', want=('mu', 'var', 'sd')))
    assert mu.shape == var.shape == sd.shape == (E, n, O) and var.dtype == np.float32
    m64, v64 = o.ensemble_forward(np.tile(X.astype(np.float64), (E, 1)), w64, np.repeat(np.arange(E), n))
    m64, v64 = m64.reshape(E, n, O), v64.reshape(E, n, O)
    rel = (np.abs(var - v64) / v64).reshape(E * n, O)
    worst = _per_rung(rel, E, lambda m: slice(m * n, (m + 1) * n))
    name = '%s form, E%d D%d O%d L%d u%d %s' % ('tile' if kernel == 'tile' else 'generic', E, D, O, L, units, act.split('.')[-1])
    _print_rungs('var of forward (%s)' % name, worst)
    REPORT['forward_var_rel_err_per_rung'][name] = [float('%.3g' % x) for x in worst]
    assert (np.abs(var - v64) <= 1e-5 * v64).all(), float(rel.max())
    np.testing.assert_allclose(sd, np.sqrt(v64), rtol=1e-5, atol=0)
    assert (np.abs(mu - m64) <= 5e-6 * np.maximum(1.0, np.abs(m64))).all()                  # the bar of tests/test_gpu_ensemble_forward.py
    for m in range(E):
        r = vc.rungs(O, m)
        # exp(v) is below half an ulp of fl32(1e-4) from v = -26.4 down: the rungs <= -40 ARE the floor.  At -20, exp(v) = 2e-9 is ~280
        # ulps of 1e-4: there var is the correctly rounded sum within one ulp (v's own error of ~1e-6 moves exp(v) by 1e-15)
        floor = r <= vc.LADDER.index(-40)
        assert (var[m][:, floor] == FLOOR).all()
        at20 = r == vc.LADDER.index(-20)
        assert (np.abs(var[m][:, at20] - v64[m][:, at20].astype(F)) <= np.spacing(FLOOR)).all() and (var[m][:, at20] > FLOOR).all()
    # MlpEnsemble.forward's map (tf.split: row r to member r // (rows / E)) on the first 16 E rows: member m's rows are what the 'all'
    # map gave member m for the same inputs, bit for bit — the same kernels and epilogue under another row map
    mu_s, var_s, sd_s = (t.cpu().numpy() for t in tr.forward(x_dev[:16 * E], map='split', want=('mu', 'var', 'sd')))
    assert var_s.shape == (16 * E, O)
    for m in range(E):
        rows = slice(16 * m, 16 * (m + 1))
        for a, b in ((mu_s, mu), (var_s, var), (sd_s, sd)):
            np.testing.assert_array_equal(a[rows], b[m][rows])
    assert (np.abs(var_s - np.concatenate([v64[m][16 * m:16 * (m + 1)] for m in range(E)])) <= 1e-5 * np.concatenate([v64[m][16 * m:16 * (m + 1)] for m in range(E)])).all()
    # forward returns the var the loss used: the NLL recomputed in fp64 from the returned mu and var is validation_loss
    nll = float(np.mean([vc.nll64(Y, mu[m], var[m]) for m in range(E)]))
    print('NLL of forward %.9g, validation_loss %.9g' % (nll, vl))
    assert abs(nll - vl) <= 1e-6 * abs(vl), (nll, vl)
    tr.close()
