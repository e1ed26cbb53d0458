"""Device weight hand-over on the GPU (cem_planner_set_weights_dev, csrc/cem_pack.h): every test builds two handles of one
configuration — H takes cem_planner_set_weights from the host, D takes the same weights from device memory — and holds D to H bit for
bit: the weight images, the bias arrays and the per-member table word by word, and whole plans.  D's workspace is filled with 0xFF
bytes before the handle is created, so a zero the pack kernels did not write shows up (H's zeros come out of the host packer's own
buffers).  Wide handles leave the three bias arrays alone on either route (their biases live in the table), so there H starts from
0xFF too."""
import ctypes as C

import numpy as np
import pytest

from tests import handover_cases as hc

pytestmark = pytest.mark.gpu

REGIONS = ('wpack', 'bias_h', 'bias_mu', 'bias_var', 'etab')


@pytest.fixture(scope='module')
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch


def _filled(cls):
    class Filled(cls):
        def _create(self, ws_ptr, nbytes, stream, out):
            self._ws_view.fill_(0xFF)
            self._torch.cuda.synchronize(self.device)
            super()._create(ws_ptr, nbytes, stream, out)
    return Filled


def _pair(cfg, max_batch=None, fill_host=False):
    from ethz_safe_learning_amd import BatchCemPlanner, CemPlanner
    base = CemPlanner if max_batch is None else BatchCemPlanner
    args = (cfg,) if max_batch is None else (cfg, max_batch)
    return (_filled(base) if fill_host else base)(*args), _filled(base)(*args)


def _dev(torch, ws):
    from ethz_safe_learning_amd.planner import flatten_weights
    return torch.from_numpy(flatten_weights(ws)).cuda()


def _assert_images_equal(H, D, what=''):
    h, d = H.weight_images(), D.weight_images()
    for k in REGIONS:
        assert h[k].size > 0
        np.testing.assert_array_equal(d[k], h[k], err_msg='%s %s' % (what, k))


def _normaliser(cfg, seed=3):
    rng = np.random.default_rng(seed)
    n = cfg.obs_dim + cfg.act_dim
    lo = rng.uniform(-2, -1, n).astype(np.float32)
    return lo, (lo + rng.uniform(2, 4, n)).astype(np.float32)


def _state(cfg, seed=4):
    return np.random.default_rng(seed).uniform(0.2, 0.9, cfg.obs_dim).astype(np.float32)


def _plan_bits(pl, state, seed=5, call=2):
    a, s, it = pl.plan(state, seed=seed, call=call)
    return a.view(np.uint32), np.float32(s).view(np.uint32), it, pl.mu_sigma().cpu().numpy().view(np.uint32)


def _assert_plans_equal(H, D, state, **kw):
    for x, y in zip(_plan_bits(H, state, **kw), _plan_bits(D, state, **kw)):
        np.testing.assert_array_equal(y, x)


# ---- images ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', sorted(hc.CASES))
def test_device_packed_images_equal_the_host_packed_ones(torch, case):
    cfg = hc.config(case)
    wide = case in hc.WIDE
    H, D = _pair(cfg, fill_host=wide)
    ws = hc.weights(cfg, seed=11, special=True)
    H.set_weights(ws)
    D.set_weights_dev(_dev(torch, ws))
    _assert_images_equal(H, D, case)
    img = H.weight_images()
    if wide:                                    # (the CPU suite holds the other two maps against cem_pack_weights_host, which packs no wide image)
        from ethz_safe_learning_amd.planner import flatten_weights
        blob = flatten_weights(ws).view(np.uint32)
        np.testing.assert_array_equal(img['wpack'][:blob.size], blob)
        images = img['wpack'][(blob.size * 4 + 255) // 256 * 64:].reshape(cfg.ensemble_size, -1)
        for m, w in enumerate(ws):
            np.testing.assert_array_equal(images[m], hc.image_wide(cfg, w))
    else:
        assert not any((v == 0xFFFFFFFF).any() for v in D.weight_images().values())      # nothing of the 0xFF fill is left in any region
    H.close(); D.close()


def test_batch_handle_images(torch):
    cfg = hc.config('obs63_act1')
    H, D = _pair(cfg, max_batch=4)
    ws = hc.weights(cfg, seed=12, special=True)
    H.set_weights(ws)
    D.set_weights_dev(_dev(torch, ws))
    _assert_images_equal(H, D)
    H.close(); D.close()


# ---- plans -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,case,kw', [
    ('cem_graph', 'tuned_nfw1', dict(use_graph=True)),
    ('safe_graph', 'tuned_nfw1', dict(use_graph=True, variant='safe', posterior_mean_threashold=0.3)),
    ('cem_eager', 'nfw2_obs100_act12', dict(use_graph=False)),
    ('safe_eager_split_members', 'split_members', dict(use_graph=False, variant='safe', posterior_mean_threashold=0.3)),
    ('bf16x3', 'bf16x3_nfw1', dict(use_graph=True)),
    ('bf16x3_nfw2', 'bf16x3_nfw2', dict(use_graph=False)),
    ('wide_relu', 'wide_u200_relu', dict(use_graph=True)),
    ('wide_tanh', 'wide_u128_tanh', dict(use_graph=False)),
], ids=lambda v: v if isinstance(v, str) else '')
def test_plans_are_bit_identical(torch, name, case, kw):
    cfg = hc.config(case, noise_stddev=0.01, smoothing=0.1, **kw)
    H, D = _pair(cfg, fill_host=case in hc.WIDE)
    ws, (lo, hi) = hc.weights(cfg, seed=21), _normaliser(cfg)
    H.set_weights(ws); H.set_normaliser(lo, hi)
    D.set_weights_dev(_dev(torch, ws)); D.set_normaliser(lo, hi)
    st = _state(cfg)
    _assert_plans_equal(H, D, st)
    _assert_plans_equal(H, D, st, call=3)                   # (a replay, where the first plan captured a graph)
    assert D.graph_status() == H.graph_status()
    assert H.graph_status() == 'graph' or not kw['use_graph'] or case in hc.WIDE
    H.close(); D.close()


def test_batch_plans_are_bit_identical(torch):
    cfg = hc.config('tuned_nfw1', use_graph=True, noise_stddev=0.01)
    H, D = _pair(cfg, max_batch=4)
    ws, (lo, hi) = hc.weights(cfg, seed=22), _normaliser(cfg)
    H.set_weights(ws); H.set_normaliser(lo, hi)
    D.set_weights_dev(_dev(torch, ws)); D.set_normaliser(lo, hi)
    states = np.stack([_state(cfg, seed=s) for s in range(4)])
    for x, y in zip(H.plan_batch(states, seed=9, calls=[4, 5, 6, 7]), D.plan_batch(states, seed=9, calls=[4, 5, 6, 7])):
        np.testing.assert_array_equal(np.ascontiguousarray(y).view(np.uint32), np.ascontiguousarray(x).view(np.uint32))
    H.close(); D.close()


def test_captured_graph_survives_a_hand_over(torch):
    cfg = hc.config('tuned_nfw1', use_graph=True)
    H, D = _pair(cfg)
    w1, w2, (lo, hi) = hc.weights(cfg, seed=31), hc.weights(cfg, seed=32), _normaliser(cfg)
    D.set_weights_dev(_dev(torch, w1)); D.set_normaliser(lo, hi)
    st = _state(cfg)
    D.plan(st, seed=1, call=0)
    assert D.graph_status() == 'graph'
    D.set_weights_dev(_dev(torch, w2))
    H.set_weights(w2); H.set_normaliser(lo, hi)
    _assert_plans_equal(H, D, st, seed=1, call=1)
    assert D.graph_status() == 'graph'
    H.close(); D.close()


# ---- the host mirror of the per-member table ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', ['tuned_nfw1', 'wide_u200_relu'])
@pytest.mark.parametrize('sequence', ['host_dev_norm', 'dev_norm_host_dev'])
def test_set_normaliser_does_not_bring_back_stale_biases(torch, case, sequence):
    """cem_planner_set_normaliser used to upload the whole host copy of the table, bias rows of the last HOST set_weights included."""
    cfg = hc.config(case)
    wide = case in hc.WIDE
    H, D = _pair(cfg, fill_host=wide)
    w1, w2, w3 = (hc.weights(cfg, seed=s) for s in (41, 42, 43))
    lo, hi = _normaliser(cfg)
    if sequence == 'host_dev_norm':
        D.set_weights(w1); D.set_weights_dev(_dev(torch, w2)); D.set_normaliser(lo, hi)
    else:
        D.set_weights_dev(_dev(torch, w2)); D.set_normaliser(lo, hi); D.set_weights(w3); D.set_weights_dev(_dev(torch, w2))
    H.set_weights(w2); H.set_normaliser(lo, hi)
    _assert_images_equal(H, D, sequence)
    _assert_plans_equal(H, D, _state(cfg))
    H.close(); D.close()


def test_host_only_calls_leave_the_table_as_before(torch):
    """set_normaliser now uploads its two rows only: after any order of host calls the device table is the host's full picture —
    normaliser rows from the last set_normaliser, bias rows from the last set_weights, the mask rows from create."""
    cfg = hc.config('obs63_act1')
    A, B = _pair(cfg)
    w1, w2 = hc.weights(cfg, seed=51), hc.weights(cfg, seed=52)
    n1, n2 = _normaliser(cfg, 1), _normaliser(cfg, 2)
    A.set_weights(w2); A.set_normaliser(*n2)
    B.set_normaliser(*n1); B.set_weights(w1); B.set_normaliser(*n2); B.set_weights(w2)
    _assert_images_equal(A, B)
    et = A.weight_images()['etab'].view(np.float32).reshape(cfg.ensemble_size, 8 + cfg.n_layers, 128)
    n = cfg.obs_dim + cfg.act_dim
    np.testing.assert_array_equal(et[:, 0, :n], np.broadcast_to(n2[0], (cfg.ensemble_size, n)))
    np.testing.assert_array_equal(et[:, 1, :n], np.broadcast_to(np.float32(1.0) / (n2[1] - n2[0]), (cfg.ensemble_size, n)))
    for m in range(cfg.ensemble_size):
        np.testing.assert_array_equal(et[m, 2, :cfg.obs_dim], w2[m]['b_mu'])
        np.testing.assert_array_equal(et[m, 8 + cfg.n_layers - 1, :cfg.units], w2[m]['b'][-1])
    A.close(); B.close()


# ---- trainer -> planner ------------------------------------------------------------------------------------------------------------
def test_trainer_blob_goes_to_the_planner_without_the_host(torch):
    from ethz_safe_learning_amd.trainer import CemTrainer
    cfg = hc.config(dict(units=32, n_layers=2, ensemble_size=3, particles=3))
    E, D_in, O = 3, 62, 60
    tr = CemTrainer(D_in, O, 32, 2, E, batch_size=16)
    tr.set_state(hc.weights(cfg, seed=61))
    rng = np.random.default_rng(62)
    x = torch.from_numpy(rng.normal(0, 1, (48, D_in)).astype(np.float32)).cuda()
    y = torch.from_numpy(rng.normal(0, 1, (48, O)).astype(np.float32)).cuda()
    perm = torch.from_numpy(np.stack([rng.permutation(48) for _ in range(E)]).astype(np.int32)).cuda()
    loss = torch.zeros((3, E), dtype=torch.float32, device='cuda')
    before = tr.weights_dev().clone()
    for s in range(3):                                          # three Adam steps; nothing synchronises before the hand-over
        tr.step(x, y, perm, 16 * s, 16, 1e-2, loss[s])
    H, D = _pair(cfg)
    D.set_weights_from(tr)
    view = tr.weights_dev()
    assert view.data_ptr() == tr.weights_dev().data_ptr() and view.numel() == tr.lib.cem_trainer_blob_floats(C.byref(tr.ccfg))
    assert tr._ws_view.data_ptr() <= view.data_ptr() < tr._ws_view.data_ptr() + tr._ws_view.numel()      # a view of the workspace, no copy
    trained = tr.get_weights()
    assert not torch.equal(before, tr.weights_dev())            # the steps moved the weights
    H.set_weights(trained)
    _assert_images_equal(H, D)
    from ethz_safe_learning_amd.planner import flatten_weights
    np.testing.assert_array_equal(view.cpu().numpy(), flatten_weights(trained))    # a member's block has the planner's field order
    H.close(); D.close(); tr.close()


class _Box:
    def __init__(self, lo, hi):
        self.low, self.high, self.shape = np.asarray(lo, np.float32), np.asarray(hi, np.float32), (len(lo),)


def _transition_model(seed=1):
    from ethz_safe_learning_amd.simba.models.transition_model import TransitionModel
    return TransitionModel('mlp_ensemble', _Box([-2.0] * 20, [2.0] * 20), _Box([-1.0] * 2, [1.0] * 2), scale_features=True,
                           sampling_propagation=True, ensemble_size=3, batch_size=16, training_steps=6, validation_split=0.0,
                           mlp_params=dict(n_layers=2, units=32, activation='tf.nn.relu', dropout_rate=0.0), seed=seed)


def test_weights_device_is_never_stale(torch):
    tm = _transition_model()
    ens = tm.model
    assert ens.weights_device() is None                         # no trainer handle before the first fit / set_weights
    rng = np.random.default_rng(71)
    x = rng.uniform(-1, 1, (64, 22)).astype(np.float32)
    np.random.seed(5)
    tm.fit(x, x[:, :20] + 0.1 * rng.normal(0, 1, (64, 20)).astype(np.float32))
    from ethz_safe_learning_amd.planner import flatten_weights
    dev = ens.weights_device()
    np.testing.assert_array_equal(dev.cpu().numpy(), flatten_weights(ens.get_weights()))
    other = hc.weights(hc.config(dict(obs_dim=20, act_dim=2, units=32, n_layers=2, ensemble_size=3, particles=3)), seed=72)
    ens.set_weights(other)
    dev = ens.weights_device()                                  # refreshed or None, never the fitted weights
    assert dev is None or np.array_equal(dev.cpu().numpy(), flatten_weights(other))
    ens.forward(np.zeros((3, 22), np.float32))                  # an inference call re-stages the trainer
    np.testing.assert_array_equal(ens.weights_device().cpu().numpy(), flatten_weights(other))


def test_fitted_model_unfolds_as_one_synced_over_the_host(torch):
    tm = _transition_model()
    rng = np.random.default_rng(81)
    x = rng.uniform(-1, 1, (64, 22)).astype(np.float32)
    np.random.seed(6)
    tm.fit(x, x[:, :20] + 0.1 * rng.normal(0, 1, (64, 20)).astype(np.float32))
    assert tm.model.weights_device() is not None
    s0 = rng.uniform(-1, 1, (6, 20)).astype(np.float32)
    acts = rng.uniform(-1, 1, (6, 4, 2)).astype(np.float32)
    eps = rng.normal(0, 1, (4, 6, 20)).astype(np.float32)
    got = tm.unfold_sequences(s0, acts, eps_model=eps).cpu().numpy()
    assert tm._planner.have_device_weights
    old = _transition_model()                                   # the same weights and statistics, staged the old way
    old.model.set_weights(tm.model.get_weights())
    old.inputs_min, old.inputs_max = tm.inputs_min, tm.inputs_max
    assert old.model.weights_device() is None
    want = old.unfold_sequences(s0, acts, eps_model=eps).cpu().numpy()
    assert not old._planner.have_device_weights
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))
    _assert_images_equal(old._planner, tm._planner)


# ---- carry and argument errors -------------------------------------------------------------------------------------------------------
def test_warm_start_carry_is_kept(torch):
    cfg = hc.config('tuned_nfw1')
    _, D = _pair(cfg)
    D.set_weights_dev(_dev(torch, hc.weights(cfg, seed=91)))
    D.plan(_state(cfg), seed=1, call=0)
    mu, sg, valid = D.carry()
    assert valid
    D.set_weights_dev(_dev(torch, hc.weights(cfg, seed=92)))
    mu2, sg2, valid2 = D.carry()
    assert valid2
    np.testing.assert_array_equal(mu2.view(np.uint32), mu.view(np.uint32))
    np.testing.assert_array_equal(sg2.view(np.uint32), sg.view(np.uint32))
    D.close()


def test_argument_errors_leave_the_handle_usable(torch):
    cfg = hc.config('tuned_nfw1')
    H, D = _pair(cfg)
    ws = hc.weights(cfg, seed=93)
    blob = _dev(torch, ws)
    lib = D.lib
    assert lib.cem_planner_set_weights_dev(D.h, C.c_void_p(blob.data_ptr()), blob.numel() - 1) == 1
    assert lib.cem_planner_set_weights_dev(D.h, None, blob.numel()) == 1
    with pytest.raises(Exception) as e:
        D.plan(_state(cfg))                                     # neither call counted as a weight sync
    assert getattr(e.value, 'status', None) == 6
    with pytest.raises(ValueError):
        D.set_weights_dev(blob.cpu())
    with pytest.raises(ValueError):
        D.set_weights_dev(blob.double())
    D.set_weights_dev(blob)
    H.set_weights(ws)
    _assert_plans_equal(H, D, _state(cfg))
    H.close(); D.close()
