"""Device weight hand-over, the parts that need no GPU: the two C ABI additions (declared, exported, mirrored; nothing else of the ABI
moved), argument checks that return before any device call, the pack kernels in the device assembly, the destination -> source maps
those kernels implement restated in NumPy (tests/handover_cases.py) against the host packer, and the model classes' fall-back to
set_weights for planners that know nothing else."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ethz_safe_learning_amd import _capi, pack_weights_host
from ethz_safe_learning_amd.planner import flatten_weights, stage_model_weights, to_c_config
from tests import handover_cases as hc
from tests import helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['cem_planner_set_weights_dev', 'cem_trainer_weights_dev']


def test_new_symbols_are_declared_exported_and_listed(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    for name in NEW:
        assert re.search(r'\bint %s\s*\(' % name, hdr), name
        assert hasattr(built_lib, name) and name in _capi.EXPORTED_SYMBOLS, name


def test_abi_version_and_config_structs_are_unchanged(built_lib, tmp_path):
    assert built_lib.cem_abi_version() == 4 and _capi.CEM_ABI_VERSION == 4
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "cem_mpc.h"\nint main(void) { printf("%zu %zu %zu", sizeof(cem_config_t), '
                   'sizeof(cem_train_config_t), sizeof(cem_layout_t)); return 0; }\n')
    exe = tmp_path / 'sz'
    try:
        subprocess.run([os.environ.get('CC', 'cc'), '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True, capture_output=True)
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.fail('the header must compile as plain C: %r' % (getattr(e, 'stderr', e),))
    cfg_size, train_size, lay_size = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    # cem_config_t: 12 int32 + 4 float + int32 + float + 2 int32 + 4 x 32 float + the scorer (3 int32, 6 float, 2 int32, 3 x 4 words) + 7 int32
    assert cfg_size == C.sizeof(_capi.CemConfig) == 4 * (12 + 4 + 1 + 1 + 2 + 4 * 32 + (3 + 6 + 2 + 12) + 7)
    assert train_size == C.sizeof(_capi.CemTrainConfig) == 4 * 15
    assert lay_size == C.sizeof(_capi.CemLayout)                              # the layout grew at its end only: the mirror follows
    assert [n for n, _ in _capi.CemLayout._fields_][:10] == ['scores_local', 'scores_global', 'actions', 'mu_sigma', 'elite_idx', 'returns',
                                                              'costs', 'result', 'stamps', 'total']


def test_null_arguments_return_invalid_arg_without_a_device_call(built_lib):
    lib = built_lib
    buf = (C.c_float * 4)()
    ptr, n = C.c_void_p(), C.c_size_t()
    assert lib.cem_planner_set_weights_dev(None, buf, 4) == 1
    assert lib.cem_planner_set_weights_dev(None, None, 0) == 1
    assert lib.cem_trainer_weights_dev(None, C.byref(ptr), C.byref(n)) == 1


def test_pack_kernels_are_in_the_device_code_without_scratch_or_spills():
    meta = hp.kernel_meta(hp.device_assembly(), r'cem_pack_')
    names = {re.match(r'_Z\d+(cem_pack_\w+?_kernel)', k).group(1) for k in meta}
    assert names == {'cem_pack_fp32_kernel', 'cem_pack_split_kernel', 'cem_pack_wide_kernel', 'cem_pack_bias_kernel'}, sorted(meta)
    for name, d in meta.items():
        assert d['vgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, (name, d)


@pytest.mark.parametrize('case', sorted(hc.TUNED) + sorted(hc.SPLIT))
def test_numpy_restatement_of_the_maps_equals_the_host_packer(built_lib, case):
    """Every word of every member's image — the zero padding, the all-zero layer-0 blocks and the slack behind the last group
    included — is where the restatement puts it, for the tuned fp32 stream and for the three-plane bf16 stream."""
    cfg = hc.config(case)
    ws = hc.weights(cfg, seed=5, special=True)
    packed = pack_weights_host(cfg, ws).view(np.uint32).reshape(cfg.ensemble_size, -1)
    image = hc.image_split if cfg.precision == 'bf16x3' else hc.image_fp32
    for m, w in enumerate(ws):
        want = image(cfg, w)
        assert want.size == packed.shape[1]
        np.testing.assert_array_equal(packed[m], want, err_msg='member %d' % m)


def test_split_restatement_is_exact_at_its_edges():
    """x0 + x1 + x2 == x for the planted normal values (their sum is exact in fp64), pieces shrink by 2^-8 each, +-0 keep their sign in the
    first piece only, bf16-exact values have no second or third piece."""
    x = hc.SPECIAL[(np.abs(hc.SPECIAL) >= 2.0 ** -126) | (hc.SPECIAL == 0)]       # (below: the pieces of a denormal lose its last bits)
    p = [(a.astype(np.uint32) << 16).view(np.float32).astype(np.float64) for a in hc.split3(x)]
    np.testing.assert_array_equal(p[0] + p[1] + p[2], x.astype(np.float64))
    assert np.all(np.abs(p[1]) <= np.abs(x) * 2.0 ** -8) and np.all(np.abs(p[2]) <= np.abs(x) * 2.0 ** -16)
    a0, a1, a2 = hc.split3(np.array([0.0, -0.0, 1.5, -0.375], np.float32))
    assert a0.tolist() == [0x0000, 0x8000, 0x3FC0, 0xBEC0] and not a1.any() and not a2.any()


def test_wide_restatement_covers_every_group_once():
    for case in sorted(hc.WIDE):
        cfg = hc.config(case)
        D, O, U, L = cfg.obs_dim + cfg.act_dim, cfg.obs_dim, cfg.units, cfg.n_layers
        nbu, nbi, nbo = -(-U // 16), -(-D // 16), -(-O // 16)
        units = hc.units_wide(cfg)
        assert len(units) == len(set(units)) == nbi * nbu + (L - 1) * nbu * nbu + 2 * nbu * nbo


# ---- the model classes keep today's route for planners that only know set_weights --------------------------------------------------
class _OldPlanner:
    def __init__(self):
        self.weights = self.normaliser = None

    def set_weights(self, w):
        self.weights = w

    def set_normaliser(self, lo, hi):
        self.normaliser = (lo, hi)


class _Box:
    def __init__(self, n):
        self.low, self.high, self.shape = -np.ones(n, np.float32), np.ones(n, np.float32), (n,)


def _model():
    from ethz_safe_learning_amd.simba.models.transition_model import TransitionModel
    return TransitionModel('mlp_ensemble', _Box(6), _Box(2), scale_features=True, sampling_propagation=True, ensemble_size=2,
                           mlp_params=dict(n_layers=2, units=16, activation='tf.nn.relu', dropout_rate=0.0), seed=1)


def test_stand_in_planner_gets_its_weights_over_set_weights():
    tm = _model()
    assert tm.model.weights_device() is None                       # no trainer handle yet
    pl = tm._planner = _OldPlanner()
    assert tm._get_planner() is pl
    assert pl.weights is tm.model.get_weights() and pl.normaliser is not None
    # ... and through the policies' sync, whatever the ensemble says about device weights
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    pol = CemMpc.__new__(CemMpc)
    pol.model = tm
    pl2 = _OldPlanner()
    pl2.staged = None
    pol._sync_model(pl2)
    assert pl2.weights is tm.model.get_weights() and pl2.staged == (tm.uid, tm.version)

    class _Ens:
        def weights_device(self):
            raise AssertionError('a planner without set_weights_dev must not be offered device weights')

        def get_weights(self):
            return 'host'
    pl3 = _OldPlanner()
    stage_model_weights(pl3, _Ens())
    assert pl3.weights == 'host'


def test_blob_layout_is_the_trainers(built_lib):
    """flatten_weights' field order — W_0, b_0, ..., W_mu, b_mu, W_var, b_var per member — and the float count are what both
    cem_weight_blob_floats and cem_trainer_blob_floats give for one shape: a trainer's blob is a planner's blob."""
    cfg = hc.config(dict(obs_dim=60, act_dim=2, units=32, n_layers=2, ensemble_size=3, particles=3, n_samples=32))
    tc = _capi.CemTrainConfig(abi_version=4, inputs_dim=62, outputs_dim=60, units=32, n_layers=2, ensemble_size=3, batch_size=16,
                              activation=0, beta1=0.9, beta2=0.999, epsilon=1e-5, clipvalue=1.0)
    n = built_lib.cem_weight_blob_floats(C.byref(to_c_config(cfg)))
    assert n == built_lib.cem_trainer_blob_floats(C.byref(tc)) == flatten_weights(hc.weights(cfg)).size
