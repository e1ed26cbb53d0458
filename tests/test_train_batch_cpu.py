"""CPU-side checks of minibatches larger than 64 rows per member in the training ABI (cem_trainer_workspace_bytes,
cem_trainer_blob_floats): every batch_size up to CEM_TRAIN_MAX_BATCH gets a workspace, which never shrinks as the batch grows
and keeps its old size up to 64 rows; a larger batch_size is refused; the config struct and the ABI version stay.  No compute calls."""
import ctypes as C
import os
import re

import pytest

from ethz_safe_learning_amd import _capi
from tests import helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (inputs_dim, outputs_dim, units, n_layers, ensemble_size, activation, dropout_rate): the shipped model (62 -> 4 x 128 -> 60, 15
# members), 256 units, a swish net (its kept pre-activations enlarge the scratch) with dropout, one narrow member
SHAPES = [(62, 60, 128, 4, 15, 0, 0.0), (62, 60, 256, 3, 5, 0, 0.0), (20, 17, 48, 2, 3, 7, 0.2), (8, 6, 17, 1, 1, 0, 0.0)]
LARGE = (65, 100, 128, 256, 257, 1000, 4095, 4096)


def _cfg(D, O, U, L, E, act, rate, batch_size):
    return hp.train_config(D, O, U, L, E, act, rate, batch_size)


def _ws(lib, shape, batch_size):
    return lib.cem_trainer_workspace_bytes(C.byref(_cfg(*shape, batch_size)))


def _layout_up_to_64(D, O, U, L, E, act, rate):
    """The workspace of every batch_size <= 64, as it always was: weights, two Adam moments, four row parts' partial gradients and
    scratch, the per-member losses, four parts' loss partials and 256 B of phase stamps, each region 256-byte aligned."""
    nat = D * U + U + (L - 1) * (U * U + U) + 2 * (U * O + O)
    stride = 256 if U > 128 else 128
    scratch_pm = (L + 8 + (L if act in (7, 8) else 0)) * 16 * stride
    o = 0
    for nbytes in (nat * E * 4, nat * E * 4, nat * E * 4, ((nat * E + 3) & ~3) * 4 * 4, scratch_pm * E * 4 * 4, E * 4, E * 4 * 2 * 4, 256):
        o = (o + nbytes + 255) & ~255
    return o


@pytest.mark.parametrize('shape', SHAPES)
def test_workspace_covers_large_minibatches(built_lib, shape):
    sizes = [_ws(built_lib, shape, b) for b in LARGE]
    assert all(s > 0 for s in sizes), dict(zip(LARGE, sizes))
    assert all(b >= a for a, b in zip(sizes, sizes[1:])), dict(zip(LARGE, sizes))       # never shrinks as the batch grows
    small = _ws(built_lib, shape, 64)
    assert sizes[0] >= small
    # at most 32 row parts: beyond 512 rows the parts take several 16-row passes and the workspace stops growing
    assert _ws(built_lib, shape, 512) == _ws(built_lib, shape, 4096)
    assert _ws(built_lib, shape, 128) < _ws(built_lib, shape, 256) < _ws(built_lib, shape, 512)


@pytest.mark.parametrize('shape', SHAPES)
def test_workspace_up_to_64_rows_is_unchanged(built_lib, shape):
    want = _layout_up_to_64(*shape)
    for b in (1, 9, 16, 17, 37, 50, 63, 64):
        assert _ws(built_lib, shape, b) == want, b


@pytest.mark.parametrize('shape', SHAPES)
def test_batch_size_above_the_maximum_is_refused(built_lib, shape):
    top = _capi.CEM_TRAIN_MAX_BATCH
    assert top == 4096
    assert _ws(built_lib, shape, top) > 0
    for b in (top + 1, 2 * top, 1 << 20):
        assert _ws(built_lib, shape, b) == 0, b
        assert built_lib.cem_trainer_blob_floats(C.byref(_cfg(*shape, b))) == 0
        h = C.c_void_p()
        buf = C.create_string_buffer(1024)
        assert built_lib.cem_trainer_create(C.byref(_cfg(*shape, b)), buf, 1024, None, C.byref(h)) == 2      # CEM_ERR_UNSUPPORTED
    assert _ws(built_lib, shape, 0) == 0                                                                      # (CEM_ERR_INVALID_ARG)


@pytest.mark.parametrize('shape', SHAPES)
def test_blob_floats_do_not_depend_on_the_batch(built_lib, shape):
    D, O, U, L, E = shape[:5]
    nat = D * U + U + (L - 1) * (U * U + U) + 2 * (U * O + O)
    for b in (1, 64, 65, 256, 4096):
        assert built_lib.cem_trainer_blob_floats(C.byref(_cfg(*shape, b))) == nat * E, b


def test_config_struct_and_abi_version_stay():
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    assert re.search(r'#define CEM_ABI_VERSION 4\b', hdr) and _capi.CEM_ABI_VERSION == 4
    assert re.search(r'#define CEM_TRAIN_MAX_BATCH 4096\b', hdr) and _capi.CEM_TRAIN_MAX_BATCH == 4096
    body = re.search(r'typedef struct cem_train_config \{(.*?)\} cem_train_config_t;', hdr, re.S).group(1)
    fields = re.findall(r'\b(?:int32_t|uint32_t|float)\s+([^;]+);', re.sub(r'/\*.*?\*/', '', body, flags=re.S))
    names = [n.strip() for f in fields for n in f.split(',')]
    assert names == ['abi_version', 'inputs_dim', 'outputs_dim', 'units', 'n_layers', 'ensemble_size', 'batch_size', 'activation',
                     'dropout_rate', 'dropout_seed_lo', 'dropout_seed_hi', 'beta1', 'beta2', 'epsilon', 'clipvalue']
    assert C.sizeof(_capi.CemTrainConfig) == 15 * 4


def test_trainer_names_the_bound(built_lib):
    from ethz_safe_learning_amd.trainer import CemTrainer
    for b in (4097, 0):
        with pytest.raises(ValueError, match='4096'):
            CemTrainer(62, 60, 128, 4, 15, batch_size=b)
