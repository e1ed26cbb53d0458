"""CPU-side checks of Adam's constants in the training ABI (cem_train_config_t: beta1, beta2, epsilon, clipvalue): cem_trainer_create
returns CEM_ERR_INVALID_ARG, and cem_trainer_workspace_bytes / cem_trainer_blob_floats 0, for a clipvalue or an epsilon that is not
finite and positive and for a beta outside [0, 1).  A clipvalue of 0 used to be accepted and zeroed every gradient.  No compute calls."""
import ctypes as C
import math

import pytest

from tests import helpers as hp

# (inputs_dim, outputs_dim, units, n_layers, ensemble_size, activation, dropout_rate): the shipped model, a swish net with dropout, one narrow member
SHAPES = [(62, 60, 128, 4, 15, 0, 0.0), (20, 17, 48, 2, 3, 7, 0.2), (8, 6, 17, 1, 1, 0, 0.0)]
INVALID_ARG = 1
_cfg = hp.train_config


def _status(lib, c):
    """(workspace bytes, blob floats, cem_trainer_create's status on a buffer that is large enough for nothing)."""
    h = C.c_void_p()
    buf = C.create_string_buffer(1024)
    return (lib.cem_trainer_workspace_bytes(C.byref(c)), lib.cem_trainer_blob_floats(C.byref(c)),
            lib.cem_trainer_create(C.byref(c), buf, 1024, None, C.byref(h)))


@pytest.mark.parametrize('field,value', [
    ('clipvalue', 0.0), ('clipvalue', -0.0), ('clipvalue', -1.0), ('clipvalue', math.inf), ('clipvalue', -math.inf), ('clipvalue', math.nan),
    ('epsilon', 0.0), ('epsilon', -1e-5), ('epsilon', math.inf), ('epsilon', math.nan),
    ('beta1', 1.0), ('beta1', -0.1), ('beta1', 1.5), ('beta1', math.nan), ('beta1', math.inf),
    ('beta2', 1.0), ('beta2', -1e-3), ('beta2', math.nan), ('beta2', -math.inf)])
def test_bad_adam_constants_are_refused(built_lib, field, value):
    for shape in SHAPES:
        c = _cfg(*shape, 64)
        setattr(c, field, value)
        assert _status(built_lib, c) == (0, 0, INVALID_ARG), (shape, field, value)


@pytest.mark.parametrize('field,value', [
    ('clipvalue', 1.0), ('clipvalue', 0.05), ('clipvalue', 1e-30), ('clipvalue', 1e30), ('clipvalue', 3.4028234663852886e38),
    ('epsilon', 1e-5), ('epsilon', 1e-12), ('epsilon', 1.0),
    ('beta1', 0.0), ('beta1', 0.9), ('beta1', 0.99999994), ('beta2', 0.0), ('beta2', 0.999)])
def test_good_adam_constants_pass(built_lib, field, value):
    """Among them the documented way to switch the clip off: a large finite clipvalue (include/cem_mpc.h)."""
    c = _cfg(*SHAPES[0], 64)
    want = built_lib.cem_trainer_workspace_bytes(C.byref(c))
    setattr(c, field, value)
    ws, blob, st = _status(built_lib, c)
    assert ws == want > 0 and blob > 0                   # the constants do not enter the layout
    assert st == 4, st                                   # CEM_ERR_WORKSPACE: validation passed, the 1 KB buffer is what is refused

