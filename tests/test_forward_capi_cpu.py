"""CPU-side checks of the ensemble-inference entry point of the C ABI (cem_trainer_forward): the symbol is exported, declared in
include/cem_mpc.h and bound in _capi; the addition is additive — ABI version, cem_train_config_t and the trainer's workspace keep the
values they had before the entry point existed.  No compute calls."""
import ctypes as C
import os
import re

from ethz_safe_learning_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# measured on a build of the commit before cem_trainer_forward, for the shipped model (62 -> 4 x 128 -> 60, 15 members, batch 64)
PARENT_SIZEOF_TRAIN_CONFIG = 60
PARENT_WORKSPACE_BYTES_SHIPPED = 36593664
PARENT_WORKSPACE_BYTES_5_MEMBERS = 12198656


def _cfg(E):
    c = _capi.CemTrainConfig()
    c.abi_version = _capi.CEM_ABI_VERSION
    c.inputs_dim, c.outputs_dim, c.units, c.n_layers, c.ensemble_size = 62, 60, 128, 4, E
    c.batch_size, c.activation, c.dropout_rate = 64, 0, 0.0
    c.beta1, c.beta2, c.epsilon, c.clipvalue = 0.9, 0.999, 1e-5, 1.0
    return c


def test_forward_symbol_is_exported_declared_and_bound(built_lib):
    assert 'cem_trainer_forward' in _capi.EXPORTED_SYMBOLS
    fn = built_lib.cem_trainer_forward                    # AttributeError if the library does not export it
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    decl = re.search(r'int cem_trainer_forward\((.*?)\);', hdr, re.S)
    assert decl, 'cem_trainer_forward is not declared in include/cem_mpc.h'
    args = [a.strip() for a in re.sub(r'\s+', ' ', decl.group(1)).split(',')]
    assert args == ['cem_trainer_t *h', 'const float *x_dev', 'int32_t n_rows', 'int32_t map', 'const float *eps_dev', 'uint64_t seed',
                    'uint64_t call', 'float *mu_out_dev', 'float *var_out_dev', 'float *sd_out_dev', 'float *sample_out_dev']
    assert re.search(r'enum cem_forward_map \{ CEM_FORWARD_SPLIT = 0, CEM_FORWARD_ALL = 1 \};', hdr)
    assert (_capi.CEM_FORWARD_SPLIT, _capi.CEM_FORWARD_ALL) == (0, 1)
    # the header comment cites the reference lines the entry point replaces
    comment = hdr[:decl.start()].rsplit('/*', 1)[1]
    assert 'mlp_ensemble.py:122-132' in comment and ':189-193' in comment and ':150-154' in comment


def test_abi_version_config_struct_and_workspace_are_the_parents(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    assert re.search(r'#define CEM_ABI_VERSION 4\b', hdr) and _capi.CEM_ABI_VERSION == 4 and built_lib.cem_abi_version() == 4
    assert C.sizeof(_capi.CemTrainConfig) == PARENT_SIZEOF_TRAIN_CONFIG
    assert built_lib.cem_trainer_workspace_bytes(C.byref(_cfg(15))) == PARENT_WORKSPACE_BYTES_SHIPPED
    assert built_lib.cem_trainer_workspace_bytes(C.byref(_cfg(5))) == PARENT_WORKSPACE_BYTES_5_MEMBERS


def test_forward_refuses_bad_arguments_before_touching_the_device(built_lib):
    """The argument checks that need no handle: a NULL handle is CEM_ERR_INVALID_ARG whatever else is passed."""
    assert built_lib.cem_trainer_forward(None, None, 15, 0, None, 0, 0, None, None, None, None) == 1
