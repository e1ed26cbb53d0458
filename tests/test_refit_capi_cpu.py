"""The score-weighted refit (cem_planner_set_refit, CEM_REFIT_SOFTMAX), the parts of its C ABI that need no GPU: the symbols, what they
refuse without a handle, the new kernel's code-object metadata, and the policies' constructor defaults.
(tests/test_warm_capi_cpu.py::test_planning_kernels_keep_their_register_counts covers the other kernels: every one keeps its registers
with the new kernel present, whose name it admits.)"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from ethz_safe_learning_amd import _capi, planner
from tests import helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cem_planner_set_refit', 'cem_planner_get_refit', 'cem_planner_refit_stats')
INVALID_ARG = 1


def test_symbols_are_declared_exported_and_listed(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    for name in SYMBOLS:
        assert re.search(r'^int %s\(' % name, hdr, re.M), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert getattr(built_lib, name) is not None
    assert re.search(r'enum cem_refit \{ CEM_REFIT_UNIFORM = 0, CEM_REFIT_SOFTMAX = 1 \}', hdr)
    assert (_capi.CEM_REFIT_UNIFORM, _capi.CEM_REFIT_SOFTMAX) == (0, 1)
    assert planner.REFITS == {'uniform': 0, 'softmax': 1}
    assert re.search(r'#define CEM_ABI_VERSION 4\b', hdr) and built_lib.cem_abi_version() == 4


def test_null_handle_is_an_invalid_argument_and_writes_nothing(built_lib):
    for kind, tau in ((0, 0.0), (1, 0.5), (1, float('nan')), (1, 0.0), (1, -1.0), (1, float('inf')), (2, 1.0), (-1, 1.0)):
        assert built_lib.cem_planner_set_refit(None, kind, tau) == INVALID_ARG
    kind, tau = C.c_int32(7), C.c_float(7.0)
    assert built_lib.cem_planner_get_refit(None, C.byref(kind), C.byref(tau)) == INVALID_ARG
    assert (kind.value, tau.value) == (7, 7.0)
    out = np.full(4, 7.0, np.float32)
    assert built_lib.cem_planner_refit_stats(None, 0, out.ctypes.data_as(C.c_void_p), 4) == INVALID_ARG
    assert (out == 7.0).all()


def test_python_wrapper_refuses_an_unknown_kind_before_any_call():
    with pytest.raises(ValueError):
        planner.CemPlanner.set_refit(None, 'mppi', 1.0)               # (no handle is touched: the kind is checked first)


@pytest.fixture(scope='module')
def isa():
    return hp.device_assembly()


def test_refit_kernel_has_no_spills_and_no_scratch(isa):
    meta = hp.kernel_meta(isa, r'cem_constraint_refit_kernel')
    assert len(meta) == 1, list(meta)
    (name, d), = meta.items()
    assert hp.kernel_function_name(name) in hp.KERNELS_SINCE_WARM_START  # what test_planning_kernels_keep_their_register_counts admits
    assert d['vgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, d
    assert 0 < d['vgpr_count'] <= 128, d                               # a 1024-thread workgroup: at most 128 VGPRs a lane
    block = re.search(r'\.name:\s+%s\s*\n(.*?)(?=\n\s+- \.|\namdhsa\.target|\Z)' % re.escape(name), isa, re.S).group(0)
    assert re.search(r'\.sgpr_spill_count:\s+0\b', block), 'SGPRs spilled into vector lanes'
    body = hp.kernel_bodies(isa, r'cem_constraint_refit_kernel')[name]
    assert not any(re.match(r'(global|flat|ds|buffer)_atomic\w*_f(32|64)|ds_add_(rtn_)?f32', l) for l in body), 'no floating-point atomics'


def test_policy_constructor_defaults_are_none():
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    assert inspect.signature(CemMpc.__init__).parameters['elite_temperature'].default is None
    assert 'kwargs' in inspect.signature(SafeCemMpc.__init__).parameters                  # ... which SafeCemMpc passes through
    fields = planner.PlannerConfig.__dataclass_fields__
    assert fields['refit'].default == 'uniform' and fields['refit_temperature'].default == 0.0
