"""The one task-scoring tile (csrc/cem_task_tile.h) without a GPU: the twelve kernels that the three units
compile from it do the memory and fp32 work that the three separate kernels did before they were folded into it."""
import json
import os
import re

import pytest

from tests import helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNITS = {'cem_task_score.hip': 'cem_task_score_kernel', 'cem_task_reference.hip': 'cem_task_reference_kernel',
         'cem_task_zones.hip': 'cem_task_zones_kernel'}


@pytest.mark.parametrize('unit', sorted(UNITS))
def test_the_folded_kernels_do_the_work_of_the_separate_ones(unit):
    """tests/golden/task_kernel_mnemonics.json was recorded from the three separate kernels, per function name and <NT, VEC>: the
    instruction count, and the count of every mnemonic that is a global or LDS access, a DPP move, a lane read or fp32 arithmetic
    (helpers.PINNED_MNEMONICS).  Each instantiation of the tile has those counts EXACTLY, and at most 1 % more instructions in all
    (scalar argument loads, waits and encodings may regroup: the one parameter block is the superset's for all three kinds)."""
    golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'task_kernel_mnemonics.json')))
    assert len(golden) == 12
    isa = hp.unit_assembly(unit)
    bodies = hp.kernel_bodies(isa, r'.')
    got = {hp.template_instance(name): hp.mnemonic_counts(body) for name, body in bodies.items()}
    assert sorted(got) == sorted(k for k in golden if k.startswith(UNITS[unit] + '<')) and len(got) == 4, sorted(got)
    for key, d in got.items():
        print(key, d['total'], golden[key]['total'])
        assert d['counts'] == golden[key]['counts'], (key, {m: (d['counts'].get(m), golden[key]['counts'].get(m))
                                                            for m in set(d['counts']) | set(golden[key]['counts'])
                                                            if d['counts'].get(m) != golden[key]['counts'].get(m)})
        assert d['total'] <= 1.01 * golden[key]['total'], (key, d['total'], golden[key]['total'])
    # products and sums are rounded separately; no atomics and no scratch anywhere in the unit
    for name, body in bodies.items():
        assert not any(re.match(r'v_(fma|fmac|mad|mac|pk_fma)_f32|\w*atomic|scratch_', line) for line in body), name


def test_the_tile_body_exists_once():
    """One body, three wrappers: the kernel headers hold no device statement of their own."""
    tile = open(os.path.join(hp.CSRC, 'cem_task_tile.h')).read()
    assert len(re.findall(r'void cem_task_rows\(', tile)) == 1 and tile.count('struct TaskParams') == 1
    for header, kernel in (('cem_task_score.h', 'cem_task_score_kernel'), ('cem_task_reference.h', 'cem_task_reference_kernel'),
                           ('cem_task_zones.h', 'cem_task_zones_kernel')):
        src = open(os.path.join(hp.CSRC, header)).read()
        code = src[src.index('#pragma once'):]
        assert re.search(r'void %s\(const TaskParams p\) \{ cem_task_rows<NT, VEC, CEM_TASK_KIND_\w+>\(p\); \}' % kernel, code), header
        assert '__shfl_xor' not in code and 'ballot' not in code and 'struct ' not in code, header
