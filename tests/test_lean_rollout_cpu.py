"""What the compiler made of csrc/cem_rollout_lean.hip (hipcc -S --cuda-device-only with the Makefile's own flags; no GPU): the unit
holds exactly the two lean kernels, they keep three workgroups per CU resident, the segmented one hands its state over like
cem_rollout_seg_kernel, and the step loop neither loads an action quad nor pays a second Philox call for the action it draws."""
import hashlib
import os
import re
import subprocess

import pytest

from tests import helpers as hp

LEAN = os.path.join(hp.CSRC, 'cem_rollout_lean.hip')
MAX_VGPRS = 168          # 512 / 168 = 3 waves per SIMD: B2's two pinned tiles plus one floating slot per CU


@pytest.fixture(scope='module')
def lean_isa():
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    h = hashlib.sha256()
    for f in sorted(os.listdir(hp.CSRC)):
        if f.endswith(('.h', '.hip')) or f == 'Makefile':
            h.update(open(os.path.join(hp.CSRC, f), 'rb').read())
    out = '/tmp/cem_lean_isa_%s.s' % h.hexdigest()[:16]
    if not os.path.exists(out):
        r = subprocess.run([hipcc] + hp.makefile_flags() + ['-S', '--cuda-device-only', '-o', out + '.tmp', LEAN], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + '.tmp', out)
    return open(out).read()


def _function_lines(isa, pattern):
    """{mangled name: [instruction and label lines]} (hp.kernel_bodies drops the labels, which the loop search needs)."""
    out = {}
    for m in re.finditer(r'^(_Z\w+):.*?\n(.*?)^\.Lfunc_end', isa, re.M | re.S):
        if re.search(pattern, m.group(1)):
            out[m.group(1)] = [l.split(';')[0].strip() for l in m.group(2).splitlines() if l.split(';')[0].strip()]
    return out


def _step_loop(lines):
    """The step loop of a rollout kernel: of the regions closed by a backward branch, the one with the most MFMAs (the smallest such)."""
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(':')}
    best = None
    for i, l in enumerate(lines):
        m = re.match(r's_c?branch\w*\s+(\.\w+)', l)
        if m and labels.get(m.group(1), len(lines)) < i:
            body = lines[labels[m.group(1)]:i + 1]
            n = sum(x.startswith('v_mfma') for x in body)
            if best is None or n > best[0] or (n == best[0] and len(body) < len(best[1])):
                best = (n, body)
    assert best and best[0] > 0
    return best[1]


def test_the_unit_holds_exactly_the_two_lean_kernels_within_their_register_budget(lean_isa):
    meta = hp.kernel_meta(lean_isa, r'.')
    assert sorted(hp.kernel_function_name(n) for n in meta) == ['cem_rollout_lean_kernel', 'cem_rollout_lean_seg_kernel'], sorted(meta)
    for name, d in meta.items():
        assert d['vgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, (name, d)
        assert d['vgpr_count'] <= MAX_VGPRS, (name, d)


def test_lean_segment_hand_over_drains_its_stores_before_the_flag(lean_isa):
    """As tests/test_isa_cpu.py asks of cem_rollout_seg_kernel: sc1 state stores, every wave's s_waitcnt vmcnt(0), the barrier, then the
    atomic ticket and the sc1 flag store."""
    bodies = hp.kernel_bodies(lean_isa, r'cem_rollout_lean_seg_kernel')
    assert len(bodies) == 1
    for name, ins in bodies.items():
        stores = [i for i, l in enumerate(ins) if l.startswith('buffer_store_dwordx4') and l.endswith('sc1')]
        assert stores, name
        last = stores[-1]
        bar = next(i for i in range(last, len(ins)) if ins[i].startswith('s_barrier'))
        between = ins[last + 1:bar]
        assert any(l.startswith('s_waitcnt') and 'vmcnt(0)' in l for l in between), (name, between)
        tail = ins[bar:]
        assert any(l.startswith('global_atomic_add') for l in tail) and any(l.startswith('global_store_dword') and 'sc1' in l for l in tail), name


def test_the_step_loop_loads_no_action_quad_and_draws_once(lean_isa):
    """The lean step loop runs TWO steps per round (compile-time exchange-buffer offsets), depth 4.  Per round its only 16-byte buffer
    loads are the weight groups (two per group: layer 0 has 4 groups, the three hidden layers and the heads 8 each) and the next
    layer's bias pair of the four dense layers — no action quad, which is the one further 16-byte load in the step loop of the generic
    one-chunk kernel cem_rollout_kernel<1, 1, 0> of csrc/cem_capi.hip.  And per step it multiplies no more often in Philox
    (v_mad_u64_u32) than the generic loop: the action is drawn by the call whose result the action lanes used to discard."""
    lean = _step_loop(next(iter(_function_lines(lean_isa, r'cem_rollout_lean_kernel').values())))
    generic_fn = _function_lines(hp.device_assembly(), r'cem_rollout_kernelILi1ELi1ELi0E')
    assert len(generic_fn) == 1, sorted(generic_fn)
    generic = _step_loop(next(iter(generic_fn.values())))

    def count(body, prefix):
        return sum(l.startswith(prefix) for l in body)
    groups = 4 + 3 * 8 + 8                                  # weight groups per step; 8 MFMAs and two 16-byte loads each
    steps = 2
    assert count(lean, 'v_mfma') == steps * groups * 8
    assert count(lean, 'buffer_load_dwordx4') == steps * (2 * groups + 2 * 4), count(lean, 'buffer_load_dwordx4')
    assert 0 < count(lean, 'v_mad_u64_u32') <= steps * count(generic, 'v_mad_u64_u32'), (count(lean, 'v_mad_u64_u32'), count(generic, 'v_mad_u64_u32'))
