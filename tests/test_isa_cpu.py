"""Build-time checks on the device ISA (no GPU): properties of the generated code that the memory model of the hand-over paths
depends on and that the compiler is free to break silently.  The kernels are compiled to assembly with the Makefile's own
flags (hipcc -S --cuda-device-only, ~25 s; cached under /tmp on the hash of the device sources)."""
import os
import re
import subprocess

import pytest

from tests import helpers as hp


@pytest.fixture(scope='module')
def isa():
    return hp.device_assembly()


def test_floating_segment_hand_over_drains_its_stores_before_the_flag(isa):
    """cem_rollout_seg_kernel: a tile's state crosses CUs (and XCDs, whose L2s are not coherent with each other) as sc1 stores
    followed by a flag.  Every wave must wait for the acknowledgement of ITS OWN stores (s_waitcnt vmcnt(0)) before the workgroup
    barrier that precedes the flag store: s_barrier does not drain stores on gfx940+, and a workgroup-scope fence compiles to no
    wait (round 2's code relied on both).  Checked for all eight <chunks, input blocks> instantiations."""
    bodies = hp.kernel_bodies(isa, r'cem_rollout_seg_kernel')
    assert len(bodies) == 8, sorted(bodies)
    for name, ins in bodies.items():
        stores = [i for i, l in enumerate(ins) if l.startswith('buffer_store_dwordx4') and l.endswith('sc1')]
        assert stores, name
        last = stores[-1]
        bar = next(i for i in range(last, len(ins)) if ins[i].startswith('s_barrier'))
        between = ins[last + 1:bar]
        assert any(l.startswith('s_waitcnt') and 'vmcnt(0)' in l for l in between), (name, between)
        # ... and the flag: an atomic ticket, then the sc1 flag store, after that barrier
        tail = ins[bar:]
        assert any(l.startswith('global_atomic_add') for l in tail) and any(l.startswith('global_store_dword') and 'sc1' in l for l in tail), name


def test_fused_select_grid_barrier_drains_before_arriving(isa):
    """cem_msel_fused_kernel: seven grid barriers; before each, every wave's sc1 stores / atomics are acknowledged
    (s_waitcnt vmcnt(0) directly before the workgroup barrier that precedes the arrival atomic)."""
    bodies = hp.kernel_bodies(isa, r'cem_msel_fused_kernel')
    assert len(bodies) == 1
    ins = next(iter(bodies.values()))
    # an arrival = the atomic add that is followed by the polling loop (sc1 load + s_sleep)
    arrivals = [i for i, l in enumerate(ins) if l.startswith('global_atomic_add') and any(x.startswith('s_sleep') for x in ins[i + 1:i + 40])]
    assert len(arrivals) >= 4, arrivals      # the phases in loops share code: at least the histogram loop, counts, compaction, moments loop
    for a in arrivals:
        bar = max(i for i in range(a) if ins[i].startswith('s_barrier'))
        assert a - bar < 20, (a, bar)
        prev = ins[max(0, bar - 3):bar]
        assert any(x.startswith('s_waitcnt') and 'vmcnt(0)' in x for x in prev), (a, prev)
    # the recovery form of the same body (one workgroup plays every slice): no arrivals, no polling — its phases are separated by
    # the workgroup's own barrier, each behind a drain of the wave's stores
    solo = hp.kernel_bodies(isa, r'cem_msel_solo_kernel')
    assert len(solo) == 1
    sins = next(iter(solo.values()))
    assert not any(l.startswith('s_sleep') for l in sins), 'the solo select must not poll'
    drained = [i for i, l in enumerate(sins) if l.startswith('s_barrier') and any(x.startswith('s_waitcnt') and 'vmcnt(0)' in x for x in sins[max(0, i - 3):i])]
    assert len(drained) >= 5, len(drained)       # zeroing, histogram loop, counts, compaction, moments loop


def test_split_rollout_kernels_fit_the_residency_their_tile_rule_assumes(isa):
    """cem_rollout_split_kernel (planning instantiations): no scratch, no spilled VGPRs, the products really are bf16 MFMAs, and the
    register counts the automatic tile sizes rest on (make_plan: up to 3 chunks at obs+act <= 64, 2 above — two resident workgroups,
    i.e. at most 256 VGPRs; a one-chunk tile of the small family keeps three, at most 170)."""
    meta = hp.kernel_meta(isa, r'cem_rollout_split_kernelILi\dELi\dELi0EE')
    assert len(meta) == 8, sorted(meta)
    for name, d in meta.items():
        rc, nfw = int(re.search(r'ILi(\d)ELi(\d)E', name).group(1)), int(re.search(r'ILi(\d)ELi(\d)E', name).group(2))
        if (nfw == 1 and rc <= 3) or (nfw == 2 and rc <= 2):          # the sizes make_plan picks by itself
            assert d['vgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, (name, d)
            assert d['vgpr_count'] <= (170 if (rc, nfw) == (1, 1) else 256), (name, d)
    m = re.search(r'^(_Z24cem_rollout_split_kernelILi1ELi1ELi0EEv13RolloutParams):.*?\n(.*?)^\.Lfunc_end', isa, re.M | re.S)   # (the kernel has an early s_endpgm)
    ins = [l.split(';')[0].strip() for l in m.group(2).splitlines() if l.strip() and not l.lstrip().startswith((';', '.'))]
    assert sum(1 for l in ins if l.startswith('v_mfma_f32_16x16x32_bf16')) >= 12 * (2 + 4 + 4), 'six products x two output blocks per chunk'
    assert not any(l.startswith('v_mfma_f32_16x16x4_f32') for l in ins), 'the split kernel must not fall back to fp32 MFMAs'
    assert any(l.startswith('v_cvt_pk_bf16_f32') for l in ins), 'the split rounds to nearest with the hardware conversion'


@pytest.mark.parametrize('kernel', hp.SCORE_KERNELS)
def test_score_kernels_stay_within_the_resources_they_had_as_separate_headers(isa, kernel):
    """csrc/cem_score.h composes the four score kernels from shared pieces.  tests/golden/score_kernel_resources.json holds, by function
    name, what the code-object metadata gave for each while it still was a copy of its own (the device sources of the commit before the
    header, these flags): no spills and no scratch, the same static LDS, and no more vector or scalar registers than then."""
    import json
    want = json.load(open(os.path.join(hp.ROOT, 'tests', 'golden', 'score_kernel_resources.json')))[kernel]
    meta = hp.kernel_meta(isa, r'^_Z\d+%s\d' % kernel, keys=tuple(want))
    assert len(meta) == 1, list(meta)
    (name, d), = meta.items()
    for k in ('vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size'):
        assert want[k] == 0 and d[k] == 0, (name, k, d)
    assert d['group_segment_fixed_size'] == want['group_segment_fixed_size'], (name, d, want)
    assert d['vgpr_count'] <= want['vgpr_count'] and d['sgpr_count'] <= want['sgpr_count'], (name, d, want)


@pytest.mark.parametrize('headers', [('cem_rollout_wide.h',), ('cem_rollout_split.h',), ('cem_rollout_wide.h', 'cem_rollout_split.h')],
                         ids=['wide_alone', 'split_alone', 'wide_then_split'])
def test_secondary_rollout_headers_stand_alone_and_in_either_order(headers, tmp_path):
    """cem_rollout_split.h and cem_rollout_wide.h take what they share with cem_rollout_tile from cem_rollout_common.h (file scope, every
    name an argument), not from macros another header happened to leave defined: each compiles alone, and wide-then-split — the order
    cem_capi.hip does NOT use — compiles too (it failed while the wide header undefined the macros the split header expands)."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    kernel = ('template __global__ void cem_rollout_split_kernel<1, 1, 0>(const RolloutParams);' if headers[-1] == 'cem_rollout_split.h'
              else 'template __global__ void cem_rollout_wide_kernel<0>(const WideParams);')
    tu = tmp_path / 'tu.hip'
    tu.write_text(''.join('#include "%s"\n' % h for h in headers) + kernel + '\n')
    r = subprocess.run([hipcc] + hp.makefile_flags() + ['--cuda-device-only', '-fsyntax-only', '-I', hp.CSRC, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
