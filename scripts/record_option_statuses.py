"""Record what the option setters of a planner handle ANSWER, sequence by sequence: tests/golden/option_statuses.json.

The file is the behaviour of the library it was recorded from; tests/test_gpu_option_model.py runs this script again on the library
under test and requires the same answers.  One handle per kind, all at the smoke shape; between two sequences everything is switched
off again and each of those calls must return 0.  cem_planner_comm_init only ever ends a sequence: an admitted call goes on into RCCL,
so it is compared as "CEM_ERR_UNSUPPORTED or not" (its raw status is written too).  RCCL is tests/fakes/libfake_rccl.so, bound for the
whole process through CEM_RCCL_LIBRARY — hence a process of its own.  On the world-size-2 handle the second rank of an admitted
communicator is a thread that joins the stand-in's shared segment once rank 0 has made it.

    python scripts/record_option_statuses.py [--out tests/golden/option_statuses.json]
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
FAKE = os.path.join(ROOT, 'tests', 'fakes', 'libfake_rccl.so')

N, H, P, E, K, I = 128, 8, 5, 5, 12, 3
KINDS = [  # name, configs() keywords, problems of a batch handle (0: a single-state handle)
    ('cem', dict(variant='cem'), 0),
    ('safe', dict(variant='safe'), 0),
    ('cost', dict(variant='cost'), 0),
    ('select2', dict(variant='cem', select_mode=2), 0),
    ('select3', dict(variant='cem', select_mode=3), 0),
    ('world2', dict(variant='cem', world_size=2, rank=0), 0),
    ('batch2', dict(variant='cem'), 2),
]
ON = ['tail', 'budget', 'softmax', 'mixed', 'keep1', 'keep1x', 'keep12', 'pop32', 'pop13', 'mean', 'readout']
OFF = ['-tail', '-budget', '-softmax', '-mixed', '-keep', '-pop', '-mean', '-readout']
MOVES = ON + OFF
THREE_WAY = ['keep1', 'keep1x', 'keep12', '-keep', 'pop32', 'pop13', '-pop', 'mean', '-mean']   # elite x schedule x mean candidate
COMM = 'comm'


def sequences():
    """Every ordered pair of moves, every ordered triple of distinct elite / schedule / mean-candidate moves, and comm_init alone and
    behind every move."""
    seqs = [(a, b) for a in MOVES for b in MOVES]
    seqs += list(itertools.permutations(THREE_WAY, 3))
    seqs += [(COMM,)] + [(a, COMM) for a in MOVES]
    return seqs


class Handle:
    def __init__(self, pl):
        import numpy as np
        from ethz_safe_learning_amd import _capi, planner
        self.pl, self.lib, self.h, self._capi = pl, pl.lib, pl.h, _capi
        self.mix = np.ascontiguousarray(planner.mixing_matrix('ar1', 0.5, H), np.float32)
        self.fake = C.CDLL(FAKE)

    def _elite(self, n_keep, across=0):
        ec = self._capi.CemEliteCarry(n_keep=n_keep, across_plans=across, shift=1, reserved=0)
        return self.lib.cem_planner_set_elite_carry(self.h, C.byref(ec))

    def _pop(self, n):
        if n is None:
            return self.lib.cem_planner_set_population_schedule(self.h, None, 0)
        return self.lib.cem_planner_set_population_schedule(self.h, (C.c_int32 * len(n))(*n), len(n))

    def move(self, m):
        lib, h, c = self.lib, self.h, self._capi
        if m == 'tail': return lib.cem_planner_set_particle_objective(h, 1, 2)
        if m == '-tail': return lib.cem_planner_set_particle_objective(h, 0, 0)
        if m == 'budget': return lib.cem_planner_set_constraint(h, 1, 2)
        if m == '-budget': return lib.cem_planner_set_constraint(h, 0, 0)
        if m == 'softmax': return lib.cem_planner_set_refit(h, 1, 0.5)
        if m == '-softmax': return lib.cem_planner_set_refit(h, 0, 0.0)
        if m == 'mixed': return lib.cem_planner_set_action_noise(h, c.CEM_NOISE_MIXED, self.mix.ctypes.data_as(C.c_void_p))
        if m == '-mixed': return lib.cem_planner_set_action_noise(h, c.CEM_NOISE_WHITE, None)
        if m == 'keep1': return self._elite(1)
        if m == 'keep1x': return self._elite(1, 1)
        if m == 'keep12': return self._elite(12)
        if m == '-keep': return self._elite(0)
        if m == 'pop32': return self._pop([128, 64, 32])
        if m == 'pop13': return self._pop([128, 64, 13])
        if m == '-pop': return self._pop(None)
        if m == 'mean': return lib.cem_planner_set_mean_candidate(h, 1)
        if m == '-mean': return lib.cem_planner_set_mean_candidate(h, 0)
        if m == 'readout': return lib.cem_planner_set_plan_readout(h, 1)
        if m == '-readout': return lib.cem_planner_set_plan_readout(h, 0)
        if m == COMM: return self.comm()
        raise KeyError(m)

    def comm(self):
        """cem_planner_comm_init with the handle's own (world_size, rank); an admitted communicator is destroyed again."""
        cfg = self.pl.cfg
        buf = (C.c_char * self._capi.CEM_COMM_ID_BYTES)()
        assert self.lib.cem_comm_unique_id(buf) == 0
        returned, peers = threading.Event(), []
        for r in range(1, cfg.world_size):          # the other ranks: join once rank 0 has made the segment, never if the call is refused
            t = threading.Thread(target=self._peer, args=(bytes(buf.raw), cfg.world_size, r, returned), daemon=True)
            t.start()
            peers.append(t)
        st = self.lib.cem_planner_comm_init(self.h, buf, cfg.world_size, cfg.rank)
        returned.set()
        for t in peers:
            t.join()
        if st == 0:
            assert self.lib.cem_planner_comm_destroy(self.h) == 0
        return st

    def _peer(self, raw, world, rank, returned):
        class Id(C.Structure):
            _fields_ = [('internal', C.c_char * 128)]
        name = raw.split(b'\0', 1)[0].decode()
        while not os.path.exists('/dev/shm' + name):
            if returned.wait(0.0005):
                return
        comm, nid = C.c_void_p(), Id()
        C.memmove(C.byref(nid), raw, 128)
        self.fake.ncclCommInitRank.argtypes = [C.POINTER(C.c_void_p), C.c_int, Id, C.c_int]
        self.fake.ncclCommDestroy.argtypes = [C.c_void_p]
        if self.fake.ncclCommInitRank(C.byref(comm), world, nid, rank) == 0:
            self.fake.ncclCommDestroy(comm)

    def reset(self):
        for m in OFF:
            st = self.move(m)
            assert st == 0, ('switching off must always be admitted', m, st)


def record():
    os.environ['CEM_RCCL_LIBRARY'] = FAKE
    from ethz_safe_learning_amd import BatchCemPlanner, CemPlanner
    from tests import helpers as hp
    pb = hp.make_problem(seed=7)
    out = dict(shape=dict(N=N, H=H, P=P, E=E, k=K, I=I), moves=MOVES, compare_comm_as='2 (CEM_ERR_UNSUPPORTED) or not', kinds={})
    for name, kw, batch in KINDS:
        _, pcfg = hp.configs(pb, N=N, H=H, P=P, E=E, k=K, I=I, noise=0.01, post=0.3, **kw)
        pl = BatchCemPlanner(pcfg, batch) if batch else CemPlanner(pcfg)
        hd = Handle(pl)
        table = {}
        for seq in sequences():
            table['>'.join(seq)] = ''.join(str(hd.move(m)) for m in seq)
            hd.reset()
        out['kinds'][name] = dict(select_mode=pl.select_mode(), statuses=table)
        pl.close()
    return out


def comparable(rec):
    """The record as two libraries are compared: a final comm_init as 'U' (CEM_ERR_UNSUPPORTED) or 'a' (anything else)."""
    kinds = {}
    for name, kd in rec['kinds'].items():
        table = {}
        for seq, st in kd['statuses'].items():
            table[seq] = st[:-1] + ('U' if st[-1] == '2' else 'a') if seq.split('>')[-1] == COMM else st
        kinds[name] = dict(select_mode=kd['select_mode'], statuses=table)
    return kinds


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'option_statuses.json'))
    a = ap.parse_args()
    rec = record()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        json.dump(rec, f, indent=0, sort_keys=False)
        f.write('\n')
    seen = sorted({ch for kd in rec['kinds'].values() for st in kd['statuses'].values() for ch in st})
    print('recorded %d sequences on %d handle kinds; statuses seen: %s' % (len(sequences()), len(rec['kinds']), ' '.join(seen)))
