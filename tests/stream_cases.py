"""The instrument of tests/test_gpu_stream_order.py: a bounded busy kernel to make a producer late or a handle's stream busy, a probe
that two streams really run side by side, and the two harnesses every ordering contract is checked with.

Nothing here is a tolerance.  A reference is the same call on the same handle with its input supplied synchronously; a second reference
with a decoy input must differ from it (else a missing wait could not show); the result under test must equal the first bit for bit.

delay lengths: max(MIN_MS, FACTOR x the consumer call's own duration, measured with events on the idle handle), capped at CAP_MS — long
against the call, short against a test run, never long enough to look like a hang.  The calibration and every chosen length are printed
and, at the end of the module, written to profiles/stream_order.txt (write_report)."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = os.path.join(ROOT, 'profiles', 'stream_order.txt')
MIN_MS, FACTOR, CAP_MS = 20.0, 20.0, 250.0
PROBE_STREAMS = 8

_lines = []
_cal = {}


def log(line):
    print(line)
    _lines.append(line)


def write_report(path=REPORT):
    """What log() collected -> profiles/stream_order.txt (a checkout that cannot be written to keeps the printed copy)."""
    if not _lines:
        return
    try:
        with open(path, 'w') as f:
            f.write('\n'.join(_lines) + '\n')
    except OSError:
        pass


# ---- the busy kernel ---------------------------------------------------------------------------------------------------------------
def event_ms(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    out = fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def calibrate():
    """Once per session: ('sleep', cycles per ms) from one timed torch.cuda._sleep, or ('matmul', ms per 4096^2 matmul) without it."""
    if _cal:
        return _cal
    import torch
    s = torch.cuda.Stream()
    if hasattr(torch.cuda, '_sleep'):
        def spin(c):
            with torch.cuda.stream(s):
                torch.cuda._sleep(c)
        cycles = 1000000
        event_ms(s, lambda: spin(cycles))                        # (first launch: module load)
        for _ in range(6):                                          # a call long enough to time: at least 5 ms, found by growing it
            ms, _ = event_ms(s, lambda: spin(cycles))
            if ms >= 5.0 or ms * 8 > CAP_MS:
                break
            cycles *= 8
        _cal.update(kind='sleep', per_ms=cycles / ms, timed_cycles=cycles, timed_ms=ms)
        log('calibration: torch.cuda._sleep(%d) took %.3f ms -> %.0f cycles per ms' % (cycles, ms, cycles / ms))
    else:
        a = torch.ones((4096, 4096), dtype=torch.float32, device='cuda')
        b = torch.empty_like(a)

        def chain(n):
            with torch.cuda.stream(s):
                for _ in range(n):
                    torch.mm(a, a, out=b)
        event_ms(s, lambda: chain(1))
        ms, _ = event_ms(s, lambda: chain(4))
        _cal.update(kind='matmul', per_ms=4 / ms, a=a, b=b, chain=chain)
        log('calibration: four 4096^2 fp32 matmuls took %.3f ms -> %.3f matmuls per ms' % (ms, 4 / ms))
    return _cal


def delay_ms(call_ms):
    """The length for a consumer call that takes call_ms on the idle handle."""
    return min(CAP_MS, max(MIN_MS, FACTOR * float(call_ms)))


def delay(stream, ms, what=None):
    """Queue a busy kernel of about `ms` milliseconds (never more than CAP_MS) on `stream`; `what` notes a length no harness chose."""
    import torch
    cal = calibrate()
    ms = min(float(ms), CAP_MS)
    if what:
        log('delay %s: %.1f ms (set by the test: the floor where the consumer is a copy of microseconds)' % (what, ms))
    with torch.cuda.stream(stream):
        if cal['kind'] == 'sleep':
            torch.cuda._sleep(int(ms * cal['per_ms']))
        else:
            for _ in range(max(1, int(np.ceil(ms * cal['per_ms'])))):
                torch.mm(cal['a'], cal['a'], out=cal['b'])


def late(tensor, true, decoy, stream, ms):
    """`tensor` holds `decoy` now and `true` only once a delay of `ms` on `stream` has run: the caller invokes the API under test next,
    with nothing that synchronises with the host in between."""
    import torch
    tensor.copy_(decoy)
    torch.cuda.synchronize()
    delay(stream, ms)
    with torch.cuda.stream(stream):
        tensor.copy_(true)


# ---- the sightedness probe -----------------------------------------------------------------------------------------------------------
def concurrent(producer, consumer):
    """True iff work on `consumer` runs while `producer` is busy: two torch streams may share one of the process's few hardware queues
    and serialise, and a missing wait between them is then invisible."""
    import torch
    flag = torch.zeros(1, dtype=torch.int32, device='cuda')
    out = torch.full((1,), -1, dtype=torch.int32, device='cuda')
    torch.cuda.synchronize()
    delay(producer, MIN_MS)
    with torch.cuda.stream(producer):
        flag.fill_(1)
    with torch.cuda.stream(consumer):
        out.copy_(flag)                                             # no wait: sees 0 unless the streams serialise
    torch.cuda.synchronize()
    return int(out.item()) == 0


def _fresh_side(ok, what, role):
    import torch
    for i in range(PROBE_STREAMS):
        s = torch.cuda.Stream()
        if ok(s):
            log('probe %s: %s stream %d of %d is concurrent' % (what, role, i + 1, PROBE_STREAMS))
            return s
    pytest.fail('%s: none of %d fresh %s streams runs concurrently with the handle\'s stream (they share a hardware queue): '
                'the ordering test would be blind' % (what, PROBE_STREAMS, role))


def producer_for(consumer, what):
    """A fresh stream whose work the consumer stream does not implicitly wait for (fails the test if 8 tries find none)."""
    return _fresh_side(lambda s: concurrent(s, consumer), what, 'producer')


def consumer_for(producer, what):
    """A fresh stream that runs while `producer` is busy."""
    return _fresh_side(lambda s: concurrent(producer, s), what, 'consumer')


def handle_beside(make, is_concurrent, what):
    """make() until is_concurrent(handle) holds — for contracts between two handles' own streams, where neither side can be swapped for
    a fresh torch stream.  The handles that did not fit are closed."""
    for i in range(PROBE_STREAMS):
        h = make()
        if is_concurrent(h):
            log('probe %s: handle %d of %d has a concurrent stream' % (what, i + 1, PROBE_STREAMS))
            return h
        h.close()
    pytest.fail('%s: none of %d handles got a stream concurrent with its partner\'s: the ordering test would be blind' % (what, PROBE_STREAMS))


# ---- bit-exact comparison --------------------------------------------------------------------------------------------------------------
def bits(x):
    """x (a tensor, an array, a scalar or a nest of them) as raw bytes on the host.  Call after a device synchronise."""
    import torch
    if isinstance(x, (tuple, list)):
        return tuple(bits(v) for v in x)
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(x))
    return a.reshape(-1).view(np.uint8).copy()


def same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    return a.shape == b.shape and bool(np.array_equal(a, b))


def assert_same(got, ref, what=''):
    if isinstance(ref, tuple):
        assert len(got) == len(ref), what
        for i, (g, r) in enumerate(zip(got, ref)):
            assert_same(g, r, '%s[%d]' % (what, i))
        return
    np.testing.assert_array_equal(got, ref, err_msg=what)


def grab(x):
    """An immediate copy on the current stream of every tensor in x (the early consumer); host values pass through."""
    import torch
    if isinstance(x, (tuple, list)):
        return [grab(v) for v in x]
    return x.clone() if torch.is_tensor(x) else x


def poison(specs):
    """Fill and free tensors of the given (shape, dtype) on the current stream: the next torch.empty of that size gets 0xFF bytes, not
    the last run's (correct) values."""
    import torch
    ts = [torch.empty(shape, dtype=dtype, device='cuda') for shape, dtype in specs]
    for t in ts:
        t.view(torch.uint8).fill_(0xFF)
    torch.cuda.synchronize()
    del ts


# ---- the two harnesses -----------------------------------------------------------------------------------------------------------------
def check_late_input(handle_stream, buf, true, decoy, call, what, prepare=None):
    """Contract (A): `call()` hands `buf` to a handle whose stream is `handle_stream`, from a current stream on which `buf` is still
    being produced.  call() returns host values or tensors that are complete once the device is idle."""
    import torch
    side = producer_for(handle_stream, what)
    with torch.cuda.stream(side):
        refs = []
        for src in (decoy, true):                                   # (the decoy first: the timed call launches nothing for the first time)
            buf.copy_(src)
            if prepare:
                prepare()
            ms, r = event_ms(handle_stream, call)
            refs.insert(0, bits(r))
        d = delay_ms(ms)
        log('delay %s: the call takes %.3f ms on the idle handle -> %.1f ms' % (what, ms, d))
        assert not same(refs[0], refs[1]), '%s: the decoy input gives the true input\'s result, a missing wait could not show' % what
        if prepare:
            prepare()
        late(buf, true, decoy, side, d)
        r = call()
        torch.cuda.synchronize()
        assert_same(bits(r), refs[0], what)


def check_early_output(handle_stream, call, what, poisoned=()):
    """Contract (B): `handle_stream` is busy when `call()` is made; what it returns is copied at once on the current stream."""
    import torch
    side = consumer_for(handle_stream, what)
    with torch.cuda.stream(side):
        call()                                                      # (warm-up: the timed call launches nothing for the first time)
        ms, r = event_ms(handle_stream, lambda: grab(call()))
        ref = bits(r)
        del r
        d = delay_ms(ms)
        log('delay %s: the call takes %.3f ms on the idle handle -> %.1f ms' % (what, ms, d))
        poison(poisoned)
        delay(handle_stream, d)
        got = grab(call())
        torch.cuda.synchronize()
        assert_same(bits(got), ref, what)


# ---- the polled return (contract E), in this process or in a child with CEM_NO_POLL set ---------------------------------------------------
GENERIC = dict(obs_dim=17, act_dim=2, E=2, n_layers=2, units=32)
GENERIC_PLAN = dict(N=64, H=4, P=2, E=2, k=8, I=2)
LEAN = dict(obs_dim=60, act_dim=2, E=5, n_layers=4, units=128)
LEAN_PLAN = dict(N=64, H=5, P=5, E=5, k=8, I=2)


def lean_planner(seed=101, **extra):
    """(problem, planner) of the lean shape: a captured graph, hence the polled return."""
    import dataclasses
    from tests import helpers as hp
    pb = hp.make_problem(seed=seed, **LEAN)
    _, pcfg = hp.configs(pb, use_graph=True, **LEAN_PLAN)
    return pb, hp.make_planner(pb, dataclasses.replace(pcfg, **extra))


def polled_pair(tail_ms):
    """Two plans back to back on a graph handle, a busy kernel of tail_ms queued on its stream in front of each (so each is issued while
    the stream still holds work), against the same two plans on a drained stream.  -> dict(ref=[...], got=[...]) of hex strings."""
    import torch
    pb, pl = lean_planner()
    st2 = (pb['state'] + np.float32(0.01)).astype(np.float32)
    pl.plan(pb['state'], seed=1, call=0)                             # captures the graph
    assert pl.graph_status() == 'graph'

    def enc(r):
        a, s, it = r
        return [np.asarray(a, np.float32).tobytes().hex(), np.float32(s).tobytes().hex(), int(it)]
    ref = []
    for state, call in ((pb['state'], 5), (st2, 6)):
        torch.cuda.synchronize()
        ref.append(enc(pl.plan(state, seed=9, call=call)))
    torch.cuda.synchronize()
    got = []
    for state, call in ((pb['state'], 5), (st2, 6)):                 # nothing synchronises between the two
        delay(pl.stream, tail_ms, 'plan behind pending work, call %d, against the 100-ms poll window' % call)
        got.append(enc(pl.plan(state, seed=9, call=call)))
    torch.cuda.synchronize()
    pl.close()
    return dict(ref=ref, got=got)


if __name__ == '__main__':
    import sys
    print('POLLED ' + json.dumps(polled_pair(float(sys.argv[1]))))
