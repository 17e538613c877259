"""Device replay sampling and priority updates (muzero_amd/csrc/learner_replay.hip), draw for draw: every pick of mzl_replay_sample against the
float64 reference of tests/replay_cases.py fed the same Philox uniforms, every importance weight against the reference on the device's own picks,
mzl_replay_update_priorities against a sequential loop, the error counters and the refusals.  tests/test_replay_host.py proves the reference and shows
that the data tell the plausible mistakes apart; tests/test_gpu_replay_device.py keeps the statistical view.

The kernels are called through the C ABI on plain tensors (no ring), which also lets num_added exceed the capacity.  Shapes are the smallest at which
each path can go wrong: item counts around the 1024-item scan block, a ring much larger than its content (stale priorities behind the live items), a
wrapped ring, 1026 scan blocks (the carry of the scan of the block totals), batches around the 256-thread block and past the 1024 threads of the
normalisation, a draw number with a high word, and two draws whose u * total IS a prefix sum (what tells `>` from `>=` in the searches).

Measured on an MI355X: profiles/replay_device/accuracy.json (python tests/test_gpu_replay_exact.py <out.json>)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

import replay_cases as rc

pytestmark = pytest.mark.gpu

WEIGHT_RTOL = 2.0 ** -22   # three half-ulp float32 roundings (the value, the maximum, the quotient: 1.5 * 2^-24) with a factor 2.7 for double pow's ulps
WEIGHT_ATOL = 2.0 ** -126  # nothing beyond float32 denormals
INVALID = -1               # MZL_E_INVALID


def _hl():
    from muzero_amd import hip_learner

    return hip_learner


def _dev():
    return torch.device('cuda', 0)


def _stream():
    return C.c_void_p(torch.cuda.current_stream(_dev()).cuda_stream)


def _bind(counters):
    """the process-wide counter pointer: set before EVERY call here (a DeviceSampler of another test may have left its own tensor bound)"""
    assert _hl().load_library().mzl_replay_set_error_counters(None if counters is None else counters.data_ptr()) == 0


@pytest.fixture(autouse=True)
def _unbind_after():
    yield
    torch.cuda.synchronize()
    _bind(None)


class Ring:
    """priorities, item counter and scratch of one capacity on the device; the scratch starts as NaN: whatever a draw reads, it has written"""

    def __init__(self, prio, num_added, proportional=True):
        lib = _hl().load_library()
        self.capacity = int(prio.shape[0])
        self.prio = torch.from_numpy(np.ascontiguousarray(prio, np.float32)).to(_dev())
        self.count = torch.tensor([num_added], dtype=torch.int64, device=_dev())
        self.scratch = torch.full((int(lib.mzl_replay_scratch_doubles(self.capacity)),), float('nan'), dtype=torch.float64, device=_dev()) if proportional else None

    def draw(self, alpha, beta, seed, draw, batch, counters=None, weights=True):
        """(index int64 [batch], weights float32 [batch] or None) as numpy, after one mzl_replay_sample"""
        idx = torch.full((batch,), -5, dtype=torch.int64, device=_dev())
        w = torch.full((batch,), -5.0, dtype=torch.float32, device=_dev()) if weights else None
        d = _hl().MzlReplayDraw(self.prio.data_ptr(), self.count.data_ptr(), self.capacity, float(alpha), float(beta), seed, draw, batch, idx.data_ptr(),
                                w.data_ptr() if weights else None, None if self.scratch is None else self.scratch.data_ptr())
        _bind(counters)
        _hl()._check(_hl().load_library().mzl_replay_sample(C.byref(d), _stream()))
        torch.cuda.synchronize()
        return idx.cpu().numpy(), (w.cpu().numpy() if weights else None)


def _describe(name, b, u, got, ref, cdf):
    edges = [float(cdf[k]) if 0 <= k < cdf.shape[0] else 0.0 for k in (ref - 1, ref)]
    return f'{name}: sample {b} u={u!r} device pick {got} reference pick {ref}, prefix sums around the reference pick {edges[0]!r} {edges[1]!r}'


def check_proportional(name, prio_live, kind, alpha, beta, u, got, got_w):
    """The assertions of one proportional draw; returns the figures profiles/replay_device/accuracy.json records."""
    n = prio_live.shape[0]
    pick, _, cdf, total = rc.ref_proportional(prio_live, alpha, beta, u)
    assert got.shape == pick.shape and got.min() >= 0 and got.max() < n, (name, int(got.min()), int(got.max()), n)
    equal = got == pick
    if total > 0:
        ok = rc.passes_band(got, prio_live, cdf, total, u, rc.tolerance(n, total))
    else:
        ok = got == 0  # nothing has weight: slot 0
    fig = dict(batch=int(u.shape[0]), equal_picks=int(equal.sum()), band_picks=int(ok.sum()))
    print(name, fig)
    for rule, good in (('band', ok), ('equality', equal)) if kind == 'rounded' else (('equality', equal),):
        if not good.all():
            b = int(np.flatnonzero(~good)[0])
            pytest.fail(f'{int((~good).sum())} of {u.shape[0]} picks miss the {rule} rule; ' + _describe(name, b, float(u[b]), int(got[b]), int(pick[b]), cdf))
    # importance weights: the float64 reference on the device's OWN picks
    ref_w = rc.ref_weights(rc.scaled(prio_live, alpha), total, got, beta, n)
    err = np.abs(got_w.astype(np.float64) - ref_w) / ref_w
    fig['max_weight_rel_err'] = float('%.4g' % err.max())
    fig['max_weight_rel_err_in_2^-24'] = round(float(err.max() / 2.0 ** -24), 3)
    print(name, fig)
    worst = int(np.argmax(err))
    assert (np.abs(got_w.astype(np.float64) - ref_w) <= WEIGHT_ATOL + WEIGHT_RTOL * ref_w).all(), \
        f'{name}: weight of sample {worst} (pick {int(got[worst])}) is {got_w[worst]!r}, reference {ref_w[worst]!r}: relative error {err[worst]:.3g} > 2^-22'
    assert got_w.max() == np.float32(1.0), (name, float(got_w.max()))
    return fig


def run_case(name):
    c = rc.cases()[name]
    ring = Ring(c.prio, c.num_added)
    out = {}
    for j, (draw, batch) in enumerate(c.draws):
        u = rc.uniforms(c.seed, draw, batch)
        got, got_w = ring.draw(c.alpha, c.beta, c.seed, draw, batch)
        out[f'draw_{draw}_batch_{batch}'] = check_proportional(f'{name} draw {draw} batch {batch}', c.prio[:c.n], c.kind, c.alpha, c.beta, u, got, got_w)
        assert np.array_equal(rc.reference(name, j)[1], got)  # (the shared reference of the host test: the same picks)
    return out


UNIFORM_RINGS = [(n, n, n) for n in rc.SIZES] + [(700, 1 << 16, 700), (1025, 1025, 3 * 1025 + 7), (4099, 4100, 4099)]  # (n, capacity, num_added)


@pytest.mark.parametrize('n,capacity,num_added', UNIFORM_RINGS)
def test_uniform_picks_equal_the_reference(n, capacity, num_added):
    ring = Ring(np.full(capacity, rc.STALE, np.float32), num_added, proportional=False)
    seed = 50 + n
    for k, draw in enumerate(rc.DRAWS):
        for batch in rc.BATCHES[k::3] + rc.BATCHES[(k + 1) % 3::3]:
            u = rc.uniforms(seed, draw, batch)
            ref = rc.ref_uniform(n, u)
            got, got_w = ring.draw(0.0, 0.0, seed, draw, batch)
            bad = np.flatnonzero(got != ref)
            assert bad.size == 0, f'uniform n={n} capacity={capacity} draw={draw} batch={batch}: sample {bad[0]} u={u[bad[0]]!r} device pick {got[bad[0]]} reference {ref[bad[0]]} (u*n={u[bad[0]] * n!r})'
            assert (got_w == np.float32(1.0)).all()
    got, none = ring.draw(0.0, 0.0, seed, 1, 257, weights=False)  # d_weights = NULL is accepted
    assert none is None and np.array_equal(got, rc.ref_uniform(n, rc.uniforms(seed, 1, 257)))
    # a uniform draw reads neither priorities nor scratch: NULL for both
    idx = torch.full((256,), -5, dtype=torch.int64, device=_dev())
    d = _hl().MzlReplayDraw(None, ring.count.data_ptr(), capacity, 0.0, 0.0, seed, 0, 256, idx.data_ptr(), None, None)
    _bind(None)
    assert _hl().load_library().mzl_replay_sample(C.byref(d), _stream()) == 0
    assert np.array_equal(idx.cpu().numpy(), rc.ref_uniform(n, rc.uniforms(seed, 0, 256)))


@pytest.mark.parametrize('name', rc.CASE_NAMES)
def test_proportional_picks_equal_the_reference(name):
    run_case(name)


@pytest.mark.parametrize('name,other_capacity', [('exact_n4099', 10000), ('exact_sparse', 700), ('rounded_sparse', 700), ('exact_zero_tails', 1 << 14)])
def test_same_seed_and_draw_give_the_same_bits(name, other_capacity):
    """Twice in one ring, and in a ring of another capacity holding the same live items (the ratio of the capacities is no power of two: a weight
    built on 1 / capacity would round differently in the two).  The Rounded case keeps its live items inside one scan block in both rings, so both
    add the same terms in the same order; the Exact ones are exact in any order."""
    c = rc.cases()[name]
    other = np.full(other_capacity, rc.STALE, np.float32)
    other[:c.n] = c.prio[:c.n]
    a, b = Ring(c.prio, c.num_added), Ring(other, c.n)
    for draw, batch in c.draws:
        i0, w0 = a.draw(c.alpha, c.beta, c.seed, draw, batch)
        i1, w1 = a.draw(c.alpha, c.beta, c.seed, draw, batch)
        i2, w2 = b.draw(c.alpha, c.beta, c.seed, draw, batch)
        assert i0.tobytes() == i1.tobytes() and w0.tobytes() == w1.tobytes(), (name, draw, 'two calls')
        assert i0.tobytes() == i2.tobytes(), (name, draw, 'two capacities', int((i0 != i2).sum()))
        assert w0.tobytes() == w2.tobytes(), (name, draw, 'two capacities', int((w0 != w2).sum()), 'weights differ')
        if batch > 1:
            assert not np.array_equal(i0, a.draw(c.alpha, c.beta, c.seed + 1, draw, batch)[0]) and not np.array_equal(i0, a.draw(c.alpha, c.beta, c.seed, draw + 1, batch)[0])


def _update(prio_t, index, value, owner, counters):
    _bind(counters)
    lib = _hl().load_library()
    _hl()._check(lib.mzl_replay_update_priorities(prio_t.data_ptr(), int(prio_t.shape[0]), index.data_ptr(), value.data_ptr(), int(index.shape[0]), owner.data_ptr(), _stream()))
    torch.cuda.synchronize()


def test_update_is_the_sequential_loop_and_feeds_the_next_draw():
    """4096 writes over 64 slots, each slot written from every 256-thread block, NaN / +inf / -inf / -1 (invalid: skipped and counted) and -0.0 /
    3.3e38 (valid) mixed in: the last VALID writer of a slot wins (include/mzlearner.h), a slot with none keeps its bits, so do the untouched ones.
    This test found two defects (13 of the 64 slots wrong): an invalid LAST writer owned its slot, so earlier valid writers were not applied, and
    finite values above 3.0e38 were rejected; `k_rp_owner_max` now ignores invalid values and every finite float32 >= 0 is valid."""
    uc = rc.update_case()
    want, bad = rc.ref_update(uc.prio, uc.index, uc.value)
    ring = Ring(uc.prio, uc.prio.shape[0])
    index, value = torch.from_numpy(uc.index).to(_dev()), torch.from_numpy(uc.value).to(_dev())
    owner = torch.full((ring.capacity,), 12345, dtype=torch.int32, device=_dev())  # (scratch: whatever it held)
    counters = torch.zeros(2, dtype=torch.int32, device=_dev())
    _update(ring.prio, index, value, owner, counters)
    got = ring.prio.cpu().numpy()
    diff = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert diff.size == 0, f'slots {diff.tolist()}: device {got[diff].tolist()} reference {want[diff].tolist()} before {uc.prio[diff].tolist()}'
    assert counters.tolist() == [0, bad], (counters.tolist(), bad)
    assert np.array_equal(got[uc.slots:].view(np.uint32), uc.prio[uc.slots:].view(np.uint32))
    # the next proportional draw on the updated array is the reference on the updated array
    draw, batch = uc.draw
    u = rc.uniforms(uc.seed, draw, batch)
    i, w = ring.draw(uc.alpha, uc.beta, uc.seed, draw, batch, counters=counters)
    check_proportional('after_update', want, 'rounded', uc.alpha, uc.beta, u, i, w)
    assert counters.tolist() == [0, bad]
    # without a counter array nothing is counted, and the same values are written
    again = Ring(uc.prio, uc.prio.shape[0])
    _update(again.prio, index, value, owner, None)
    assert again.prio.cpu().numpy().tobytes() == want.tobytes() and counters.tolist() == [0, bad]
    # a single write, and a batch that is no multiple of the block
    one = Ring(uc.prio, uc.prio.shape[0])
    _update(one.prio, index[:257], value[:257], owner, counters)
    want257, bad257 = rc.ref_update(uc.prio, uc.index[:257], uc.value[:257])
    assert one.prio.cpu().numpy().tobytes() == want257.tobytes() and counters.tolist() == [0, bad + bad257]


def test_draws_from_an_empty_replay_return_slot_zero_and_are_counted():
    counters = torch.zeros(2, dtype=torch.int32, device=_dev())
    ring = Ring(np.full(1500, 2.0, np.float32), 0)
    for k, (alpha, batch) in enumerate(((0.0, 257), (0.6, 257), (1.0, 1), (0.0, 4096))):
        i, w = ring.draw(alpha, 0.4, 3, k, batch, counters=counters)
        assert not i.any() and (w == np.float32(1.0)).all() and counters.tolist() == [k + 1, 0], (alpha, batch, counters.tolist())
    i, w = ring.draw(0.6, 0.4, 3, 9, 256, counters=None)  # a NULL counter pointer: nothing is counted
    assert not i.any() and counters.tolist() == [4, 0]
    ring.count.fill_(1)  # one item: not empty, slot 0 for everyone, nothing counted
    for alpha in (0.0, 0.6):
        i, w = ring.draw(alpha, 0.4, 3, 0, 255, counters=counters)
        assert not i.any() and (w == np.float32(1.0)).all() and counters.tolist() == [4, 0]


def test_device_sampler_counts_and_check_errors_raises_what_the_host_class_raises():
    from muzero_amd.replay import PrioritizedReplay

    for alpha in (0.0, 0.6):
        rp = PrioritizedReplay(300, alpha, 0.4, np.random.RandomState(0), device='cuda')
        rp.allocate(dict(state=(3,), action=(2,), pi_prob=(2, 4), value=(2,), reward=(2,)))
        prio_t, count_t = rp.attach_device_writer()
        s = rp.device_sampler(seed=4)
        s.check_errors()  # nothing yet
        for _ in range(3):
            idx, w, _ = s.sample(64)
            assert not idx.cpu().numpy().any() and (w is None) == (alpha == 0)
        assert s._errors.tolist() == [3, 0]
        with pytest.raises(RuntimeError, match='empty replay'):
            s.check_errors()
        assert s._errors.tolist() == [0, 0]
        s.check_errors()  # cleared
        prio = np.linspace(1.0, 2.0, 200).astype(np.float32)
        prio_t[:200] = torch.from_numpy(prio).to(prio_t.device)
        count_t.fill_(200)
        idx, w, _ = s.sample(257)  # draw number 3 of this sampler
        u = rc.uniforms(4, 3, 257)
        if alpha == 0:
            assert np.array_equal(idx.cpu().numpy(), rc.ref_uniform(200, u))
        else:
            check_proportional('device_sampler', prio, 'rounded', alpha, 0.4, u, idx.cpu().numpy(), w.cpu().numpy())
        s.check_errors()
        index = torch.tensor([5, 6, 5, 7, 6], dtype=torch.int64, device=prio_t.device)
        value = torch.tensor([9.0, float('nan'), 8.0, float('inf'), 3.0], dtype=torch.float32, device=prio_t.device)
        s.update_priorities(index, value)
        p = prio_t.cpu().numpy()
        assert p[5] == 8.0 and p[6] == 3.0 and p[7] == prio[7] and s._errors.tolist() == [0, 2]
        with pytest.raises(ValueError, match='Priorities must be finite and positive'):
            s.check_errors()
        s.check_errors()
        # both kinds at once: the invalid priority is reported first, and both are cleared
        count_t.fill_(0)
        s.sample(64)
        s.update_priorities(index[:2], value[:2])
        with pytest.raises(ValueError):
            s.check_errors()
        assert s._errors.tolist() == [0, 0]


def test_refusals_name_the_argument_and_launch_nothing():
    hl, lib = _hl(), _hl().load_library()
    counters = torch.zeros(2, dtype=torch.int32, device=_dev())
    ring = Ring(np.full(64, 1.0, np.float32), 0)  # (empty: a launch would bump counter [0])
    idx = torch.full((64,), -5, dtype=torch.int64, device=_dev())
    w = torch.full((64,), -5.0, dtype=torch.float32, device=_dev())
    _bind(counters)

    def draw(**kw):
        a = dict(d_priority=ring.prio.data_ptr(), d_num_added=ring.count.data_ptr(), capacity=64, priority_exponent=0.6, importance_sampling_exponent=0.4, seed=1, draw=0,
                 batch=64, d_index=idx.data_ptr(), d_weights=w.data_ptr(), d_scratch=ring.scratch.data_ptr())
        a.update(kw)
        return hl.MzlReplayDraw(*[a[f] for f, _ in hl.MzlReplayDraw._fields_])

    bad_args, needs = 'mzl_replay_sample: bad arguments', 'mzl_replay_sample: proportional draws need d_priority, d_weights and d_scratch'
    for kw, msg in ((dict(capacity=0), bad_args), (dict(capacity=-3), bad_args), (dict(batch=0), bad_args), (dict(batch=-1), bad_args), (dict(d_num_added=None), bad_args),
                    (dict(d_index=None), bad_args), (dict(capacity=0, priority_exponent=0.0), bad_args), (dict(batch=0, priority_exponent=0.0), bad_args),
                    (dict(d_priority=None), needs), (dict(d_weights=None), needs), (dict(d_scratch=None), needs)):
        assert lib.mzl_replay_sample(C.byref(draw(**kw)), _stream()) == INVALID, kw
        assert lib.mzl_last_error().decode() == msg, (kw, lib.mzl_last_error())
    assert lib.mzl_replay_sample(None, _stream()) == INVALID and lib.mzl_last_error().decode() == bad_args
    owner = torch.zeros(64, dtype=torch.int32, device=_dev())
    index = torch.zeros(64, dtype=torch.int64, device=_dev())
    value = torch.full((64,), float('nan'), dtype=torch.float32, device=_dev())  # (a launch would bump counter [1])
    ok = [ring.prio.data_ptr(), 64, index.data_ptr(), value.data_ptr(), 64, owner.data_ptr()]
    for pos, arg in ((5, None), (0, None), (2, None), (3, None), (1, 0), (4, 0)):  # a NULL d_owner first
        a = list(ok)
        a[pos] = arg
        assert lib.mzl_replay_update_priorities(*a, _stream()) == INVALID, (pos, arg)
        assert lib.mzl_last_error().decode() == 'mzl_replay_update_priorities: bad arguments'
    torch.cuda.synchronize()
    assert counters.tolist() == [0, 0] and (idx == -5).all() and (w == -5.0).all() and (ring.prio == 1.0).all() and not owner.any()
    # the same arguments unbroken are accepted, and now the counters move
    assert lib.mzl_replay_sample(C.byref(draw()), _stream()) == 0 and lib.mzl_replay_update_priorities(*ok, _stream()) == 0
    torch.cuda.synchronize()
    assert counters.tolist() == [1, 64] and not idx.cpu().numpy().any()


if __name__ == '__main__':  # python tests/test_gpu_replay_exact.py <out.json>: what every proportional case measures
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    result = {'statistic': 'per draw: picks equal to the float64 reference, picks inside the reference item widened by n * 2^-50 * total, and the largest relative error of '
                           'the float32 importance weights against the float64 reference on the device\'s own picks',
              'weight_bar': '2^-22 = %.4g (4 in units of 2^-24)' % WEIGHT_RTOL, 'cases': {name: run_case(name) for name in rc.CASE_NAMES}}
    _bind(None)
    with open(sys.argv[1], 'w') as f_:
        json.dump(result, f_, indent=1)
        f_.write('\n')
    print(json.dumps(result, indent=1))
