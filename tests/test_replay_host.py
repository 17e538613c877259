"""The reference of tests/replay_cases.py and its data, proved on the host (no GPU): the reference IS np.random.choice's inverse-CDF method and
`PrioritizedReplay._draw`'s weight formula, the Exact data are exact, no pick of the Rounded data lies where rounding could excuse a wrong pick, and
every mistake a kernel of learner_replay.hip could plausibly make changes the reference's output on the committed data -- so
tests/test_gpu_replay_exact.py, which holds the kernels to this reference on this data, can tell them apart."""
import numpy as np
import pytest

import replay_cases as rc
from helpers import philox_uniforms
from muzero_amd.replay import PrioritizedReplay


def _draws():
    return [(name, j) for name in rc.CASE_NAMES for j in range(len(rc.cases()[name].draws))]


def test_the_case_list_is_the_committed_one_and_covers_the_listed_shapes():
    cs = rc.cases()
    assert tuple(cs) == rc.CASE_NAMES
    for kind in ('exact', 'rounded'):
        mine = [c for c in cs.values() if c.kind == kind]
        assert {c.n for c in mine} >= set(rc.SIZES)
        assert {b for c in mine for _, b in c.draws} == set(rc.BATCHES)
        assert {d for c in mine for d, _ in c.draws} == set(rc.DRAWS)
        assert any(c.capacity > 50 * c.n for c in mine) and any(c.num_added == 3 * c.capacity + 7 for c in mine)
        assert any((c.capacity + rc.RB - 1) // rc.RB == 1026 for c in mine)
    assert {c.alpha for c in cs.values() if c.kind == 'rounded'} == {0.5, 0.6}
    for c in cs.values():
        assert c.n == min(c.num_added, c.capacity) and (c.prio[c.n:] == rc.STALE).all() and c.prio.dtype == np.float32


def test_uniforms_are_the_helper_stream_sample_by_sample():
    for seed, draw in ((5, 0), (2 ** 63 + 12345, 1), (39, 2 ** 32 + 3), (7, 2 ** 64 - 1)):
        u = rc.uniforms(seed, draw, 300)
        for b in (0, 1, 2, 63, 64, 255, 256, 299):
            assert u[b] == philox_uniforms(seed, draw & 0xFFFFFFFF, draw >> 32, b, 1)[0]
    assert not np.array_equal(rc.uniforms(5, 0, 64), rc.uniforms(5, 2 ** 32, 64))  # the high word of the draw number is part of the key


@pytest.mark.parametrize('n', [1, 2, 3, 255, 1024, 1025, 4099])
@pytest.mark.parametrize('s', [0, 1, 2])
def test_reference_is_numpy_choice_on_the_same_uniforms(n, s):
    """np.random.choice(p=...) draws random_sample(size) and searches its own cumsum of p (normalised, last entry forced to 1) from the right; the
    reference searches the unnormalised sums for u * total.  The two can differ only where u sits on an item's edge to rounding: inside the band.  For
    the seeds committed here they do not differ at all."""
    size, alpha, beta = 4096, 0.6, 0.4
    prio = rc._floats(np.random.RandomState(100 + n), n)
    scaled = prio.astype(np.float64) ** alpha
    probs = scaled / scaled.sum()
    choice = np.random.RandomState(s).choice(n, size, p=probs)
    u = np.random.RandomState(s).random_sample(size)
    pick, wts, cdf, total = rc.ref_proportional(prio, alpha, beta, u)
    differ = pick != choice
    _, inside = rc.band(cdf, total, u, rc.tolerance(n, total))
    assert not (differ & ~inside).any()
    assert differ.sum() == 0, (n, s, int(differ.sum()))
    # the weights: PrioritizedReplay._draw's formula on the same picks
    host = ((1.0 / n) / probs[pick]) ** beta
    host /= host.max()
    np.testing.assert_allclose(wts, host, rtol=1e-13, atol=0)
    assert wts.max() == 1.0


def test_reference_weights_are_the_host_replay_class_itself():
    """`PrioritizedReplay._draw` run for real (it draws from the process-global numpy RNG): the same picks and weights from the reference fed the
    uniforms of a twin generator."""
    n, alpha, beta, size = 777, 0.5, 0.7, 512
    prio = rc._floats(np.random.RandomState(5), n)
    rp = PrioritizedReplay(n, alpha, beta, np.random.RandomState(0))
    rp._prio[:], rp._count = prio, n
    state = np.random.get_state()
    try:
        np.random.seed(99)
        picks, is_w = rp._draw(size)
    finally:
        np.random.set_state(state)
    pick, wts, _, _ = rc.ref_proportional(prio, alpha, beta, np.random.RandomState(99).random_sample(size))
    assert np.array_equal(pick, picks)
    np.testing.assert_allclose(wts, is_w, rtol=2e-6, atol=0)  # (_draw works on the float32 priorities: float32 pow)


def test_exact_data_meet_the_bounds_of_the_exact_claim():
    for c in rc.cases().values():
        if c.kind != 'exact':
            continue
        live = c.prio[:c.n]
        assert c.alpha == 1.0 and (live == np.floor(live)).all() and live.min() >= 0 and live.max() <= 255
        assert float(live.astype(np.float64).sum()) <= 255.0 * c.n < 2.0 ** 53
        w = rc.scaled(live, c.alpha)
        assert np.array_equal(np.cumsum(w), rc.scan3(w))  # any summation order: here the kernels' three-level one
        if c.n >= 255 and 'all_zero' not in c.name and 'single' not in c.name:
            assert (live == 0).mean() > (0.15 if c.name in rc.EDGES else 0.25)  # many zeros (the edge cases need a mean of 128 to reach 2^27)
    z = rc.cases()['exact_zero_tails'].prio
    assert not z[1000:2048].any() and not z[3000:3080].any() and not z[4096:4099].any() and z[:1000].any() and z[2048:3000].any() and z[3080:4096].any()
    live = rc.cases()['exact_carry'].prio
    blocks = np.flatnonzero(np.add.reduceat(live, np.arange(0, live.shape[0], rc.RB)))
    assert tuple(blocks) == rc.CARRY_BLOCKS and tuple(np.flatnonzero(np.add.reduceat(rc.cases()['rounded_carry'].prio, np.arange(0, live.shape[0], rc.RB)))) == rc.CARRY_BLOCKS


@pytest.mark.parametrize('name,j', _draws())
def test_no_reference_pick_lies_inside_the_band(name, j):
    """What keeps the GPU test from excusing a wrong pick as rounding: for the committed seeds no u * total lies within tol of an edge of its item
    (expected count ~ batch * n * 2 * tol / total ~ 1e-4).  Asserted from the reference alone."""
    c = rc.cases()[name]
    u, pick, wts, cdf, total = rc.reference(name, j)
    assert ((pick >= 0) & (pick < c.n)).all() and pick.shape[0] == c.draws[j][1]
    if total > 0:
        assert (c.prio[pick] > 0).all()
        if c.kind == 'rounded':  # (the Exact class needs no band: its rule is equality, and its sums are exact)
            dist, inside = rc.band(cdf, total, u, rc.tolerance(c.n, total))
            assert inside.sum() == 0, (name, j, float(dist.min()))
            assert rc.passes_band(pick, c.prio[:c.n], cdf, total, u, rc.tolerance(c.n, total)).all()
            # the tolerance is a tiny share of the narrowest item (1e-8 at n = 4099, 3e-5 at the 10^6 items of the 1026-block case): the band
            # cannot swallow an item, so a pick that passes the rule is the reference's pick or its direct neighbour at an edge
            assert rc.tolerance(c.n, total) < 1e-4 * rc.scaled(c.prio[:c.n][c.prio[:c.n] > 0], c.alpha).min()
        # and the kernels' summation order, modelled, picks the same slots
        assert np.array_equal(np.minimum(np.searchsorted(rc.scan3(rc.scaled(c.prio[:c.n], c.alpha)), u * total, side='right'), c.n - 1), pick)
    else:
        assert not pick.any() and (wts == 1.0).all()
    assert wts.max() == 1.0 and wts.min() > 0


@pytest.mark.parametrize('name', list(rc.EDGES))
def test_edge_cases_put_a_draw_exactly_on_a_prefix_sum(name):
    seed, b, x, k = rc.EDGES[name]
    c = rc.cases()[name]
    u, pick, _, cdf, total = rc.reference(name, 0)
    assert c.seed == seed and total == rc.EDGE_TOTAL and u[b] * total == x == cdf[k - 1] and c.prio[k - 1] > 0 and c.prio[k] > 0
    assert pick[b] == k  # side='right': the item that BEGINS at the prefix sum
    assert rc.ref_proportional(c.prio[:c.n], c.alpha, c.beta, u, side='left')[0][b] == k - 1
    assert (k % rc.RB == 0) == (name == 'exact_edge_block')


def _changed(mistake, names=rc.CASE_NAMES):
    """the (case, draw) pairs on which `mistake(case, u, reference picks, reference weights)` -> (picks, weights) differs from the reference"""
    out = []
    for name in names:
        c = rc.cases()[name]
        for j in range(len(c.draws)):
            u, pick, wts, _, _ = rc.reference(name, j)
            p2, w2 = mistake(c, u)
            if not np.array_equal(p2, pick) or not np.allclose(w2, wts, rtol=2.0 ** -22, atol=0):
                out.append((name, j))
    return out


def _prop(**kw):
    return lambda c, u: rc.ref_proportional(c.prio[:c.n], c.alpha, c.beta, u, **kw)[:2]


def test_each_deliberate_mistake_changes_the_reference():
    live = lambda c: c.prio[:c.n]
    exclusive = lambda c: np.concatenate([[0.0], np.cumsum(rc.scaled(live(c), c.alpha))[:-1]])
    mistakes = {
        "side='left'": _prop(side='left'),
        'exclusive prefix sums': lambda c, u: rc.ref_proportional(live(c), c.alpha, c.beta, u, cdf=exclusive(c))[:2],
        'no division by the maximum': _prop(normalize=False),
        'the carry between chunks dropped': lambda c, u: rc.ref_proportional(live(c), c.alpha, c.beta, u, cdf=rc.scan3(rc.scaled(live(c), c.alpha), carry=False))[:2],
        'the walk-back removed': _prop(walk=False),
        'stale slots read (capacity for n)': lambda c, u: rc.ref_proportional(c.prio, c.alpha, c.beta, u)[:2],
    }
    hits = {k: _changed(m) for k, m in mistakes.items()}
    for k, h in hits.items():
        assert h, f'no committed case tells "{k}" from the reference'
    # where each one shows: side='left' only where u * total can EQUAL a prefix sum (integers: the Exact class), the carry only past block 1023, the
    # walk-back only where nothing has weight, the item count only where the ring is not full
    assert {n for n, _ in hits["side='left'"]} == set(rc.EDGES)
    assert {n for n, _ in hits['the carry between chunks dropped']} == {'exact_carry', 'rounded_carry'} | set(rc.EDGES)  # the 1026-block cases
    assert {n for n, _ in hits['the walk-back removed']} == {'exact_all_zero', 'exact_all_zero_sparse'}
    assert {n for n, _ in hits['stale slots read (capacity for n)']} == {'exact_sparse', 'rounded_sparse', 'exact_all_zero_sparse'}
    # 1 / capacity for 1 / n scales every weight of a batch by one factor, and the division by the maximum takes it out again: in exact arithmetic
    # the normalised weights are blind to it.  It shows before the division (compared here), and in the BITS after it: the kernel rounds the
    # undivided weight to float32, so the same live items in rings of two capacities (ratio not a power of two) give different float32 weights --
    # which is what the GPU test's same-draw-in-two-capacities check sees.
    for name in ('exact_sparse', 'rounded_sparse'):
        c = rc.cases()[name]
        u, pick, _, _, total = rc.reference(name, 0)
        w = rc.scaled(live(c), c.alpha)
        assert not np.allclose(rc.ref_weights(w, total, pick, c.beta, c.capacity, normalize=False), rc.ref_weights(w, total, pick, c.beta, c.n, normalize=False), rtol=0.5)

        def as_kernel(size):
            raw = rc.ref_weights(w, total, pick, c.beta, size, normalize=False).astype(np.float32)
            return raw / raw.max()
        assert np.array_equal(as_kernel(c.n), as_kernel(c.n)) and (as_kernel(c.n) != as_kernel(c.capacity)).sum() > 100
    # the uniform pick
    for n in rc.SIZES:
        u = rc.uniforms(3, 0, 257)
        assert not np.array_equal(rc.ref_uniform(n, u, rounding=np.ceil), rc.ref_uniform(n, u)) or n == 1
        assert rc.ref_uniform(n, u).max() <= n - 1 and (rc.ref_uniform(0, u) == 0).all()
    # the update
    uc = rc.update_case()
    new, bad = rc.ref_update(uc.prio, uc.index, uc.value)
    first, _ = rc.ref_update(uc.prio, uc.index, uc.value, first_wins=True)
    assert (new[:uc.slots] != first[:uc.slots]).sum() > uc.slots // 2


def test_update_data_hold_every_corner_the_docstring_names():
    uc = rc.update_case()
    new, bad = rc.ref_update(uc.prio, uc.index, uc.value)
    valid = np.isfinite(uc.value) & (uc.value >= 0)
    assert bad == int((~valid).sum()) and bad > 400
    assert uc.index.min() == 0 and uc.index.max() == uc.slots - 1 and uc.index.shape == (4096,)
    counts = np.bincount(uc.index, minlength=uc.slots)
    assert counts.min() >= 32
    for slot in range(uc.slots):  # every slot is written from many of the sixteen 256-thread blocks
        assert np.unique(np.flatnonzero(uc.index == slot) // 256).shape[0] >= 12
    for v in rc.SPECIALS:  # every special value occurs, -0.0 with its sign
        v32 = np.float32(v)
        assert (uc.value.view(np.uint32) == v32.view(np.uint32)).sum() > 20 or np.isnan(v32) and np.isnan(uc.value).sum() > 20
    last = {s: uc.value[np.flatnonzero(uc.index == s)[-1]] for s in range(56, 64)}
    assert np.isnan(last[56]) and last[57] == np.inf and last[58] == -1.0 and last[59] == -np.inf and np.isnan(last[63])
    assert last[60] == np.float32(3.3e38) and np.isfinite(last[60]) and last[61] == 0 and np.signbit(last[61])
    # the last VALID writer wins where the last writer is invalid; a slot with no valid writer keeps its bits
    for s in (56, 57, 58, 59):
        w = np.flatnonzero((uc.index == s) & valid)
        assert new[s] == uc.value[w[-1]] and new[s] != uc.prio[s] and w[-1] < np.flatnonzero(uc.index == s)[-1]
    assert new[60] == np.float32(3.3e38) and new[61].view(np.uint32) == 0x80000000 and new[63] == 2.25
    assert not valid[uc.index == 62].any() and new[62].view(np.uint32) == uc.prio[62].view(np.uint32)
    assert np.array_equal(new[uc.slots:].view(np.uint32), uc.prio[uc.slots:].view(np.uint32))
    # the draw that follows the update: no pick inside the band, more than the two huge slots drawn
    u = rc.uniforms(uc.seed, *uc.draw)
    pick, wts, cdf, total = rc.ref_proportional(new, uc.alpha, uc.beta, u)
    assert rc.band(cdf, total, u, rc.tolerance(new.shape[0], total))[1].sum() == 0 and np.unique(pick).shape[0] > 40
