"""The draw-for-draw reference of device replay sampling (muzero_amd/csrc/learner_replay.hip; include/mzlearner.h, mzl_replay_sample /
mzl_replay_update_priorities) in numpy float64, and the data the tests run it on.  No GPU, no torch: tests/test_replay_host.py proves the
reference and the data here, tests/test_gpu_replay_exact.py holds the kernels to them.

The device's uniforms are Philox4x32-10 keyed by (seed; draw low word, draw high word, sample), the first double of the stream
(tests/helpers.py::philox_uniforms), so a draw can be checked pick for pick, not only as a distribution.

Two classes of data:
  Exact    alpha = 1, integer priorities 0 ... 255 with many zeros: every prefix sum is an integer far below 2^53, exact in float64 in ANY summation
           order -- the device's three-level scan and numpy's sequential cumsum hold the same numbers, u * total rounds once on both sides, and
           every pick must be equal.
  Rounded  alpha in {0.5, 0.6}, random float32 priorities: the prefix sums differ by summation order and by the ulps of pow.  A pick passes when
           u * total lies inside its item widened by tol = n * 2^-50 * total on each side (`band`); the seeds here are chosen so that NO pick of the
           reference lies that close to an edge (asserted from the reference alone in tests/test_replay_host.py), which makes the rule equality.
"""
import functools
from typing import NamedTuple, Tuple

import numpy as np

RB = 1024  # elements per scan block of the kernels
M32 = 0xFFFFFFFF
BATCHES = (1, 255, 256, 257, 1025, 4096)
DRAWS = (0, 1, 2 ** 32 + 3)  # (the last one reaches the high counter word)
SIZES = (1, 2, 255, 1023, 1024, 1025, 4099)
STALE = 7.0  # what the slots past the live items hold: a draw must never see it


@functools.lru_cache(maxsize=None)
def uniforms(seed: int, draw: int, batch: int) -> np.ndarray:
    """u[b] = philox_uniforms(seed, draw & 0xffffffff, draw >> 32, b, 1)[0], all b at once (uint64 lanes; the host test compares it with
    tests/helpers.py::philox_uniforms element for element)."""
    c = [np.zeros(batch, np.uint64), np.full(batch, draw & M32, np.uint64), np.full(batch, (draw >> 32) & M32, np.uint64), np.arange(batch, dtype=np.uint64)]
    k0, k1, m, s32 = seed & M32, (seed >> 32) & M32, np.uint64(M32), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    u = ((c[0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (c[1] >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0
    u.setflags(write=False)
    return u


def ref_uniform(n: int, u: np.ndarray, rounding=np.floor) -> np.ndarray:
    """min(floor(u * n), n - 1); slot 0 of an empty replay."""
    if n < 1:
        return np.zeros(u.shape[0], np.int64)
    return np.minimum(rounding(u * float(n)).astype(np.int64), n - 1)


def scaled(prio: np.ndarray, alpha: float) -> np.ndarray:
    return prio.astype(np.float64) ** alpha


def walk_back(pick: np.ndarray, w: np.ndarray) -> np.ndarray:
    """The nearest slot at or below each pick that has weight (slot 0 when there is none)."""
    last = np.where(w > 0, np.arange(w.shape[0]), 0)
    return np.maximum.accumulate(last)[pick]


def ref_proportional(prio: np.ndarray, alpha: float, beta: float, u: np.ndarray, *, side='right', cdf=None, size=None, normalize=True, walk=True):
    """(picks int64, importance weights float64, cdf, total) of `prio` = the live items.  The keyword arguments exist for the deliberate mistakes
    of tests/test_replay_host.py: another `side`, other prefix sums, another item count in 1 / n, no division by the maximum, no walk-back."""
    n = prio.shape[0]
    if n < 1:
        return np.zeros(u.shape[0], np.int64), np.ones(u.shape[0]), np.zeros(0), 0.0
    w = scaled(prio, alpha)
    cdf = np.cumsum(w) if cdf is None else cdf
    total = float(cdf[-1])
    pick = np.minimum(np.searchsorted(cdf, u * total, side=side), n - 1).astype(np.int64)
    if walk:
        pick = walk_back(pick, w)
    return pick, ref_weights(w, total, pick, beta, n if size is None else size, normalize), cdf, total


def ref_weights(w: np.ndarray, total: float, pick: np.ndarray, beta: float, size: int, normalize=True) -> np.ndarray:
    """((1 / n) / (w[pick] / total)) ^ beta, divided by the maximum; ones where nothing has weight."""
    with np.errstate(divide='ignore', invalid='ignore'):
        p = w[pick] / total
        raw = np.where(p > 0, ((1.0 / size) / p) ** beta, 0.0)
    if not raw.max() > 0:
        return np.ones(pick.shape[0])
    return raw / raw.max() if normalize else raw


def band(cdf: np.ndarray, total: float, u: np.ndarray, tol: float) -> Tuple[np.ndarray, np.ndarray]:
    """For each sample: the distance of u * total from the nearest edge of its item, in units of tol, and whether it is below 1 (inside the band
    in which another summation order may pick a neighbour)."""
    x = u * total
    a = np.minimum(np.searchsorted(cdf, x, side='right'), cdf.shape[0] - 1)
    lower = np.where(a > 0, cdf[np.maximum(a - 1, 0)], 0.0)
    dist = np.minimum(x - lower, cdf[a] - x) / tol
    return dist, dist < 1.0


def tolerance(n: int, total: float) -> float:
    """n * 2^-50 * total: each prefix is a sum of at most n non-negative float64 terms in some order ((n - 1) * 2^-53 of the total), each term a pow
    good to a few ulp, u * total one more rounding; the factor 8 over n * 2^-53 covers them with room to spare."""
    return n * 2.0 ** -50 * total


def passes_band(pick: np.ndarray, prio: np.ndarray, cdf: np.ndarray, total: float, u: np.ndarray, tol: float) -> np.ndarray:
    """The Rounded rule: prio[a] > 0 and cdf[a - 1] - tol <= u * total < cdf[a] + tol."""
    x = u * total
    lower = np.where(pick > 0, cdf[np.maximum(pick - 1, 0)], 0.0)
    return (prio[pick] > 0) & (lower - tol <= x) & (x < cdf[pick] + tol)


def ref_update(prio: np.ndarray, index: np.ndarray, value: np.ndarray, first_wins=False) -> Tuple[np.ndarray, int]:
    """priority[index[b]] = value[b] in a sequential loop: the last b of a repeated index wins.  A non-finite or negative value is skipped and
    counted (include/mzlearner.h: "the value is skipped") -- so the last VALID writer of a slot wins.  Returns (new priorities, count)."""
    out, bad, seen = prio.copy(), 0, set()
    for i, v in zip(index.tolist(), value):
        if not np.isfinite(v) or v < 0:
            bad += 1
            continue
        if first_wins and i in seen:
            continue
        seen.add(i)
        out[i] = v
    return out, bad


def scan3(w: np.ndarray, carry=True) -> np.ndarray:
    """The kernels' three-level scan as a model: inclusive sums inside blocks of 1024, the block totals scanned in chunks of 1024 blocks with a
    running carry, the global prefix = offset of the block + local prefix.  `carry=False` is the mistake of dropping the carry."""
    n = w.shape[0]
    nb = (n + RB - 1) // RB
    padded = np.zeros(nb * RB)
    padded[:n] = w
    local = np.cumsum(padded.reshape(nb, RB), axis=1)
    block_sum = local[:, -1]
    block_off = np.zeros(nb + 1)
    run = 0.0
    for c0 in range(0, nb, RB):
        inc = np.cumsum(block_sum[c0:c0 + RB])
        block_off[c0 + 1:c0 + 1 + inc.shape[0]] = (run if carry else 0.0) + inc
        run += inc[-1]
    return (block_off[:-1, None] + local).reshape(-1)[:n]


class Case(NamedTuple):
    name: str
    kind: str           # 'exact' | 'rounded'
    prio: np.ndarray    # float32 [capacity]: the live items first, STALE behind them
    n: int              # live items = min(num_added, capacity)
    capacity: int
    num_added: int
    alpha: float
    beta: float
    seed: int           # the Philox seed of the draws
    draws: tuple        # ((draw number, batch), ...)


def _ints(rs, n, zero_share=0.5):
    p = rs.randint(1, 256, n).astype(np.float32)
    p[rs.random_sample(n) < zero_share] = 0.0
    if not p.any():
        p[rs.randint(0, n)] = 3.0
    return p


def _floats(rs, n):
    p = rs.uniform(0.01, 2.0, n).astype(np.float32)
    p[rs.random_sample(n) < 0.1] = 0.0
    if not p.any():
        p[rs.randint(0, n)] = 0.5
    return p


def _case(name, kind, live, capacity, alpha, beta, seed, draws, num_added=None):
    prio = np.full(capacity, STALE, np.float32)
    prio[:live.shape[0]] = live
    prio.setflags(write=False)
    return Case(name, kind, prio, live.shape[0], capacity, live.shape[0] if num_added is None else num_added, alpha, beta, seed, tuple(draws))


def _plan(k):
    """three (draw, batch) pairs; over the size sweep every batch and every draw number meets every other"""
    return tuple((DRAWS[j], BATCHES[(2 * k + j) % len(BATCHES)]) for j in range(3))


CARRY_CAPACITY = RB * RB + 1500  # 1026 blocks: the second chunk of k_rp_scan_totals holds blocks 1024 and 1025
CARRY_BLOCKS = (0, 1023, 1024, 1025)


def _carry_live(rs, gen):
    live = np.zeros(CARRY_CAPACITY, np.float32)
    for b in CARRY_BLOCKS:
        lo, hi = b * RB, min((b + 1) * RB, CARRY_CAPACITY)
        live[lo:hi] = gen(rs, hi - lo)
    return live


EDGE_TOTAL = 2 ** 27
# (seed, sample, u * 2^27) found by searching seeds for a uniform whose low 26 bits are zero: with total = 2^27, u * total is an INTEGER, and the
# data put a prefix sum exactly there.  Only such a draw tells `>` from `>=` in the searches (side='right' from side='left').
EDGES = {'exact_edge_block': (100968, 3920, 28022542, 214 * RB),       # the prefix sum of a block's end: the search over the block totals
         'exact_edge_item': (126732, 2347, 17862308, 136 * RB + 485)}  # the prefix sum of an item inside a block: the search inside the block


def _edge_live(name):
    """integers 0 ... 255 over all 1026 blocks with sum(live[:k]) == the edge's integer and sum(live) == 2^27, slots k - 1 and k nonzero"""
    _, _, x, k = EDGES[name]
    rs = np.random.RandomState(k)
    live = rs.randint(96, 256, CARRY_CAPACITY).astype(np.int64)
    live[rs.random_sample(CARRY_CAPACITY) < 0.2] = 0
    live[k - 1:k + 1] = 7
    for part, target in ((live[:k], x), (live[k:], EDGE_TOTAL - x)):
        while part.sum() != target:
            excess = int(part.sum() - target)
            ok = rs.permutation(np.flatnonzero(part >= 2 if excess > 0 else (part > 0) & (part < 255)))[:abs(excess)]
            part[ok] -= np.sign(excess)
    return live.astype(np.float32)


# The Philox seed of each Rounded case is committed here; tests/test_replay_host.py asserts that none of its reference picks lies inside the band.
@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for k, n in enumerate(SIZES):
        rs = np.random.RandomState(1000 + n)
        out.append(_case(f'exact_n{n}', 'exact', _ints(rs, n), n, 1.0, 0.4 + 0.1 * (k % 3), 11 + k, _plan(k)))
        alpha = (0.5, 0.6)[k % 2]
        out.append(_case(f'rounded_n{n}', 'rounded', _floats(rs, n), n, alpha, 0.4 + 0.2 * (k % 3), 21 + k, _plan(k + 1)))
    rs = np.random.RandomState(7)
    out.append(_case('exact_sparse', 'exact', _ints(rs, 700), 1 << 16, 1.0, 1.0, 31, ((0, 4096), (1, 257))))
    out.append(_case('rounded_sparse', 'rounded', _floats(rs, 700), 1 << 16, 0.6, 0.4, 32, ((0, 4096), (2 ** 32 + 3, 255))))
    out.append(_case('exact_wrapped', 'exact', _ints(rs, 1025), 1025, 1.0, 0.5, 33, ((1, 1025), (2 ** 32 + 3, 4096)), num_added=3 * 1025 + 7))
    out.append(_case('rounded_wrapped', 'rounded', _floats(rs, 2500), 2500, 0.5, 1.0, 34, ((0, 4096), (1, 256)), num_added=3 * 2500 + 7))
    # zero-priority slots in the middle, at a block's tail, as whole blocks
    tails = _ints(rs, 4099, 0.3)
    tails[1000:1024] = 0.0  # the tail of block 0
    tails[1024:2048] = 0.0  # block 1
    tails[3000:3072] = 0.0  # the tail of block 2
    tails[3072:3080] = 0.0  # the head of block 3
    tails[4096:] = 0.0      # all of the last, short block
    out.append(_case('exact_zero_tails', 'exact', tails, 4099, 1.0, 0.6, 35, ((0, 4096), (1, 1025))))
    for slot in (0, 2047, 2048, 4098):  # a single nonzero slot: first, last of a block, first of a block, last of all
        one = np.zeros(4099, np.float32)
        one[slot] = 5.0
        out.append(_case(f'exact_single_{slot}', 'exact', one, 4099, 1.0, 0.5, 36, ((0, 257),)))
    out.append(_case('exact_all_zero', 'exact', np.zeros(1025, np.float32), 1025, 1.0, 0.5, 37, ((0, 257), (1, 1))))
    out.append(_case('exact_all_zero_sparse', 'exact', np.zeros(3, np.float32), 4099, 1.0, 0.5, 37, ((0, 256),)))
    out.append(_case('exact_carry', 'exact', _carry_live(np.random.RandomState(8), _ints), CARRY_CAPACITY, 1.0, 0.5, 38, ((0, 4096), (2 ** 32 + 3, 1025))))
    out.append(_case('rounded_carry', 'rounded', _carry_live(np.random.RandomState(9), _floats), CARRY_CAPACITY, 0.5, 0.4, 39, ((0, 4096), (1, 257))))
    for name, (seed, _, _, _) in EDGES.items():
        out.append(_case(name, 'exact', _edge_live(name), CARRY_CAPACITY, 1.0, 0.5, seed, ((0, 4096),)))
    return {c.name: c for c in out}


CASE_NAMES = tuple(f'{k}_n{n}' for n in SIZES for k in ('exact', 'rounded')) + (
    'exact_sparse', 'rounded_sparse', 'exact_wrapped', 'rounded_wrapped', 'exact_zero_tails', 'exact_single_0', 'exact_single_2047', 'exact_single_2048',
    'exact_single_4098', 'exact_all_zero', 'exact_all_zero_sparse', 'exact_carry', 'rounded_carry', 'exact_edge_block', 'exact_edge_item')


@functools.lru_cache(maxsize=None)
def reference(name: str, j: int):
    """(u, picks, weights float64, cdf, total) of draw j of a case: computed once, shared, read-only."""
    c = cases()[name]
    draw, batch = c.draws[j]
    u = uniforms(c.seed, draw, batch)
    pick, wts, cdf, total = ref_proportional(c.prio[:c.n], c.alpha, c.beta, u)
    for a in (pick, wts, cdf):
        a.setflags(write=False)
    return u, pick, wts, cdf, total


class UpdateCase(NamedTuple):
    prio: np.ndarray    # float32 [capacity] before the update
    index: np.ndarray   # int64 [batch], all inside [0, slots)
    value: np.ndarray   # float32 [batch]
    slots: int          # the update touches [0, slots); [slots, capacity) keeps its bits
    alpha: float
    beta: float
    seed: int
    draw: Tuple[int, int]


SPECIALS = (np.nan, np.inf, -1.0, -0.0, 3.3e38)  # invalid, invalid, invalid, valid (a zero), valid (finite: float32 reaches 3.4e38)


@functools.lru_cache(maxsize=None)
def update_case():
    """4096 writes over 64 slots of an 80-slot array, every slot repeated ~64 times across the sixteen 256-thread blocks, a fifth of the values
    special.  Slots 56 ... 59 END on an invalid value after valid ones, slot 60 ends on 3.3e38, slot 61 on -0.0, slot 62 gets only invalid values,
    slot 63 a valid value followed by several invalid ones in later blocks."""
    rs = np.random.RandomState(12)
    slots, capacity, batch = 64, 80, 4096
    prio = rs.uniform(0.5, 1.5, capacity).astype(np.float32)
    prio[64:] = np.array([0.0, -0.0, 1e-42, 3.0e38] * 4, np.float32)  # bits a rewrite through arithmetic would not keep
    index = rs.randint(0, 56, batch).astype(np.int64)
    value = rs.uniform(0.0, 4.0, batch).astype(np.float32)
    pos = rs.permutation(batch)[:batch // 5]
    value[pos] = np.array(SPECIALS, np.float32)[rs.randint(0, len(SPECIALS), pos.shape[0])]
    for k, (slot, last) in enumerate(((56, np.nan), (57, np.inf), (58, -1.0), (59, -np.inf), (60, 3.3e38), (61, -0.0))):
        where = np.arange(40 + k, batch, 67)  # ~60 writes spread over every block
        index[where], value[where] = slot, rs.uniform(0.0, 4.0, where.shape[0]).astype(np.float32)
        value[where[-1]] = last
    where = np.arange(46, batch, 61)
    index[where], value[where] = 62, np.array([np.nan, np.inf, -2.5], np.float32)[np.arange(where.shape[0]) % 3]
    where = np.arange(47, batch, 59)
    index[where], value[where] = 63, np.float32(np.nan)
    value[where[3]] = 2.25  # in block 0; every later writer of slot 63 is invalid
    for a in (prio, index, value):
        a.setflags(write=False)
    return UpdateCase(prio, index, value, slots, 0.05, 0.5, 41, (0, 4096))
