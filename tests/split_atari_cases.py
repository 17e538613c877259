"""One stride-1 conv of the Atari learner's tile path (muzero_amd/csrc/learner_conv.hip AtariRun, the HALO / PLANE builds of
muzero_amd/csrc/mz_learn_conv_split.h) on the CPU: a model of the route -- cut the plane into tiles with their halo, convolve the inner positions of
each tile in the split arithmetic, write them back into the plane -- and the data of tests/test_split_atari_learner_host.py and
tests/test_gpu_split_atari_learner.py.  numpy only; builds on tests/conv_layer_cases.py (classes W, X, M, split3, the references) and takes the
Locator's coded input from tests/wgrad_layer_cases.py.

`bug=` re-introduces ONE deliberate mistake (MUTATIONS) into the model: the host file shows that the integer data tells each of them from the
int64 conv, so the GPU test, which runs the same data, would."""
import zlib

import numpy as np

import conv_layer_cases as cc
from conv_fused_cases import dgrad_weight
from wgrad_layer_cases import locator_x

TILE = 12
MUTATIONS = tuple('drop_' + t for t in cc.TERMS) + ('seam_shift', 'halo_not_zeroed', 'last_block')
PLANES = {'p24': (24, 24), 'p48': (48, 48)}         # 2 x 2 tiles of 12 x 12; 4 x 3 wide tiles of 12 x 16
CHANNELS = ((16, 16), (48, 24), (32, 32))          # (cin, cout) of the LAYER: 48 -> 24 has a partial 32-channel block and a partial output tile
BATCHES = (1, 2)
CLASSES = tuple(cc.INT_CLASSES) + ('locator',)


def tile_w(W, wide=True):
    """AtariRun::tile_w: 16 columns where the plane's width divides into at least three such tiles, else 12."""
    return 16 if wide and W % 16 == 0 and W // 16 >= 3 else TILE


def cut_tiles(x, tw, bug=None):
    """k_lc_tile_gather: [B, C, H, W] -> [B * nty * ntx, C, 14, tw + 2], the tiles with their one-position halo, zero outside the plane."""
    B, C, H, W = x.shape
    xp = np.zeros((B, C, H + 2, W + 2), x.dtype)
    xp[:, :, 1:-1, 1:-1] = x
    if bug == 'halo_not_zeroed':  # the halo column left of the plane repeats the plane's first column
        xp[:, :, 1:-1, 0] = x[:, :, :, 0]
    nty, ntx = H // TILE, W // tw
    out = np.zeros((B, nty, ntx, C, TILE + 2, tw + 2), x.dtype)
    for ty in range(nty):
        for tx in range(ntx):
            x0 = tx * tw + (1 if bug == 'seam_shift' and tx > 0 else 0)  # every seam one column to the right
            col = xp[:, :, ty * TILE:ty * TILE + TILE + 2, x0:x0 + tw + 2]
            out[:, ty, tx, :, :, :col.shape[3]] = col
    return out.reshape(B * nty * ntx, C, TILE + 2, tw + 2)


def put_tiles(inner, B, H, W, tw):
    """The PLANE epilogue (or k_lc_tile_scatter): inner positions [B * tiles, C, 12, tw] -> the plane [B, C, H, W]."""
    nty, ntx = H // TILE, W // tw
    t = inner.reshape(B, nty, ntx, inner.shape[1], TILE, tw)
    return np.ascontiguousarray(t.transpose(0, 3, 1, 4, 2, 5)).reshape(B, inner.shape[1], H, W)


def tile_conv_model(x, w, exact=False, wide=True, bug=None):
    """conv(x [B, cin, H, W], w [cout, cin, 3, 3]) as the tile path's split builds sum it: per tile, per 32-channel block of the input, the six
    issued terms hh, hm, mh, hl, lh, mm of the split operands, inner positions only.  float64 (or, exact=True on integer data, int64)."""
    B, cin, H, W = x.shape
    tw = tile_w(W, wide)
    dtype = np.int64 if exact else np.float64
    X, Wt = cc.split3(x), cc.split3(w)
    tiles = [cut_tiles(t, tw, bug) for t in X]
    n_cb = cin // 32 if bug == 'last_block' else -(-cin // 32)  # the mistake: whole blocks only
    acc = np.zeros((tiles[0].shape[0], w.shape[0], TILE, tw), dtype)
    for cb in range(n_cb):
        sl = slice(32 * cb, min(32 * cb + 32, cin))
        for name, (a, b) in cc.TERMS.items():
            if bug == 'drop_' + name:
                continue
            acc += cc.conv_acc(tiles[a][:, sl], Wt[b][:, sl], dtype)[:, :, 1:-1, 1:-1]  # (the haloed tile zero-padded once more: its inner outputs are the valid conv)
    return put_tiles(acc, B, H, W, tw)


# ------------------------------------------------------------------------------------------ integer data
def _seed(*key):
    return zlib.crc32(repr(key).encode()) % (1 << 31)


def seam_positions(H, W, wide=True):
    """(row, column) on both sides of every tile seam, in the plane's corners and in each tile's corners: where a Locator value must be right."""
    tw = tile_w(W, wide)
    rows = sorted({0, H - 1} | {r for s in range(TILE, H, TILE) for r in (s - 1, s)})
    cols = sorted({0, W - 1} | {c for s in range(tw, W, tw) for c in (s - 1, s)})
    return [(r, c) for r in rows for c in cols]


def locator_weights(c_in, c_out, draw):
    """One-hot weights: output channel co reads input channel (7 co + draw) % c_in through tap (co + 4 draw) % 9 -- with the coded input, an output
    value names the (image, channel, position) that was read."""
    w = np.zeros((c_out, c_in, 3, 3), np.float32)
    for co in range(c_out):
        tap = (co + 4 * draw) % 9
        w[co, (7 * co + draw) % c_in, tap // 3, tap % 3] = 1.0
    return w


def int_case(cls, plane, chan, B, direction):
    """(input [B, c_in, H, W], [conv weight [c_out, c_in, 3, 3]]) of class `cls` for the conv the hook runs in `direction` on layer `chan`: the
    data gradient convolves dy [B, cout, H, W] with the transposed, tap-flipped weight.  W, X, M (tests/conv_layer_cases.py): the first, a middle and
    the last draw group (three input channels each: the last sits in the partial 32-channel block where there is one), every part of a group."""
    H, W = PLANES[plane]
    cin, cout = chan
    c_in, c_out = (cin, cout) if direction == 0 else (cout, cin)
    seed = _seed(cls, plane, chan, B, direction)
    if cls == 'locator':
        return locator_x(B, c_in, H, W), [locator_weights(c_in, c_out, d) for d in range(2)]
    x = cc.int_input(cls, seed, B, c_in, H, W)
    draws = cc.int_draws(cls, seed + 1, c_in, c_out)
    groups = -(-c_in // 3)
    parts = len(draws) // groups
    keep = sorted({0, groups // 2, groups - 1})
    return x, [draws[g * parts + p][0] for g in keep for p in range(parts)]


def hook_weight(w_conv, direction):
    """The LAYER's weight [cout, cin, 3, 3] the hook takes, from the weight of the conv it then runs."""
    return w_conv if direction == 0 else dgrad_weight(w_conv)


def epilogue_operands(plane, chan, B, direction):
    """Integer skip, mask, mcoef and partner planes of the conv's output shape: small values, a third of the mask at or below zero."""
    H, W = PLANES[plane]
    c_out = chan[1] if direction == 0 else chan[0]
    rs = np.random.RandomState(_seed('epi', plane, chan, B, direction))
    shape = (B, c_out, H, W)
    skip = rs.randint(-500, 501, shape).astype(np.float32)
    mask = rs.randint(-2, 5, shape).astype(np.float32)
    mcoef = np.stack([rs.choice([-1.0, 1.0, 2.0], c_out), rs.randint(-2, 3, c_out)]).astype(np.float32)
    partner = rs.randint(-3, 4, shape).astype(np.float32)
    return skip, mask, mcoef, partner


def small_case(plane, chan, B, direction):
    """x and w in {-1, 0, 1} with weights on three input channels: |y| <= 27, so a tile's statistics partials are exact float32 sums as well."""
    H, W = PLANES[plane]
    c_in, c_out = chan if direction == 0 else chan[::-1]
    rs = np.random.RandomState(_seed('small', plane, chan, B, direction))
    x = rs.randint(-1, 2, (B, c_in, H, W)).astype(np.float32)
    w = np.zeros((c_out, c_in, 3, 3), np.float32)
    ch = rs.choice(c_in, 3, replace=False)
    w[:, ch] = rs.randint(-1, 2, (c_out, 3, 3, 3)).astype(np.float32)
    return x, w
