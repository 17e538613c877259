"""One conv layer's WEIGHT gradient on the CPU: the float64 / int64 reference, the float32 yardstick, a model of how the kernel cuts the batch
(chunks, staging rounds, image slots) that can be broken on purpose, and the data and case tables of tests/test_wgrad_layer_host.py and
tests/test_gpu_wgrad_layer.py (HipLearner.debug_wgrad: k_lc_wgrad, k_lc_wgrad_act, k_lc_wreduce of muzero_amd/csrc/mz_learn_conv.h).  numpy
only: importable without a GPU.

    dW[co][ci][ky][kx] = sum_{b, p} dy[b][co][p] * x[b][ci][p + (ky - 1, kx - 1)]      (zero outside the image)

with the staging transforms applied first: dy = c1 dz + c2 y + c3 per output channel, x' = relu(a x + b) per input channel, the dynamics
net's action planes behind the real channels (conv_layer_cases.full_input), and for the tile path the outer ring of every dy image set to 0."""
import functools

import numpy as np

import conv_layer_cases as cc

TAPMASKS = (0x010, 0x018, 0x012, 0x01b)  # the parity planes' tap sets of the stride-2 convs (learner_conv.hip par_tapmap)


# ------------------------------------------------------------------------------------------ the reference
def transform(dz, x, y=None, dcoef=None, xcoef=None, action=None, num_actions=0, cin=None, ring=False, dtype=np.float64):
    """(dy [B, cout, h, w], x' [B, cin, h, w]) in `dtype`: the operands the reduction multiplies."""
    dy = np.asarray(dz).astype(dtype)
    if dcoef is not None:
        c = np.asarray(dcoef).astype(dtype).reshape(3, 1, -1, 1, 1)
        dy = c[0] * dy + c[1] * np.asarray(y).astype(dtype) + c[2]
    if ring:
        dy = dy.copy()
        dy[:, :, 0, :] = 0
        dy[:, :, -1, :] = 0
        dy[:, :, :, 0] = 0
        dy[:, :, :, -1] = 0
    xt = np.asarray(x).astype(dtype)
    if xcoef is not None:
        a = np.asarray(xcoef).astype(dtype).reshape(2, 1, -1, 1, 1)
        xt = np.maximum(a[0] * xt + a[1], 0)
    return dy, cc.full_input(xt, action, num_actions, cin)


def _shifted(xf):
    """[9, B, C, h * w]: x at p + tap, zero outside the image."""
    B, C, h, w = xf.shape
    xp = np.zeros((B, C, h + 2, w + 2), xf.dtype)
    xp[:, :, 1:-1, 1:-1] = xf
    return np.stack([xp[:, :, ky:ky + h, kx:kx + w].reshape(B, C, h * w) for ky in range(3) for kx in range(3)])


def wgrad_images(dy, xf):
    """[B, cout, cin, 3, 3] float64: every image's own contribution.  Integer operands below 2^24 with a few thousand terms stay far under
    2^53: the float64 products and sums are then exact, and wgrad_acc's int64 result is this one converted."""
    B, co = dy.shape[:2]
    d = np.asarray(dy, np.float64).reshape(B, co, -1)
    xs = _shifted(np.asarray(xf, np.float64))
    return np.stack([np.matmul(d, xs[t].transpose(0, 2, 1)) for t in range(9)], axis=-1).reshape(B, co, xf.shape[1], 3, 3)


def wgrad_acc(dy, xf, dtype=np.float64):
    """sum over images and positions in float64, or (integer operands) exactly in int64."""
    out = _wgrad_sum(dy, xf)
    if dtype == np.int64:
        assert np.array_equal(np.rint(np.asarray(dy, np.float64)), dy) and np.array_equal(np.rint(np.asarray(xf, np.float64)), xf), 'int64 needs integer operands'
        assert float(_wgrad_sum(np.abs(dy), np.abs(xf)).max()) < 2.0 ** 52
        return np.rint(out).astype(np.int64)
    return out


def _wgrad_sum(dy, xf):
    """wgrad_images summed over the images, as one matrix product per tap (no per-image tensors: batches in the hundreds)."""
    B, co = dy.shape[:2]
    d = np.ascontiguousarray(np.asarray(dy, np.float64).reshape(B, co, -1).transpose(1, 0, 2)).reshape(co, -1)
    xs = _shifted(np.asarray(xf, np.float64))
    return np.stack([d @ np.ascontiguousarray(xs[t].transpose(1, 0, 2)).reshape(xf.shape[1], -1).T for t in range(9)], axis=-1).reshape(co, xf.shape[1], 3, 3)


def wgrad64(dz, x, dtype=np.float64, **kw):
    """The weight gradient [cout, cin, 3, 3] in float64 (dtype=np.int64: the exact integer twin); kw: transform's."""
    return wgrad_acc(*transform(dz, x, dtype=dtype, **kw), dtype=dtype)


def chain32(dz, x, **kw):
    """The same sum as ONE float32 chain per output element, sequential over (image, position) in image order, every product and every add
    rounded to float32; the transforms are applied in float32 first."""
    dy, xf = transform(dz, x, dtype=np.float32, **kw)
    B, co = dy.shape[:2]
    d = dy.reshape(B, co, -1)
    xs = _shifted(xf)  # [9, B, C, hw]
    acc = np.zeros((co, xf.shape[1], 9), np.float32)
    for b in range(B):
        for p in range(d.shape[2]):
            acc = acc + d[b, :, p].reshape(co, 1, 1) * xs[:, b, :, p].T.reshape(1, -1, 9)
    assert acc.dtype == np.float32
    return acc.reshape(co, xf.shape[1], 3, 3)


def apply_tapmask(ref, mask, preload=None):
    """What the output holds after a parity plane's launch (learner_conv.hip par_tapmap, k_lc_wreduce's tap map): accumulator tap (sy, sx) of the
    mask goes to weight tap (krow(p, sy), krow(q, sx)); every other weight tap keeps the preload (zeros)."""
    p, q = {0x010: (0, 0), 0x018: (0, 1), 0x012: (1, 0), 0x01b: (1, 1)}[mask]
    krow = lambda par, s: (1 if s == 1 else -1) if par == 0 else {0: 0, 1: 2}.get(s, -1)  # noqa: E731
    out = np.zeros_like(ref) if preload is None else np.asarray(preload).astype(ref.dtype).copy()
    for sy in range(3):
        for sx in range(3):
            ky, kx = krow(p, sy), krow(q, sx)
            assert ((mask >> (3 * sy + sx)) & 1) == (ky >= 0 and kx >= 0)
            if ky >= 0 and kx >= 0:
                out[:, :, ky, kx] = ref[:, :, sy, sx]
    return out


SLICES = {'whole': None, 'cout': (1, 2, 3), 'cin': (0, 2, 3), 'tap': (0, 1)}  # axes of [cout, cin, 3, 3] for conv_layer_cases.rel_rms


# ------------------------------------------------------------------------------------------ how the kernel cuts the batch
def structure(B, sg, ipw):
    """[chunk][round] -> the images of that staging round, in slot order: chunk c is images c ipw .. , a round is the next sg of them."""
    return [[list(range(r, min(r + sg, min(c + ipw, B)))) for r in range(c, min(c + ipw, B), sg)] for c in range(0, B, ipw)]


MUTATIONS = ('drop_last_image_of_chunk', 'stale_idle_slot', 'separator_leak', 'swap_dx', 'transpose_tile', 'drop_chunk', 'double_chunk',
             'ignore_accumulate', 'action_plus_one', 'ring_not_zeroed', 'ring_rows_shift')


def model(dz, x, sg=1, ipw=1, cols=True, preload=None, accumulate=False, mutation=None, img=None, **kw):
    """The reference again, built the way the kernel builds it -- per chunk a partial, per staging round the images of its slots -- so that one
    step can be done WRONGLY (`mutation`).  float64; exact on the integer classes.  With mutation=None it equals wgrad64 (+ preload)."""
    assert mutation is None or mutation in MUTATIONS
    ring = kw.get('ring', False)
    if mutation == 'action_plus_one':
        kw = dict(kw, action=(np.asarray(kw['action']) + 1) % kw['num_actions'])
    if mutation == 'ring_not_zeroed':
        kw = dict(kw, ring=False)
    dy, xf = transform(dz, x, **kw)
    if mutation == 'ring_rows_shift':  # the x planes one row off against dy
        xf = np.concatenate([xf[:, :, 1:], np.zeros_like(xf[:, :, :1])], axis=2)
    assert ring or mutation not in ('ring_not_zeroed', 'ring_rows_shift')
    B, h, w = dy.shape[0], dy.shape[2], dy.shape[3]
    if img is None or mutation in ('action_plus_one', 'ring_not_zeroed', 'ring_rows_shift'):  # (img: wgrad_images of the unbroken operands, made once)
        img = wgrad_images(dy, xf)
    parts = []
    for chunk in structure(B, sg, ipw):
        part = np.zeros(img.shape[1:])
        last = chunk[-1][-1]
        for ri, rnd in enumerate(chunk):
            for b in rnd:
                if not (mutation == 'drop_last_image_of_chunk' and b == last):
                    part += img[b]
            if mutation == 'stale_idle_slot' and ri > 0:  # the slots this round leaves idle still hold the previous round's images
                for b in chunk[ri - 1][len(rnd):]:
                    part += img[b]
            if mutation == 'separator_leak' and cols:  # image g's last column as the left neighbour of image g + 1's first column
                for g0, g1 in zip(rnd[:-1], rnd[1:]):
                    xl = np.zeros((xf.shape[1], h + 2))
                    xl[:, 1:-1] = xf[g0, :, :, w - 1]
                    for ky in range(3):
                        part[:, :, ky, 0] += dy[g1, :, :, 0] @ xl[:, ky:ky + h].T
        parts.append(part)
    if mutation == 'drop_chunk':
        parts = parts[:-1]
    if mutation == 'double_chunk':
        parts = parts + parts[:1]
    out = sum(parts, np.zeros(img.shape[1:]))
    if mutation == 'swap_dx':
        out = out[:, :, :, ::-1].copy()
    if mutation == 'transpose_tile':
        co, ci = out.shape[:2]
        pad = np.zeros((-(-co // 16) * 16, -(-ci // 16) * 16, 3, 3))
        pad[:co, :ci] = out
        t = pad.reshape(pad.shape[0] // 16, 16, pad.shape[1] // 16, 16, 3, 3).transpose(0, 3, 2, 1, 4, 5).reshape(pad.shape)
        out = t[:co, :ci].copy()
    if preload is not None and accumulate and mutation != 'ignore_accumulate':
        out = out + np.asarray(preload, np.float64)
    return out


# ------------------------------------------------------------------------------------------ shapes and runs
# (board, cin_real, cin, num_actions, cout, batch)
SHAPES = {
    'b3_9to16_n5': (3, 9, 9, 0, 16, 5),            # hw % 4 != 0; with SG forced: many images per round, batch not a multiple of SG
    'b5_40to24_n7': (5, 40, 40, 0, 24, 7),         # hw = 25, channels off 16 and 32, odd ci_tiles
    'b6_128to128_n11': (6, 128, 128, 0, 128, 11),  # several blocks; with SG / ipw forced: short last chunk AND short last round
    # batches at which the update ITSELF reaches the edges (make_geom and Sched::wgrad_ops on 256 CUs, no override):
    'b3_9to16_n2003': (3, 9, 9, 0, 16, 2003),      # 3 x 3: SG = 8 side by side, 251 chunks of one round, the last chunk 3 images: many images per round, batch off SG
    'b6_128to128_n73': (6, 128, 128, 0, 128, 73),  # SG = 5 (over 4): 15 chunks of one round, the last one 3 images -- a short last chunk AND a short last round
    'b6_128to128_n128': (6, 128, 128, 0, 128, 128),  # SG = 4 (over 5): 32 chunks of 4 -- the choice make_geom's comment describes; 32 groups: XCD remap on
    'b6_128to128_n8': (6, 128, 128, 0, 128, 8),    # 8 chunks of 4 x 4 blocks: the smallest launch whose XCD remap moves workgroups
    'b9_8to8_n1': (9, 8, 8, 0, 8, 1),              # one image, one chunk, everything padded
    'b13_24to24_n3': (13, 24, 24, 0, 24, 3),
    'b15_35to20_n3': (15, 35, 35, 0, 20, 3),       # SG = 1, the largest LDS
    'b9_32a82to32_n5': (9, 32, 114, 82, 32, 5),    # the sparse action route by the update's rule (six extra tiles)
    'b3_16a10to16_n5': (3, 16, 26, 10, 16, 5),     # fewer than four extra tiles: in-kernel planes by the update's rule
    # second layers of the pairs
    'b6_40to24_n11': (6, 40, 40, 0, 24, 11),
    'b9_8to8_n4': (9, 8, 8, 0, 8, 4),
    'b9_8to8_n4b': (9, 8, 8, 0, 8, 4),             # (another seed)
    'b9_8to8_n5': (9, 8, 8, 0, 8, 5),
    'b6_64to64_n4': (6, 64, 64, 0, 64, 4),
    'b6_64to64_n4b': (6, 64, 64, 0, 64, 4),
}
ATARI_TILES = {'t14x14_128to128_n3': (14, 14, 128, 128, 3), 't14x18_128to128_n2': (14, 18, 128, 128, 2), 't14x18_4to128_n2': (14, 18, 4, 128, 2),
               't14x14_4to16_n3': (14, 14, 4, 16, 3)}


def _run(shape, expect, **over):
    return dict(shape=shape, over=over, expect=expect)


def E(sg, layout, ipw, act='none', remap=None):
    return dict(sg=sg, layout=layout, ipw=ipw, act=act, remap=remap)  # remap None: not asserted (0 wherever the group count is no multiple of 8)


# What the hook must report for each run: SG, the planes' layout ('single' | 'cols' | 'rows'), images per chunk, the action route -- written down
# from make_geom and Sched::wgrad_ops for a 256-CU device; the GPU test fails with the name if the kernel ran something else.
PLAIN_RUNS = {
    'b3_9to16_n5': _run('b3_9to16_n5', E(1, 'single', 1)),
    'b5_40to24_n7': _run('b5_40to24_n7', E(1, 'single', 1)),
    'b6_128to128_n11': _run('b6_128to128_n11', E(1, 'single', 1)),
    'b3_9to16_n2003': _run('b3_9to16_n2003', E(8, 'cols', 8, remap=0)),
    'b6_128to128_n73': _run('b6_128to128_n73', E(5, 'cols', 5, remap=0)),
    'b6_128to128_n128': _run('b6_128to128_n128', E(4, 'cols', 4, remap=1)),
    # the XCD remap at 4 x 4 blocks per chunk: on (the update's choice: 8 groups) it permutes the workgroups, off it is the launch order
    'b6_128to128_n8': _run('b6_128to128_n8', E(1, 'single', 1, remap=1)),
    'b6_128to128_n8-remap-off': _run('b6_128to128_n8', E(1, 'single', 1, remap=0), remap=2),
    'b6_128to128_n128-remap-off': _run('b6_128to128_n128', E(4, 'cols', 4, remap=0), remap=2),
    'b9_8to8_n1': _run('b9_8to8_n1', E(1, 'single', 1)),
    'b13_24to24_n3': _run('b13_24to24_n3', E(1, 'single', 1)),
    'b15_35to20_n3': _run('b15_35to20_n3', E(1, 'single', 1)),
    'b9_32a82to32_n5': _run('b9_32a82to32_n5', E(1, 'single', 1, 'sparse')),
    'b9_32a82to32_n5-kernel': _run('b9_32a82to32_n5', E(1, 'single', 1, 'kernel'), act_route=1),
    'b3_16a10to16_n5': _run('b3_16a10to16_n5', E(1, 'single', 1, 'kernel')),
    'b3_16a10to16_n5-sparse': _run('b3_16a10to16_n5', E(1, 'single', 1, 'sparse'), act_route=2),
    'b3_16a10to16_n5-sg4': _run('b3_16a10to16_n5', E(4, 'cols', 4, 'kernel'), sg=4),  # the in-kernel planes of images side by side
    # images per chunk forced on the 6 x 6 shape (SG = 4, side by side): 1, SG, B, and 5 -- chunks of 5, 5, 1: two rounds of 4 + 1, a chunk of one image
    'b6_128to128_n11-sg4-ipw1': _run('b6_128to128_n11', E(4, 'cols', 1), sg=4, ipw=1),
    'b6_128to128_n11-sg4-ipw4': _run('b6_128to128_n11', E(4, 'cols', 4), sg=4, ipw=4),
    'b6_128to128_n11-sg4-ipw11': _run('b6_128to128_n11', E(4, 'cols', 11), sg=4, ipw=11),
    'b6_128to128_n11-sg4-ipw5': _run('b6_128to128_n11', E(4, 'cols', 5), sg=4, ipw=5),
    'b5_40to24_n7-sg3-ipw7': _run('b5_40to24_n7', E(3, 'cols', 7), sg=3, ipw=7),  # one chunk, rounds of 3, 3, 1: two idle slots over a full round
    'b5_40to24_n7-sg3-rows-ipw7': _run('b5_40to24_n7', E(3, 'rows', 7), sg=3, layout=2, ipw=7),
    'b6_128to128_n11-sg4-ipw8': _run('b6_128to128_n11', E(4, 'cols', 8), sg=4, ipw=8),  # a short last chunk (3 images) whose only round is short
}
# every SG the staging lanes and the LDS allow on the three smallest boards, side by side (layout 1) and stacked (2); ipw follows as whole rounds
SG_LIMITS = {'b3_9to16_n5': (16, 16), 'b5_40to24_n7': (8, 6), 'b6_128to128_n11': (5, 5)}  # (side by side, stacked); 3 x 3: the update's cap of 16
for _s, (_nc, _nr) in SG_LIMITS.items():
    for _lay, _n in ((1, _nc), (2, _nr)):
        for _sg in range(1, _n + 1):
            PLAIN_RUNS[f'{_s}-sg{_sg}-{"cols" if _lay == 1 else "rows"}'] = _run(
                _s, E(_sg, 'single' if _sg == 1 else ('cols' if _lay == 1 else 'rows'), _sg), sg=_sg, layout=_lay)
SG_REFUSED = {'b5_40to24_n7': ((1, 9), (2, 7)), 'b6_128to128_n11': ((1, 6), (2, 6)), 'b15_35to20_n3': ((1, 2),)}  # (layout, SG): over the budget

ACCUMULATE_RUNS = ('b5_40to24_n7', 'b6_128to128_n11-sg4-ipw5', 'b9_32a82to32_n5', 'b3_16a10to16_n5')
TRANSFORM_RUNS = ('b5_40to24_n7', 'b6_128to128_n11-sg4-ipw5', 'b9_8to8_n1', 'b15_35to20_n3')
# pairs: (first, second, overrides) -> expected (SG, ipw, remap flag of the launch).  A paired launch has one workgroup per CU of its own.
PAIR_RUNS = {
    # ci_tiles 8 | 3, cout 128 | 24: the second job's workgroups past its own input-channel blocks return early; the grids differ: never remapped
    'different_grids': ('b6_128to128_n11', 'b6_40to24_n11', dict(), (1, 1, 0)),
    'different_grids_sg4': ('b6_128to128_n11', 'b6_40to24_n11', dict(sg=4, remap=1), (4, 4, 0)),
    # two equal grids, 4 + 4 chunks: a group count the 8 XCDs divide
    'equal_remap_on': ('b9_8to8_n4', 'b9_8to8_n4b', dict(remap=1), (1, 1, 1)),
    'equal_remap_off': ('b9_8to8_n4', 'b9_8to8_n4b', dict(remap=2), (1, 1, 0)),
    # (one block per chunk above: the remap is the identity there.)  2 x 2 blocks per chunk, 4 + 4 chunks: the remap moves every workgroup
    'equal_blocks_remap_on': ('b6_64to64_n4', 'b6_64to64_n4b', dict(remap=1), (1, 1, 1)),
    'equal_blocks_remap_off': ('b6_64to64_n4', 'b6_64to64_n4b', dict(remap=2), (1, 1, 0)),
}
# steps: (shape, nsrc, overrides) -> expected (SG, ipw, cps)
STEP_RUNS = {
    'b6_n11_k2': ('b6_128to128_n11', 2, dict(), (1, 1, 11)),
    'b6_n11_k2_sg4': ('b6_128to128_n11', 2, dict(sg=4), (4, 4, 3)),
    'b6_n11_k5': ('b6_128to128_n11', 5, dict(), (1, 2, 6)),
    'b6_n11_k5_cps1': ('b6_128to128_n11', 5, dict(ipw=11), (1, 11, 1)),
    'b9_n5_k2_cps1': ('b9_8to8_n5', 2, dict(ipw=5), (1, 5, 1)),
    'b9_n5_k5': ('b9_8to8_n5', 5, dict(), (1, 1, 5)),
}
# ring: (tile, ring_rows) the update's conditions allow: 14 x 14 (pitch 16, 12 inner columns) 0, 1, 3; 14 x 18 (pitch 20, 16 inner columns) 0, 1, 2
# third entry: images per chunk forced (0: the update's -- one tile per workgroup at these batches; B: every tile in ONE workgroup, a staging round per
# tile over the same planes, as the update's batch x tiles images give it -- the spare dy tail and the shifted x rows are rewritten round after round)
RING_RUNS = [('t14x14_128to128_n3', 0, 0), ('t14x14_128to128_n3', 1, 0), ('t14x14_128to128_n3', 3, 0), ('t14x18_128to128_n2', 0, 0), ('t14x18_128to128_n2', 1, 0),
             ('t14x18_128to128_n2', 2, 0), ('t14x18_4to128_n2', 2, 0), ('t14x14_4to16_n3', 3, 0),
             ('t14x14_128to128_n3', 0, 3), ('t14x14_128to128_n3', 1, 3), ('t14x14_128to128_n3', 3, 3), ('t14x18_128to128_n2', 1, 2), ('t14x18_128to128_n2', 2, 2),
             ('t14x14_4to16_n3', 3, 2)]
RING_REFUSED = [('t14x14_4to16_n3', 2), ('t14x18_4to128_n2', 3)]
RING_NSTEPS = {(14, 14, 0): 14, (14, 14, 1): 12, (14, 14, 3): 9, (14, 18, 0): 18, (14, 18, 1): 15, (14, 18, 2): 12}


# ------------------------------------------------------------------------------------------ integer data
CLASSES = ('locator', 'dense', 'wide')
WIDE_MAX = (1 << 18) - 1


def _seed(key, cls, k=0):
    names = sorted(SHAPES) + sorted(ATARI_TILES)
    return 1000 * names.index(key) + 100 * CLASSES.index(cls) + k


def locator_required(h, w, B, sg, ipw, ring=False):
    """(image, position) pairs a Locator's one-hot dz must visit: the four corners and edges, the last pixel, the first and last column AND the
    first and last row of every image slot of a staging round (the separator is a zero column side by side, a zero row stacked), an image of a
    short last round, the first and last image of a short last chunk; ring: ring pixels and the inner pixels next to the tile's rows 0 and h - 1."""
    req, st = [], structure(B, sg, ipw)
    mid_r, mid_c = h // 2, w // 2
    spots = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (0, mid_c), (h - 1, mid_c), (mid_r, 0), (mid_r, w - 1), (h - 1, w - 1)]
    if ring:
        spots += [(1, 1), (1, w - 2), (h - 2, 1), (h - 2, w - 2), (1, mid_c), (h - 2, mid_c), (mid_r, 1), (mid_r, w - 2)]
    for i, (r, c) in enumerate(spots):
        req.append((i % B, r * w + c))
    big = max((rnd for ch in st for rnd in ch), key=len)  # a fullest round: one image per slot
    for gi, b in enumerate(big):
        r = gi % h
        req += [(b, r * w), (b, r * w + w - 1), (b, gi % w), (b, (h - 1) * w + gi % w)]
    for ch in st:
        if len(ch[-1]) < sg:
            req.append((ch[-1][-1], (h // 2) * w + w // 2))
            break
    if B % ipw:
        last = st[-1]
        req += [(last[0][0], 1 % (h * w)), (last[-1][-1], (h * w - 2) % (h * w))]
    return list(dict.fromkeys(req))


def locator_x(B, cr, h, w):
    """x[b][ci][p] = 1 + b hw + p + ci (B hw + 1): a distinct integer for every (image, channel, position); 0 is 'nothing read'."""
    code = 1 + np.arange(B * h * w).reshape(B, 1, h, w)
    return (code + np.arange(cr).reshape(1, cr, 1, 1) * (B * h * w + 1)).astype(np.float32)


def locator_draws(key, B, cr, cout, h, w, sg, ipw, ring=False, max_draws=6):
    """[(dz, x)]: dz one-hot per output channel, channel co of draw d at required pair (d cout + co) % n."""
    req = locator_required(h, w, B, sg, ipw, ring)
    x = locator_x(B, cr, h, w)
    n_draws = min(max_draws, -(-len(req) // cout))
    assert n_draws * cout >= len(req), (key, len(req), cout)
    draws = []
    for d in range(n_draws):
        dz = np.zeros((B, cout, h, w), np.float32)
        for co in range(cout):
            b, p = req[(d * cout + co) % len(req)]
            dz[b, co, p // w, p % w] = 1.0
        draws.append((dz, x))
    return draws


def locator_visited(draws):
    return {(int(b), int(r) * dz.shape[3] + int(c)) for dz, _ in draws for b, _, r, c in np.argwhere(dz != 0)}


def dense_draw(seed, B, cr, cout, h, w):
    """Small integers on every position of both operands."""
    rs = np.random.RandomState(seed)
    dz = rs.choice([-2, -1, 1, 2], (B, cout, h, w)).astype(np.float32)
    x = rs.choice([-3, -2, -1, 1, 2, 3], (B, cr, h, w)).astype(np.float32)
    return dz, x


def _sparse_dz(rs, B, cout, h, w, nnz, mags):
    dz = np.zeros((B, cout, h * w), np.float32)
    for co in range(cout):
        for _ in range(nnz):
            dz[rs.randint(B), co, rs.randint(h * w)] = rs.choice(mags) * rs.choice([-1, 1])
    return dz.reshape(B, cout, h, w)


def wide_draws(seed, B, cr, cout, h, w):
    """Sparse operands whose products need most of a float32 mantissa, a few per output: (18-bit dy, two per channel) x (5-bit x); (5-bit dy) x
    (18-bit x, 30 % dense); (12-bit dy, one per channel) x (12-bit x): sum |dy x| stays under 2 * (2^18 - 1) * 31 < 2^24."""
    rs = np.random.RandomState(seed)
    pool18, pool12 = cc.int_pool(WIDE_MAX), cc.int_pool((1 << 12) - 1)
    shape = (B, cr, h, w)
    small = np.arange(1, 32)
    a = (_sparse_dz(rs, B, cout, h, w, 2, pool18), (rs.choice(small, shape) * rs.choice([-1, 1], shape) * (rs.rand(*shape) < 0.5)).astype(np.float32))
    b = (_sparse_dz(rs, B, cout, h, w, 2, small), (rs.choice(pool18, shape) * rs.choice([-1, 1], shape) * (rs.rand(*shape) < 0.3)).astype(np.float32))
    c = (_sparse_dz(rs, B, cout, h, w, 1, pool12), (rs.choice(pool12, shape) * rs.choice([-1, 1], shape)).astype(np.float32))
    return [a, b, c]


def wide_transform_draw(seed, B, cr, cout, h, w):
    """dict(dz, x, y, dcoef, xcoef) of the Wide class with small integer coefficients: dy = c1 dz + c2 y + c3 with c1 in +-{1, 2, 3}, c2 in
    {-1, 1}, c3 in {-1, 0, 0, 1} (a non-zero c3 makes that channel's dy dense), x' = relu(a x + b) with a in {1, 2, 3} and b in {-600 .. -1}:
    the ReLU zeroes every negative x and the small positive ones.  10-bit magnitudes: |dy| <= 3 * 1023 + 31, x' <= 3 * 1023."""
    rs = np.random.RandomState(seed)
    pool = cc.int_pool((1 << 10) - 1)
    dz = _sparse_dz(rs, B, cout, h, w, 2, pool)
    y = ((dz != 0) * rs.randint(-31, 32, dz.shape)).astype(np.float32)
    shape = (B, cr, h, w)
    x = (rs.choice(pool, shape) * rs.choice([-1, 1], shape) * (rs.rand(*shape) < 0.5)).astype(np.float32)
    dcoef = np.stack([rs.choice([-3, -2, -1, 1, 2, 3], cout), rs.choice([-1, 1], cout), rs.choice([-1, 0, 0, 1], cout)]).astype(np.float32)
    xcoef = np.stack([rs.choice([1, 2, 3], cr), -rs.randint(1, 601, cr)]).astype(np.float32)
    return dict(dz=dz, x=x, y=y, dcoef=dcoef, xcoef=xcoef)


def actions(B, A):
    return (np.arange(B) * 37 % A).astype(np.int32) if A else None


@functools.lru_cache(maxsize=None)
def int_draws(key, cls, sg=1, ipw=1):
    """[(dz, x)] of class `cls` for a shape of SHAPES; the Locator's positions depend on how the run cuts the batch (sg, ipw)."""
    board, cr, cin, A, cout, B = SHAPES[key]
    if cls == 'locator':
        out = locator_draws(key, B, cr, cout, board, board, sg, ipw)
    elif cls == 'dense':
        out = [dense_draw(_seed(key, cls), B, cr, cout, board, board)]
    else:
        out = wide_draws(_seed(key, cls), B, cr, cout, board, board)
    for dz, x in out:
        dz.setflags(write=False)
        x.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tile_draws(key, cls):
    h, w, cr, cout, B = ATARI_TILES[key]
    if cls == 'locator':
        return locator_draws(key, B, cr, cout, h, w, 1, 1, ring=True)
    if cls == 'dense':
        return [dense_draw(_seed(key, cls), B, cr, cout, h, w)]
    return wide_draws(_seed(key, cls), B, cr, cout, h, w)


def int_bound(dz, x, **kw):
    """(max over outputs of sum |dy x'|, max |dy|, max |x'|, all integers): under 2^24 each, every partial sum of every order is an exact float32."""
    dy, xf = transform(dz, x, **kw)
    whole = np.array_equal(dy, np.rint(dy)) and np.array_equal(xf, np.rint(xf))
    return float(wgrad_acc(np.abs(dy), np.abs(xf)).max()), float(np.abs(dy).max()), float(np.abs(xf).max()), whole


def first_difference(out, ref):
    """None, or a message naming the first differing element."""
    bad = np.argwhere(np.asarray(out) != np.asarray(ref))
    if len(bad) == 0:
        return None
    i = tuple(bad[0])
    return f'{len(bad)} of {np.asarray(ref).size} elements differ, first at (co, ci, ky, kx) = {bad[0].tolist()}: kernel {np.asarray(out)[i]!r} != reference {np.asarray(ref)[i]!r}'


def locate(value, B, cr, h, w):
    """What a Locator value says was read: 'image b channel ci position (r, c)'."""
    v = int(value)
    if v <= 0:
        return 'nothing (0)'
    ci, code = divmod(v, B * h * w + 1)
    b, p = divmod(code - 1, h * w)
    return f'x[image {b}][channel {ci}][({p // w}, {p % w})]'
