"""The Atari representation's launches outside its stride-1 convs (muzero_amd/csrc/learner_conv.hip AtariRun: s2_fwd, s2_dgrad, pool_fwd, pool_bwd,
relu_bwd, entry, entry12, gather, scatter; launch_entry, launch_normalize) on the CPU: numpy references, models of the route the kernels take, and the
seeded data of tests/test_atari_stage_host.py and tests/test_gpu_atari_stage.py.  numpy only; builds on tests/split_atari_cases.py (cut_tiles,
put_tiles, tile_w, locator_weights, _seed), tests/conv_layer_cases.py (conv_acc) and tests/wgrad_layer_cases.py (locator_x).

The stride-2 conv and its data gradient have TWO references each: a direct int64 sum over (2 oy + ky - 1, 2 ox + kx - 1) with zero padding, and a
model of the route -- parity planes, tap maps, accumulation, tiles.  `bug=` plants ONE deliberate mistake (MUTATIONS) into a model: the host file
shows that the committed data tells each of them from the reference, so the GPU test, which runs the same data, would."""
import numpy as np

import conv_layer_cases as cc
import split_atari_cases as sa
from split_atari_cases import TILE, _seed, cut_tiles, locator_weights, put_tiles, tile_w
from wgrad_layer_cases import locator_x

MUTATIONS = ('parity_swapped', 'odd_plane_origin', 'plane_overwrites', 'edge_repeats', 'dgrad_forward_taps', 'pool_valid_count', 'pool_bwd_window',
             'argmin_last', 'minmax_terms_swapped', 'scale_dropped', 'mask_ge', 'pivot_zero', 'inner_only_ignored', 'bnbwd_coef_order')

# (cin, cout, out H, out W, B): the smallest shapes that reach each build and edge
S2_FWD = ((4, 16, 24, 24, 2),     # 12 x 12 tiles, four of them, seams both ways
          (3, 16, 48, 48, 1),     # a 96 x 96 source: 16-wide tiles (NPT 16 builds), a partial channel quad
          (20, 24, 24, 24, 1),    # a partial 16-block and a partial output tile
          (128, 16, 24, 24, 1))   # conv_2's depth
S2_DGRAD = ((16, 32, 24, 24, 2), (8, 128, 24, 24, 1))   # the LAYER's (cin, cout), dy H x W, B
S2_DGRAD_WIDE = (8, 16, 48, 48, 1)                      # dy 48 x 48: 16-wide tiles, which the compact data-gradient tap sets are not built for
S2_CLASSES = ('locator', 'small')
POOLS = ((24, 24), (12, 12), (6, 6), (12, 24))          # the pooled plane's source, B * C = 3 * 5 (no multiple of 256 elements)
ENTRY_C = (8, 13, 24, 72, 136)                          # CPT 2, 2 with a ragged last group, 8, 16, 32
ENTRY_HW = {36: (6, 6), 144: (12, 12), 576: (24, 24), 2304: (48, 48)}
ENTRY_CLASSES = ('pow2', 'ties', 'flat', 'float')
EXACT_CLASSES = ('pow2', 'ties')


# ------------------------------------------------------------------------------------------ tap maps (learner_conv.hip par_row, par_row_d)
def par_row(p, s):
    """Forward: stride-1 tap s of parity plane p is weight tap par_row(p, s) (-1: none).  Row 2 oy + ky - 1: ky = 1 is the even plane's row oy, ky = 0 / 2
    are the odd plane's rows oy - 1 / oy."""
    return (1 if s == 1 else -1) if p == 0 else {0: 0, 1: 2}.get(s, -1)


def par_row_d(p, s):
    """Data gradient: dx row 2 y + p collects dy row y + s - 1 through weight tap par_row_d(p, s): p = 0 -> ky = 1 at s = 1; p = 1 -> ky = 0 from dy row
    y + 1 (s = 2) and ky = 2 from dy row y (s = 1)."""
    return (1 if s == 1 else -1) if p == 0 else {2: 0, 1: 2}.get(s, -1)


def par_tapmap(p, q, dgrad):
    f = par_row_d if dgrad else par_row
    return [(f(p, sy) * 3 + f(q, sx)) if f(p, sy) >= 0 and f(q, sx) >= 0 else -1 for sy in range(3) for sx in range(3)]


def par_tapmask(p, q, dgrad):
    return sum(1 << t for t, m in enumerate(par_tapmap(p, q, dgrad)) if m >= 0)


FWD_MASKS = tuple(par_tapmask(pq >> 1, pq & 1, False) for pq in range(4))    # 0x010, 0x018, 0x012, 0x01b
DGRAD_MASKS = tuple(par_tapmask(pq >> 1, pq & 1, True) for pq in range(4))   # 0x010, 0x030, 0x090, 0x1b0


def _plane_weight(w, p, q, dgrad, forward_taps=False):
    """The stride-1 kernel a parity plane's tiles are convolved with (k_lc_pack_par): tap t is weight tap tapmap[t], zero where the plane has none; the
    data gradient's copy is transposed ([cin][cout])."""
    m = par_tapmap(p, q, dgrad and not forward_taps)
    src = np.transpose(w, (1, 0, 2, 3)) if dgrad else w
    out = np.zeros(src.shape, w.dtype)
    for t, k in enumerate(m):
        if k >= 0:
            out[:, :, t // 3, t % 3] = src[:, :, k // 3, k % 3]
    return out


# ------------------------------------------------------------------------------------------ stride-2 conv: the direct sums
def s2_direct(x, w):
    """y[b, co, oy, ox] = sum x[b, ci, 2 oy + ky - 1, 2 ox + kx - 1] w[co, ci, ky, kx], zero padding; int64."""
    B, cin, H2, W2 = x.shape
    H, W = H2 // 2, W2 // 2
    xp = np.zeros((B, cin, H2 + 2, W2 + 2), np.int64)
    xp[:, :, 1:-1, 1:-1] = x
    wi = np.asarray(w).astype(np.int64)
    out = np.zeros((B, w.shape[0], H, W), np.int64)
    for ky in range(3):
        for kx in range(3):
            out += np.einsum('bchw,oc->bohw', xp[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2], wi[:, :, ky, kx])
    return out


def s2_dgrad_direct(dy, w):
    """dx[b, ci, 2 oy + ky - 1, 2 ox + kx - 1] += dy[b, co, oy, ox] w[co, ci, ky, kx]; int64, [B, cin, 2H, 2W]."""
    B, cout, H, W = dy.shape
    wi, dyi = np.asarray(w).astype(np.int64), np.asarray(dy).astype(np.int64)
    full = np.zeros((B, w.shape[1], 2 * H + 2, 2 * W + 2), np.int64)
    for ky in range(3):
        for kx in range(3):
            full[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2] += np.einsum('bohw,oc->bchw', dyi, wi[:, :, ky, kx])
    return full[:, :, 1:-1, 1:-1]


# ------------------------------------------------------------------------------------------ stride-2 conv: the route
def _parity_plane(x, p, q, bug=None):
    """k_lc_tile_gather with sy = sx = 2 and origin (p, q): plane position (y, x) is source element (2 y + p, 2 x + q)."""
    if bug == 'parity_swapped':
        p, q = q, p
    plane = x[:, :, p::2, q::2]
    if bug == 'odd_plane_origin' and p == 1:  # the odd plane read one row late
        late = np.zeros_like(plane)
        late[:, :, :-1] = plane[:, :, 1:]
        plane = late
    return plane


def _tiles(plane, tw, bug=None):
    t = cut_tiles(plane, tw)
    if bug == 'edge_repeats':  # row -1 reads row 0: the halo row above the plane repeats the plane's first row
        B, _, H, W = plane.shape
        v = t.reshape(B, H // TILE, W // tw, plane.shape[1], TILE + 2, tw + 2)
        v[:, 0, :, :, 0, :] = v[:, 0, :, :, 1, :]
    return t


def s2_route(x, w, wide=True, bug=None):
    """The forward conv as AtariRun::s2_fwd runs it: per parity plane gather -> tiles with halo, a stride-1 conv of the tiles on the plane's taps,
    accumulated on the tiles, whose inner positions are scattered into the plane.  int64."""
    B, cin, H2, W2 = x.shape
    H, W = H2 // 2, W2 // 2
    tw = tile_w(W, wide)
    acc = None
    for pq in range(4):
        p, q = pq >> 1, pq & 1
        t = _tiles(_parity_plane(np.asarray(x), p, q, bug), tw, bug)
        y = cc.conv_acc(t, _plane_weight(w, p, q, False), np.int64)
        acc = y if acc is None or (bug == 'plane_overwrites' and pq == 2) else acc + y
    return put_tiles(acc[:, :, 1:-1, 1:-1], B, H, W, tw)


def s2_dgrad_route(dy, w, wide=True, bug=None):
    """The data gradient as AtariRun::s2_dgrad runs it: the dy tiles with halo, per parity (p, q) of dx a stride-1 conv on the transposed copy's taps
    (par_row_d) and a scatter into that parity of the 2H x 2W plane.  int64; -2^40 marks what no parity wrote."""
    B, cout, H, W = dy.shape
    tw = tile_w(W, wide)
    t = cut_tiles(np.asarray(dy), tw)
    dx = np.full((B, w.shape[1], 2 * H, 2 * W), -(1 << 40), np.int64)
    for pq in range(4):
        p, q = pq >> 1, pq & 1
        y = cc.conv_acc(t, _plane_weight(w, p, q, True, forward_taps=bug == 'dgrad_forward_taps'), np.int64)
        if bug == 'parity_swapped':
            p, q = q, p
        dx[:, :, p::2, q::2] = put_tiles(y[:, :, 1:-1, 1:-1], B, H, W, tw)
    return dx


def s2_case(cls, shape, dgrad=False):
    """(plane, [layer weights [cout, cin, 3, 3]]) of class `cls`: the forward conv's x [B, cin, 2H, 2W] or the data gradient's dy [B, cout, H, W].
    locator: one-hot weights, one tap per output channel of the conv that runs (all nine taps covered) and coded input; small: dense {-2 .. 2}."""
    cin, cout, H, W, B = shape
    k_in, k_out = (cout, cin) if dgrad else (cin, cout)
    h, wd = (H, W) if dgrad else (2 * H, 2 * W)
    if cls == 'locator':
        ws = [locator_weights(k_in, k_out, d) for d in range(2)]
        return locator_x(B, k_in, h, wd), [np.ascontiguousarray(np.transpose(v, (1, 0, 2, 3))) if dgrad else v for v in ws]
    rs = np.random.RandomState(_seed('s2', cls, shape, dgrad))
    return rs.randint(-2, 3, (B, k_in, h, wd)).astype(np.float32), [rs.randint(-2, 3, (cout, cin, 3, 3)).astype(np.float32)]


def s2_bound(x, w, dgrad=False):
    """max over outputs of sum |x| |w|: under 2^24, every partial sum of every summation order is an exact float32."""
    return int((s2_dgrad_direct if dgrad else s2_direct)(np.abs(x), np.abs(w)).max())


# ------------------------------------------------------------------------------------------ pools, ReLU backward
def pool_fwd_ref(x, bug=None):
    """AvgPool2d(3, 2, 1), count_include_pad: int64 window sums, then float32(sum) / float32(9)."""
    B, C, ih, iw = x.shape
    oh, ow = ih // 2, iw // 2
    xp = np.zeros((B, C, ih + 2, iw + 2), np.int64)
    xp[:, :, 1:-1, 1:-1] = x
    inb = np.zeros((ih + 2, iw + 2), np.int64)
    inb[1:-1, 1:-1] = 1
    s, n = np.zeros((B, C, oh, ow), np.int64), np.zeros((oh, ow), np.int64)
    for ky in range(3):
        for kx in range(3):
            s += xp[:, :, ky:ky + 2 * oh:2, kx:kx + 2 * ow:2]
            n += inb[ky:ky + 2 * oh:2, kx:kx + 2 * ow:2]
    div = n.astype(np.float32) if bug == 'pool_valid_count' else np.float32(9)
    return s.astype(np.float32) / div


def pool_bwd_ref(g, bug=None):
    """Its backward: every input pixel collects 1 / 9 of the outputs whose window covers it.  g [B, C, oh, ow] -> [B, C, 2 oh, 2 ow]."""
    B, C, oh, ow = g.shape
    full = np.zeros((B, C, 2 * oh + 2, 2 * ow + 2), np.int64)
    taps = range(1, 3) if bug == 'pool_bwd_window' else range(3)  # the mistake: a 2 x 2 window
    for ky in taps:
        for kx in taps:
            full[:, :, ky:ky + 2 * oh:2, kx:kx + 2 * ow:2] += np.asarray(g).astype(np.int64)
    return full[:, :, 1:-1, 1:-1].astype(np.float32) / np.float32(9)


def pool_case(hw, B=3, C=5):
    ih, iw = hw
    rs = np.random.RandomState(_seed('pool', hw))
    return rs.randint(-50, 51, (B, C, ih, iw)).astype(np.float32), rs.randint(-50, 51, (B, C, ih // 2, iw // 2)).astype(np.float32)


def relu_case():
    """g, x of n = 1000 elements ([1, 5, 10, 20]): x holds +0.0, -0.0 and the smallest positive subnormal among ordinary values."""
    rs = np.random.RandomState(_seed('relu'))
    g = rs.randn(1, 5, 10, 20).astype(np.float32)
    x = rs.randn(1, 5, 10, 20).astype(np.float32)
    special = np.array([0.0, -0.0, 1e-45, -1e-45, np.finfo(np.float32).tiny], np.float32)
    x.reshape(-1)[::7] = special[np.arange(len(x.reshape(-1)[::7])) % len(special)]
    return g, x


def relu_bwd_ref(g, x):
    return np.where(x > 0, g, np.float32(0)).astype(np.float32)


# ------------------------------------------------------------------------------------------ entry, normalize
def entry_ref(x, gs, scale, extra, partner, bug=None, d_rule='f32'):
    """k_lc_entry in float64 (the formula of its header comment): with G = scale gs, s = (x - mn) / d,
        dx_c = G_c / d - [c == imin] sum_k G_k / d - ([c == imax] - [c == imin]) sum_k G_k s_k / d,
    the arg-min / arg-max at the LOWEST attaining channel, d = float32(float32(mx - mn) + float32(1e-8)); + extra; masked by x > 0 (strict).
    x [B, C, ...]; returns dict(dz, d, G, s, sum1 [B, C], sum2 [B, C]: the per-image sums of dz and dz * partner)."""
    x64 = np.asarray(x, np.float64)
    B, C = x.shape[:2]
    t = np.zeros(x64.shape)
    out = {}
    if gs is not None:
        G = np.asarray(gs, np.float64) * (1.0 if bug == 'scale_dropped' else scale)
        x32 = np.asarray(x, np.float32)
        mn, mx = x32.min(1, keepdims=True), x32.max(1, keepdims=True)
        if d_rule == 'f32':
            d = ((mx - mn).astype(np.float32) + np.float32(1e-8)).astype(np.float32).astype(np.float64)
        else:
            d = mx.astype(np.float64) - mn + 1e-8
        ch = np.arange(C).reshape((1, C) + (1,) * (x.ndim - 2))
        first = lambda hit: np.where(hit, ch, C).min(1, keepdims=True)  # noqa: E731
        last = lambda hit: np.where(hit, ch, -1).max(1, keepdims=True)  # noqa: E731
        imn, imx = (last if bug == 'argmin_last' else first)(x32 == mn), first(x32 == mx)
        s = (x64 - mn) / d
        sg, sgs = G.sum(1, keepdims=True), (G * s).sum(1, keepdims=True)
        a, b = (imx, imn) if bug == 'minmax_terms_swapped' else (imn, imx)
        t = G / d + np.where(ch == a, -sg / d + sgs / d, 0.0) + np.where(ch == b, -sgs / d, 0.0)
        out.update(d=d, G=G, s=s)
    if extra is not None:
        t = t + np.asarray(extra, np.float64)
    dz = np.where((x64 >= 0) if bug == 'mask_ge' else (x64 > 0), t, 0.0)
    flat = dz.reshape(B, C, -1)
    out.update(dz=dz, sum1=flat.sum(2), sum2=(flat * np.asarray(partner, np.float64).reshape(B, C, -1)).sum(2))
    return out


def entry_bound(ref, extra):
    """The derived bound per element of dz for the inexact classes (flat, float):
        (C + 8) 2^-24 (|G_c| + sum_k |G_k| + 2 sum_k |G_k s_k|) / d + |extra_c| 2^-23
    -- one rounding per addition of the channel sums plus the divisions and subtractions."""
    G, s, d = ref['G'], ref['s'], ref['d']
    C = G.shape[1]
    b = (C + 8) * 2.0 ** -24 * (np.abs(G) + np.abs(G).sum(1, keepdims=True) + 2 * np.abs(G * s).sum(1, keepdims=True)) / d
    return b + (0 if extra is None else np.abs(np.asarray(extra, np.float64)) * 2.0 ** -23)


def normalize_ref(x):
    """k_lc_normalize as a float32 expression: (x - mn) / ((mx - mn) + 1e-8f), every operation rounded once (IEEE division, no contraction)."""
    x = np.asarray(x, np.float32)
    mn, mx = x.min(1, keepdims=True), x.max(1, keepdims=True)
    d = ((mx - mn).astype(np.float32) + np.float32(1e-8)).astype(np.float32)
    return ((x - mn).astype(np.float32) / d).astype(np.float32)


def channel_groups(C):
    """(channels per thread, channel groups in use) of the entry / normalize / scatter kernels: thread group g holds channels g cpt .. g cpt + cpt - 1."""
    cpt = -(-C // 8)
    return cpt, -(-C // cpt)


def _pow2_x(rs, B, C, n, interior_only):
    """Integer x [B, C, n] with attained minimum m and attained maximum m + R per pixel; m >= 1 at (well over) half of the pixels, m = 0 with several
    zero channels at the rest.  interior_only: every other channel strictly between (R in {2, 4, 8}), so only the forced channels attain."""
    m = np.where(rs.rand(B, 1, n) < 0.65, rs.randint(1, 4, (B, 1, n)), 0)
    R = rs.choice([2, 4, 8] if interior_only else [1, 2, 4, 8], (B, 1, n))
    if interior_only:
        x = m + 1 + rs.randint(0, 1 << 30, (B, C, n)) % (R - 1)
    else:
        x = m + rs.randint(0, 1 << 30, (B, C, n)) % (R + 1)
        x = np.where((m == 0) & (rs.rand(B, C, n) < 0.3), 0, x)  # several zero channels where the minimum is 0
    return x, m, R


def _put(x, ch, val):
    np.put_along_axis(x, ch, val, axis=1)


def entry_case(cls, B, C, n, key=0):
    """dict(x, gs, extra, partner) [B, C, n] float32 of class `cls` (see the module's tests for what each class is for)."""
    rs = np.random.RandomState(_seed('entry', cls, B, C, n, key))
    ints = lambda lo, hi: rs.randint(lo, hi + 1, (B, C, n)).astype(np.float32)  # noqa: E731
    out = dict(gs=ints(-2, 2), extra=ints(-3, 3), partner=ints(-3, 3))
    if cls == 'pow2':
        x, m, R = _pow2_x(rs, B, C, n, False)
        a = rs.randint(0, C, (B, 1, n))
        b = (a + 1 + rs.randint(0, C - 1, (B, 1, n))) % C
        _put(x, a, m)
        _put(x, b, m + R)
    elif cls == 'ties':
        x, m, R = _pow2_x(rs, B, C, n, True)
        cpt, ng = channel_groups(C)
        last0 = (ng - 1) * cpt
        pix = np.arange(n).reshape(1, 1, n) + np.zeros((B, 1, 1), np.int64)
        q = pix // 3
        first_of = lambda g: (g % ng) * cpt  # noqa: E731
        # pattern 1 (and the fallback): each extreme attained in two different channel groups
        sets = {1: ([first_of(q), first_of(q + 2)], [first_of(q + 1), first_of(q + 3)])}
        # pattern 0: inside one thread's channel run (needs two channels per thread: the groups before the last always hold cpt)
        if cpt >= 2:
            sets[0] = ([first_of(q % (ng - 1)), first_of(q % (ng - 1)) + 1], [first_of((q + 1) % (ng - 1)), first_of((q + 1) % (ng - 1)) + 1])
        else:
            sets[0] = sets[1]
        # pattern 2: every attaining channel of one extreme in the LAST group (q even: the minimum, q odd: the maximum), the other in groups 0 and 2
        in_last = [last0 + 0 * q, np.minimum(last0 + 1, C - 1) + 0 * q]
        other = [first_of(0 * q), first_of(0 * q + 2)]
        sets[2] = ([np.where(q % 2 == 0, u, v) for u, v in zip(in_last, other)], [np.where(q % 2 == 0, v, u) for u, v in zip(in_last, other)])
        for pat, (mins, maxs) in sets.items():
            sel = pix % 3 == pat
            for chs, val in ((mins, m), (maxs, m + R)):
                for ch in chs:
                    cur = np.take_along_axis(x, ch, axis=1)
                    _put(x, ch, np.where(sel, val, cur))
    elif cls == 'flat':
        v = np.where(rs.rand(B, 1, n) < 0.5, 0.0, rs.randint(1, 4, (B, 1, n)) + np.round(rs.rand(B, 1, n), 2))
        x = v + np.zeros((B, C, n))
    elif cls == 'float':
        x = np.maximum(rs.randn(B, C, n) + 0.5, 0.0)
        out = dict(gs=rs.randn(B, C, n).astype(np.float32), extra=rs.randn(B, C, n).astype(np.float32), partner=rs.randn(B, C, n).astype(np.float32))
    else:
        raise ValueError(cls)
    out['x'] = x.astype(np.float32)
    return out


def entry_exactness(case, scale, use_extra):
    """(d exact, dz dyadic, bound) for an exact class.  With integer x, gs, extra and partner, scale 1/2 | 1 and d = R in {1, 2, 4, 8}: G has step
    1/2, s step 1/8, G s and G / d step 1/16, sum G s / d step 1/128 -- every quantity the kernel forms is a multiple of U^-1 = 2^-7.  `bound` is the
    largest sum of absolute values, in units of U^-1, over the channel sums with the terms of dz behind them and over the per-image statistics: under
    2^24, every partial sum in any order is an exact float32."""
    U = 2.0 ** 7
    x = case['x'].astype(np.float64)
    mn, mx = x.min(1, keepdims=True), x.max(1, keepdims=True)
    d32 = ((mx - mn).astype(np.float32) + np.float32(1e-8)).astype(np.float32)
    d_exact = bool(np.all(mx - mn >= 1) and np.all(d32 == mx - mn))
    extra = case['extra'] if use_extra else None
    ref = entry_ref(case['x'], case['gs'], scale, extra, case['partner'])
    G, s, d, dz = ref['G'], ref['s'], ref['d'], ref['dz']
    dyadic = bool(np.all(dz * U == np.rint(dz * U)) and np.all(G * s / d * U == np.rint(G * s / d * U)))
    terms = (np.abs(G).sum(1, keepdims=True) + np.abs(G * s).sum(1, keepdims=True) + np.abs(G)) / d + (0 if extra is None else np.abs(extra))
    B, C = x.shape[:2]
    stat = (np.abs(dz) * np.maximum(np.abs(case['partner'].astype(np.float64)), 1.0)).reshape(B, C, -1).sum(2)
    return d_exact, dyadic, max(float(terms.max()), float(stat.max())) * U


# ------------------------------------------------------------------------------------------ gather, scatter
def gather_ref(src0, src1, coef, mode, stride, origin, inner_only, tw, bug=None):
    """k_lc_tile_gather: plane position (y, x) is source element (stride y + py, stride x + px); the staging transform (ident | bnrelu: relu(a v + b) |
    bnbwd: c1 v + c2 y + c3) is applied inside the plane, what lies outside is zero; inner_only zeroes every tile's halo ring.  float32 (the
    coefficients and data are integers: every fma is exact)."""
    py, px = origin
    plane = np.asarray(src0, np.float64)[:, :, py::stride, px::stride]
    C = plane.shape[1]
    if mode != 'ident':
        k = np.asarray(coef, np.float64).reshape(3, 1, C, 1, 1)
    if mode == 'bnrelu':
        plane = np.maximum(k[0] * plane + k[1], 0.0)
    elif mode == 'bnbwd':
        y = np.asarray(src1, np.float64)[:, :, py::stride, px::stride]
        c1, c2 = (k[1], k[0]) if bug == 'bnbwd_coef_order' else (k[0], k[1])
        plane = c1 * plane + c2 * y + k[2]
    t = cut_tiles(plane, tw)
    if inner_only and bug != 'inner_only_ignored':
        t[:, :, 0, :] = 0
        t[:, :, -1, :] = 0
        t[:, :, :, 0] = 0
        t[:, :, :, -1] = 0
    return t.astype(np.float32)


def gather_case(B, C, H, W, stride, key=0):
    """Integer sources [B, C, stride H, stride W] (never zero, so a zeroed ring or an outside position shows) and integer coefficients [3, C]."""
    rs = np.random.RandomState(_seed('gather', B, C, H, W, stride, key))
    shape = (B, C, stride * H, stride * W)
    src0 = (rs.randint(1, 40, shape) * rs.choice([-1, 1], shape)).astype(np.float32)
    src1 = (rs.randint(1, 40, shape) * rs.choice([-1, 1], shape)).astype(np.float32)
    coef = np.stack([rs.choice([-2, -1, 1, 2, 3], C), rs.choice([-3, -1, 2, 4, 5], C), rs.randint(1, 8, C)]).astype(np.float32)
    return src0, src1, coef


def scatter_ref(tiles, B, H, W, tw, stride, origin, skip, src_inner):
    """k_lc_tile_scatter: the inner positions of every tile -> the plane (one parity of a stride H x stride W plane, NaN elsewhere), + skip.
    Returns (dst float32, the written values [B, C, H, W] float64)."""
    inner = tiles if src_inner else tiles[:, :, 1:-1, 1:-1]
    v = put_tiles(np.asarray(inner, np.float64), B, H, W, tw)
    py, px = origin
    if skip is not None:
        v = v + np.asarray(skip, np.float64)[:, :, py::stride, px::stride]
    dst = np.full((B, tiles.shape[1], stride * H, stride * W), np.nan, np.float32)
    dst[:, :, py::stride, px::stride] = v
    return dst, v


def scatter_stats(v, bug=None):
    """The pivoted forward statistics per (image, chunk of 32 plane positions, channel): (pivot = the chunk's first value, sum (v - pivot),
    sum (v - pivot)^2, positions in the chunk).  [B * chunks, C, 4] float64."""
    B, C, H, W = v.shape
    flat = v.reshape(B, C, H * W)
    nch = -(-H * W // 32)
    out = np.zeros((B, nch, C, 4))
    for k in range(nch):
        ck = flat[:, :, 32 * k:32 * k + 32]
        pvt = ck[:, :, :1]
        u = ck if bug == 'pivot_zero' else ck - pvt  # the mistake: summed without the pivot but reported with it
        out[:, k, :, 0], out[:, k, :, 1], out[:, k, :, 2], out[:, k, :, 3] = pvt[:, :, 0], u.sum(2), (u * u).sum(2), ck.shape[2]
    return out.reshape(B * nch, C, 4)


def scatter_case(B, C, H, W, tw, src_inner, stride, key=0):
    """Integer tiles (the halo holds values too: a wrong offset into a whole tile shows) and an integer skip plane."""
    rs = np.random.RandomState(_seed('scatter', B, C, H, W, tw, src_inner, stride, key))
    n = B * (H // TILE) * (W // tw)
    tiles = rs.randint(-20, 21, (n, C) + ((TILE, tw) if src_inner else (TILE + 2, tw + 2))).astype(np.float32)
    skip = rs.randint(-30, 31, (B, C, stride * H, stride * W)).astype(np.float32)
    return tiles, skip


assert sa.TILE == 12
