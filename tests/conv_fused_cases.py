"""One conv of the learner's BatchNorm towers as the update runs it -- staging transform, write-through, epilogue, statistics partials, the
finalize kernels, k_lc_apply -- on the CPU: the references and the data of tests/test_conv_fused_host.py and tests/test_gpu_conv_fused.py.
numpy only; builds on tests/conv_layer_cases.py.

Layouts are the kernels' (muzero_amd/csrc/mz_learn_conv.h): activations [B, C, h, w]; coef [3, C] = (a, b, -) | (c1, c2, c3); forward partials
[groups, cpad, 4] = (p, sum (y - p), sum (y - p)^2, n) per image group of G images, p = the group's first image's output at pixel 0; backward
partials [groups, cpad, 2] = (sum t, sum t * partner).  `bug=` re-introduces ONE deliberate mistake (MUTATIONS) into a reference."""
import numpy as np

import conv_layer_cases as cc

MUTATIONS = ('pad_slot_counted', 'short_group_full', 'n_full_for_short', 'pivot_wrong_image', 'relu_dropped_mat', 'residual_dropped', 'c3_dropped',
             'in1_as_in0', 'skip_after_mask', 'mask_ge', 'mcoef_ignored', 'partner_from_mask', 'biased_running_var', 'accumulate_ignored',
             'group_past_unroll_dropped', 'slice_order')
EPS = 1e-5
MOMENTUM = 0.1


def pad16(c):
    return (c + 15) // 16 * 16


def _col(v):
    return np.asarray(v, np.float64).reshape(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------ geometry (make_geom's conv tiling)
def conv_geom(h, w, B, wg_per_group=2, cus=256):
    """(NPT, G) as make_geom picks them for B images: the shortest launch, ties to the denser packing."""
    hw, qp = h * w, (h * w + 3) // 4
    best = None
    for cand in (5, 6, 9, 13, 15):
        G = min(16 * cand // hw, 64 // qp)
        if G < 1:
            continue
        eff, cost = G * hw / (16.0 * cand), -(-(-(-B // G) * wg_per_group) // cus) * cand
        if best is None or cost < best[0] or (cost == best[0] and eff > best[1] + 1e-9):
            best = (cost, eff, cand, G)
    return best[2], best[3]


# ------------------------------------------------------------------------------------------ the conv and what surrounds it
def stage(mode, in0, in1=None, coef=None, bug=None, pre=False):
    """The staged operand in float64 (exact on the integer classes).  pre=True: before the ReLU."""
    x = np.asarray(in0, np.float64)
    if mode == 'ident':
        return x
    c = [_col(coef[k]) for k in range(3)]
    if mode == 'bnbwd':
        y = x if bug == 'in1_as_in0' else np.asarray(in1, np.float64)
        return c[0] * x + c[1] * y + (0.0 if bug == 'c3_dropped' else c[2])
    t = c[0] * x + c[1]
    if mode == 'bnres' and bug != 'residual_dropped':
        t = t + np.asarray(in1, np.float64)
    return t if pre else np.maximum(t, 0.0)


def mat_out(mode, in0, in1, coef, bug=None):
    """What the write-through leaves: the staged operand itself."""
    return stage(mode, in0, in1, coef, bug=None if bug == 'relu_dropped_mat' else bug, pre=bug == 'relu_dropped_mat')


def dgrad_weight(w):
    """The layer's weight [cout, cin, 3, 3] <-> the data gradient's: channels swapped, taps flipped (its own inverse)."""
    return np.ascontiguousarray(np.asarray(w).transpose(1, 0, 2, 3)[:, :, ::-1, ::-1])


def epilogue(y, skip=None, mask=None, mcoef=None, bug=None):
    """The data-gradient epilogue: + skip, THEN zero where not (ma * mask + mb > 0) (mcoef None: mask > 0)."""
    t = np.asarray(y, np.float64)
    if skip is not None and bug != 'skip_after_mask':
        t = t + skip
    if mask is not None:
        v = np.asarray(mask, np.float64)
        if mcoef is not None and bug != 'mcoef_ignored':
            v = _col(mcoef[0]) * v + _col(mcoef[1])
        t = np.where(v >= 0 if bug == 'mask_ge' else v > 0, t, 0.0)
    if skip is not None and bug == 'skip_after_mask':
        t = t + skip
    return t


def partials_fwd(y, G, npt=None, bug=None):
    """[groups, cpad, 4] float64 from the conv output y [B, C, h, w]."""
    y = np.asarray(y, np.float64)
    B, C, h, w = y.shape
    hw, groups = h * w, -(-B // G)
    out = np.zeros((groups, pad16(C), 4))
    for g in range(groups):
        img = y[g * G:(g + 1) * G].reshape(-1, C, hw)
        n = img.shape[0]
        p = (img[1] if bug == 'pivot_wrong_image' and n > 1 else img[0])[:, 0]
        u = img - p.reshape(1, C, 1)
        s1, s2 = u.sum(axis=(0, 2)), (u * u).sum(axis=(0, 2))
        extra = 0  # slots that hold no output (an accumulator of zeros) and are counted by mistake: each adds (0 - p), (0 - p)^2
        if bug == 'pad_slot_counted':
            extra += npt * 16 - G * hw
        if bug == 'short_group_full':
            extra += (G - n) * hw
        out[g, :C, 0], out[g, :C, 1], out[g, :C, 2] = p, s1 - extra * p, s2 + extra * p * p
        out[g, :C, 3] = (G if bug == 'n_full_for_short' else n) * hw
    return out


def partials_bwd(t, partner, G, mask=None, bug=None):
    """[groups, cpad, 2] float64: (sum t, sum t * partner) per image group."""
    t = np.asarray(t, np.float64)
    pv = np.asarray(mask if bug == 'partner_from_mask' and mask is not None else partner, np.float64)
    B, C = t.shape[:2]
    groups = -(-B // G)
    out = np.zeros((groups, pad16(C), 2))
    for g in range(groups):
        sl = slice(g * G, (g + 1) * G)
        out[g, :C, 0], out[g, :C, 1] = t[sl].sum(axis=(0, 2, 3)), (t[sl] * pv[sl]).sum(axis=(0, 2, 3))
    return out


# ------------------------------------------------------------------------------------------ the finalize kernels
def slice_sums(cols, unroll, bug=None):
    """sum over the groups of cols [groups, ...] in the kernels' order: slice j adds groups j, j + 16, .. one after the other (the unrolled loop takes
    `unroll` of them at a time, a tail loop the rest), then the 16 slices are added in slice order.  All float64."""
    cols = np.asarray(cols, np.float64)
    if bug == 'slice_order':
        return np.cumsum(cols, axis=0)[-1]
    tot = np.zeros(cols.shape[1:])
    for s in range(16):
        mine = cols[s::16]
        if bug == 'group_past_unroll_dropped':
            mine = mine[:len(mine) // unroll * unroll]
        tot = tot + (np.cumsum(mine, axis=0)[-1] if len(mine) else 0.0)
    return tot


def bn_fwd(part, gamma, beta, count, running_mean=None, running_var=None, bug=None):
    """k_lc_bn_fwd in float64 from its inputs as given (the GPU tests pass float32 arrays): dict(mean, var, invstd, a, b, running_mean, running_var), [C] each."""
    C = len(gamma)
    P = np.asarray(part).astype(np.float64)[:, :C]
    p, s1, s2, n = (P[:, :, k] for k in range(4))
    T0, T1, T2, U1, U2, V = (slice_sums(c, 4, bug) for c in (n, s1, s2, n * p, n * p * p, p * s1))
    mean_p = np.where(T0 > 0, (U1 + T1) / np.where(T0 > 0, T0, 1.0), 0.0)
    nvar = T2 + 2.0 * V - 2.0 * mean_p * T1 + U2 - 2.0 * mean_p * U1 + mean_p * mean_p * T0
    count = float(count)
    mean, var = (U1 + T1) / count, np.maximum(nvar / count, 0.0)
    invstd = 1.0 / np.sqrt(var + EPS)
    out = dict(mean=mean, var=var, invstd=invstd, a=np.asarray(gamma).astype(np.float64) * invstd, n=T0)
    out['b'] = np.asarray(beta).astype(np.float64) - mean * out['a']
    if running_mean is not None:
        unb = var if bug == 'biased_running_var' or count <= 1 else var * count / (count - 1.0)
        out['running_mean'] = (1 - MOMENTUM) * np.asarray(running_mean).astype(np.float64) + MOMENTUM * mean
        out['running_var'] = (1 - MOMENTUM) * np.asarray(running_var).astype(np.float64) + MOMENTUM * unb
    return out


def bn_bwd(part, gamma, save, count, dgamma0=None, dbeta0=None, accumulate=False, bug=None):
    """k_lc_bn_bwd in float64 from its inputs as given (save = (mean, invstd) [2, C]): dict(c1, c2, c3, dgam, s1, dgamma, dbeta, cancel)."""
    C = len(gamma)
    P = np.asarray(part).astype(np.float64)[:, :C]
    s1, s2 = slice_sums(P[:, :, 0], 8, bug), slice_sums(P[:, :, 1], 8, bug)
    mean, invstd = (np.asarray(save).astype(np.float64)[k, :C] for k in range(2))
    gam, M = np.asarray(gamma).astype(np.float64), float(count)
    dgam = (s2 - mean * s1) * invstd
    c1 = gam * invstd
    out = dict(c1=c1, c2=-c1 * invstd * dgam / M, c3=-c1 * s1 / M + c1 * mean * invstd * dgam / M, dgam=dgam, s1=s1,
               cancel=np.abs(s2 - mean * s1) / np.maximum(np.maximum(np.abs(s2), np.abs(mean * s1)), 1e-300))
    acc = accumulate and bug != 'accumulate_ignored'
    out['dgamma'] = dgam + (np.asarray(dgamma0, np.float64) if acc else 0.0)
    out['dbeta'] = s1 + (np.asarray(dbeta0, np.float64) if acc else 0.0)
    return out


def apply32(y, res, coef):
    """k_lc_apply in float32: relu(fmaf(a, y, b) + res) -- the fused multiply-add as ONE rounding of the float64 a y + b (tests/forced_masks.py), then a
    float32 add."""
    y = np.asarray(y, np.float32)
    t = (_col(np.asarray(coef[0], np.float32)) * y.astype(np.float64) + _col(np.asarray(coef[1], np.float32))).astype(np.float32)
    if res is not None:
        t = t + np.asarray(res, np.float32)
    return np.maximum(t, np.float32(0))


def ulp(v):
    """An upper bound of one float32 ulp of |v|: 2^-23 |v| (and the smallest normal's below it)."""
    return np.maximum(np.abs(np.asarray(v, np.float64)) * 2.0 ** -23, 2.0 ** -149)


# ------------------------------------------------------------------------------------------ float32 models of the variance (the ill-conditioned case)
def var_pivot32(y, G):
    """The variance per channel as the conv kernel's float32 partials + the float64 finalize make it (one float32 running sum per group)."""
    y = np.asarray(y, np.float32)
    B, C, h, w = y.shape
    groups = -(-B // G)
    part = np.zeros((groups, pad16(C), 4), np.float32)
    for g in range(groups):
        img = np.ascontiguousarray(y[g * G:(g + 1) * G].transpose(1, 0, 2, 3)).reshape(C, -1)
        p = img[:, 0].copy()
        u = img - p[:, None]
        part[g, :C, 0], part[g, :C, 3] = p, img.shape[1]
        part[g, :C, 1] = np.cumsum(u, axis=1, dtype=np.float32)[:, -1]
        part[g, :C, 2] = np.cumsum(u * u, axis=1, dtype=np.float32)[:, -1]
    return bn_fwd(part, np.ones(C, np.float32), np.zeros(C, np.float32), B * h * w)['var']


def var_naive32(y, G):
    """E[y^2] - mean^2 from float32 partial sums (sum y, sum y^2) per group, finalized in float64: what the pivot replaces."""
    y = np.asarray(y, np.float32)
    B, C, h, w = y.shape
    s1, s2 = np.zeros(C), np.zeros(C)
    for g in range(-(-B // G)):
        img = np.ascontiguousarray(y[g * G:(g + 1) * G].transpose(1, 0, 2, 3)).reshape(C, -1)
        s1 += np.cumsum(img, axis=1, dtype=np.float32)[:, -1].astype(np.float64)
        s2 += np.cumsum(img * img, axis=1, dtype=np.float32)[:, -1].astype(np.float64)
    n = B * h * w
    return s2 / n - (s1 / n) ** 2


def ill_conditioned(seed, B, cin, cout, h, w, ratio=1e6):
    """(x, w) whose conv output has mean^2 / var of about `ratio` in every channel: inputs 1 + noise, weights on the centre tap only (the zero
    padding would otherwise put a step of the mean's size at the border)."""
    rs = np.random.RandomState(seed)
    x = (1.0 + rs.uniform(-1, 1, (B, cin, h, w)) * np.sqrt(3.0 * cin / ratio)).astype(np.float32)
    wt = np.zeros((cout, cin, 3, 3), np.float32)
    wt[:, :, 1, 1] = rs.uniform(0.75, 1.0, (cout, cin)) / cin
    return x, wt


def finalize_parts(seed, groups, C, kind, n=72):
    """Host-made partials [groups, pad16(C), 4 | 2] float32 for the finalize kernels alone.  fwd: pivots ~ N(0, 1), sums of a group of n values of
    unit variance around them.  bwd: integer sums of dz (dbeta is then exact), float sums of dz y."""
    rs = np.random.RandomState(seed)
    part = np.zeros((groups, pad16(C), 4 if kind == 'fwd' else 2), np.float32)
    if kind == 'fwd':
        s1 = rs.randn(groups, C) * np.sqrt(n)
        part[:, :C, 0], part[:, :C, 1], part[:, :C, 2], part[:, :C, 3] = rs.randn(groups, C), s1, n * rs.uniform(0.5, 1.5, (groups, C)) + s1 * s1 / n, n
    else:
        part[:, :C, 0], part[:, :C, 1] = rs.randint(-500, 501, (groups, C)), rs.randn(groups, C) * 100.0
    return part


FINALIZE_GROUPS = (1, 16, 17, 48, 49, 112, 113, 130, 3001)
FINALIZE_C = 20  # not a multiple of 16: cpad 32, twelve padding channels


def finalize_operands(seed, C):
    rs = np.random.RandomState(seed)
    f = lambda a: a.astype(np.float32)  # noqa: E731
    return dict(gamma=f(rs.uniform(0.5, 1.5, C)), beta=f(rs.randn(C)), running_mean=f(rs.randn(C)), running_var=f(rs.uniform(0.5, 2.0, C)),
                save=f(np.stack([rs.randn(C), rs.uniform(0.5, 2.0, C)])), dgamma=f(rs.randn(C)), dbeta=f(rs.randint(-50, 51, C)))


# ------------------------------------------------------------------------------------------ integer data
COEF_POOL = np.array([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0])
S_MAX = 3  # class S: staged values in 0 .. 3 (data gradient: -3 .. 3), weights +-1 on three input channels: |y| <= 81


def s_draws(seed, cin, cout):
    """Class S weights: draw d has +-1 on EVERY tap of input channels 3 d .. 3 d + 2 of every output channel, zero elsewhere (at most 27 nonzero)."""
    rs = np.random.RandomState(seed)
    draws = []
    for d in range(-(-cin // 3)):
        w3 = np.zeros((cout, cin + 3, 3, 3), np.float32)
        w3[:, 3 * d:3 * d + 3] = rs.choice([-1.0, 1.0], (cout, 3, 3, 3))
        draws.append((np.ascontiguousarray(w3[:, :cin]), np.zeros(cout, np.float32)))
    return draws


def s_target(seed, B, C, h, w, G, signed):
    """Class S staged operand: integers in 0 .. 3 (signed: -3 .. 3), about a third zero.  In the first image of every group of G, among the positions
    the output at pixel 0 reads -- (0, 0), (0, 1), (1, 0), (1, 1) -- of each channel triple, exactly ONE value is odd (channel 3 d at (0, 0)): with +-1
    weights on the triple the output at pixel 0, the pivot, is odd -- never zero -- in every output channel."""
    rs = np.random.RandomState(seed)
    t = rs.randint(1, S_MAX + 1, (B, C, h, w)) * (rs.rand(B, C, h, w) > 1 / 3)
    if signed:
        t = t * rs.choice([-1, 1], t.shape)
    first = t[::G]
    for img in (first, t[1::G]) if G > 1 else (first,):  # even (0 or +-2) around the corner; the group's SECOND image keeps it so: its pixel 0 is even in
        img[:, :, :2, :2] = np.sign(img[:, :, :2, :2]) * 2 * (np.abs(img[:, :, :2, :2]) // 2)  # every channel and differs from the pivot
    first[:, ::3, 0, 0] = rs.choice([1, 3], first[:, ::3, 0, 0].shape)  # one odd value per triple
    return t.astype(np.float64)


def int_target(cls, seed, B, C, h, w, G, signed):
    """The staged operand of class `cls` (W, X, M of conv_layer_cases; S): what the transform must land on.  Unsigned: what a ReLU can leave."""
    if cls == 'S':
        return s_target(seed, B, C, h, w, G, signed)
    t = cc.int_input(cls, seed, B, C, h, w).astype(np.float64)
    if not signed:
        rs = np.random.RandomState(seed + 1)
        t = np.abs(t) * (rs.rand(*t.shape) > 1 / 3)
    return t


def raw_inputs(mode, target, seed):
    """dict(in0, in1, coef) of float32 arrays whose transform `mode` is EXACTLY `target` in float32 arithmetic: per-channel multipliers from
    +-{1/2, 1, 2}, integer offsets, integer residual / y; where the target of a ReLU mode is zero the pre-activation is a negative integer."""
    rs = np.random.RandomState(seed)
    B, C, h, w = target.shape
    if mode == 'ident':
        return dict(in0=target.astype(np.float32), in1=None, coef=None)
    a, b, c3 = rs.choice(COEF_POOL, C), rs.randint(-3, 4, C).astype(np.float64), rs.randint(-3, 4, C).astype(np.float64)
    other = rs.randint(-4, 5, target.shape).astype(np.float64)
    if mode == 'bnbwd':  # target = c1 dz + c2 y + c3
        c2 = rs.choice(COEF_POOL, C)
        in0 = (target - _col(c2) * other - _col(c3)) / _col(a)
        coef = np.stack([a, c2, c3])
    else:
        pre = np.where(target > 0, target, -rs.randint(1, 4, target.shape).astype(np.float64))
        in0 = (pre - _col(b) - (other if mode == 'bnres' else 0.0)) / _col(a)
        coef = np.stack([a, b, np.zeros(C)])
    d = dict(in0=in0.astype(np.float32), in1=other.astype(np.float32) if mode in ('bnres', 'bnbwd') else None, coef=coef.astype(np.float32))
    assert np.array_equal(d['in0'], in0) and np.array_equal(stage(mode, d['in0'], d['in1'], d['coef']), target), 'the transform does not land on the target'
    return d


def epilogue_data(seed, B, C, h, w):
    """dict(skip, mask, mcoef, partner): small integers.  The mask holds exact zeros and -- for every channel -- elements m0 with ma m0 + mb == 0."""
    rs = np.random.RandomState(seed)
    ma = rs.choice(COEF_POOL, C)
    m0 = rs.choice([-2, 2], C)                      # the value of the mask that the affine map sends to zero
    mcoef = np.stack([ma, -ma * m0]).astype(np.float32)
    mask = rs.randint(-2, 3, (B, C, h, w)).astype(np.float32)
    return dict(skip=rs.randint(-4, 5, (B, C, h, w)).astype(np.float32), mask=mask, mcoef=mcoef, partner=rs.randint(-3, 4, (B, C, h, w)).astype(np.float32))


# what tower_bwd builds (and skip alone): name -> (skip, mask, mcoef, partner: None | 'mask' | 'own', statistics)
DGRAD_COMBOS = {
    'second_conv': (False, True, True, 'mask', 'bwd'),   # a block's second conv: mask = relu(a y1 + b) never materialised, partner IS the mask buffer
    'first_conv': (True, True, False, 'own', 'bwd'),     # a block's first conv: + the skip gradient, the block input as the mask, y of the layer below
    'skip_alone': (True, False, False, None, None),      # the first block of a tower without a conv block
    'bare': (False, False, False, None, None),           # the conv block's own data gradient
}
# forward: name -> (in_mode, write-through)
FWD_COMBOS = {'ident': ('ident', False), 'bnrelu': ('bnrelu', False), 'bnrelu_mat': ('bnrelu', True), 'bnres': ('bnres', False), 'bnres_mat': ('bnres', True)}

# id: (h, w, batch, c_in, c_out of the conv that runs, no_side, what the case is there for: the build name's fields)
GEOMS = {
    'g3x3': (3, 3, 20, 5, 6, False, dict(NPT=5, SIDE=0, G=8, groups=3)),       # quads straddle images, G > 1, a short last group (4 of 8)
    'g3x3_c72': (3, 3, 20, 8, 72, False, dict(NPT=5, SIDE=0, G=8, groups=3, z=2)),  # a second blockIdx.z: the write-through comes from slice 0 only
    'g6x6': (6, 6, 5, 5, 6, False, dict(NPT=5, SIDE=0, G=2, groups=3)),        # hw % 4 == 0: every batch regular
    'g6x6_c24': (6, 6, 5, 40, 24, False, dict(NPT=5, SIDE=0, G=2, groups=3)),  # c_in off 16 and 32, c_out with a partial tile
    'g5x7': (5, 7, 5, 5, 6, False, dict(NPT=5, SIDE=0, G=2, groups=3)),        # not square, hw % 4 == 3
    'g7x7': (7, 7, 2, 5, 6, False, dict(NPT=5, SIDE=0, G=1, groups=2)),        # ragged last tile; one fast batch, then the slow path
    'g9x9': (9, 9, 2, 20, 6, False, dict(NPT=6, SIDE=0, G=1, groups=2)),       # c_in off 16
    'g13x13': (13, 13, 2, 5, 6, False, dict(NPT=13, SIDE=0, G=1, groups=2)),
    'g15_side': (15, 15, 2, 5, 6, False, dict(NPT=15, SIDE=15, G=1, groups=2)),  # fast and slow epilogue in one workgroup
    'g15_generic': (15, 15, 2, 5, 6, True, dict(NPT=15, SIDE=0, G=1, groups=2)),
}
FULL_CLASSES = ('S', 'W', 'X', 'M')
CLASSES_OF = {k: (('S', 'X') if '_c' in k else FULL_CLASSES) for k in GEOMS}


def case_seed(key, cls, what):
    return 1000 * sorted(GEOMS).index(key) + 100 * FULL_CLASSES.index(cls) + what


def draws_of(cls, seed, c_in, c_out):
    return s_draws(seed, c_in, c_out) if cls == 'S' else cc.int_draws(cls, seed, c_in, c_out)


def forward_case(key, cls, combo):
    """dict(target, raw inputs, draws, mat_preload) of one forward run."""
    h, w, B, ci, co, _, exp = GEOMS[key]
    mode, mat = FWD_COMBOS[combo]
    target = int_target(cls, case_seed(key, cls, 1), B, ci, h, w, exp['G'], signed=mode == 'ident' and cls != 'S')
    d = raw_inputs(mode, target, case_seed(key, cls, 2))
    d.update(mode=mode, target=target, draws=draws_of(cls, case_seed(key, cls, 3), ci, co),
             mat_preload=np.full(target.shape, -77.0, np.float32) if mat else None)
    return d


def dgrad_case(key, cls):
    """dict(target, raw inputs of IN_BNBWD, draws of the EFFECTIVE conv c_in -> c_out, epilogue data) of the data-gradient runs of a geometry."""
    h, w, B, ci, co, _, exp = GEOMS[key]
    target = int_target(cls, case_seed(key, cls, 4), B, ci, h, w, exp['G'], signed=True)
    d = raw_inputs('bnbwd', target, case_seed(key, cls, 5))
    d.update(mode='bnbwd', target=target, draws=draws_of(cls, case_seed(key, cls, 6), ci, co), epi=epilogue_data(case_seed(key, cls, 7), B, co, h, w))
    return d


def dgrad_reference(d, wt, combo, G, bug=None):
    """(output, partials or None) of one data-gradient run; wt: the effective weight [c_out, c_in, 3, 3]."""
    skip, mask, mcoef, partner, stat = DGRAD_COMBOS[combo]
    e = d['epi']
    staged = stage('bnbwd', d['in0'], d['in1'], d['coef'], bug=bug)
    y = cc.conv_acc(staged, wt, np.float64)
    t = epilogue(y, e['skip'] if skip else None, e['mask'] if mask else None, e['mcoef'] if mcoef else None, bug=bug)
    part = partials_bwd(t, e['mask'] if partner == 'mask' else e['partner'], G, mask=e['mask'] if mask else None, bug=bug) if stat else None
    return t, part


def first_difference(out, ref, names):
    """None, or where two arrays first differ, in the words of `names` (one per axis)."""
    out, ref = np.asarray(out), np.asarray(ref)
    bad = np.argwhere(~((out == ref) | (np.isnan(out) & np.isnan(ref))))
    if len(bad) == 0:
        return None
    i = tuple(bad[0])
    return f'{len(bad)} of {out.size} differ, first at ' + ', '.join(f'{n} {v}' for n, v in zip(names, i)) + f': {out[i]!r} != {ref[i]!r}'
