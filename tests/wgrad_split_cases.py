"""The split-bf16 weight gradient (k_lc_wgrad_bf16x3, muzero_amd/csrc/mz_learn_conv_split_wgrad.h) on the CPU: the split planes' geometry and the
update's chunking written down from learner_conv.hip (make_geom_wsplit, Sched::wgrad_ops / wgrad_ops_steps; a 256-CU device), a numpy model of the
kernel -- the pitch layout of a staging round, 32-position steps, three bf16 terms per operand, six products per step in the kernel's order,
float32 accumulators, float32 chunk reduction -- whose terms can be dropped on purpose, and the extra Locator positions this kernel needs.
numpy only: importable without a GPU."""
import functools

import numpy as np

import conv_layer_cases as cc
import wgrad_layer_cases as wc

CUS = 256
LDS_MAX = 160 * 1024
SG_CAP = 16  # the update's cap on images per staging round (MZLC_WGRAD_SG)
TERMS = tuple(cc.TERMS)  # hh, hm, mh, hl, lh, mm: (dy term, x term)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ geometry (make_geom_wsplit)
def planes(h, w, sg, rows):
    """(pitch, steps, dy plane stride, x plane stride, LDS bytes) of a round of `sg` images, side by side or (rows) stacked."""
    rows = rows and sg > 1
    p8 = 8 * cdiv(w + 1 if (rows or sg == 1) else sg * (w + 1), 8)
    ns = cdiv((sg * (h + 1) - 1 if rows else h) * p8, 32)
    spy, spx = 32 * ns + 8, 32 * ns + 2 * p8 + 24
    return p8, ns, spy, spx, 640 + 192 * (spy + spx)


def geom(h, w, B, cout, cin_real, sg=0, layout=0, cus=CUS):
    """dict(sg, layout, P, nsteps, lds) the split path picks for one layer's launch of B images (sg > 0: forced; layout 2: stacked), or None
    where nothing fits (the hook then refuses with 'SG override')."""
    QP = cdiv(h * w, 4)
    blocks = cdiv(cdiv(cout, 16), 2) * cdiv(cdiv(cin_real, 16), 2)
    best = None
    for s in range(sg or 1, (sg or SG_CAP) + 1):
        if s * QP > 64:
            break
        p8, ns, _, _, lds = planes(h, w, s, layout == 2)
        if lds > LDS_MAX:
            continue
        chunks = min(max(cus // blocks, 1), B)
        ipw = cdiv(cdiv(B, chunks), s) * s
        cost = cdiv(cdiv(B, ipw) * blocks * 2, cus) * (ipw // s) * ns  # (one workgroup per CU: the kernel's registers)
        if best is None or cost <= best[0]:
            best = (cost, dict(sg=s, layout='single' if s == 1 else ('rows' if layout == 2 else 'cols'), P=p8, nsteps=ns, lds=lds))
    return None if best is None else best[1]


def images_per_chunk(B, sg, cout, cin, pairs=False, action=False, ipw=0, nsrc=0, cus=CUS):
    """Sched::wgrad_ops (nsrc == 0) / wgrad_ops_steps: images per chunk; cin: the channels the MFMA kernel covers."""
    blocks = cdiv(cdiv(cout, 16), 2) * cdiv(cdiv(cin, 16), 2)
    chunks = (1 if (pairs and not action) else 2) * cus // blocks
    if nsrc:
        chunks //= nsrc
    chunks = min(max(chunks, 1), B)
    n = cdiv(cdiv(B, chunks), sg) * sg
    return min(ipw, B) if ipw else n


def sparse_route(cin_real, cin, act_route=0):
    return cin > cin_real and (act_route == 2 if act_route else cdiv(cin, 16) - cdiv(cin_real, 16) >= 4)


def expect_plain(rid):
    """What the hook must report for run `rid` of wc.PLAIN_RUNS on a wgrad_precision='bf16x3' handle: dict(sg, layout, ipw, act, remap, nsteps, P)."""
    run = wc.PLAIN_RUNS[rid]
    board, cr, cin, A, cout, B = wc.SHAPES[run['shape']]
    over = run['over']
    g = geom(board, board, B, cout, cr, over.get('sg', 0), over.get('layout', 0))
    sparse = sparse_route(cr, cin, over.get('act_route', 0))
    ipw = images_per_chunk(B, g['sg'], cout, cr if sparse or not A else cin, action=bool(A), ipw=over.get('ipw', 0))
    return dict(sg=g['sg'], layout=g['layout'], ipw=ipw, act='none' if not A else ('sparse' if sparse else 'kernel'), remap=run['expect']['remap'],
                nsteps=g['nsteps'], P=g['P'])


def expect_pair(pid):
    first, second, over, (_, _, remap) = wc.PAIR_RUNS[pid]
    board, cr, cin, A, cout, B = wc.SHAPES[first]
    g = geom(board, board, B, cout, cr, over.get('sg', 0))
    return g['sg'], images_per_chunk(B, g['sg'], cout, cin, pairs=True, ipw=over.get('ipw', 0)), remap


def expect_steps(sid):
    key, nsrc, over, _ = wc.STEP_RUNS[sid]
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    g = geom(board, board, B, cout, cr, over.get('sg', 0))
    ipw = images_per_chunk(B, g['sg'], cout, cin, ipw=over.get('ipw', 0), nsrc=nsrc)
    return g['sg'], ipw, cdiv(B, ipw)


# every SG the split budget allows on the three smallest boards (side by side, stacked), and the first one over it
def sg_limit(key, layout):
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    n = 0
    while n < SG_CAP and geom(board, board, B, cout, cr, n + 1, layout) is not None:
        n += 1
    return n


SG_SHAPES = ('b3_9to16_n5', 'b5_40to24_n7', 'b6_128to128_n11')
SG_RUNS = [(key, lay, sg) for key in SG_SHAPES for lay in (1, 2) for sg in range(1, sg_limit(key, lay) + 1)]
SG_REFUSED = [(key, lay, sg_limit(key, lay) + 1) for key in ('b5_40to24_n7', 'b6_128to128_n11') for lay in (1, 2)] + [('b15_35to20_n3', 1, 2)]

PLAIN_IDS = ['b3_9to16_n5', 'b5_40to24_n7', 'b6_128to128_n11', 'b6_128to128_n11-sg4-ipw1', 'b6_128to128_n11-sg4-ipw4', 'b6_128to128_n11-sg4-ipw11',
             'b6_128to128_n11-sg4-ipw5', 'b6_128to128_n11-sg4-ipw8', 'b5_40to24_n7-sg3-ipw7', 'b6_128to128_n8', 'b6_128to128_n8-remap-off', 'b9_8to8_n1',
             'b13_24to24_n3', 'b15_35to20_n3', 'b9_32a82to32_n5', 'b9_32a82to32_n5-kernel', 'b3_16a10to16_n5', 'b3_16a10to16_n5-sparse', 'b3_16a10to16_n5-sg4']


# ------------------------------------------------------------------------------------------ the kernel's model
def _round_planes(dy, xf, imgs, sg, rows, P, ns):
    """(Y [co, 32 ns], X [ci, 32 ns + 2 P + 24]) float32: the planes of one staging round as the kernel fills them (idle slots stay zero)."""
    co, ci, h, w = dy.shape[1], xf.shape[1], dy.shape[2], dy.shape[3]
    Y, X = np.zeros((co, 32 * ns), np.float32), np.zeros((ci, 32 * ns + 2 * P + 24), np.float32)
    py, px = np.divmod(np.arange(h * w), w)
    for gi, b in enumerate(imgs):
        pos = (gi * (h + 1) + py) * P + px if (rows and sg > 1) else py * P + gi * (w + 1) + px
        assert pos.max() < 32 * ns
        Y[:, pos] = dy[b].reshape(co, -1)
        X[:, pos + P + 8] = xf[b].reshape(ci, -1)
    return Y, X


def model(dz, x, sg=1, ipw=1, rows=False, terms=TERMS, exact=False, **kw):
    """The split weight gradient [cout, cin, 3, 3] built the way k_lc_wgrad_bf16x3 builds it.  float32 accumulators (every MFMA's 32 products
    summed exactly, then added to the accumulator and rounded), chunks reduced in order in float32; exact=True: int64 throughout (integer data)."""
    dy, xf = wc.transform(dz, x, dtype=np.float32, **kw)
    B, co, h, w = dy.shape
    ci = xf.shape[1]
    P, ns = planes(h, w, sg, rows)[:2]
    pairs = {**cc.TERMS, **cc.DROPPED}
    acc_t = np.int64 if exact else np.float32
    out = np.zeros((co, ci, 9), acc_t)
    for chunk in wc.structure(B, sg, ipw):
        acc = np.zeros((co, ci, 9), acc_t)
        for rnd in chunk:
            Y, X = _round_planes(dy, xf, rnd, sg, rows, P, ns)
            Yt, Xt = cc.split3(Y), cc.split3(X)
            for g in range(ns):
                for t in range(9):
                    o = 32 * g + (t // 3 - 1) * P + (t % 3 - 1) + P + 8
                    for name in terms:
                        a, b = pairs[name]
                        prod = Yt[a][:, 32 * g:32 * g + 32] @ Xt[b][:, o:o + 32].T  # (float64: 32 products of 16-bit mantissas, exact)
                        acc[:, :, t] = (acc[:, :, t] + (np.rint(prod).astype(np.int64) if exact else prod)).astype(acc_t)
        out = (out + acc).astype(acc_t)
    return out.reshape(co, ci, 3, 3)


# ------------------------------------------------------------------------------------------ the Locator's extra positions
def locator_required(h, w, B, sg, ipw, rows=False):
    """(image, pixel) pairs beyond wc.locator_required: in EVERY image slot of a fullest round, every pixel whose plane position f has a dx = -1 / +1
    neighbour in another lane's 8-position group or another 32-position step (f % 8 in {0, 7}) or in another dword (f even: the left one, f odd:
    the right one; f % 8 in {1, 2} stand for those inside a group); on boards up to 6 x 6 every position of every slot."""
    P = planes(h, w, sg, rows)[0]
    big = max((rnd for ch in wc.structure(B, sg, ipw) for rnd in ch), key=len)
    req = []
    for gi, b in enumerate(big):
        for p in range(h * w):
            py, px = divmod(p, w)
            f = (gi * (h + 1) + py) * P + px if (rows and sg > 1) else py * P + gi * (w + 1) + px
            if h * w <= 36 or f % 8 in (0, 1, 2, 7):
                req.append((b, p))
    return req


def locator_draws(key, sg, ipw, rows=False):
    """[(dz, x)] covering locator_required, one-hot dz per output channel (wc.locator_x codes)."""
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    req = locator_required(board, board, B, sg, ipw, rows)
    x = wc.locator_x(B, cr, board, board)
    draws = []
    for d in range(cdiv(len(req), cout)):
        dz = np.zeros((B, cout, board, board), np.float32)
        for co in range(cout):
            b, p = req[(d * cout + co) % len(req)]
            dz[b, co, p // board, p % board] = 1.0
        draws.append((dz, x))
    return draws


@functools.lru_cache(maxsize=None)
def int_cases(key, sg, ipw, rows=False):
    """[(class, draw, dz, x, kw, int64 reference)] of a shape for a run that stages `sg` images per round in chunks of `ipw`: wc's three classes plus
    this kernel's Locator positions ('locator8'); references computed once and shared, read-only."""
    board, cr, cin, A, cout, B = wc.SHAPES[key]
    kw = dict(action=wc.actions(B, A), num_actions=A, cin=cin) if A else {}
    cases = [(cls, i, dz, x) for cls in wc.CLASSES for i, (dz, x) in enumerate(wc.int_draws(key, cls, sg, ipw))]
    cases += [('locator8', i, dz, x) for i, (dz, x) in enumerate(locator_draws(key, sg, ipw, rows))]
    out = []
    for cls, i, dz, x in cases:
        ref = wc.wgrad64(dz, x, dtype=np.int64, **kw)
        ref.setflags(write=False)
        out.append((cls, i, dz, x, kw, ref))
    return out
