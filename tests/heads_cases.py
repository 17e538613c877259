"""The conv learner's head block (csrc/mz_learn_conv.h k_lch_*) as a numpy float64 model, stage by stage, with a float32 "chain" twin of every
stage, and the data the tests run it on.  No GPU, no torch.

A geometry is `Geom(P, hw, A, K, Sr, Sv)`.  The heads are 0 reward (1 plane, Sr outputs, reads the dynamics tower's raw output F_rew), 1 policy
(2 planes, A outputs) and 2 value (1 plane, Sv outputs), both on the prediction tower's output F_pred; group g = 3 t + head is one application.  A
head with one output is a squared-error head (kind 0), the policy a soft-target cross entropy (kind 1), a head with a support a cross entropy against
the 2-hot projection of signed_hyperbolic(target) (kind 2).

Every stage function takes `dt`: np.float64 is the model (einsum / exact algebra), np.float32 the chain twin -- the same operation with every product
and sum rounded to float32, sums running sequentially (np.cumsum) in the order the kernel walks them.  The kernels' wave butterflies and fused
multiply-adds are a different, no worse, order: the GPU test gives a kernel twice the chain's error against the float64 model on the same inputs.
Stages that the kernels run in float64 (k_lch_bn, k_lch_bnb) have a chain that is the float64 value rounded where the kernel rounds.

`model(case, g, mut=...)` is the whole block in float64; `mut` names ONE deliberate arithmetic mistake (MUTATIONS), for tests/test_heads_host.py."""
import collections

import numpy as np

Geom = collections.namedtuple('Geom', 'P hw A K Sr Sv')
HEAD_NAMES = ('reward', 'policy', 'value')
MUTATIONS = ('no_1_over_K', 'weight_dropped_from_gradient', 'sp_dropped', 'targets_swapped', 'row_b_not_idx', 'no_clamp', 'no_1e-5', 'unit_spacing',
             'priority_from_t1', 'biased_running_var', 'running_once', 'policy_plane2_not_in_dF', 'reward_du_in_dF_pred', 'no_c3', 'dgamma_misses_a_step')
f32, f64 = np.float32, np.float64


def heads(g):
    """(oc, n_out, kind, source tower, target table) per head."""
    return ((1, g.Sr, 0 if g.Sr == 1 else 2, 'F_rew', 'reward'), (2, g.A, 1, 'F_pred', None), (1, g.Sv, 0 if g.Sv == 1 else 2, 'F_pred', 'value'))


def n_max(g):
    return max(g.A, g.Sr, g.Sv)


def ulp(x):
    """float32 spacing at |x| (of the binade's lower end: the conservative one)."""
    return np.spacing(np.abs(np.asarray(x, f64)).astype(f32)).astype(f64)


def seqsum(x, axis, dt):
    """sum along `axis`: float64 pairwise, or a running float32 sum in index order."""
    if dt == f64:
        return np.sum(np.asarray(x, f64), axis=axis)
    x = np.asarray(x, f32)
    if x.shape[axis] == 0:
        return np.zeros(np.delete(x.shape, axis), f32)
    return np.take(np.cumsum(x, axis=axis, dtype=f32), -1, axis=axis)


# ---- stages -------------------------------------------------------------------------------------------------------------------------------------------
def st_conv(F, w1, dt):
    """k_lch_conv: u[b][o][p] = sum_c w1[o][c] F[b][c][p], c ascending."""
    F, w1 = np.asarray(F, dt), np.asarray(w1, dt)
    if dt == f64:
        return np.einsum('oc,bcp->bop', w1, F)
    acc = np.zeros((F.shape[0], w1.shape[0], F.shape[2]), f32)
    for c in range(F.shape[1]):
        acc = acc + w1[None, :, c, None] * F[:, None, c, :]
    return acc


def st_pivot(u, piv, dt):
    """k_lch_conv's per-image partials around the pivot (u at position 0): [B][oc][2] = sum (u - p), sum (u - p)^2."""
    d = (np.asarray(u, dt) - np.asarray(piv, dt)[..., None]).astype(dt)
    return np.stack([seqsum(d, -1, dt), seqsum(d * d, -1, dt)], -1)


def st_bn(part, piv, n, gamma, beta, rm, rv, dt, mut=None):
    """k_lch_bn for one application: batch statistics from the pivoted partials [B][oc][2] and pivots [B][oc] of images of n positions; returns
    dict a, b, mean, invstd, rm, rv (the running statistics after this step).  The kernel works in float64 and rounds its outputs."""
    part, piv = np.asarray(part, f64), np.asarray(piv, f64)
    M = float(part.shape[0] * n)
    mean = (n * piv + part[..., 0]).sum(0) / M
    dp = piv - mean
    var = np.maximum((part[..., 1] + 2.0 * dp * part[..., 0] + n * dp * dp).sum(0) / M, 0.0)
    invstd = 1.0 / np.sqrt(var + 1e-5)
    unb = var if (mut == 'biased_running_var' or M <= 1.0) else var * M / (M - 1.0)
    if dt == f64:
        a = np.asarray(gamma, f64) * invstd
        return dict(a=a, b=np.asarray(beta, f64) - mean * a, mean=mean, invstd=invstd, rm=0.9 * np.asarray(rm, f64) + 0.1 * mean, rv=0.9 * np.asarray(rv, f64) + 0.1 * unb)
    inv32 = invstd.astype(f32)
    a = np.asarray(gamma, f32) * inv32
    return dict(a=a, b=np.asarray(beta, f32) - mean.astype(f32) * a, mean=mean.astype(f32), invstd=inv32,
                rm=(0.9 * np.asarray(rm, f32).astype(f64) + 0.1 * mean).astype(f32), rv=(0.9 * np.asarray(rv, f32).astype(f64) + 0.1 * unb).astype(f32))


def st_pre(u, a, b, dt):
    """the pre-activation a u + b, [B][oc][hw]."""
    return np.asarray(a, dt)[None, :, None] * np.asarray(u, dt) + np.asarray(b, dt)[None, :, None]


def st_feat(u, a, b, dt):
    return np.maximum(st_pre(u, a, b, dt), dt(0))


def st_logits(feat, lw, lb, dt):
    """logits[b][n] = lb[n] + sum_k feat[b][k] lw[n][k], k ascending; feat [B][nf]."""
    feat, lw, lb = np.asarray(feat, dt), np.asarray(lw, dt), np.asarray(lb, dt)
    if dt == f64:
        return feat @ lw.T + lb
    acc = np.broadcast_to(lb, (feat.shape[0], lw.shape[0])).astype(f32)
    for k in range(feat.shape[1]):
        acc = acc + feat[:, k, None] * lw[None, :, k]
    return acc


def signed_hyperbolic(x, dt):
    x = np.asarray(x, dt)
    return np.sign(x) * (np.sqrt(np.abs(x) + dt(1)) - dt(1)) + dt(0.001) * x


def signed_parabolic(x, dt):
    x = np.asarray(x, dt)
    e = dt(0.001)
    z = np.sqrt(dt(1) + dt(4) * e * (e + dt(1) + np.abs(x))) / dt(2) / e - dt(1.0 / 2.0 / 0.001)  # (the constant: a Python float in util.py, rounded once)
    return np.sign(x) * (z * z - dt(1))


def two_hot(x, S, dt, mut=None):
    """The 2-hot projection of signed_hyperbolic(x) onto linspace(-half, half, S), half = (S - 1) // 2: clamp, the two neighbouring bins share the mass,
    1e-5 in the interpolation denominator.  x [B] -> [B][S]."""
    half = dt((S - 1) // 2)
    z = signed_hyperbolic(x, dt)
    if mut != 'no_clamp':
        z = np.clip(z, -half, half)
    span = dt(2) * half
    pos = (z + half) / span * dt(S - 1)
    lo, hi = np.floor(pos), np.ceil(pos)
    slo, shi = lo / dt(S - 1) * span - half, hi / dt(S - 1) * span - half
    with np.errstate(invalid='ignore', divide='ignore'):
        wlo = (shi - z) / (shi - slo + (dt(0) if mut == 'no_1e-5' else dt(1e-5)))
    if mut == 'no_1e-5':
        wlo = np.where(shi == slo, dt(1), wlo)  # (0 / 0 without the constant: all the mass on the one bin)
    out = np.zeros((len(z), S), dt)
    r = np.arange(len(z))
    for b, wt in ((lo, wlo), (hi, dt(1) - wlo)):
        ok = (b >= 0) & (b <= S - 1)  # (all true with the clamp; without it the mass of a bin off the support is lost)
        np.add.at(out, (r[ok], b[ok].astype(int)), wt[ok])
    return out


def support(S, dt, mut=None):
    half = (S - 1) // 2
    if mut == 'unit_spacing':
        return (np.arange(S) - half).astype(dt)
    return np.linspace(-half, half, S).astype(dt) if S > 1 else np.zeros(1, dt)


def st_targets(case, g, hd, t, mut=None):
    """(scalar target [B] or None, policy rows [B][A] or None) of head hd at step t, float32 as stored."""
    rows = np.arange(len(case['idx'])) if mut == 'row_b_not_idx' else np.asarray(case['idx'])
    tab = heads(g)[hd][4]
    if tab is None:
        return None, case['pi'][rows, t]
    if mut == 'targets_swapped':
        tab = 'value' if tab == 'reward' else 'reward'
    return case[tab][rows, t], None


def st_loss(logits, kind, scalar, pi, w, K, dt, mut=None, S=None):
    """k_lch_loss's loss part for one group: returns dict lpart [B], dlogit [B][n], prio [B] (the scalar-space |prediction - target|; the caller keeps
    the value head's at the priority step), and for the counted-ulp checks softmax [B][n], lse [B] (of logits - max), target [B][n]."""
    lg, w = np.asarray(logits, dt), np.asarray(w, dt)
    B = lg.shape[0]
    gs = w / (dt(B) * dt(K))
    if mut == 'no_1_over_K':
        gs = w / dt(B)
    if mut == 'weight_dropped_from_gradient':
        gs = np.ones_like(w) / (dt(B) * dt(K))
    if kind == 0:
        d = lg[:, 0] - np.asarray(scalar, dt)
        return dict(lpart=d * d * w, dlogit=(dt(2) * d * gs)[:, None], prio=np.abs(d))
    tg = np.asarray(pi, dt) if kind == 1 else two_hot(scalar, S, dt, mut)
    mx = lg.max(1, keepdims=True)
    e = np.exp(lg - mx)
    se = seqsum(e, 1, dt)
    sp = seqsum(tg, 1, dt)
    spl = seqsum(tg * (lg - mx), 1, dt)
    lse = np.log(se)
    sm = e / se[:, None]
    if mut == 'sp_dropped':
        sp = np.ones_like(sp)
    out = dict(lpart=(sp * lse - spl) * w, dlogit=(sm * sp[:, None] - tg) * gs[:, None], softmax=sm, lse=lse, target=tg)
    if kind == 2:
        sev = seqsum(e * support(S, dt, mut)[None, :], 1, dt)
        out['expect'] = sev / se
        out['prio'] = np.abs(signed_parabolic(sev / se, dt) - np.asarray(scalar, dt))
    return out


def st_dz(dlogit, lw, feat, dt):
    """dz[b][k] = [feat > 0] sum_n lw[n][k] dlogit[b][n], n ascending."""
    dl, lw = np.asarray(dlogit, dt), np.asarray(lw, dt)
    if dt == f64:
        a = dl @ lw
    else:
        a = np.zeros((dl.shape[0], lw.shape[1]), f32)
        for n in range(lw.shape[0]):
            a = a + lw[None, n, :] * dl[:, n, None]
    return np.where(np.asarray(feat) > 0, a, dt(0))


def st_bpart(dz, u, dt):
    """k_lch_loss's backward partials [B][oc][2] = sum dz, sum dz u over the positions."""
    dz, u = np.asarray(dz, dt), np.asarray(u, dt)
    return np.stack([seqsum(dz, -1, dt), seqsum(dz * u, -1, dt)], -1)


def st_bnb(bpart, mean, invstd, gamma, M, dt, mut=None):
    """k_lch_bnb for one application: dict dgamma, dbeta (this step's), c1, c2, c3.  Float64 in the kernel, outputs rounded."""
    s = np.asarray(bpart, f64).sum(0)
    s1, s2 = s[..., 0], s[..., 1]
    mean, invstd, gam = np.asarray(mean, f64), np.asarray(invstd, f64), np.asarray(gamma, f64)
    dgam = (s2 - mean * s1) * invstd
    c1 = gam * invstd
    c3 = -c1 * s1 / M + c1 * mean * invstd * dgam / M
    if mut == 'no_c3':
        c3 = np.zeros_like(c3)
    out = dict(dgamma=dgam, dbeta=s1, c1=c1, c2=-c1 * invstd * dgam / M, c3=c3)
    return out if dt == f64 else {k: (v.astype(f32) if k.startswith('c') else v) for k, v in out.items()}


def st_du(dz, u, c1, c2, c3, dt):
    c1, c2, c3 = (np.asarray(c, dt)[None, :, None] for c in (c1, c2, c3))
    return c1 * np.asarray(dz, dt) + (c2 * np.asarray(u, dt) + c3)


def st_dF(dus, w1s, dt):
    """k_lch_dx: dF[b][c][p] = sum over the heads e on this tower output, their planes o: w1_e[o][c] du_e[b][o][p], in that order."""
    acc = None
    for du, w1 in zip(dus, w1s):
        du, w1 = np.asarray(du, dt), np.asarray(w1, dt)
        for o in range(w1.shape[0]):
            term = w1[o][None, :, None] * du[:, o][:, None, :]
            acc = term if acc is None else acc + term
    return acc


def st_dw1(du, F, dt):
    """k_lch_dw1: dw1[o][c] = sum_b sum_p du[b][o][p] F[b][c][p]."""
    du, F = np.asarray(du, dt), np.asarray(F, dt)
    if dt == f64:
        return np.einsum('bop,bcp->oc', du, F)
    out = np.zeros((du.shape[1], F.shape[1]), f32)
    for o in range(du.shape[1]):
        out[o] = seqsum((du[:, o][:, None, :] * F).transpose(1, 0, 2).reshape(F.shape[1], -1), 1, f32)
    return out


def st_dlin(dlogit, feat, dt):
    """k_lch_dlin: dlw[n][k] = sum_b dlogit[b][n] feat[b][k], dlb[n] = sum_b dlogit[b][n], b ascending."""
    dl, feat = np.asarray(dlogit, dt), np.asarray(feat, dt)
    if dt == f64:
        return dl.T @ feat, dl.sum(0)
    acc, accb = np.zeros((dl.shape[1], feat.shape[1]), f32), np.zeros(dl.shape[1], f32)
    for b in range(dl.shape[0]):
        acc = acc + dl[b][:, None] * feat[b][None, :]
        accb = accb + dl[b]
    return acc, accb


# ---- the whole block --------------------------------------------------------------------------------------------------------------------------------------
def model(case, g, mut=None, dt=f64):
    """The head block on `case` in float64 (or as one float32 chain).  Returns loss, prio [B], dF_pred / dF_rew [K][B][P][hw], grads (per head a dict
    w1, gamma, beta, lw, lb), running (per head (mean, var)), nbt [3], and per group (list index 3 t + head) the intermediates u, part, piv, bn, pre,
    feat, logits, loss (st_loss's dict), dz, bpart, bnb, du."""
    K, B, hw = g.K, len(case['idx']), g.hw
    H = heads(g)
    G = [None] * (3 * K)
    running = [(np.asarray(r[0], dt), np.asarray(r[1], dt)) for r in case['running']]
    nbt = np.array(case['nbt'], np.int64)
    prio_t = 1 if (mut == 'priority_from_t1' and K > 1) else 0
    prio, lsum = None, 0.0
    for t in range(K):
        for hd, (oc, n, kind, src, _) in enumerate(H):
            p = case['heads'][hd]
            r = dict(F=case[src][t])
            r['u'] = st_conv(r['F'], p['w1'], dt)
            r['piv'] = r['u'][..., 0]
            r['part'] = st_pivot(r['u'], r['piv'], dt)
            r['bn'] = st_bn(r['part'], r['piv'], hw, p['gamma'], p['beta'], running[hd][0], running[hd][1], dt, mut)
            if not (mut == 'running_once' and t > 0):
                running[hd] = (r['bn']['rm'], r['bn']['rv'])
                nbt[hd] += 1
            r['pre'] = st_pre(r['u'], r['bn']['a'], r['bn']['b'], dt)
            r['feat'] = np.maximum(r['pre'], dt(0))
            r['logits'] = st_logits(r['feat'].reshape(B, -1), p['lw'], p['lb'], dt)
            sc, pi = st_targets(case, g, hd, t, mut)
            r['loss'] = st_loss(r['logits'], kind, sc, pi, case['w'], K, dt, mut, n)
            lsum = lsum + np.asarray(r['loss']['lpart'], f64).sum()
            if hd == 2 and t == prio_t:
                prio = r['loss']['prio']
            r['dz'] = st_dz(r['loss']['dlogit'], p['lw'], r['feat'].reshape(B, -1), dt).reshape(B, oc, hw)
            r['bpart'] = st_bpart(r['dz'], r['u'], dt)
            r['bnb'] = st_bnb(r['bpart'], r['bn']['mean'], r['bn']['invstd'], p['gamma'], float(B * hw), dt, mut)
            r['du'] = st_du(r['dz'], r['u'], r['bnb']['c1'], r['bnb']['c2'], r['bnb']['c3'], dt)
            G[3 * t + hd] = r
    dFp, dFr, grads = [], [], []
    for t in range(K):
        rw, po, va = G[3 * t], G[3 * t + 1], G[3 * t + 2]
        dus, w1s = [po['du'], va['du']], [case['heads'][1]['w1'], case['heads'][2]['w1']]
        if mut == 'policy_plane2_not_in_dF':
            dus[0], w1s[0] = po['du'][:, :1], np.asarray(w1s[0])[:1]
        if mut == 'reward_du_in_dF_pred':
            dus.append(rw['du'])
            w1s.append(case['heads'][0]['w1'])
        dFp.append(st_dF(dus, w1s, dt))
        dFr.append(st_dF([rw['du']], [case['heads'][0]['w1']], dt))
    wparts = []
    for hd, (oc, n, kind, src, _) in enumerate(H):
        steps = []
        for t in range(K):
            r = G[3 * t + hd]
            dlw, dlb = st_dlin(r['loss']['dlogit'], r['feat'].reshape(B, -1), dt)
            steps.append(dict(w1=st_dw1(r['du'], r['F'], dt), lw=dlw, lb=dlb))
        wparts.append(steps)
        tt = range(K - 1) if (mut == 'dgamma_misses_a_step' and K > 1) else range(K)
        gd = {}
        for k in ('w1', 'lw', 'lb'):
            acc = np.zeros_like(steps[0][k])
            for s in steps:
                acc = acc + s[k]
            gd[k] = acc
        gd['gamma'] = np.sum([G[3 * t + hd]['bnb']['dgamma'] for t in tt], 0)
        gd['beta'] = np.sum([G[3 * t + hd]['bnb']['dbeta'] for t in range(K)], 0)
        grads.append(gd)
    return dict(loss=lsum / B, prio=prio, dF_pred=np.stack(dFp), dF_rew=np.stack(dFr), grads=grads, running=running, nbt=nbt, groups=G, wparts=wparts)


# ---- data ---------------------------------------------------------------------------------------------------------------------------------------------
MARGIN = 2.0 ** -10  # x the largest |a u + b| of the case: the least |pre-activation| a random case may hold


def _params(rs, g, integer):
    out = []
    for oc, n, kind, _, _ in heads(g):
        nf = oc * g.hw
        if integer:
            w1 = (rs.randint(-1, 2, (oc, g.P)) * (rs.rand(oc, g.P) < 0.6)).astype(f32)
            lw = rs.randint(-2, 3, (n, nf)).astype(f32) / 8
        else:
            w1 = (rs.standard_normal((oc, g.P)) * np.sqrt(2.0 / g.P)).astype(f32)
            lw = (rs.standard_normal((n, nf)) * np.sqrt(2.0 / nf)).astype(f32)
        out.append(dict(w1=w1, gamma=(1.0 + 0.2 * rs.standard_normal(oc)).astype(f32), beta=(0.3 * rs.standard_normal(oc)).astype(f32), lw=lw,
                        lb=(0.05 * rs.standard_normal(n)).astype(f32)))
    return out


def _targets(rs, g, B, rows):
    idx = rs.randint(0, rows, B).astype(np.int64)  # (repeats and any order)
    return dict(pi=rs.dirichlet(np.ones(g.A), size=(rows, g.K)).astype(f32), value=(rs.uniform(-1, 1, (rows, g.K)) * (8.0 if g.Sv > 1 else 1.0)).astype(f32),
                reward=(rs.uniform(-1, 1, (rows, g.K)) * (3.0 if g.Sr > 1 else 1.0)).astype(f32), idx=idx, w=rs.uniform(0.3, 1.0, B).astype(f32),
                running=[((0.1 * rs.standard_normal(oc)).astype(f32), (0.5 + np.abs(rs.standard_normal(oc))).astype(f32)) for oc, *_ in heads(g)],
                nbt=np.array([7, 11, 13], np.int64))


def pre_activations(case, g):
    """float64 a u + b of every group, [3 K] arrays [B][oc][hw]."""
    out = []
    for t in range(g.K):
        for hd, (oc, n, kind, src, _) in enumerate(heads(g)):
            p = case['heads'][hd]
            u = st_conv(case[src][t], p['w1'], f64)
            bn = st_bn(st_pivot(u, u[..., 0], f64), u[..., 0], g.hw, p['gamma'], p['beta'], 0.0, 1.0, f64)
            out.append(st_pre(u, bn['a'], bn['b'], f64))
    return out


def margin(case, g):
    """(least |a u + b|, largest |a u + b|) over every element of every group, float64."""
    pre = pre_activations(case, g)
    return min(float(np.abs(p).min()) for p in pre), max(float(np.abs(p).max()) for p in pre)


def _off_the_kink(rs, case, g, draw):
    """Redraw the tower-output columns F[t][b][:][p] that leave a pre-activation within the margin, until none does (a column feeds every plane on its
    tower; the batch statistics move a little with each redraw, hence the loop)."""
    for _ in range(200):
        pre = pre_activations(case, g)
        top = max(float(np.abs(p).max()) for p in pre)
        bad = {'F_rew': np.zeros((g.K, len(case['idx']), g.hw), bool), 'F_pred': np.zeros((g.K, len(case['idx']), g.hw), bool)}
        for i, p in enumerate(pre):
            bad[heads(g)[i % 3][3]][i // 3] |= (np.abs(p) < 1.5 * MARGIN * top).any(1)  # (1.5: clear of the bar itself)
        if not bad['F_rew'].any() and not bad['F_pred'].any():
            return case
        for k, m in bad.items():
            t, b, p = np.nonzero(m)
            case[k][t, b, :, p] = draw((len(t), g.P))
    raise RuntimeError('no case off the kink in 200 rounds')


def random_case(g, B, seed, rows=None):
    """Seeded random data with every |a u + b| >= MARGIN x the case's largest (margin(case, g) says so; tests/test_heads_host.py asserts it)."""
    rs = np.random.RandomState(seed)
    rows = rows or B + 3
    case = dict(F_pred=rs.standard_normal((g.K, B, g.P, g.hw)).astype(f32), F_rew=rs.standard_normal((g.K, B, g.P, g.hw)).astype(f32), heads=_params(rs, g, False))
    case.update(_targets(rs, g, B, rows))
    return _off_the_kink(rs, case, g, lambda shape: rs.standard_normal(shape).astype(f32))


def integer_case(g, B, seed, rows=None):
    """Small integers: F in [-2, 2], w1 in {-1, 0, 1}: |u| <= 2 P, the pivoted sums stay below hw (4 P)^2 -- below 2^24 for P <= 40, hw <= 240
    (integer_bound says what the case reaches) -- so u, the partials and the pivots are exact in float32 in any order.  Off the kink like random_case."""
    rs = np.random.RandomState(seed)
    rows = rows or B + 3
    draw = lambda shape: rs.randint(-2, 3, shape).astype(f32)  # noqa: E731
    case = dict(F_pred=draw((g.K, B, g.P, g.hw)), F_rew=draw((g.K, B, g.P, g.hw)), heads=_params(rs, g, True))
    case.update(_targets(rs, g, B, rows))
    return _off_the_kink(rs, case, g, draw)


def integer_bound(case, g):
    """The largest sum of absolute terms any forward sum of an integer case reaches (u itself, sum |u - p|, sum (u - p)^2)."""
    top = 0.0
    for t in range(g.K):
        for hd, (oc, n, kind, src, _) in enumerate(heads(g)):
            w1, F = np.abs(case['heads'][hd]['w1']).astype(f64), case[src][t].astype(f64)
            u = st_conv(F, case['heads'][hd]['w1'], f64)
            d = u - u[..., :1]
            top = max(top, float(np.einsum('oc,bcp->bop', w1, np.abs(F)).max()), float(np.abs(d).sum(-1).max()), float((d * d).sum(-1).max()))
    return top


# ---- the hook's flat layouts -------------------------------------------------------------------------------------------------------------------------------
def flat_params(hp):
    return np.concatenate([np.concatenate([np.asarray(p[k], f32).ravel() for k in ('w1', 'gamma', 'beta', 'lw', 'lb')]) for p in hp])


def split_params(flat, g):
    out, o = [], 0
    for oc, n, *_ in heads(g):
        d = {}
        for k, shape in (('w1', (oc, g.P)), ('gamma', (oc,)), ('beta', (oc,)), ('lw', (n, oc * g.hw)), ('lb', (n,))):
            sz = int(np.prod(shape))
            d[k] = np.asarray(flat[o:o + sz]).reshape(shape)
            o += sz
        out.append(d)
    return out


def split_wpart(wpart, g):
    """[K][hp_total] -> per head a list over steps of dict w1, lw, lb."""
    out, o = [], 0
    for oc, n, *_ in heads(g):
        sizes = (('w1', (oc, g.P)), ('lw', (n, oc * g.hw)), ('lb', (n,)))
        steps = []
        for t in range(wpart.shape[0]):
            d, oo = {}, o
            for k, shape in sizes:
                sz = int(np.prod(shape))
                d[k] = wpart[t, oo:oo + sz].reshape(shape)
                oo += sz
            steps.append(d)
        o += sum(int(np.prod(s)) for _, s in sizes)
        out.append(steps)
    return out


# ---- edge data ------------------------------------------------------------------------------------------------------------------------------------------
def edge_case(g, B, seed):
    """random_case with the targets, rows and weights at their edges (the tower outputs and parameters, hence the margins, are random_case's): value and
    reward targets at 0, at +-(half +- 0.01) in transformed space, and far outside the support; policy rows all zero and summing to 0.5; weights zero
    and spread over 1e4; idx out of order with repeats, never the identity."""
    case = random_case(g, B, seed, rows=B + 5)
    rs = np.random.RandomState(seed + 1)
    rows = B + 5
    for tab, S in (('value', g.Sv), ('reward', g.Sr)):
        half = (S - 1) // 2 if S > 1 else 1
        zs = [0.0, half - 0.01, half + 0.01, -(half - 0.01), -(half + 0.01), 3.0 * half + 1.0, -(3.0 * half + 1.0)]
        xs = np.concatenate([signed_parabolic(np.array(zs), f64), [0.0, 1e4, -1e4]])
        flat = case[tab].reshape(-1)
        flat[rs.permutation(flat.size)[:min(flat.size, len(xs))]] = xs[:min(flat.size, len(xs))].astype(f32)
    case['pi'][0] = 0.0
    case['pi'][1] *= 0.5
    case['idx'] = np.concatenate([[1, 0, 0], rs.randint(0, rows, B)])[:B].astype(np.int64) if B > 1 else np.array([1], np.int64)
    case['w'] = (10.0 ** rs.uniform(-2, 2, B)).astype(f32)
    if B > 2:
        case['w'][rs.permutation(B)[:max(1, B // 8)]] = 0.0
    return case


def variant(case, g, name):
    """A copy of `case` with one parameter edge: 'big_logits' (Linear weights scaled so that logits reach +-80), 'gamma0' (gamma = 0 on the policy's second
    plane: its pre-activation is beta alone), 'constant_plane' (the value head's 1x1 conv is zero: u = 0, variance 0, invstd = 1 / sqrt(1e-5))."""
    c = dict(case)
    c['heads'] = [dict(p) for p in case['heads']]
    if name == 'big_logits':
        ref = model(case, g)
        for hd in range(3):
            top = max(float(np.abs(ref['groups'][3 * t + hd]['logits']).max()) for t in range(g.K))
            s = f32(80.0 / max(top, 1e-3))
            c['heads'][hd]['lw'], c['heads'][hd]['lb'] = case['heads'][hd]['lw'] * s, case['heads'][hd]['lb'] * s
    elif name == 'gamma0':
        c['heads'][1]['gamma'] = np.array([case['heads'][1]['gamma'][0], 0.0], f32)
        c['heads'][1]['beta'] = np.array([case['heads'][1]['beta'][0], 0.5], f32)
    elif name == 'constant_plane':
        c['heads'][2]['w1'] = np.zeros_like(case['heads'][2]['w1'])
        c['heads'][2]['beta'] = np.array([0.5], f32)
    else:
        raise KeyError(name)
    return c


# ---- the cases of tests/test_gpu_heads.py (tests/test_heads_host.py checks their data bounds without a GPU) ----------------------------------------------------
GEOMS = {  # name: (kind, Geom, what the net is built from)
    'board3': Geom(16, 9, 10, 2, 1, 1), 'board5': Geom(16, 25, 26, 3, 1, 1), 'board15': Geom(16, 225, 226, 2, 1, 1), 'board15x16': Geom(16, 240, 241, 2, 1, 1),
    'board3_p40': Geom(40, 9, 10, 3, 1, 1), 'atari': Geom(8, 36, 6, 3, 11, 5), 'atari301': Geom(8, 36, 6, 2, 11, 301),
}
BATCHES = {'board3': (1, 2, 63, 64, 65, 130), 'board5': (2, 65), 'board15': (2, 65, 130), 'board15x16': (3, 64), 'board3_p40': (1, 63), 'atari': (1, 2, 63, 65),
           'atari301': (2, 64)}


def case_seed(name, B):
    return 1000 * (sorted(GEOMS).index(name) + 1) + B
