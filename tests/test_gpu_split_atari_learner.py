"""The opt-in split-bf16 convs of the Atari learner (mzl_set_atari_precision; HipLearner(tower_precision=, stage_precision=);
muzero_amd/csrc/mz_learn_conv_split.h, the HALO / PLANE builds) and the first per-launch test of the tile path at BOTH precisions.

1. One tile-path conv through mzl_debug_conv_tile -- the update's own gather, geometry, op builder and dispatcher -- on a 24 x 24 plane (2 x 2 tiles of
   12 x 12) and a 48 x 48 plane (4 x 3 wide tiles of 12 x 16), batch 1 and 2, 16 -> 16, 48 -> 24 and 32 -> 32 channels, forward and data gradient, on
   the integer data of tests/split_atari_cases.py (classes W, X, M and the Locator; tests/test_split_atari_learner_host.py checks the bounds and that
   each planted mistake breaks it): the whole plane EQUALS the int64 conv, border and every tile seam included, with and without skip and mask, on the
   plane route and on both scatter routes, at 'f32' and 'bf16x3'.  The statistics partials on small integers equal the exact sums.
2. The same hook on seeded random data against float64: relative rms error over the whole output and per output channel at most BAR = 2 x a
   sequential float32 chain's (tests/test_gpu_conv_layer.py's bar and statistics).
3. Whole gradients on the small Atari fixture net at batch 2 and 3, K = 1 and 2, for the four switch combinations, against float64 autograd on the
   pass's own branches: every tensor within max(the float32 path's bar, 2 x the float32 HIP learner's error on that tensor).
4. The reference fixture at tests/test_gpu_atari_learner.py's bars.  5. Identity and determinism.  6. Refusals.

Which tensors must be byte-identical to the all-'f32' handle, from the graph: a parameter's gradient is a function of dL/d(its layer's output), and
every such path starts at the loss, whose inputs (the heads' outputs) lie downstream of res_blocks_1 (stage) and of res_blocks_3 and the 6 x 6 towers
(tower) in the forward pass -- so with either switch on NO gradient tensor is free of a split conv, forward or backward, and none is held to
equality.  What IS upstream of every split conv is the forward pass of the layers before the first split layer: with stage_precision 'f32' and
tower_precision 'bf16x3' the BatchNorm running statistics of res_blocks_1 and res_blocks_2 are byte-identical to the all-'f32' handle's, and test 3
holds them to that; with both 'f32' everything is (test 5)."""
import copy
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import conv_fused_cases as cfc
import conv_layer_cases as cc
import split_atari_cases as sa
from helpers import build_conv, build_mlp, conv_case, load_golden, mlp_case
from muzero_amd.replay import Transition
from test_gpu_conv_layer import BAR
from test_gpu_conv_learner import _same_branch, same_branch_bar

pytestmark = pytest.mark.gpu
PRECISIONS = ('f32', 'bf16x3')
COMBOS = (('f32', 'f32'), ('bf16x3', 'f32'), ('f32', 'bf16x3'), ('bf16x3', 'bf16x3'))  # (tower_precision, stage_precision)
SPLIT_COMBOS = COMBOS[1:]
G = load_golden('learn_cases.npz')


def _hip(net, dev, max_batch, K=5, **kw):
    from muzero_amd.hip_learner import HipLearner

    kw.setdefault('lr', 1e-3)
    return HipLearner(net, dev, K, max_batch, **kw)


def _ring(tr, dev):
    B = tr.state.shape[0]
    return dict(state=torch.from_numpy(tr.state).to(dev).reshape(B, -1).contiguous(), action=torch.from_numpy(tr.action).to(dev),
                pi_prob=torch.from_numpy(tr.pi_prob).to(dev), value=torch.from_numpy(tr.value).to(dev), reward=torch.from_numpy(tr.reward).to(dev))


def _atari_net(dev):
    net = build_conv(conv_case('atari_s')).to(dev)
    net.train()
    return net


@pytest.fixture(scope='module')
def hook():
    """A small Atari learner with both switches at their default: the hook takes its precision from the call."""
    dev = torch.device('cuda', 0)
    hl = _hip(_atari_net(dev), dev, 2, K=1)
    yield hl
    hl.close()


# ------------------------------------------------------------------------------------------ 1. one tile conv, exact integers
RUNS = [(p, c, B, d) for p in sa.PLANES for c in sa.CHANNELS for B in sa.BATCHES for d in (0, 1)]
RUN_IDS = [f'{p}-{c[0]}to{c[1]}-n{B}-d{d}' for p, c, B, d in RUNS]


def _expect_name(name, precision, plane, route):
    wide = plane == 'p48'
    npt = {'plane': 12 if wide else 9, 'inner': 12 if wide else 9, 'whole': 16 if wide else 13}[route]
    kernel = 'bf16x3 k_lc_conv_bf16x3 ' if precision == 'bf16x3' else 'f32 k_lc_conv '
    want = f'{kernel}NPT={npt} HALO={0 if route == "whole" else 1} PLANE={1 if route == "plane" else 0} tile=12x{16 if wide else 12} '
    assert name.startswith(want), (name, want)


def _first_difference(out, ref):
    bad = np.argwhere(out != ref)
    return None if len(bad) == 0 else f'{len(bad)} outputs differ, first at (image, channel, y, x) = {bad[0].tolist()}: {out[tuple(bad[0])]} != {ref[tuple(bad[0])]}'


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('plane,chan,B,direction', RUNS, ids=RUN_IDS)
def test_integer_tile_conv_equals_the_int64_conv(hook, plane, chan, B, direction, precision):
    H, W = sa.PLANES[plane]
    launches = 0
    for cls in sa.CLASSES:
        x, ws = sa.int_case(cls, plane, chan, B, direction)
        for i, w in enumerate(ws):
            ref = cc.int_reference(x, w, np.zeros(w.shape[0], np.float32)).astype(np.float32)
            out, name = hook.debug_conv_tile(direction, sa.hook_weight(w, direction), x, precision=precision)
            _expect_name(name, precision, plane, 'plane')
            d = _first_difference(out, ref)
            assert d is None, f'{precision} class {cls} {plane} {chan} batch {B} direction {direction} draw {i} ({name}): {d}'
            launches += 1
            if cls == 'locator':  # what was read on both sides of every seam and in every corner, by name
                for r, c in sa.seam_positions(H, W):
                    assert np.array_equal(out[:, :, r, c], ref[:, :, r, c]), (r, c)
    # the epilogue on the plane route: + skip, then the mask (with and without its coefficients), as the update's data gradients use them
    x, ws = sa.int_case('M', plane, chan, B, direction)
    w = ws[-1]
    conv = cc.int_reference(x, w, np.zeros(w.shape[0], np.float32))
    skip, mask, mcoef, partner = sa.epilogue_operands(plane, chan, B, direction)
    for kw, ref in ((dict(skip=skip), cfc.epilogue(conv, skip)), (dict(skip=skip, mask=mask, partner=partner), cfc.epilogue(conv, skip, mask)),
                    (dict(mask=mask, mcoef=mcoef, partner=partner), cfc.epilogue(conv, None, mask, mcoef))):
        out, name = hook.debug_conv_tile(direction, sa.hook_weight(w, direction), x, precision=precision, **kw)[:2]
        d = _first_difference(out, ref.astype(np.float32))
        assert d is None, f'{precision} {plane} {chan} batch {B} direction {direction} epilogue {sorted(kw)} ({name}): {d}'
        assert ('ST_BWD' in name) == ('mask' in kw), name
    # the scatter routes (MZLC_NO_OUT_PLANE / MZLC_NO_HALO_IN's forms): the HALO builds without PLANE, the whole haloed tiles (NPT 16 / 13)
    for route in ('inner', 'whole'):
        out, name = hook.debug_conv_tile(direction, sa.hook_weight(w, direction), x, skip=skip, precision=precision, route=route)
        _expect_name(name, precision, plane, route)
        d = _first_difference(out, cfc.epilogue(conv, skip).astype(np.float32))
        assert d is None, f'{precision} {plane} {chan} batch {B} direction {direction} route {route} ({name}): {d}'
    print(f'{plane} {chan} batch {B} direction {direction} {precision}: {launches + 5} launches, {name}')


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('plane', list(sa.PLANES))
def test_tile_statistics_partials_are_the_exact_sums(hook, plane, precision):
    """ST_FWD (pivot, sum (y - p), sum (y - p)^2, n) and ST_BWD (sum t, sum t partner) per tile, on integers small enough that every sum is exact."""
    chan, B = (48, 24), 2
    H, W = sa.PLANES[plane]
    tw = sa.tile_w(W)
    for direction in (0, 1):
        x, w = sa.small_case(plane, chan, B, direction)
        conv = cc.int_reference(x, w, np.zeros(w.shape[0], np.float32)).astype(np.float64)
        tiles = lambda a: sa.cut_tiles(np.asarray(a, np.float64), tw)[:, :, 1:-1, 1:-1]  # noqa: E731  [B * tiles, C, 12, tw] in the kernel's tile order
        out, name, part = hook.debug_conv_tile(direction, sa.hook_weight(w, direction), x, precision=precision, want_part=True)
        assert 'ST_FWD' in name and np.array_equal(out, conv.astype(np.float32))
        assert np.array_equal(part.astype(np.float64), cfc.partials_fwd(tiles(conv), 1)), (plane, direction, name)
        skip, mask, _, partner = sa.epilogue_operands(plane, chan, B, direction)
        t = cfc.epilogue(conv, skip % 3, mask)
        out, name, part = hook.debug_conv_tile(direction, sa.hook_weight(w, direction), x, skip=skip % 3, mask=mask, partner=partner, precision=precision, want_part=True)
        assert 'ST_BWD' in name and np.array_equal(out, t.astype(np.float32))
        assert np.array_equal(part.astype(np.float64), cfc.partials_bwd(tiles(t), tiles(partner), 1)), (plane, direction, name)


# ------------------------------------------------------------------------------------------ 2. one tile conv, random data
@functools.lru_cache(maxsize=None)
def _random_reference(plane, direction):
    """(input, the hook's weight, float64 reference, the chain's statistics) of the 48 -> 24 layer at batch 2: computed once, shared by both
    precisions, never written to.  Slices: the whole output (2 x c_out x H x W values) and each output channel (2 x H x W >= 1152 values)."""
    H, W = sa.PLANES[plane]
    c_in, c_out = (48, 24) if direction == 0 else (24, 48)
    d = cc.random_layer(3100 + 2 * sorted(sa.PLANES).index(plane) + direction, 2, c_in, c_in, c_out, H, W)
    ref, c32 = cc.conv64(d['x'], d['w']), cc.chain32(d['x'], d['w'])
    e_chain = {s: cc.rel_rms(c32, ref, cc.SLICES[s]) for s in ('whole', 'channel')}
    w_hook = sa.hook_weight(d['w'], direction)
    for a in (d['x'], w_hook, ref):
        a.setflags(write=False)
    return d['x'], w_hook, ref, e_chain


def tile_accuracy(hl, plane, direction, precision):
    """{slice: (kernel error / chain error per slice, kernel error, chain error)} and the build name (also tools/split_atari_learner_bench.py)."""
    x, w_hook, ref, e_chain = _random_reference(plane, direction)
    out, name = hl.debug_conv_tile(direction, w_hook, x, precision=precision)
    res = {}
    for s in ('whole', 'channel'):
        e = cc.rel_rms(out, ref, cc.SLICES[s])
        res[s] = (np.atleast_1d(e / e_chain[s]), np.atleast_1d(e), np.atleast_1d(e_chain[s]))
    return res, name


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('direction', (0, 1))
@pytest.mark.parametrize('plane', list(sa.PLANES))
def test_random_tile_conv_matches_float64_within_twice_a_float32_chain(hook, plane, direction, precision):
    res, name = tile_accuracy(hook, plane, direction, precision)
    print(f'{plane} direction {direction} {precision}: {name}')
    for s, (r, e, ec) in res.items():
        print(f'  {s}: E kernel {e.max():.3g} (max), E chain32 {ec.max():.3g} (max), ratio max {r.max():.3f} median {np.median(r):.3f} over {r.size} slices')
    for s, (r, e, ec) in res.items():
        assert np.all(e <= BAR * ec), f'{plane} direction {direction} {precision} {s}: E = {r.max():.3f} x chain32 (bar {BAR})'


# ------------------------------------------------------------------------------------------ 3. the whole gradient
def _fixture_batch(B, K, seed):
    name, kind, (chan, fh, fw), A = conv_case('atari_s')[:4]
    rs = np.random.RandomState(seed)
    tr = Transition(rs.uniform(0, 1, (B, chan, fh, fw)).astype(np.float32), rs.randint(0, A, (B, K)).astype(np.int8),
                    rs.dirichlet(np.ones(A), size=(B, K)).astype(np.float32), (rs.uniform(-1, 1, (B, K)) * 8.0).astype(np.float32),
                    rs.uniform(-1, 1, (B, K)).astype(np.float32))
    return tr, rs.uniform(0.3, 1.0, B).astype(np.float32)


def _grad_run(dev, tr, w, B, K, **kw):
    """One gradient of a fresh learner on the fixture net: everything test 3 compares."""
    net = _atari_net(dev)
    hl = _hip(net, dev, B, K=K, **kw)
    loss, prio = hl.grad(_ring(tr, dev), None, torch.from_numpy(w).to(dev), B)
    errs, err_t32, loss_d, _, flipped = _same_branch(hl, net, tr, w, B, K, dev)
    out = dict(errs=errs, err_t32=err_t32, loss=float(loss), loss_d=loss_d, flipped=flipped, grad=hl.grad_flat.clone(), prio=prio.clone(),
               running={k: v.clone() for k, v in hl.buffer_views.items()}, precisions=hl.debug_precisions())
    hl.close()
    return out


@pytest.mark.parametrize('B,K', [(2, 1), (2, 2), (3, 1), (3, 2)])
def test_split_gradients_match_float64_autograd_on_the_pass_own_branches(B, K):
    dev = torch.device('cuda', 0)
    tr, w = _fixture_batch(B, K, 40 + 10 * B + K)
    f32 = _grad_run(dev, tr, w, B, K)
    assert f32['precisions'] == (0, 0, 0)
    for tower, stage in SPLIT_COMBOS:
        r = _grad_run(dev, tr, w, B, K, tower_precision=tower, stage_precision=stage)
        assert r['precisions'] == (int(tower == 'bf16x3'), int(stage == 'bf16x3'), 0)
        assert abs(r['loss'] - r['loss_d']) <= 2e-6 * max(1.0, abs(r['loss_d'])), (tower, stage)
        _, _, flat_bar = same_branch_bar(r['errs'], r['err_t32'])
        worst = max(r['errs'], key=lambda k: r['errs'][k] / max(flat_bar, 2.0 * f32['errs'][k]))
        e, bar = r['errs'][worst], max(flat_bar, 2.0 * f32['errs'][worst])
        print(f'n{B} K{K} tower {tower} stage {stage}: worst tensor {worst} {e:.2e} bar {bar:.2e} (f32 HIP learner {f32["errs"][worst]:.2e}, flat bar {flat_bar:.2e})')
        assert e <= bar, (tower, stage, worst, e, bar, 'f32 HIP learner:', f32['errs'][worst], 'decisions float64 would have taken differently:', r['flipped'])
        assert not torch.equal(r['grad'], f32['grad'])  # (the switch really selects another arithmetic)
        if stage == 'f32':  # the forward pass before the first split layer (see the module docstring)
            early = [k for k in r['running'] if k.startswith(('represent_net.res_blocks_1.', 'represent_net.res_blocks_2.'))]
            assert len(early) == 24
            for k in early:
                assert torch.equal(r['running'][k], f32['running'][k]), k


# ------------------------------------------------------------------------------------------ 4. the reference fixture
@pytest.mark.parametrize('tower,stage', SPLIT_COMBOS)
def test_split_loss_priorities_and_three_updates_match_the_reference(tower, stage):
    """tests/test_gpu_atari_learner.py's recipe and bars on `learn_conv_atari_s` (three updates, clip on the second, an LR milestone)."""
    from test_gpu_atari_learner import REP_TOL, TIGHT, _rel

    pre = 'learn_conv_atari_s'
    dev = torch.device('cuda', 0)
    net = _atari_net(dev)
    hl = _hip(net, dev, 8, lr=1e-3, milestones=[2], gamma=0.1, max_grad_norm=10.0, tower_precision=tower, stage_precision=stage)
    tr = Transition(*[G[f'{pre}_{f}'] for f in Transition._fields])
    B = tr.state.shape[0]
    ring, w = _ring(tr, dev), torch.from_numpy(G[f'{pre}_weights']).to(dev)
    losses = []
    for step in range(3):
        loss, prio = hl.grad(ring, None, w, B)
        if step == 0:
            np.testing.assert_allclose(prio.cpu().numpy(), G[f'{pre}_prio'], rtol=1e-3, atol=1e-3)
            for pn in hl.views:
                e = _rel(hl.grad_views[pn].cpu().numpy(), G[f'{pre}_grad_{pn}'])
                assert e <= (REP_TOL if pn.split('.')[0] == 'represent_net' else TIGHT), (pn, e)
        hl.apply(clip=(step == 1))
        losses.append(float(loss))
    np.testing.assert_allclose(losses, G[f'{pre}_losses'], rtol=3e-2)
    np.testing.assert_allclose(losses[0], G[f'{pre}_losses'][0], rtol=1e-5)
    sd = net.state_dict()
    moved, bad = 1e-3 + 1e-3 + 1e-4, []
    for pn in sd:
        ref, got = G[f'{pre}_final_{pn}'], sd[pn].cpu().numpy()
        if 'num_batches_tracked' in pn:
            assert int(got) == int(ref), pn
            continue
        d = np.abs(got - ref)
        ok = float(d.max()) <= 2e-2 * max(1.0, float(np.abs(ref).max())) if 'running' in pn else float(d.max()) <= 2 * moved + 1e-6 and float(np.median(d)) <= 2e-4
        if not ok:
            bad.append((pn, float(d.max()), float(np.median(d))))
    assert not bad, bad
    assert abs(hl.current_lr() - 1e-4) < 1e-12 and hl.steps == 3
    hl.close()


# ------------------------------------------------------------------------------------------ 5. identity and determinism
def _packed3(hl):
    """The handle's split operand copies as uint32 words (mzl_debug_tensor 'packed3'), or None where it has none."""
    from muzero_amd.hip_learner import load_library

    lib = load_library()
    lib.mzl_debug_tensor.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]
    ptr, cnt = C.c_void_p(), C.c_int64()
    torch.cuda.synchronize()
    if lib.mzl_debug_tensor(hl._h, b'packed3', 0, 0, C.byref(ptr), C.byref(cnt)) != 0:
        return None
    out = np.empty(cnt.value, np.uint32)
    hip = C.CDLL('libamdhip64.so')
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), ptr, out.nbytes, 2) == 0
    return out


def _one_update(dev, tr, w, B, K, env=None, **kw):
    """(gradient, loss, priorities, weights after one update, running statistics, split copies after the update and after a fresh commit)."""
    if env:
        os.environ[env] = '1'
    try:
        hl = _hip(_atari_net(dev), dev, B, K=K, **kw)
    finally:
        if env:
            del os.environ[env]
    loss, prio = hl.grad(_ring(tr, dev), None, torch.from_numpy(w).to(dev), B)
    g, loss, prio = hl.grad_flat.clone(), loss.clone(), prio.clone()
    hl.apply()
    after_apply = _packed3(hl)
    hl.commit()
    out = (g, loss, prio, hl.params.clone(), hl.running.clone(), after_apply, _packed3(hl))
    hl.close()
    return out


NAMES = ('gradient', 'loss', 'priorities', 'weights', 'running statistics')


def test_explicit_f32_is_the_handle_that_never_called_the_setter():
    dev = torch.device('cuda', 0)
    tr, w = _fixture_batch(3, 2, 5)
    never = _one_update(dev, tr, w, 3, 2)
    named = _one_update(dev, tr, w, 3, 2, tower_precision='f32', stage_precision='f32')  # (given by name: HipLearner calls the setter with MZL_CONV_F32 twice)
    for a, b, what in zip(never, named, NAMES):
        assert torch.equal(a, b), what
    assert never[5] is None and named[5] is None  # no split copy exists on either


@pytest.mark.parametrize('tower,stage', SPLIT_COMBOS)
def test_split_update_is_bit_reproducible_and_repacks_its_copies(tower, stage):
    dev = torch.device('cuda', 0)
    tr, w = _fixture_batch(3, 2, 6)
    first = _one_update(dev, tr, w, 3, 2, tower_precision=tower, stage_precision=stage)
    for env in (None, 'MZLC_NO_PAIR'):  # a second run; the two towers of a step one job per launch
        other = _one_update(dev, tr, w, 3, 2, env=env, tower_precision=tower, stage_precision=stage)
        for a, b, what in zip(first, other, NAMES):
            assert torch.equal(a, b), (env, what)
    after_apply, fresh = first[5], first[6]
    assert after_apply is not None and after_apply.any() and np.array_equal(after_apply, fresh)  # mzl_apply repacked what mzl_commit packs
    words = {('bf16x3', 'f32'): 0, ('f32', 'bf16x3'): 1, ('bf16x3', 'bf16x3'): 2}
    sizes = []
    for t, s in sorted(words, key=words.get):
        hl = _hip(_atari_net(dev), dev, 3, K=2, tower_precision=t, stage_precision=s)
        sizes.append(len(_packed3(hl)))
        hl.close()
    assert sizes[0] + sizes[1] == sizes[2] and min(sizes) > 0  # copies exist for the split layers only


# ------------------------------------------------------------------------------------------ 6. refusals
def test_refusals():
    from muzero_amd import hip_learner as hlm

    dev = torch.device('cuda', 0)
    for kw in (dict(tower_precision='bf16x3'), dict(stage_precision='bf16x3')):
        with pytest.raises(hlm.LearnerError, match='mzl_set_atari_precision.*MZL_NET_ATARI.*conv_precision'):
            _hip(build_conv(conv_case('board3')).to(dev), dev, 4, **kw)
        with pytest.raises(hlm.LearnerError, match='mzl_set_atari_precision.*MZL_NET_ATARI'):
            _hip(build_mlp(mlp_case('tiny')).to(dev), dev, 4, **kw)
    with pytest.raises(ValueError, match='tower_precision'):
        _hip(_atari_net(dev), dev, 2, tower_precision=2)
    # the refusals from before this switch stay, with their messages (mzl_create's own check answers before the conv learner's)
    with pytest.raises(hlm.LearnerError, match='conv_precision MZL_CONV_BF16X3 needs net_kind MZL_NET_BOARD: the tap-set, tile and plane convs of MZL_NET_ATARI have no split-bf16 build'):
        _hip(_atari_net(dev), dev, 2, conv_precision='bf16x3')
    with pytest.raises(hlm.LearnerError, match='wgrad_precision: MZL_NET_ATARI has no split-bf16 weight gradient'):
        _hip(_atari_net(dev), dev, 2, wgrad_precision='bf16x3')
    # the ABI itself: unknown values, a bound handle, a null handle; a refusal leaves the handle as it was
    lib = hlm.load_library()
    hl = _hip(_atari_net(dev), dev, 2, K=1, tower_precision='bf16x3')
    assert hl.debug_precisions() == (1, 0, 0)
    for t, s in ((2, 0), (0, -1), (1, 7)):
        assert lib.mzl_set_atari_precision(hl._h, t, s) == -1 and 'tower_precision and stage_precision' in lib.mzl_last_error().decode()
    assert lib.mzl_set_atari_precision(hl._h, 0, 1) == -3 and 'mzl_bind' in lib.mzl_last_error().decode()
    assert lib.mzl_set_atari_precision(hl._h, 0, 0) == -3
    assert lib.mzl_set_atari_precision(None, 1, 1) == -1
    assert hl.debug_precisions() == (1, 0, 0)
    board = _hip(build_conv(conv_case('board3')).to(dev), dev, 4)
    assert lib.mzl_set_atari_precision(board._h, 0, 0) == -1 and 'conv_precision' in lib.mzl_last_error().decode()  # (bound or not: a board handle is refused)
    # the hooks: mzl_debug_conv keeps refusing Atari handles, the tile hook refuses board handles and validates its arguments
    with pytest.raises(hlm.LearnerError, match='mzl_debug_conv: board nets only'):
        hl.debug_conv(0, np.zeros((4, 4, 3, 3), np.float32), np.zeros((1, 4, 3, 3), np.float32))
    ok_w, ok_x = np.zeros((16, 16, 3, 3), np.float32), np.zeros((1, 16, 24, 24), np.float32)
    with pytest.raises(hlm.LearnerError, match='mzl_debug_conv_tile: Atari nets only'):
        board.debug_conv_tile(0, ok_w, ok_x)
    hl.debug_conv_tile(0, ok_w, ok_x)
    for direction, x, kw in ((2, ok_x, {}), (0, np.zeros((1, 16, 20, 24), np.float32), {}), (0, np.zeros((1, 16, 24, 40), np.float32), {}),
                             (0, ok_x, dict(mask=ok_x)), (0, ok_x, dict(skip=ok_x, want_part=True)), (0, ok_x, dict(mask=ok_x, partner=ok_x, route='inner'))):
        with pytest.raises(hlm.LearnerError, match='mzl_debug_conv_tile'):
            hl.debug_conv_tile(direction, ok_w, x, **kw)
    hl.close()
    board.close()
