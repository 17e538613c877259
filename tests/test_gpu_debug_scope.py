"""The diagnostic hooks leave the handle as they found it -- also when they refuse.

Every mzl_debug_* hook that flips a switch of the handle (halo_in, out_plane, xcd_remap, act_sparse, ring_rows, row_steps, quad_steps, bad_dispatch) does
so inside one scope object (csrc/mz_learn_conv_debug.h, DebugCall) whose destructor puts ALL of them back, whichever way the hook returns.  Here: one
update's gradient from fixed parameters and a fixed batch, then hook calls with non-default switches -- accepted ones and one that an argument check
refuses AFTER the switches were set -- then the same update again: the same bits, the same precisions, and the switches a hook's build name reports
(ring_rows, remap, the action route) as before.  The smallest handles of the other hook tests, batch 2."""
import re

import numpy as np
import pytest
import torch

from helpers import build_conv, conv_case
from muzero_amd.replay import Transition

pytestmark = pytest.mark.gpu
B = 2
# mzlc_debug_conv_tile's refusal of a width that is no whole number of 12-column tiles: it fires after the call set halo_in / out_plane / bad_dispatch
NOT_TILED = 'bad shape: W must divide into tiles of 12 columns (or 16: widths that are a multiple of 16 and at least 48)'


def _learner(name, K, max_batch):
    from muzero_amd.hip_learner import HipLearner

    dev = torch.device('cuda', 0)
    net = build_conv(conv_case(name)).to(dev)
    net.train()
    return HipLearner(net, dev, K, max_batch, lr=1e-3)


def _ring(name, K, seed):
    _, _, shape, A = conv_case(name)[:4]
    rs = np.random.RandomState(seed)
    tr = Transition(rs.uniform(0, 1, (B,) + shape).astype(np.float32), rs.randint(0, A, (B, K)).astype(np.int8), rs.dirichlet(np.ones(A), size=(B, K)).astype(np.float32),
                    rs.uniform(-1, 1, (B, K)).astype(np.float32), rs.uniform(-1, 1, (B, K)).astype(np.float32))
    dev = torch.device('cuda', 0)
    return dict(state=torch.from_numpy(tr.state).to(dev).reshape(B, -1).contiguous(), action=torch.from_numpy(tr.action).to(dev), pi_prob=torch.from_numpy(tr.pi_prob).to(dev),
                value=torch.from_numpy(tr.value).to(dev), reward=torch.from_numpy(tr.reward).to(dev))


def _update(hl, ring):
    loss, prio = hl.grad(ring, None, None, B)
    torch.cuda.synchronize()
    return hl.grad_flat.clone(), loss.clone(), prio.clone()


def _switches(name):
    """What a mzl_debug_wgrad build name says of the handle's switches (a call without overrides runs what the update would)."""
    return {k: v for k, v in re.findall(r'(\w+)=(\S+)', name) if k in ('ring_rows', 'nsteps', 'remap', 'act')}


def _z(*shape):
    return np.zeros(shape, np.float32)


def test_atari_hooks_leave_the_handle_as_they_found_it():
    from muzero_amd.hip_learner import LearnerError

    hl = _learner('atari_s', 1, 2)  # (tests/test_gpu_atari_stage.py's handle)
    try:
        ring = _ring('atari_s', 1, 5)
        g0, l0, p0 = _update(hl, ring)
        assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
        prec = hl.debug_precisions()
        tile = dict(dz=_z(8, 16, 14, 14), x=_z(8, 4, 14, 14), ipw=1)  # (8 chunks: a group count the XCD remap takes, so the name shows the switch)
        probe = _switches(hl.debug_wgrad(mode='ring', **tile)[1])
        assert probe['ring_rows'] != '0' and probe['remap'] == '1', probe  # (the handle's defaults, which the calls below switch off)

        w, x = np.ones((8, 4, 3, 3), np.float32), np.ones((B, 4, 12, 24), np.float32)
        for route, halo, plane in (('whole', 0, 0), ('inner', 1, 0)):  # halo_in / out_plane off | out_plane off
            out, name = hl.debug_conv_tile(0, w, x, route=route)
            assert f' HALO={halo} PLANE={plane} ' in name and not np.isnan(out).any(), name
        _, name = hl.debug_wgrad(mode='ring', ring_rows=0, remap=2, **tile)  # ring_rows / row_steps / quad_steps off, xcd_remap off
        assert ' ring_rows=0 ' in name and ' remap=0 ' in name, name
        for route in ('whole', 'inner', 'plane'):  # refused after the call set its switches: H = 12, W = 20
            with pytest.raises(LearnerError, match=re.escape(NOT_TILED)):
                hl.debug_conv_tile(0, w, np.ones((B, 4, 12, 20), np.float32), route=route)

        assert _switches(hl.debug_wgrad(mode='ring', **tile)[1]) == probe
        assert hl.debug_precisions() == prec
        g1, l1, p1 = _update(hl, ring)
        assert torch.equal(g0, g1) and torch.equal(l0, l1) and torch.equal(p0, p1), 'the update after the hook calls differs from the same update before them'
    finally:
        hl.close()


def test_a_hook_builds_its_geometry_from_the_switches_the_handle_was_created_under():
    """MZLC_DENSE_TILING is read once, at create, into the handle: a hook called after the variable is gone tiles as that handle does.  5 x 5 images
    (25 pixels, 7 pixel quads), batch 8, a 16-channel layer -- two workgroups per image group, paired -- on more than 6 CUs.  By launch time (make_geom's
    cost: rounds of workgroups over the CUs x tiles per workgroup; every tiling is one round here) the smallest tiling wins: NPT 5, 3 images in 80
    slots.  By density: NPT 13, 8 images in 208 slots (200 / 208 against 75 / 80, 75 / 96, 125 / 144 and 225 / 240).  The first pair is the
    precondition that checks this arithmetic; a library that asked the environment again at the call would give it for both handles."""
    import os

    from muzero_amd.hip_learner import HipLearner

    dev = torch.device('cuda', 0)
    case = ('board5x16', 'board', (5, 5, 5), 26, 1, 16, 1, 1, 23)  # (CONV_CASES' layout: 5 x 5 board, one block, 16 planes)

    def learner(env=None):  # (the variable is gone again when the constructor has returned)
        net = build_conv(case).to(dev)
        net.train()
        if env:
            assert env not in os.environ
            os.environ[env] = '1'
        try:
            return HipLearner(net, dev, 1, 8, lr=1e-3)
        finally:
            if env:
                del os.environ[env]

    rs = np.random.RandomState(7)
    job = dict(weight=rs.randn(16, 16, 3, 3).astype(np.float32), in0=rs.randn(8, 16, 5, 5).astype(np.float32))
    plain, dense = learner(), learner('MZLC_DENSE_TILING')
    try:
        assert 'MZLC_DENSE_TILING' not in os.environ
        out_p, name_p = plain.debug_conv_fused(job)
        out_d, name_d = dense.debug_conv_fused(job)
        assert ' NPT=5 ' in name_p and ' G=3 ' in name_p, name_p
        assert ' NPT=13 ' in name_d and ' G=8 ' in name_d, name_d
        assert float(np.abs(out_p['out']).max()) > 0
        assert np.array_equal(out_p['out'], out_d['out']), 'a conv output depends on the pixel tiling'  # (the summation order is per output element)
    finally:
        plain.close()
        dense.close()


def test_board_hooks_leave_the_handle_as_they_found_it():
    from muzero_amd.hip_learner import LearnerError

    hl = _learner('board3', 5, 4)  # (tests/test_gpu_conv_fused.py's handle)
    try:
        ring = _ring('board3', 5, 6)
        g0, l0, p0 = _update(hl, ring)
        assert bool(torch.isfinite(g0).all()) and float(g0.abs().max()) > 0
        prec = hl.debug_precisions()
        # 82 action planes behind 32 real channels (six extra channel tiles: the sparse route by the update's rule), 8 chunks (the XCD remap takes them)
        layer = dict(dz=_z(8, 32, 9, 9), x=_z(8, 32, 9, 9), action=np.arange(8, dtype=np.int32) * 11, num_actions=82, cin=114, sg=1, ipw=1)
        probe = _switches(hl.debug_wgrad(**layer)[1])
        assert probe['act'] == 'sparse' and probe['remap'] == '1', probe  # (the handle's defaults, which the call below switches off)

        _, name = hl.debug_wgrad(act_route=1, remap=2, **layer)  # the action planes inside the MFMA kernel, xcd_remap off
        assert ' act=kernel ' in name and ' remap=0 ' in name, name
        with pytest.raises(LearnerError, match='Atari nets only'):  # (the tile hook refuses a board handle before it touches anything)
            hl.debug_conv_tile(0, np.ones((8, 4, 3, 3), np.float32), np.ones((B, 4, 12, 20), np.float32), route='whole')

        assert _switches(hl.debug_wgrad(**layer)[1]) == probe
        assert hl.debug_precisions() == prec
        g1, l1, p1 = _update(hl, ring)
        assert torch.equal(g0, g1) and torch.equal(l0, l1) and torch.equal(p0, p1), 'the update after the hook calls differs from the same update before them'
    finally:
        hl.close()
