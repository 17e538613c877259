"""ctypes binding of libmzlearner_hip.so (C ABI: include/mzlearner.h) and `HipLearner`, the learner step of the MLP nets and -- round 5 --
of the board-game conv nets (`MuZeroBoardGameNet`: residual towers with train-mode BatchNorm) on hand-written gfx950 kernels (SURVEY 8 f2:
`calc_loss` pipeline.py:541-612 + backward + clip + Adam / MultiStepLR :238-255).

`HipLearner` owns ONE flat float32 device tensor holding master weights, gradient, exp_avg and exp_avg_sq; the network's
parameters are views into it (so `network.state_dict()` / checkpoints keep the reference's layout, pipeline.py:224-230), and
the kernels read sampled items straight out of the HBM replay ring by row index.  There is no PyTorch autograd and no ATen
kernel on the step; torch is the allocator, the stream and -- for a data-parallel learner -- the RCCL all-reduce of the flat
gradient between `grad()` and `apply()`.  No CPU fallback: without the library or a GPU the constructor raises."""
import ctypes as C
import os
from typing import Optional, Sequence

import numpy as np
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libmzlearner_hip.so')

# every symbol include/mzlearner.h declares (tests/test_abi.py checks the library exports all of them)
ABI_SYMBOLS = ['mzl_last_error', 'mzl_create', 'mzl_destroy', 'mzl_set_wgrad_precision', 'mzl_set_atari_precision', 'mzl_num_params', 'mzl_grad_floats', 'mzl_num_tensors', 'mzl_tensor_info',
               'mzl_num_buffers', 'mzl_num_running', 'mzl_buffer_info', 'mzl_bind_buffers', 'mzl_bind', 'mzl_commit', 'mzl_grad', 'mzl_apply',
               'mzl_replay_scratch_doubles', 'mzl_replay_sample', 'mzl_replay_update_priorities', 'mzl_replay_set_error_counters']
NET_MLP, NET_BOARD, NET_ATARI = 0, 1, 2
CONV_PRECISIONS = {'f32': 0, 'bf16x3': 1}  # MZL_CONV_F32 / MZL_CONV_BF16X3 (include/mzlearner.h)
WGRAD_PRECISIONS = {'f32': 0, 'bf16x3': 1}  # MZL_WGRAD_F32 / MZL_WGRAD_BF16X3


class LearnerError(RuntimeError):
    pass


def _conv_precision(v):
    if isinstance(v, str) and v in CONV_PRECISIONS:
        return CONV_PRECISIONS[v]
    if not isinstance(v, (str, bool)) and v in (0, 1):
        return int(v)
    raise ValueError(f"conv_precision must be 0, 1, 'f32' or 'bf16x3', not {v!r}")


def _wgrad_precision(v):
    if isinstance(v, str) and v in WGRAD_PRECISIONS:
        return WGRAD_PRECISIONS[v]
    if not isinstance(v, (str, bool)) and v in (0, 1):
        return int(v)
    raise ValueError(f"wgrad_precision must be 0, 1, 'f32' or 'bf16x3', not {v!r}")


def _atari_precision(v, which):
    """tower_precision / stage_precision of an Atari handle (mzl_set_atari_precision): MZL_CONV_F32 / MZL_CONV_BF16X3."""
    if isinstance(v, str) and v in CONV_PRECISIONS:
        return CONV_PRECISIONS[v]
    if not isinstance(v, (str, bool)) and v in (0, 1):
        return int(v)
    raise ValueError(f"{which} must be 0, 1, 'f32' or 'bf16x3', not {v!r}")


class MzlConfig(C.Structure):
    _fields_ = [('in_dim', C.c_int32), ('num_actions', C.c_int32), ('num_planes', C.c_int32), ('hidden_dim', C.c_int32),
                ('value_support_size', C.c_int32), ('reward_support_size', C.c_int32), ('unroll_steps', C.c_int32), ('max_batch', C.c_int32),
                ('grad_slices', C.c_int32), ('net_kind', C.c_int32), ('in_channels', C.c_int32), ('board_h', C.c_int32), ('board_w', C.c_int32),
                ('num_res_blocks', C.c_int32), ('conv_precision', C.c_int32)]


class MzlReplayDraw(C.Structure):
    _fields_ = [('d_priority', C.c_void_p), ('d_num_added', C.c_void_p), ('capacity', C.c_int64), ('priority_exponent', C.c_double),
                ('importance_sampling_exponent', C.c_double), ('seed', C.c_uint64), ('draw', C.c_uint64), ('batch', C.c_int32), ('d_index', C.c_void_p),
                ('d_weights', C.c_void_p), ('d_scratch', C.c_void_p)]


class MzlBatch(C.Structure):
    _fields_ = [('d_state', C.c_void_p), ('d_action', C.c_void_p), ('d_pi_prob', C.c_void_p), ('d_value', C.c_void_p), ('d_reward', C.c_void_p),
                ('d_index', C.c_void_p), ('d_weights', C.c_void_p), ('d_loss', C.c_void_p), ('d_priorities', C.c_void_p), ('batch', C.c_int32),
                ('state_is_int8', C.c_int32), ('action_bytes', C.c_int32),
                ('state_row_bytes', C.c_int32), ('frame_stack', C.c_int32), ('frame_channels', C.c_int32)]


_lib = None


class MzlWgradLayer(C.Structure):
    """mzl_wgrad_layer (csrc/mz_learn_conv_host.h): one layer's host operands of mzl_debug_wgrad."""
    _fields_ = [(n, C.c_void_p) for n in ('dz', 'x', 'y', 'dcoef', 'xcoef', 'action', 'preload', 'out')] + \
               [(n, C.c_int32) for n in ('cin_real', 'cin', 'cout', 'pad_')]


class MzlWgradCall(C.Structure):
    """mzl_wgrad_call (csrc/mz_learn_conv_host.h)."""
    _fields_ = [(n, C.c_int32) for n in ('mode', 'batch', 'h', 'w', 'num_actions', 'nsrc', 'accumulate', 'sg', 'layout', 'ipw', 'remap', 'act_route',
                                         'ring_rows', 'tapmask')] + [('layer', MzlWgradLayer * 2)]


class MzlTileCall(C.Structure):
    """mzl_tile_call (csrc/mz_learn_conv_host.h): the host operands of mzl_debug_conv_tile."""
    _fields_ = [(n, C.c_int32) for n in ('direction', 'precision', 'route', 'batch', 'cin', 'cout', 'H', 'W', 'groups', 'pad_')] + \
               [(n, C.c_void_p) for n in ('weight', 'in_', 'skip', 'mask', 'mcoef', 'partner', 'out', 'part')]


class MzlStageCall(C.Structure):
    """mzl_stage_call (csrc/mz_learn_conv_host.h): the host operands of mzl_debug_atari_stage."""
    _fields_ = [(n, C.c_int32) for n in ('op', 'batch', 'cin', 'cout', 'H', 'W', 'mode', 'stride', 'py', 'px', 'inner_only', 'src_inner', 'want_stats', 'launcher',
                                         'groups')] + [('scale', C.c_float)] + \
               [(n, C.c_void_p) for n in ('weight', 'in0', 'in1', 'in2', 'in3', 'coef', 'out', 'stats')]


STAGE_OPS = {'s2_fwd': 0, 's2_dgrad': 1, 'pool_fwd': 2, 'pool_bwd': 3, 'relu_bwd': 4, 'entry': 5, 'normalize': 6, 'gather': 7, 'scatter': 8}
ENTRY_LAUNCHERS = {'atari': 0, 'tower': 1, 'rep12': 2}
TILE_ROUTES = {'plane': 0, 'inner': 1, 'whole': 2}
WGRAD_MODES = {'plain': 0, 'pair': 1, 'steps': 2, 'ring': 3}

_FUSED_IN = ('weight', 'in0', 'in1', 'coef', 'mat_preload', 'skip', 'mask', 'mcoef', 'partner', 'gamma', 'beta', 'save_in', 'part_in')
_FUSED_OUT = ('out', 'mat_out', 'part', 'coef_out', 'save_out', 'running_mean', 'running_var', 'dgamma', 'dbeta', 'num_batches')


class MzlFusedConv(C.Structure):
    """mzl_fused_conv (csrc/mz_learn_conv_host.h): one job's host operands of mzl_debug_conv_fused."""
    _fields_ = [(n, C.c_void_p) for n in _FUSED_IN + _FUSED_OUT] + \
               [(n, C.c_int32) for n in ('direction', 'in_mode', 'stat_mode', 'finalize', 'accumulate', 'partner_is_mask', 'cin', 'cout')]


class MzlFusedCall(C.Structure):
    """mzl_fused_call (csrc/mz_learn_conv_host.h)."""
    _fields_ = [(n, C.c_int32) for n in ('mode', 'batch', 'h', 'w', 'groups', 'no_side')] + [('count', C.c_float), ('pad_', C.c_int32), ('conv', MzlFusedConv * 2)]


_HEADS_IN = ('F_pred', 'F_rew', 'params', 'running', 'nbt', 'pi', 'value', 'reward', 'idx', 'w')
_HEADS_OUT = ('u', 'spart_fwd', 'spiv', 'coef', 'save', 'feat', 'dlogit', 'dzb', 'spart_bwd', 'lpart', 'loss', 'prio', 'running_out', 'nbt_out', 'dF_pred', 'dF_rew',
              'wpart', 'grads')


class MzlHeadsCall(C.Structure):
    """mzl_heads_call (csrc/mz_learn_conv_host.h): the host operands of mzl_debug_heads."""
    _fields_ = [('batch', C.c_int32), ('rows', C.c_int32)] + [(n, C.c_void_p) for n in _HEADS_IN + _HEADS_OUT]


FUSED_MODES = {'conv': 0, 'pair': 1, 'finalize': 2, 'apply': 3}
IN_MODES = {'ident': 0, 'bnrelu': 1, 'bnbwd': 2, 'bnres': 3}
STAT_MODES = {None: 0, 'none': 0, 'fwd': 1, 'bwd': 2}


def load_library():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LearnerError(f'{LIB_PATH} not found: build it with `python -m muzero_amd.build` (hipcc, gfx950). The HIP learner has no CPU fallback.')
    L = C.CDLL(LIB_PATH)
    vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
    L.mzl_last_error.restype = C.c_char_p
    L.mzl_create.argtypes = [C.POINTER(MzlConfig), C.c_int, C.POINTER(vp)]
    L.mzl_destroy.argtypes = [vp]
    if hasattr(L, 'mzl_set_wgrad_precision'):  # (an older library loaded for an A/B run, tools/*_vs_parent.py, has none; wgrad_precision != 0 then fails at the call)
        L.mzl_set_wgrad_precision.argtypes = [vp, i32]
    if hasattr(L, 'mzl_set_atari_precision'):  # (the same: the parent commit's library has none)
        L.mzl_set_atari_precision.argtypes = [vp, i32, i32]
    L.mzl_num_params.argtypes = [vp]
    L.mzl_num_params.restype = i64
    L.mzl_grad_floats.argtypes = [vp]
    L.mzl_grad_floats.restype = i64
    L.mzl_tensor_info.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(i64), C.POINTER(i32), C.POINTER(i32)]
    L.mzl_num_tensors.argtypes = [vp]
    L.mzl_num_tensors.restype = i32
    L.mzl_num_buffers.argtypes = [vp]
    L.mzl_num_buffers.restype = i32
    L.mzl_num_running.argtypes = [vp]
    L.mzl_num_running.restype = i64
    L.mzl_buffer_info.argtypes = [vp, i32, C.POINTER(C.c_char_p), C.POINTER(i64), C.POINTER(i32)]
    L.mzl_bind_buffers.argtypes = [vp, vp, vp]
    L.mzl_bind.argtypes = [vp, vp, vp, vp, vp]
    L.mzl_commit.argtypes = [vp, vp]
    L.mzl_grad.argtypes = [vp, C.POINTER(MzlBatch), vp]
    L.mzl_apply.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, i64, vp]
    L.mzl_replay_scratch_doubles.argtypes = [i64]
    L.mzl_replay_scratch_doubles.restype = i64
    L.mzl_replay_sample.argtypes = [C.POINTER(MzlReplayDraw), vp]
    L.mzl_replay_update_priorities.argtypes = [vp, i64, vp, vp, i32, vp, vp]
    L.mzl_replay_set_error_counters.argtypes = [vp]
    if hasattr(L, 'mzl_debug_conv'):  # (tools/split_learner_bench.py also loads the parent commit's library, which has no hook)
        L.mzl_debug_conv.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp, C.POINTER(C.c_char_p)]  # diagnostic: exported, not declared
    if hasattr(L, 'mzl_debug_wgrad'):
        L.mzl_debug_wgrad.argtypes = [vp, C.POINTER(MzlWgradCall), C.POINTER(C.c_char_p)]  # diagnostic: exported, not declared
    if hasattr(L, 'mzl_debug_conv_fused'):
        L.mzl_debug_conv_fused.argtypes = [vp, C.POINTER(MzlFusedCall), C.POINTER(C.c_char_p)]  # diagnostic: exported, not declared
    if hasattr(L, 'mzl_debug_conv_tile'):
        L.mzl_debug_conv_tile.argtypes = [vp, C.POINTER(MzlTileCall), C.POINTER(C.c_char_p)]  # diagnostic: exported, not declared
        L.mzl_debug_precisions.argtypes = [vp, C.POINTER(i32)]
    if hasattr(L, 'mzl_debug_atari_stage'):
        L.mzl_debug_atari_stage.argtypes = [vp, C.POINTER(MzlStageCall), C.POINTER(C.c_char_p)]  # diagnostic: exported, not declared
    if hasattr(L, 'mzl_debug_heads'):
        L.mzl_debug_heads.argtypes = [vp, C.POINTER(MzlHeadsCall)]  # diagnostic: exported, not declared
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise LearnerError(f'libmzlearner_hip: {load_library().mzl_last_error().decode()} (status {rc})')


class _OptimizerView:
    """What `run_training` (pipeline.py:170-286) holds as `optimizer`: the checkpoint's 'optimizer' entry in torch.optim.Adam's format."""

    def __init__(self, hl):
        self.hip_learner = hl

    def state_dict(self):
        return self.hip_learner.optimizer_state_dict()

    def load_state_dict(self, sd):
        self.hip_learner.load_optimizer_state_dict(sd)

    @property
    def param_groups(self):
        return self.hip_learner.optimizer_state_dict()['param_groups']


class _SchedulerView:
    """... and as `lr_scheduler` (MultiStepLR): state for the checkpoint, `get_last_lr` for the metrics."""

    def __init__(self, hl):
        self.hip_learner = hl

    def state_dict(self):
        return self.hip_learner.lr_scheduler_state_dict()

    def load_state_dict(self, sd):
        self.hip_learner.steps = int(sd.get('last_epoch', self.hip_learner.steps))

    def get_last_lr(self):
        return [self.hip_learner.current_lr()]

    def step(self):  # (the schedule advances inside HipLearner.apply)
        pass


def conv_learner_flops(input_shape, num_actions: int, num_res_blocks: int, num_planes: int, unroll_steps: int) -> float:
    """Algorithmic FLOPs (2 x multiply-accumulate) of ONE sample's update of a MuZeroBoardGameNet: forward + weight gradient of every 3 x 3
    conv of the K-step unroll (pipeline.py:575-592; the dynamics net's first conv over its num_planes + num_actions inputs, network.py:440-446)
    + data gradient wherever an input needs one (not the observation, not the constant action planes).  Heads and elementwise work are not
    counted (< 0.1 %)."""
    c0, h, w = input_shape
    P, A, R, K, hw = num_planes, num_actions, num_res_blocks, unroll_steps, h * w
    tower = 2 * R * P * P * 9 * hw
    fwd = (c0 * P * 9 * hw + tower) + K * ((P + A) * P * 9 * hw + tower) + K * tower
    dgrad = tower + K * (P * P * 9 * hw + tower) + K * tower
    return 2.0 * (2 * fwd + dgrad)


def atari_learner_flops(input_shape, num_actions: int, num_res_blocks: int, num_planes: int, unroll_steps: int) -> float:
    """conv_learner_flops for a MuZeroAtariNet (network.py:312-353 of the reference: conv_1 (stride 2) -> two 128-plane blocks at 48 x 48 ->
    conv_2 (stride 2) -> two blocks at 24 x 24 -> pool -> two blocks at 12 x 12 -> pool; dynamics / prediction towers on 6 x 6).  Algorithmic:
    the 14 x 14 halo tiles the kernels actually convolve (1.36 x the positions of the two large stages) are not counted."""
    c0, h, w = input_shape
    P, A, R, K = num_planes, num_actions, num_res_blocks, unroll_steps
    s1, s2, s3, s4 = (h // 2) * (w // 2), (h // 4) * (w // 4), (h // 8) * (w // 8), (h // 16) * (w // 16)
    rep_first = c0 * 128 * 9 * s1  # forward + weight gradient only
    rep_rest = 4 * 128 * 128 * 9 * s1 + 128 * P * 9 * s2 + 4 * P * P * 9 * s2 + 4 * P * P * 9 * s3
    tower = 2 * R * P * P * 9 * s4
    fwd = rep_first + rep_rest + K * ((P + A) * P * 9 * s4 + tower) + K * tower
    dgrad = rep_rest + K * (P * P * 9 * s4 + tower) + K * tower
    return 2.0 * (2 * fwd + dgrad)


class HipLearner:
    """The learner step of `run_training` (pipeline.py:238-255) for a `MuZeroMLPNet`, a `MuZeroBoardGameNet` or a `MuZeroAtariNet` on the GPU, as HIP kernels.
    (Conv nets: the BatchNorm layers run in TRAIN mode whatever `network.training` says -- a learner step is a training step -- and their
    running statistics, `num_batches_tracked` included, are module buffers re-pointed at the learner's flat buffer vectors.)

    `network`'s parameters are re-pointed at views of the learner's flat weight vector: after every `apply()` the module holds the
    new weights (its `state_dict()` is the checkpoint's 'network' entry as before).  Adam / MultiStepLR follow torch's definitions
    (`torch.optim.Adam(lr, weight_decay)` with L2-in-gradient, `MultiStepLR(milestones, gamma)`): `optimizer_state_dict()` returns
    what `torch.optim.Adam.state_dict()` would."""

    def __init__(self, network, device, unroll_steps: int, max_batch: int, lr: float, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 milestones: Sequence[int] = (), gamma: float = 0.1, clip_grad: bool = False, max_grad_norm: float = 40.0, grad_slices: Optional[int] = None,
                 conv_precision=0, wgrad_precision=0, tower_precision=0, stage_precision=0):
        """conv_precision: 'f32' (0, the default) or 'bf16x3' (1): board nets only -- the towers' forward and data-gradient convs as split-bf16
        MFMAs (csrc/mz_learn_conv_split.h).  wgrad_precision: 'f32' (0, the default) or 'bf16x3' (1): board nets only, independent of
        conv_precision -- the towers' weight gradients as split-bf16 MFMAs (csrc/mz_learn_conv_split_wgrad.h).  tower_precision / stage_precision:
        'f32' (0, the default) or 'bf16x3' (1), Atari nets only (mzl_set_atari_precision), independent of each other: the forward convs and data
        gradients of the whole-image towers (res_blocks_3, dynamics, prediction) / of the tile path's stride-1 convs (res_blocks_1, res_blocks_2) as
        split-bf16 MFMAs.  BatchNorm, heads and Adam stay float32 either way."""
        self._h = C.c_void_p()
        self.conv_precision = _conv_precision(conv_precision)
        self.wgrad_precision = _wgrad_precision(wgrad_precision)
        self.tower_precision = _atari_precision(tower_precision, 'tower_precision')
        self.stage_precision = _atari_precision(stage_precision, 'stage_precision')
        if not torch.cuda.is_available():
            raise LearnerError('HipLearner needs a GPU (no CPU fallback)')
        L = load_library()
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device() if torch.cuda.is_available() else 0)
        spec = network.planner_spec()
        if spec['kind'] not in ('mlp', 'board', 'atari'):
            raise LearnerError(f"HipLearner covers MuZeroMLPNet, MuZeroBoardGameNet and MuZeroAtariNet, not {spec['kind']!r}")
        self.kind = spec['kind']
        tiles = (max_batch + 15) // 16
        if self.kind in ('board', 'atari'):
            grad_slices = 1
        if grad_slices is None:
            # long reductions (large batches): the weight-gradient kernel runs one 8-wave workgroup per (layer, slice) -- 8 unrolled layers
            # with grad_slices slices each, 2 representation layers with grad_slices / K -- and all of them should be resident at once
            cus = torch.cuda.get_device_properties(device).multi_processor_count if torch.cuda.is_available() else 256
            grad_slices = 1 if tiles * unroll_steps < 256 else max(2, min(64, int(cus / (8.0 + 2.0 / unroll_steps)), tiles * unroll_steps // 8))
        in_dim = int(np.prod(spec['input_shape']))
        if self.kind in ('board', 'atari'):
            c0, bh, bw = spec['input_shape']
            cfg = MzlConfig(in_dim, spec['num_actions'], spec['num_planes'], 1, spec['value_support_size'], spec['reward_support_size'], unroll_steps, max_batch, 1,
                            NET_BOARD if self.kind == 'board' else NET_ATARI, c0, bh, bw, spec['num_res_blocks'], self.conv_precision)
        else:
            cfg = MzlConfig(in_dim, spec['num_actions'], spec['num_planes'], spec['hidden_dim'], spec['value_support_size'], spec['reward_support_size'],
                            unroll_steps, max_batch, grad_slices, NET_MLP, 0, 0, 0, 0, self.conv_precision)
        _check(L.mzl_create(C.byref(cfg), self.device.index or 0, C.byref(self._h)))
        self._wide_tiles = 'MZLC_NO_WIDE_TILES' not in os.environ  # (read by the library at create; debug_atari_stage sizes its tile arrays by it)
        if self.wgrad_precision:  # (the default never calls the setter: the handle is what mzl_create made)
            _check(L.mzl_set_wgrad_precision(self._h, self.wgrad_precision))
        # (the same: the default, 0, leaves the handle as mzl_create made it; a value given by NAME on an Atari net is passed on even when it is
        # 'f32' -- the setter called with MZL_CONV_F32 twice is the same update bit for bit, and tests/test_gpu_split_atari_learner.py holds it to that)
        named = self.kind == 'atari' and (isinstance(tower_precision, str) or isinstance(stage_precision, str))
        if self.tower_precision or self.stage_precision or named:
            _check(L.mzl_set_atari_precision(self._h, self.tower_precision, self.stage_precision))
        self.K, self.A, self.in_dim, self.max_batch = unroll_steps, spec['num_actions'], in_dim, max_batch
        if self.kind in ('board', 'atari'):  # (debug_heads: planes, positions of the hidden state, reward / value support)
            self._heads_geom = (spec['num_planes'], bh * bw if self.kind == 'board' else (bh // 16) * (bw // 16), spec['reward_support_size'], spec['value_support_size'])
        self.total = int(L.mzl_num_params(self._h))
        gfl = int(L.mzl_grad_floats(self._h))
        self.flat = torch.zeros(3 * self.total + gfl, dtype=torch.float32, device=self.device)
        self.params, self.exp_avg, self.exp_avg_sq = (self.flat[i * self.total:(i + 1) * self.total] for i in range(3))
        self.grads = self.flat[3 * self.total:]
        self.grad_flat = self.grads[:self.total]  # the complete gradient after grad() (slice 0)
        self.views, self.grad_views = {}, {}
        module_shapes = {k: tuple(p.shape) for k, p in network.named_parameters()}
        for i in range(int(L.mzl_num_tensors(self._h))):
            name, off, rows, cols = C.c_char_p(), C.c_int64(), C.c_int32(), C.c_int32()
            _check(L.mzl_tensor_info(self._h, i, C.byref(name), C.byref(off), C.byref(rows), C.byref(cols)))
            key = name.value.decode()
            n = rows.value * (cols.value if cols.value else 1)
            shape = module_shapes.get(key, (rows.value, cols.value) if cols.value else (rows.value,))  # (conv weights: [cout, cin, 3, 3] / [oc, P, 1, 1])
            if int(np.prod(shape)) != n:
                raise LearnerError(f'{key}: the module holds {shape}, the learner {n} elements')
            self.views[key] = self.params[off.value:off.value + n].view(shape)
            self.grad_views[key] = self.grad_flat[off.value:off.value + n].view(shape)
        _check(L.mzl_bind(self._h, self.params.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()))
        # BatchNorm buffers (conv nets): flat running statistics + one num_batches_tracked per layer, written by the kernels
        self.buffer_views = {}
        nbuf = int(L.mzl_num_buffers(self._h))
        self.running = torch.zeros(max(1, int(L.mzl_num_running(self._h))), dtype=torch.float32, device=self.device)
        self.num_batches = torch.zeros(max(1, nbuf), dtype=torch.int64, device=self.device)
        for i in range(nbuf):
            name, off, cnt = C.c_char_p(), C.c_int64(), C.c_int32()
            _check(L.mzl_buffer_info(self._h, i, C.byref(name), C.byref(off), C.byref(cnt)))
            key, o, c = name.value.decode(), off.value, cnt.value
            self.buffer_views[key + '.running_mean'] = self.running[o:o + c]
            self.buffer_views[key + '.running_var'] = self.running[o + c:o + 2 * c]
            self.buffer_views[key + '.num_batches_tracked'] = self.num_batches[i]
        if nbuf:
            _check(L.mzl_bind_buffers(self._h, self.running.data_ptr(), self.num_batches.data_ptr()))
        self.lr_init, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), tuple(betas), float(eps)
        self.milestones, self.gamma = sorted(int(m) for m in milestones), float(gamma)
        self.clip_grad, self.max_grad_norm = bool(clip_grad), float(max_grad_norm)
        self.steps = 0
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.priorities = torch.zeros(max_batch, dtype=torch.float32, device=self.device)
        self._ones = torch.ones(max_batch, dtype=torch.float32, device=self.device)
        self._iota = torch.arange(max_batch, dtype=torch.int64, device=self.device)
        self.network = network
        self.optimizer, self.lr_scheduler = _OptimizerView(self), _SchedulerView(self)
        self.adopt(network)

    # ---- weights ----
    def adopt(self, network) -> None:
        """Copy `network`'s weights into the flat vector and make its parameters views of it."""
        sd = network.state_dict()
        mine = set(self.views) | set(self.buffer_views)
        if set(sd) != mine:
            raise LearnerError(f'state_dict keys do not match the learner\'s network: {sorted(set(sd) ^ mine)}')
        with torch.no_grad():
            for k, v in sd.items():
                dst = self.views[k] if k in self.views else self.buffer_views[k]
                if tuple(v.shape) != tuple(dst.shape):
                    raise LearnerError(f'{k}: shape {tuple(v.shape)} != {tuple(dst.shape)}')
                dst.copy_(v.to(self.device, dst.dtype))
            for k, p in network.named_parameters():
                p.data = self.views[k]
            for k, b in network.named_buffers():
                if k in self.buffer_views:
                    b.data = self.buffer_views[k]
        self.network = network
        self.commit()

    def planner_weights(self):
        """The network's weights as a planner binds them (`planner.Planner.bind_device_weights` / `reload`): the parameter views and the
        BatchNorm running statistics, views of the learner's flat vectors -- stable device addresses the kernels of `apply()` write."""
        out = dict(self.views)
        out.update({k: v for k, v in self.buffer_views.items() if not k.endswith('num_batches_tracked')})
        return out

    def _param_versions(self):
        return tuple(p._version for p in self.network.parameters())

    def load_state_dict(self, sd) -> None:
        with torch.no_grad():
            for k, v in sd.items():
                dst = self.views[k] if k in self.views else self.buffer_views[k]
                dst.copy_(torch.as_tensor(v).to(self.device, dst.dtype))
        self.commit()

    def state_dict(self):
        out = {k: v.detach().clone() for k, v in self.views.items()}
        out.update({k: v.detach().clone() for k, v in self.buffer_views.items()})
        return out

    def _bump_epoch(self) -> None:
        # torch's version counters do not see writes through the flat vector's views or by the kernels: the module's inference engine
        # (network.MuZeroNet._weights_version) rebinds on this epoch (load_state_dict / adopt left it on the old weights)
        self.network._mz_weights_epoch = getattr(self.network, '_mz_weights_epoch', 0) + 1

    def commit(self) -> None:
        """Rebuild the MFMA operand copies from the master weights (after anything other than `apply` wrote them)."""
        _check(load_library().mzl_commit(self._h, self._stream()))
        self._seen_versions = self._param_versions()
        self._bump_epoch()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- optimizer bookkeeping in torch's terms ----
    def current_lr(self, step: Optional[int] = None) -> float:
        """MultiStepLR: the rate of update number `step` (0-based count of updates done before it)."""
        s = self.steps if step is None else step
        return self.lr_init * self.gamma ** sum(1 for m in self.milestones if m <= s)

    def _param_names(self):
        return [k for k, _ in self.network.named_parameters()]  # torch.optim's parameter indices follow this order

    def optimizer_state_dict(self):
        names = self._param_names()
        state = {}
        for i, k in enumerate(names):
            v = self.views[k]
            off = v.data_ptr() - self.params.data_ptr()
            off //= 4
            state[i] = dict(step=torch.tensor(float(self.steps)), exp_avg=self.exp_avg[off:off + v.numel()].view(v.shape).clone(),
                            exp_avg_sq=self.exp_avg_sq[off:off + v.numel()].view(v.shape).clone())
        group = dict(lr=self.current_lr(), betas=self.betas, eps=self.eps, weight_decay=self.weight_decay, amsgrad=False, maximize=False,
                     params=list(range(len(names))))
        return dict(state=state, param_groups=[group])

    def load_optimizer_state_dict(self, osd) -> None:
        names = self._param_names()
        for i, k in enumerate(names):
            st = osd['state'].get(i)
            if st is None:
                continue
            v = self.views[k]
            off = (v.data_ptr() - self.params.data_ptr()) // 4
            self.exp_avg[off:off + v.numel()].copy_(st['exp_avg'].reshape(-1).to(self.device))
            self.exp_avg_sq[off:off + v.numel()].copy_(st['exp_avg_sq'].reshape(-1).to(self.device))
            self.steps = int(float(st['step']))

    def lr_scheduler_state_dict(self):
        return dict(milestones={m: 1 for m in self.milestones}, gamma=self.gamma, last_epoch=self.steps, _step_count=self.steps + 1,
                    base_lrs=[self.lr_init], _last_lr=[self.current_lr()])

    # ---- the step ----
    def grad(self, ring, index: Optional[torch.Tensor], weights: Optional[torch.Tensor], batch: int, frame_spec=None):
        """Loss and gradient of one batch (pipeline.py:241-244).  `ring`: mapping field -> device tensor [rows, ...] (the replay's
        storages, or a stacked batch with index=None); `index`: int64 device tensor [batch] of rows; `weights`: float32 [batch] or None
        (uniform replay: ones).  Fills `self.grad_flat`, `self.loss`, `self.priorities[:batch]`; enqueues only.  States may be float32,
        int8, or the packed uint8 rows of a `PrioritizedReplay(state_format='frames_u8')` (conv nets; the ring's storages carry their
        `frame_spec`, a plain mapping takes it from the argument): the gather kernel decodes them exactly."""
        if batch < 1 or batch > self.max_batch:
            raise LearnerError(f'batch {batch} outside [1, max_batch = {self.max_batch}]')
        if self._param_versions() != self._seen_versions:
            # torch wrote the parameters (network.load_state_dict on a checkpoint -- the reference's resume path, pipeline.py:810-817 -- or an
            # in-place edit): the master weights are those tensors, the kernels' operand copies are rebuilt from them
            self.commit()
        st, ac = ring['state'], ring['action']
        frame_spec = frame_spec if frame_spec is not None else getattr(ring, 'frame_spec', None)
        frames = st.dtype == torch.uint8
        if st.dtype not in (torch.float32, torch.int8, torch.uint8) or not st.is_contiguous():
            raise LearnerError(f'state storage must be contiguous float32, int8 or packed uint8 frames, got {st.dtype}')
        if ac.dtype not in (torch.int8, torch.int16) or not ac.is_contiguous():
            raise LearnerError(f'action storage must be contiguous int8 or int16, got {ac.dtype}')
        row_bytes = fs = fc = 0
        if frames:
            if frame_spec is None or len(tuple(frame_spec)) != 5:
                raise LearnerError('uint8 states are state_format frames_u8 rows: frame_spec = (S, C, H, W, A) is required')
            fs, fc, fh, fw, fa = (int(v) for v in frame_spec)
            row_bytes = int(np.prod(st.shape[1:]))
            if fa != self.A or fs * (fc + 1) * fh * fw != self.in_dim or st.dim() != 2:
                raise LearnerError(f'state_format frames_u8: frame_spec {tuple(frame_spec)} does not match the learner ({self.in_dim} observation elements, {self.A} actions)')
        elif int(np.prod(st.shape[1:])) != self.in_dim:
            raise LearnerError('replay item shapes do not match the learner')
        if tuple(ac.shape[1:]) != (self.K,) or tuple(ring['pi_prob'].shape[1:]) != (self.K, self.A):
            raise LearnerError('replay item shapes do not match the learner')
        for f in ('pi_prob', 'value', 'reward'):
            if ring[f].dtype != torch.float32 or not ring[f].is_contiguous():
                raise LearnerError(f'{f} storage must be contiguous float32')
        if index is None:
            index = self._iota[:batch]
        # every pointer handed to the kernels must be memory of the learner's GPU: a host-resident replay (PrioritizedReplay's default
        # device) would be read as a device address
        for name, t in (('state', st), ('action', ac), ('pi_prob', ring['pi_prob']), ('value', ring['value']), ('reward', ring['reward']),
                        ('index', index), ('weights', self._ones if weights is None else weights)):
            if t.device != self.device:
                raise LearnerError(f'{name} lives on {t.device}, the learner on {self.device}: build the replay with device=\'cuda\' '
                                   f'(muzero_amd.replay.PrioritizedReplay(..., device=\'cuda\')) and pass device tensors')
        if index.dtype != torch.int64 or index.numel() != batch:
            raise LearnerError('index must be an int64 tensor of `batch` rows')
        w = self._ones if weights is None else weights
        if w.dtype != torch.float32 or w.numel() < batch:
            raise LearnerError('weights must be a float32 tensor of `batch` entries')
        b = MzlBatch(st.data_ptr(), ac.data_ptr(), ring['pi_prob'].data_ptr(), ring['value'].data_ptr(), ring['reward'].data_ptr(),
                     index.data_ptr(), w.data_ptr(), self.loss.data_ptr(), self.priorities.data_ptr(), batch,
                     2 if frames else (1 if st.dtype == torch.int8 else 0), ac.element_size(), row_bytes, fs, fc)
        _check(load_library().mzl_grad(self._h, C.byref(b), self._stream()))
        self._keep = (ring, index, w)  # alive until the next call (the kernels read them asynchronously)
        if self.buffer_views:
            self._bump_epoch()  # (train-mode BatchNorm: the forward pass has updated the running statistics the planner folds into its weights)
        return self.loss, self.priorities[:batch]

    def apply(self, clip: Optional[bool] = None) -> None:
        """clip_grad_norm_ (if configured) + optimizer.step() + lr_scheduler.step() (pipeline.py:246-250)."""
        clip = self.clip_grad if clip is None else clip
        lr = self.current_lr()
        self.steps += 1
        _check(load_library().mzl_apply(self._h, lr, self.betas[0], self.betas[1], self.eps, self.weight_decay, self.max_grad_norm if clip else 0.0,
                                        self.steps, self._stream()))
        self._bump_epoch()

    def step(self, ring, index, weights, batch: int, allreduce: bool = True, frame_spec=None):
        """One update.  With an initialised multi-rank process group the flat gradient is averaged over the ranks in ONE all-reduce
        (RCCL; xGMI rings are per-link bound, so one 1-30 MB transfer beats per-tensor collectives) between gradient and update."""
        loss, prio = self.grad(ring, index, weights, batch, frame_spec=frame_spec)
        if allreduce:
            import torch.distributed as dist

            if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
                dist.all_reduce(self.grad_flat, op=dist.ReduceOp.SUM)
                self.grad_flat.div_(dist.get_world_size())
        self.apply()
        return loss, prio

    def step_transitions(self, transitions, weights=None, frame_spec=None):
        """One update on a stacked batch (`Transition` of arrays / tensors, as `replay.sample` returns them).  uint8 states are packed
        `frames_u8` rows [B, row bytes] and need their `frame_spec`."""
        def dev(x, dt):
            t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
            return t.to(self.device, dt).contiguous()

        st = transitions.state
        st_dt = torch.int8 if (torch.is_tensor(st) and st.dtype == torch.int8) or (not torch.is_tensor(st) and np.asarray(st).dtype == np.int8) else torch.float32
        if frame_spec is not None and ((torch.is_tensor(st) and st.dtype == torch.uint8) or (not torch.is_tensor(st) and np.asarray(st).dtype == np.uint8)):
            st_dt = torch.uint8
        B = int(st.shape[0])
        ring = dict(state=dev(st, st_dt).reshape(B, -1), action=dev(transitions.action, torch.int16 if self.A > 128 else torch.int8),
                    pi_prob=dev(transitions.pi_prob, torch.float32), value=dev(transitions.value, torch.float32), reward=dev(transitions.reward, torch.float32))
        w = None if weights is None else dev(weights, torch.float32)
        return self.step(ring, None, w, B, frame_spec=frame_spec if st_dt == torch.uint8 else None)

    def debug_conv(self, direction: int, weight, x, action=None, num_actions: int = 0, cin: Optional[int] = None):
        """Diagnostic (tests): ONE 3 x 3 conv through the learner's packers, tiling chooser and dispatcher at this handle's conv_precision
        (identity staging; no statistics, skip or mask).  direction 0: the forward conv of x [B, cin_real, h, w] (+ action planes up to `cin`
        channels) with weight [cout, cin, 3, 3]; direction 1: the data gradient of dy = x [B, cout, h, w].  Host arrays; returns (out, build name)."""
        weight = np.ascontiguousarray(weight, np.float32)
        x = np.ascontiguousarray(x, np.float32)
        if weight.ndim != 4 or x.ndim != 4:
            raise LearnerError('mzl_debug_conv: weight [cout, cin, 3, 3] and x [B, channels, h, w]')
        cout, wcin = int(weight.shape[0]), int(weight.shape[1])
        B, xc, bh, bw = (int(v) for v in x.shape)
        cin = wcin if cin is None else int(cin)
        if tuple(weight.shape[2:]) != (3, 3) or cin != wcin or (direction == 0 and xc > cin) or (direction != 0 and xc != cout):
            raise LearnerError(f'mzl_debug_conv: weight {weight.shape} / cin {cin} do not fit x {x.shape} in direction {direction}')
        cin_real = xc if direction == 0 else cin
        out = np.zeros((B, cout if direction == 0 else cin, bh, bw), np.float32)
        act = None if action is None else np.ascontiguousarray(action, np.int32)
        name = C.c_char_p()
        _check(load_library().mzl_debug_conv(self._h, int(direction), B, cin_real, cin, cout, bh, bw, weight.ctypes.data_as(C.c_void_p),
                                             x.ctypes.data_as(C.c_void_p), None if act is None else act.ctypes.data_as(C.c_void_p), int(num_actions),
                                             out.ctypes.data_as(C.c_void_p), C.byref(name)))
        return out, (name.value or b'').decode()

    def debug_conv_tile(self, direction: int, weight, x, skip=None, mask=None, mcoef=None, partner=None, precision='f32', route: str = 'plane',
                        want_part: bool = False):
        """Diagnostic (tests): ONE stride-1 conv of the Atari net's tile path as the update builds it (gather into haloed tiles, op builder,
        dispatcher), at `precision` ('f32' | 'bf16x3') whatever the handle's switches.  direction 0: the forward conv of the plane x [B, cin, H, W]
        with weight [cout, cin, 3, 3]; direction 1: the data gradient of dy = x [B, cout, H, W].  route: 'plane' (the update: the out_plane
        epilogue; skip, mask + partner (+ mcoef) and the statistics partials belong to it), 'inner' / 'whole' (inner-only or whole haloed tiles and
        k_lc_tile_scatter; skip only).  Host arrays; returns (out, build name) or, want_part, (out, build name, partials [tiles, pad16(c_out), 4 | 2])."""
        f32 = np.float32
        weight, x = np.ascontiguousarray(weight, f32), np.ascontiguousarray(x, f32)
        if weight.ndim != 4 or x.ndim != 4 or tuple(weight.shape[2:]) != (3, 3):
            raise LearnerError('mzl_debug_conv_tile: weight [cout, cin, 3, 3] and x [B, channels, H, W]')
        cout, cin = int(weight.shape[0]), int(weight.shape[1])
        B, xc, H, W = (int(v) for v in x.shape)
        c_out = cout if direction == 0 else cin
        if xc != (cin if direction == 0 else cout):
            raise LearnerError(f'mzl_debug_conv_tile: weight {weight.shape} does not fit x {x.shape} in direction {direction}')
        if route not in TILE_ROUTES:
            raise ValueError(f"route must be one of {sorted(TILE_ROUTES)}, not {route!r}")
        keep = [weight, x]

        def arr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, f32)
            if tuple(a.shape) != shape:
                raise LearnerError(f'mzl_debug_conv_tile: an operand of shape {a.shape}, expected {shape}')
            keep.append(a)
            return a.ctypes.data_as(C.c_void_p)

        out = np.zeros((B, c_out, H, W), f32)
        cpo = (c_out + 15) // 16 * 16
        # (a masked conv always leaves its ST_BWD sums; rows: at least the tiles of the call)
        part = np.zeros((B * (H // 12) * (W // 12), cpo, 2 if mask is not None else 4), f32) if want_part or mask is not None else None
        call = MzlTileCall(int(direction), _atari_precision(precision, 'precision'), TILE_ROUTES[route], B, cin, cout, H, W, 0, 0,
                           weight.ctypes.data_as(C.c_void_p), x.ctypes.data_as(C.c_void_p), arr(skip, out.shape), arr(mask, out.shape), arr(mcoef, (2, c_out)),
                           arr(partner, out.shape), out.ctypes.data_as(C.c_void_p), None if part is None else part.ctypes.data_as(C.c_void_p))
        name = C.c_char_p()
        _check(load_library().mzl_debug_conv_tile(self._h, C.byref(call), C.byref(name)))
        name = (name.value or b'').decode()
        return (out, name, part[:call.groups]) if want_part else (out, name)

    def debug_atari_stage(self, op: str, **a):
        """Diagnostic (tests): ONE launch group of the Atari representation outside its stride-1 convs, through the members the update calls
        (mzl_debug_atari_stage).  Host arrays in, (result, build name) or (result, build name, statistics partials) out:
          's2_fwd'    weight [cout, cin, 3, 3], x [B, cin, 2H, 2W]                     -> y [B, cout, H, W]
          's2_dgrad'  weight, dy [B, cout, H, W]                                       -> dx [B, cin, 2H, 2W]
          'pool_fwd'  x [B, C, ih, iw]                                                 -> [B, C, ih / 2, iw / 2]
          'pool_bwd'  g [B, C, ih / 2, iw / 2]                                         -> [B, C, ih, iw]
          'relu_bwd'  g, x [B, C, H, W]                                                -> dz
          'entry'     x [B, C, H, W], gs=None, extra=None, partner, scale=1.0, launcher='atari' | 'tower' | 'rep12'
                                                                                       -> dz, name, partials [groups, pad16(C), 2]
          'normalize' x [B, C, H, W]                                                   -> s
          'gather'    src0 [B, C, stride H, stride W], src1=None, coef=None [3, C], mode='ident' | 'bnrelu' | 'bnbwd', stride=1, origin=(0, 0),
                      inner_only=False                                                 -> tiles [B nty ntx, C, 14, tw + 2]
          'scatter'   tiles [B nty ntx, C, 14, tw + 2] (src_inner: [.., C, 12, tw]), H, W (the tiled plane), stride=1, origin=(0, 0), skip=None,
                      src_inner=False, want_stats=False                                -> plane [B, C, stride H, stride W] (NaN where this parity
                                                                                          does not write)[, name, partials [groups, pad16(C), 4]]"""
        if op not in STAGE_OPS:
            raise ValueError(f"op must be one of {sorted(STAGE_OPS)}, not {op!r}")
        f32 = np.float32
        keep = []

        def arr(v, ndim=4):
            if v is None:
                return None
            v = np.ascontiguousarray(v, f32)
            if v.ndim != ndim:
                raise LearnerError(f'mzl_debug_atari_stage: {op}: an operand of {v.ndim} dimensions, expected {ndim}')
            keep.append(v)
            return v

        def ptr(v):
            return None if v is None else v.ctypes.data_as(C.c_void_p)

        def same(v, ref, what):
            if v is not None and v.shape != ref.shape:
                raise LearnerError(f'mzl_debug_atari_stage: {op}: {what} of shape {v.shape}, expected {ref.shape}')
            return v

        call = MzlStageCall()
        call.op, call.scale, call.stride = STAGE_OPS[op], 1.0, 1
        stats = None
        if op in ('s2_fwd', 's2_dgrad'):
            w, x = arr(a.pop('weight')), arr(a.pop('x' if op == 's2_fwd' else 'dy'))
            if tuple(w.shape[2:]) != (3, 3) or x.shape[1] != w.shape[1 if op == 's2_fwd' else 0]:
                raise LearnerError(f'mzl_debug_atari_stage: {op}: weight {w.shape} does not fit the plane {x.shape}')
            B, _, h, wd = x.shape
            if op == 's2_fwd':
                if h % 2 or wd % 2:
                    raise LearnerError(f'mzl_debug_atari_stage: s2_fwd: x: odd source sizes {h} x {wd}')
                H, W, out = h // 2, wd // 2, np.zeros((B, w.shape[0], h // 2, wd // 2), f32)
            else:
                H, W, out = h, wd, np.zeros((B, w.shape[1], 2 * h, 2 * wd), f32)
            call.batch, call.cin, call.cout, call.H, call.W = B, w.shape[1], w.shape[0], H, W
            call.weight, call.in0 = ptr(w), ptr(x)
        elif op in ('pool_fwd', 'pool_bwd'):
            x = arr(a.pop('x' if op == 'pool_fwd' else 'g'))
            B, Cn, h, wd = x.shape
            H, W = (h, wd) if op == 'pool_fwd' else (2 * h, 2 * wd)
            out = np.zeros((B, Cn, H // 2, W // 2) if op == 'pool_fwd' else (B, Cn, H, W), f32)
            call.batch, call.cin, call.H, call.W, call.in0 = B, Cn, H, W, ptr(x)
        elif op == 'relu_bwd':
            g = arr(a.pop('g'))
            x = same(arr(a.pop('x')), g, 'x')
            out = np.zeros(g.shape, f32)
            (call.batch, call.cin, call.H, call.W), call.in0, call.in1 = g.shape, ptr(g), ptr(x)
        elif op in ('entry', 'normalize'):
            x = arr(a.pop('x'))
            out = np.zeros(x.shape, f32)
            (call.batch, call.cin, call.H, call.W), call.in0 = x.shape, ptr(x)
            if op == 'entry':
                launcher = a.pop('launcher', 'atari')
                if launcher not in ENTRY_LAUNCHERS:
                    raise ValueError(f"launcher must be one of {sorted(ENTRY_LAUNCHERS)}, not {launcher!r}")
                call.launcher, call.scale = ENTRY_LAUNCHERS[launcher], float(a.pop('scale', 1.0))
                call.in1, call.in2 = ptr(same(arr(a.pop('gs', None)), x, 'gs')), ptr(same(arr(a.pop('extra', None)), x, 'extra'))
                call.in3 = ptr(same(arr(a.pop('partner', None)), x, 'partner'))
                stats = np.zeros((x.shape[0] * -(-(x.shape[2] * x.shape[3]) // 32), (x.shape[1] + 15) // 16 * 16, 2), f32)
        elif op == 'gather':
            src0 = arr(a.pop('src0'))
            src1 = same(arr(a.pop('src1', None)), src0, 'src1')
            B, Cn, h, wd = src0.shape
            mode, stride, (py, px) = a.pop('mode', 'ident'), int(a.pop('stride', 1)), a.pop('origin', (0, 0))
            if mode not in ('ident', 'bnrelu', 'bnbwd'):
                raise ValueError(f"mode must be 'ident', 'bnrelu' or 'bnbwd', not {mode!r}")
            if stride not in (1, 2) or h % stride or wd % stride:
                raise LearnerError(f'mzl_debug_atari_stage: gather: stride {stride} on a source of odd sizes or not 1 | 2: {h} x {wd}')
            coef = arr(a.pop('coef', None), 2)
            if coef is not None and coef.shape != (3, Cn):
                raise LearnerError(f'mzl_debug_atari_stage: gather: coef of shape {coef.shape}, expected {(3, Cn)}')
            H, W = h // stride, wd // stride
            tw = 16 if self.debug_atari_wide_tiles(W) else 12
            out = np.zeros((B * (H // 12) * (W // tw), Cn, 14, tw + 2), f32)
            call.batch, call.cin, call.H, call.W, call.mode, call.stride, call.py, call.px = B, Cn, H, W, IN_MODES[mode], stride, int(py), int(px)
            call.inner_only, call.in0, call.in1, call.coef = int(bool(a.pop('inner_only', False))), ptr(src0), ptr(src1), ptr(coef)
        else:  # scatter
            tiles = arr(a.pop('tiles'))
            H, W, stride, (py, px) = int(a.pop('H')), int(a.pop('W')), int(a.pop('stride', 1)), a.pop('origin', (0, 0))
            src_inner, want_stats = bool(a.pop('src_inner', False)), bool(a.pop('want_stats', False))
            Cn = tiles.shape[1]
            tw = 16 if self.debug_atari_wide_tiles(W) else 12
            B = tiles.shape[0] // max(1, (H // 12) * (W // tw))
            if H < 12 or W < 12 or stride not in (1, 2) or tiles.shape != (B * (H // 12) * (W // tw), Cn) + ((12, tw) if src_inner else (14, tw + 2)) or B < 1:
                raise LearnerError(f'mzl_debug_atari_stage: scatter: tiles of shape {tiles.shape} do not cut a {H} x {W} plane (tile width {tw})')
            out = np.zeros((B, Cn, stride * H, stride * W), f32)
            skip = same(arr(a.pop('skip', None)), out, 'skip')
            call.batch, call.cin, call.H, call.W, call.stride, call.py, call.px = B, Cn, H, W, stride, int(py), int(px)
            call.src_inner, call.want_stats, call.in0, call.in1 = int(src_inner), int(want_stats), ptr(tiles), ptr(skip)
            if want_stats:
                stats = np.zeros((B * -(-(H * W) // 32), (Cn + 15) // 16 * 16, 4), f32)
        if a:
            raise TypeError(f'debug_atari_stage({op!r}): unexpected arguments {sorted(a)}')
        call.out, call.stats = ptr(out), ptr(stats)
        name = C.c_char_p()
        _check(load_library().mzl_debug_atari_stage(self._h, C.byref(call), C.byref(name)))
        name = (name.value or b'').decode()
        return (out, name) if stats is None else (out, name, stats[:call.groups])

    def debug_atari_wide_tiles(self, W: int) -> bool:
        """AtariRun::tile_w: does this handle cut a plane of width W into 16-column tiles?  (MZLC_NO_WIDE_TILES=1 at create: never.)"""
        return self._wide_tiles and W % 16 == 0 and W // 16 >= 3

    def debug_precisions(self):
        """Diagnostic (tests): (tower_precision, stage_precision, wgrad_precision) as the HANDLE holds them (conv nets)."""
        v = (C.c_int32 * 3)()
        _check(load_library().mzl_debug_precisions(self._h, v))
        return tuple(int(x) for x in v)

    def debug_wgrad(self, dz, x, mode: str = 'plain', y=None, dcoef=None, xcoef=None, action=None, num_actions: int = 0, cin: Optional[int] = None,
                    preload=None, accumulate: bool = False, second=None, sg: int = 0, layout: int = 0, ipw: int = 0, remap: int = 0, act_route: int = 0,
                    ring_rows: int = -1, tapmask: int = 0):
        """Diagnostic (tests): ONE layer's weight gradient through the learner's op builders, geometry chooser and dispatcher (mzl_debug_wgrad).
        dz [B, cout, h, w] and x [B, cin_real, h, w] (mode 'steps': a leading source axis on dz, x, y, dcoef, xcoef); optional y with dcoef
        [3, cout] (dy = c1 dz + c2 y + c3), xcoef [2, cin_real] (x' = relu(a x + b)), action [B] with num_actions and cin > cin_real, preload
        [cout, cin, 3, 3] (+ accumulate).  mode 'pair': `second` = dict(dz=, x=, ...) of the other layer of the launch; 'ring' (Atari handles):
        haloed tiles, ring_rows -1 .. 3 and a tap mask.  Overrides (0: what the update chooses): sg images per staging round, layout 1 side by
        side / 2 stacked, ipw images per chunk, remap 1 on / 2 off, act_route 1 in-kernel / 2 sparse.  Returns (dW [cout, cin, 3, 3], name of
        what ran); mode 'pair': ((dW, dW of the second layer), name)."""
        lib = load_library()
        if not hasattr(lib, 'mzl_debug_wgrad'):
            raise LearnerError('mzl_debug_wgrad: this library has no such hook')
        if mode not in WGRAD_MODES:
            raise LearnerError(f'mzl_debug_wgrad: mode {mode!r} (one of {sorted(WGRAD_MODES)})')
        lead = 1 if mode == 'steps' else 0
        call = MzlWgradCall()
        keep = []

        def arr(a, dt=np.float32):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            return a.ctypes.data

        def fill(J, dz, x, y=None, dcoef=None, xcoef=None, action=None, cin=None, preload=None):
            dz, x = np.ascontiguousarray(dz, np.float32), np.ascontiguousarray(x, np.float32)
            if dz.ndim != 4 + lead or x.ndim != 4 + lead or dz.shape[:lead + 1] != x.shape[:lead + 1] or dz.shape[-2:] != x.shape[-2:]:
                raise LearnerError(f'mzl_debug_wgrad: dz {dz.shape} and x {x.shape} do not fit (mode {mode})')
            cout, cr = int(dz.shape[lead + 1]), int(x.shape[lead + 1])
            cin = cr if cin is None else int(cin)
            for a, shape, what in ((y, dz.shape, 'y'), (dcoef, dz.shape[:lead] + (3, cout), 'dcoef'), (xcoef, dz.shape[:lead] + (2, cr), 'xcoef'),
                                   (action, (dz.shape[lead],), 'action'), (preload, (cout, cin, 3, 3), 'preload')):
                if a is not None and tuple(np.shape(a)) != tuple(shape):
                    raise LearnerError(f'mzl_debug_wgrad: {what} {np.shape(a)} is not {tuple(shape)}')
            out = np.zeros((cout, max(cin, 0), 3, 3), np.float32)
            keep.append(out)
            J.dz, J.x, J.y, J.dcoef, J.xcoef = arr(dz), arr(x), arr(y), arr(dcoef), arr(xcoef)
            J.action, J.preload, J.out = arr(action, np.int32), arr(preload), out.ctypes.data
            J.cin_real, J.cin, J.cout = cr, cin, cout
            return out, dz.shape

        out0, shp = fill(call.layer[0], dz, x, y, dcoef, xcoef, action, cin, preload)
        outs = [out0]
        if mode == 'pair':
            if second is None:
                raise LearnerError("mzl_debug_wgrad: mode 'pair' needs `second`")
            o1, shp1 = fill(call.layer[1], **second)
            if shp1[0] != shp[0] or shp1[-2:] != shp[-2:]:
                raise LearnerError('mzl_debug_wgrad: the two layers of a pair share batch and board')
            outs.append(o1)
        call.mode, call.batch, call.h, call.w = WGRAD_MODES[mode], int(shp[lead]), int(shp[-2]), int(shp[-1])
        call.num_actions, call.nsrc, call.accumulate = int(num_actions), int(shp[0]) if lead else 1, int(bool(accumulate))
        call.sg, call.layout, call.ipw, call.remap, call.act_route = int(sg), int(layout), int(ipw), int(remap), int(act_route)
        call.ring_rows, call.tapmask = int(ring_rows), int(tapmask)
        name = C.c_char_p()
        _check(lib.mzl_debug_wgrad(self._h, C.byref(call), C.byref(name)))
        return (tuple(outs) if mode == 'pair' else out0), (name.value or b'').decode()

    def debug_conv_fused(self, job, mode: str = 'conv', second=None, no_side: bool = False, batch: Optional[int] = None, hw=None, count: Optional[float] = None):
        """Diagnostic (tests): ONE conv of a BatchNorm tower as the update runs it (mzl_debug_conv_fused: the op builders, make_geom, launch_ops).
        `job` (and `second`, mode 'pair') is a dict:
          weight [cout, cin, 3, 3], direction 0 forward | 1 data gradient, in0 [B, c_in, h, w], in_mode 'ident' | 'bnrelu' | 'bnbwd' | 'bnres', in1, coef
          [3, c_in]; mat_preload (asks for the write-through); skip, mask, mcoef [2, c_out], partner (an array, or the string 'mask': the mask buffer
          itself); stat 'fwd' | 'bwd' | None; finalize 'fwd' | 'bwd' | None with gamma, beta, save [2, c_out], running_mean, running_var, num_batches,
          accumulate, dgamma, dbeta.
        mode 'finalize': part [groups, pad16(C), 4 | 2], finalize, count and the finalize operands, no conv; mode 'apply': y, res (or None), coef [2, C].
        Returns (dict of what came back -- out, mat_out, part, groups, coef [3, cpad], save [2, cpad], running_mean, running_var, num_batches, dgamma,
        dbeta -- or a tuple of two for a pair, the name of what ran)."""
        lib = load_library()
        if not hasattr(lib, 'mzl_debug_conv_fused'):
            raise LearnerError('mzl_debug_conv_fused: this library has no such hook')
        if mode not in FUSED_MODES:
            raise LearnerError(f'mzl_debug_conv_fused: mode {mode!r} (one of {sorted(FUSED_MODES)})')
        call = MzlFusedCall()
        keep = []
        f32 = np.float32

        def arr(a, dt=f32):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dt)
            keep.append(a)
            return a.ctypes.data

        def new(shape, src=None, dt=f32):
            a = np.zeros(shape, dt) if src is None else np.array(src, dt).reshape(shape)
            keep.append(a)
            return a

        def fill(J, job):
            res = {}
            fin = STAT_MODES[job.get('finalize')]
            J.finalize, J.accumulate = fin, int(bool(job.get('accumulate', False)))
            if mode == 'apply':
                y = np.ascontiguousarray(job['y'], f32)
                B, Cc, bh, bw = y.shape
                J.cin = J.cout = Cc
                res['out'] = new(y.shape)
                J.in0, J.in1, J.coef, J.out = arr(y), arr(job.get('res')), arr(job['coef']), res['out'].ctypes.data
                return res, (B, bh, bw)
            if mode == 'finalize':
                part = np.ascontiguousarray(job['part'], f32)
                Cc = int(np.shape(job['gamma'])[0])
                J.cin = J.cout = Cc
                J.part_in = arr(part)
                res['groups'] = int(part.shape[0])
                shape = (batch or 1,) + tuple(hw or (1, 1))
            else:
                weight, in0 = np.ascontiguousarray(job['weight'], f32), np.ascontiguousarray(job['in0'], f32)
                if weight.ndim != 4 or in0.ndim != 4 or tuple(weight.shape[2:]) != (3, 3):
                    raise LearnerError('mzl_debug_conv_fused: weight [cout, cin, 3, 3] and in0 [B, channels, h, w]')
                J.direction = int(job.get('direction', 0))
                J.cout, J.cin = int(weight.shape[0]), int(weight.shape[1])
                c_in, c_out = (J.cout, J.cin) if J.direction else (J.cin, J.cout)
                B, xc, bh, bw = in0.shape
                if xc != c_in:
                    raise LearnerError(f'mzl_debug_conv_fused: in0 {in0.shape} does not fit weight {weight.shape} in direction {J.direction}')
                shape = (B, bh, bw)
                oshape = (B, c_out, bh, bw)
                for k, shp in (('in1', in0.shape), ('mat_preload', in0.shape), ('coef', (3, c_in)), ('skip', oshape), ('mask', oshape), ('mcoef', (2, c_out))):
                    if job.get(k) is not None and tuple(np.shape(job[k])) != tuple(shp):
                        raise LearnerError(f'mzl_debug_conv_fused: {k} {np.shape(job[k])} is not {tuple(shp)}')
                J.in_mode, J.stat_mode = IN_MODES[job.get('in_mode', 'ident')], STAT_MODES[job.get('stat')]
                J.weight, J.in0, J.in1, J.coef = arr(weight), arr(in0), arr(job.get('in1')), arr(job.get('coef'))
                J.skip, J.mask, J.mcoef = arr(job.get('skip')), arr(job.get('mask')), arr(job.get('mcoef'))
                partner = job.get('partner')
                if isinstance(partner, str):
                    J.partner_is_mask = 1
                else:
                    J.partner = arr(partner)
                res['out'] = new(oshape)
                J.out = res['out'].ctypes.data
                if job.get('mat_preload') is not None:
                    res['mat_out'] = new(in0.shape)
                    J.mat_preload, J.mat_out = arr(job['mat_preload']), res['mat_out'].ctypes.data
                Cc = c_out
            cpad = (Cc + 15) // 16 * 16
            if mode != 'finalize' and J.stat_mode:
                res['part'] = new((shape[0], cpad, 4 if J.stat_mode == 1 else 2))  # (at most one group per image; cut to the groups that ran)
                J.part = res['part'].ctypes.data
            if fin:
                res['coef'] = new((3, cpad))
                J.coef_out, J.gamma = res['coef'].ctypes.data, arr(job['gamma'])
            if fin == 1:
                res['save'] = new((2, cpad))
                J.save_out, J.beta = res['save'].ctypes.data, arr(job['beta'])
                if job.get('running_mean') is not None:
                    res['running_mean'], res['running_var'] = new((Cc,), job['running_mean']), new((Cc,), job['running_var'])
                    J.running_mean, J.running_var = res['running_mean'].ctypes.data, res['running_var'].ctypes.data
                if job.get('num_batches') is not None:
                    res['num_batches'] = new((1,), [job['num_batches']], np.int64)
                    J.num_batches = res['num_batches'].ctypes.data
            if fin == 2:
                res['dgamma'], res['dbeta'] = new((Cc,), job.get('dgamma')), new((Cc,), job.get('dbeta'))
                J.save_in, J.dgamma, J.dbeta = arr(job['save']), res['dgamma'].ctypes.data, res['dbeta'].ctypes.data
            return res, shape

        res0, shape = fill(call.conv[0], job)
        results = [res0]
        if mode == 'pair':
            if second is None:
                raise LearnerError("mzl_debug_conv_fused: mode 'pair' needs `second`")
            res1, shape1 = fill(call.conv[1], second)
            if shape1 != shape:
                raise LearnerError('mzl_debug_conv_fused: the two jobs of a pair share batch and board')
            results.append(res1)
        call.mode, call.batch, call.h, call.w, call.no_side = FUSED_MODES[mode], int(shape[0]), int(shape[1]), int(shape[2]), int(bool(no_side))
        if mode == 'finalize':
            call.groups, call.count = res0['groups'], float(count)
        name = C.c_char_p()
        _check(lib.mzl_debug_conv_fused(self._h, C.byref(call), C.byref(name)))
        for r in results:
            if mode in ('conv', 'pair'):
                r['groups'] = int(call.groups)
                if 'part' in r:
                    r['part'] = r['part'][:call.groups]
            if 'num_batches' in r:
                r['num_batches'] = int(r['num_batches'][0])
        return (tuple(results) if mode == 'pair' else res0), (name.value or b'').decode()

    def debug_heads(self, F_pred, F_rew, params, running, nbt, pi, value, reward, idx, w, skip=()):
        """Diagnostic (tests): the head block alone through the update's own launch code (mzl_debug_heads), on temporary buffers: the learner's state is
        not touched.  F_pred, F_rew [K, B, P, hw]; params, running, nbt in the hook's flat layouts (csrc/mz_learn_conv_host.h; tests/heads_cases.py
        builds them); pi [rows, K, A], value, reward [rows, K], idx [B], w [B].  Returns a dict of every output, shaped (NaN where no kernel wrote);
        names in `skip` are passed as null pointers and left out."""
        lib = load_library()
        if not hasattr(lib, 'mzl_debug_heads'):
            raise LearnerError('mzl_debug_heads: this library has no such hook')
        if self.kind not in ('board', 'atari'):
            call = MzlHeadsCall()
            _check(lib.mzl_debug_heads(self._h, C.byref(call)))
        P, hw, Sr, Sv = self._heads_geom
        K, A = self.K, self.A
        f32 = np.float32
        ins = dict(F_pred=np.ascontiguousarray(F_pred, f32), F_rew=np.ascontiguousarray(F_rew, f32), params=np.ascontiguousarray(params, f32),
                   running=np.ascontiguousarray(running, f32), nbt=np.ascontiguousarray(nbt, np.int64), pi=np.ascontiguousarray(pi, f32),
                   value=np.ascontiguousarray(value, f32), reward=np.ascontiguousarray(reward, f32), idx=np.ascontiguousarray(idx, np.int64), w=np.ascontiguousarray(w, f32))
        B, rows = int(ins['idx'].shape[0]), int(ins['value'].shape[0])
        ng, nmax = 3 * K, max(A, Sr, Sv)
        npar = sum(oc * P + 2 * oc + n * oc * hw + n for oc, n in ((1, Sr), (2, A), (1, Sv)))
        want = dict(F_pred=(K, B, P, hw), F_rew=(K, B, P, hw), params=(npar,), running=(8,), nbt=(3,), pi=(rows, K, A), value=(rows, K), reward=(rows, K), idx=(B,), w=(B,))
        for k, shp in want.items():
            if tuple(ins[k].shape) != shp:
                raise LearnerError(f'mzl_debug_heads: {k} {tuple(ins[k].shape)} is not {shp}')
        shapes = dict(u=(ng, B, 2, hw), spart_fwd=(ng, B, 2, 2), spiv=(ng, B, 2), coef=(ng, 2, 5), save=(ng, 2, 2), feat=(ng, B, 2 * hw), dlogit=(ng, B, nmax),
                      dzb=(ng, B, 2, hw), spart_bwd=(ng, B, 2, 2), lpart=(ng, B), loss=(1,), prio=(B,), running_out=(8,), nbt_out=(3,), dF_pred=(K, B, P, hw),
                      dF_rew=(K, B, P, hw), wpart=(K, npar - 4 * 2), grads=(npar,))
        out = {k: np.zeros(shp, np.int64 if k == 'nbt_out' else f32) for k, shp in shapes.items() if k not in skip}
        call = MzlHeadsCall()
        call.batch, call.rows = B, rows
        for k, a in list(ins.items()) + list(out.items()):
            setattr(call, k, a.ctypes.data)
        _check(lib.mzl_debug_heads(self._h, C.byref(call)))
        return out

    def close(self) -> None:
        if self._h:
            load_library().mzl_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
