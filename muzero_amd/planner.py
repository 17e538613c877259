"""ctypes binding of libmzplanner_hip.so (C ABI: include/mzplanner.h).

This module is the only place where the Python mirror of the reference API touches native code.  There is no CPU
fallback: if the library cannot be loaded, or no MI355X is visible, the calls raise PlannerError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'lib', 'libmzplanner_hip.so')

NET_MLP, NET_BOARD, NET_ATARI = 0, 1, 2
ENV_NONE, ENV_CARTPOLE, ENV_TICTACTOE, ENV_GOMOKU, ENV_SYNTHETIC, ENV_EXTERNAL, ENV_CATCH, ENV_BREAKOUT = 0, 1, 2, 3, 4, 5, 6, 7
ENV_CONNECT4 = 8
ENV_OTHELLO = 9
ENV_GO = 10
_NET_KINDS = {'mlp': NET_MLP, 'board': NET_BOARD, 'atari': NET_ATARI}
ARENA_NONE, ARENA_RANDOM, ARENA_PLANNER = 0, 1, 2  # opponent kinds of mz_arena_reset
SIDE_CHALLENGER, SIDE_OPPONENT, SIDE_RANDOM, SIDE_OPENING = 0, 1, 2, 3  # who chose a ply's move (arena_read_ply 'side')
ARENA_UNFINISHED, ARENA_WIN_CHALLENGER, ARENA_WIN_OPPONENT, ARENA_DRAW = 0, 1, 2, 3  # arena_result 'winner'

# every symbol include/mzplanner.h declares (tests/test_abi.py checks the library exports all of them)
ABI_SYMBOLS = [
    'mz_last_error', 'mz_version', 'mz_planner_describe', 'mz_planner_create', 'mz_planner_destroy', 'mz_planner_set_tower_precision', 'mz_planner_set_param', 'mz_planner_commit_params',
    'mz_planner_bind_param_device', 'mz_planner_refresh_params',
    'mz_planner_initial_inference', 'mz_planner_recurrent_inference', 'mz_planner_hidden_size', 'mz_planner_search',
    'mz_planner_search_scripted', 'mz_selfplay_reset', 'mz_selfplay_step', 'mz_selfplay_read', 'mz_selfplay_counters',
    'mz_selfplay_record_info',
    'mz_selfplay_attach_replay', 'mz_selfplay_reset_external', 'mz_selfplay_external_act', 'mz_selfplay_external_commit',
    'mz_selfplay_reset_catch', 'mz_selfplay_reset_breakout', 'mz_selfplay_reset_othello', 'mz_othello_debug_step', 'mz_othello_debug_mask', 'mz_othello_debug_board',
    'mz_selfplay_reset_go', 'mz_go_debug_step', 'mz_go_debug_mask', 'mz_go_debug_board', 'mz_arena_reset_go',
    'mz_arena_reset', 'mz_arena_step', 'mz_arena_read_ply', 'mz_arena_result',
    'mz_arena_reset_catch', 'mz_arena_reset_breakout', 'mz_arena_reset_othello', 'mz_arena_reset_external', 'mz_arena_external_act', 'mz_arena_external_commit',
    'mz_profile_begin', 'mz_profile_end', 'mz_planner_synchronize',
]


class PlannerError(RuntimeError):
    pass


class MzConfig(C.Structure):
    _fields_ = [
        ('net_kind', C.c_int32), ('obs_c', C.c_int32), ('obs_h', C.c_int32), ('obs_w', C.c_int32), ('num_actions', C.c_int32),
        ('num_planes', C.c_int32), ('hidden_dim', C.c_int32), ('num_res_blocks', C.c_int32), ('value_support_size', C.c_int32),
        ('reward_support_size', C.c_int32), ('num_simulations', C.c_int32), ('discount', C.c_double), ('pb_c_base', C.c_double),
        ('pb_c_init', C.c_double), ('is_board_game', C.c_int32), ('has_known_bounds', C.c_int32), ('known_bounds_min', C.c_double),
        ('known_bounds_max', C.c_double), ('root_dirichlet_alpha', C.c_double), ('root_exploration_eps', C.c_double),
        ('num_envs', C.c_int32), ('max_ties', C.c_int32), ('seed', C.c_uint64), ('legacy_scalar_promotion', C.c_int32),
        ('conv_precision', C.c_int32),
    ]


class MzRngInputs(C.Structure):
    _fields_ = [('h_noise', C.c_void_p), ('h_u_tie', C.c_void_p), ('h_u_final', C.c_void_p)]


class MzReplayRing(C.Structure):
    _fields_ = [('capacity', C.c_int64), ('state', C.c_void_p), ('action', C.c_void_p), ('pi_prob', C.c_void_p), ('value', C.c_void_p),
                ('reward', C.c_void_p), ('priority', C.c_void_p), ('num_added', C.c_void_p), ('origin', C.c_void_p),
                ('acc_seq_length', C.c_int32), ('unroll_steps', C.c_int32), ('td_steps', C.c_int32), ('state_format', C.c_int32)]


class MzExternalEnv(C.Structure):
    _fields_ = [('stack_history', C.c_int32), ('is_obs_image', C.c_int32), ('frame_c', C.c_int32), ('frame_h', C.c_int32), ('frame_w', C.c_int32),
                ('frame_u8', C.c_int32), ('max_episode_steps', C.c_int32), ('temp_switch_steps', C.c_int32), ('record_format', C.c_int32)]


class MzCatchEnv(C.Structure):
    _fields_ = [('rows', C.c_int32), ('cols', C.c_int32), ('record_format', C.c_int32)]


class MzBreakoutEnv(C.Structure):
    _fields_ = [('rows', C.c_int32), ('cols', C.c_int32), ('brick_rows', C.c_int32), ('max_moves', C.c_int32), ('record_format', C.c_int32)]


class MzConnect4Env(C.Structure):
    _fields_ = [('num_to_win', C.c_int32), ('temp_switch_steps', C.c_int32)]


class MzOthelloEnv(C.Structure):
    _fields_ = [('temp_switch_steps', C.c_int32)]


class MzGoEnv(C.Structure):
    _fields_ = [('temp_switch_steps', C.c_int32), ('komi2', C.c_int32), ('max_plies', C.c_int32), ('allow_resign', C.c_int32)]


_lib = None


def load_library():
    """dlopen the planner library and declare its prototypes.  Raises PlannerError if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise PlannerError(
            f'{LIB_PATH} not found: build it with `python -m muzero_amd.build` (hipcc, gfx950). The planning path has no CPU fallback.'
        )
    import torch  # noqa: F401  -- torch bundles its own HIP runtime: load it first so ONE libamdhip64 serves the process
    L = C.CDLL(LIB_PATH)
    vp, i32, i64p = C.c_void_p, C.c_int32, C.POINTER(C.c_int64)
    L.mz_last_error.restype = C.c_char_p
    L.mz_version.restype = C.c_char_p
    L.mz_planner_describe.restype = C.c_char_p
    L.mz_planner_describe.argtypes = [C.c_void_p]
    L.mz_planner_create.argtypes = [C.POINTER(MzConfig), C.c_int, C.POINTER(vp)]
    L.mz_planner_destroy.argtypes = [vp]
    L.mz_planner_set_tower_precision.argtypes = [vp, i32]
    L.mz_planner_set_param.argtypes = [vp, C.c_char_p, vp, i64p, i32]
    L.mz_planner_commit_params.argtypes = [vp]
    L.mz_planner_bind_param_device.argtypes = [vp, C.c_char_p, vp, i64p, i32]
    L.mz_planner_refresh_params.argtypes = [vp, vp]
    L.mz_debug_read_packed.argtypes = [vp, i32, vp, i64p, C.POINTER(C.c_char_p)]
    L.mz_debug_packed_info.argtypes = [vp, i32, i64p]
    L.mz_debug_conv3x3.argtypes = [vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp, i32, vp, C.POINTER(C.c_char_p)]
    L.mz_debug_res_tower.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, C.POINTER(C.c_char_p), C.POINTER(C.c_float)]
    L.mz_planner_initial_inference.argtypes = [vp, i32, vp, vp, vp, vp]
    L.mz_planner_recurrent_inference.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
    L.mz_planner_hidden_size.argtypes = [vp]
    L.mz_planner_hidden_size.restype = i32
    L.mz_planner_search.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, C.POINTER(MzRngInputs), vp, vp, vp, vp]
    L.mz_planner_search_scripted.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, C.POINTER(MzRngInputs), vp, vp, vp, vp, vp, vp]
    L.mz_selfplay_reset.argtypes = [vp, i32, vp]
    L.mz_selfplay_step.argtypes = [vp, C.c_double, i32]
    L.mz_selfplay_read.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.mz_selfplay_counters.argtypes = [vp, i64p]
    L.mz_selfplay_record_info.argtypes = [vp, i64p]
    L.mz_selfplay_attach_replay.argtypes = [vp, C.POINTER(MzReplayRing)]
    L.mz_selfplay_reset_external.argtypes = [vp, C.POINTER(MzExternalEnv)]
    L.mz_selfplay_external_act.argtypes = [vp, vp, vp, vp, vp, C.c_double, vp]
    L.mz_selfplay_external_commit.argtypes = [vp, vp, vp]
    L.mz_selfplay_reset_catch.argtypes = [vp, C.POINTER(MzCatchEnv)]
    L.mz_selfplay_reset_breakout.argtypes = [vp, C.POINTER(MzBreakoutEnv)]
    L.mz_arena_reset_breakout.argtypes = [vp, C.POINTER(MzBreakoutEnv), vp]
    # (the Connect Four entries: include/mzplanner.h declares them `extern int ...`, outside ABI_SYMBOLS: see the note there)
    L.mz_selfplay_reset_connect4.argtypes = [vp, C.POINTER(MzConnect4Env)]
    L.mz_connect4_debug_step.argtypes = [vp, vp]
    L.mz_connect4_debug_mask.argtypes = [vp, vp]
    L.mz_arena_reset_connect4.argtypes = [vp, C.POINTER(MzConnect4Env), i32, vp, i32]
    L.mz_selfplay_reset_othello.argtypes = [vp, C.POINTER(MzOthelloEnv)]
    L.mz_othello_debug_step.argtypes = [vp, vp]
    L.mz_othello_debug_mask.argtypes = [vp, vp]
    L.mz_othello_debug_board.argtypes = [vp, vp]
    L.mz_arena_reset_othello.argtypes = [vp, C.POINTER(MzOthelloEnv), i32, vp, i32]
    L.mz_selfplay_reset_go.argtypes = [vp, C.POINTER(MzGoEnv)]
    L.mz_go_debug_step.argtypes = [vp, vp]
    L.mz_go_debug_mask.argtypes = [vp, vp]
    L.mz_go_debug_board.argtypes = [vp, vp]
    L.mz_arena_reset_go.argtypes = [vp, C.POINTER(MzGoEnv), i32, vp, i32]
    L.mz_arena_reset.argtypes = [vp, i32, i32, vp, i32, vp]
    L.mz_arena_step.argtypes = [vp, i32]
    L.mz_arena_read_ply.argtypes = [vp] + [vp] * 9
    L.mz_arena_result.argtypes = [vp, vp, vp, vp, i64p, vp]
    L.mz_arena_reset_catch.argtypes = [vp, C.POINTER(MzCatchEnv), vp, vp]
    L.mz_arena_reset_external.argtypes = [vp, C.POINTER(MzExternalEnv)]
    L.mz_arena_external_act.argtypes = [vp, vp, vp, vp, vp, vp, vp]
    L.mz_arena_external_commit.argtypes = [vp, vp, vp]
    L.mz_profile_begin.argtypes = [vp]
    L.mz_profile_end.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.mz_planner_synchronize.argtypes = [vp]
    for name in ABI_SYMBOLS:
        fn = getattr(L, name)
        if fn.restype is C.c_int:
            fn.restype = C.c_int
    _lib = L
    return L


def _chk(rc):
    if rc != 0:
        raise PlannerError(f'mzplanner error {rc}: {load_library().mz_last_error().decode()}')


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


CONV_PRECISIONS = {'f32': 0, 'bf16x3': 1}  # MZ_CONV_F32 / MZ_CONV_BF16X3 (include/mzplanner.h)


def _conv_precision(v):
    if isinstance(v, str) and v in CONV_PRECISIONS:
        return CONV_PRECISIONS[v]
    if not isinstance(v, (str, bool)) and v in (0, 1):
        return int(v)
    raise ValueError(f"conv_precision must be 0, 1, 'f32' or 'bf16x3', not {v!r}")


TOWER_PRECISIONS = {'f32': 0, 'bf16x3': 1}  # MZ_TOWER_F32 / MZ_TOWER_BF16X3 (include/mzplanner.h)


def _tower_precision(v):
    if isinstance(v, str) and v in TOWER_PRECISIONS:
        return TOWER_PRECISIONS[v]
    if not isinstance(v, (str, bool)) and v in (0, 1):
        return int(v)
    raise ValueError(f"tower_precision must be 0, 1, 'f32' or 'bf16x3', not {v!r}")


RECORD_FORMATS = {'f32': 0, 'frames_u8': 1}  # MZ_RECORD_F32 / MZ_RECORD_FRAMES_U8 (include/mzplanner.h)


def _record_format(v):
    if isinstance(v, str) and v in RECORD_FORMATS:
        return RECORD_FORMATS[v]
    raise ValueError(f"record_format must be 'f32' or 'frames_u8', not {v!r}")


def make_mz_config(spec, config=None, num_envs=1, max_ties=0, seed=1, keep_shape=False, **search_overrides):
    """Build an mz_config from a network spec (MuZeroNet.planner_spec()) and a MuZeroConfig-like object.  MLP nets get their input
    flattened (obs_c = all elements, obs_h = obs_w = 1) unless `keep_shape`: then a [C, H, W] input keeps its shape -- the MLP kernels read
    only the product, `selfplay_reset_catch` reads the frame geometry off it."""
    shape = tuple(spec['input_shape'])
    if spec['kind'] == 'mlp' and not (keep_shape and len(shape) == 3):
        c, h, w = int(np.prod(shape)), 1, 1
    else:
        c, h, w = shape
    g = lambda name, default: search_overrides.get(name, getattr(config, name, default) if config is not None else default)  # noqa: E731
    kb = g('known_bounds', None)
    return MzConfig(
        net_kind=_NET_KINDS[spec['kind']], obs_c=c, obs_h=h, obs_w=w, num_actions=spec['num_actions'], num_planes=spec['num_planes'],
        hidden_dim=spec['hidden_dim'], num_res_blocks=spec['num_res_blocks'], value_support_size=spec['value_support_size'],
        reward_support_size=spec['reward_support_size'], num_simulations=int(g('num_simulations', 1)), discount=float(g('discount', 1.0)),
        pb_c_base=float(g('pb_c_base', 19652)), pb_c_init=float(g('pb_c_init', 1.25)), is_board_game=int(bool(g('is_board_game', False))),
        has_known_bounds=int(kb is not None), known_bounds_min=float(kb[0]) if kb is not None else 0.0,
        known_bounds_max=float(kb[1]) if kb is not None else 0.0, root_dirichlet_alpha=float(g('root_dirichlet_alpha', 0.25)),
        root_exploration_eps=float(g('root_exploration_eps', 0.25)), num_envs=int(num_envs), max_ties=int(max_ties), seed=int(seed),
        legacy_scalar_promotion=int(bool(g('legacy_scalar_promotion', False))), conv_precision=_conv_precision(g('conv_precision', 0)),
    )


def _is_tensor(t):
    import torch

    return isinstance(t, torch.Tensor)


def device_weights(state_dict, device_index, expect=None):
    """The tensors of `state_dict` a planner on GPU `device_index` can bind in place (`Planner.bind_device_weights`): every entry except
    `num_batches_tracked` must be a contiguous float32 CUDA tensor on that GPU; `expect`: keys that must be there (`num_batches_tracked`
    aside).  Returns {key: tensor}; raises ValueError naming the first key that does not qualify.  Pure: touches no GPU."""
    import torch

    out = {}
    for name, t in state_dict.items():
        if name.endswith('num_batches_tracked'):
            continue
        if not _is_tensor(t):
            raise ValueError(f'{name}: not a torch tensor ({type(t).__name__})')
        if t.device.type != 'cuda':
            raise ValueError(f'{name}: on {t.device}, not on the planner\'s GPU (cuda:{device_index})')
        if t.device.index is not None and t.device.index != device_index:
            raise ValueError(f'{name}: on {t.device}, the planner is on cuda:{device_index}')
        if t.dtype != torch.float32:
            raise ValueError(f'{name}: {t.dtype}, the planner binds float32')
        if not t.is_contiguous():
            raise ValueError(f'{name}: not contiguous')
        out[name] = t.detach()
    for name in expect or ():
        if not name.endswith('num_batches_tracked') and name not in out:
            raise ValueError(f'{name}: missing from the state_dict')
    return out


def can_bind(state_dict, device_index):
    """Whether `device_weights` accepts `state_dict` (the owners of a planner fall back to `load_state_dict` otherwise)."""
    try:
        device_weights(state_dict, device_index)
        return True
    except ValueError:
        return False


class Planner:
    """One planner handle on one GPU (mz_planner*)."""

    def __init__(self, mz_config, device_id=0, tower_precision='f32'):
        """`tower_precision` 'bf16x3': the fused residual towers on the split-bf16 kernel (mz_planner_set_tower_precision)."""
        tp = _tower_precision(tower_precision)
        self.lib = load_library()
        self.cfg = mz_config
        h = C.c_void_p()
        _chk(self.lib.mz_planner_create(C.byref(mz_config), int(device_id), C.byref(h)))
        self.h = h
        self.tower_precision = tp
        if tp:
            try:
                self.set_tower_precision(tp)
            except PlannerError:
                self.lib.mz_planner_destroy(self.h)
                self.h = None
                raise
        self.device_id = int(device_id)
        self.A = mz_config.num_actions
        self.S = mz_config.num_simulations
        self.B = mz_config.num_envs
        self.obs_dim = mz_config.obs_c * mz_config.obs_h * mz_config.obs_w
        self.hidden_size = self.lib.mz_planner_hidden_size(self.h)
        self.max_ties = mz_config.max_ties if mz_config.max_ties > 0 else 4 * self.S + 8

    def close(self):
        if getattr(self, 'h', None):
            if getattr(self, '_replay_keepalive', None) is not None:
                try:
                    self.detach_replay()  # hand write cursor and priorities back: the replay outlives this planner
                except Exception:
                    pass
            self.lib.mz_planner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tower_precision(self, precision):
        """mz_planner_set_tower_precision: legal before the first load_state_dict / refresh_weights of the handle."""
        tp = _tower_precision(precision)
        _chk(self.lib.mz_planner_set_tower_precision(self.h, tp))
        self.tower_precision = tp

    # ---- weights ----
    def load_state_dict(self, state_dict):
        if getattr(self, '_refreshed', False):  # pack kernels of a refresh may still be writing the buffers this commit fills
            self.synchronize()
            self._refreshed = False
        for name, t in state_dict.items():
            if name.endswith('num_batches_tracked'):
                continue
            a = np.ascontiguousarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype=np.float32)
            shape = (C.c_int64 * max(a.ndim, 1))(*(a.shape if a.ndim else (1,)))
            _chk(self.lib.mz_planner_set_param(self.h, name.encode(), _p(a), shape, max(a.ndim, 1)))
        _chk(self.lib.mz_planner_commit_params(self.h))

    def bind_device_weights(self, state_dict):
        """Bind `state_dict`'s tensors where they are, in this planner's GPU memory (mz_planner_bind_param_device): contiguous float32 CUDA
        tensors, e.g. `HipLearner.planner_weights()` or a module's `state_dict()`.  Nothing is copied: the planner keeps references and
        `refresh_weights` reads them.  `num_batches_tracked` is skipped; anything else that cannot be bound raises ValueError with its key."""
        w = device_weights(state_dict, self.device_id)
        for name, t in w.items():
            shape = (C.c_int64 * max(t.dim(), 1))(*(tuple(t.shape) if t.dim() else (1,)))
            _chk(self.lib.mz_planner_bind_param_device(self.h, name.encode(), C.c_void_p(t.data_ptr()), shape, max(t.dim(), 1)))
        self._bound = w
        self._bound_ptrs = {k: t.data_ptr() for k, t in w.items()}

    def refresh_weights(self, stream=None):
        """Repack the bound tensors into the planner's operand copies on the GPU (mz_planner_refresh_params), ordered after the work
        `stream` holds now and before its later work; `stream`: a torch.cuda.Stream, default torch's current stream on this GPU.  No host
        synchronisation (but see the first refresh of a binding, include/mzplanner.h)."""
        import torch

        if not getattr(self, '_bound', None):
            raise PlannerError('refresh_weights: bind_device_weights first')
        if stream is None:
            stream = torch.cuda.current_stream(self.device_id)
        _chk(self.lib.mz_planner_refresh_params(self.h, C.c_void_p(int(stream.cuda_stream))))
        self._refreshed = True

    def reload(self, state_dict, stream=None, host=False):
        """Hand `state_dict` to the planner the cheapest way it allows: bound in place and refreshed on the GPU when every tensor is a
        contiguous float32 tensor on this GPU (binding again only if an address or the key set changed), through the host
        (`load_state_dict`) otherwise or with `host=True`.  Returns 'device' or 'host'."""
        if not host and can_bind(state_dict, self.device_id):
            ptrs = {k: t.data_ptr() for k, t in state_dict.items() if not k.endswith('num_batches_tracked')}
            if ptrs != getattr(self, '_bound_ptrs', None):
                self.bind_device_weights(state_dict)
            self.refresh_weights(stream)
            return 'device'
        self.load_state_dict(state_dict)
        return 'host'

    def read_packed(self):
        """Test hook (mz_debug_read_packed): every packed weight buffer of the handle as [(label, device address, bytes)]."""
        out, i = [], 0
        while True:
            n, label, info = C.c_int64(), C.c_char_p(), (C.c_int64 * 4)()
            if self.lib.mz_debug_read_packed(self.h, i, None, C.byref(n), C.byref(label)) != 0:
                return out
            name = label.value.decode()
            buf = np.empty(n.value, np.uint8)
            _chk(self.lib.mz_debug_read_packed(self.h, i, _p(buf), None, None))
            _chk(self.lib.mz_debug_packed_info(self.h, i, info))
            out.append((name, int(info[0]), buf.tobytes()))
            i += 1

    def debug_conv3x3(self, x, weight, bias=None, rows=None, action=None, num_actions=0, cin=None, residual=None, relu=False):
        """Test hook (mz_debug_conv3x3): one 3x3 stride-1 conv layer through the planner's own packers and launcher, in this handle's
        conv_precision.  x [B, cin_real, h, w], weight [cout, cin, 3, 3], bias [cout]; rows [B]: image b is x[rows[b]], read through
        per-image pointers; action [B]: channels cin_real .. cin - 1 are the action planes of a num_actions-action net; residual
        [B, cout, h, w].  Returns (out [B, cout, h, w] float32, name of the kernel build that ran)."""
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
        i32 = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.int32)  # noqa: E731
        x, weight, bias, residual, rows, action = f32(x), f32(weight), f32(bias), f32(residual), i32(rows), i32(action)
        B, cin_real, h, w = x.shape
        cout = weight.shape[0]
        cin = cin_real if cin is None else int(cin)
        if weight.shape != (cout, cin, 3, 3) or (bias is not None and bias.shape != (cout,)) or \
                (residual is not None and residual.shape != (B, cout, h, w)) or (rows is not None and rows.shape != (B,)) or \
                (action is not None and action.shape != (B,)):
            raise ValueError('debug_conv3x3: mis-shaped argument')
        out, name = np.empty((B, cout, h, w), np.float32), C.c_char_p()
        _chk(self.lib.mz_debug_conv3x3(self.h, B, cin_real, cin, cout, h, w, _p(weight), _p(bias), _p(x), _p(rows), _p(action), int(num_actions),
                                       _p(residual), int(bool(relu)), _p(out), C.byref(name)))
        return out, name.value.decode()

    def debug_res_tower(self, x, weights, biases, timed=False):
        """Test hook (mz_debug_res_tower): one residual tower through the planner's own packers and `tower_run`, in this handle's precision
        (split-bf16 where conv_precision or tower_precision is 'bf16x3').  x [B, P, h, w], weights [n_convs, P, P, 3, 3], biases
        [n_convs, P], n_convs even.  Returns (out [B, P, h, w] float32, name of the build that ran, with G and NPT); timed=True adds the
        tower's launches in ms, between two HIP events on the planner's stream (tools/split_tower_bench.py)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        weights = np.ascontiguousarray(weights, dtype=np.float32)
        biases = np.ascontiguousarray(biases, dtype=np.float32)
        B, P, h, w = x.shape
        n = weights.shape[0]
        if weights.shape != (n, P, P, 3, 3) or biases.shape != (n, P):
            raise ValueError('debug_res_tower: mis-shaped argument')
        out, name = np.empty((B, P, h, w), np.float32), C.c_char_p()
        ms = C.c_float()
        _chk(self.lib.mz_debug_res_tower(self.h, B, P, h, w, n, _p(weights), _p(biases), _p(x), _p(out), C.byref(name), C.byref(ms) if timed else None))
        return (out, name.value.decode(), float(ms.value)) if timed else (out, name.value.decode())

    def pack_stats(self):
        """Test / measurement hook: dict(launches, bytes_read, bytes_written) of one refresh."""
        info = (C.c_int64 * 4)()
        _chk(self.lib.mz_debug_packed_info(self.h, 0, info))
        return dict(launches=int(info[1]), bytes_read=int(info[2]), bytes_written=int(info[3]))

    # ---- inference (network.py:62-111) ----
    def initial_inference(self, obs):
        obs = np.ascontiguousarray(obs, np.float32).reshape(-1, self.obs_dim)
        b = obs.shape[0]
        hidden = np.empty((b, self.hidden_size), np.float32)
        pi = np.empty((b, self.A), np.float32)
        value = np.empty(b, np.float32)
        _chk(self.lib.mz_planner_initial_inference(self.h, b, _p(obs), _p(hidden), _p(pi), _p(value)))
        return hidden, pi, value

    def recurrent_inference(self, hidden, action):
        hidden = np.ascontiguousarray(hidden, np.float32).reshape(-1, self.hidden_size)
        action = np.ascontiguousarray(action, np.int32).reshape(-1)
        b = hidden.shape[0]
        out = np.empty((b, self.hidden_size), np.float32)
        reward = np.empty(b, np.float32)
        pi = np.empty((b, self.A), np.float32)
        value = np.empty(b, np.float32)
        _chk(self.lib.mz_planner_recurrent_inference(self.h, b, _p(hidden), _p(action), _p(out), _p(reward), _p(pi), _p(value)))
        return out, reward, pi, value

    # ---- search (mcts.py:302-407) ----
    def _rng(self, b, noise, u_tie, u_final):
        if noise is None and u_tie is None and u_final is None:
            return None, ()
        u_tie_a = np.full((b, self.max_ties), 0.5, np.float64)
        if u_tie is not None:
            u = np.asarray(u_tie, np.float64).reshape(b, -1)
            n = min(u.shape[1], self.max_ties)
            u_tie_a[:, :n] = u[:, :n]
        u_final_a = np.ascontiguousarray(np.broadcast_to(0.5 if u_final is None else u_final, (b,)), np.float64)
        noise_a = None if noise is None else np.ascontiguousarray(noise, np.float64).reshape(b, self.A)
        rng = MzRngInputs(noise_a.ctypes.data if noise_a is not None else None, u_tie_a.ctypes.data, u_final_a.ctypes.data)
        return rng, (u_tie_a, u_final_a, noise_a)

    def search(self, obs, mask, current_player, opponent_player, temperature, deterministic=False, noise=None, u_tie=None, u_final=None):
        obs = np.ascontiguousarray(obs, np.float32).reshape(-1, self.obs_dim)
        b = obs.shape[0]
        mask_a = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(b, self.A)
        cur = np.ascontiguousarray(np.broadcast_to(current_player, (b,)), np.int32)
        opp = np.ascontiguousarray(np.broadcast_to(opponent_player, (b,)), np.int32)
        temp = np.ascontiguousarray(np.broadcast_to(temperature, (b,)), np.float64)
        rng, keep = self._rng(b, noise, u_tie, u_final)
        action = np.empty(b, np.int32)
        pi = np.empty((b, self.A), np.float64)
        root = np.empty(b, np.float64)
        visits = np.empty((b, self.A), np.int32)
        _chk(self.lib.mz_planner_search(
            self.h, b, _p(obs), _p(mask_a), _p(cur), _p(opp), _p(temp), int(bool(deterministic)), C.byref(rng) if rng is not None else None,
            _p(action), _p(pi), _p(root), _p(visits),
        ))
        del keep
        return dict(action=action, pi=pi, root_value=root, visits=visits)

    def search_scripted(self, pi0, values, rewards, mask, current_player, opponent_player, temperature, deterministic=False, noise=None,
                        u_tie=None, u_final=None):
        pi0 = np.ascontiguousarray(pi0, np.float32).reshape(-1, self.A)
        b = pi0.shape[0]
        values = np.ascontiguousarray(values, np.float32).reshape(b, self.S)
        rewards = np.ascontiguousarray(rewards, np.float32).reshape(b, self.S)
        mask_a = None if mask is None else np.ascontiguousarray(mask, np.uint8).reshape(b, self.A)
        cur = np.ascontiguousarray(np.broadcast_to(current_player, (b,)), np.int32)
        opp = np.ascontiguousarray(np.broadcast_to(opponent_player, (b,)), np.int32)
        temp = np.ascontiguousarray(np.broadcast_to(temperature, (b,)), np.float64)
        rng, keep = self._rng(b, noise, u_tie, u_final)
        action = np.empty(b, np.int32)
        pi = np.empty((b, self.A), np.float64)
        root = np.empty(b, np.float64)
        visits = np.empty((b, self.A), np.int32)
        tp = np.empty((b, self.S), np.int32)
        ta = np.empty((b, self.S), np.int32)
        _chk(self.lib.mz_planner_search_scripted(
            self.h, b, _p(pi0), _p(values), _p(rewards), _p(mask_a), _p(cur), _p(opp), _p(temp), int(bool(deterministic)),
            C.byref(rng) if rng is not None else None, _p(action), _p(pi), _p(root), _p(visits), _p(tp), _p(ta),
        ))
        del keep
        return dict(action=action, pi=pi, root_value=root, visits=visits, trace_parent=tp, trace_action=ta)

    # ---- device-resident self-play (pipeline.py:83-113) ----
    def selfplay_reset(self, env_kind, init_state=None):
        init = None if init_state is None else np.ascontiguousarray(init_state, np.float64).reshape(self.B, 4)
        _chk(self.lib.mz_selfplay_reset(self.h, int(env_kind), _p(init)))

    def selfplay_step(self, temperature=1.0, n_moves=1):
        _chk(self.lib.mz_selfplay_step(self.h, float(temperature), int(n_moves)))

    # ---- self-play on host-stepped environments (mz_selfplay_reset_external / _act / _commit) ----
    def selfplay_reset_external(self, stack_history=0, is_obs_image=False, frame_shape=None, frame_u8=False, max_episode_steps=0,
                                temp_switch_steps=0, record_format='f32'):
        """Start self-play on `num_envs` envs stepped by the caller.  `stack_history` 0: `external_act` gets whole observations (float32);
        S > 0: it gets the newest unstacked frame of shape `frame_shape` ([C, H, W] images, [D] vectors) and the device applies
        StackFrameAndAction(S, is_obs_image) (gym_env.py:271-353); `frame_u8`: uint8 frames scaled by 1 / 255 on the device
        (ScaledFloatFrame, gym_env.py:214-224).  `max_episode_steps` bounds the record ring when a replay is attached; `temp_switch_steps`
        is the board schedule's switch from temperature 1.0 to 0.1 (used when `external_act` gets temperature < 0).  `record_format`
        'frames_u8': the record ring keeps one uint8 frame per move instead of the float32 stacked observation (mzplanner.h
        MZ_RECORD_FRAMES_U8: stacked uint8 image frames only); `selfplay_read` and the attached `frames_u8` replay get the same bytes."""
        rfmt = _record_format(record_format)
        if frame_shape is None:
            frame_shape = (self.obs_dim,)
        fs = tuple(int(d) for d in frame_shape)
        if is_obs_image:
            if len(fs) != 3:
                raise ValueError(f'image frames are [C, H, W], got {fs}')
            c, h, w = fs
        else:
            c, h, w = int(np.prod(fs)), 1, 1
        keep = getattr(self, '_replay_keepalive', None)
        ring = None if keep is None else keep[0]._ring
        if ring is not None and getattr(ring, 'state_format', 'f32') == 'frames_u8' and stack_history > 0 and is_obs_image and \
                tuple(ring.frame_spec[:4]) != (int(stack_history), c, h, w):  # (an env without stacked image frames: the library refuses it)
            # (the kernel sizes a row from the env: a ring built for other frames would be written out of bounds)
            raise PlannerError(f'the attached replay\'s frame_spec {tuple(ring.frame_spec)} is not this env\'s (stack_history, C, H, W) = '
                               f'{(int(stack_history), c, h, w)}')
        self._ext_frame = (fs, np.uint8 if frame_u8 else np.float32)
        x = MzExternalEnv(int(stack_history), int(bool(is_obs_image)), c, h, w, int(bool(frame_u8)), int(max_episode_steps), int(temp_switch_steps), rfmt)
        _chk(self.lib.mz_selfplay_reset_external(self.h, C.byref(x)))

    def external_act(self, frames, mask, cur, opp, temperature):
        """One search over every env's current frame (see selfplay_reset_external): frames [B, ...], mask [B, A] (bool), cur / opp [B]
        player ids.  Returns the sampled actions, int32 [B]."""
        shape, dt = self._ext_frame
        B = self.B
        f = np.ascontiguousarray(frames, dt)
        if f.size != B * int(np.prod(shape)):
            raise ValueError(f'frames: expected {B} frames of shape {shape}, got an array of shape {f.shape}')
        m = np.ascontiguousarray(mask, np.uint8).reshape(B, self.A)
        c = np.ascontiguousarray(np.broadcast_to(cur, (B,)), np.int32)
        o = np.ascontiguousarray(np.broadcast_to(opp, (B,)), np.int32)
        action = np.empty(B, np.int32)
        _chk(self.lib.mz_selfplay_external_act(self.h, _p(f), _p(m), _p(c), _p(o), float(temperature), _p(action)))
        return action

    def external_commit(self, reward, done):
        """The outcome of the last `external_act`'s actions: reward [B] (float32), done [B].  An env reported done hands its reset frame
        to the next external_act."""
        r = np.ascontiguousarray(np.broadcast_to(reward, (self.B,)), np.float32)
        d = np.ascontiguousarray(np.broadcast_to(done, (self.B,)), np.uint8)
        _chk(self.lib.mz_selfplay_external_commit(self.h, _p(r), _p(d)))

    def _check_image_game_replay(self):
        """An attached frames_u8 replay must hold this planner's own frames: the kernel sizes a row from the env, so a ring built for other
        frames would be written out of bounds."""
        cfg = self.cfg
        keep = getattr(self, '_replay_keepalive', None)
        ring = None if keep is None else keep[0]._ring
        if ring is not None and getattr(ring, 'state_format', 'f32') == 'frames_u8' and cfg.obs_c % 2 == 0 and \
                tuple(ring.frame_spec[:4]) != (cfg.obs_c // 2, 1, cfg.obs_h, cfg.obs_w):
            raise PlannerError(f'the attached replay\'s frame_spec {tuple(ring.frame_spec)} is not this env\'s (stack_history, C, H, W) = '
                               f'{(cfg.obs_c // 2, 1, cfg.obs_h, cfg.obs_w)}')

    def selfplay_reset_breakout(self, rows=12, cols=12, brick_rows=3, max_moves=200, record_format='f32'):
        """Start self-play on the device Breakout env (mz_selfplay_reset_breakout; `games.BreakoutEnv` is the same game on the host): a
        `rows` x `cols` grid drawn on the planner's own frame as for `selfplay_reset_catch`, `brick_rows` rows of bricks, episodes of at
        most `max_moves` moves, 3 actions, reward 1 per brick.  `selfplay_step` then plays whole moves on the device."""
        rfmt = _record_format(record_format)
        self._check_image_game_replay()
        x = MzBreakoutEnv(int(rows), int(cols), int(brick_rows), int(max_moves), rfmt)
        _chk(self.lib.mz_selfplay_reset_breakout(self.h, C.byref(x)))

    def arena_reset_breakout(self, rows=12, cols=12, brick_rows=3, max_moves=200, start_codes=None):
        """Start `num_envs` evaluation games of the device Breakout env (mz_arena_reset_breakout; geometry as `selfplay_reset_breakout`).
        Env e starts from start code `start_codes[e]` (default e % (2 * cols): every ball column and both directions equally often).
        `arena_step` then plays whole plies on the device; a game's return is the number of bricks it broke."""
        sc = None if start_codes is None else np.ascontiguousarray(start_codes, np.int32).reshape(self.B)
        x = MzBreakoutEnv(int(rows), int(cols), int(brick_rows), int(max_moves), 0)
        _chk(self.lib.mz_arena_reset_breakout(self.h, C.byref(x), _p(sc)))
        self._arena_opponent = None

    def selfplay_reset_catch(self, rows=12, cols=12, record_format='f32'):
        """Start self-play on the device Catch env (mz_selfplay_reset_catch; `games.CatchEnv` is the same game on the host): a `rows` x
        `cols` grid drawn on the planner's own frame (obs_c = 2 * stack_history, obs_h x obs_w pixels, cells of obs_h / rows x obs_w / cols),
        3 actions.  `selfplay_step` then plays whole moves on the device.  `record_format` as in `selfplay_reset_external`."""
        rfmt = _record_format(record_format)
        self._check_image_game_replay()
        x = MzCatchEnv(int(rows), int(cols), rfmt)
        _chk(self.lib.mz_selfplay_reset_catch(self.h, C.byref(x)))

    def selfplay_reset_connect4(self, num_to_win=4, temp_switch_steps=0):
        """Start self-play on the device Connect Four env (mz_selfplay_reset_connect4; `games.ConnectFourEnv` is the same game on the host):
        the board is the planner's own (9, rows, cols) input, `num_actions` = cols + 1.  `temp_switch_steps`: the board temperature
        schedule's switch from 1.0 to 0.1 (0: 6).  `selfplay_step` then plays whole moves on the device."""
        x = MzConnect4Env(int(num_to_win), int(temp_switch_steps))
        _chk(self.lib.mz_selfplay_reset_connect4(self.h, C.byref(x)))

    def debug_connect4_step(self, actions):
        """Test hook (mz_connect4_debug_step): one move of all envs with `actions` [B] through the launches of a self-play move, without
        the search; the recorded policy is the one-hot of the action, the root value 0.  An illegal action raises before any launch."""
        a = np.ascontiguousarray(actions, np.int32).reshape(self.B)
        _chk(self.lib.mz_connect4_debug_step(self.h, _p(a)))

    def debug_connect4_mask(self):
        """Test hook (mz_connect4_debug_mask): the device Connect Four envs' legal-action masks, uint8 [B, A]."""
        m = np.empty((self.B, self.A), np.uint8)
        _chk(self.lib.mz_connect4_debug_mask(self.h, _p(m)))
        return m

    def selfplay_reset_othello(self, temp_switch_steps=0):
        """Start self-play on the device Othello env (mz_selfplay_reset_othello; `games.OthelloEnv` is the same game on the host): the
        board is the planner's own (9, rows, cols) input, rows and cols in 4..8, `num_actions` = rows * cols + 2 (placements, pass,
        resign).  `temp_switch_steps`: the board temperature schedule's switch from 1.0 to 0.1 (0: 6)."""
        x = MzOthelloEnv(int(temp_switch_steps))
        _chk(self.lib.mz_selfplay_reset_othello(self.h, C.byref(x)))

    def debug_othello_step(self, actions):
        """Test hook (mz_othello_debug_step): one move of all envs with `actions` [B] through the launches of a self-play move, without
        the search; the recorded policy is the one-hot of the action, the root value 0.  An illegal action raises before any launch."""
        a = np.ascontiguousarray(actions, np.int32).reshape(self.B)
        _chk(self.lib.mz_othello_debug_step(self.h, _p(a)))

    def debug_othello_mask(self):
        """Test hook (mz_othello_debug_mask): the device Othello envs' legal-action masks, uint8 [B, A]."""
        m = np.empty((self.B, self.A), np.uint8)
        _chk(self.lib.mz_othello_debug_mask(self.h, _p(m)))
        return m

    def debug_othello_board(self):
        """Test hook (mz_othello_debug_board): the device Othello envs' boards, int8 [B, rows * cols] (0 empty, 1 black, 2 white); in an
        arena a finished game's row is its frozen final board."""
        b = np.empty((self.B, self.obs_dim // 9), np.int8)
        _chk(self.lib.mz_othello_debug_board(self.h, _p(b)))
        return b

    def selfplay_reset_go(self, komi2=15, max_plies=0, allow_resign=True, temp_switch_steps=0):
        """Start self-play on the device Go env (mz_selfplay_reset_go; `games.GoEnv` is the same game on the host): the board is the
        planner's own (9, rows, cols) input, rows and cols in 3..19 (square above 64 points), `num_actions` = rows * cols + 2
        (placements, pass, resign).  `komi2`: twice the komi; `max_plies`: the ply that ends the game by the count (0: 2 * rows * cols);
        `allow_resign` False: the resignation is never legal; `temp_switch_steps`: the board temperature schedule's switch from 1.0 to
        0.1 (0: 6)."""
        x = MzGoEnv(int(temp_switch_steps), int(komi2), int(max_plies), int(bool(allow_resign)))
        _chk(self.lib.mz_selfplay_reset_go(self.h, C.byref(x)))

    def debug_go_step(self, actions):
        """Test hook (mz_go_debug_step): one move of all envs with `actions` [B] through the launches of a self-play move, without the
        search; the recorded policy is the one-hot of the action, the root value 0.  An illegal action raises before any launch."""
        a = np.ascontiguousarray(actions, np.int32).reshape(self.B)
        _chk(self.lib.mz_go_debug_step(self.h, _p(a)))

    def debug_go_mask(self):
        """Test hook (mz_go_debug_mask): the device Go envs' legal-action masks, uint8 [B, A]."""
        m = np.empty((self.B, self.A), np.uint8)
        _chk(self.lib.mz_go_debug_mask(self.h, _p(m)))
        return m

    def debug_go_board(self):
        """Test hook (mz_go_debug_board): the device Go envs' boards, int8 [B, rows * cols] (0 empty, 1 black, 2 white); in an arena a
        finished game's row is its frozen final board, captures included."""
        b = np.empty((self.B, self.obs_dim // 9), np.int8)
        _chk(self.lib.mz_go_debug_board(self.h, _p(b)))
        return b

    def selfplay_read(self, n_moves, fields=None):
        """Records of the last `n_moves` moves, arrays [n_moves, B, ...].  `fields`: subset of ('obs', 'action', 'reward', 'pi',
        'root_value', 'player', 'done') to copy out (default all): with the device epilogue attached a host loop only needs
        rewards and done flags for its episode statistics."""
        B, A, D = self.B, self.A, self.obs_dim
        spec = dict(obs=((n_moves, B, D), np.float32), action=((n_moves, B), np.int32), reward=((n_moves, B), np.float32),
                    pi=((n_moves, B, A), np.float64), root_value=((n_moves, B), np.float64), player=((n_moves, B), np.int32),
                    done=((n_moves, B), np.uint8))
        want = set(spec) if fields is None else set(fields)
        out = {k: np.empty(shp, dt) for k, (shp, dt) in spec.items() if k in want}
        ptr = [(_p(out[k]) if k in out else None) for k in ('obs', 'action', 'reward', 'pi', 'root_value', 'player', 'done')]
        _chk(self.lib.mz_selfplay_read(self.h, n_moves, *ptr))
        return out

    def attach_replay(self, replay, config, obs_shape=None, with_origin=False):
        """Device epilogue (mz_selfplay_attach_replay): finished trajectories become (Transition, priority) items in `replay`
        -- a `muzero_amd.replay.PrioritizedReplay(device='cuda')` -- on the GPU, with the reference's target / unroll-window
        arithmetic (pipeline.py:118-165, 632-767); the host only reads `replay.num_added`.  `config` supplies acc_seq_length,
        unroll_steps, td_steps.  Call before `selfplay_reset`.  `with_origin`: also record which env produced each item
        (returned tensor; tests).  A replay built with `state_format='int8'` / `'frames_u8'` gets its states in that exact compact form
        (mzplanner.h MZ_STATE_*); the env's reset refuses a format its observations do not fit."""
        import torch

        from muzero_amd.replay import STATE_FORMATS, state_row_bytes

        K, A = int(config.unroll_steps), self.A
        shp = tuple(obs_shape) if obs_shape is not None else (self.obs_dim,)
        adt = torch.int8 if A <= 128 else torch.int16  # (int16 where the reference's int8 field overflows: pipeline.py:753, Gomoku 15x15)
        if replay._ring is None:
            replay.allocate(dict(state=shp, action=(K,), pi_prob=(K, A), value=(K,), reward=(K,)), dict(action=adt))
        ring = replay._ring
        fmt = getattr(ring, 'state_format', 'f32')
        sdt = {'f32': torch.float32, 'int8': torch.int8, 'frames_u8': torch.uint8}[fmt]
        if ring['state'].device.type != 'cuda' or ring['state'].dtype != sdt or ring['action'].dtype != adt:
            raise PlannerError(f'attach_replay needs a replay on the GPU with float32 states and {adt} actions ({A} actions)' if fmt == 'f32' else
                               f'attach_replay needs a replay on the GPU; state_format {fmt!r} stores {sdt} states and {adt} actions ({A} actions)')
        if fmt == 'frames_u8':
            S, Cf, H, W, Af = ring.frame_spec
            if Af != A or S * (Cf + 1) * H * W != self.obs_dim:
                raise PlannerError(f'replay frame_spec {ring.frame_spec} does not match the planner ({self.obs_dim} observation elements, {A} actions)')
            state_elems = self.obs_dim if tuple(ring['state'].shape[1:]) == (state_row_bytes(fmt, (self.obs_dim,), ring.frame_spec),) else -1
        else:
            state_elems = int(np.prod(ring['state'].shape[1:]))
        if state_elems != self.obs_dim or tuple(ring['pi_prob'].shape[1:]) != (K, A):
            raise PlannerError('replay item shapes do not match the planner (observation size, unroll_steps, num_actions)')
        prio, count = replay.attach_device_writer()
        origin = torch.full((replay.capacity,), -1, dtype=torch.int32, device=ring['state'].device) if with_origin else None
        r = MzReplayRing(replay.capacity, ring['state'].data_ptr(), ring['action'].data_ptr(), ring['pi_prob'].data_ptr(), ring['value'].data_ptr(),
                         ring['reward'].data_ptr(), prio.data_ptr(), count.data_ptr(), origin.data_ptr() if with_origin else None,
                         int(config.acc_seq_length), K, int(config.td_steps), STATE_FORMATS[fmt])
        torch.cuda.synchronize()
        _chk(self.lib.mz_selfplay_attach_replay(self.h, C.byref(r)))
        self._replay_keepalive = (replay, prio, count, origin)
        return origin

    def detach_replay(self):
        """Drains the planner's stream, detaches the epilogue and hands counter / priorities back to the replay's host side."""
        _chk(self.lib.mz_selfplay_attach_replay(self.h, None))
        if self._replay_keepalive is not None:
            self._replay_keepalive[0].detach_device_writer()
        self._replay_keepalive = None

    # ---- arena: evaluation games in lock-step (mz_arena_*; pipeline.py:289-397, 400-488) ----
    def arena_reset(self, env_kind, opponent=None, opening_plies=0, init_state=None):
        """Start `num_envs` evaluation games on the device env `env_kind`.  `opponent`: None (one-player envs), 'random', or a second
        `Planner` on the same GPU with the same configuration (apart from the seed) and loaded weights -- it is borrowed until this
        planner's next reset or close, and kept alive here.  Two-player envs: the challenger (this planner) is black in envs [0, B/2) and
        white in [B/2, B); the first `opening_plies` plies are random moves shared by env i and env i + B/2."""
        if opponent is None:
            kind, q = ARENA_NONE, None
        elif isinstance(opponent, str):
            if opponent != 'random':
                raise ValueError(f"opponent must be None, 'random' or a Planner, got {opponent!r}")
            kind, q = ARENA_RANDOM, None
        elif isinstance(opponent, Planner):
            kind, q = ARENA_PLANNER, opponent
        else:
            raise ValueError(f"opponent must be None, 'random' or a Planner, got {opponent!r}")
        init = None if init_state is None else np.ascontiguousarray(init_state, np.float64).reshape(self.B, 4)
        _chk(self.lib.mz_arena_reset(self.h, int(env_kind), kind, q.h if q is not None else None, int(opening_plies), _p(init)))
        self._arena_opponent = q

    def arena_reset_connect4(self, opponent, opening_plies=0, num_to_win=4):
        """Start `num_envs` evaluation games of the device Connect Four env (mz_arena_reset_connect4): `arena_reset`'s two-player arena
        -- `opponent` 'random' or a second `Planner`, colours balanced over the two halves, paired random openings -- on this game.
        Random moves are drawn from the legal columns only: they never resign."""
        if isinstance(opponent, Planner):
            kind, q = ARENA_PLANNER, opponent
        elif opponent == 'random':
            kind, q = ARENA_RANDOM, None
        else:
            raise ValueError(f"opponent must be 'random' or a Planner, got {opponent!r}")
        x = MzConnect4Env(int(num_to_win), 0)
        _chk(self.lib.mz_arena_reset_connect4(self.h, C.byref(x), kind, q.h if q is not None else None, int(opening_plies)))
        self._arena_opponent = q

    def arena_reset_othello(self, opponent, opening_plies=0):
        """Start `num_envs` evaluation games of the device Othello env (mz_arena_reset_othello): `arena_reset`'s two-player arena --
        `opponent` 'random' or a second `Planner`, colours balanced over the two halves, paired random openings -- on this game.  Random
        moves are drawn from the legal placements, or are the pass where there is none: they never resign."""
        if isinstance(opponent, Planner):
            kind, q = ARENA_PLANNER, opponent
        elif opponent == 'random':
            kind, q = ARENA_RANDOM, None
        else:
            raise ValueError(f"opponent must be 'random' or a Planner, got {opponent!r}")
        x = MzOthelloEnv(0)
        _chk(self.lib.mz_arena_reset_othello(self.h, C.byref(x), kind, q.h if q is not None else None, int(opening_plies)))
        self._arena_opponent = q

    def arena_reset_go(self, opponent, opening_plies=0, komi2=15, max_plies=0, allow_resign=True):
        """Start `num_envs` evaluation games of the device Go env (mz_arena_reset_go): `arena_reset`'s two-player arena -- `opponent`
        'random' or a second `Planner`, colours balanced over the two halves, paired random openings -- on this game, with
        `selfplay_reset_go`'s rules.  Random moves are drawn from the legal placements and the pass: they never resign."""
        if isinstance(opponent, Planner):
            kind, q = ARENA_PLANNER, opponent
        elif opponent == 'random':
            kind, q = ARENA_RANDOM, None
        else:
            raise ValueError(f"opponent must be 'random' or a Planner, got {opponent!r}")
        x = MzGoEnv(0, int(komi2), int(max_plies), int(bool(allow_resign)))
        _chk(self.lib.mz_arena_reset_go(self.h, C.byref(x), kind, q.h if q is not None else None, int(opening_plies)))
        self._arena_opponent = q

    def arena_reset_catch(self, rows=12, cols=12, ball_cols=None, start_rows=None):
        """Start `num_envs` evaluation games of the device Catch env (mz_arena_reset_catch; geometry as `selfplay_reset_catch`).  Env e
        starts with the paddle at cols // 2 and the ball in column `ball_cols[e]` (default e % cols: every column equally often) and row
        `start_rows[e]` (default 0; 0 .. rows - 2).  `arena_step` then plays whole plies on the device."""
        bc = None if ball_cols is None else np.ascontiguousarray(ball_cols, np.int32).reshape(self.B)
        sr = None if start_rows is None else np.ascontiguousarray(start_rows, np.int32).reshape(self.B)
        x = MzCatchEnv(int(rows), int(cols), 0)
        _chk(self.lib.mz_arena_reset_catch(self.h, C.byref(x), _p(bc), _p(sr)))
        self._arena_opponent = None

    def arena_reset_external(self, stack_history=0, is_obs_image=False, frame_shape=None, frame_u8=False, max_episode_steps=0):
        """Start `num_envs` evaluation games on envs stepped by the caller (mz_arena_reset_external).  The frames are described as for
        `selfplay_reset_external`; `arena_external_act` / `arena_external_commit` play a ply around the caller's env.step."""
        if frame_shape is None:
            frame_shape = (self.obs_dim,)
        fs = tuple(int(d) for d in frame_shape)
        if is_obs_image:
            if len(fs) != 3:
                raise ValueError(f'image frames are [C, H, W], got {fs}')
            c, h, w = fs
        else:
            c, h, w = int(np.prod(fs)), 1, 1
        x = MzExternalEnv(int(stack_history), int(bool(is_obs_image)), c, h, w, int(bool(frame_u8)), int(max_episode_steps), 0, 0)
        _chk(self.lib.mz_arena_reset_external(self.h, C.byref(x)))
        self._arena_frame = (fs, np.uint8 if frame_u8 else np.float32)
        self._arena_opponent = None

    def arena_external_act(self, frames, mask, cur, opp):
        """One deterministic search over every env's newest frame (see arena_reset_external): frames [B, ...], mask [B, A], cur / opp [B]
        player ids; the entries of finished (frozen) envs are ignored.  Returns (actions int32 [B], live uint8 [B]): step env e with
        actions[e] where live[e] is 1."""
        shape, dt = self._arena_frame
        B = self.B
        f = np.ascontiguousarray(frames, dt)
        if f.size != B * int(np.prod(shape)):
            raise ValueError(f'frames: expected {B} frames of shape {shape}, got an array of shape {f.shape}')
        m = np.ascontiguousarray(mask, np.uint8).reshape(B, self.A)
        c = np.ascontiguousarray(np.broadcast_to(cur, (B,)), np.int32)
        o = np.ascontiguousarray(np.broadcast_to(opp, (B,)), np.int32)
        action, live = np.empty(B, np.int32), np.empty(B, np.uint8)
        _chk(self.lib.mz_arena_external_act(self.h, _p(f), _p(m), _p(c), _p(o), _p(action), _p(live)))
        return action, live

    def arena_external_commit(self, reward, done):
        """The outcome of the last `arena_external_act`'s actions on the live envs: reward [B] (float32), done [B] (frozen envs' entries
        are ignored).  A done env is frozen and tallied."""
        r = np.ascontiguousarray(np.broadcast_to(reward, (self.B,)), np.float32)
        d = np.ascontiguousarray(np.broadcast_to(done, (self.B,)), np.uint8)
        _chk(self.lib.mz_arena_external_commit(self.h, _p(r), _p(d)))

    def arena_step(self, n_plies=1):
        """`n_plies` lock-step plies, enqueued without a host synchronisation."""
        _chk(self.lib.mz_arena_step(self.h, int(n_plies)))

    def arena_read_ply(self):
        """The last ply per env: dict(obs, mask, player -- the root before the move; side (SIDE_*), pi, root_value, action, u -- the move;
        live -- 1 where the env was live when the ply began, elsewhere the other fields are those of its last ply)."""
        B, A, D = self.B, self.A, self.obs_dim
        out = dict(obs=np.empty((B, D), np.float32), mask=np.empty((B, A), np.uint8), player=np.empty(B, np.int32), side=np.empty(B, np.int32),
                   pi=np.empty((B, A), np.float64), root_value=np.empty(B, np.float64), action=np.empty(B, np.int32), u=np.empty(B, np.float64),
                   live=np.empty(B, np.uint8))
        _chk(self.lib.mz_arena_read_ply(self.h, *[_p(out[k]) for k in ('obs', 'mask', 'player', 'side', 'pi', 'root_value', 'action', 'u', 'live')]))
        return out

    def arena_result(self):
        """The tally: dict(winner [B] (ARENA_*), length [B], ret [B], challenger_wins, opponent_wins, draws, finished_plies, live)."""
        B = self.B
        winner, length, ret = np.empty(B, np.int32), np.empty(B, np.int32), np.empty(B, np.float64)
        totals, live = (C.c_int64 * 4)(), C.c_int32()
        _chk(self.lib.mz_arena_result(self.h, _p(winner), _p(length), _p(ret), totals, C.cast(C.byref(live), C.c_void_p)))
        return dict(winner=winner, length=length, ret=ret, challenger_wins=int(totals[0]), opponent_wins=int(totals[1]), draws=int(totals[2]),
                    finished_plies=int(totals[3]), live=int(live.value))

    def record_info(self):
        """The record ring as the last reset sized it (mz_selfplay_record_info): dict(format ('f32' / 'frames_u8'), ring_len (moves),
        bytes_per_move (one move's observation or frame records), bytes (all record arrays))."""
        c = (C.c_int64 * 4)()
        _chk(self.lib.mz_selfplay_record_info(self.h, c))
        return dict(format={v: k for k, v in RECORD_FORMATS.items()}[int(c[0])], ring_len=int(c[1]), bytes_per_move=int(c[2]), bytes=int(c[3]))

    def selfplay_counters(self):
        c = (C.c_int64 * 4)()
        _chk(self.lib.mz_selfplay_counters(self.h, c))
        return dict(env_steps=c[0], simulations=c[1], episodes=c[2], episode_steps=c[3])

    # ---- measurement ----
    def synchronize(self):
        _chk(self.lib.mz_planner_synchronize(self.h))

    def profile_begin(self):
        _chk(self.lib.mz_profile_begin(self.h))

    def describe(self) -> str:
        """The kernel build the last search launch dispatched to + the diagnostic switches as this handle read them (mz_planner_describe)."""
        return self.lib.mz_planner_describe(self.h).decode()

    def profile_end(self):
        ms, kms, n = C.c_double(), C.c_double(), C.c_int64()
        _chk(self.lib.mz_profile_end(self.h, C.byref(ms), C.byref(kms), C.byref(n)))
        return dict(elapsed_ms=ms.value, search_kernel_ms=kms.value, search_kernel_launches=n.value)


class InferenceEngine:
    """Planner used only for MuZeroNet.initial_inference / recurrent_inference (network.py:62-111)."""

    def __init__(self, spec, device=None, num_envs=16):
        idx = 0
        if device is not None and getattr(device, 'type', 'cuda') != 'cuda':
            raise PlannerError(f'initial/recurrent inference run on the HIP planner only; got device {device} (no CPU fallback)')
        if device is not None and getattr(device, 'index', None) is not None:
            idx = device.index
        self.planner = Planner(make_mz_config(spec, None, num_envs=num_envs), idx)

    def load_state_dict(self, sd):
        self.planner.load_state_dict(sd)

    def reload(self, sd):
        return self.planner.reload(sd)

    def initial_inference(self, obs):
        return self.planner.initial_inference(obs)

    def recurrent_inference(self, hidden, action):
        return self.planner.recurrent_inference(hidden, action)
