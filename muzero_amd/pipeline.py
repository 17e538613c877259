"""Host-side mirror of the self-play half of muzero/pipeline.py.

The reference runs one Python actor process per environment (pipeline.py:41-167): per step a `uct_search`, an
`env.step`, a trajectory append, and at episode end target computation + `make_unroll_sequence` + `data_queue.put`.
Here the per-step part (search, action sampling, env.step, record, auto-reset) is one lock-step move of thousands of
device-resident environments inside the HIP planner (`mz_selfplay_step`); this module only drains the device record
ring, cuts it into episodes and emits the same `(Transition, priority)` stream.

Functions with a reference counterpart keep its name, arguments and error behaviour:
compute_n_step_target (pipeline.py:632-673), compute_mc_return_target (:676-707), make_unroll_sequence (:710-767),
create_checkpoint / load_checkpoint (:802-807), run_self_play (:41-167).
"""
import collections
import copy
import os
import time
from typing import Any, Iterable, List, Mapping, NamedTuple, Optional, Text

import numpy as np


class Transition(NamedTuple):
    """Same fields, same order as replay.py:27-32 (the wire format between actors and the learner)."""
    state: Optional[np.ndarray]
    action: Optional[np.ndarray]
    pi_prob: Optional[np.ndarray]
    value: Optional[np.ndarray]
    reward: Optional[np.ndarray]


def compute_n_step_target(rewards: List[float], root_values: List[float], td_steps: int, discount: float) -> List[float]:
    """z_t = sum_{i<n} discount^i r_{t+i} + discount^n v_{t+n}, zero padded past the end (pipeline.py:632-673).
    Sums run left to right in float64 like the reference's Python `sum`, so results are bit-identical."""
    if len(rewards) != len(root_values):
        raise ValueError('Arguments `rewards` and `root_values` don have the same length.')
    T = len(rewards)
    r = list(rewards) + [0] * td_steps
    v = list(root_values) + [0] * td_steps
    pw = [discount**i for i in range(td_steps + 1)]
    out = []
    for t in range(T):
        acc = 0
        for i in range(td_steps):
            acc = acc + pw[i] * r[t + i]
        out.append(acc + pw[td_steps] * v[t + td_steps])
    return out


def compute_mc_return_target(rewards: List[float], player_ids: List[float]) -> List[float]:
    """Board games: +/- final reward from each mover's perspective, all zeros for a draw (pipeline.py:676-707)."""
    if len(rewards) != len(player_ids):
        raise ValueError('Arguments `rewards` and `player_ids` don have the same length.')
    T = len(rewards)
    out = [0.0] * T
    final_reward, final_player = rewards[-1], player_ids[-1]
    if final_reward != 0.0:
        for t in range(T):
            out[t] = final_reward if player_ids[t] == final_player else -final_reward
    return out


def make_unroll_sequence(observations, actions, rewards, pi_probs, values, priorities, unroll_steps) -> Iterable:
    """Yield (Transition, priority) per step with K-step stacked action / reward / value / policy; steps past the end are
    absorbing (action 0, reward 0, value 0, uniform policy) (pipeline.py:710-767).

    Differences from the reference, both deliberate: the caller's lists are NOT mutated (the reference extends them in
    place, pipeline.py:739-747), and actions are stored as int8 only when they fit (A <= 128) -- the reference's
    unconditional int8 cannot represent Gomoku 15x15 actions; larger action spaces get int16."""
    T = len(observations)
    K = unroll_steps
    n_act = len(pi_probs[-1])
    acts = list(actions) + ([0] * K if len(actions) == T else [])
    rews = list(rewards) + ([0] * K if len(rewards) == T else [])
    vals = list(values) + ([0] * K if len(values) == T else [])
    pis = list(pi_probs) + ([np.ones_like(pi_probs[-1]) / n_act] * K if len(pi_probs) == T else [])
    assert len(acts) == len(rews) == len(vals) == len(pis) == T + K
    act_dtype = np.int8 if n_act <= 128 else np.int16
    for t in range(T):
        yield (
            Transition(
                state=observations[t],
                action=np.array(acts[t:t + K], dtype=act_dtype),
                reward=np.array(rews[t:t + K], dtype=np.float32),
                value=np.array(vals[t:t + K], dtype=np.float32),
                pi_prob=np.array(pis[t:t + K], dtype=np.float32),
            ),
            priorities[t],
        )


def _compact(obj):
    """Tensors that are views of a larger storage are cloned: torch.save writes a tensor's WHOLE storage, and the parameters of a module that
    hip_learner.HipLearner adopted are views of one flat vector that also holds Adam's moments and the gradient slices -- a checkpoint of such
    a module would otherwise carry that vector (4x-33x the weights) inside its 'network' entry."""
    import torch

    if torch.is_tensor(obj):
        return obj.detach().clone() if obj.untyped_storage().nbytes() > obj.numel() * obj.element_size() else obj
    # only plain containers are rebuilt; everything else (namedtuples, defaultdicts, user classes) passes through unchanged.  An OrderedDict --
    # network.state_dict() -- is shallow-copied and its values replaced in place, so its `_metadata` attribute (the per-module version
    # info torch.save writes and load_state_dict reads) stays with it
    if isinstance(obj, dict) and type(obj) in (dict, collections.OrderedDict):
        out = copy.copy(obj)
        for k, v in obj.items():
            out[k] = _compact(v)
        if hasattr(obj, '_metadata'):
            out._metadata = obj._metadata
        return out
    if type(obj) in (list, tuple):
        return type(obj)(_compact(v) for v in obj)
    return obj


def create_checkpoint(state_to_save: Mapping[Text, Any], ckpt_file: str) -> None:
    """pipeline.py:802-803: torch.save of {'network', 'optimizer', 'lr_scheduler', 'train_steps'}."""
    import torch

    torch.save(_compact(state_to_save), ckpt_file)


def load_checkpoint(ckpt_file: str, device) -> Mapping[Text, Any]:
    """pipeline.py:806-807 (weights_only=False: the reference checkpoints hold optimizer / scheduler state dicts)."""
    import torch

    return torch.load(ckpt_file, map_location=torch.device(device), weights_only=False)


# ------------------------------------------------------------------------------------------------------------------
# multi-GPU sharding: environments are independent, so ranks own disjoint env ranges and never exchange data
# ------------------------------------------------------------------------------------------------------------------
def shard_range(total_envs: int, rank: int, world_size: int):
    """Contiguous env id range [lo, hi) of `rank` (sizes differ by at most one)."""
    if not 0 <= rank < world_size:
        raise ValueError(f'rank {rank} outside world of size {world_size}')
    base, extra = divmod(total_envs, world_size)
    lo = rank * base + min(rank, extra)
    return lo, lo + base + (1 if rank < extra else 0)


def aggregate_throughput(local_units: float, local_seconds: float):
    """Whole-job rate: total units of all ranks / slowest rank's time (the bench.py contract).  Uses the default
    torch.distributed group when initialised (RCCL on GPUs, gloo in the CPU tests); a single process otherwise."""
    import torch
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        return local_units / local_seconds, local_units, local_seconds
    dev = 'cuda' if dist.get_backend() == 'nccl' else 'cpu'
    units = torch.tensor([float(local_units)], dtype=torch.float64, device=dev)
    secs = torch.tensor([float(local_seconds)], dtype=torch.float64, device=dev)
    dist.all_reduce(units, op=dist.ReduceOp.SUM)
    dist.all_reduce(secs, op=dist.ReduceOp.MAX)
    return float(units.item() / secs.item()), float(units.item()), float(secs.item())


def weights_key(network, train_steps_counter=None, config=None):
    """What an actor watches to know that the learner refreshed `network` (pipeline.py:261-267: every checkpoint_interval
    train steps).  In one process the tensors' version counters change; in another process (the reference's layout:
    shared-memory parameters, mp.Process actors) only the storage changes, so the signal that travels is the network's
    `weights_epoch` -- a shared-memory buffer the learner bumps AFTER `load_state_dict` (`MuZeroNet.publish_weights`).
    (Round 2 keyed on the train-step counter crossing a checkpoint_interval boundary: that fires BEFORE the learner has
    written the checkpoint and copied the weights, so a remote actor reloaded the old values and stayed one checkpoint
    behind.)  `train_steps_counter` / `config` are accepted for the old call sites and ignored."""
    epoch = getattr(network, 'weights_epoch', None)
    return network._weights_version(), (int(epoch.item()) if epoch is not None else 0)


# ------------------------------------------------------------------------------------------------------------------
# self-play actor over the device-resident planner
# ------------------------------------------------------------------------------------------------------------------
class EpisodeAssembler:
    """Cuts the lock-step record stream [moves, envs, ...] into per-env episodes and turns finished episodes into
    (Transition, priority) items exactly like pipeline.py:144-165."""

    def __init__(self, config, num_envs: int, obs_shape=None):
        self.config = config
        self.open = [[] for _ in range(num_envs)]
        self.obs_shape = None if obs_shape is None else tuple(obs_shape)  # the env's observation shape (records are flat rows)

    def feed(self, rec) -> Iterable:
        cfg = self.config
        n_moves, B = rec['action'].shape
        for m in range(n_moves):
            for b in range(B):
                o = rec['obs'][m, b] if self.obs_shape is None else rec['obs'][m, b].reshape(self.obs_shape)
                self.open[b].append((o, int(rec['action'][m, b]), float(rec['reward'][m, b]), rec['pi'][m, b],
                                     float(rec['root_value'][m, b]), int(rec['player'][m, b])))
                # same order as the reference's loop body: the mid-episode flush check first (pipeline.py:118-142), then the
                # end of the episode (:144-165) -- when both fall on one step the prefix is flushed and the rest finishes
                if (not cfg.is_board_game) and len(self.open[b]) == cfg.acc_seq_length + cfg.unroll_steps + cfg.td_steps:
                    yield from self._flush_prefix(b)
                if rec['done'][m, b]:
                    traj, self.open[b] = self.open[b], []
                    yield from self._finish(traj)

    def _finish(self, traj):
        cfg = self.config
        obs, actions, rewards, pis, roots, players = map(list, zip(*traj))
        if cfg.is_board_game:
            targets = compute_mc_return_target(rewards, players)
        else:
            targets = compute_n_step_target(rewards, roots, cfg.td_steps, cfg.discount)
        prios = np.abs(np.array(roots) - np.array(targets))
        yield from make_unroll_sequence(obs, actions, rewards, pis, targets, prios, cfg.unroll_steps)

    def _flush_prefix(self, b):
        cfg = self.config
        n = cfg.acc_seq_length
        obs, actions, rewards, pis, roots, _ = map(list, zip(*self.open[b]))
        targets = compute_n_step_target(rewards, roots, cfg.td_steps, cfg.discount)
        prios = np.abs(np.array(roots) - np.array(targets))
        k = n + cfg.unroll_steps
        yield from make_unroll_sequence(obs[:n], actions[:k], rewards[:k], pis[:k], targets[:k], prios[:k], cfg.unroll_steps)
        del self.open[b][:n]


DEVICE_ENVS = ('CartPole-v1', 'TicTacToe', 'Gomoku', 'Synthetic-Atari', 'Catch', 'Breakout', 'ConnectFour', 'Othello', 'Go')


def _catch_args(env) -> dict:
    """The grid of a `games.CatchEnv` (or a wrapper of one) as the planner's Catch resets take it; the defaults for a name."""
    return dict(rows=int(getattr(env, 'rows', 12)), cols=int(getattr(env, 'cols', 12)))


def _breakout_args(env) -> dict:
    """The grid of a `games.BreakoutEnv` (or a wrapper of one) as the planner's Breakout resets take it; the defaults for a name."""
    return dict(rows=int(getattr(env, 'rows', 12)), cols=int(getattr(env, 'cols', 12)), brick_rows=int(getattr(env, 'brick_rows', 3)),
                max_moves=int(getattr(env, 'max_moves', 200)))


# Device envs drawn on the network's own frame (the planner keeps the [C, H, W] input shape): name -> (the reset arguments off an env object
# or the defaults, the planner's self-play reset, its arena reset, the env's own move cap from those arguments)
IMAGE_GAMES = {
    'Catch': (_catch_args, 'selfplay_reset_catch', 'arena_reset_catch', lambda args: args['rows'] - 1),
    'Breakout': (_breakout_args, 'selfplay_reset_breakout', 'arena_reset_breakout', lambda args: args['max_moves']),
}


def _connect4_num_to_win(env, config) -> int:
    """Stones in a line that win Connect Four: off a `games.ConnectFourEnv` object, else off the config (`make_connect4_config`), else 4."""
    return int(getattr(env, 'num_to_win', None) or getattr(config, 'num_to_win', None) or 4)


def _go_args(env, config) -> dict:
    """Go's rules as the planner's Go resets take them: off a `games.GoEnv` object, else off the config (`make_go_config`), else the
    defaults (komi2 15, max_plies 0 = 2 * rows * cols, resignation allowed)."""
    def pick(name, default):
        v = getattr(env, name, None)
        v = getattr(config, name, None) if v is None else v
        return default if v is None else v
    return dict(komi2=int(pick('komi2', 15)), max_plies=int(pick('max_plies', 0)), allow_resign=bool(pick('allow_resign', True)))


MAX_ENV_THREADS = 16


def _device_env_name(env) -> Optional[str]:
    """The device environment `env` names (a string, or an object whose `name` / `spec.id` is one), else None."""
    if isinstance(env, str):
        return env
    name = getattr(env, 'name', None) or getattr(getattr(env, 'spec', None), 'id', None)
    return name if name in DEVICE_ENVS else None


def resolve_self_play_envs(env, num_envs: int):
    """How run_self_play plays `env`: ('device', name) for a device environment (a name, or one object whose name is one);
    ('host', [env objects]) for a list / tuple of env objects, a factory `i -> env` (called `num_envs` times), or one env object
    without a device implementation (then B = 1)."""
    if isinstance(env, str):
        if env not in DEVICE_ENVS:
            raise ValueError(f'no device environment for {env!r}; available: {sorted(DEVICE_ENVS)}')
        return 'device', env
    if isinstance(env, (list, tuple)):
        envs = list(env)
    elif _device_env_name(env) is not None:
        return 'device', _device_env_name(env)
    elif hasattr(env, 'reset') and hasattr(env, 'step'):
        envs = [env]
    elif callable(env):
        envs = [env(i) for i in range(int(num_envs))]
    else:
        raise ValueError(f'env must name a device environment ({sorted(DEVICE_ENVS)}), or be an env object, a list of them or a factory '
                         f'i -> env; got {env!r}')
    if not envs:
        raise ValueError('no environments to play')
    for e in envs:
        if not (hasattr(e, 'reset') and hasattr(e, 'step')):
            raise ValueError(f'an environment needs reset() and step(action); got {e!r}')
    return 'host', envs


def device_stack_parts(env):
    """When `env` is a `games.StackFrameAndAction` -- directly or inside `games.PlayerIdAndActionMaskWrapper` (as `games.CartPoleEnv`
    is) -- the device can do its stacking: returns (env to step, stack_history, is_obs_image, frames_u8).  The env to step is the
    stacker's inner env; when that is a `games.ScaledFloatFrame`, it is the env inside it and its uint8 frames are scaled on the
    device.  None otherwise."""
    from muzero_amd.games import PlayerIdAndActionMaskWrapper, ScaledFloatFrame, StackFrameAndAction

    inner = env.env if isinstance(env, PlayerIdAndActionMaskWrapper) else env
    if not isinstance(inner, StackFrameAndAction):
        return None
    base, u8 = inner.env, False
    if isinstance(base, ScaledFloatFrame):
        base, u8 = base.env, True
    return base, int(inner.stack_history), bool(inner.is_obs_image), u8


def board_temperature_switch(config, train_steps: int = 0) -> int:
    """The board schedule's switch from temperature 1.0 to 0.1 (config.py:236-249: 6 TicTacToe, 30 Gomoku), read off
    `config.visit_softmax_temperature_fn`."""
    fn = config.visit_softmax_temperature_fn
    for s in range(100000):
        if fn(s, train_steps) != 1.0:
            if fn(s, train_steps) != 0.1 or fn(s + 1000, train_steps) != 0.1 or s == 0:
                break
            return s
    raise ValueError('host-stepped board games support the temperature schedule "1.0 for the first n moves, then 0.1" (config.py:236-249)')


def run_self_play(config, rank, network, device, env, data_queue, train_steps_counter, stop_event, tag: str = None,
                  moves_per_drain: int = 16, max_moves: Optional[int] = None, device_stack: bool = True, env_threads: int = 1,
                  record_format: str = 'f32') -> int:
    """Self-play until `stop_event` is set (pipeline.py:41-167).  `env` names a device environment ('CartPole-v1',
    'TicTacToe', 'Gomoku', 'ConnectFour' (`games.ConnectFourEnv` on the device, on the board net's own (9, rows, cols) input), 'Othello'
    (`games.OthelloEnv` likewise, rows * cols + 2 actions), 'Go' (`games.GoEnv` likewise; komi2, max_plies and allow_resign off the env
    object, else off the config, else 15 / 2 * rows * cols / True),
    'Synthetic-Atari': random frames standing in for the absent emulator, or 'Catch': `games.CatchEnv` on the
    device, its grid read off `env` when that is a CatchEnv object, else 12 x 12 on the network's frame, or 'Breakout': `games.BreakoutEnv`
    likewise, with its brick rows and move cap); `config.num_envs` of them advance in lock-step on GPU `device`.  `data_queue` is either a queue -- items put on it are the reference's
    `(Transition, priority)` tuples, assembled on the host from the device records -- or a
    `muzero_amd.replay.PrioritizedReplay(device='cuda')`: then the planner's DEVICE EPILOGUE builds the items on the GPU and
    writes them straight into that replay (no host assembly, no queue, no data collector thread); only rewards and done
    flags are read back for the episode statistics.  Returns the number of env steps played.

    Host-stepped environments: `env` may also be a list / tuple of env objects, a factory `i -> env` (called `config.num_envs`
    times), or one env object with no device implementation (B = 1) -- anything with the reference's interface (reset, step,
    actions_mask, current_player, opponent_player; the last three default to an all-legal mask and players 1 / 1).  Each move
    is one batched search on the GPU (`Planner.external_act`), env.step on the host, one `external_commit`; an env that is done
    is reset on the host.  Envs that are `games.StackFrameAndAction` (directly or inside `games.PlayerIdAndActionMaskWrapper`)
    have their stacking done on the device from the newest frame (`device_stack=False`: on the host).  The actor owns the env
    objects while it runs: it may step an inner env of a wrapper, leaving the wrapper's own state stale.  `env_threads` (1 to 16)
    host threads step the envs.  `record_format` 'frames_u8' (host-stepped envs whose uint8 image frames the device stacks, 'Catch' and 'Breakout';
    the other device envs ignore it): the planner's record ring keeps one uint8 frame per move instead of the float32 observation
    (`Planner.selfplay_reset_external`); what reaches `data_queue` is the same."""
    kind, target = resolve_self_play_envs(env, int(getattr(config, 'num_envs', 1)))
    if kind == 'host':
        return _run_self_play_host(config, rank, network, device, target, data_queue, train_steps_counter, stop_event, tag, moves_per_drain,
                                   max_moves, device_stack, env_threads, record_format)
    from muzero_amd import planner as pl

    kinds = {'CartPole-v1': pl.ENV_CARTPOLE, 'TicTacToe': pl.ENV_TICTACTOE, 'Gomoku': pl.ENV_GOMOKU, 'Synthetic-Atari': pl.ENV_SYNTHETIC}
    name = target
    if name in IMAGE_GAMES:
        pl._record_format(record_format)  # (an unknown name: before any GPU work)
    num_envs = int(getattr(config, 'num_envs', 1))
    idx = device.index if getattr(device, 'index', None) is not None else 0
    p = pl.Planner(pl.make_mz_config(network.planner_spec(), config, num_envs=num_envs, seed=int(getattr(config, 'planner_seed', 1)) + 7919 * rank,
                                     keep_shape=name in IMAGE_GAMES), idx, tower_precision=getattr(config, 'tower_precision', 'f32'))
    p.reload(network.state_dict())
    from muzero_amd.replay import PrioritizedReplay

    on_device = isinstance(data_queue, PrioritizedReplay)
    if on_device:  # ONE device writer per replay (attach_device_writer raises on a second one): every actor rank its own shard
        p.attach_replay(data_queue, config, obs_shape=getattr(network, 'input_shape', None))
    if name in IMAGE_GAMES:
        args, selfplay_reset, _, _ = IMAGE_GAMES[name]
        getattr(p, selfplay_reset)(record_format=record_format, **args(env))
    elif name == 'ConnectFour':  # the board is the network's own input; the switch step is the config's schedule
        p.selfplay_reset_connect4(_connect4_num_to_win(env, config), board_temperature_switch(config, train_steps_counter.value) if config.is_board_game else 0)
    elif name == 'Othello':
        p.selfplay_reset_othello(board_temperature_switch(config, train_steps_counter.value) if config.is_board_game else 0)
    elif name == 'Go':
        p.selfplay_reset_go(temp_switch_steps=board_temperature_switch(config, train_steps_counter.value) if config.is_board_game else 0, **_go_args(env, config))
    else:
        p.selfplay_reset(kinds[name])
    asm = EpisodeAssembler(config, num_envs, getattr(network, 'input_shape', None))
    from muzero_amd import metrics as mzm

    tracker = mzm.ActorMetrics(mzm.run_file(config, f'actor{rank}', tag), num_envs)  # trackers.py:74-80 tag names

    version = weights_key(network)
    played = 0
    while not stop_event.is_set() and (max_moves is None or played < max_moves):
        key = weights_key(network)  # read BEFORE copying: a publish that lands during the copy makes the next check fire again
        if key != version:  # learner pushed new weights (pipeline.py:266)
            p.reload(network.state_dict())
            version = key
        n = moves_per_drain if max_moves is None else min(moves_per_drain, max_moves - played)
        # classic/atari schedules depend on train steps only; board games on the env's own step count (config.py:236-267)
        T = -1.0 if config.is_board_game else float(config.visit_softmax_temperature_fn(0, train_steps_counter.value))
        p.selfplay_step(T, n)
        if on_device:
            rec = p.selfplay_read(n, fields=('reward', 'done'))
            tracker.moves(rec['reward'], rec['done'])
        else:
            rec = p.selfplay_read(n)
            tracker.moves(rec['reward'], rec['done'])
            for item in asm.feed(rec):
                data_queue.put(item)
        played += n
    tracker.close()
    p.close()  # (detaches the device epilogue: the replay's write cursor and priorities go back to its host side)
    return played * num_envs


def _run_self_play_host(config, rank, network, device, envs, data_queue, train_steps_counter, stop_event, tag, moves_per_drain, max_moves,
                        device_stack, env_threads, record_format='f32') -> int:
    """run_self_play over host-stepped env objects (see there): the reference's loop body (pipeline.py:83-113) for all envs at once."""
    from muzero_amd import metrics as mzm
    from muzero_amd import planner as pl
    from muzero_amd.replay import PrioritizedReplay

    env_threads = int(env_threads)
    if not 1 <= env_threads <= MAX_ENV_THREADS:
        raise ValueError(f'env_threads must be 1 to {MAX_ENV_THREADS}, got {env_threads}')
    pl._record_format(record_format)  # (an unknown name: before any GPU work)
    B = len(envs)
    parts = [device_stack_parts(e) for e in envs] if device_stack else [None] * B
    stacked = all(pt is not None for pt in parts)
    if stacked and len({pt[1:] for pt in parts}) != 1:
        raise ValueError('all envs must stack the same way (stack_history, is_obs_image, ScaledFloatFrame)')
    step_envs = [pt[0] for pt in parts] if stacked else list(envs)
    S, image, u8 = parts[0][1:] if stacked else (0, False, False)
    frames = [np.asarray(e.reset()) for e in step_envs]
    frame_shape = frames[0].shape
    frame_dtype = np.uint8 if u8 else np.float32

    idx = device.index if getattr(device, 'index', None) is not None else 0
    p = pl.Planner(pl.make_mz_config(network.planner_spec(), config, num_envs=B, seed=int(getattr(config, 'planner_seed', 1)) + 7919 * rank), idx, tower_precision=getattr(config, 'tower_precision', 'f32'))
    p.reload(network.state_dict())
    on_device = isinstance(data_queue, PrioritizedReplay)
    obs_shape = getattr(network, 'input_shape', None)
    if on_device:
        p.attach_replay(data_queue, config, obs_shape=obs_shape)
    spec = getattr(envs[0], 'spec', None)
    max_steps = int(getattr(spec, 'max_episode_steps', None) or getattr(envs[0], 'max_episode_steps', None) or 0)
    board = bool(config.is_board_game)
    p.selfplay_reset_external(stack_history=S, is_obs_image=image, frame_shape=frame_shape, frame_u8=u8, max_episode_steps=max_steps,
                              temp_switch_steps=board_temperature_switch(config, train_steps_counter.value) if board else 0,
                              record_format=record_format)
    asm = EpisodeAssembler(config, B, obs_shape)
    tracker = mzm.ActorMetrics(mzm.run_file(config, f'actor{rank}', tag), B)
    ones = np.ones((B, p.A), np.uint8)
    rewards = np.zeros(B, np.float32)
    dones = np.zeros(B, np.uint8)

    def step_range(lo, hi, actions):
        for i in range(lo, hi):
            obs, r, d, _ = step_envs[i].step(int(actions[i]))
            if d:
                obs = step_envs[i].reset()  # (pipeline.py:83: the next game starts from a fresh reset)
            frames[i], rewards[i], dones[i] = np.asarray(obs), r, 1 if d else 0

    pool = None
    if env_threads > 1:
        from concurrent.futures import ThreadPoolExecutor

        pool = ThreadPoolExecutor(env_threads)
    cuts = [B * t // env_threads for t in range(env_threads + 1)]

    version = weights_key(network)
    played = pending = 0
    try:
        while not stop_event.is_set() and (max_moves is None or played < max_moves):
            key = weights_key(network)
            if key != version:  # learner pushed new weights (pipeline.py:266)
                p.reload(network.state_dict())
                version = key
            T = -1.0 if board else float(config.visit_softmax_temperature_fn(0, train_steps_counter.value))
            mask = np.stack([np.asarray(m, np.uint8).reshape(-1) for m in (getattr(e, 'actions_mask', None) for e in envs)]) \
                if all(getattr(e, 'actions_mask', None) is not None for e in envs) else ones
            cur = np.array([getattr(e, 'current_player', 1) for e in envs], np.int32)
            opp = np.array([getattr(e, 'opponent_player', 1) for e in envs], np.int32)
            actions = p.external_act(np.stack(frames).astype(frame_dtype, copy=False), mask, cur, opp, T)
            if pool is None:
                step_range(0, B, actions)
            else:
                for f in [pool.submit(step_range, cuts[t], cuts[t + 1], actions) for t in range(env_threads)]:
                    f.result()
            p.external_commit(rewards, dones)
            tracker.moves(rewards[None].copy(), dones[None].copy())
            played += 1
            pending += 1
            if not on_device and pending == moves_per_drain:
                for item in asm.feed(p.selfplay_read(pending)):
                    data_queue.put(item)
                pending = 0
        if not on_device and pending:
            for item in asm.feed(p.selfplay_read(pending)):
                data_queue.put(item)
    finally:
        if pool is not None:
            pool.shutdown()
        tracker.close()
        p.close()
    return played * B


# ------------------------------------------------------------------------------------------------------------------
# evaluation matches on the device arena (Planner.arena_*)
# ------------------------------------------------------------------------------------------------------------------
ARENA_ENVS = ('CartPole-v1', 'TicTacToe', 'Gomoku', 'Catch', 'Breakout', 'ConnectFour', 'Othello', 'Go')
_UNFINISHED, _WIN_CHALLENGER, _WIN_OPPONENT, _DRAW = 0, 1, 2, 3  # planner.ARENA_* (kept here so this module imports without the library)


class MatchResult(NamedTuple):
    """Outcome of `play_match`.  Per game, in env-index order: `winner` (1 challenger, 2 opponent, 3 draw -- or a finished one-player
    episode), `length` (plies) and `ret` (the undiscounted return of a one-player episode; +1 / -1 / 0 from the challenger's side of a
    board game).  For two-player envs games [0, n/2) had the challenger as black, games [n/2, n) as white."""
    winner: np.ndarray
    length: np.ndarray
    ret: np.ndarray
    two_player: bool

    @property
    def num_games(self) -> int:
        return int(len(self.winner))

    @property
    def wins(self) -> int:
        return int((self.winner == _WIN_CHALLENGER).sum())

    @property
    def losses(self) -> int:
        return int((self.winner == _WIN_OPPONENT).sum())

    @property
    def draws(self) -> int:
        return int((self.winner == _DRAW).sum())

    @property
    def score(self) -> float:
        """(wins + draws / 2) / games."""
        return (self.wins + 0.5 * self.draws) / max(self.num_games, 1)

    def by_colour(self) -> dict:
        """{'black': (wins, draws, losses), 'white': (...)}: the challenger's games as each colour (two-player envs)."""
        if not self.two_player:
            raise ValueError('by_colour: a one-player match has no colours')
        h = self.num_games // 2
        part = lambda w: (int((w == _WIN_CHALLENGER).sum()), int((w == _DRAW).sum()), int((w == _WIN_OPPONENT).sum()))  # noqa: E731
        return dict(black=part(self.winner[:h]), white=part(self.winner[h:]))

    def elo(self, challenger_elo: float, opponent_elo: float) -> float:
        """The challenger's rating after folding the decided games, in env-index order, through `rating.compute_elo_rating` with the
        opponent's rating held fixed.  Draws are skipped, as pipeline.py:378-383 skips them."""
        from muzero_amd.rating import compute_elo_rating

        if not self.two_player:
            raise ValueError('elo: a one-player match has no opponent')
        r = challenger_elo
        for w in self.winner:
            if w == _WIN_CHALLENGER:
                r, _ = compute_elo_rating(0, r, opponent_elo)
            elif w == _WIN_OPPONENT:
                r, _ = compute_elo_rating(1, r, opponent_elo)
        return r


def resolve_arena_env(env) -> str:
    """The device env an arena plays `env` on: a name, or an object with a device twin (resolved as run_self_play resolves it)."""
    name = _device_env_name(env)
    if name is None and hasattr(env, 'board_size') and hasattr(env, 'num_to_win'):  # games.BoardGameEnv and its subclasses
        if env.board_size == 3 and env.num_to_win == 3:
            name = 'TicTacToe'
        elif env.num_to_win == 5:
            name = 'Gomoku'
    if name is None:
        from muzero_amd.games import CartPoleEnv

        if isinstance(env, CartPoleEnv):
            name = 'CartPole-v1'
    if name not in ARENA_ENVS:
        raise ValueError(f'no arena for {env!r}: the arena plays the device envs {sorted(ARENA_ENVS)} (a name, or an env object with a device twin)')
    return name


def play_match(config, challenger_network, opponent, device, env, num_games: int, opening_plies: Optional[int] = None, tag: str = None,
               init_state=None) -> MatchResult:
    """`num_games` evaluation games in lock-step on the GPU (Planner.arena_*), every searched move a deterministic search
    (pipeline.py:374, 468).  `opponent`: a network (two-player envs), 'random' (two-player envs), or None (one-player envs).  `env`: a
    device-env name ('TicTacToe', 'Gomoku', 'ConnectFour', 'Othello', 'Go', 'CartPole-v1', 'Catch', 'Breakout') or an env object with a device twin.  Two-player envs: `num_games` must be
    even -- the challenger plays black in the first half and white in the second, game i and game i + num_games / 2 share their
    `opening_plies` random opening plies (default: 2 against a network, 0 otherwise; deterministic play from one opening would repeat one
    game).  `init_state`: CartPole start states [num_games, 4].  `tag` names the match in error messages.

    'Catch' (or a `games.CatchEnv` / `games.make_catch_env` object, whose grid is used): game e has its ball in column e % cols, row 0.
    'Breakout' (or a `games.BreakoutEnv` / `games.make_breakout_env` object, whose grid, brick rows and move cap are used): game e starts from
    start code e % (2 * cols); a game's `ret` is the number of bricks it broke.
    Host-stepped envs: `env` may also be a list / tuple of env objects or a factory `i -> env` (called `num_games` times), as
    `run_self_play` takes them: each is reset once and played to its end through the host-stepped arena (`Planner.arena_external_act` /
    `_commit`), live envs stepped on the calling thread; envs that are `games.StackFrameAndAction` have their stacking done on the
    device.  Both are one-player matches: any opponent is a ValueError."""
    what = f'play_match({tag})' if tag else 'play_match'
    if isinstance(env, (list, tuple)) or (callable(env) and not hasattr(env, 'step')):  # what resolve_self_play_envs calls 'host'
        return _play_match_host(config, challenger_network, opponent, device, env, int(num_games), opening_plies, init_state, what)
    name = resolve_arena_env(env)
    two = name != 'CartPole-v1' and name not in IMAGE_GAMES
    num_games = int(num_games)
    if num_games < 1:
        raise ValueError(f'{what}: num_games must be >= 1, got {num_games}')
    if two and num_games % 2:
        raise ValueError(f'{what}: {name} is a two-player env, num_games must be even (colours are balanced), got {num_games}')
    is_net = opponent is not None and not isinstance(opponent, str)
    if isinstance(opponent, str) and opponent != 'random':
        raise ValueError(f"{what}: opponent must be a network, 'random' or None, got {opponent!r}")
    if two and opponent is None:
        raise ValueError(f"{what}: {name} needs an opponent (a network or 'random')")
    if not two and opponent is not None:
        raise ValueError(f'{what}: {name} is a one-player env, opponent must be None')
    if is_net and not (hasattr(opponent, 'planner_spec') and hasattr(opponent, 'state_dict')):
        raise ValueError(f"{what}: opponent must be a network, 'random' or None, got {opponent!r}")
    if opening_plies is None:
        opening_plies = 2 if is_net else 0
    if int(opening_plies) < 0:
        raise ValueError(f'{what}: opening_plies must be >= 0, got {opening_plies}')
    if init_state is not None and name != 'CartPole-v1':
        raise ValueError(f'{what}: init_state is for CartPole-v1 only')
    if is_net and opponent.planner_spec() != challenger_network.planner_spec():
        raise ValueError(f'{what}: challenger and opponent networks differ in shape')
    from muzero_amd import planner as pl

    kinds = {'CartPole-v1': pl.ENV_CARTPOLE, 'TicTacToe': pl.ENV_TICTACTOE, 'Gomoku': pl.ENV_GOMOKU}
    idx = device.index if getattr(device, 'index', None) is not None else 0
    seed = int(getattr(config, 'planner_seed', 1))
    p = pl.Planner(pl.make_mz_config(challenger_network.planner_spec(), config, num_envs=num_games, seed=seed + 104729, keep_shape=name in IMAGE_GAMES), idx,
                   tower_precision=getattr(config, 'tower_precision', 'f32'))
    q = None
    try:
        p.reload(challenger_network.state_dict())
        if is_net:
            q = pl.Planner(pl.make_mz_config(opponent.planner_spec(), config, num_envs=num_games, seed=seed + 130003), idx, tower_precision=getattr(config, 'tower_precision', 'f32'))
            q.reload(opponent.state_dict())
        # the env's own cap: a Catch ball's fall, Breakout's move cap, CartPole's TimeLimit, a board's point count
        if name in IMAGE_GAMES:
            args, _, arena_reset, move_cap = IMAGE_GAMES[name]
            getattr(p, arena_reset)(**args(env))
            cap = move_cap(args(env))
        elif name == 'ConnectFour':
            p.arena_reset_connect4(q if is_net else opponent, int(opening_plies), _connect4_num_to_win(env, config))
            cap = p.obs_dim // 9  # one ply per point
        elif name == 'Othello':
            p.arena_reset_othello(q if is_net else opponent, int(opening_plies))
            cap = 2 * (p.obs_dim // 9 - 4)  # at most nn - 4 placements, each after at most one pass
        elif name == 'Go':
            go = _go_args(env, config)
            p.arena_reset_go(q if is_net else opponent, int(opening_plies), **go)
            cap = go['max_plies'] or 2 * (p.obs_dim // 9)  # the ply that ends the game by the count
        else:
            p.arena_reset(kinds[name], q if is_net else opponent, int(opening_plies), init_state)
            cap = p.A - 1 if two else 500
        res = p.arena_result()
        played = 0
        while res['live'] > 0 and played < cap:
            n = min(8, cap - played)
            p.arena_step(n)
            played += n
            res = p.arena_result()
        if res['live'] > 0:
            raise RuntimeError(f'{what}: {res["live"]} games still running after the env cap of {cap} plies')
        return MatchResult(res['winner'].copy(), res['length'].copy(), res['ret'].copy(), two)
    finally:
        p.close()  # (the challenger first: it borrows the opponent's planner)
        if q is not None:
            q.close()


def _play_match_host(config, network, opponent, device, env, num_games, opening_plies, init_state, what) -> MatchResult:
    """play_match over host-stepped env objects (see there)."""
    if num_games < 1:
        raise ValueError(f'{what}: num_games must be >= 1, got {num_games}')
    if opponent is not None:
        raise ValueError(f'{what}: host-stepped envs are played as one-player matches, opponent must be None')
    if opening_plies or init_state is not None:
        raise ValueError(f'{what}: host-stepped envs take no opening plies and no init_state')
    kind, envs = resolve_self_play_envs(env, num_games)
    if kind != 'host':
        raise ValueError(f'{what}: expected env objects, got {env!r}')
    if len(envs) != num_games:
        raise ValueError(f'{what}: {len(envs)} env objects for num_games = {num_games}')
    from muzero_amd import planner as pl

    B = num_games
    parts = [device_stack_parts(e) for e in envs]
    stacked = all(pt is not None for pt in parts)
    if stacked and len({pt[1:] for pt in parts}) != 1:
        raise ValueError(f'{what}: all envs must stack the same way (stack_history, is_obs_image, ScaledFloatFrame)')
    step_envs = [pt[0] for pt in parts] if stacked else list(envs)
    S, image, u8 = parts[0][1:] if stacked else (0, False, False)
    frames = [np.asarray(e.reset()) for e in step_envs]
    frame_dtype = np.uint8 if u8 else np.float32
    idx = device.index if getattr(device, 'index', None) is not None else 0
    seed = int(getattr(config, 'planner_seed', 1))
    p = pl.Planner(pl.make_mz_config(network.planner_spec(), config, num_envs=B, seed=seed + 104729), idx,
                   tower_precision=getattr(config, 'tower_precision', 'f32'))
    try:
        p.reload(network.state_dict())
        p.arena_reset_external(stack_history=S, is_obs_image=image, frame_shape=frames[0].shape, frame_u8=u8)
        ones = np.ones((B, p.A), np.uint8)
        rewards, dones = np.zeros(B, np.float32), np.zeros(B, np.uint8)
        res = p.arena_result()
        while res['live'] > 0:
            mask = np.stack([np.asarray(m, np.uint8).reshape(-1) for m in (getattr(e, 'actions_mask', None) for e in envs)]) \
                if all(getattr(e, 'actions_mask', None) is not None for e in envs) else ones
            cur = np.array([getattr(e, 'current_player', 1) for e in envs], np.int32)
            opp = np.array([getattr(e, 'opponent_player', 1) for e in envs], np.int32)
            actions, live = p.arena_external_act(np.stack(frames).astype(frame_dtype, copy=False), mask, cur, opp)
            for i in np.flatnonzero(live):
                obs, r, d, _ = step_envs[i].step(int(actions[i]))
                frames[i], rewards[i], dones[i] = np.asarray(obs), r, 1 if d else 0
            p.arena_external_commit(rewards, dones)
            if dones[live != 0].any():
                res = p.arena_result()
        return MatchResult(res['winner'].copy(), res['length'].copy(), res['ret'].copy(), False)
    finally:
        p.close()


def run_board_game_evaluator(config, old_checkpoint_network, new_ckpt_network, device, env, temperature, checkpoint_files, stop_event,
                             initial_elo: int = -2000, tag: str = None, on_result=None, match_games: int = 0, opening_plies: int = 2) -> float:
    """pipeline.py:289-397: for every new checkpoint, one deterministic game new (black) vs previous (white) checkpoint on a
    host `games.BoardGameEnv`, searches through the HIP planner; Elo update as the reference does (white inherits black's
    rating).  `on_result(black_elo, env.steps, train_steps)` stands in for the tensorboard trackers.  Returns the final Elo.

    `match_games` > 0: each checkpoint is judged by a device match of that many games instead (`play_match`: new checkpoint against
    the previous one, colours balanced, `opening_plies` random opening plies per pair); the Elo is the match folded game by game
    (`MatchResult.elo`) against the previous checkpoint's rating, and the step count handed to the trackers is the mean game length."""
    from muzero_amd import mcts
    from muzero_amd.games import BoardGameEnv
    from muzero_amd.rating import compute_elo_rating

    if not isinstance(env, BoardGameEnv):
        raise ValueError(f'Expect env to be a valid BoardGameEnv instance, got {env}')
    for net in (old_checkpoint_network, new_ckpt_network):
        for p in net.parameters():
            p.requires_grad = False
    black_elo = white_elo = initial_elo
    from muzero_amd import metrics as mzm

    tracker = mzm.EvaluatorMetrics(mzm.run_file(config, 'evaluator', tag))  # trackers.py:173-189 tag names
    while True:
        if stop_event.is_set() and len(checkpoint_files) == 0:
            break
        if len(checkpoint_files) == 0:
            time.sleep(0.001)
            continue
        loaded_state = load_checkpoint(checkpoint_files.pop(0), device)
        new_ckpt_network.load_state_dict(loaded_state['network'])
        train_steps = loaded_state['train_steps']
        new_ckpt_network.eval()
        old_checkpoint_network.eval()
        if match_games > 0:
            match = play_match(config, new_ckpt_network, old_checkpoint_network, device, env, match_games, opening_plies=opening_plies, tag=tag)
            black_elo = match.elo(black_elo, white_elo)
            white_elo = black_elo
            steps = int(round(float(match.length.mean())))
            tracker.board_game_step(black_elo, steps, train_steps)
            if on_result is not None:
                on_result(black_elo, steps, train_steps)
            old_checkpoint_network.load_state_dict(new_ckpt_network.state_dict())
            continue
        obs = env.reset()
        done = False
        while not done:
            network = new_ckpt_network if env.current_player == env.black_player_id else old_checkpoint_network
            action, *_ = mcts.uct_search(state=obs, network=network, device=device, config=config, temperature=temperature,
                                         actions_mask=env.actions_mask, current_player=env.current_player, opponent_player=env.opponent_player,
                                         deterministic=True)
            obs, _, done, _ = env.step(action)
        if env.winner == env.black_player_id:
            black_elo, _ = compute_elo_rating(0, black_elo, white_elo)
        elif env.winner == env.white_player_id:
            black_elo, _ = compute_elo_rating(1, black_elo, white_elo)
        white_elo = black_elo
        tracker.board_game_step(black_elo, env.steps, train_steps)
        if on_result is not None:
            on_result(black_elo, env.steps, train_steps)
        old_checkpoint_network.load_state_dict(new_ckpt_network.state_dict())
    tracker.close()
    return black_elo


def run_evaluator(config, new_ckpt_network, device, env, temperature, checkpoint_files, stop_event, tag: str = None, num_episodes: int = 1,
                  on_result=None, device_episodes: int = 0) -> List:
    """pipeline.py:400-488: for every new checkpoint, `num_episodes` deterministic episodes on a host environment exposing
    `reset / step / actions_mask / current_player / opponent_player` (e.g. `games.CartPoleEnv`), searches through the HIP
    planner.  `on_result(eval_returns, eval_steps, train_steps)` stands in for the tensorboard trackers; the list of those
    triples is returned.

    `device_episodes` > 0: each checkpoint plays that many episodes in lock-step on the device twin of `env` instead (`play_match`
    with no opponent; CartPole, or Catch and Breakout on the device arena), or, when `env` is a list or a factory `i -> env` of host env objects,
    through the host-stepped arena; the same tracker calls receive their returns and lengths."""
    from muzero_amd import mcts

    for p in new_ckpt_network.parameters():
        p.requires_grad = False
    from muzero_amd import metrics as mzm

    tracker = mzm.EvaluatorMetrics(mzm.run_file(config, 'evaluator', tag))  # trackers.py:165-170 tag names
    results = []
    while True:
        if stop_event.is_set() and len(checkpoint_files) == 0:
            break
        if len(checkpoint_files) == 0:
            time.sleep(0.001)
            continue
        loaded_state = load_checkpoint(checkpoint_files.pop(0), device)
        new_ckpt_network.load_state_dict(loaded_state['network'])
        train_steps = loaded_state['train_steps']
        new_ckpt_network.eval()
        eval_returns, eval_steps = [], []
        if device_episodes > 0:
            match = play_match(config, new_ckpt_network, None, device, env, device_episodes, tag=tag)
            eval_returns, eval_steps = [float(r) for r in match.ret], [int(n) for n in match.length]
        for _ in range(num_episodes if device_episodes <= 0 else 0):
            obs = env.reset()
            done, steps, returns = False, 0, 0.0
            while not done:
                action, *_ = mcts.uct_search(state=obs, network=new_ckpt_network, device=device, config=config, temperature=temperature,
                                             actions_mask=env.actions_mask, current_player=env.current_player,
                                             opponent_player=env.opponent_player, deterministic=True)
                obs, reward, done, _ = env.step(action)
                steps += 1
                returns += reward
            eval_returns.append(returns)
            eval_steps.append(steps)
        results.append((eval_returns, eval_steps, train_steps))
        tracker.step(eval_returns, eval_steps, train_steps)
        if on_result is not None:
            on_result(eval_returns, eval_steps, train_steps)
    tracker.close()
    return results


def rank_env() -> tuple:
    """(rank, local_rank, world_size) from the torchrun environment."""
    return int(os.environ.get('RANK', '0')), int(os.environ.get('LOCAL_RANK', '0')), int(os.environ.get('WORLD_SIZE', '1'))
