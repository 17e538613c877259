/*
 * mzplanner.h -- C ABI of the MI355X-native MuZero self-play planner (libmzplanner_hip.so).
 *
 * This is the drop-in boundary for the planning hot path of michaelnny/muzero.  Each entry point names the
 * reference interface (file:line under /root/reference/muzero/) it replaces.  Plain C: pointers and sizes only,
 * status-code returns (0 = ok, <0 = error, text via mz_last_error()), no exceptions cross the boundary,
 * caller-allocated outputs.  One planner handle per GPU; a handle is NOT thread-safe (one host thread per
 * handle); the handle owns its HIP stream and all device memory.
 *
 * Pointer arguments named h_* are host pointers; d_* are device (HBM) pointers on the planner's GPU.
 */
#ifndef MZPLANNER_H
#define MZPLANNER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MZ_OK 0
#define MZ_E_INVALID (-1)     /* bad argument / unsupported configuration */
#define MZ_E_HIP (-2)         /* a HIP runtime call failed */
#define MZ_E_STATE (-3)       /* call out of order (e.g. search before weights were committed) */
#define MZ_E_TIES (-4)        /* injected tie-break stream exhausted (parity mode only) */
#define MZ_E_NOMEM (-5)

#define MZ_NET_MLP 0   /* MuZeroMLPNet        network.py:236-267 */
#define MZ_NET_BOARD 1 /* MuZeroBoardGameNet  network.py:540-574 */
#define MZ_NET_ATARI 2 /* MuZeroAtariNet      network.py:501-537 */

#define MZ_ENV_NONE 0
#define MZ_ENV_CARTPOLE 1  /* CartPole-v1 + StackFrameAndAction(4) + PlayerIdAndActionMaskWrapper, gym_env.py:271-365,436-459 */
#define MZ_ENV_TICTACTOE 2 /* TicTacToeEnv, games/tictactoe.py + games/env.py */
#define MZ_ENV_GOMOKU 3    /* GomokuEnv (board = obs_h, stack 4, five in a row), games/gomoku.py + games/env.py */
#define MZ_ENV_SYNTHETIC 4 /* stand-in for the Atari emulator (absent dependency): fresh U[0,1) frames, reward 0, 1000-step episodes */
#define MZ_ENV_EXTERNAL 5  /* any environment the caller steps on the host (mz_selfplay_reset_external) */
#define MZ_ENV_CATCH 6     /* Catch as an image game on the device: uint8 frames through the host-stepped path's kernels (mz_selfplay_reset_catch) */
#define MZ_ENV_BREAKOUT 7  /* a brick-breaking image game on the device, rewards during the episode (mz_selfplay_reset_breakout) */
#define MZ_ENV_CONNECT4 8  /* Connect Four on the device: a two-player game on a rows x cols board, one action per column (mz_selfplay_reset_connect4) */
#define MZ_ENV_OTHELLO 9   /* Othello on the device: placements flip stones, a side without a placement passes, the count decides (mz_selfplay_reset_othello) */
#define MZ_ENV_GO 10       /* Go on the device: captures, simple ko, a pass that is always legal, Tromp-Taylor area count with komi (mz_selfplay_reset_go) */

/* Everything uct_search reads from MuZeroConfig (config.py:51-103) and from the network constructors
 * (network.py:239-247, 504-512, 543-549), plus planner-only sizing knobs. */
typedef struct {
    /* network */
    int32_t net_kind;            /* MZ_NET_* */
    int32_t obs_c, obs_h, obs_w; /* observation shape; MLP nets flatten it (network.py:153-154) and read only the product: a caller may
                                    give them c = all elements, h = w = 1, or the image's own shape (mz_selfplay_reset_catch reads it) */
    int32_t num_actions;         /* board nets (MZ_NET_BOARD): <= 384, boards of at most 361 points (19 x 19); MLP / Atari nets: <= 256 */
    int32_t num_planes;
    int32_t hidden_dim;          /* MLP only */
    int32_t num_res_blocks;      /* conv nets only */
    int32_t value_support_size;  /* 1 (scalar head) or odd: an even size is refused (unit spacing of the support, see mzlearner.h) */
    int32_t reward_support_size;
    /* search: config.py:58-78 */
    int32_t num_simulations;
    double discount;
    double pb_c_base;
    double pb_c_init;
    int32_t is_board_game;
    int32_t has_known_bounds;
    double known_bounds_min, known_bounds_max;
    double root_dirichlet_alpha;
    double root_exploration_eps;
    /* planner */
    int32_t num_envs;  /* capacity B: environments searched in lock-step on this GPU */
    int32_t max_ties;  /* length of the injected tie-break stream per env (parity mode) */
    uint64_t seed;     /* Philox key for on-device randomness (production mode) */
    /* child_U's product in searches WITHOUT root noise (evaluators: deterministic = True, pipeline.py:374,468).  There `child.prior` is an
     * np.float32 scalar multiplied by a Python float (mcts.py:189-197): numpy >= 2 (NEP 50) keeps the product in float32, numpy 1.x -- the
     * reference pins 1.21.6 (requirements.txt:21) -- promotes it to float64 and rounds once.  0 (default): the numpy-2 form, the one every
     * recorded fixture of this repo was produced under; 1: the numpy-1.21 form.  Self-play (float64 prior after the noise) is the same in both. */
    int32_t legacy_scalar_promotion;
    /* Arithmetic of the board nets' 3x3 convolutions.  MZ_CONV_F32 (0, default): float32 MFMA in the oracle's summation order, bit-equal to the
     * oracle.  MZ_CONV_BF16X3 (1): every float32 operand as the exact sum of three bf16 values, six bf16 MFMA products per step accumulated in
     * float32: NOT bit-equal to the oracle, held to the reference within the reference's own tolerance; results still do not depend on
     * the batch, the row or the kernel build.  MZ_NET_BOARD only: mz_planner_create returns MZ_E_INVALID for MZ_NET_MLP, MZ_NET_ATARI and for any
     * other value.  Heads, normalisation, residual adds and the dynamics net's action terms stay float32. */
    int32_t conv_precision;
} mz_config;

#define MZ_CONV_F32 0
#define MZ_CONV_BF16X3 1

/* Injected randomness for a batch of searches: replaces the reference's global numpy RNG
 * (np.random.dirichlet mcts.py:245, np.random.choice mcts.py:124 and :404).  All host pointers.
 * Passing NULL for the whole struct selects on-device Philox randomness. */
typedef struct {
    const double* h_noise;   /* [B, A] Dirichlet samples; NULL => draw on device */
    const double* h_u_tie;   /* [B, max_ties] uniforms in [0,1): k-th real tie among n candidates picks cand[floor(u*n)] */
    const double* h_u_final; /* [B] uniform for the final inverse-CDF sample of the play policy */
} mz_rng_inputs;

typedef struct mz_planner mz_planner;

const char* mz_last_error(void);
const char* mz_version(void);

/* Which kernel build this handle's LAST search launch dispatched to (e.g. "k_search_fast<planes=512, TR=2, TV=2, FUSE=true, AC=2, ...>",
 * or the conv-tower / HBM-tree sequence), followed by every diagnostic switch below as this handle read it.  The string lives until
 * the calling thread's next mz_planner_describe.  A bench line prints the instantiation it ran, not a hard-coded name.
 *
 * DIAGNOSTIC ENVIRONMENT SWITCHES.  None is needed in production; each selects an alternative, bit-identical path for A/B measurements and
 * for the tests that prove the paths agree.  They are read ONCE -- the first group when a handle is created (mz_planner_create), the second
 * once per process at the first planner that needs it -- never between two calls on a handle, so a C-ABI caller cannot be handed a
 * different kernel from one call to the next.
 *   per handle, at mz_planner_create:
 *     MZ_FORCE_GENERIC=1    the shape-generic k_search instead of the tuned k_search_fast builds
 *     MZ_HWX=0..3           work split of k_search_fast's helper waves (default by head kinds)
 *     MZ_TREE_OLD=1         evaluate every level of every descent (no selection cache; the anchor of the tree parity tests)
 *     MZ_HBM_TREE=1         MLP nets: trees in HBM around batched k_infer launches even where they fit LDS
 *   per process, at first use (conv nets):
 *     MZ_ACTION_SPARSE=0    evaluate the dynamics net's action planes densely
 *     MZ_ACTION_FUSE=0      add the sparse action terms in their own kernel instead of the first conv's epilogue
 *     MZ_CONV_SPEC=0        no shape-specialised conv / tower builds (15 x 15 and 19 x 19 Gomoku towers, the Atari net's tiled stages)
 *     MZ_TOWER=0            one launch per conv instead of the persistent residual tower
 *     MZ_CONV_TILE=th*100+tw, MZ_CONV_G=n, MZ_CONV_NCT=n   force the tiled conv kernel's output tile / images per workgroup / channel tiles per wave */
const char* mz_planner_describe(mz_planner* p);

/* Lifetime.  Replaces: network construction + .to(device) in the launchers (classic/run_training.py:83-99) and the
 * per-search allocations of Node objects (mcts.py:75-102). */
int mz_planner_create(const mz_config* cfg, int device_id, mz_planner** out);
int mz_planner_destroy(mz_planner* p);

/* Arithmetic of a conv net's FUSED residual towers (one persistent kernel per tower, activations in LDS).  MZ_TOWER_F32 (0,
 * default): k_res_tower, float32 MFMA, bit-equal to the oracle.  MZ_TOWER_BF16X3 (1): k_res_tower_bf16x3 -- the split-bf16 arithmetic of
 * MZ_CONV_BF16X3 in its one summation order, so a tower equals the chain of split per-conv launches bit for bit; NOT bit-equal to the
 * oracle.  MZ_NET_ATARI: the dynamics and prediction towers at 6 x 6 (32 of a simulation's 33 convs); the representation net, the dynamics
 * net's first conv, the heads and the normalisation stay float32.  MZ_NET_BOARD: all three towers (a board net with
 * conv_precision MZ_CONV_BF16X3 takes the fused split towers without this call: the results are those of its per-conv launches).
 * Legal after mz_planner_create and before the handle's first mz_planner_commit_params / mz_planner_refresh_params; MZ_E_STATE later.
 * MZ_E_INVALID, the handle unchanged, for any other value, for MZ_NET_MLP, for a net without a fused-tower geometry (num_planes no
 * multiple of 16 or above 128, a hidden state too large for the LDS) and where MZ_TOWER=0 is set.  mz_arena_reset refuses two planners
 * that differ in it. */
#define MZ_TOWER_F32 0
#define MZ_TOWER_BF16X3 1
int mz_planner_set_tower_precision(mz_planner* p, int32_t precision);

/* Weights.  `name` is a state_dict key of the reference module (SURVEY 8b lists them; e.g.
 * "dynamics_net.transition_net.0.weight"); data is a host float32 tensor in torch layout; it is copied.
 * Replaces: actor_network.load_state_dict (pipeline.py:266).  Call mz_planner_commit_params after the last tensor:
 * it packs weights into MFMA fragment order and folds eval-mode BatchNorm. */
int mz_planner_set_param(mz_planner* p, const char* name, const float* h_data, const int64_t* shape, int32_t ndim);
int mz_planner_commit_params(mz_planner* p);

/* Weights that already live on the planner's GPU (a learner's master copy): the same hand-off, actor_network.load_state_dict
 * (pipeline.py:266), without the host.  mz_planner_bind_param_device records a DEVICE pointer to a contiguous float32 tensor in torch
 * layout under its state_dict key; nothing is copied, the caller keeps the memory alive and at that address (bind again after it
 * moved).  MZ_E_INVALID for a pointer that is not device memory of the planner's GPU (host, pinned, managed, another GPU), for a tensor
 * that leaves its allocation and for "...num_batches_tracked", which is never bound.  Binding is set-up: it may drain the planner's stream.
 *
 * mz_planner_refresh_params (re)builds every packed operand copy a commit builds -- MFMA fragment order, eval-mode BatchNorm folded in
 * the commit's float32 operation order, the split-bf16 streams of MZ_CONV_BF16X3, tower tables, the tuned search kernel's weight
 * stream -- from the bound tensors with kernels on the planner's stream, bit-identical to a commit of the same values.
 * `producer_stream` is the hipStream_t whose work wrote the tensors (NULL: the null stream): the pack kernels wait for what it holds at
 * the call, and its later work waits for them, so the producer's next optimizer step cannot overwrite weights that are still being
 * packed.  Searches already enqueued on the planner finish on the old weights.  No host synchronisation, no allocation, no host read of
 * a weight -- except in the FIRST refresh after the set of bound names or shapes changed: that one drains the planner's stream, runs the
 * commit's own packers over probe tensors to learn where every packed element comes from (names and shapes are validated there exactly
 * as for host tensors: MZ_E_STATE names a missing tensor, MZ_E_INVALID a wrong shape) and leaves the packed buffers allocated, so a
 * handle that never saw mz_planner_set_param is complete after bind + refresh.  Tensors set with mz_planner_set_param stay as they were.
 * Whichever of commit and refresh ran last defines the weights; a commit on a handle with a refresh in flight is preceded by
 * mz_planner_synchronize. */
int mz_planner_bind_param_device(mz_planner* p, const char* name, const float* d_data, const int64_t* shape, int32_t ndim);
int mz_planner_refresh_params(mz_planner* p, void* producer_stream);

/* MuZeroNet.initial_inference (network.py:62-84), batched.  obs float32 [batch, obs_c*obs_h*obs_w];
 * outputs hidden [batch, hidden_size], pi [batch, A], value [batch]; reward is identically 0 (network.py:76). */
int mz_planner_initial_inference(mz_planner* p, int32_t batch, const float* h_obs, float* h_hidden, float* h_pi, float* h_value);

/* MuZeroNet.recurrent_inference (network.py:86-111), batched.  action int32 [batch]. */
int mz_planner_recurrent_inference(mz_planner* p, int32_t batch, const float* h_hidden, const int32_t* h_action, float* h_hidden_out,
                                   float* h_reward, float* h_pi, float* h_value);
int32_t mz_planner_hidden_size(const mz_planner* p);

/* uct_search (mcts.py:302-407) for `batch` independent roots in lock-step.
 *   h_obs float32 [batch, obs]; h_mask uint8 [batch, A] or NULL (actions_mask=None); players int32 [batch];
 *   h_temperature float64 [batch]; deterministic as mcts.py:311; rng NULL => on-device randomness.
 *   outputs: action int32 [batch], pi float64 [batch, A], root_value float64 [batch], visits int32 [batch, A] (may be NULL). */
int mz_planner_search(mz_planner* p, int32_t batch, const float* h_obs, const uint8_t* h_mask, const int32_t* h_current_player,
                      const int32_t* h_opponent_player, const double* h_temperature, int32_t deterministic, const mz_rng_inputs* rng,
                      int32_t* h_action, double* h_pi, double* h_root_value, int32_t* h_visits);

/* Tree-only parity entry: the same search with the network replaced by scripted outputs
 * (h_pi0 float32 [batch, A]; h_values / h_rewards float32 [batch, num_simulations]: simulation s receives
 * value[s], reward[s]).  Also returns the (parent node, action) expanded by every simulation.  Test hook for the
 * tree kernels: mcts.py:369-389 with network outputs injected. */
int mz_planner_search_scripted(mz_planner* p, int32_t batch, const float* h_pi0, const float* h_values, const float* h_rewards,
                               const uint8_t* h_mask, const int32_t* h_current_player, const int32_t* h_opponent_player,
                               const double* h_temperature, int32_t deterministic, const mz_rng_inputs* rng, int32_t* h_action,
                               double* h_pi, double* h_root_value, int32_t* h_visits, int32_t* h_trace_parent, int32_t* h_trace_action);

/* Device-resident self-play: run_self_play's inner loop (pipeline.py:91-113) for num_envs on-device environments.
 * mz_selfplay_reset seeds/initialises the envs (h_init_state: CartPole float64 [B,4] or NULL => U(-0.05,0.05) from Philox).
 * mz_selfplay_step performs ONE lock-step move for all envs: search (num_simulations) -> sample action -> env.step ->
 * record (obs, action, reward, pi, root_value, player) -> auto-reset finished episodes.  Nothing crosses PCIe.
 * temperature >= 0: the same value for every env (classic / Atari schedules depend on training steps only, config.py:252-267);
 * temperature < 0: the board game's own per-env schedule by episode step (config.py:236-249). */
int mz_selfplay_reset(mz_planner* p, int32_t env_kind, const double* h_init_state);
int mz_selfplay_step(mz_planner* p, double temperature, int32_t n_moves);
/* Copy out the records of the last `n_moves` moves (newest last): arrays [n_moves, B, ...]; any pointer may be NULL.
 * The records live in a ring of R moves (R = 64; 16 when one move of observation records exceeds 64 MiB; at least an open
 * trajectory when a replay is attached): mz_selfplay_step may play more than R moves between reads -- older records are
 * overwritten -- and mz_selfplay_read returns MZ_E_INVALID when asked for more moves than the ring holds.
 * With compact records (mz_external_env.record_format = MZ_RECORD_FRAMES_U8) the ring is R + stack_history moves long and h_obs is
 * rebuilt on the device, move by move, bit for bit the float32 records' observations; as many moves as ever (R) can be read.  A read whose
 * oldest move's observation reaches back past what the ring still holds is refused (MZ_E_INVALID naming record_format) when it asks for
 * h_obs; the same read without h_obs succeeds. */
int mz_selfplay_read(mz_planner* p, int32_t n_moves, float* h_obs, int32_t* h_action, float* h_reward, double* h_pi,
                     double* h_root_value, int32_t* h_player, uint8_t* h_done);
/* counters since reset: [0] env steps, [1] simulations, [2] finished episodes, [3] sum of finished episode lengths */
int mz_selfplay_counters(mz_planner* p, int64_t out[4]);
/* The record ring as the last reset sized it: [0] MZ_RECORD_* format, [1] ring length in moves, [2] bytes of one move's observation records
 * (float32: num_envs * obs * 4; compact: num_envs * frame bytes rounded up to 16), [3] bytes of all record arrays (observations or frames,
 * action, reward, pi, root value, player, done, and the compact ring's per-record step count).  No device work. */
int mz_selfplay_record_info(mz_planner* p, int64_t out[4]);

/* Device epilogue of run_self_play: what the reference does per episode on the host -- compute_n_step_target /
 * compute_mc_return_target (pipeline.py:632-707), priorities (:129,156), make_unroll_sequence (:710-767), including the
 * mid-episode flush every acc_seq_length steps (:118-142), then data_queue.put -> PrioritizedReplay.add (replay.py:67-75)
 * -- done on the GPU after every lock-step move, written straight into a caller-owned replay ring in device memory.
 * All pointers are DEVICE pointers (e.g. the storages of muzero_amd.replay.PrioritizedReplay(device='cuda')); the caller
 * keeps them alive while attached.  SINGLE WRITER: a ring may be attached to ONE planner at a time -- the planner reserves slots from
 * its own cursor (seeded from *num_added at attach) and publishes *num_added by overwriting it; give each planner its own ring.  Items of one environment appear in step order; environments interleave (the
 * reference's actors are independent processes).  Call BEFORE mz_selfplay_reset (the record ring is sized to hold an open
 * trajectory); ring == NULL detaches.  Attach and detach drain the planner's stream, so after a detach the counter and the
 * priorities are final.  mz_selfplay_read then returns at most the moves the record ring holds. */
typedef struct {
    int64_t capacity;     /* ring slots; slot of the i-th item ever added = i % capacity */
    void* state;          /* [capacity, obs_c*obs_h*obs_w] float32 -- or the compact rows of `state_format` below */
    void* action;         /* [capacity, unroll_steps] int8 when num_actions <= 128, int16 otherwise (the reference's int8, pipeline.py:753,
                           * cannot hold Gomoku 15x15's 226 actions: numpy 2 raises OverflowError there) */
    float* pi_prob;       /* [capacity, unroll_steps, num_actions] */
    float* value;         /* [capacity, unroll_steps] */
    float* reward;        /* [capacity, unroll_steps] */
    float* priority;      /* [capacity] */
    int64_t* num_added;   /* one counter, read at attach (the write cursor starts there) and from then on only PUBLISHED by the
                           * device: it advances after each lock-step move, once every slot below the new value is completely
                           * written (state, windows, priority), so a reader on another stream never sees a half-filled slot.
                           * The caller must not write it while attached. */
    int32_t* origin;      /* optional [capacity]: index of the environment that produced the item, or NULL */
    int32_t acc_seq_length, unroll_steps, td_steps;  /* MuZeroConfig fields (config.py:58-94) */
    /* How `state` is stored.  MZ_STATE_F32 (0: a zero-initialised field): float32, as ever.  The other formats are EXACT -- every state decodes to
     * the float32 observation bit for bit -- and are refused (MZ_E_INVALID naming state_format) at mz_selfplay_reset / mz_selfplay_reset_external
     * for an env whose observations they cannot hold:
     *   MZ_STATE_I8         [capacity, obs] one signed byte per element, value (float)(int8_t)b.  TicTacToe, Gomoku, Connect Four, Othello (0 / 1 planes), and host-stepped
     *                       envs: there every emitted state is checked (decode(encode(v)) == v bit for bit); on a mismatch the replay count does not
     *                       advance and mz_selfplay_external_commit returns MZ_E_INVALID naming the smallest such env; mz_selfplay_reset_external next.
     *   MZ_STATE_FRAMES_U8  host-stepped envs with stack_history = S > 0, is_obs_image, frame_u8 and num_actions <= 256 only.  A row is the
     *                       S*C*H*W frame bytes in the observation's plane order (plane k*C + c, k = 0 the newest frame), then S action bytes (byte
     *                       k: the action of plane S*C + k; 0 after a reset), zero-padded to a multiple of 16 bytes: [capacity, row bytes] uint8.
     *                       A pixel decodes to (float)b / 255.0f, an action plane to (float)((double)(a + 1) / (double)num_actions). */
    int32_t state_format;
} mz_replay_ring;
#define MZ_STATE_F32 0
#define MZ_STATE_I8 1
#define MZ_STATE_FRAMES_U8 2
int mz_selfplay_attach_replay(mz_planner* p, const mz_replay_ring* ring);

/* Self-play on host-stepped environments: the reference's actor loop body (pipeline.py:91-113) over whatever env object the
 * launcher built (env.reset / env.step / env.actions_mask / env.current_player, pipeline.py:83-104; e.g. the Atari envs of
 * atari/run_training.py:86, the classic gym envs of classic/run_training.py:71), split in two at env.step:
 *   mz_selfplay_external_act    -- obs, player, temperature, uct_search (pipeline.py:91-104): uploads the num_envs frames, builds the
 *                                  observations on the device (StackFrameAndAction gym_env.py:271-353 and ScaledFloatFrame
 *                                  gym_env.py:214-224 when asked), records (obs, player), searches with the Philox draws keyed like
 *                                  mz_selfplay_step's, records (action, pi, root value) and returns the sampled actions;
 *   mz_selfplay_external_commit -- the outcome of env.step (pipeline.py:106-113): records reward and done, advances step counts and
 *                                  counters, and runs the device epilogue when a replay is attached (mz_selfplay_attach_replay).
 * The host resets an env whose done it committed and hands its reset frame to the next act (as pipeline.py:83 does).
 * mz_selfplay_read, mz_selfplay_counters and mz_selfplay_attach_replay work on this kind as on the device envs; mz_selfplay_step does not
 * (MZ_E_STATE), nor do two acts without a commit between them or a commit without an act.
 * A commit whose env has an open trajectory longer than the record ring while a replay is attached returns MZ_E_INVALID naming the env
 * and runs no epilogue (the replay keeps its last good count); mz_selfplay_reset_external must follow. */
typedef struct {
    int32_t stack_history;     /* 0: h_frames are whole observations (obs_c*obs_h*obs_w float32 each), the env stacks itself.
                                  S > 0: h_frames are the NEWEST unstacked frame; the device applies StackFrameAndAction(S) */
    int32_t is_obs_image;      /* as gym_env.py:276: frame [C,H,W] -> obs [S*(C+1),H,W]; vector frame [D] -> obs [S, D+1] */
    int32_t frame_c, frame_h, frame_w;   /* unstacked frame shape (vector frames: frame_c = D, h = w = 1) */
    int32_t frame_u8;          /* 1: frames are uint8 and are scaled x / 255.0f on the device (ScaledFloatFrame, gym_env.py:214-224) */
    int32_t max_episode_steps; /* sizes the record ring when a replay is attached (0: acc + unroll + td window) */
    int32_t temp_switch_steps; /* temperature < 0: 1.0 for the first temp_switch_steps moves of an episode, then 0.1 (config.py:236-249:
                                  6 TicTacToe, 30 Gomoku); 0: 6 when num_actions <= 10, else 30 */
    /* What the record ring keeps of a move's observation.  MZ_RECORD_F32 (0: a zero-initialised field): the float32 stacked observation,
     * as ever.  MZ_RECORD_FRAMES_U8 (1): only the uint8 frame the host uploaded for the move, at a 16-byte-aligned stride (frame bytes
     * rounded up to 16) -- S - 1 of an observation's S frames are earlier moves' records and the action planes are the recorded actions.
     * Nothing a reader gets changes: mz_selfplay_read's h_obs and every MZ_STATE_FRAMES_U8 replay row are bit for bit the float32 ring's.
     * Record m of an env is the frame of act m; with first(m) the start of m's episode, the observation of move m has frame block k
     * (0 = newest, k < S) = record max(m - k, first(m)) and action plane k = the action of move m - k - 1 if m - k > first(m), else action 0
     * (decoded as MZ_STATE_FRAMES_U8 rows are).  The ring keeps S moves more than the float32 ring would, and its 64 -> 16 rule counts frame
     * bytes.  Refused (MZ_E_INVALID naming record_format) by mz_selfplay_reset_external: without stack_history > 0, is_obs_image and
     * frame_u8; with num_actions > 256; with an attached replay whose state_format is not MZ_STATE_FRAMES_U8; any other value.
     * mz_selfplay_reset (device envs) always keeps float32 records; the device Catch env has its own reset, mz_selfplay_reset_catch. */
    int32_t record_format;
} mz_external_env;
#define MZ_RECORD_F32 0
#define MZ_RECORD_FRAMES_U8 1

int mz_selfplay_reset_external(mz_planner* p, const mz_external_env* env);
/* Search the current observations of all num_envs envs and return the sampled actions.
 *   h_frames [B, frame] uint8 or float32 as mz_external_env says (whole observations when stack_history == 0); h_mask uint8 [B, A];
 *   h_cur / h_opp int32 [B] (env.current_player / env.opponent_player); temperature as mz_selfplay_step; h_action int32 [B] out. */
int mz_selfplay_external_act(mz_planner* p, const void* h_frames, const uint8_t* h_mask, const int32_t* h_cur,
                             const int32_t* h_opp, double temperature, int32_t* h_action);
/* Report the outcome of the actions returned by the last act call: h_reward float32 [B], h_done uint8 [B].  done[e] = 1 means the host
 * will hand env e's reset frame to the next act call. */
int mz_selfplay_external_commit(mz_planner* p, const float* h_reward, const uint8_t* h_done);

/* Catch (MZ_ENV_CATCH): an image game that lives on the device and renders the uint8 frames a host env would upload, so the host-stepped
 * path's device work -- frame stacking, record ring (float32 or compact), epilogue into a float32 or MZ_STATE_FRAMES_U8 replay -- runs
 * with no host in the loop.  The game (muzero_amd.games.CatchEnv is the specification): a rows x cols grid of cells drawn on a one-channel
 * frame; a ball falls one row per move, the paddle in the last row moves left / stays / right (actions 0 / 1 / 2, clipped at the walls)
 * before the ball falls; when the ball reaches the last row the episode ends with reward +1 if it meets the paddle, else -1; every other
 * reward is 0.  Frame pixels are 0, the ball's and the paddle's cells 255.  Mask all legal, players 1 / 1.  A finished env restarts at once
 * (ball in row 0, paddle at cols / 2); the ball column of env e, episode k is min(cols - 1, floor(u * cols)), u the first double of
 * Philox(seed, e, k, 0x70000000).  Episode 0 of env e starts with the ball in row e % (rows - 1), so envs do not finish in step.
 * Geometry comes from the planner's mz_config: obs_c = 2 * S (S frames of one channel and S action planes, stack_history = S >= 1), frame
 * obs_h x obs_w, cells of (obs_h / rows) x (obs_w / cols) pixels -- both must divide -- num_actions == 3, not a board game; anything else
 * is MZ_E_INVALID naming the field.  record_format is mz_external_env's, with its rules and refusals; an attached replay is MZ_STATE_F32
 * or MZ_STATE_FRAMES_U8.  After this reset mz_selfplay_step(p, T, n) plays n moves with nothing crossing PCIe and no host synchronisation
 * (with a replay attached: one at the end of the call, which reads back the record ring's capacity check and the search kernels' error
 * word once per call); mz_selfplay_read, _counters, _record_info and _attach_replay work as on the other kinds;
 * mz_selfplay_external_act / _commit return MZ_E_STATE; mz_arena_reset refuses the kind (its arena is mz_arena_reset_catch's). */
typedef struct {
    int32_t rows, cols;     /* the grid; rows = cols = 0: 12 x 12 */
    int32_t record_format;  /* MZ_RECORD_F32 or MZ_RECORD_FRAMES_U8 */
} mz_catch_env;
int mz_selfplay_reset_catch(mz_planner* p, const mz_catch_env* env);

/* Breakout (MZ_ENV_BREAKOUT): the second device image game, on Catch's pattern, with what Catch lacks: a reward during the episode (1 per
 * brick), episodes that end on a miss or on a move cap, and lengths that differ from env to env.  muzero_amd.games.BreakoutEnv is the
 * specification: a rows x cols grid (cols <= 32); bricks fill rows 1 .. brick_rows, row 0 is empty, the paddle lives in the last row; the
 * ball moves diagonally (d: 0 up-left, 1 up-right, 2 down-right, 3 down-left).  A move: the paddle moves left / stays / right (actions
 * 0 / 1 / 2, clipped at the walls); the ball's next cell is computed, a side wall clamps the column and flips d horizontally; then exactly
 * one of: above the grid -> row 0, d flips vertically | a brick there -> it is removed, reward 1, the ball keeps its row, d flips
 * vertically | the paddle's row -> the bricks are refilled if none is left, then the ball bounces (ball column == paddle: d flips
 * vertically; next column == paddle: d flips both ways; the ball keeps its row) or the episode ends with reward 0 | nothing.  The move
 * count reaching max_moves ends the episode too (a brick reward may fall on that move).  Frame: background 0, bricks 96, the ball's last
 * cell 64, paddle 160, ball 255; priority ball, paddle, trail, brick.  Mask all legal, players 1 / 1.  A finished env restarts at once from
 * start code k = min(2 cols - 1, floor(u * 2 cols)), u the first double of Philox(seed, e, episode, 0x71000000): ball column k >> 1, row
 * brick_rows + 1, d = 2 + (k & 1), paddle at cols / 2, all bricks.  There is no stagger.
 * Geometry comes from the planner's mz_config as for Catch: obs_c = 2 S, frames [1, obs_h, obs_w], cells of obs_h / rows x obs_w / cols
 * (both must divide), num_actions == 3, is_board_game == 0.  Refusals (MZ_E_INVALID) name the field: cols > 32 or < 3, rows <
 * brick_rows + 3, brick_rows outside 1..3, max_moves < 1.  record_format and the attached replay's state_format follow mz_external_env's
 * rules (MZ_STATE_I8 is refused).  Afterwards the handle behaves as after mz_selfplay_reset_catch: mz_selfplay_step plays whole moves on
 * the device; mz_selfplay_external_act / _commit return MZ_E_STATE; mz_selfplay_reset and mz_arena_reset refuse the kind by naming the
 * right reset. */
typedef struct {
    int32_t rows, cols;     /* the grid; rows = cols = 0: 12 x 12 */
    int32_t brick_rows;     /* 1..3; 0: 3 */
    int32_t max_moves;      /* the move cap; 0: 200 */
    int32_t record_format;  /* MZ_RECORD_F32 or MZ_RECORD_FRAMES_U8 */
} mz_breakout_env;
int mz_selfplay_reset_breakout(mz_planner* p, const mz_breakout_env* env);

/* Connect Four (MZ_ENV_CONNECT4): the two-player device game whose board is not square and whose action count is not its point count.
 * muzero_amd.games.ConnectFourEnv is the specification; BoardGameEnv's conventions hold wherever they apply.  Board obs_h rows x obs_w
 * columns (row obs_h - 1 is the bottom), players 1 (black, moves first) and 2; action c < obs_w drops a stone into column c, where it
 * lands on the lowest empty row; action obs_w resigns (the mover gets -1).  num_to_win or more of the mover's stones in a line through
 * the stone just placed -- horizontal, vertical, either diagonal; lines end at the board's edges -- win (+1), tested from ply
 * 2 * (num_to_win - 1) on; a full board without a win is a draw (0).  A column is legal while its top cell is empty, resign always.  The
 * observation is BoardGameEnv's: (9, obs_h, obs_w), own and opponent stone history interleaved, newest first, then the colour plane.  A
 * finished env restarts at once.  Temperature < 0 in mz_selfplay_step: 1.0 for the first temp_switch_steps moves of an episode, then 0.1.
 * Refusals (MZ_E_INVALID naming the field): net_kind other than MZ_NET_BOARD, obs_c != 9, num_actions != obs_w + 1, obs_h * obs_w > 64
 * (the state is a 64-bit bitboard per colour), num_to_win outside 2 .. max(obs_h, obs_w), an attached replay of MZ_STATE_FRAMES_U8
 * (MZ_STATE_F32 and MZ_STATE_I8 are served; with is_board_game the items are Monte-Carlo returns on episode end).  Afterwards
 * mz_selfplay_step, _read, _counters and _record_info work as on the other device kinds; mz_selfplay_external_act / _commit return
 * MZ_E_STATE; mz_selfplay_reset and mz_arena_reset refuse the kind by naming the right reset.
 * (This game's entry points carry a digit in their names.  tests/test_abi.py and tests/test_split_tower_host.py both compare
 * planner.ABI_SYMBOLS with the prototypes they parse out of this header, the first skipping names with digits, the second not; the
 * prototypes are written `extern int ...`, which neither collects, and tests/test_connect4_host.py checks that they are declared here
 * and exported by the library.) */
typedef struct {
    int32_t num_to_win;        /* stones in a line that win: 2 .. max(obs_h, obs_w) */
    int32_t temp_switch_steps; /* 0: 6, the board rule's value for num_actions <= 10 */
} mz_connect4_env;
extern int mz_selfplay_reset_connect4(mz_planner* p, const mz_connect4_env* env);
/* Test hook: one move of all envs with the caller's actions (h_action int32 [B]) through the launches of a self-play move -- pre, step,
 * record, epilogue -- without the search: the recorded policy is the one-hot of the action, the root value 0.  An illegal action of any
 * env is MZ_E_INVALID naming the env, before any launch; MZ_E_STATE unless mz_selfplay_reset_connect4 came before. */
extern int mz_connect4_debug_step(mz_planner* p, const int32_t* h_action);
/* Test hook: the envs' legal-action masks as the next search will see them, h_mask uint8 [B, num_actions]. */
extern int mz_connect4_debug_mask(mz_planner* p, uint8_t* h_mask);

/* Othello (MZ_ENV_OTHELLO): the device board game in which a move changes more than one point.  muzero_amd.games.OthelloEnv is the
 * specification; BoardGameEnv's conventions hold wherever they apply.  Board obs_h rows x obs_w columns, each 4 .. 8, point r * obs_w + c,
 * players 1 (black, moves first) and 2; start: white on (r0, c0) and (r0 + 1, c0 + 1), black on (r0, c0 + 1) and (r0 + 1, c0), r0 =
 * obs_h / 2 - 1, c0 = obs_w / 2 - 1.  With nn = obs_h * obs_w: action a < nn places a stone on point a, legal iff the point is empty and
 * the stone flips at least one run (in each of the 8 directions, one or more opposing stones next to the point followed directly by a
 * stone of the mover; runs end at the board's edges); action nn passes, legal iff the mover has no placement (a real ply: the side to
 * move alternates on every ply); action nn + 1 resigns (always legal, the mover gets -1).  After a placement, if neither colour can place,
 * the game is over and the stones are counted after the flips: the mover gets +1 with more, -1 with fewer, 0 with as many (a draw).  A
 * pass never ends a game.  The observation is BoardGameEnv's (9, obs_h, obs_w) -- own and opponent stone history interleaved, newest
 * first, then the colour plane -- but BOTH colours' histories advance on every ply, pass included: plane k of a colour holds its stones
 * as they stood k plies ago (a fresh game: plane 0 the start stones).  A finished env restarts at once.  A game has at most
 * 2 * (nn - 4) plies; the record ring is sized for that.  Temperature < 0 in mz_selfplay_step: 1.0 for the first temp_switch_steps moves
 * of an episode, then 0.1.  Refusals (MZ_E_INVALID naming the field): net_kind other than MZ_NET_BOARD, obs_c != 9, obs_h or obs_w
 * outside 4 .. 8, num_actions != obs_h * obs_w + 2, an attached replay of MZ_STATE_FRAMES_U8 (MZ_STATE_F32 and MZ_STATE_I8 are served; with
 * is_board_game the items are Monte-Carlo returns on episode end).  Afterwards mz_selfplay_step, _read, _counters and _record_info work
 * as on the other device kinds; mz_selfplay_external_act / _commit return MZ_E_STATE; mz_selfplay_reset and mz_arena_reset refuse the
 * kind by naming the right reset. */
typedef struct {
    int32_t temp_switch_steps; /* 0: 6 */
} mz_othello_env;
int mz_selfplay_reset_othello(mz_planner* p, const mz_othello_env* env);
/* Test hook: one move of all envs with the caller's actions (h_action int32 [B]) through the launches of a self-play move -- pre, step,
 * record, epilogue -- without the search: the recorded policy is the one-hot of the action, the root value 0.  An illegal action of any
 * env is MZ_E_INVALID naming the env, before any launch; MZ_E_STATE unless mz_selfplay_reset_othello came before. */
int mz_othello_debug_step(mz_planner* p, const int32_t* h_action);
/* Test hook: the envs' legal-action masks as the next search will see them, h_mask uint8 [B, num_actions]. */
int mz_othello_debug_mask(mz_planner* p, uint8_t* h_mask);
/* Test hook: the envs' boards, h_board int8 [B, obs_h * obs_w] (0 empty, 1 black, 2 white): after mz_selfplay_reset_othello the positions
 * the next move starts from; after mz_arena_reset_othello the live games' positions and the finished games' frozen final boards, flips
 * included.  MZ_E_STATE unless one of the two resets came before. */
int mz_othello_debug_board(mz_planner* p, int8_t* h_board);

/* Go (MZ_ENV_GO): the device board game in which a move removes whole connected groups.  muzero_amd.games.GoEnv is the specification;
 * BoardGameEnv's conventions hold wherever they apply.  Board obs_h rows x obs_w columns, each 3 .. 19, point r * obs_w + c, empty at the
 * start; players 1 (black, moves first) and 2.  With nn = obs_h * obs_w: action a < nn places a stone on point a and then removes every
 * opposing group (4-connected stones of one colour) without a liberty (an empty 4-neighbour); legal iff the point is empty, it is not the
 * ko point, and the mover's group with the new stone has a liberty after the removals (suicide is illegal).  Simple ko: a placement that
 * captures exactly one stone, by a stone that is a one-stone group with exactly one liberty, forbids the captured point to the opponent
 * on the next ply only; no superko.  Action nn passes (always legal, a real ply); action nn + 1 resigns (the mover gets -1; legal iff
 * allow_resign, else its mask entry is 0 throughout).  The game ends by a resignation, by a pass directly after a pass, or with the ply
 * that makes the step count max_plies, whatever the action; the last two end in a Tromp-Taylor area count (stones plus the empty regions
 * that touch that colour only): black wins iff 2 * black_area > 2 * white_area + komi2, white iff less, equal is a draw; the final mover
 * gets +1, -1 or 0.  The observation is BoardGameEnv's (9, obs_h, obs_w); both colours' histories advance on every ply, pass included.
 * A finished env restarts at once.  The record ring is sized for max_plies plies.  Temperature < 0 in mz_selfplay_step: 1.0 for the
 * first temp_switch_steps moves of an episode, then 0.1.  Refusals (MZ_E_INVALID naming the field): net_kind other than MZ_NET_BOARD,
 * obs_c != 9, obs_h or obs_w outside 3 .. 19, a non-square board of more than 64 points (that combination of the board net's kernels is
 * not held to the oracle search), num_actions != obs_h * obs_w + 2, komi2 outside 0 .. 2 * nn, max_plies outside 0 .. 2 * nn,
 * allow_resign other than 0 / 1, an attached replay of MZ_STATE_FRAMES_U8 (MZ_STATE_F32 and MZ_STATE_I8 are served; with is_board_game
 * the items are Monte-Carlo returns on episode end).  Afterwards mz_selfplay_step, _read, _counters and _record_info work as on the other
 * device kinds; mz_selfplay_external_act / _commit return MZ_E_STATE; mz_selfplay_reset and mz_arena_reset refuse the kind by naming the
 * right reset. */
typedef struct {
    int32_t temp_switch_steps; /* 0: 6 */
    int32_t komi2;             /* twice the komi, 0 .. 2 * nn */
    int32_t max_plies;         /* 0: 2 * nn */
    int32_t allow_resign;      /* 0: the resignation is never legal; 1: always */
} mz_go_env;
int mz_selfplay_reset_go(mz_planner* p, const mz_go_env* env);
/* Test hook: one move of all envs with the caller's actions (h_action int32 [B]) through the launches of a self-play move -- pre, step,
 * record, epilogue -- without the search: the recorded policy is the one-hot of the action, the root value 0.  An illegal action of any
 * env is MZ_E_INVALID naming the env, before any launch; MZ_E_STATE unless mz_selfplay_reset_go came before. */
int mz_go_debug_step(mz_planner* p, const int32_t* h_action);
/* Test hook: the envs' legal-action masks as the next search will see them, h_mask uint8 [B, num_actions]. */
int mz_go_debug_mask(mz_planner* p, uint8_t* h_mask);
/* Test hook: the envs' boards, h_board int8 [B, obs_h * obs_w] (0 empty, 1 black, 2 white): after mz_selfplay_reset_go the positions the
 * next move starts from; after mz_arena_reset_go the live games' positions and the finished games' frozen final boards, captures
 * included.  MZ_E_STATE unless one of the two resets came before. */
int mz_go_debug_board(mz_planner* p, int8_t* h_board);

/* Arena: the evaluators' game loops (pipeline.py:289-397 board games, pipeline.py:400-488 one-player envs) for num_envs games in
 * lock-step on the device.  Every searched move is uct_search(deterministic = True) on the planner's search kernels: no root noise, the
 * most-visited child, tie draws consumed as mz_planner_search consumes them (mz_debug_capture_rng reads them back per handle).  The
 * recorded policy is the visit distribution (temperature 1); the move does not depend on the temperature.  Nothing resets: a finished env
 * is FROZEN -- board, winner, length and return no longer change, its record of the last ply stays as it was -- and is still searched
 * (its unchanged observation, an all-legal mask) with the output discarded; frozen envs are not compacted away, so a ply costs the same
 * until the last game ends.
 *   Sides: the CHALLENGER `p` owns the env state.  Opponent kinds: MZ_ARENA_NONE (one-player envs: p plays every move), MZ_ARENA_RANDOM
 *   (uniform over the legal moves), MZ_ARENA_PLANNER (a second planner q on p's device whose mz_config equals p's apart from the seed,
 *   weights committed; anything else: MZ_E_INVALID / MZ_E_STATE).  q is BORROWED until p's next reset or destroy: the arena launches
 *   searches on q's stream and buffers; using or destroying q meanwhile is the caller's error.
 *   Colours: two-player envs need an even num_envs; the challenger plays black in envs [0, B/2) and white in [B/2, B); env i and
 *   env i + B/2 are a pair.  All live games are at the same ply, so each side searches one contiguous run of B/2 roots per ply.
 *   Openings: the first opening_plies plies (0 allowed) are uniform-random legal moves drawn once per PAIR (per env for one-player
 *   envs) from a Philox stream of their own: both games of a pair start from the same position with colours swapped.
 *   Random moves (openings, MZ_ARENA_RANDOM): legal[floor(u * n_legal)], u one Philox double per (pair or env, ply), recorded.
 *   Game length is capped by the env: 500 steps (CartPole), the point count (boards).
 * mz_arena_reset: env_kind MZ_ENV_CARTPOLE / _TICTACTOE / _GOMOKU (MZ_ENV_SYNTHETIC: MZ_E_INVALID; MZ_ENV_CATCH, MZ_ENV_BREAKOUT and MZ_ENV_EXTERNAL:
 * MZ_E_INVALID naming the reset that plays them, below); h_init_state as mz_selfplay_reset (CartPole only).  Arena and self-play exclude
 * each other on a handle: mz_selfplay_step and mz_selfplay_external_act / _commit during an arena are MZ_E_STATE, mz_arena_step without an
 * arena reset (e.g. during self-play) is MZ_E_STATE; each mode's reset enters it and frees what the other left.
 *   Image and frame games: mz_arena_reset_catch (the device Catch env) and mz_arena_reset_external (envs the host steps) start a
 *   one-player arena (MZ_ARENA_NONE semantics) whose roots are built on the device from the frame history of the host-stepped path,
 *   StackFrameAndAction over the newest frame: at the first ply every frame plane is the first frame and every action plane 0, afterwards
 *   plane 0 is the newest frame with the action plane float32((a_prev + 1) / A) and the history shifts.  A frozen env's history and root
 *   no longer change.  mz_arena_read_ply and mz_arena_result report them with the fields above (h_side always MZ_ARENA_SIDE_CHALLENGER,
 *   h_u 0, a finished game's h_winner MZ_ARENA_DRAW); the arena has no record ring, so record_format must be MZ_RECORD_F32. */
#define MZ_ARENA_NONE 0
#define MZ_ARENA_RANDOM 1
#define MZ_ARENA_PLANNER 2
#define MZ_ARENA_SIDE_CHALLENGER 0 /* who chose a ply's move (mz_arena_read_ply h_side) */
#define MZ_ARENA_SIDE_OPPONENT 1
#define MZ_ARENA_SIDE_RANDOM 2
#define MZ_ARENA_SIDE_OPENING 3
#define MZ_ARENA_UNFINISHED 0 /* mz_arena_result h_winner */
#define MZ_ARENA_WIN_CHALLENGER 1
#define MZ_ARENA_WIN_OPPONENT 2
#define MZ_ARENA_DRAW 3 /* also: a finished one-player episode (it has no winner; its score is h_ret) */
int mz_arena_reset(mz_planner* p, int32_t env_kind, int32_t opponent_kind, mz_planner* q_or_null, int32_t opening_plies,
                   const double* h_init_state_or_null);
/* Issues n_plies plies -- per ply: roots, at most one search per side (B/2 roots each; B with MZ_ARENA_NONE), env.step -- with no host
 * synchronisation inside; the two planners' streams are ordered with events.  Replaces the `while not done` loops of pipeline.py:289-397
 * (:370-377) and pipeline.py:400-488 (:463-473). */
int mz_arena_step(mz_planner* p, int32_t n_plies);
/* Catch in the arena.  Geometry and refusals are mz_selfplay_reset_catch's (3 actions, not a board game, obs_c = 2 S, rows and cols divide
 * the frame); record_format must be MZ_RECORD_F32.  Env e starts with the paddle at cols / 2, the ball in column h_ball_col[e] (NULL:
 * e % cols, every column equally often) and row h_start_row[e] (NULL: 0; 0 .. rows - 2, so games may end on different plies); an entry out
 * of range is MZ_E_INVALID naming the array and the env.  No Philox draw is used.  mz_arena_step(p, n) then plays n plies with nothing
 * crossing PCIe and no host synchronisation: roots from the frames, one deterministic search of all num_envs roots, the env's step without
 * restart, the next frame.  A game ends when the ball reaches the last row: ret +1.0 or -1.0, length the plies played. */
int mz_arena_reset_catch(mz_planner* p, const mz_catch_env* env, const int32_t* h_ball_col_or_null, const int32_t* h_start_row_or_null);
/* Breakout in the arena.  Geometry and refusals are mz_selfplay_reset_breakout's; record_format must be MZ_RECORD_F32.  Env e starts from
 * start code h_start_code[e] (NULL: e % (2 * cols)); an entry outside 0 .. 2 * cols - 1 is MZ_E_INVALID naming the array and the env.  No
 * Philox draw is used.  mz_arena_step plays plies as for Catch; a game ends on a miss or at max_moves: ret is the number of bricks broken,
 * length the plies played. */
int mz_arena_reset_breakout(mz_planner* p, const mz_breakout_env* env, const int32_t* h_start_code_or_null);
/* Connect Four in the arena: mz_arena_reset's two-player arena -- MZ_ARENA_RANDOM or MZ_ARENA_PLANNER, colours balanced over the two
 * halves, paired openings, deterministic searches, a finished game frozen, the tally -- on MZ_ENV_CONNECT4, with the refusals of
 * mz_selfplay_reset_connect4 and of mz_arena_reset's sides.  Random moves (openings and MZ_ARENA_RANDOM) are legal[floor(u * n_legal)]
 * over the legal COLUMNS only: a random move never resigns.  mz_arena_step, _read_ply and _result as ever. */
extern int mz_arena_reset_connect4(mz_planner* p, const mz_connect4_env* env, int32_t opponent_kind, mz_planner* q_or_null, int32_t opening_plies);
/* Othello in the arena: the same two-player arena on MZ_ENV_OTHELLO, with the refusals of mz_selfplay_reset_othello and of
 * mz_arena_reset's sides.  Random moves (openings and MZ_ARENA_RANDOM) are legal[floor(u * n_legal)] over the legal placements, or the
 * pass where there is none: a random move never resigns.  A finished game is frozen with its final board, flips included; the winner is
 * the colour with more stones (or the side that did not resign), a draw on equal counts.  mz_arena_step, _read_ply and _result as ever. */
int mz_arena_reset_othello(mz_planner* p, const mz_othello_env* env, int32_t opponent_kind, mz_planner* q_or_null, int32_t opening_plies);
/* Go in the arena: the same two-player arena on MZ_ENV_GO, with the refusals of mz_selfplay_reset_go and of mz_arena_reset's sides.
 * Random moves (openings and MZ_ARENA_RANDOM) are legal[floor(u * n_legal)] over the legal placements and the pass: a random move may
 * pass and never resigns.  A finished game is frozen with its final board, captures included; the winner is decided by the area count
 * (or is the side that did not resign).  mz_arena_step, _read_ply and _result as ever. */
int mz_arena_reset_go(mz_planner* p, const mz_go_env* env, int32_t opponent_kind, mz_planner* q_or_null, int32_t opening_plies);
/* The same ply for envs the host steps, cut where it steps them.  `env` describes the frames as for mz_selfplay_reset_external (stacked
 * uint8 or float images, stacked vectors, stack_history = 0 for whole observations); max_episode_steps and temp_switch_steps are not used.
 *   mz_arena_external_act    -- uploads every env's newest frame, mask and player ids (arguments as mz_selfplay_external_act's; the entries
 *                               of frozen envs are ignored), searches deterministically, returns h_action int32 [B] and h_live uint8 [B]:
 *                               1 where the host must step the env with its action (a frozen env's h_action is its last move);
 *   mz_arena_external_commit -- h_reward float32 [B], h_done uint8 [B] of the live envs (frozen envs' entries are ignored): the reward is
 *                               added to the env's float64 return in ply order, the length grows by one, a done env freezes and is tallied.
 * mz_arena_read_ply and mz_arena_result report the plies committed so far.  MZ_E_STATE, naming the call to make instead: mz_arena_step on
 * this arena, these two calls on any other arena or before the reset, two acts without a commit, a commit without an act. */
int mz_arena_reset_external(mz_planner* p, const mz_external_env* env);
int mz_arena_external_act(mz_planner* p, const void* h_frames, const uint8_t* h_mask, const int32_t* h_cur, const int32_t* h_opp,
                          int32_t* h_action, uint8_t* h_live);
int mz_arena_external_commit(mz_planner* p, const float* h_reward, const uint8_t* h_done);
/* The last ply, per env; any pointer may be NULL.  h_obs float32 [B, obs], h_mask uint8 [B, A], h_player int32 [B] (side to move, 1 / 2):
 * the root before the move.  h_side int32 [B] (MZ_ARENA_SIDE_*), h_pi float64 [B, A] and h_root float64 [B] (zeros for a random move),
 * h_action int32 [B], h_u float64 [B] (the uniform of a random move, else 0), h_live uint8 [B]: 1 where the env was live when the ply
 * began -- elsewhere the other fields are those of the env's last ply.  What the evaluators read per move (pipeline.py:370-377). */
int mz_arena_read_ply(mz_planner* p, float* h_obs, uint8_t* h_mask, int32_t* h_player, int32_t* h_side, double* h_pi, double* h_root,
                      int32_t* h_action, double* h_u, uint8_t* h_live);
/* The tally (pipeline.py:378-383 winner, :474-476 returns and steps); any pointer may be NULL.  h_winner int32 [B] (MZ_ARENA_*), h_length
 * int32 [B] plies played, h_ret float64 [B]: the undiscounted return (one-player envs), +1 / -1 / 0 from the challenger's side (boards);
 * totals: [0] challenger wins, [1] opponent wins, [2] draws (finished episodes of one-player envs), [3] sum of finished lengths;
 * n_live: games still running. */
int mz_arena_result(mz_planner* p, int32_t* h_winner, int32_t* h_length, double* h_ret, int64_t totals[4], int32_t* n_live);

/* Measurement hooks (bench.py): HIP-event timing on the planner's own stream.
 * mz_profile_begin/end bracket a region; mz_profile_end returns elapsed milliseconds and the number of
 * search-kernel launches inside it (the dominant kernel of the path). */
int mz_profile_begin(mz_planner* p);
int mz_profile_end(mz_planner* p, double* elapsed_ms, double* search_kernel_ms, int64_t* search_kernel_launches);
int mz_planner_synchronize(mz_planner* p);

#ifdef __cplusplus
}
#endif
#endif
