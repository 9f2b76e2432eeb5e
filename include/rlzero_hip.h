/*
 * rlzero_hip.h -- C ABI of the MI355X (gfx950) AlphaZero self-play MCTS engine.
 *
 * This is the drop-in boundary for ONE path of jianzhnie/RLZero: the
 * select -> expand -> evaluate -> backup loop of AlphaZero MCTS plus the Gomoku /
 * TicTacToe board rules it steps through.  The reference is pure Python and has no FFI;
 * each entry point below names the reference function(s) (file:line, relative to the
 * reference repository) whose work it takes over for a whole batch of lock-stepped games.
 * INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *  - plain C, no torch types.  `d_` pointers are DEVICE pointers (e.g. tensor.data_ptr()),
 *    `h_` pointers are HOST pointers.  `stream` is a hipStream_t passed as void*.
 *  - every function returns 0 (RZ_OK) or a negative RZ_ERR_* code; the message is
 *    available from rz_last_error() (thread local).  No exception crosses the ABI.
 *  - an engine is NOT thread safe: one host thread per engine (the reference is
 *    single-threaded).  Launch functions enqueue on `stream` and do
 *    not synchronise, allocate or free: they can be captured in a hipGraph.
 *  - one tree per game, ONE simulation in flight per tree (the reference runs
 *    simulations strictly sequentially, rlzero/mcts/alphazero_mcts.py:82-85); the
 *    parallelism is across games.
 *
 * Boards: two bitboards per game, RZ_BOARD_WORDS u64 words per colour, bit `a` = move
 * `a` = h*B + w (rlzero/games/gomoku/gomoku_env.py:227-234).  Layout of a board array:
 * [n_games][2][RZ_BOARD_WORDS] (colour 0 = player id 0 = first player).
 */
#ifndef RLZERO_HIP_H
#define RLZERO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RZ_ABI_VERSION 47
#define RZ_MAX_BOARD_SIZE 16
#define RZ_BOARD_WORDS 4 /* 4 x 64 bits >= 16*16 cells */
#define RZ_MAX_IN_FLIGHT 16 /* rz_config.sims_in_flight */

enum {
    RZ_OK = 0,
    RZ_ERR_ARG = -1,      /* bad argument / config */
    RZ_ERR_HIP = -2,      /* a HIP runtime call failed */
    RZ_ERR_OOM = -3,      /* device allocation failed */
    RZ_ERR_OVERFLOW = -4, /* a game ran out of arena slots / block-queue entries */
    RZ_ERR_ILLEGAL = -5,  /* an illegal move was submitted (gomoku_env.py:51-53 asserts) */
    RZ_ERR_INTERNAL = -6
};

enum {
    RZ_GAME_GOMOKU = 0,  /* TicTacToe = Gomoku(board_size 3, n_in_row 3), tools/play.py:35; action = cell */
    RZ_GAME_CONNECT4 = 1 /* no implementation in the reference (docs/open-spiel_alphazero.md:58 only names
                            it): build-defined.  board_height x board_width (default 6 x 7), n_in_row
                            (default 4), action = column, stones drop to the lowest empty cell, cell =
                            row*width + column with row 0 at the bottom; same planes / search / API */
};

enum {
    RZ_SCORE_UCT_REF = 0, /* the reference's rule: W/N + c*sqrt(ln(Np)/N), +inf if unvisited
                             (rlzero/mcts/node.py:41-42,75-88); bit-exact, fp64 */
    RZ_SCORE_PUCT = 1     /* opt-in: Q + c*(P*sqrt(Np)/(N+1)) (node.py:105-117 is dead code in the
                             reference and divides by zero at N=0; here Q=0 at N=0); fp64, every
                             child initialised at expansion */
};

enum { RZ_EVAL_V0 = 0, RZ_EVAL_VLIN = 1 }; /* synthetic evaluators, SURVEY.md Appendix B */

/* per-game error bits reported by rz_get_stats */
enum {
    RZ_FLAG_ARENA_FULL = 1,
    RZ_FLAG_BLOCKS_FULL = 2,
    RZ_FLAG_ILLEGAL_MOVE = 4,
    RZ_FLAG_LOGTAB = 8,
    RZ_FLAG_INTERNAL = 16,
    RZ_FLAG_REUSE_DROPPED = 32,/* NOT an error: rz_advance_roots found the kept subtree larger than the carry limit (see
                                  rz_config.pool_factor: more than int(pool_factor * n_playout) + 7 expanded nodes for a
                                  pool_factor * n_playout without a fraction, or too many prior floats / record slots) and
                                  restarted that game's search from a fresh root (the reference's tree is unbounded,
                                  alphazero_mcts.py:96-103); counted in rz_stats.reuse_dropped, part of rz_stats.error_flags */
    RZ_FLAG_QUEUE_FULL = 64    /* rz_play_queue_push (ABI 45) would have overwritten a game id that no slot had claimed: nothing was
                                  written (an error of the engine, booked on game 0) */
};

typedef struct rz_engine rz_engine;

typedef struct rz_config {
    int32_t abi_version; /* RZ_ABI_VERSION */
    int32_t game_kind;   /* RZ_GAME_GOMOKU */
    int32_t board_size;  /* B <= RZ_MAX_BOARD_SIZE (GomokuEnv(board_size=), gomoku_env.py:19-31) */
    int32_t n_in_row;    /* GomokuEnv(n_in_row=) */
    int32_t n_games;     /* games searched in lock-step on this GPU */
    int32_t n_playout;   /* simulations per move: sizes the arenas and the ln table
                            (AlphaZeroPlayer(n_playout=), alphazero_mcts.py:112-130) */
    int32_t score_mode;  /* RZ_SCORE_* */
    int32_t add_noise;   /* != 0: priors are mixed 0.75/0.25 with Dirichlet(0.3) noise at every expanded
                            node (node.py:63-69; is_selfplay in alphazero_mcts.py:124-129).  Drawn on the
                            device from a counter-based stream (noise_seed, game, expansion #; rz_set_noise_keys): same
                            distribution as numpy's, not its global stream.  RZ_SCORE_UCT_REF never reads
                            the prior, so the noise cannot change its search. */
    double c_puct;       /* AlphaZeroPlayer(c_puct=) */
    double pool_factor;  /* sizes a game's two arenas (0 -> 2.0), A = actions of a position:
                              qcap = int((pool_factor + 1) * n_playout) + 8    expanded nodes (= prior blocks),
                              prior floats = qcap * A,
                              record slots = qcap * A + 2 (RZ_SCORE_PUCT: a record per child) or
                                             qcap * 16 + 2 * A + 64 (RZ_SCORE_UCT_REF: records of visited children only, in
                                             blocks of 4, 8, ... doubling up to the node's children).
                            An expansion that does not fit is refused and flagged (RZ_FLAG_BLOCKS_FULL: nodes or prior
                            floats, RZ_FLAG_ARENA_FULL: record slots), never written.  rz_advance_roots carries a kept
                            subtree only when it leaves room for the n_playout expansions of the coming search -- summed
                            over its expanded nodes (k children, a child block of c records each):
                              sum k <= prior floats - (n_playout + 1) * A,
                              1 + sum c <= record slots - (n_playout + 1) * 8 - 2 * A,
                              nodes <= qcap - n_playout - 1;
                            else the subtree is dropped (RZ_FLAG_REUSE_DROPPED). */
    int32_t device;      /* HIP device ordinal */
    int32_t noise_seed;  /* seed of the Dirichlet stream */
    int32_t board_height; /* RZ_GAME_CONNECT4 only (0 -> 6) */
    int32_t board_width;  /* RZ_GAME_CONNECT4 only (0 -> 7) */
    int32_t sims_in_flight; /* 0 / 1 (default): ONE simulation in flight per tree, the reference's sequential search
                               (alphazero_mcts.py:82-85) -- the only mode the parity tests use.  K > 1 (opt-in, NOT
                               the reference's algorithm): K simulations of a tree share one evaluator batch; every node
                               of a selected path carries a virtual loss (N += 1, W -= 1) until its backup.  Leaf
                               arrays of this ABI (d_obs, d_logp, d_value, d_raw, d_hid) then have n_games * K rows,
                               row = game * K + slot.  Device evaluators only. */
    int32_t in_flight_impl; /* sims_in_flight > 1: 0 = the level-synchronous kernel (a workgroup of K waves per game: child
                               records of all slots' nodes staged per level, slots walked in slot order), 1 = its sequential
                               restatement (one wave, one slot after the other); same trees, bit for bit */
} rz_config;

typedef struct rz_stats {
    int32_t error_flags;     /* OR of RZ_FLAG_* over all games since the last clear */
    int32_t first_bad_game;  /* lowest game index with a flag, or -1 */
    int64_t arena_slots;     /* node-record capacity per game per arena */
    int64_t prior_floats;    /* prior-block capacity (floats) per game per arena */
    int64_t max_slots_used;  /* max over games of the current arena top */
    int64_t max_blocks_used; /* max over games of expanded nodes in the current arena */
    int64_t device_bytes;    /* bytes of HBM the engine allocated */
    int64_t n_select_calls;  /* rz_select_step launches so far */
    int64_t reuse_dropped;   /* kept subtrees dropped by rz_advance_roots since the last clear (RZ_FLAG_REUSE_DROPPED) */
} rz_stats;

int rz_abi_version(void);
/* The hash of the sources, headers and flags this library was built from (rlzero_amd/_build.py): the binding refuses a library
 * whose hash differs from the source tree beside it, and build() recompiles on a hash mismatch, not on file times. */
const char *rz_source_hash(void);
const char *rz_last_error(void);

/* Lifetime.  rz_create allocates every buffer up front (nothing is allocated later). */
int rz_create(const rz_config *cfg, rz_engine **out);
int rz_destroy(rz_engine *e);
/* Board rows, columns and size A of the action space (Gomoku: A = cells; Connect4: A = columns).
 * Every per-action array of this ABI (d_logp, d_probs, d_visits, d_w, d_p) is [n_games][A]. */
int rz_geometry(rz_engine *e, int32_t *height, int32_t *width, int32_t *n_actions);

/* ln(n) table for n = 0 .. count-1 (entry 0 unused).  The engine fills it at creation
 * with the host libm's log(), the function CPython's math.log() calls in
 * rlzero/mcts/node.py:84-85; the device never evaluates a logarithm itself.  This entry
 * replaces the table (e.g. with one produced by math.log on another host). */
int rz_upload_log_table(rz_engine *e, const double *h_table, int64_t count);
int rz_log_table_size(rz_engine *e, int64_t *count);

/* Root positions.  Import boards for the games selected by d_mask (NULL = all games):
 * what AlphaZeroPlayer.get_action reads from `game_env` (alphazero_mcts.py:136-146:
 * states, current player, last_move).  reset_trees != 0 also discards those games'
 * trees (AlphaZeroMCTS.update_with_move(-1), alphazero_mcts.py:96-103). */
int rz_set_roots(rz_engine *e, const uint64_t *d_stones, const int32_t *d_to_move,
                 const int32_t *d_last_move, const uint8_t *d_mask, int reset_trees,
                 void *stream);
int rz_get_roots(rz_engine *e, uint64_t *d_stones, int32_t *d_to_move, int32_t *d_last_move,
                 void *stream);
/* Games with active == 0 are skipped by select / expand_backup (finished games). */
int rz_set_active(rz_engine *e, const uint8_t *d_active, void *stream);
/* The Dirichlet noise of game g (rz_config.add_noise; node.py:63-69) is drawn from a counter-based stream keyed (key[g], expansion #).
 * By default key[g] = noise_seed ^ g << 20: a stream per SLOT of this engine.  A host that deals games to slots, lanes and GPUs
 * (rlzero_amd.selfplay) gives every game a key of its own when it starts -- d_keys uint64 [n_games], d_mask uint8 [n_games] or NULL
 * (all) selects the slots; their expansion counters restart at 0 -- so that a game's noise, like its move draws, depends on (seed,
 * game id) and not on where the game is played.  d_keys == NULL restores the default keys.  (The reference draws from numpy's
 * global stream, node.py:65: one stream for everything, in the order the single process happens to expand nodes.) */
int rz_set_noise_keys(rz_engine *e, const uint64_t *d_keys, const uint8_t *d_mask, void *stream);

/* SELECT + STEP: for every active game walk from the root to a leaf
 * (AlphaZeroMCTS._playout select loop, alphazero_mcts.py:48-54; TreeNode.select /
 * uct_value, node.py:32-42,75-88), applying each chosen move to a private copy of the
 * board (the reference's copy.deepcopy + GomokuEnv.step, alphazero_mcts.py:83,
 * gomoku_env.py:49-70), then classify the leaf (GomokuEnv.game_end_winner,
 * gomoku_env.py:196-203 -> has_a_winner :116-170).  If d_obs != NULL also writes the
 * leaf's observation planes float32 [n_games][4][B][B] (GomokuEnv.current_state,
 * gomoku_env.py:95-114) -- the input of the evaluator. */
int rz_select_step(rz_engine *e, float *d_obs, void *stream);
/* sims_in_flight > 1 only: how many of the K slots the NEXT launches back up (rz_expand_backup*, rz_tree_step*) and
 * select (rz_select_step, rz_tree_step*); default K, K.  A search of n simulations is ceil(n / K) steps, the last one
 * with the remainder, so that N(root) grows by exactly n. */
int rz_set_in_flight(rz_engine *e, int32_t k_backup, int32_t k_select);

/* Device pointers to the engine's leaf arrays, valid for its lifetime: stones uint64 [n_games * K][2][4], side to move and
 * last cell int32 [n_games * K] of the leaves of the last rz_select_step / rz_tree_step (row = game * K + slot).  An
 * evaluator that reads positions (rz_net_trunk_leaves) needs no observation planes: pass d_obs = NULL to the select calls. */
int rz_leaf_buffers(rz_engine *e, const uint64_t **d_stones, const int32_t **d_to_move, const int32_t **d_last_cell);

/* Observation planes of the current leaves / of the root positions (current_state). */
int rz_encode_leaf_obs(rz_engine *e, float *d_obs, void *stream);
int rz_encode_root_obs(rz_engine *e, float *d_obs, void *stream);

/* Leaf positions for an evaluator that runs on the host (any policy_value_fn callable,
 * alphazero_mcts.py:28-31,59).  d_terminal: 0 = not ended, 1 = tie, 2 = won. */
int rz_get_leaves(rz_engine *e, uint64_t *d_stones, int32_t *d_to_move, int32_t *d_last_move,
                  int32_t *d_terminal, void *stream);

/* Synthetic evaluators of SURVEY.md Appendix B computed from the leaf bitboards:
 * d_value float32 [n_games]; d_logp (nullable) float32 [n_games][B*B] = log(1/k) on
 * empty cells, -inf elsewhere. */
int rz_eval_synthetic(rz_engine *e, int kind, float *d_logp, float *d_value, void *stream);

/* Random-rollout evaluator of the pure-MCTS opponent: RolloutMCTS._evaluate
 * (rlzero/mcts/rollout_mcts.py:49-74, rollout_policy :96-100) from every leaf, on bitboards.
 * Move of ply p = the floor(u*k)-th legal move, u from splitmix64(seed, game, sim_index, p)
 * (the reference draws k uniforms from numpy's global stream and takes the arg-max: also a
 * uniform choice).  d_value float32 [n_games] follows the reference's perspective rule (:68-72).
 * Pair with rz_expand_backup(e, NULL, d_value): uniform priors (rollout_mcts.py:102-108). */
int rz_eval_rollout(rz_engine *e, uint64_t seed, uint32_t sim_index, int32_t n_limit, float *d_value,
                    void *stream);

/* EXPAND + BACKUP: terminal rule and value (alphazero_mcts.py:60-68), TreeNode.expand
 * (node.py:44-73; priors = exp(d_logp) on the leaf's legal moves as in
 * AlphaZeroAgent.policy_value_fn, alphazero_agent.py:41-45; d_logp == NULL -> uniform),
 * TreeNode.update_recursive(-leaf_value) (node.py:119-144).  d_value: leaf value from
 * the evaluator, [n_games], float32 (the reference converts the fp32 net output to a
 * Python float exactly, alphazero_agent.py:45) or float64 for host evaluators. */
int rz_expand_backup(rz_engine *e, const float *d_logp, const float *d_value, void *stream);
int rz_expand_backup_f64(rz_engine *e, const float *d_logp, const double *d_value, void *stream);
/* same, but d_probs float32 [n_games][B*B] holds the evaluator's probabilities themselves (a host
 * policy_value_fn returns (action, prob) pairs, alphazero_mcts.py:28-31): stored unchanged. */
int rz_expand_backup_probs(rz_engine *e, const float *d_probs, const double *d_value, void *stream);

/* rz_expand_backup of the pending leaves followed by rz_select_step of the next simulation in
 * ONE launch (two consecutive iterations of the reference's loop, alphazero_mcts.py:82-85,
 * share a kernel boundary).  Same arguments as the two calls it replaces. */
int rz_tree_step(rz_engine *e, const float *d_logp, const float *d_value, float *d_obs, void *stream);

/* The evaluator's UN-NORMALISED head outputs, as rz_net_heads_gemm leaves them: policy logits raw [rows][ld] (ld >= A)
 * and the value head's hidden layer hid [rows][64] with its last weights w2 [64], b2 [1].  n_parts == 1: raw / hid are
 * final (bias added, hid ReLU'd).  n_parts == 4 (RZ_NET_HEADS_SPLIT_PARTS): raw / hid hold the four K-quarter partial
 * sums of the FC GEMM, part q at raw + q * raw_part_stride / hid + q * hid_part_stride (floats), and the consumer
 * finishes logit = ((p0 + p1) + p2) + p3 -> fmaf(sum, *act_scale, act_bias[a]), hidden unit = relu(fmaf(sum,
 * *val_scale, val_bias[u])) -- the very operations, in the very order, of the GEMM kernels that reduce the parts
 * themselves, so every route gives the same bits. */
typedef struct rz_raw_heads {
    const float *raw;
    const float *hid;
    const float *w2;
    const float *b2;
    const float *act_scale; /* [1], n_parts == 4 only */
    const float *act_bias;  /* [ld] */
    const float *val_scale; /* [1] */
    const float *val_bias;  /* [64] */
    int64_t raw_part_stride;
    int64_t hid_part_stride;
    int32_t ld;
    int32_t n_parts;
} rz_raw_heads;

/* rz_expand_backup / rz_tree_step fed with those outputs: log_softmax and tanh(hid . w2 + b2) are finished inside the
 * tree kernel (same wave per game), saving the separate rz_net_heads finishing launch.  Pair with
 * rz_net_trunk(.., NULL, ..) + rz_net_heads_gemm.  Bit-identical to the un-fused route. */
int rz_expand_backup_raw(rz_engine *e, const rz_raw_heads *heads, void *stream);
int rz_tree_step_raw(rz_engine *e, const rz_raw_heads *heads, float *d_obs, void *stream);

/* ---------------------------------------------------------------------------------------
 * DEFERRED PRIORS (RZ_SCORE_UCT_REF, one simulation in flight per tree).  The reference's selection rule
 * (node.py:32-42,75-88) never reads TreeNode.prior: what the NEXT simulation of a tree depends on is the leaf VALUE
 * alone (alphazero_mcts.py:59-71).  So the policy half of policy_value_fn (alphazero_agent.py:41-45: act_fc1,
 * log_softmax, exp) and TreeNode.expand's priors with their Dirichlet noise (node.py:44-73) need not sit between two
 * simulations: the tree step of this route finishes the value head, reserves the expanded node's prior block (same
 * offsets as the other routes), backs up and selects; the leaf's policy features wait in a per-step store and ALL
 * priors of a search are written by one batched GEMM + one kernel before anything reads them (tree reuse, read-outs).
 * Every number stored is the one the other routes store, except that the value head's first layer is summed in f32 by
 * the game's own workgroup (k ascending in eight slices) instead of by the FC GEMM: values agree to f32 rounding,
 * not bit for bit.  A step of a lane is TWO launches (trunk, tree step) instead of three.
 *
 * rz_value_head: what the trunk of this route leaves for the tree step (rz_net_trunk_leaves_deferred). */
typedef struct rz_value_head {
    const float *valfeat; /* [rows][ld]: ReLU'd outputs of val_conv1, plane-major (2 x S), zero padded to ld */
    const float *w1t;     /* val_fc1.weight as [groups][64 hidden units][4 inputs] (inputs zero padded to 4 * groups) */
    const float *b1;      /* [64] val_fc1.bias */
    const float *w2;      /* [64] val_fc2.weight */
    const float *b2;      /* [1] */
    int32_t ld;           /* = 4 * groups */
    int32_t groups;       /* 16, 32, 64 or 128: four waves of the game's workgroup x 2 halves x 2, 4, 8 or 16 groups; 4 * groups
                           * >= 2 * S (refused otherwise): the tree step also sizes its bitboard arithmetic by it -- a head of
                           * 16 / 32 groups means a board of at most 64 cells, one 64-bit word per colour */
} rz_value_head;
/* rz_deferred_logits: the policy logits of the stored leaves after rz_net_deferred_gemm: row = slot * rows_per_slot + leaf */
typedef struct rz_deferred_logits {
    const float *raw; /* [n_slots * rows_per_slot][ld], final (scaled, bias added): what k_heads_split leaves */
    int32_t ld;
    int32_t rows_per_slot;
} rz_deferred_logits;
/* Room for `slots` steps between two flushes (per game: a pending-expansion record of 80 bytes per slot).  Needs
 * RZ_SCORE_UCT_REF and sims_in_flight == 1. */
int rz_deferred_reserve(rz_engine *e, int32_t slots);
/* Opt-in device-side launch trace (rlzero_amd/csrc/rz_trace.h; rlzero_amd/trace.py): d_trace = uint64 [2 + 8 * slots * n_games] of
 * THIS engine's lane with [0] = slots (steps of a search) and [1] = n_games filled in, or NULL to detach.  The deferred route's
 * kernels launched AFTERWARDS (a hipGraph keeps what it captured) leave one record per workgroup: start / end on the 100 MHz
 * clock, step, block, CU; a search overwrites the records of the one before it.  A diagnostic: traced instantiations of the
 * kernels run, not the production ones. */
int rz_trace_attach(rz_engine *e, void *d_trace);   /* the evaluator's half: rz_net_trace_attach below */
/* The engine's device view (pointers and geometry the tree code reads: rlzero_amd/csrc/rz_tree.h, struct Dev) for kernels of the
 * SAME build that run tree code outside the engine's own launches -- rz_net_search_resident.  out_bytes must be that build's
 * sizeof(Dev); valid until rz_destroy / the next rz_deferred_reserve. */
int rz_device_view(rz_engine *e, void *out, int64_t out_bytes);
/* Per-game simulation counts of rz_net_search_resident (ABI 28): d_counts int32 [n_games], every count >= 1 (the caller's to
 * check) -- game g runs min(d_counts[g], n_sims) simulations of a launch, whose n_sims stays the maximum the store slots are
 * reserved for; the trees, priors and values of a game are those of a uniform search with its count.  d_order (or NULL: identity)
 * int32 [n_games], a permutation: workgroup b of k_delta_res searches game d_order[b] (longest first keeps a full search out of
 * the last round of a grid beyond two games per CU; the other resident kernels keep the identity).  Both arrays are copied on
 * `stream`.  d_counts NULL clears them.  They come before rz_play_set_cap's budgets while set.  RZ_ERR_ARG on an engine without the
 * resident search's route (RZ_SCORE_PUCT, sims_in_flight > 1), and from the step-by-step tree calls while counts are set. */
int rz_set_playouts(rz_engine *e, const int32_t *d_counts, const int32_t *d_order, void *stream);
/* What the resident search reads: the counts and the order in force (rz_set_playouts', else rz_play_set_cap's, else NULL / NULL) */
int rz_playouts_view(rz_engine *e, const int32_t **d_counts, const int32_t **d_order);
/* Host copies of both for inspection (synchronous): *h_source = 0 none in force, 1 rz_set_playouts', 2 rz_play_set_cap's, | 4 when an
 * order is in force (h_order is written then, h_counts whenever *h_source != 0; either may be NULL) */
int rz_playouts_read(rz_engine *e, int32_t *h_counts, int32_t *h_order, int32_t *h_source);
/* int32 [n_games]: the store slot the NEXT leaf of each game goes to (= steps since the last flush); the trunk reads it */
int rz_deferred_slots(rz_engine *e, const int32_t **d_slot_of_game);
/* rz_expand_backup / rz_tree_step of this route (pair with rz_select_step(e, NULL, ..) + rz_net_trunk_leaves_deferred) */
int rz_expand_backup_deferred(rz_engine *e, const rz_value_head *head, void *stream);
int rz_tree_step_deferred(rz_engine *e, const rz_value_head *head, void *stream);
/* Writes the priors of every expansion pending in slots [0, n_slots) -- exp(log_softmax) over the leaf's legal moves mixed
 * with its Dirichlet noise: the operations of rz_expand_backup_raw -- and empties the slots.  Must run before
 * rz_advance_roots / rz_set_roots / the prior read-outs; without pending slots a no-op. */
int rz_deferred_flush(rz_engine *e, const rz_deferred_logits *logits, int32_t n_slots, void *stream);
/* The kept flush (ABI 29), for the move step on the device: between rz_play_draw and rz_play_apply the move is known, and the only
 * priors of the search that anything can read afterwards are those of the blocks that survive update_with_move -- the kept child's
 * subtree and the root's own block.  Priors exist for every block a caller can reach; blocks of subtrees a move discards are never
 * written.  rz_deferred_keep lists the pending records that are needed -- leaf board == root board; or the mover's stone on the
 * cell of the move (every leaf below the kept child, and harmlessly a transposition); or every record with a block where no move
 * was drawn (a stall, a resignation) -- as rows[i] = slot * n_games + game, game-major, slots ascending, *count of them (device
 * memory: the launches that follow read it there).  rz_net_deferred_gemm_rows forms the logits of listed row i in row i of its
 * output; rz_deferred_flush_kept writes those records' priors, the operations of rz_deferred_flush on the same numbers.  RZ_ERR_ARG
 * outside a drawn move.  Every other reader of priors (read-outs, rz_advance_roots, rz_set_roots) needs rz_deferred_flush. */
typedef struct rz_kept_rows {
    const int32_t *rows;  /* device, [capacity] */
    const int32_t *count; /* device, [1] */
    int64_t capacity;     /* slots reserved * n_games */
    int32_t n_games;
    int32_t reserved;
} rz_kept_rows;
int rz_deferred_keep(rz_engine *e, rz_kept_rows *out, void *stream);
int rz_deferred_flush_kept(rz_engine *e, const rz_deferred_logits *logits, void *stream);
/* Policy on demand (ABI 32; rz_net_search_resident_values): the pending records carry no policy features, so EVERY flush goes by rows --
 * rows (rz_deferred_keep, or rz_deferred_keep_all: every record with a block of every game, inside a drawn move or outside one; it
 * leaves rz_deferred_keep_stats alone) -> rz_net_policy_rows -> rz_net_deferred_gemm_rows -> rz_deferred_flush_kept, or outside a drawn
 * move rz_deferred_flush_rows: the same priors over the listed rows, and the slots emptied as rz_deferred_flush empties them.  A pending
 * record also holds its leaf's side to move and last move (one word; every deferred route writes it). */
int rz_deferred_keep_all(rz_engine *e, rz_kept_rows *out, void *stream);
int rz_deferred_flush_rows(rz_engine *e, const rz_deferred_logits *logits, void *stream);
/* h_out2 = {records listed, records with a block (what rz_deferred_flush would have written)} over the rz_deferred_keep calls since
 * the last reset; synchronises */
int rz_deferred_keep_stats(rz_engine *e, uint64_t *h_out2, int32_t reset);

/* Root statistics after the simulations (AlphaZeroMCTS.simulate, alphazero_mcts.py:88-90):
 * visit count / W of the root child of every action, 0 for illegal or unvisited actions;
 * [n_games][B*B].  rz_root_stats: N and W of the roots themselves, [n_games]. */
int rz_root_visits(rz_engine *e, int32_t *d_visits, void *stream);
int rz_root_wsum(rz_engine *e, double *d_w, void *stream);
int rz_root_priors(rz_engine *e, float *d_p, void *stream);
int rz_root_stats(rz_engine *e, int32_t *d_n, double *d_w, void *stream);
/* The values resignation looks at, one wave per game: d_out [n_games][2] fp64 = {v_root, q_best}, v_root = -W(root) / N(root) (the
 * root holds values as seen by the player who moved into it: the value for the player to move), q_best = max W(c) / N(c) over
 * the root's children with N > 0.  NaN where N(root) == 0 / no child is visited.  Separately rounded IEEE divisions: the bits
 * numpy gives for the same W and N. */
int rz_root_values(rz_engine *e, double *d_out, void *stream);

/* Tree reuse: AlphaZeroMCTS.update_with_move (alphazero_mcts.py:96-103).  d_moves[g] >= 0:
 * the subtree of that root child becomes the tree (statistics kept); -1: fresh tree
 * (reset_player, alphazero_mcts.py:132-134); -2: leave the game untouched.  Must be called
 * BEFORE rz_step_games for the same move (it ranks the move on the current root board). */
int rz_advance_roots(rz_engine *e, const int32_t *d_moves, void *stream);

/* GomokuEnv.step + game_end_winner on the root boards (gomoku_env.py:49-70,196-203):
 * d_moves[g] < 0 = no move.  d_winner: player id or -1 (tie / not ended); d_ended 0/1. */
int rz_step_games(rz_engine *e, const int32_t *d_moves, int32_t *d_winner, uint8_t *d_ended,
                  void *stream);

/* ---------------------------------------------------------------------------------------
 * THE MOVE STEP ON THE DEVICE.  What the self-play loop does between two searches -- AlphaZeroMCTS.simulate's read-out of the
 * root visits (alphazero_mcts.py:88-90), AlphaZeroPlayer.get_action's draw (:147-148), update_with_move (:96-103), env.step +
 * game_end_winner (game.py:109-118), reset_player at the end of a game (:128) and the start of the next one -- for every game
 * of the engine, enqueued on the stream with NO host round trip: the host keeps whole moves enqueued ahead and reads what
 * happened from a log, a move or more behind.
 *
 * The draw.  numpy.random.choice(acts, p=probs) of the reference is acts[searchsorted(cumsum(p) / cumsum(p)[-1], u, 'right')]
 * with p = softmax(log(N + 1e-10) / T) (alphazero_mcts.py:10-14,91-92).  The device evaluates the same expression in fp64 with
 * ITS log / exp (numpy's are not reproducible on another machine, let alone a GPU) on the uniform u = the counter-based
 * uniform of (seed, game id, ply) (rlzero_amd/selfplay.py: move_uniform -- integer arithmetic, the same bits) and draws the move
 * ONLY when u lies farther than stall_margin (relative to the total) from both edges of the chosen interval: rounding differences
 * between the two evaluations are ~1e-14, so the host's numpy expression on the logged visit counts -- the arbiter -- picks the
 * same move.  Otherwise the game STALLS: no move, the slot is skipped by the coming searches, and the host, reading the log,
 * decides with numpy and hands the move back (rz_play_resolve).  pi itself is never computed on the device: the host forms it
 * from the logged counts with the reference's expression (and verifies every move the device drew).
 *
 * The log: int32 [ring_steps][n_games][RZ_PLAY_RECORD_WORDS + A]; the record of move step s (counted per engine from
 * rz_play_attach) and slot g is row s % ring_steps.  Words: [0..1] game id (int64), [2] ply before the move, [3] the move (action)
 * or -1, [4] RZ_PLAY_* flags | (winner + 1) << 16, [5] N(root), [6] float bits of the draw's distance to the nearer interval edge
 * (relative), [7] the resignation statistic (below; 0 while resignation is off); then per action the visit count of the root
 * child, -1 for an illegal action.  The host must read a row before ring_steps more moves overwrite it.
 *
 * Resignation (AlphaGo Zero's rule; an opt-in extension -- the reference plays every game to its end -- off after every
 * rz_play_attach).  rz_play_set_resign(threshold, disabled_frac) turns it on: for every RUNNING slot that has just searched,
 * k_play_draw forms v_root = -W(root) / N(root) and q_best = max W(c) / N(c) over the root's children with N > 0 (the values of
 * rz_root_values) and logs s = max(v_root, q_best) (NaN when either is) as float bits in word [7].  A game whose uniform
 * u(seed, game id) -- splitmix64 keyed with a salt of its own (rlzero_amd/selfplay.py: resign_uniform, the same bits) -- is below
 * disabled_frac is a calibration game: it never resigns, its records carry RZ_PLAY_NO_RESIGN, and RZ_PLAY_WOULD_RESIGN where the
 * rule would have fired.  In every other game the mover resigns when v_root < threshold and q_best < threshold (NaN never
 * fires): no draw, move -1, flags RUNNING | SEARCHED | ENDED | RESIGNED, winner 1 - ply % 2 (player 0 moves first), and
 * rz_play_apply ends the game as it ends a finished one (fresh tree, slot idle, refill) without a game step.
 *
 * Playout cap randomization (KataGo, Wu 2019, section 3.1; an opt-in extension, off after every rz_play_attach; ABI 28).
 * rz_play_set_cap(n_fast, p_full) turns it on: the search before ply `ply` of game `gid` has the full budget n_playout when
 * cap_uniform(seed, gid, ply) < p_full -- a splitmix64 chain with a salt of its own (rlzero_amd/selfplay.py: cap_uniform, the same
 * bits) -- and n_fast simulations otherwise.  k_play_apply writes the budget of every slot that is running after the step (a
 * refilled slot at ply 0 included) into a device array that the resident search reads (min(budget, n_sims) simulations for the
 * game), a one-workgroup kernel behind it orders the slots -- full budget, fast, inactive; stable -- for k_delta_res's workgroups,
 * and k_play_draw sets RZ_PLAY_FULL on the searched records of full searches.  Only those are policy training samples; every
 * game still gives a value target.  Dirichlet noise and temperature are the same on both kinds of move.
 *
 * Per-ply temperature (AlphaGo Zero / AlphaZero: T = 1 for the first 30 plies, then T -> 0; KataGo: T decaying with a half-life of
 * about the board size; an opt-in extension, off after every rz_play_attach; ABI 33).  rz_play_set_temperatures hands over a host
 * table: T before ply p, the last entry for every later ply.  The library forms 1 / T on the host -- the IEEE division of
 * rz_play_attach's 1 / temperature, and Python's --, pads the table to the board's cell count and writes it in stream order into a
 * device array of its own, which k_play_draw indexes with the slot's ply (word [2] of the record: T follows from it, no record
 * word or flag changes).  The stall margin follows the ply: the configured stall_margin if positive, else 1e-10 * max(1, 1 / T)
 * with the ply's T.  A stalled slot keeps its ply, so the resolved move belongs to the same T.  The host forms pi and verifies
 * every move with the same table.  Noise and the search are untouched; a match keeps the temperature of rz_play_attach.
 *
 * Slots refill themselves: a slot whose game has ended (or that is idle) takes the next entry of a queue of game ids shared by
 * the engines (lanes) of a GPU -- d_queue_ids int64 [..], d_queue_ctl int32 [2] = {head, entries valid}; the device advances
 * head atomically, the host may append ids and then raise the count -- and starts that game: empty board, player 0 to move, a
 * fresh tree, its Dirichlet stream keyed (seed, game id) exactly as rlzero_amd.selfplay keys it.
 *
 * Network-vs-network matches (an opt-in mode, off after every rz_play_attach; ABI 30): GameControl.start_play (game.py:61-94) with
 * two AlphaZeroPlayer(is_selfplay=False) (alphazero_mcts.py:136-165), each with a network of its own.  rz_play_set_match hands
 * over a table of openings -- legal, non-terminal positions -- and changes three things in the move step, none in a search kernel:
 *   * games 2k and 2k + 1 are a PAIR: a refilled slot starts from opening (game id >> 1) % n_openings (stones, side to move, last
 *     move; fresh tree; ply 0, counted from the opening), and network A is player 0 of the even game, player 1 of the odd one;
 *   * the draw's uniform is that of (seed, game id >> 1, 2 * ply + 1): the second of get_action's two draws (:157), shared by the
 *     two games of a pair -- a network against itself plays every pair as the same game twice;
 *   * every move is searched from a fresh root (reset_player, :158): k_play_apply drops the tree where it keeps the drawn child's
 *     subtree in self-play, after a resolved stall too.
 * rz_play_side(side) sets the engine's active flags to the running games whose mover is network `side`.  One move of a match, all
 * on one stream: rz_play_side(0), the resident search with A's evaluator, rz_play_side(1), the resident search with B's,
 * rz_play_draw, the flush of the pending priors, rz_play_apply.  Stalled and idle slots are searched by neither.  The log is the
 * one above; who won and by how much is the host's to say (rlzero_amd/match.py). */
#define RZ_PLAY_RECORD_WORDS 8
enum {
    RZ_PLAY_RUNNING = 1,   /* the slot holds a game: the visit counts are valid */
    RZ_PLAY_STALLED = 2,   /* no move drawn (u too close to an interval edge): waiting for rz_play_resolve */
    RZ_PLAY_RESOLVED = 4,  /* the move came from rz_play_resolve */
    RZ_PLAY_ENDED = 8,     /* the game ended with this move; winner + 1 in bits 16.. (0: tie) */
    RZ_PLAY_SEARCHED = 16, /* the slot took part in the search before this move step (n_playout simulations) */
    RZ_PLAY_RESIGNED = 32, /* the mover resigned (move -1, with RZ_PLAY_ENDED and the winner) */
    RZ_PLAY_NO_RESIGN = 64,     /* a calibration game: resignation disabled (every searched record of it while the rule is on) */
    RZ_PLAY_WOULD_RESIGN = 128, /* a calibration game's record where the rule would have fired */
    RZ_PLAY_FULL = 256     /* playout cap (rz_play_set_cap): a searched record whose search had the full budget; never set without a cap */
};
typedef struct rz_play_config {
    uint64_t seed;         /* move uniforms keyed (seed, game id, ply), Dirichlet streams keyed (seed, game id) */
    double temperature;    /* T of softmax(log(N + 1e-10) / T) */
    double stall_margin;   /* 0 -> 1e-10 * max(1, 1 / T); a test hook otherwise (0.05 stalls one draw in ten) */
    const int64_t *d_queue_ids;
    int32_t *d_queue_ctl;
    int32_t *d_log;        /* the log ring [ring_steps][n_games][8 + A]: device memory, or (what rlzero_amd passes) pinned host memory that
                            * the device can address -- the kernels only write it (one read-modify-write of a record's flags when its
                            * game ends), so the host reads rows in place behind an event and no copy sits between two moves; host
                            * memory that this engine's device cannot address is refused (hipHostGetDevicePointer) */
    int32_t ring_steps;
    int32_t reserved;
} rz_play_config;
/* Attach (allocates the per-slot state on first use; every slot idle, inactive, with a fresh tree; move step counter 0). */
int rz_play_attach(rz_engine *e, const rz_play_config *cfg);
/* The queue of game ids as a RING (ABI 45; for a collection that never stops the device: ids are appended while games run).
 * rz_play_queue_ring(e, capacity): from now on d_queue_ids holds `capacity` entries (the caller's to provide) and k_play_apply reads
 * the entry of head at head mod capacity (rz_play.h: queue_slot); head and the valid count stay ever-growing int32 counts.
 * Capacity 0 -- the default after every rz_play_attach -- is the linear queue.  Every engine (lane) that shares the queue takes the
 * same capacity.  The capacity is a kernel ARGUMENT of the move step: valid after rz_play_attach and before the first move step is
 * enqueued or captured, RZ_ERR_ARG afterwards.
 * rz_play_queue_push(e, first_id, count, stream): ONE small launch on `stream`, no host wait -- ids first_id .. first_id + count - 1
 * go behind the valid count, then the count is raised (vector stores, a fence, the count last: a k_play_apply that sees the new
 * count reads the ids).  The caller orders the push before the move steps that are to see it on other streams.  A push that would
 * overwrite an entry no slot has claimed, or take the valid count past the int32 range (rz_play.h: queue_room), writes nothing and
 * sets RZ_FLAG_QUEUE_FULL.  RZ_ERR_ARG for count > capacity, a negative count or id, and on a linear queue; count 0 launches nothing. */
int rz_play_queue_ring(rz_engine *e, int32_t capacity);
int rz_play_queue_push(rz_engine *e, int64_t first_id, int32_t count, void *stream);
/* After the search of a move, BEFORE rz_deferred_flush: read the root visits into the log, draw (or stall, or take a resolved
 * move).  One launch. */
int rz_play_draw(rz_engine *e, void *stream);
/* Then, in ONE launch (a wave per slot): update_with_move + env.step + game_end_winner with the moves just drawn, the end of finished
 * games and the refill of idle slots (rz_play_apply without a draw before it only refills: how a run starts).  A
 * rz_deferred_flush between the two calls leaves the restart of the pending-priors counters to this launch. */
int rz_play_apply(rz_engine *e, void *stream);
/* The resignation rule (above), enqueued on `stream` as a write into a small device buffer that k_play_draw reads -- not a kernel
 * argument: a captured move graph takes a new threshold without a new capture.  threshold NaN: off again (word [7] 0, no resign
 * flags).  disabled_frac in [0, 1].  Valid after rz_play_attach; a graph captured before the FIRST call since rz_play_attach keeps
 * the resignation-free draw (capture again). */
int rz_play_set_resign(rz_engine *e, double threshold, double disabled_frac, void *stream);
/* The playout cap (above), enqueued on `stream` as writes into small device arrays -- the rule and the budgets of the searches that
 * are coming under it: a captured move graph takes new values without a new capture.  n_fast in 1 .. n_playout, p_full in (0, 1];
 * p_full NaN: off again (every search n_playout simulations, no RZ_PLAY_FULL).  Valid after rz_play_attach on an engine of the
 * resident search's route (RZ_SCORE_UCT_REF, sims_in_flight == 1; RZ_ERR_ARG otherwise); a graph captured before the FIRST call
 * since rz_play_attach has no cap (capture again).  While a cap is set the step-by-step tree calls (rz_tree_step*,
 * rz_expand_backup*) return RZ_ERR_ARG: only rz_net_search_resident knows per-game budgets. */
int rz_play_set_cap(rz_engine *e, int32_t n_fast, double p_full, void *stream);
/* The temperature schedule (above): h_temps double [n] in HOST memory, T before ply p; plies >= n use h_temps[n - 1].  The table
 * travels as kernel arguments of small launches on `stream` that write the engine's device array -- not a kernel argument of the
 * draw: a captured move graph takes a new table without a new capture.  n == 0 (h_temps ignored): off again, every ply at
 * rz_play_attach's temperature, the same bits as before.  RZ_ERR_ARG for an entry that is not finite and positive, for n above the
 * board's cell count (rows x cols -- a game has no more plies; Connect4 too, whatever its action count) and while a match is on.
 * Valid after rz_play_attach; a graph captured before the FIRST call since rz_play_attach keeps the constant temperature (capture
 * again). */
int rz_play_set_temperatures(rz_engine *e, const double *h_temps, int32_t n, void *stream);
/* Whether the cap's searches take their workgroups in the partition's order (default) or in slot order (0: no order kernel in the
 * move step; a measurement's switch).  A host-side setting read when launches are enqueued: set it before a move graph is captured. */
int rz_play_set_cap_order(rz_engine *e, int32_t longest_first);
/* The root values of the move step (ABI 44; an opt-in extension: the value target of the learner, rz_replay_add_values).  d_ring:
 * float32 [ring_steps][n_games] of the caller, ring_steps as in rz_play_attach -- device memory, or pinned host memory the device can
 * address (as d_log) --; NULL: off again.  With a ring, lane 0 of a slot's wave in k_play_draw writes float32(v_root), v_root =
 * N(root) > 0 ? -(W(root) / N(root)) : NaN (rz_play.h: root_value; rz_root_values' [0], the same fp64 bits), into row
 * step % ring_steps for every slot that holds a game -- a stalled slot's root does not change, so its rows repeat the value of its
 * searched record -- and NaN for an idle slot.  The record's words and the visit counts are untouched (word [7] stays the
 * resignation statistic).  The ring is a kernel ARGUMENT of the draw: the call is valid after rz_play_attach and before the first
 * move step is enqueued or captured (a whole-move graph is then captured with the ring in it and stays one replay), RZ_ERR_ARG
 * afterwards and while a match is on; rz_play_set_match is refused while a ring is set.  rz_play_attach turns it off.  `stream` is
 * unused: nothing is enqueued. */
int rz_play_set_root_values(rz_engine *e, float *d_ring, void *stream);
/* FORCED PLAYOUTS AND POLICY TARGET PRUNING (ABI 47; an opt-in extension of RZ_SCORE_PUCT self-play after Wu 2019, section 3.2; the
 * two rules are rlzero_amd/csrc/rz_forced.h, in fp64, tested on the CPU).  With N the visit count of the ROOT RECORD (the N whose
 * square root the PUCT term uses; under tree reuse whatever the record holds) and n, p a root child's visit count and stored prior
 * (the noised one where noise is on):
 *   forced playouts   in the ROOT's child scan a child with n > 0 and n n < (k p) N scores +infinity; several such children resolve
 *                     by the first-maximum rule.  Deeper levels, and a root that is still a leaf, are untouched.
 *   pruning           the best child (the first with the largest n) keeps n; every other child loses playouts one at a time, at
 *                     most f of them (f the largest integer with f f <= (k p) N), while its PUCT at one playout fewer (its q = w / n
 *                     held constant) stays below the best child's PUCT; a child left with a single playout goes to 0.
 * rz_set_forced_playouts: k > 0 turns the rule on for every search of the engine that follows -- the three-launch step (rz_select_step,
 * rz_tree_step, rz_tree_step_raw) on any board and rz_net_search_resident_puct -- and 0 turns it off (the default: nothing changes).
 * RZ_ERR_ARG: an engine whose rule is not RZ_SCORE_PUCT, sims_in_flight > 1, a match that is on, k negative or not finite, and --
 * k travels in the kernel arguments -- once a move step has been enqueued or captured, or a ring of pruned counts set, since
 * rz_play_attach ("attach again").  (rz_play_set_match refuses every RZ_SCORE_PUCT engine, so no match can begin while k > 0.)
 * rz_root_pruned_visits: d_out int32 [n_games][A] <- the pruned count of every legal action of the roots, -1 for an illegal one
 * (k_root_pruned: one wave per game, the children in action order as rz_root_visits gives them); k == 0: the raw counts.
 * rz_play_set_pruned_visits: the same launch inside the device move step, in front of the draw (so a whole-move graph holds it and
 * stays one replay): d_ring int32 [ring_steps][n_games][A] of the caller -- device memory, or pinned host memory the device can
 * address --, row step % ring_steps aligned with the log's rows; a stalled slot repeats its searched row, an idle slot holds -1.
 * The log's records and its raw counts do not change: the move is still drawn from them.  NULL: off again.  Valid after
 * rz_play_attach with k > 0 and before the first move step is enqueued or captured; rz_play_attach turns it off.  `stream` unused. */
int rz_set_forced_playouts(rz_engine *e, double k);
int rz_root_pruned_visits(rz_engine *e, int32_t *d_out, void *stream);
int rz_play_set_pruned_visits(rz_engine *e, int32_t *d_ring, void *stream);
/* Match mode (above).  The table -- d_open_stones uint64 [n_openings][2][RZ_BOARD_WORDS], d_open_to_move / d_open_last int32
 * [n_openings], device memory -- is copied on `stream` into the engine's own; launches enqueued after the call read it.
 * n_openings == 0 (pointers ignored): off again.  Valid after rz_play_attach, before the games are queued, on an engine without
 * Dirichlet noise on the resident search's route (RZ_SCORE_UCT_REF, sims_in_flight == 1), with neither resignation nor a playout
 * cap nor a temperature schedule set since rz_play_attach: RZ_ERR_ARG otherwise -- and rz_play_set_resign / rz_play_set_cap /
 * rz_play_set_temperatures return RZ_ERR_ARG while it is on.
 * Like theirs, the flag is a kernel argument: with it off the move step reads and writes nothing more than before. */
int rz_play_set_match(rz_engine *e, const uint64_t *d_open_stones, const int32_t *d_open_to_move, const int32_t *d_open_last, int32_t n_openings,
                      void *stream);
/* The active flags of the coming search: slot g is searched iff it is running and its mover is network `side` (0 = A, 1 = B; A
 * moves iff (side to move == 0) == (game id even)).  One launch, a thread per slot.  RZ_ERR_ARG while match mode is off. */
int rz_play_side(rz_engine *e, int32_t side, void *stream);
/* A host copy of the active flags uint8 [n_games] for inspection (synchronous): what rz_set_active, the move step and rz_play_side
 * have left for the next search. */
int rz_active_read(rz_engine *e, uint8_t *h_active);
/* The host's decision for a stalled slot (one tiny launch); taken by the next rz_play_draw. */
int rz_play_resolve(rz_engine *e, int32_t slot, int32_t move, void *stream);
/* Drop every game: all slots idle with fresh trees (a run that stops early). */
int rz_play_stop(rz_engine *e, void *stream);
/* Host copies of the per-slot state for inspection (synchronous): game ids int64 [n_games] (-1: idle), plies int32, states
 * int32 (0 idle, 1 running, 2 stalled), and the move steps done so far. */
int rz_play_state(rz_engine *e, int64_t *h_game_id, int32_t *h_ply, int32_t *h_state, int64_t *h_steps);

/* Synchronises `stream`-independent state: waits for the device, then reports flags. */
int rz_get_stats(rz_engine *e, rz_stats *out);
int rz_clear_errors(rz_engine *e);
/* The cheap form for a per-move check (the single-game API polls after every search): waits for `stream` only and reads the OR of
 * the games' RZ_FLAG_* bits (and, optionally, the count of dropped subtrees) -- 4 + 4 bytes; rz_get_stats names the game when a
 * bit is set. */
int rz_poll_errors(rz_engine *e, int32_t *h_flags, int32_t *h_reuse_dropped, void *stream);

/* Inspection for parity tests: copies game `g`'s current arena to HOST arrays of max_slots
 * entries -- per node record: N, W, slot of the first child record (-1 = none yet), number of
 * visited children (= child records in use), number of children K (0 = not expanded), offset of
 * the node's block of K child priors -- plus the root's own prior and the used-slot count.
 * rz_copy_priors copies the prior arena those offsets index.  Synchronous. */
int rz_copy_arena(rz_engine *e, int32_t game, int64_t max_slots, int32_t *h_n, double *h_w,
                  int32_t *h_first_child, int32_t *h_n_visited, int32_t *h_n_children,
                  int32_t *h_prior_block, float *h_root_prior, int32_t *h_top);
int rz_copy_priors(rz_engine *e, int32_t game, int64_t max_floats, float *h_priors, int32_t *h_count);

/* The scoring arithmetic alone, for bit-exactness tests against CPython:
 * out[i] = w[i]/n[i] + c*sqrt(ln(np[i])/n[i]) with ln from the engine's table. */
int rz_uct_scores(rz_engine *e, const double *d_w, const int32_t *d_n, const int32_t *d_np,
                  double c_puct, double *d_out, int64_t count, void *stream);

/* ---------------------------------------------------------------------------------------
 * Policy-value network forward (the evaluator's dense contraction), hand-written MFMA kernels.
 * Replaces PolicyValueNet.forward (rlzero/games/gomoku/policy_value_net.py:34-52) for a batch
 * of leaf observations: conv3x3 4->32->64->128 (+ReLU), conv1x1 heads, the three FC layers,
 * log_softmax and tanh.  f32 results: the default trunk (RZ_NET_SPLIT_F16) carries every f32 operand of
 * conv1..conv3 as a pair of f16 values on the f16 matrix pipe and accumulates in f32 (error against fp64
 * at the level of the exact-f32 kernel, 1e-7 relative) and the FC GEMM that follows it does the same
 * (rz_net_set_heads_algo); the other algorithms use the f32-input MFMA.
 *
 * rz_net_load takes HOST pointers to the 16 tensors of PolicyValueNet.state_dict() in its
 * order (conv1.weight, conv1.bias, conv2.*, conv3.*, act_conv1.*, act_fc1.*, val_conv1.*,
 * val_fc1.*, val_fc2.*; policy_value_net.py:12-25), fp32, contiguous, torch layout.
 * rz_net_reserve sizes the internal feature buffer (the launch path never allocates).
 * The board is height x width (<= 16 x 16) and the policy head has n_actions outputs (Gomoku:
 * height = width = B, n_actions = B*B; Connect4: 6 x 7, 7).
 * rz_net_forward: d_obs float32 [n][4][H][W] -> d_logp [n][n_actions] (log-probabilities),
 * d_value [n].  rz_net_trunk exposes the first kernel alone: d_feat [n][6][B*B] = ReLU'd
 * outputs of act_conv1 (4 planes) and val_conv1 (2 planes); d_feat == NULL writes the
 * internal buffer that rz_net_heads (the FC layers + log_softmax + tanh) reads, so
 * rz_net_trunk(.., NULL, ..) + rz_net_heads == rz_net_forward (lets a caller time the
 * dominant kernel by itself). */
typedef struct rz_net rz_net;
enum {
    RZ_NET_DIRECT = 0,      /* conv2/conv3 as direct implicit GEMM on the f32-input MFMA: bit-for-bit a k-ordered fp32 fmaf
                               chain (the exact reference arithmetic; also what a net without finite activation bounds runs on) */
    RZ_NET_WINOGRAD_F4 = 1, /* conv2/conv3 as Winograd F(4x4,3x3) on the f32-input MFMA: 4x fewer multiply-adds than
                               DIRECT; fp32 throughout, ~1e-6 relative from DIRECT */
    RZ_NET_SPLIT_F16 = 2    /* default: conv1..conv3 as direct convolutions on the f16 matrix pipe with every f32 operand carried
                               as a hi + lo pair of f16 values (three MFMAs per product, f32 accumulation): as accurate as
                               DIRECT (1e-7 relative against fp64).  The f16 pieces of a layer's activations are stored times a
                               power of two that rz_net_load derives from bounds on the activations (observation planes in
                               [0, 1]), so weights of any scale stay in range on MCTS leaves; only inputs beyond [0, 1]
                               can overflow, which sets RZ_NET_FLAG_F16_RANGE.  Boards of 11 .. 16 rows and columns run
                               k_trunk_rows (v_mfma_f32_16x16x32_f16, one N-tile per board row, waves split the output
                               channels), all others k_trunk_split (32 x 32 x 16 tiles of whole rows, waves split the rows) */
    ,
    RZ_NET_SPLIT_F16_TILES = 3  /* the same arithmetic with k_trunk_split on every board size (the checker of k_trunk_rows:
                               the two agree to f32 accumulation rounding, not bit for bit -- the MFMA shapes sum in
                               different orders) */
    ,
    RZ_NET_SPLIT_F16_FP8 = 4 /* OPT-IN, narrower than the reference's f32 (never the default, never the benchmark's headline):
                               RZ_NET_SPLIT_F16 with the two CROSS terms hi x lo + lo x hi of conv3 (80 % of the trunk's products)
                               on the block-scaled FP8 pipe -- one v_mfma_scale_f32_16x16x128_f8f6f4 per tap (weights e4m3,
                               activations e5m2) instead of four f16 MFMAs, 2 f16-MFMA equivalents per product instead of 3.
                               The cross terms then carry 3 .. 4 bits instead of 11: ~2^-14 per product, between plain f16
                               (2^-11) and the default (2^-22); measured on the logits: DESIGN.md.  Boards of 11 .. 16 rows and
                               columns, position-fed entry points only (rz_net_trunk_leaves*, rz_net_search_resident);
                               rz_net_trunk / rz_net_forward (float planes) return RZ_ERR_ARG while it is selected. */
};
/* rz_net_range_info: h_info8 = {bound on conv1's, conv2's activations and on the head features for inputs in [0, 1];
 * the three activation scales chosen from them; 1.0 if the bounds are finite (0.0: RZ_NET_SPLIT_F16 runs RZ_NET_DIRECT
 * instead for this net); 0} -- valid after rz_net_load. */
int rz_net_range_info(rz_net *net, float *h_info8);
/* rz_net_error_flags: sticky bits set by the kernels since creation / the last call (synchronises the device) */
enum { RZ_NET_FLAG_F16_RANGE = 1 };
int rz_net_error_flags(rz_net *net, uint32_t *h_flags);
int rz_net_set_algo(rz_net *net, int32_t algo);
/* The Winograd trunk runs as persistent workgroups (one per CU: its LDS and registers fill a CU),
 * each looping over its boards.  max_workgroups > 0 caps their number so that the remaining CUs stay
 * free for the latency-bound tree / FC kernels of ANOTHER stream (a second lane of games) running
 * beside the trunk; 0 (default) = one workgroup per CU.  Workgroups are dealt to the 8 XCDs in turn:
 * use a multiple of 8. */
int rz_net_set_max_workgroups(rz_net *net, int32_t max_workgroups);
/* The first FC layers of the two heads (act_fc1, val_fc1; policy_value_net.py:43,48) as one GEMM over the leaf batch.
 * RZ_NET_HEADS_F32: the f32-input MFMA GEMM (32 x 32 output blocks, many small workgroups).  RZ_NET_HEADS_SPLIT_32 /
 * _64: on the f16 matrix pipe with hi + lo f16 operand pairs (k_heads_split, the arithmetic of RZ_NET_SPLIT_F16), 32 /
 * 64 boards per workgroup; needs the f16 feature pieces that the RZ_NET_SPLIT_F16 trunk writes into the internal
 * buffer, and falls back to F32 when the last trunk was another one.
 * RZ_NET_HEADS_AUTO (default): after the RZ_NET_SPLIT_F16 trunk SPLIT_64 when the trunk is capped by
 * rz_net_set_max_workgroups (the GEMM then has only the few CUs the trunk leaves free), otherwise SPLIT_PARTS up to 256
 * boards and SPLIT_32 above -- all give the same bits; F32 after the other trunks.  RZ_NET_HEADS_SPLIT_PARTS: the same arithmetic with NO reduction inside
 * the GEMM -- one single-wave workgroup per (32 boards x 32 outputs x K quarter), no LDS, few registers, so its waves fit on
 * a CU beside a resident trunk workgroup of another lane; the four partial sums are added by the consumer (the tree kernel
 * of the fused route, k_heads_finish otherwise; see rz_raw_heads) in the order the other shapes use: same bits again.
 * Choose before the trunk is launched: into the internal buffer the
 * RZ_NET_SPLIT_F16 trunk writes only what the chosen GEMM reads (F32 chosen later runs SPLIT on the pieces present). */
enum { RZ_NET_HEADS_AUTO = 0, RZ_NET_HEADS_F32 = 1, RZ_NET_HEADS_SPLIT_32 = 2, RZ_NET_HEADS_SPLIT_64 = 3, RZ_NET_HEADS_SPLIT_PARTS = 4,
       RZ_NET_HEADS_IN_TRUNK = 5   /* boards of up to 10 rows on the RZ_NET_SPLIT_F16 trunk: every trunk workgroup runs these layers on
                                      its own board behind the feature stage (no GEMM launch; the bits of the SPLIT shapes); what AUTO
                                      picks for an un-capped batch of at most one board per CU while the FC weights are at most 40 KB (6 x 6, Connect4);
                                      other boards: as AUTO */ };
int rz_net_set_heads_algo(rz_net *net, int32_t heads_algo);
int rz_net_create(int32_t height, int32_t width, int32_t n_actions, int32_t device, rz_net **out);
int rz_net_destroy(rz_net *net);
/* Uploads (and re-packs) the 16 tensors of PolicyValueNet.state_dict().  Later calls reuse the device
 * buffers of the first one, so launches captured in a hipGraph stay valid across weight updates.  Every
 * receptive-field base (rz_net_delta_bases) is invalidated: it was computed with the previous weights. */
int rz_net_load(rz_net *net, const float *const *h_params, int32_t n_params);
int rz_net_reserve(rz_net *net, int32_t max_boards);
int rz_net_trunk(rz_net *net, const float *d_obs, int32_t n_boards, float *d_feat, void *stream);
/* The RZ_NET_SPLIT_F16 trunk fed with the leaf POSITIONS instead of their float planes: d_stones uint64 [n][2][4]
 * (colour 0 / colour 1 bitboards, bit = cell), d_to_move, d_last_cell int32 [n] -- the engine's own leaf arrays
 * (rz_leaf_buffers).  The kernel builds the four planes of GomokuEnv.current_state (gomoku_env.py:95-114) itself; into
 * the internal feature buffer only (pair with rz_net_heads_gemm / rz_net_heads).  Same bits as rz_net_trunk on the planes
 * rz_select_step would have written. */
int rz_net_trunk_leaves(rz_net *net, const uint64_t *d_stones, const int32_t *d_to_move, const int32_t *d_last_cell,
                        int32_t n_boards, void *stream);
/* Deferred priors (see rz_value_head): room for `slots` steps of `max_boards` leaves in the policy-feature store
 * (slots x ceil(max_boards / 32) tiles of f16 pieces) and for their logits. */
int rz_net_deferred_reserve(rz_net *net, int32_t max_boards, int32_t slots);
/* rz_net_trunk_leaves of the deferred route: board b's policy features go to slot d_slot_of_board[b] of the store, its
 * value features (f32) to the rows of *out; no FC GEMM follows. */
int rz_net_trunk_leaves_deferred(rz_net *net, const uint64_t *d_stones, const int32_t *d_to_move, const int32_t *d_last_cell,
                                 int32_t n_boards, const int32_t *d_slot_of_board, rz_value_head *out, void *stream);
/* act_fc1 (policy_value_net.py:43) over the stored leaves of slots [0, n_slots) as ONE GEMM (k_heads_split's arithmetic) */
int rz_net_deferred_gemm(rz_net *net, int32_t n_boards, int32_t n_slots, rz_deferred_logits *out, void *stream);
/* The same GEMM over the listed rows of the store only (rz_deferred_keep): the A fragments are gathered row by row, the K quarters,
 * the MFMA order, the sum of the quarters and the epilogue are rz_net_deferred_gemm's -- the same bits -- and the logits of listed row
 * i are row i of `out` (rows_per_slot = 0: not slot-indexed).  A fixed grid strides over the device's count. */
int rz_net_deferred_gemm_rows(rz_net *net, const rz_kept_rows *kept, rz_deferred_logits *out, void *stream);
int rz_net_trace_attach(rz_net *net, void *d_trace);   /* see rz_trace_attach */
/* RECEPTIVE-FIELD ("delta") LEAF EVALUATION -- PolicyValueNet.forward (policy_value_net.py:34-52) on the leaves of a search WITHOUT
 * recomputing what the root already determines.  The reference's search is near breadth-first (alphazero_mcts.py:42-71 under
 * node.py:32-42: a 15 x 15 / 800 leaf is the root plus one or two stones), and three 3 x 3 convolutions move conv3's output only in
 * the 7 x 7 window around a changed cell.  rz_net_delta_bases evaluates, per game, two pseudo-positions of the ROOT (its stones seen
 * by the side to move / by the other side one stone later; no last-move plane) and keeps conv1's / conv2's outputs and the six head
 * feature planes in a cache (rz_net_delta_reserve: 209 KB per game); rz_net_delta_leaves then computes, per leaf, only the cells
 * inside the windows of the cells where its planes (gomoku_env.py:95-114) differ from the base of its parity, with k_trunk_rows'
 * arithmetic cell by cell, and takes every other cell from the base: THE SAME BITS as rz_net_trunk_leaves_deferred (the store slot
 * d_slot_of_board[b], the value rows of *out).  The cache validates itself: a leaf whose stones do not contain the cached root's, or
 * with more than four changed cells, or a game without bases, is evaluated by the same kernel without a base (four passes over
 * the board's quadrants) -- correct whatever the caller did, only slower; rebuild the bases whenever the roots move.  The bases
 * belong to the weights they were built with: rz_net_load invalidates every one of them, so after an upload a leaf takes the
 * route without a base until rz_net_delta_bases runs again -- correct, only slower; rebuild them after every rz_net_load too.
 * Boards of 11 .. 16 rows and columns, RZ_NET_SPLIT_F16.  d_active (may be NULL): games whose flag is 0 are skipped.  d_feat32 (may be
 * NULL): also the features as f32 [n][6][S] (tests); d_slot_of_board may then be NULL (nothing goes to the store; out may be NULL).
 * without_base != 0: every leaf takes the four-pass route (a checker). */
int rz_net_delta_reserve(rz_net *net, int32_t n_games);
int rz_net_delta_invalidate(rz_net *net, void *stream);
/* rz_net_search_resident on these boards, once the cache holds the engine's games: the resident search with THIS trunk (k_delta_res:
 * 82 KB of LDS, two games per CU, ANY number of games per launch -- a workgroup depends on nothing outside its game, so a grid beyond
 * 2 x CUs runs in rounds, a CU's free half going to the next game as a search ends; the bases of the roots are built by the call itself
 * when select_first != 0).  on = 0: the full-board resident kernel (one game per CU, at most CUs games) as before.  Default: on. */
int rz_net_delta_resident(rz_net *net, int32_t on);
int rz_net_delta_bases(rz_net *net, const uint64_t *d_root_stones, const int32_t *d_root_to_move, int32_t n_games, void *stream);
int rz_net_delta_leaves(rz_net *net, const uint64_t *d_stones, const int32_t *d_to_move, const int32_t *d_last_cell, int32_t n_boards,
                        const int32_t *d_slot_of_board, const uint8_t *d_active, float *d_feat32, int32_t without_base, rz_value_head *out,
                        void *stream);
/* the same on an engine's own arrays: the bases of every game from its ROOT positions (call whenever the roots have moved: after
 * rz_set_roots, rz_step_games, rz_play_apply -- a forgotten call costs time, not correctness), and rz_net_trunk_leaves_deferred's
 * step on its leaves (board b = game b, store slot pend[b], inactive games skipped).  One simulation in flight per tree. */
int rz_net_delta_bases_engine(rz_net *net, rz_engine *engine, void *stream);
int rz_net_delta_step(rz_net *net, rz_engine *engine, rz_value_head *out, void *stream);
/* ... and rz_net_trunk_leaves' step on its leaves: the features into the internal buffer's f16 tiles (policy and value K-steps),
 * rz_net_heads_gemm next -- the three-launch step (the opt-in PUCT rule) with this trunk.  One simulation in flight per tree;
 * RZ_NET_HEADS_F32 is refused (it reads f32 features).  Replaces the same reference lines as rz_net_trunk_leaves
 * (policy_value_net.py:34-46 on gomoku_env.py:95-114's planes). */
int rz_net_delta_trunk_engine(rz_net *net, rz_engine *engine, void *stream);
/* counters since the last reset (synchronises): {leaves evaluated against a base, leaves without one, conv3 tiles of 16 cells, changed
 * cells, conv2 tiles of 16 cells, root scans of the resident search answered from the pre-scan, and -- of workgroup 0 of the LAST resident launch -- its shader-clock cycles >> 8 and its ticks
 * of the constant 100 MHz clock: the clock the search ran at = 256 [6] / (10 ns [7])} */
int rz_net_delta_stats(rz_net *net, uint32_t *h_out8, int32_t reset);
/* RESIDENT SEARCH -- n_sims consecutive simulations of every active game of `engine` (AlphaZeroMCTS.simulate's loop,
 * alphazero_mcts.py:82-85) in ONE launch, one workgroup per game: trunk -> value head -> expand / backup -> next selection without
 * a kernel boundary, the leaf handed from the tree code to the trunk through LDS.  Kernels that hold a whole CU (151 KB of LDS: boards
 * of 8 .. 10 rows, and 11 .. 16 without rz_net_delta_reserve) take at most one game per CU (the single-game API, BASELINE configs[0]
 * and [1]); the two that hold half a CU -- k_delta_res (above; configs[3]) and k_trunk_split on the compact LDS grid (boards of up to 7
 * columns, 69 KB: TicTacToe .. 7x7, Connect4's 6x7 = configs[2]) -- take any number of games, two per
 * CU at a time.  The deferred-priors route's arithmetic and bookkeeping: the first leaf comes from
 * rz_select_step(engine, NULL, ..) before the call (select_first == 0: a search continued in pieces) or is selected by the launch
 * itself (select_first != 0: the same selection by the same code, one launch less); rz_net_deferred_gemm + rz_deferred_flush later;
 * the engine's slots advance by n_sims.  Same trees, values and priors as rz_net_trunk_leaves_deferred + rz_tree_step_deferred, bit for bit.
 * CONTRACT: game g's leaves go to store slots pend[g] .. pend[g] + n_sims - 1 (pend[g] = its steps since the last
 * rz_deferred_flush), so pend[g] + n_sims must not exceed the slots of rz_net_deferred_reserve / rz_deferred_reserve: flush first.
 * n_sims beyond either capacity is refused (RZ_ERR_ARG); a leaf whose slot still lies beyond the store (a caller that did not
 * flush) is not written anywhere and its game is flagged RZ_FLAG_INTERNAL by the tree code -- never an out-of-bounds write.
 * The same holds for rz_net_trunk_leaves_deferred (slot d_slot_of_board[b]). */
int rz_net_search_resident(rz_net *net, rz_engine *engine, int32_t n_sims, int32_t select_first, void *stream);
/* POLICY ON DEMAND (ABI 32).  Under RZ_SCORE_UCT_REF a search never reads a prior, and a move keeps well under 1 % of a search's
 * expansions: rz_net_search_resident_values is rz_net_search_resident whose leaves are evaluated for the two value planes only --
 * k_delta_res without the policy head sums, their shares and their stores; nothing is written to the feature store.  Trees, values
 * and records are rz_net_search_resident's, bit for bit.  It exists where k_delta_res runs (rz_net_delta_reserve for the engine's
 * games, rz_net_delta_resident on, a board of 11 .. 16 rows and columns): RZ_ERR_ARG elsewhere, never another kernel.  The records of
 * such a search must be flushed by rows: rz_net_policy_rows evaluates the listed records' leaves once more (the leaf from the record,
 * against the game's bases where they are still the leaf's; otherwise without a base) and writes their four policy planes to the
 * record's own place in the store -- the bits rz_net_search_resident writes there -- for rz_net_deferred_gemm_rows behind it.  Records
 * of the two kinds of search must not share a flush: flush between them. */
int rz_net_search_resident_values(rz_net *net, rz_engine *engine, int32_t n_sims, int32_t select_first, void *stream);
int rz_net_policy_rows(rz_net *net, rz_engine *engine, const rz_kept_rows *kept, void *stream);
/* RESIDENT SEARCH UNDER PUCT (ABI 46; opt-in: HipNetEvaluator.resident_puct).  rz_net_search_resident above is the deferred-priors
 * route's and refuses RZ_SCORE_PUCT, whose selection reads the priors of the node it stands on.  rz_net_search_resident_puct runs n_sims
 * simulations of every active game of a RZ_SCORE_PUCT engine in ONE launch, one workgroup per game, one game per CU: the trunk
 * (k_trunk_split, one N-tile per wave), the first FC layers of both heads on the game's own leaf inside the same workgroup (the arithmetic
 * of k_heads_split; final logits and the value head's hidden row in row g of the net's internal buffers), then the body of
 * rz_tree_step_raw -- log_softmax, tanh, priors with their Dirichlet noise, the dense child records, backup, next selection -- and the
 * next leaf handed to the trunk through LDS.  The trees, priors, values and noise counters of rz_net_trunk_leaves + rz_net_heads_gemm +
 * rz_tree_step_raw, bit for bit (policy_value_net.py:34-52, node.py:44-88, alphazero_mcts.py:49-85).  select_first as in
 * rz_net_search_resident; games whose active flag is 0 are skipped.  Nothing is stored for a flush: no rz_deferred_reserve, no
 * rz_net_deferred_reserve, no pending records.
 * RZ_ERR_ARG: an engine that is not RZ_SCORE_PUCT with one simulation in flight; a board of more than 10 rows or columns; a net
 * without the split-f16 trunk (RZ_NET_SPLIT_F16 with finite activation bounds); RZ_NET_HEADS_F32 (the three-launch step would then use
 * another arithmetic); an engine whose board is not the net's; more games than CUs; more games than rz_net_reserve()d.  Per-game
 * simulation counts (rz_set_playouts, the playout cap) and matches keep refusing RZ_SCORE_PUCT. */
int rz_net_search_resident_puct(rz_net *net, rz_engine *engine, int32_t n_sims, int32_t select_first, void *stream);
int rz_net_heads(rz_net *net, int32_t n_boards, float *d_logp, float *d_value, void *stream);
/* only the FC GEMM of the heads on the internal features; returns the device pointers that
 * rz_tree_step_raw / rz_expand_backup_raw consume (valid until the next rz_net_reserve / load) */
int rz_net_heads_gemm(rz_net *net, int32_t n_boards, rz_raw_heads *out, void *stream);
int rz_net_forward(rz_net *net, const float *d_obs, int32_t n_boards, float *d_logp,
                   float *d_value, void *stream);

/* ---------------------------------------------------------------------------------------
 * MuZero search tree (BASELINE.json configs[4]).  The reference only names
 * MuZero (README.md:3, rlzero/algorithms/rl_args.py:21-24); the algorithm is the published
 * pseudocode of arXiv:1911.08265v2 (run_mcts, select_child, ucb_score, expand_node, backpropagate,
 * MinMaxStats), single-player form.  The learned model stays with the caller: per simulation
 *   rz_mz_select         -> (parent slot, action, leaf slot) per game; the caller gathers the parents'
 *                           hidden states, runs dynamics + prediction on the batch, keeps the new
 *                           hidden state of game g at slot leaf[g];
 *   rz_mz_expand_backup  <- reward, policy PROBABILITIES [n_games][n_actions] (softmax evaluated by the
 *                           network head in fp32), value; expands the leaf and backs the value up with
 *                           the discount, updating the game's min-max statistics.
 * rz_mz_init_roots starts a search (expand_node(root, initial inference) + add_exploration_noise with
 * caller-supplied Dirichlet samples, fresh MinMaxStats).  d_mask (optional, [n_games] bytes): games with
 * 0 are left untouched.  Slots: root = 0; the children of a node are consecutive slots. */
typedef struct rz_muzero rz_muzero;
typedef struct rz_mz_config {
    int32_t abi_version; /* RZ_ABI_VERSION */
    int32_t n_games;
    int32_t n_actions;   /* 1..64 */
    int32_t n_sims;      /* simulations per search (sizes the tree: 1 + n_actions * (n_sims + 1) slots) */
    double discount;     /* 0.997 */
    double pb_c_base;    /* 19652 */
    double pb_c_init;    /* 1.25 */
    int32_t device;
    int32_t reserved;
} rz_mz_config;

int rz_mz_create(const rz_mz_config *cfg, rz_muzero **out);
int rz_mz_destroy(rz_muzero *e);
/* log((n + pb_c_base + 1) / pb_c_base) for n = 0 .. n_sims + 1, filled at creation by the host libm;
 * this entry replaces it (e.g. with math.log's values from another host). */
int rz_mz_upload_log_table(rz_muzero *e, const double *h_table, int64_t count);
int rz_mz_init_roots(rz_muzero *e, const float *d_probs, const double *d_noise, double noise_frac,
                     const uint8_t *d_mask, void *stream);
int rz_mz_select(rz_muzero *e, int32_t *d_parent, int32_t *d_action, int32_t *d_leaf, const uint8_t *d_mask,
                 void *stream);
int rz_mz_expand_backup(rz_muzero *e, const float *d_reward, const float *d_probs, const float *d_value,
                        const uint8_t *d_mask, void *stream);
/* what: 0 = visit counts (int32), 1 = value sums, 2 = rewards, 3 = priors (float64) of the root's children,
 * [n_games][n_actions] */
/* The search in ONE launch (k_mz_search): the model of rlzero_amd/muzero/network.py -- dynamics g(s, a) -> (r, s'),
 * prediction f(s) -> (p, v), hidden size 64, <= 8 actions -- evaluated inside the kernel on the matrix pipe, a workgroup
 * keeping <= 16 games, its waves' weight fragments in registers and (when they fit) the games' trees in LDS for all n_sims
 * simulations.  rz_mz_set_search_shape: games per workgroup, 0 (default) = chosen from n_games and the CU count so that
 * every CU holds at least two workgroups when there are games enough (4 / 8 / 16).  rz_mz_load_model takes HOST pointers to 14 fp32 tensors in torch layout
 * ([out][in]): dyn1.weight [64][64 + A], dyn1.bias, dyn2.weight, dyn2.bias, rew1.weight, rew1.bias, rew2.weight [1][64],
 * rew2.bias, pre1.weight, pre1.bias, pol.weight [A][64], pol.bias, val.weight [1][64], val.bias; call again after every
 * optimiser step.  rz_mz_search: d_hidden float32 [n_games][slots_per_game][64] with slot 0 = the root's state from the
 * initial inference (rz_mz_init_roots first); runs n_sims simulations of every game and leaves every node's state at its slot.  The six trace arrays (all or none):
 * per simulation and game what the kernel selected and what its network returned, [n_sims][n_games] (probs:
 * x n_actions) -- the parity tests feed them to the CPython restatement of the pseudocode. */
int rz_mz_load_model(rz_muzero *e, const float *const *h_params, int32_t n_params, int32_t hidden);
int rz_mz_search(rz_muzero *e, float *d_hidden, int32_t n_sims, int32_t *d_trace_parent, int32_t *d_trace_action,
                 int32_t *d_trace_leaf, float *d_trace_reward, float *d_trace_probs, float *d_trace_value, void *stream);
int rz_mz_set_search_shape(rz_muzero *e, int32_t games_per_workgroup);
/* The value transform (ABI 43; csrc/rz_mz_value.h): MuZero's invertible h(x) = sign(x) (sqrt(|x| + 1) - 1) + eps x, eps = 0.001
 * (arXiv:1911.08265v2 appendix F), for a model whose scalar reward and value heads are trained on h of their targets (the paper's
 * categorical support is not built).  rz_mz_set_value_transform(e, 1): every launcher of k_mz_search -- rz_mz_search, rz_mz_play_env,
 * rz_mz_play_cartpole -- takes the kernel's VT instantiation, in which wave 0 replaces the network's reward and value of a simulation by
 * float32(h^-1(float64(.))) right after the heads are finished: before the trace arrays are written (they hold what entered the
 * backup) and before expand + backup.  The tree, its MinMax bounds, the root value of a record, what Reanalyse writes back and the
 * priorities therefore stay in raw units; the root's own predicted value is not used by the search and is not touched.  0 (the default):
 * the instantiations without it, the code of ABI 42.  The step-by-step route (rz_mz_expand_backup) takes what the caller hands it: the
 * caller applies the inverse.  No launch; takes effect with the next one. */
int rz_mz_set_value_transform(rz_muzero *e, int32_t on);
/* Whole MOVES of CartPole-v1 environments in one launch (k_mz_search with its MOVES stages): per move the initial
 * inference h(o) -> s0, f(s0) -> root priors (+ Dirichlet(alpha) noise, weight noise_frac; probabilities and noise are each
 * normalised in fp64, so the stored root priors sum to 1 within 1e-12), n_sims simulations, the action
 * drawn from visits ^ (1 / temperature) (arg-max at temperature <= 0), one record and the environment step with
 * auto-reset.  dirichlet_alpha >= 0.1, else RZ_ERR_ARG: a draw is a float32 Gamma(alpha) floored at 1e-30, and
 * P(Gamma(alpha, 1) < 1e-30) = 1e-30^alpha / Gamma(alpha + 1) is 3.5e-8 at the default 0.25 and 1.05e-3 at 0.1 but 3.2e-2 at
 * 0.05 and 0.128 at 0.03 -- when BOTH actions' draws are floored the noise is uniform where a Dirichlet draw is almost one-hot
 * (at 0.1: about one move in 10^6; at 0.03: one in 60).  rz_mz_load_representation: HOST pointers to rep1.weight [64][obs_dim], rep1.bias, rep2.weight [64][64],
 * rep2.bias (torch layout), beside rz_mz_load_model.
 * Whole moves run the four 64 x 64 layers on the f16 matrix pipe and keep d_hidden in their own format: a slot's 256 bytes
 * are 64 f16 "hi" values followed by 64 f16 "lo" values, the state of unit k being (hi[k] + lo[k]) / 16.
 * The environments: d_state float64 [n_games][4] (x, x_dot, theta, theta_dot), d_steps / d_episode int64 [n_games], updated
 * in place (initial states of an episode: the counter-based stream of rlzero_amd/muzero/cartpole.py keyed (env_seed,
 * environment, episode)).  Random draws come from a counter-based stream keyed (noise_seed, environment, episode, step).
 * The history stays on the device: a record is 8 + A float64 -- observation before the move (4) | action | reward | visit
 * counts (A) | root value | done; every move's record goes to d_ring [n_games][ring_steps][8 + A] at step % ring_steps
 * (global step index = first_step + move of the launch; ring_steps >= 500 + n_moves), d_episode_start int64 [n_games]
 * holds the step at which the running episode began.  When an episode ENDS its records are copied, as one contiguous run,
 * to d_arena [arena_rows][8 + A] and (environment, end step, length, first arena row) is appended to d_entries int64
 * [max_entries][4] -- the host reads finished episodes, not moves.  d_counters int64 [4], zeroed by the caller before the
 * launch: [0] arena rows claimed, [1] entries, [2] episodes that did not fit into the arena (their entry has row -1:
 * read them from d_ring). */
typedef struct rz_mz_cartpole_play {
    double *d_state;
    int64_t *d_steps, *d_episode, *d_episode_start;
    uint64_t env_seed, noise_seed;
    double noise_frac, dirichlet_alpha, temperature;
    double *d_ring;
    int32_t ring_steps, reserved;
    int64_t first_step;
    double *d_arena;
    int64_t arena_rows;
    int64_t *d_counters, *d_entries;
    int64_t max_entries;
} rz_mz_cartpole_play;
int rz_mz_load_representation(rz_muzero *e, const float *const *h_params, int32_t n_params, int32_t obs_dim, int32_t hidden);
int rz_mz_play_cartpole(rz_muzero *e, float *d_hidden, int32_t n_sims, int32_t n_moves, const rz_mz_cartpole_play *play, void *stream);
/* One step of n_envs CartPole-v1 environments (gymnasium classic_control/cartpole.py: Euler, tau 0.02, 500-step limit)
 * with auto-reset, in ONE launch: d_obs float32 [n_envs][4] = the observation AFTER the step (after the reset for a
 * finished environment), d_reward float32, d_terminated / d_truncated uint8.  It is rz_mz_env_step(RZ_MZ_ENV_CARTPOLE, ..., 500)
 * with every pointer required (the same kernel, the same bits): an action outside 0..1 is clamped to it, as there (the kernel this
 * entry point had of its own took every action other than 1 as 0; such input was never specified). */
int rz_cartpole_step(double *d_state, int64_t *d_steps, int64_t *d_episode, const int64_t *d_actions, int32_t n_envs, uint64_t seed,
                     float *d_obs, float *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, void *stream);
/* Moves kept on the device for any environment the library knows (ABI 41; csrc/rz_muzero_moves.h: k_mz_env_step, k_mz_env_move,
 * k_mz_root_noise; the rules: csrc/rz_mz_env.h).  kind: RZ_MZ_ENV_CARTPOLE (4 state doubles, 4 observations, 2 actions) or
 * RZ_MZ_ENV_ACROBOT (Acrobot-v1: 4 state doubles theta1, theta2, dtheta1, dtheta2; 6 observations cos / sin of the two angles and
 * the two velocities; 3 actions = torque -1, 0, +1; reward -1 per step, 0 for the step that reaches the goal).
 * rz_mz_env_step: one step of n_envs environments with auto-reset in ONE launch, d_state
 * float64 [n_envs][4], the time limit max_episode_steps an argument; d_obs float32 [n_envs][D] after the reset.  d_actions NULL:
 * no step, only d_obs is written (the observation of the current state; d_reward and the flags may be NULL then).
 * rz_mz_env_move: the move behind a finished search (rz_mz_search on the same stream), a thread per environment: the action from
 * the root's visit counts ^ (1 / temperature) (first maximum at temperature <= 0) with the whole moves' draw keyed (noise_seed,
 * environment, episode, step); the record obs (D) | action | reward | visits (A) | root value | done to d_ring [n_games]
 * [ring_steps][D + 4 + A] at step % ring_steps; the environment step; for a finished episode its run in d_arena, its entry
 * (environment, end step, length, first arena row or -1), d_episode_start, the next episode's initial state; the state; the next
 * observation to d_obs float32 [n_games][D].  Counters, entries, arena and ring are laid out as rz_mz_play_cartpole's (the caller
 * zeroes d_counters before the first move that uses an arena); ring_steps >= max_episode_steps, max_entries >= n_games.  The
 * tree's n_actions must be the environment's.
 * rz_mz_root_noise: d_eta float64 [n_games][n_actions] = the normalised Dirichlet(alpha) noise of the whole moves under their key
 * (noise_seed, environment, d_episode, d_steps), in the form rz_mz_init_roots takes; dirichlet_alpha >= 0.1 (see above), at most
 * 8 actions. */
#define RZ_MZ_ENV_CARTPOLE 0
#define RZ_MZ_ENV_ACROBOT 1
typedef struct rz_mz_env_play {
    double *d_state;
    int64_t *d_steps, *d_episode, *d_episode_start;
    uint64_t env_seed, noise_seed;
    double temperature;
    int64_t max_episode_steps;
    double *d_ring;
    int32_t ring_steps, reserved;
    int64_t step;
    double *d_arena;
    int64_t arena_rows;
    int64_t *d_counters, *d_entries;
    int64_t max_entries;
    float *d_obs;
} rz_mz_env_play;
int rz_mz_env_step(int32_t kind, double *d_state, int64_t *d_steps, int64_t *d_episode, const int64_t *d_actions, int32_t n_envs, uint64_t seed,
                   int64_t max_episode_steps, float *d_obs, float *d_reward, uint8_t *d_terminated, uint8_t *d_truncated, void *stream);
int rz_mz_env_move(rz_muzero *e, int32_t kind, const rz_mz_env_play *play, void *stream);
/* Whole MOVES of any environment the library knows, in one launch (ABI 42; k_mz_search<TREE_LDS, MOVES = true, Env>): what
 * rz_mz_play_cartpole does, with the environment's step, observation, reset, reward and action count taken from its trait in
 * csrc/rz_mz_env.h and the time limit from the play record.  kind: RZ_MZ_ENV_CARTPOLE or RZ_MZ_ENV_ACROBOT.  The play record is
 * rz_mz_cartpole_play's, field for field, followed by max_episode_steps; d_state is float64 [n_games][4] for both kinds, a record
 * is D + 4 + A float64 (CartPole 10, Acrobot 13), ring_steps >= max_episode_steps + n_moves.  RZ_ERR_ARG, with a message that names
 * the reason, for an unknown kind, a tree whose n_actions or a loaded representation whose obs_dim is not the environment's,
 * dirichlet_alpha < 0.1, a ring too small, or no representation loaded.  rz_mz_play_cartpole is this call with RZ_MZ_ENV_CARTPOLE
 * and max_episode_steps 500. */
typedef struct rz_mz_whole_play {
    double *d_state;
    int64_t *d_steps, *d_episode, *d_episode_start;
    uint64_t env_seed, noise_seed;
    double noise_frac, dirichlet_alpha, temperature;
    double *d_ring;
    int32_t ring_steps, reserved;
    int64_t first_step;
    double *d_arena;
    int64_t arena_rows;
    int64_t *d_counters, *d_entries;
    int64_t max_entries;
    int64_t max_episode_steps;
} rz_mz_whole_play;
int rz_mz_play_env(rz_muzero *e, int32_t kind, float *d_hidden, int32_t n_sims, int32_t n_moves, const rz_mz_whole_play *play, void *stream);
int rz_mz_root_noise(rz_muzero *e, const int64_t *d_episode, const int64_t *d_steps, uint64_t noise_seed, double dirichlet_alpha, double *d_eta,
                     void *stream);
int rz_mz_root_children(rz_muzero *e, int32_t what, void *d_out, void *stream);
int rz_mz_root_stats(rz_muzero *e, int32_t *d_n, double *d_value_sum, double *d_vmin, double *d_vmax, void *stream);
int rz_mz_geometry(rz_muzero *e, int32_t *slots_per_game, int64_t *device_bytes);
int rz_mz_error_flags(rz_muzero *e, int32_t *flags);
/* A read-only view of the trees (ABI 34; tests and debugging: both calls launch no kernel).
 * rz_mz_tree_nodes synchronises the device and copies every game's node records, h_nodes rz_mz_node [n_games][slots_per_game],
 * and tops, h_top int32 [n_games] (slots handed out so far; records at or past a game's top are stale), to the HOST.  Every
 * route leaves its complete trees there when a launch ends -- rz_mz_play_cartpole the trees of the launch's LAST move -- so
 * what a search did can be read back without a trace: slots are handed out in expansion order (the expanded non-root slots
 * sorted by first_child are the simulations in order), the children of slot s sit at first_child[s] + a, their priors are the
 * network's probabilities, reward is stored in the node, and a leaf's value follows from the backup identity
 * value_sum[s] = v[s] + sum over children (N_c * reward_c + discount * value_sum_c) (no v term for the root).
 * rz_mz_search_plan: what a launch of the fused search (whole_moves 0: rz_mz_search) or of whole moves (whole_moves 1:
 * rz_mz_play_env / rz_mz_play_cartpole, for the tree's action count) would be for the current shape (rz_mz_set_search_shape), from the function the launch itself uses: games
 * per workgroup, whether the trees live in LDS (1) or stay in HBM (0), dynamic LDS bytes.  Any output pointer may be NULL. */
typedef struct rz_mz_node {
    int32_t n;           /* visit count */
    int32_t first_child; /* slot of the first child, -1 = not expanded */
    double value_sum;
    double prior;
    float reward;
    int32_t pad;
} rz_mz_node;
int rz_mz_tree_nodes(rz_muzero *e, void *h_nodes, int32_t *h_top);
int rz_mz_search_plan(rz_muzero *e, int32_t whole_moves, int32_t *games_per_workgroup, int32_t *tree_in_lds, int32_t *lds_bytes);

/* ---------------------------------------------------------------------------------------------------------------------
 * Device replay buffer (ABI 31; rz_replay.hip; an opt-in extension -- the reference's learner keeps its samples in a host
 * deque, tools/train_alphazero.py:32,59-79,88-90).  Gomoku, square boards of 3 .. 16 rows, A = B * B actions (Connect4: ABI 39,
 * the section after Reanalyse).
 *
 * The store is a ring of `capacity` self-contained POSITIONS (eviction is per position, nothing refers to a game):
 *   stones  uint64 [capacity][2][RZ_BOARD_WORDS]   [0] = the stones of the player to move, [1] = the opponent's (bit a = cell a)
 *   meta    int32  [capacity]                      bits 0..8 last move + 1 (0: none), bit 9 ply parity, bits 10..11 z + 1
 *   pi      float32[capacity][A]
 * The write cursor and the count are HOST state of the handle (rz_replay_state) and travel to the kernels as arguments.
 * Position j counts from the OLDEST one held; an ENTRY is e = 8 * j + k, k = the symmetry in get_equi_data's order
 * (train_alphazero.py:59-79) -- entry for entry what deque(maxlen = 8 * capacity).extend(get_equi_data(play_data)) holds.
 * Every call below takes a stream and is ordered on it; calls of one handle come from one host thread.
 *
 * rz_replay_set_tables: h_src_state / h_src_pi int16 [8][A] -- for output cell o of symmetry k the SOURCE cell of the planes
 *   and of pi.  Two different permutations (the reference rotates the planes by +k * 90 degrees and pi through a flipud /
 *   rot90 / flipud sandwich): the host obtains both by pushing arange(A) through the reference's numpy expressions
 *   (rlzero_amd/replay.py: symmetry_tables).  Entries outside 0 .. A-1 are refused.  Required before gather / sample.
 * rz_replay_add: n_games finished games in ONE launch (k_replay_add: a workgroup per game, a thread per ply).  h_offsets int32
 *   [n_games + 1] into h_moves int32 / h_keep uint8 (a game's plies; a game longer than A plies is refused), h_winner int32
 *   (0, 1, -1 = tie), h_pi float32 [kept plies of all games, in order][A].  Thread p forms the position before move p from the
 *   moves q < p (a stone of ply q is the mover's when q and p have the same parity) and z (+1 on the winner's plies, -1 on the
 *   loser's, 0 on a tie: game.py:121-126); the kept plies are compacted in ply order and written, with their pi rows, to
 *   consecutive ring slots modulo capacity; plies without a keep flag still place their stones.  Of more kept plies than the
 *   capacity only the last `capacity` are written.  One staging copy (pinned host memory of the handle) precedes the launch.
 * rz_replay_gather: n entries in ONE launch (k_replay_gather: a workgroup per entry, a thread per output cell) into
 *   d_states float32 [n][4][B][B] (own stones, the opponent's, the last move's one-hot, ones iff the ply is even:
 *   gomoku_env.py:95-114), d_pis float32 [n][A], d_zs float32 [n].  The indices are int64, from the host (h_indices: checked
 *   here, RZ_ERR_ARG for one outside 0 .. 8 * count - 1) or from the device (d_indices: checked by the kernel -- such an entry
 *   is not written and bit 1 of the flags of rz_replay_poll_errors is set); exactly one of the two is not NULL.
 * rz_replay_sample: the same kernel body with the indices drawn on the device (k_replay_sample): entry i of update `step` is
 *   mulhi64(x, 8 * count) of the splitmix64 chain x = sm(sm(sm(seed ^ "replay\0\0") ^ step) ^ i) -- WITH replacement, where
 *   random.sample draws without; integer only, every entry's probability within 2^-64 of 1 / (8 * count).
 *   rlzero_amd/replay.py: replay_index gives the same bits.  RZ_ERR_ARG on an empty buffer.
 * rz_replay_read: a SYNCHRONOUS copy of n raw records from position `first` (oldest = 0) to host arrays (any may be NULL).
 * rz_replay_poll_errors: the device's flag word (waits for `stream`), cleared by the call. */
typedef struct rz_replay rz_replay;
int rz_replay_create(int32_t board_size, int64_t capacity, int32_t device, rz_replay **out);
int rz_replay_destroy(rz_replay *r);
int rz_replay_set_tables(rz_replay *r, const int16_t *h_src_state, const int16_t *h_src_pi, void *stream);
int rz_replay_state(rz_replay *r, int64_t *count, int64_t *cursor, int64_t *capacity);
int rz_replay_add(rz_replay *r, int32_t n_games, const int32_t *h_offsets, const int32_t *h_moves, const uint8_t *h_keep,
                  const int32_t *h_winner, const float *h_pi, void *stream);
int rz_replay_gather(rz_replay *r, const int64_t *h_indices, const int64_t *d_indices, int64_t n, float *d_states, float *d_pis,
                     float *d_zs, void *stream);
int rz_replay_sample(rz_replay *r, uint64_t seed, uint64_t step, int64_t n, float *d_states, float *d_pis, float *d_zs,
                     void *stream);
int rz_replay_read(rz_replay *r, int64_t first, int64_t n, uint64_t *h_stones, int32_t *h_meta, float *h_pi, void *stream);
int rz_replay_poll_errors(rz_replay *r, int32_t *flags, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * Reanalyse for the device replay buffer (ABI 38; rz_replay.hip: k_replay_positions, k_replay_update_pi; rz_replay_rules.h;
 * rlzero_amd/replay.py: ReplayReanalyser): the two device ends of searching stored positions again with the current network.
 * Between them the caller hands the roots to a search engine (rz_set_roots takes exactly these arrays), searches, and reads the
 * visit counts (rz_root_visits).  No function or kernel above changes.
 *
 * rz_replay_positions: n positions in ONE launch (k_replay_positions: a thread per position and record word).  Position i (0 = the
 *   oldest held) is resolved to its physical ring slot, written to d_where int32 [n], and its record is written as a root in the
 *   engine's layout: d_stones uint64 [n][2][RZ_BOARD_WORDS] by PLAYER (the record's mover is player `parity`, its opponent
 *   1 - parity), d_to_move int32 [n] = the ply's parity, d_last_move int32 [n] = (meta & 511) - 1.  The indices are int64, from
 *   the host (h_indices: checked here, RZ_ERR_ARG for one outside 0 .. count - 1, and staged), from the device (d_indices: checked
 *   by the kernel), or, both NULL, the device's own draws of refresh `step`: position i is mulhi64(x, count) of
 *   x = sm(sm(sm(seed ^ "azreanal") ^ step) ^ i) -- uniform over POSITIONS, not entries: the eight symmetries of a position share
 *   one pi row (rlzero_amd/replay.py: replay_reanalyse_draws gives the same bits; the salt keeps a refresh and a mini-batch of
 *   one update number apart).  seed and step are ignored when indices are given.  A device index out of range: where = -1,
 *   nothing else written for the row, bit 1 of the flags of rz_replay_poll_errors set.  RZ_ERR_ARG on an empty buffer.
 *   *ticket receives the number of positions EVER stored in this handle (host state, advanced by rz_replay_add), also for n = 0.
 * rz_replay_update_pi: ONE launch (k_replay_update_pi: a workgroup per row, a thread per action).  For every row with
 *   0 <= where < capacity it writes pi[where][a] = (float)((double)max(N[a], 0) / (double)sum) from d_visits int32 [n][A], the sum
 *   taken over max(N, 0) in int64 (an integer reduction: exact in any order) -- the visit distribution, i.e. the reference's pi
 *   at temperature 1 up to rounding (a documented deviation from its softmax(log(N + 1e-10)) expression).  A sum of 0, or any
 *   other where -- the -1 of a refused or a padding row -- writes nothing; stones and meta are never written.  `ticket` must be what
 *   rz_replay_positions returned and still be the handle's counter: an add in between may have given a slot to another position,
 *   and the result of a search must never land there -- RZ_ERR_ARG, no launch.  Two rows that name one slot BOTH write it: the
 *   search is deterministic, so they carry the same bits.
 * rz_replay_ticket: the handle's counter as it is now (rz_replay_state keeps its three values). */
int rz_replay_ticket(rz_replay *r, int64_t *ticket);
int rz_replay_positions(rz_replay *r, const int64_t *h_indices, const int64_t *d_indices, uint64_t seed, uint64_t step, int64_t n,
                        int32_t *d_where, uint64_t *d_stones, int32_t *d_to_move, int32_t *d_last_move, int64_t *ticket, void *stream);
int rz_replay_update_pi(rz_replay *r, const int32_t *d_where, int64_t n, const int32_t *d_visits, int64_t ticket, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * The device replay buffer for Connect4 (ABI 39; rz_replay.hip: the <true> instantiations of k_replay_add / k_replay_gather /
 * k_replay_sample; rz_replay_rules.h: cell_of_ply, first_illegal_drop; rlzero_amd/replay.py: DeviceReplay(game='connect4')).
 * Build-defined, like RZ_GAME_CONNECT4 itself: the reference has no Connect4.  rz_replay_create and rz_replay_set_tables keep
 * their signatures and behaviour, and a Gomoku handle writes the bits it wrote before.
 *
 * A handle has a GAME and four sizes: C cells (rows * cols), A actions = the width of a pi row (Gomoku: C; Connect4: cols),
 * S symmetries (Gomoku: 8; Connect4: 2) and the column count.  An ENTRY is e = S * j + k: symmetry k of the j-th oldest position,
 * so 8 * count above reads S * count.  The record of a Connect4 position is the Gomoku record over CELLS (cell = row * cols +
 * column, row 0 at the bottom): two bitboards, the meta word -- its "last move + 1" field holds the last CELL + 1, which is what
 * plane 2 marks and what rz_set_roots takes as the last move of a Connect4 root -- and a pi row of `cols` floats.
 * The two symmetries: k = 0 the position as played, k = 1 its left-right mirror (every plane [:, :, ::-1], pi[::-1]); the
 * rotations of a square board do not exist under gravity.  As for Gomoku they are tables the host obtains by pushing cell and
 * column numbers through those numpy expressions (rlzero_amd/replay.py: symmetry_tables(..., game='connect4')).
 *
 * rz_replay_create_game: game_kind RZ_GAME_GOMOKU (rows == cols, 3 .. 16: rz_replay_create) or RZ_GAME_CONNECT4 (rows and cols
 *   1 .. 16 each, rz_create's limit).
 * rz_replay_set_tables_game: h_src_state int16 [n_symmetries][n_cells], h_src_pi int16 [n_symmetries][n_actions]; the three
 *   sizes must be the handle's (RZ_ERR_ARG otherwise), entries outside 0 .. n_cells - 1 / 0 .. n_actions - 1 are refused.
 *   rz_replay_set_tables is this call with (8, A, A) and refuses a Connect4 handle.
 * rz_replay_geometry: the handle's game and sizes (any pointer may be NULL).
 * rz_replay_add on a Connect4 handle: h_moves are COLUMNS; a column outside 0 .. cols - 1, or a column played more often than
 *   the board has rows, is refused before the launch (RZ_ERR_ARG), as a move outside the board is for Gomoku.  The kernel turns
 *   the columns into cells -- the cell of ply q is (plies q' < q in the same column) * cols + column, a thread per ply over the
 *   move list in LDS -- and forms the positions from the cells as before.  h_pi is [kept plies][cols].
 * rz_replay_gather / rz_replay_sample on a Connect4 handle: a thread per CELL; d_states float32 [n][4][rows][cols], d_pis
 *   float32 [n][cols] (written by the first `cols` threads).  rz_replay_positions is unchanged (d_last_move is the last cell);
 *   rz_replay_update_pi takes d_visits int32 [n][cols]. */
int rz_replay_create_game(int32_t game_kind, int32_t rows, int32_t cols, int64_t capacity, int32_t device, rz_replay **out);
int rz_replay_set_tables_game(rz_replay *r, int32_t n_symmetries, int32_t n_cells, int32_t n_actions, const int16_t *h_src_state,
                              const int16_t *h_src_pi, void *stream);
int rz_replay_geometry(rz_replay *r, int32_t *game_kind, int32_t *rows, int32_t *cols, int32_t *n_cells, int32_t *n_actions,
                       int32_t *n_symmetries);

/* ---------------------------------------------------------------------------------------------------------------------
 * Value targets from the search (ABI 44; rz_replay.hip: k_replay_add<.., true>, k_replay_gather<.., true>, k_replay_sample<.., true>,
 * k_replay_update_q; rz_replay_rules.h: value_target; rlzero_amd/replay.py: mixed_value_targets).  Opt-in, both games; without
 * rz_replay_enable_values nothing is allocated and every call above launches the kernels of ABI 43.
 *
 * rz_replay_enable_values: a float32 array q [capacity] beside the meta words, every slot NaN.  Only while nothing has been stored
 *   in the handle (RZ_ERR_ARG afterwards); a second call is a no-op.
 * rz_replay_add_values: rz_replay_add with h_q float32 [kept plies] -- the root value the mover's search saw at every kept ply
 *   (rz_play_set_root_values), in the order of h_pi's rows -- stored in q beside the position.  h_q NULL, or rz_replay_add on a
 *   handle with values: NaN.  RZ_ERR_ARG for h_q on a handle without values.
 * rz_replay_set_value_mix: lam in [0, 1] (default 0) of the value target rz_replay_gather / rz_replay_sample write,
 *   zs[i] = isnan(q) ? z : float32((1 - lam) * double(z) + lam * double(q)) -- fp64, each product rounded before the sum (no fused
 *   multiply-add).  lam travels to the kernels by value.  At lam = 0 the kernels without q run and zs is z, the bits of ABI 43.
 *   RZ_ERR_ARG for lam outside [0, 1] (NaN included) and for lam > 0 on a handle without values.  Host state: no launch.
 * rz_replay_update_values: Reanalyse's way back for q, ONE launch (k_replay_update_q: a thread per row).  d_where int32 [n] as
 *   rz_replay_positions wrote it, d_root_values float64 [n][2] as rz_root_values writes it ([0]: the root value for the player to
 *   move): q[d_where[i]] = float32(d_root_values[i][0]).  A row with d_where < 0 or outside the capacity, or a NaN value, writes
 *   nothing; stones, meta, pi and every other slot stay as they are.  `ticket` as in rz_replay_update_pi: RZ_ERR_ARG, and nothing
 *   launched, if positions were stored since rz_replay_positions.  RZ_ERR_ARG on a handle without values.
 * rz_replay_read_values: a SYNCHRONOUS copy of q of n positions from position `first` (oldest = 0), like rz_replay_read. */
int rz_replay_enable_values(rz_replay *r, void *stream);
int rz_replay_add_values(rz_replay *r, int32_t n_games, const int32_t *h_offsets, const int32_t *h_moves, const uint8_t *h_keep,
                         const int32_t *h_winner, const float *h_pi, const float *h_q, void *stream);
int rz_replay_set_value_mix(rz_replay *r, double lam);
int rz_replay_update_values(rz_replay *r, const int32_t *d_where, int64_t n, const double *d_root_values, int64_t ticket, void *stream);
int rz_replay_read_values(rz_replay *r, int64_t first, int64_t n, float *h_q, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * MuZero device replay (ABI 35; rz_mz_replay.hip, rz_mz_target.h; an opt-in extension beside the host ReplayBuffer of
 * rlzero_amd/muzero/selfplay.py).  Limits: obs_dim D <= 16, n_actions A <= 8, unroll_steps K 1 .. 16, td_steps 1 .. 64,
 * max_episode_steps T <= 65536, capacity E <= 2^22 episodes and E * T <= 2^30 steps: RZ_ERR_ARG otherwise, before any launch.
 *
 * The store is fixed stride -- episode slot e holds up to T steps -- and structure of arrays:
 *   obs        float32 [E][T][D]        action  int32   [E][T]        reward  float64 [E][T]
 *   root_value float64 [E][T]           policy  float32 [E][T][A]     length  int32   [E]
 * The slots form a ring over EPISODES; the write cursor, the count and a copy of the lengths are HOST state of the handle
 * (rz_mz_replay_state; h_lengths int32 [count], oldest first, may be NULL) and travel to the kernels as arguments.  Episode j
 * counts from the OLDEST one held: after any sequence of add / ingest calls the store holds what the host
 * ReplayBuffer(capacity = E) holds after `add` of the same episodes in the same order (empty episodes skipped, the oldest
 * dropped when full).  Every call below takes a stream and is ordered on it; calls of one handle come from one host thread.
 *
 * rz_mz_replay_create: h_disc float64 [td_steps + 1] = discount ** i as the HOST evaluates it (the very expression of
 *   ReplayBuffer._value_target): no pow runs on the device.
 * rz_mz_replay_add: n_episodes episodes in ONE launch (k_mzr_add: a workgroup per episode, a wave per step row, lanes across
 *   the row).  h_rows float64 [sum of h_lengths][D + 4 + A], the episodes one behind the other, every row a packed record of
 *   rz_mz_play_cartpole: obs (D) | action | reward | visit counts (A) | root value | done.  The policy stored is
 *   (float)(visits / sum(visits)) with the division in fp64 (EpisodeSeq.fields_of_packed's expression); an episode whose
 *   h_flags entry (may be NULL = 0) has bit 0 set carries the float32 POLICY in those columns, which is only cast.  obs is cast to
 *   float32.  An episode longer than T, an action outside 0 .. A-1: RZ_ERR_ARG, nothing is stored.  One staging copy precedes
 *   the launch.
 * rz_mz_replay_ingest: the same kernel body (k_mzr_ingest) reading the rows from DEVICE memory -- d_arena float64
 *   [arena_rows][row_doubles], the arena of a launch of rz_mz_play_cartpole on the same stream -- by the entries (h_lengths[i],
 *   h_first_rows[i]); only the entry table is staged.  row_doubles must be D + 4 + A and every run of rows must lie inside
 *   0 .. arena_rows - 1 (RZ_ERR_ARG; the kernel checks again and sets RZ_MZ_REPLAY_BAD_ROWS instead of reading outside).
 * rz_mz_replay_gather: n entries in ONE launch (k_mzr_gather: a thread per entry and unroll step) into d_obs float32 [n][D],
 *   d_actions int64 [n][K], d_tv / d_tr / d_mask float32 [n][K + 1], d_tp float32 [n][K + 1][A] -- ReplayBuffer.sample's six
 *   arrays for those draws, bit for bit.  The draws are int64 [n][K + 2]: episode, position, the K filler actions (used for
 *   actions[., k] when step position + k lies past the end), from the host (h_draws: checked here, RZ_ERR_ARG) or from the device
 *   (d_draws: checked by the kernel -- such an entry is not written and RZ_MZ_REPLAY_BAD_INDEX is set); exactly one is not NULL.
 *   Row k at step i = position + k: inside the episode (i < length) the value target is
 *   (float)((i + td < length ? root_value[i + td] * disc[td] : 0.0) + reward[i] * disc[0] + reward[i + 1] * disc[1] + ...) over
 *   the steps below min(i + td, length), summed in ascending order in fp64 (the build's -ffp-contract=off keeps multiply and
 *   add apart), the policy row is the stored one and the mask 1; outside: 0, the uniform policy (float)(1.0 / A), 0.  For k > 0
 *   the action and reward are those of step i - 1 while i - 1 < length, else the filler and 0.
 * rz_mz_replay_sample: the same rows with the draws made on the device (k_mzr_sample): counter c = i * (K + 2) + j of update
 *   `step` gives mulhi64(x, m) of the splitmix64 chain x = sm(sm(sm(seed ^ "mzreplay") ^ step) ^ c) -- j = 0 the episode, m =
 *   count; j = 1 the position, m = that episode's length (the host buffer's distribution); j = 2 + k the filler of actions[., k],
 *   m = A.  rlzero_amd/muzero/replay.py: mz_replay_draws gives the same bits.  RZ_ERR_ARG on an empty buffer.
 * rz_mz_replay_read: a SYNCHRONOUS copy of episodes first .. first + n - 1 (oldest = 0) to host arrays of the store's stride
 *   ([n][T][..], h_length [n]; any may be NULL).
 * rz_mz_replay_poll_errors: the device's flag word (waits for `stream`), cleared by the call. */
#define RZ_MZ_REPLAY_BAD_INDEX 1 /* a draw from the device was out of range */
#define RZ_MZ_REPLAY_BAD_ROWS 2  /* an entry's rows lay outside its block */
typedef struct rz_mz_replay rz_mz_replay;
int rz_mz_replay_create(int32_t obs_dim, int32_t n_actions, int64_t capacity_episodes, int32_t max_episode_steps, int32_t unroll_steps,
                        int32_t td_steps, const double *h_disc, int32_t device, rz_mz_replay **out);
int rz_mz_replay_destroy(rz_mz_replay *r);
int rz_mz_replay_state(rz_mz_replay *r, int64_t *count, int64_t *cursor, int64_t *capacity, int32_t *h_lengths);
int rz_mz_replay_add(rz_mz_replay *r, int32_t n_episodes, const int32_t *h_lengths, const int32_t *h_flags, const double *h_rows,
                     void *stream);
int rz_mz_replay_ingest(rz_mz_replay *r, int32_t n_episodes, const int32_t *h_lengths, const int64_t *h_first_rows, const double *d_arena,
                        int64_t arena_rows, int32_t row_doubles, void *stream);
int rz_mz_replay_gather(rz_mz_replay *r, const int64_t *h_draws, const int64_t *d_draws, int64_t n, float *d_obs, int64_t *d_actions,
                        float *d_tv, float *d_tr, float *d_tp, float *d_mask, void *stream);
int rz_mz_replay_sample(rz_mz_replay *r, uint64_t seed, uint64_t step, int64_t n, float *d_obs, int64_t *d_actions, float *d_tv,
                        float *d_tr, float *d_tp, float *d_mask, void *stream);
int rz_mz_replay_read(rz_mz_replay *r, int64_t first, int64_t n, float *h_obs, int32_t *h_action, double *h_reward, double *h_root_value,
                      float *h_policy, int32_t *h_length, void *stream);
int rz_mz_replay_poll_errors(rz_mz_replay *r, int32_t *flags, void *stream);
/* The value transform of the targets (ABI 43; csrc/rz_mz_value.h, csrc/rz_mz_target.h: unroll_row<VT>).  rz_mz_replay_set_value_transform(r, 1):
 * the launch that forms a mini-batch -- rz_mz_replay_gather, rz_mz_replay_sample, and the gather behind a prioritized draw -- writes
 * d_tv = float32(h(z)) and d_tr = float32(h(u)), z the fp64 n-step return exactly as formed without it and u the stored fp64
 * reward; rows past the episode's end stay 0, and nothing else of a batch changes (k_mzr_gather<true> / k_mzr_sample<true>; 0, the
 * default: the kernels of ABI 42).  The store keeps raw rewards and root values, and the priorities (k_mzr_prio) stay
 * |root value - n-step return| in raw units.  No launch; takes effect with the next one. */
int rz_mz_replay_set_value_transform(rz_mz_replay *r, int32_t on);

/* ---------------------------------------------------------------------------------------------------------------------
 * MuZero Reanalyse (ABI 36; rz_mz_replay.hip: k_mzr_positions, k_mzr_update; rz_mz_target.h; rlzero_amd/muzero/reanalyse.py):
 * the two device ends of searching stored steps again with the current network.  Between them the caller runs a search from
 * the observations handed out (rz_mz_init_roots + rz_mz_search or the step loop) and reads its roots (rz_mz_root_children,
 * rz_mz_root_stats).  No function or kernel above changes.
 *
 * rz_mz_replay_positions: n entries in ONE launch (k_mzr_positions: a thread per entry and observation element).  Entry i is
 *   resolved to a physical (slot, position), written to d_where int32 [n][2], and its stored observation goes to d_obs float32
 *   [n][D].  The entries come from h_draws int64 [n][2] (episode, 0 = the oldest held; position: checked here, RZ_ERR_ARG, and
 *   staged), from d_draws (device memory: checked by the kernel), or, both NULL, from the device's own draws of refresh `step`:
 *   counter c = 2 i + j gives mulhi64(x, m) of x = sm(sm(sm(seed ^ "mzreanal") ^ step) ^ c) -- j = 0 the episode, m = count;
 *   j = 1 the position, m = that episode's length (rlzero_amd/muzero/reanalyse.py: mz_reanalyse_draws gives the same bits; the
 *   salt keeps a refresh and a mini-batch of one update number apart).  seed and step are ignored when draws are given.  A device
 *   draw out of range: where = (-1, -1), the observation row zeroed, RZ_MZ_REPLAY_BAD_INDEX set, nothing read for it.
 *   *ticket receives the number of episodes EVER stored in this handle (host state, advanced by add / ingest), also for n = 0.
 * rz_mz_replay_update: ONE launch (k_mzr_update: a thread per entry and action, plus one per entry for the value).  For every
 *   entry whose where is valid -- 0 <= slot < E, 0 <= position < T and below the slot's length, checked in the kernel -- it writes
 *   policy[slot][position][a] = (float)((double)visits[a] / (double)sum(visits)) from d_visits int32 [n][A] (a sum of 0: the
 *   uniform policy (float)(1.0 / A)) and root_value[slot][position] = d_root_sum[i] / (double)max(d_root_n[i], 1) (d_root_n int32
 *   [n], d_root_sum float64 [n]: rz_mz_root_stats' N and value sum).  Nothing else is written; an entry with another where -- the
 *   (-1, -1) of a refused or a padding row -- writes nothing.  `ticket` must be what rz_mz_replay_positions returned and still be
 *   the handle's counter: an add or ingest in between may have given a slot to another episode, and the result of a search must
 *   never land there -- RZ_ERR_ARG, no launch.  Two entries that name the same step BOTH write it: the search is deterministic,
 *   so they carry the same bits and the order of the two writes does not matter. */
int rz_mz_replay_positions(rz_mz_replay *r, const int64_t *h_draws, const int64_t *d_draws, uint64_t seed, uint64_t step, int64_t n,
                           int32_t *d_where, float *d_obs, int64_t *ticket, void *stream);
int rz_mz_replay_update(rz_mz_replay *r, const int32_t *d_where, int64_t n, const int32_t *d_visits, const int32_t *d_root_n,
                        const double *d_root_sum, int64_t ticket, void *stream);

/* ---------------------------------------------------------------------------------------------------------------------
 * MuZero prioritized replay (ABI 37; rz_mz_replay.hip: k_mzr_prio, k_mzr_scan, k_mzr_draw_prio; rz_mz_target.h;
 * rlzero_amd/muzero/replay.py): arXiv:1911.08265v2 appendix G with alpha = 1.  Stored step t is drawn with probability
 * w_t / total, where w_t = priority_weight(|root_value[t] - value_target(t)|) is a FIXED-POINT integer: p * 2^16 truncated, at
 * least 1, 2^32 from p = 2^16 on, 1 for a NaN.  Integer sums are exact in any order, so the prefix sums a parallel scan forms
 * on the device are the bits of a host loop (replay.py: mz_priority_weights, mz_prioritized_draws).  Opt-in: until
 * rz_mz_replay_enable_priorities nothing of this is allocated or launched, and no function or kernel above changes.
 *
 * rz_mz_replay_enable_priorities: allocates cum uint64 [E][T] (the inclusive prefix of w inside each slot), mass uint64 [E],
 *   ecum uint64 [E] (the inclusive prefix of the masses over the episodes held, oldest first), the total and a dirty mark per
 *   slot, and marks every episode held.  RZ_ERR_ARG if E * T > 2^30 (the total stays below 2^62).  From then on add / ingest
 *   mark the slots they wrote and update marks the slots of its valid `where` rows (a changed root value moves the priority of
 *   its step and of the step td_steps before it, both in that slot), each with one small launch behind their own; the handle
 *   notes on the host that the prefixes are stale.  A second call does nothing.
 * rz_mz_replay_refresh_priorities: two launches on `stream`, no host synchronisation -- k_mzr_prio (a workgroup per episode
 *   held; a clean slot returns at once, a marked one gets its weights, its prefix by a wave scan with a carry over the waves
 *   and over chunks of 256 steps, its mass, and its mark cleared) and k_mzr_scan (one workgroup: ecum and the total).
 * rz_mz_replay_read_priorities: SYNCHRONOUS (tests, debugging): refreshes, then h_w int64 [n][T] receives the weights of episodes
 *   first .. first + n - 1 (oldest = 0) as differences of cum, 0 past an episode's end; *h_total (may be NULL) the total.
 * rz_mz_replay_draw_prioritized: refreshes on `stream` if anything was written since the last refresh, then ONE launch
 *   (k_mzr_draw_prio, a thread per entry).  Entry i takes ONE target g in 0 .. total - 1 -- d_targets[i] (int64 [n], device
 *   memory) or, d_targets NULL, mulhi64(x, total) of x = sm(sm(sm(seed ^ "mzpriori") ^ step) ^ c), c = i * (K + 2) -- and
 *   resolves it by two searches: j = the first episode with ecum[j] > g, then the first position of it with
 *   cum[position] > g - ecum[j - 1].  d_draws int64 [n][K + 2] receives (j, position, K filler actions: counters c + 2 + k,
 *   uniform over A; c + 1 is unused) in the layout rz_mz_replay_gather takes as d_draws, d_prob float64 [n] the step's
 *   probability (double)w / (double)total.  A target outside 0 .. total - 1 sets RZ_MZ_REPLAY_BAD_INDEX; that entry's row is
 *   all -1, which rz_mz_replay_gather refuses too, and its probability 0.  RZ_ERR_ARG on an empty buffer or while priorities
 *   are off. */
int rz_mz_replay_enable_priorities(rz_mz_replay *r, void *stream);
int rz_mz_replay_refresh_priorities(rz_mz_replay *r, void *stream);
int rz_mz_replay_read_priorities(rz_mz_replay *r, int64_t first, int64_t n, int64_t *h_w, int64_t *h_total, void *stream);
int rz_mz_replay_draw_prioritized(rz_mz_replay *r, uint64_t seed, uint64_t step, int64_t n, const int64_t *d_targets, int64_t *d_draws,
                                  double *d_prob, void *stream);

/* ---------------------------------------------------------------------------------------------
 * The fused MuZero learner (ABI 40; rz_mz_learn.hip: k_mzl_grad, k_mzl_reduce, k_mzl_adam; rz_mz_learn.h; an opt-in route beside
 * rlzero_amd/muzero/agent.py: MuZeroAgent.learn, whose arithmetic it restates in float32): forward through initial_inference
 * and K recurrent_inference steps, the three losses, backward through the unroll, clip_grad_norm_ and torch's single-tensor
 * Adam with weight decay in THREE launches on `stream`, no host synchronisation.  Hidden size 64 only, obs_dim <= 16,
 * n_actions <= 8, unroll_steps <= 16 (the device replay's limits).  Every reduction (weight gradients across workgroups, the
 * norm, the loss means) runs in a fixed order without floating-point atomics: the same inputs give the same bits.
 *
 * rz_mz_learner_bind: params void* [18] = the DEVICE storage of weight and bias of rep1 rep2 dyn1 dyn2 rew1 rew2 pre1 pol val
 *   (contiguous float32, row-major [out][in], 16-byte aligned), read and written where they lie; exp_avg / exp_avg_sq float32
 *   [n_params] flat in that order (rz_mz_learner_n_params), owned by the caller.
 * The batch: the six tensors of rz_mz_replay_gather -- d_obs float32 [n][D], d_actions int64 [n][K], d_tv / d_tr float32
 *   [n][K + 1], d_tp float32 [n][K + 1][A], d_mask float32 [n][K + 1] -- and d_weights float32 [n] or NULL (all ones);
 *   1 <= n <= max_batch.  An action outside 0 .. A-1 is read as 0, indexes nothing, and sets RZ_MZ_LEARNER_BAD_ACTION
 *   (rz_mz_learner_poll_errors; sticky until polled); while the flag stands rz_mz_learner_step updates nothing, and
 *   rz_mz_learner_poll_errors reports in *skipped how many updates were dropped (the caller takes them off its step count).
 * rz_mz_learner_grads: d_flat_grad float32 [n_params] = the raw gradient of the loss (before the clip), d_out4 float32 [4] =
 *   (loss, value, reward, policy) means; two launches, nothing is updated.
 * rz_mz_learner_step: the same, then the clip by max_norm and Adam step number `step_count` (1 = the first) on the bound
 *   parameters and moments; the bias corrections are formed on the host in double from step_count. */
enum { RZ_MZ_LEARNER_BAD_ACTION = 1 };
typedef struct rz_mz_learner_config {
    int32_t abi_version; /* RZ_ABI_VERSION */
    int32_t obs_dim, n_actions, hidden, unroll_steps, max_batch, device, reserved;
    double lr, weight_decay, beta1, beta2, eps, max_norm;
} rz_mz_learner_config;
typedef struct rz_mz_learner rz_mz_learner;
int rz_mz_learner_create(const rz_mz_learner_config *cfg, rz_mz_learner **out);
int rz_mz_learner_destroy(rz_mz_learner *l);
int rz_mz_learner_n_params(rz_mz_learner *l, int64_t *n_params);
int rz_mz_learner_bind(rz_mz_learner *l, void *const *d_params, float *d_exp_avg, float *d_exp_avg_sq);
int rz_mz_learner_grads(rz_mz_learner *l, const float *d_obs, const int64_t *d_actions, const float *d_tv, const float *d_tr, const float *d_tp,
                        const float *d_mask, const float *d_weights, int64_t n, float *d_flat_grad, float *d_out4, void *stream);
int rz_mz_learner_step(rz_mz_learner *l, const float *d_obs, const int64_t *d_actions, const float *d_tv, const float *d_tr, const float *d_tp,
                       const float *d_mask, const float *d_weights, int64_t n, int64_t step_count, float *d_out4, void *stream);
int rz_mz_learner_poll_errors(rz_mz_learner *l, int32_t *flags, int32_t *skipped, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RLZERO_HIP_H */
