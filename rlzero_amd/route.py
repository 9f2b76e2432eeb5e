"""Which kernels evaluate a leaf -- "the route" -- decided in ONE place on this side of the C ABI, on plain values (no torch, no library):
HipNet, HipNetEvaluator, MCTSEngine and BatchedSelfPlay.for_network ask ``decide()`` and restate nothing of it.

The library decides the same once more for the net it holds: ``rows_kernel_covers`` / ``split_trunk_ok`` / ``delta_covers`` /
``compact_grid_covers`` / ``trunk_class`` in csrc/rz_net.hip.  THAT is the one other place that must agree with this module; its
RZ_ERR_ARG returns (rz_net_trunk_leaves*, rz_net_search_resident, rz_net_search_resident_puct, rz_net_delta_*, rz_net_set_algo) are the
backstop when they do not.
"""
import os
from collections import namedtuple

from ._hip import SCORE_PUCT, SCORE_UCT_REF   # (constants only: importing _hip loads nothing)

# the algorithm classes (HipNet.set_algo names)
SPLIT_TRUNKS = ('split_f16', 'split_f16_tiles', 'split_f16_fp8')   # the split-f16 trunks: fed positions, deferred priors
EVERY_BOARD_SPLIT_TRUNKS = ('split_f16', 'split_f16_tiles')        # ... of every board size ('split_f16_fp8': the rows kernel's only)
DELTA_TRUNKS = ('split_f16', )                                     # ... with the receptive-field trunk (k_trunk_delta / k_delta_res)
RESIDENT_TRUNKS = ('split_f16', 'split_f16_fp8')                   # ... with the one-launch resident search


def rows_kernel_board(rows, cols):
    """k_trunk_rows' boards, one N-tile per row (rz_net.hip: rows_kernel_covers)."""
    return 11 <= rows <= 16 and 11 <= cols <= 16


def tile_resident_board(rows, cols):
    """The boards k_trunk_split<.., RES> searches resident: one N-tile per wave at most."""
    return rows <= 10 and cols <= 10


def compact_grid_board(rows, cols, environ=None):
    """The boards k_trunk_split has a compact LDS grid for (rz_net.hip: compact_grid_covers): N-tiles of min(32 // cols, 16) rows,
    at most two of them, at most 7 columns, tile rows + the halo inside 15 grid rows.  RZ_NET_COMPACT=0 switches the grid off."""
    if cols > 7 or cols < 1:
        return False
    tile_rows = min(32 // cols, 16)
    tiles = (rows + tile_rows - 1) // tile_rows
    return tiles <= 2 and tiles * tile_rows + 2 <= 15 and _on(environ, 'RZ_NET_COMPACT')


def _on(environ, name):   # (read at every call and behind every other condition: a look into os.environ costs more than the rest of decide())
    return (os.environ if environ is None else environ).get(name, '1') != '0'


def fc_in_trunk_pays(rows, cols, n_actions):
    """True when the trunk's workgroups should run the first FC layers on their own boards (HipNet.set_heads_algo('in_trunk'))
    instead of a GEMM launch of its own: boards of up to 10 rows whose FC weights (hi + lo f16) are at most 40 KB -- every workgroup
    streams them for its one board (6x6: 39 KB, TicTacToe +6 %; Connect4: 26 KB, 512 games on two lanes +3 %; 9x9: 146 KB, -5 to
    -11 %: profiles/r03/in_trunk_fc.txt).  rz_net.hip's launch_trunk holds the same condition (``fc_here``) and must agree."""
    cells = rows * cols
    return rows <= 10 and (n_actions * 4 * cells + 64 * 2 * cells) * 4 <= 40 * 1024


def policy_on_demand(route, move_step=False, flush_kept=True, match=False, allowed=True):
    """Whether the NEXT resident search of an engine runs without policy features (rz_net_search_resident_values: the value planes per
    leaf, the policy planes formed at the flush for the records it lists -- rz_net_policy_rows).  It pays where flushes are kept flushes:
    ``route`` (a Route) runs k_delta_res, the engine has the device move step attached (``move_step``), its moves flush what they keep
    (``flush_kept``), it plays no match (``match``: two evaluators a move, every change a full flush), and the engine's switch
    (``allowed``: MCTSEngine.policy_on_demand, from RZ_POLICY_ON_DEMAND, '0' = off) allows it.  Everything else keeps writing the store.
    The library refuses the call where k_delta_res does not run (RZ_ERR_ARG), whatever this says."""
    return bool(route.resident and route.resident_delta and move_step and flush_kept and not match and allowed)


def pend_lw_pack(to_move, last):
    """The word a pending record carries beside its stones (rz_tree.h: pend_lw_pack): the leaf's last move + 1 (0: none) in the low half,
    its side to move above."""
    return ((int(last) + 1) & 0xffff) | (int(to_move) << 16)


def pend_lw_unpack(word):
    """-> (side to move, last move or -1)."""
    return (int(word) >> 16) & 1, (int(word) & 0xffff) - 1


Route = namedtuple('Route', 'needs_planes deferred delta delta_three_launch resident resident_delta compact_resident resident_per_cu')
Route.__doc__ = """How the leaves of a search are evaluated:
needs_planes        the trunk reads float observation planes (otherwise the engine's leaf bitboards: no plane is written)
deferred            trunk -> tree step, the policy half in one batch later (otherwise trunk -> FC GEMM -> tree step)
delta               the receptive-field trunk against cached bases of the root is usable
delta_three_launch  ... and the three-launch step runs on it
resident            a whole search is ONE launch, one workgroup per game
resident_delta      the resident search could run the receptive-field trunk (k_delta_res): two games per CU
compact_resident    the net's resident search runs on the compact LDS grid: two games per CU
resident_per_cu     resident workgroups a CU holds (2: a launch takes any number of games, in rounds beyond 2 x CUs)"""


def decide(rows, cols, algo='split_f16', split_ok=True, heads_algo='auto', use_positions=True, deferred_priors=True, delta_trunk=True,
           resident_search=True, score_mode=SCORE_UCT_REF, in_flight=1, n_games=0, n_cus=0, same_board=True, environ=None, resident_puct=False):
    """-> Route.  ``rows`` / ``cols`` / ``algo`` / ``split_ok`` (rz_net_load found finite activation bounds) / ``heads_algo``: the net;
    ``use_positions`` and the three switches: the evaluator; ``score_mode`` / ``in_flight`` / ``n_games`` / ``same_board`` (its board is
    the net's): the engine; ``n_cus``: the chip.  ``environ``: RZ_NET_DELTA, RZ_NET_DELTA_RESIDENT, RZ_NET_COMPACT ('0' = off) are read
    from it at every call -- None: os.environ; {}: what the kernels can do, whatever the environment says.
    ``resident_puct`` (the evaluator's opt-in switch, HipNetEvaluator.resident_puct; off: every Route is what it was without it): the
    resident search under PUCT (rz_net_search_resident_puct, whose refusals in csrc/rz_net.hip state this rule once more) --
    ``resident`` is then also true when resident_puct_refusal() finds nothing: the split-f16 trunk fed positions, one simulation in
    flight, PUCT, a board of up to 10 x 10 that is the net's, any FC arithmetic but 'f32', the resident switch on, at most one game
    per CU.  ``resident_per_cu`` is 1 there and ``deferred`` stays false: nothing of such a search waits for a flush."""
    split = split_ok and algo in SPLIT_TRUNKS
    one_sim = in_flight == 1
    deferred = bool(split and deferred_priors and use_positions and one_sim and score_mode in (SCORE_UCT_REF, 'uct_ref'))
    rows_board = rows_kernel_board(rows, cols)
    delta = bool(split and delta_trunk and same_board and rows_board and algo in DELTA_TRUNKS and _on(environ, 'RZ_NET_DELTA'))
    resident_delta = delta and _on(environ, 'RZ_NET_DELTA_RESIDENT')
    net_resident = split and algo in RESIDENT_TRUNKS and (rows_board or tile_resident_board(rows, cols))
    compact = net_resident and not rows_board and compact_grid_board(rows, cols, environ)
    per_cu = 2 if (resident_delta or (compact and same_board)) else 1
    if resident_puct and resident_puct_refusal(rows, cols, algo, split_ok, heads_algo, use_positions, resident_search, score_mode, in_flight,
                                               n_games, n_cus, same_board) is None:
        return Route(False, False, False, False, True, False, False, 1)   # (no receptive-field trunk up to 10 rows; the 18 x 18 grid)
    return Route(not (use_positions and split), deferred, delta, bool(delta and use_positions and one_sim and not deferred and heads_algo != 'f32'),
                 bool(resident_search and deferred and net_resident and (per_cu >= 2 or n_games <= n_cus)), resident_delta, compact, per_cu)


def resident_puct_refusal(rows, cols, algo='split_f16', split_ok=True, heads_algo='auto', use_positions=True, resident_search=True,
                          score_mode=SCORE_PUCT, in_flight=1, n_games=0, n_cus=0, same_board=True):
    """Why the resident search under PUCT (rz_net_search_resident_puct) cannot serve these numbers -> a sentence, or None when it can.
    THE rule of that route on this side of the ABI (decide(resident_puct=True) asks here); rz_net.hip's refusals are the other copy."""
    if score_mode not in (SCORE_PUCT, 'puct'):
        return 'score_mode %r: the resident PUCT search is for score_mode \'puct\' (uct_ref has the resident search of the deferred route)' % (score_mode, )
    if in_flight != 1:
        return 'sims_in_flight %d: the resident search runs one simulation in flight per tree' % in_flight
    if not (split_ok and algo in SPLIT_TRUNKS):
        return 'net_algo %r: the resident search needs the split-f16 trunk (a net with finite activation bounds)' % (algo, )
    if not use_positions:
        return 'the resident search is fed positions (use_positions)'
    if not tile_resident_board(rows, cols):
        return 'a board of %d x %d: the resident PUCT search exists for boards of up to 10 rows and columns' % (rows, cols)
    if not same_board:
        return 'engine and network disagree on the board'
    if heads_algo == 'f32':
        return 'heads_algo \'f32\': the resident PUCT search runs the FC layers on the f16 pipe'
    if not resident_search:
        return 'the resident search is switched off (resident_search)'
    if n_games > n_cus:
        return '%d games on %d CUs: the resident PUCT search holds one game per CU' % (n_games, n_cus)
    return None
