"""The kept flush (rz_deferred_keep, rz_net_deferred_gemm_rows, rz_deferred_flush_kept; MCTSEngine.flush_kept): between the draw and
the tree reuse of a move on the device only the priors the move keeps are written -- the kept child's subtree and the root's own
block.  Priors exist for every block a caller can reach; blocks of subtrees a move discards are never written.  The keep test never
misses a needed record (CPU, against the oracle's leaf paths), and twin engines -- one with the kept flush, one with the full flush --
leave the same log rows and, node by node, the same reachable trees and priors on every route a move on the device can take."""
import numpy as np
import pytest

from oracle.connect4_ref import RefConnect4
from oracle.gomoku_ref import RefGomoku
from oracle.mcts_ref import RefSearch

from move_step_twin import SEED, reachable as _reachable

WORDS = 4   # 64-bit words of a colour's bitboard (RZ_BOARD_WORDS)


# ----------------------------------------------------------------------------------------------- CPU: the keep test
def _words(x):
    return np.array([(x >> (64 * j)) & 0xFFFFFFFFFFFFFFFF for j in range(WORDS)], dtype=np.uint64)


def _board(env):
    b = env.bitboards()
    return np.stack([_words(b[0]), _words(b[1])])


def keep_needed(root, mover, keep_cell, leaf):
    """k_keep_mark's test on [2][WORDS] uint64 boards: ``keep_cell`` < 0 -- no move drawn -- keeps everything; else the root's own
    block (leaf board == root board) and every leaf with the mover's stone on the cell of the move."""
    if keep_cell < 0:
        return True
    if np.array_equal(leaf, root):
        return True
    return bool((leaf[mover][keep_cell >> 6] >> np.uint64(keep_cell & 63)) & np.uint64(1))


def _cell(env, action):
    if isinstance(env, RefConnect4):
        probe = env.clone()
        before = probe.bitboards()
        probe.step(action)
        after = probe.bitboards()
        return ((before[0] | before[1]) ^ (after[0] | after[1])).bit_length() - 1
    return int(action)


def _leaf(env, path):
    e = env.clone()
    for a in path:
        e.step(a)
    return _board(e)


def _value_fn(env):
    legal = env.leagel_actions()
    b = env.bitboards()
    v = ((b[0] * 0x9E3779B97F4A7C15 + b[1] * 0xC2B2AE3D27D4EB4F) >> 7) % 2001 / 1000.0 - 1.0   # deterministic, in [-1, 1]
    return [(a, 1.0 / len(legal)) for a in legal], v


@pytest.mark.parametrize('game', ['gomoku', 'connect4'])
def test_keep_test_never_misses(game):
    env = RefGomoku.from_moves(6, 4, [14, 15, 20]) if game == 'gomoku' else RefConnect4.from_moves([3, 3, 2], 6, 7, 4)
    search = RefSearch(_value_fn, 150 if game == 'gomoku' else 400, 5)
    extra = transposed = 0
    for ply in range(4):
        search.leaf_log = []
        search.simulate(env, 1.0)
        paths = [p for p, _ in search.leaf_log]
        visits = sorted(((kid.n, a) for a, kid in zip(search.root.acts, search.root.kids) if kid.n > 0), reverse=True)
        root, mover = _board(env), env.current_player()
        for _, mv in visits[:3]:   # the three most visited children as the drawn move
            cell = _cell(env, mv)
            for path in paths:
                kept = keep_needed(root, mover, cell, _leaf(env, path))
                if len(path) == 0 or path[0] == mv:
                    assert kept, (ply, mv, path)   # a miss would be a wrong prior
                elif kept:   # a row too many: the same stones by another order (the mover's later move lands on the cell)
                    assert any(_cell_at(env, path, i) == cell for i in range(2, len(path), 2)), (ply, mv, path)
                    extra += 1
            assert all(keep_needed(root, mover, -2, _leaf(env, path)) for path in paths[:5])   # no move drawn: everything
        # a hand-made transposition (a, b, mv) -- the mover's a, the opponent's b, then the move (other columns in Connect4, so that
        # the move lands on the same cell): its leaf has the mover's stone on the cell -- kept, a row too many and harmless
        mv = visits[0][1]
        others = [x for x in env.leagel_actions() if x != mv]
        assert keep_needed(root, mover, _cell(env, mv), _leaf(env, (others[0], others[-1], mv)))
        transposed += 1
        env.step(mv)
        search.update_with_move(mv)
    assert transposed == 4


def _cell_at(env, path, i):
    e = env.clone()
    for a in path[:i]:
        e.step(a)
    return _cell(e, path[i])


# ----------------------------------------------------------------------------------------------- GPU: twin engines
def _net(game, shape):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    torch.manual_seed(4)
    if game == 'connect4':
        return PolicyValueNet(6, 7, 7).to('cuda:0'), (6, 7, 7)
    return PolicyValueNet(shape).to('cuda:0'), shape


class _Twin(object):
    """An engine with its evaluator, attached to the move step on the device with games 0 .. n_games - 1 in its slots."""

    def __init__(self, kept, game, shape, n_row, n_games, n_playout, net, net_shape, graph=False, stall_margin=0.0, cap=None, resident=True):
        import torch
        from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
        self.ev = HipNetEvaluator(net, net_shape, 'cuda:0', max_boards=n_games)
        self.ev.resident_search = resident   # (False: the two-launch step of the lanes that share CUs)
        self.eng = MCTSEngine(shape, n_row, n_games=n_games, n_playout=n_playout, device='cuda:0', game=game, add_noise=True, noise_seed=3)
        self.eng.flush_kept = kept
        self.queue = torch.arange(n_games, dtype=torch.int64, device='cuda:0')
        self.ctl = torch.tensor([0, n_games], dtype=torch.int32, device='cuda:0')
        self.eng.play_attach(SEED, 1.0, self.queue, self.ctl, ring_steps=16, stall_margin=stall_margin)
        self.eng.play_refill()
        if cap is not None:
            self.eng.play_set_cap(*cap)
        self.route = self.eng._ask(self.ev)[0]
        self.graph = self.eng.warm_move_graph(self.ev) if graph else None
        assert (self.graph is not None) == graph

    def search(self):
        self.eng.sim_chunk(self.ev, self.eng.n_playout, self.route)

    def move(self, search=True):
        import torch
        if self.graph is not None:
            row = self.eng.play_move_replay(self.graph)
        else:
            if search:
                self.search()
            row = self.eng.play_move()
        torch.cuda.synchronize()
        rows = self.eng.play_log[row].cpu().numpy().copy()
        # which slot took which game from the queue is a race of the refill's workgroups: everything is compared by game id
        gid = (rows[:, 0].astype(np.int64) & 0xFFFFFFFF) | (rows[:, 1].astype(np.int64) << 32)
        self.slot_of = np.argsort(gid, kind='stable')
        assert sorted(gid.tolist()) == list(range(len(gid)))
        return rows[self.slot_of]

    def close(self):
        st = self.eng.check()
        self.ev.hip.check_flags()
        assert st.reuse_dropped == 0
        self.eng.close()
        self.ev.hip.close()


def _same_trees(a, b, n_games, what):
    for g in range(n_games):   # (game ids: _Twin.move)
        assert _reachable(a.eng, int(a.slot_of[g])) == _reachable(b.eng, int(b.slot_of[g])), (what, g)


def _same_rows(rows, what):
    where = np.argwhere(rows[0] != rows[1])
    assert where.size == 0, (what, [(g, w, int(rows[0][g, w]), int(rows[1][g, w])) for g, w in where[:8].tolist()])


def _pair(*args, **kw):
    return _Twin(True, *args, **kw), _Twin(False, *args, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [False, True], ids=['play_move', 'move_graph'])
def test_trees_equal_on_the_receptive_field_route(graph):
    """11 x 11, 48 simulations: fewer than the legal moves, so every leaf is at depth 1 and a move keeps exactly one expansion per
    game -- and the root's own block at ply 0."""
    G, moves = 6, 6
    net, net_shape = _net('gomoku', 11)
    kept, full = _pair('gomoku', 11, 5, G, 48, net, net_shape, graph=graph)
    assert kept.route.resident_delta and full.route.resident_delta
    kept.eng.flush_kept_stats(reset=True)
    for ply in range(moves):
        rows = kept.move(), full.move()
        _same_rows(rows, ply)
        assert (rows[0][:, 3] >= 0).all()   # (no stall, no end)
        _same_trees(kept, full, G, ply)
        got = kept.eng.flush_kept_stats(reset=True)
        # ply 0: the root and 47 children are expanded; later the root is the kept child, expanded already
        assert got == (G * (2 if ply == 0 else 1), G * 48), (ply, got)
    assert full.eng.flush_kept_stats() == (0, 0)
    kept.close()
    full.close()


def _expanded_paths(eng, g):
    """The action paths of the expanded nodes of game g's tree."""
    from rlzero_amd.engine import bits_to_int
    a = eng.arena(g)
    stones, _, _ = eng.get_roots()
    out, stack = set(), [((), 0, bits_to_int(stones[g, 0]) | bits_to_int(stones[g, 1]))]
    while stack:
        path, s, occ = stack.pop()
        if int(a['K'][s]) == 0:
            continue
        out.add(path)
        legal = eng.legal_actions(occ)
        for r in range(int(a['NV'][s])):
            stack.append((path + (legal[r], ), int(a['FC'][s]) + r, occ | (1 << eng.cell_of_action(occ, legal[r]))))
    return out


@pytest.mark.gpu
def test_deeper_trees():
    """200 simulations on 121 cells: leaves at depth 2 and, from the second move, reused subtrees.  The kept flush writes at least the
    expansions below the chosen child (counted on the full-flush twin's arenas) and at most all of them."""
    G, moves = 6, 3
    net, net_shape = _net('gomoku', 11)
    kept, full = _pair('gomoku', 11, 5, G, 200, net, net_shape)
    kept.eng.flush_kept_stats(reset=True)
    for ply in range(moves):
        before = [_expanded_paths(full.eng, g) for g in range(G)]
        full.search()
        after = [_expanded_paths(full.eng, g) for g in range(G)]   # (reads the arena: the full twin's priors are written here)
        rows = kept.move(), full.move(search=False)
        _same_rows(rows, ply)
        _same_trees(kept, full, G, ply)
        exact = 0
        for g in range(G):
            mv, slot = int(rows[1][g, 3]), int(full.slot_of[g])
            assert mv >= 0
            new = after[slot] - before[slot]
            exact += sum(1 for p in new if len(p) == 0 or p[0] == mv)
        got, pending = kept.eng.flush_kept_stats(reset=True)
        assert pending == sum(len(after[g] - before[g]) for g in range(G)), ply
        assert exact <= got <= pending, (ply, exact, got, pending)
    kept.close()
    full.close()


@pytest.mark.gpu
def test_every_slot_stalls():
    """The largest stall_margin rz_play_attach takes (it refuses 0.5 and more: a uniform is never farther than half its interval from
    both edges, so the last double below 0.5 already lets no draw through): every slot stalls and keeps its whole tree -- every record
    is listed, more rows (48 x 200 = 9600) than one round of the GEMM's and the priors' fixed grids holds -- then the host's moves
    are applied."""
    G, n = 48, 200
    net, net_shape = _net('gomoku', 11)
    kept, full = _pair('gomoku', 11, 5, G, n, net, net_shape, stall_margin=float(np.nextafter(0.5, 0.0)))
    kept.eng.flush_kept_stats(reset=True)
    rows = kept.move(), full.move()
    _same_rows(rows, 'stall')
    assert (rows[0][:, 3] == -1).all()
    got, pending = kept.eng.flush_kept_stats(reset=True)
    assert got == pending == G * n, (got, pending)
    _same_trees(kept, full, G, 'stalled')
    visits = rows[0][:, 8:]
    for g in range(G):
        mv = int(np.argmax(visits[g]))
        kept.eng.play_resolve(int(kept.slot_of[g]), mv)
        full.eng.play_resolve(int(full.slot_of[g]), mv)
    rows = kept.move(), full.move()
    _same_rows(rows, 'stall')
    assert (rows[0][:, 3] >= 0).all()
    assert kept.eng.flush_kept_stats() == (0, 0)   # (a stalled slot is not searched)
    _same_trees(kept, full, G, 'resolved')
    kept.close()
    full.close()


@pytest.mark.gpu
@pytest.mark.parametrize('graph', [False, True], ids=['play_move', 'move_graph'])
def test_playout_cap(graph):
    G = 8
    net, net_shape = _net('gomoku', 11)
    kept, full = _pair('gomoku', 11, 5, G, 160, net, net_shape, graph=graph, cap=(20, 0.5))
    budgets = set()
    for ply in range(3):
        counts = kept.eng.playouts()[0]
        budgets.update(int(c) for c in counts)
        rows = kept.move(), full.move()
        _same_rows(rows, ply)
        _same_trees(kept, full, G, ply)
    assert budgets == {20, 160}
    kept.close()
    full.close()


@pytest.mark.gpu
@pytest.mark.parametrize('case', ['compact_resident_6x6', 'two_launch_9x9', 'connect4'])
def test_the_other_routes(case):
    game, shape, n_row, G, n, graph = {'compact_resident_6x6': ('gomoku', 6, 4, 4, 32, True), 'two_launch_9x9': ('gomoku', 9, 5, 4, 32, False),
                                       'connect4': ('connect4', (6, 7), 4, 4, 60, True)}[case]
    net, net_shape = _net(game, shape)
    kept, full = _pair(game, shape, n_row, G, n, net, net_shape, graph=graph, resident=graph)
    assert kept.route.deferred
    assert kept.route.compact_resident == graph and kept.route.resident == graph
    kept.eng.flush_kept_stats(reset=True)
    for ply in range(4):
        rows = kept.move(), full.move()
        _same_rows(rows, ply)
        _same_trees(kept, full, G, ply)
    got, pending = kept.eng.flush_kept_stats()
    assert 0 < got < pending
    kept.close()
    full.close()
