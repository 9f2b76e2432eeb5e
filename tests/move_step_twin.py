"""Shared by the GPU tests of the device move step and by profiles/sharp_net_agreement.py (no test lives here): ``Twin``, an engine with
its evaluator attached to the move step on the device -- tests/test_policy_on_demand.py pairs one on demand with one that writes the
feature store --, and ``reachable``, every field of every node a caller can reach in a game's arena."""
import numpy as np

SEED = 13
B, N_ROW = 11, 5


class Twin(object):
    """An engine with its evaluator on the device move step; ``on_demand`` False: the switch off, every search writes the store.
    ``board``: its rows (``net`` is a net of that board); ``roots``: one position per slot -- ``roots_by_game``: per game id --, set
    behind the refill."""

    def __init__(self, on_demand, net, G, n_playout, graph=False, stall_margin=0.0, cap=None, queue_games=None, roots=None, board=B,
                 add_noise=True, c_puct=5.0, roots_by_game=False):
        import torch
        from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
        self.ev = HipNetEvaluator(net, board, 'cuda:0', max_boards=G)
        self.eng = MCTSEngine(board, N_ROW, n_games=G, n_playout=n_playout, c_puct=c_puct, device='cuda:0', add_noise=add_noise, noise_seed=3)
        assert self.eng.flush_kept
        self.eng.policy_on_demand = on_demand
        self.on_demand = on_demand
        n_q = G if queue_games is None else queue_games
        self.queue = torch.arange(n_q, dtype=torch.int64, device='cuda:0')
        self.ctl = torch.tensor([0, n_q], dtype=torch.int32, device='cuda:0')
        self.eng.play_attach(SEED, 1.0, self.queue, self.ctl, ring_steps=16, stall_margin=stall_margin)
        self.eng.play_refill()
        if cap is not None:
            self.eng.play_set_cap(*cap)
        if roots is not None:
            from rlzero_amd.engine import int_to_bits
            if roots_by_game:   # (which slot took which game is the refill's race, and twins are compared by game)
                roots = [roots[int(g)] for g in self.eng.play_state()[0]]
            stones = np.array([[int_to_bits(e.bitboards()[0]), int_to_bits(e.bitboards()[1])] for e in roots], dtype=np.uint64)
            self.eng.set_roots(stones, [e.current_player() for e in roots], [e.last_move for e in roots], reset_trees=True)
        self.route = self.eng._ask(self.ev)[0]
        assert self.route.resident and self.route.resident_delta
        self.graph = None
        if graph:
            self.warm()

    def warm(self):
        self.graph = self.eng.warm_move_graph(self.ev)
        assert self.graph is not None

    def search(self, n=None):
        self.eng.sim_chunk(self.ev, self.eng.n_playout if n is None else n, self.route)

    def move(self, search=True):
        import torch
        if self.graph is not None:
            row = self.eng.play_move_replay(self.graph)
        else:
            if search:
                self.search()
            row = self.eng.play_move()
        torch.cuda.synchronize()
        from rlzero_amd import playlog
        rows = self.eng.play_log[row].cpu().numpy().copy()
        # (an idle slot's row holds nothing to read; which slot stays idle is the refill's race)
        slots, d, _ = playlog.running(rows[None])
        self.slot_of = slots[np.argsort(d.game, kind='stable')]
        assert len(set(d.game.tolist())) == len(slots)
        return rows[self.slot_of]

    def modes(self):
        return dict(self.eng.search_launches)

    def close(self):
        st = self.eng.check()
        self.ev.hip.check_flags()
        assert st.reuse_dropped == 0
        # every resident search of this twin ran in its own mode
        assert self.eng.search_launches[not self.on_demand] == 0 and self.eng.search_launches[self.on_demand] > 0, self.eng.search_launches
        self.eng.close()
        self.ev.hip.close()


def reachable(eng, g):
    """Every field of every node reachable from the root of game g, in breadth-first order, with the priors of every expanded one;
    what lies above the arena tops, and child records beyond the visited ones, is old data."""
    a = eng.arena(g)
    out, slots, at = [('root_prior', np.float32(a['root_prior']).tobytes())], [0], 0
    while at < len(slots):
        s = slots[at]
        at += 1
        fc, nv, k, pb = int(a['FC'][s]), int(a['NV'][s]), int(a['K'][s]), int(a['PB'][s])
        assert s < a['top']
        pri = b''
        if k > 0:
            assert pb >= 0 and pb + k <= len(a['PRI'])
            pri = a['PRI'][pb:pb + k].tobytes()
            if nv > 0:
                slots.extend(range(fc, fc + nv))
        out.append((s, int(a['N'][s]), float(a['W'][s]).hex(), fc, nv, k, pb, pri))
    return out
