"""How far is the device from the reference's own runs on boards of 11, 15 and 16 rows when the values MATTER?

tests/golden/g9_* (tests/golden/gen_golden.py g9; loaders: tests/sharp_fixture.py) hold, on oracle.evaluators.sharp_weights, the
reference's net outputs on 24 positions per board, searches of the reference's AlphaZeroMCTS with its own torch-CPU evaluator (every
simulation's leaf and value, the tree) and self-play games, with the tolerances E = 4 x max |torch f32 - torch f64| measured there.
The functions below run the same work on the GPU and return the largest difference each route shows; tests/test_sharp_net_rows.py
and tests/test_policy_on_demand_sharp.py assert them against E, and the report lists them:

    python profiles/sharp_net_agreement.py > profiles/sharp_net/agreement.txt      (on an MI355X)
"""
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (REPO, os.path.join(REPO, 'tests'), os.path.join(REPO, 'profiles')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import sharp_fixture as sf   # noqa: E402

FORWARD_ROUTES = ('split_f16', 'direct', 'split_f16_tiles')


# ---------------------------------------------------------------------------------------------------------------- plumbing
def boards_of(move_lists):
    """Move lists (colours alternating from player 0) -> bitboards uint64 [n][2][4], side to move, last cell."""
    n = len(move_lists)
    stones = np.zeros((n, 2, 4), dtype=np.uint64)
    for i, moves in enumerate(move_lists):
        for j, c in enumerate(moves):
            stones[i, j % 2, c >> 6] |= np.uint64(1) << np.uint64(c & 63)
    to_move = np.array([len(m) % 2 for m in move_lists], dtype=np.int32)
    last = np.array([m[-1] if m else -1 for m in move_lists], dtype=np.int32)
    return stones, to_move, last


def hip_net(B, max_boards):
    """HipNet on the board's sharp weights; the default route must be the split-f16 one (finite activation bounds)."""
    from rlzero_amd.engine import HipNet
    hip = HipNet(B, 'cuda:0', max_boards=max_boards).load_state_dict(sf.weights(B))
    assert hip.range_info()['split_ok'], hip.range_info()
    return hip


def module_of(B):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    net = PolicyValueNet(B)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sf.weights(B).items()})
    return net


_hiprt = None


def _from_device(ptr, count, dtype=np.float32):
    """``count`` values at a device address the library handed out -> numpy (synchronous copy)."""
    global _hiprt
    if _hiprt is None:
        _hiprt = ctypes.CDLL('libamdhip64.so')
    out = np.empty(count, dtype=dtype)
    assert _hiprt.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(out.nbytes), 2) == 0
    return out


def heads_of_delta(hip, roots, leaves, without_base=False):
    """rz_net_delta_leaves on ``leaves`` (move lists) against bases of ``roots`` -> (log_probs [n,S], value [n]) as float64: the log-softmax
    of the policy GEMM's logits (rz_net_deferred_gemm on the stored features) and the value layers on the value rows the kernel left,
    both finished here in float64 from the DEVICE's arrays (val_fc1 as the loader packed it) -- what the tree kernels finish in f32."""
    import torch
    from rlzero_amd.engine import _ptr
    n, S = len(leaves), hip.n_cells
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a.view(np.int64) if a.dtype == np.uint64 else a)).to('cuda:0')   # noqa: E731
    r_st, r_tm, _ = boards_of(roots)
    l_st, l_tm, l_last = boards_of(leaves)
    keep = [dev(a) for a in (r_st, r_tm, l_st, l_tm, l_last)]
    hip.reserve(n)
    hip.delta_reserve(n)
    hip.deferred_reserve(n, 1)
    hip.delta_bases(_ptr(keep[0]), _ptr(keep[1]), n)
    slot = torch.zeros(n, dtype=torch.int32, device='cuda:0')
    head = hip.delta_leaves(_ptr(keep[2]), _ptr(keep[3]), _ptr(keep[4]), n, slot_of=_ptr(slot), without_base=without_base)
    torch.cuda.synchronize()
    ld, groups = int(head.ld), int(head.groups)
    rows = _from_device(head.valfeat, n * ld).reshape(n, ld).astype(np.float64)
    w1t = _from_device(head.w1t, groups * 64 * 4).reshape(groups, 64, 4).astype(np.float64)
    b1, w2, b2 = (_from_device(p, k).astype(np.float64) for p, k in ((head.b1, 64), (head.w2, 64), (head.b2, 1)))
    assert not rows[:, 2 * S:].any()
    hidden = np.maximum(np.einsum('ngj,ghj->nh', rows.reshape(n, groups, 4), w1t) + b1, 0.0)
    value = np.tanh(hidden @ w2 + b2[0])
    logits = hip.deferred_gemm(n, 1)
    torch.cuda.synchronize()
    raw = _from_device(logits.raw, int(logits.rows_per_slot) * int(logits.ld)).reshape(-1, int(logits.ld))[:n, :S].astype(np.float64)
    raw -= raw.max(axis=1, keepdims=True)
    return raw - np.log(np.exp(raw).sum(axis=1, keepdims=True)), value


# ---------------------------------------------------------------------------------------------------------------- a. the net
def forward_errors(B):
    """-> {route: (max |value - reference's|, max |log_probs - reference's|)} on the 24 recorded positions: HipNet.forward with each
    conv algorithm, then the receptive-field kernel against bases 1 / 2 / 3 stones back and without a base."""
    import torch
    pos = sf.net(B)
    hip = hip_net(B, 32)
    out = {}
    planes = torch.from_numpy(pos['planes']).to('cuda:0')
    for algo in FORWARD_ROUTES:
        hip.set_algo(algo)
        logp, value = hip.forward(planes)
        out['forward ' + algo] = (float(np.max(np.abs(value.cpu().numpy().astype(np.float64) - pos['value']))),
                                  float(np.max(np.abs(logp.cpu().numpy().astype(np.float64) - pos['log_probs']))))
    hip.set_algo('split_f16')
    assert hip.supports_delta()
    for back, without_base in ((1, False), (2, False), (3, False), (1, True)):
        roots = [m[:max(0, len(m) - back)] for m in pos['moves']]
        hip.delta_stats(reset=True)
        logp, value = heads_of_delta(hip, roots, pos['moves'], without_base)
        st = hip.delta_stats()
        assert st['delta'] + st['no_base'] == 24 and (st['no_base'] == 24 if without_base else st['delta'] >= 20), st
        out['delta without a base' if without_base else 'delta %d back' % back] = (
            float(np.max(np.abs(value - pos['value']))), float(np.max(np.abs(logp - pos['log_probs']))))
    hip.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- c. the leaves
def leaf_errors(B):
    """Every non-terminal leaf the reference evaluated, through rz_net_delta_leaves against a base of its search's root ->
    [(case name, max |value - reference's|, leaves against the base, leaves without one)]."""
    head = sf.search(B)
    hip = hip_net(B, max(c['n_playout'] for c in head['cases']))
    out = []
    for rec in head['cases']:
        terminal = set(rec['terminal'])
        keep = [i for i in range(len(rec['leaves'])) if i not in terminal]
        leaves = [rec['pre'] + rec['leaves'][i][0] for i in keep]
        want = np.array([float.fromhex(rec['leaves'][i][1]) for i in keep])
        hip.delta_stats(reset=True)
        _, value = heads_of_delta(hip, [rec['pre']] * len(leaves), leaves)
        st = hip.delta_stats()
        assert st['delta'] + st['no_base'] == len(leaves), st
        out.append((rec['name'], float(np.max(np.abs(value - want))), st['delta'], st['no_base']))
    hip.close()
    return out


# ---------------------------------------------------------------------------------------------------------------- d. the searches
def search_on_device(B, cases, resident, on_demand=None, copies=1):
    """All ``cases`` of a board as the games of one engine, searched by the device with its own values ->
    (trees [{path: (N, W)}], root visit vectors, delta counters, the route).  ``on_demand`` True / False: the engine has the device
    move step attached and its switch set so (search_attached: one sim_chunk without / with policy features in the store), with
    ``copies`` of every case (case k in slots k, k + n, ..: trees and visit vectors of every slot)."""
    from oracle.gomoku_ref import RefGomoku
    if on_demand is not None:
        assert resident, 'policy on demand is the resident search\'s'
        r = search_attached(B, cases, on_demand, copies)
        return r['trees'], r['visits'], r['stats'], r['route']
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine, int_to_bits
    sims = cases[0]['n_playout']
    envs = [RefGomoku.from_moves(B, c['n'], c['pre']) for c in cases]
    evaluator = HipNetEvaluator(module_of(B), B, 'cuda:0', max_boards=len(envs))
    assert evaluator.hip.range_info()['split_ok']
    evaluator.resident_search = resident
    eng = MCTSEngine(B, 5, n_games=len(envs), n_playout=sims, c_puct=cases[0]['c_puct'], device='cuda:0')
    route = evaluator.route(eng)
    stones = np.array([[int_to_bits(e.bitboards()[0]), int_to_bits(e.bitboards()[1])] for e in envs], dtype=np.uint64)
    eng.set_roots(stones, [e.current_player() for e in envs], [e.last_move for e in envs], reset_trees=True)
    evaluator.hip.delta_stats(reset=True)
    eng.simulate(evaluator, sims, use_graph=False)
    stats = evaluator.hip.delta_stats()
    visits = eng.root_visits().copy()
    trees = [eng.tree_dump(g) for g in range(len(envs))]
    eng.check()
    eng.close()
    evaluator.hip.close()
    return trees, visits, stats, route


def tree_difference(tree, rec):
    """-> (nodes whose N differs from the reference's dump (or that only one side has), max |W - W_ref| / N over the others)."""
    want = {tuple(p): (n, float.fromhex(w)) for p, n, w in rec['tree']}
    bad, worst = 0, 0.0
    for path in set(want) | set(tree):
        if path not in want or path not in tree or tree[path][0] != want[path][0]:
            bad += 1
        elif want[path][0] > 0:
            worst = max(worst, abs(tree[path][1] - want[path][1]) / want[path][0])
    return bad, worst


# ---------------------------------------------------------------------------------------------------------------- f. policy on demand
COPIES = 7   # of every case in one engine: game indices beyond 32, the second 32-board tile of the feature store


def expanded_leaves(rec):
    """The paths of a case's non-terminal leaves: the nodes its search expands, each once."""
    terminal = set(rec['terminal'])
    return [tuple(p) for i, (p, _) in enumerate(rec['leaves']) if i not in terminal]


def leaf_planes(B, rec, paths):
    """float32 [n, 4, B, B]: the observation planes of ``rec``'s root with each of ``paths`` played on it."""
    from oracle.gomoku_ref import RefGomoku
    root = RefGomoku.from_moves(B, rec['n'], rec['pre'])
    out = np.empty((len(paths), 4, B, B), dtype=np.float32)
    for i, path in enumerate(paths):
        env = root.clone()
        for m in path:
            env.step(m)
        out[i] = env.current_state()
    return out


def logp64_rows(B, rec, paths):
    """oracle.evaluators.net_forward in float64 on the CPU, one batch -> log-probabilities float64 [n, S]."""
    import torch
    from oracle.evaluators import net_forward
    with torch.no_grad():
        return net_forward(sf.weights(B), leaf_planes(B, rec, paths), torch.float64)[0].numpy()


_logp64 = {}


def logp64_of(B, rec):
    """{path: float64 log-probabilities [S]} of every node the case's search expands; computed once per case and left unchanged."""
    key = (B, rec['name'])
    if key not in _logp64:
        paths = expanded_leaves(rec)
        rows = logp64_rows(B, rec, paths)
        rows.setflags(write=False)
        _logp64[key] = dict(zip(paths, rows))
    return _logp64[key]


def expanded_blocks(eng, slot):
    """{path: (legal cells ascending, the node's prior block PRI[PB : PB + K] float32)} over the expanded nodes reachable from the
    root of ``slot`` (reads the arena: whatever is pending is flushed)."""
    from rlzero_amd.engine import bits_to_int
    a = eng.arena(slot)
    stones, _, _ = eng.get_roots()
    out, stack = {}, [((), 0, bits_to_int(stones[slot, 0]) | bits_to_int(stones[slot, 1]))]
    while stack:
        path, s, occ = stack.pop()
        k, pb = int(a['K'][s]), int(a['PB'][s])
        if k == 0:
            continue
        assert 0 <= pb and pb + k <= len(a['PRI']), (slot, path, k, pb)
        legal = eng.legal_actions(occ)
        out[path] = (legal, a['PRI'][pb:pb + k].copy())
        assert int(a['NV'][s]) <= len(legal), (slot, path, int(a['NV'][s]), len(legal))
        for r in range(int(a['NV'][s])):
            stack.append((path + (legal[r], ), int(a['FC'][s]) + r, occ | (1 << legal[r])))
    return out


def block_errors(blocks, ref, prefix=()):
    """-> (max |log(float64(prior)) - ref[prefix + path][cell]| over every block of ``blocks`` and legal cell -- inf for a prior that
    is zero, negative or not a number --, blocks whose K is not the number of legal moves)."""
    worst, wrong_k = 0.0, 0
    for path, (legal, pri) in blocks.items():
        if len(pri) != len(legal):
            wrong_k += 1
            continue
        with np.errstate(divide='ignore', invalid='ignore'):
            err = np.abs(np.log(pri.astype(np.float64)) - ref[tuple(prefix) + path][legal])
        worst = max(worst, float(np.max(np.where(np.isfinite(err), err, np.inf))))
    return worst, wrong_k


def attached_twin(B, cases, on_demand, copies=1, graph=False):
    """tests/move_step_twin.py's Twin (evaluator + engine on the device move step, slots refilled) on the board's sharp weights:
    case k at the root of slots k, k + n, ..; no noise, the cases' c_puct and simulation count."""
    from oracle.gomoku_ref import RefGomoku
    from move_step_twin import Twin
    sims, c_puct = cases[0]['n_playout'], cases[0]['c_puct']
    assert all((c['n_playout'], c['c_puct'], c['n']) == (sims, c_puct, 5) for c in cases)
    envs = [RefGomoku.from_moves(B, c['n'], c['pre']) for c in cases] * copies
    twin = Twin(on_demand, module_of(B), len(envs), sims, roots=envs, board=B, add_noise=False, c_puct=c_puct, graph=graph)
    assert twin.ev.hip.range_info()['split_ok']
    return twin


def search_attached(B, cases, on_demand, copies=1):
    """One sim_chunk of the cases' simulations on attached_twin, then everything a comparison reads, on the host -> {'route',
    'launches' (search_launches), 'stats' (delta counters), 'visits', 'trees' and 'reachable' (move_step_twin.reachable) per slot,
    'blocks' (expanded_blocks) of the first copy of every case, 'root_priors'}.  The first read-out flushes: on demand every record by
    rows (k_trunk_policy_rows -> k_heads_rows -> k_deferred_priors_rows), else the store's GEMM and k_deferred_priors."""
    from move_step_twin import reachable
    twin = attached_twin(B, cases, on_demand, copies)
    eng, hip, G = twin.eng, twin.ev.hip, len(cases) * copies
    hip.delta_stats(reset=True)
    twin.search()
    out = {'route': twin.route, 'launches': twin.modes(), 'stats': hip.delta_stats()}
    out['visits'] = eng.root_visits().copy()
    out['trees'] = [eng.tree_dump(g) for g in range(G)]
    out['reachable'] = [reachable(eng, g) for g in range(G)]
    out['blocks'] = [expanded_blocks(eng, g) for g in range(len(cases))]
    out['root_priors'] = eng.root_priors().copy()
    twin.close()   # (engine.check(), HipNet.check_flags(), and: every search of the twin ran in its own mode)
    return out


def prior_errors(B, on_demand, searched=None):
    """The priors a full flush writes against the float64 net -> [(case, max |log(float64(prior)) - logp64| over the legal cells of
    every expanded node, expanded nodes, blocks of a wrong K)]; ``searched``: a search_attached result of the board's robust cases."""
    cases = [c for c in sf.search(B)['cases'] if c['robust']]
    r = search_attached(B, cases, on_demand, COPIES) if searched is None else searched
    out = []
    for rec, blocks in zip(cases, r['blocks']):
        worst, wrong_k = block_errors(blocks, logp64_of(B, rec))
        out.append((rec['name'], worst, len(blocks), wrong_k))
    return out


# ---------------------------------------------------------------------------------------------------------------- e. the games
class Injected(object):
    """numpy.random.choice(acts, p=probs) from a recorded uniform (numpy's legacy algorithm: inverse CDF, side='right')."""

    def __init__(self, us):
        self.us = list(us)
        self.real = np.random.choice

    def __call__(self, acts, p=None):
        cdf = np.cumsum(np.asarray(p, dtype=np.float64))
        cdf /= cdf[-1]
        return np.asarray(acts)[cdf.searchsorted(self.us.pop(0), side='right')]


def play_on_device(game, n_plies, device='cuda:0'):
    """The first ``n_plies`` plies of a recorded game through the reference's API (GameControl.start_self_play + AlphaZeroPlayer on the
    hand-written evaluator) -> (plies whose visit vector and move equal the reference's before the first difference, delta counters)."""
    import torch
    from rlzero_amd.games import GameControl, GomokuEnv
    from rlzero_amd.games.gomoku.alphazero_agent import AlphaZeroAgent
    from rlzero_amd.mcts import AlphaZeroPlayer
    B = game['B']
    agent = AlphaZeroAgent(B, device=device)
    agent.policy_value_net.load_state_dict({k: torch.from_numpy(v) for k, v in sf.weights(B).items()})
    plies = game['plies'][:n_plies]
    inj = Injected([float.fromhex(p['u']) for p in plies])
    seen, stats = [], {}

    class Stop(Exception):
        pass

    np.random.choice = inj
    player = AlphaZeroPlayer(agent.policy_value_fn, n_playout=game['n_playout'], c_puct=game['c_puct'], is_selfplay=True)
    try:
        real = player.mcts.simulate

        def spy(env, temperature=1e-3):
            if len(seen) == len(plies):
                raise Stop()
            k = len(seen)
            if [int(m) for m in env.states.keys()] != game['moves'][:k]:
                raise Stop()
            acts, probs = real(env, temperature)
            visits = player.mcts._engine.root_visits()[0]
            seen.append([int(visits[a]) for a in acts])
            if list(acts) != plies[k]['acts'] or seen[-1] != plies[k]['N']:
                raise Stop()
            return acts, probs

        player.mcts.simulate = spy
        try:
            GameControl(GomokuEnv(B, game['n'])).start_self_play(player, temperature=game['T'])
        except Stop:
            pass
        hip = player.mcts._evaluator.hip
        assert hip.range_info()['split_ok']
        stats = hip.delta_stats()
    finally:
        np.random.choice = inj.real
        eng = getattr(player.mcts, '_engine', None)
        if eng is not None:
            eng.close()
    agree = 0
    while agree < len(seen) and seen[agree] == plies[agree]['N']:
        agree += 1
    return agree, stats


# ---------------------------------------------------------------------------------------------------------------- the report
def report(out=sys.stdout):
    for B in sf.BOARDS:
        head = sf.search(B)
        E, E_lp = sf.tolerances(B)
        out.write('%d x %d  sharp_weights(seed %d, gain %g)  E = %.3g (value)  E_lp = %.3g (log-probabilities)  value std %.3f over %d positions\n'
                  % (B, B, head['seed'], head['gain'], E, E_lp, head['stats']['value_std'], head['stats']['n_positions']))
        for route, (dv, dl) in forward_errors(B).items():
            out.write('  %-28s max |value - reference| %.3g   max |log_probs - reference| %.3g\n' % (route, dv, dl))
        for name, dv, delta, no_base in leaf_errors(B):
            out.write('  leaves of %-9s  max |value - reference| %.3g   (%d against the root\'s base, %d without one)\n' % (name, dv, delta, no_base))
        robust = [c for c in head['cases'] if c['robust']]
        out.write('  robust search cases: %d of %d (%s)\n' % (len(robust), len(head['cases']), ', '.join(c['name'] for c in robust)))
        for resident in (True, False):
            trees, _, stats, _ = search_on_device(B, robust, resident)
            for rec, tree in zip(robust, trees):
                bad, worst = tree_difference(tree, rec)
                out.write('  search %-9s %s: %d of %d nodes with another N, max |W - W_ref| / N %.3g\n'
                          % (rec['name'], 'resident' if resident else 'two-launch', bad, len(rec['tree']), worst))
        for on_demand in (True, False):   # the device move step attached, 7 copies of every case: policy on demand / the store written
            mode = 'on demand' if on_demand else 'store'
            trees, _, _, _ = search_on_device(B, robust, True, on_demand, COPIES)
            w_err = [tree_difference(tree, robust[g % len(robust)]) for g, tree in enumerate(trees)]
            out.write('  attached, %-9s: %d slots, %d nodes with another N, max |W - W_ref| / N %.3g (E = %.3g)\n'
                      % (mode, len(w_err), sum(b for b, _ in w_err), max(x for _, x in w_err), E))
            for name, worst, nodes, wrong_k in prior_errors(B, on_demand):
                out.write('  priors %-9s %-9s: %d expanded nodes, %d with a wrong K, max |log prior - log_probs (f64)| %.3g (E_lp + 2^-22 = %.3g)\n'
                          % (name, mode, nodes, wrong_k, worst, E_lp + 2.0 ** -22))
        out.flush()
    for g in sf.games():
        agree, stats = play_on_device(g, g['robust_plies'])
        out.write('game %d x %d / %d playouts, seed %d: %d plies recorded, %d robust, %d of them identical on the device (visit vectors, moves)\n'
                  % (g['B'], g['B'], g['n_playout'], g['seed'], len(g['plies']), g['robust_plies'], agree))
        out.flush()


if __name__ == '__main__':
    report()
