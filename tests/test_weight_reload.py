"""Weight reloads on every evaluation route: HipNet.load_state_dict (rz_net_load) and HipNetEvaluator.refresh.

After every learner step the trainer uploads new weights into the SAME device buffers, so that captured hipGraphs stay valid.  Device
state derived from the weights must not outlive an upload: the packed copies (Winograd, split hi / lo, fp8, the FC layouts), the
activation bounds and scales (and with them the trunk route), the receptive-field bases of the roots, the deferred feature store and
the graphs captured on a route.  Every check loads W1, uses it, loads W2 and compares with a FRESH build on W2, bit for bit; every check
also asserts that W2 changes the result, so that none compares W1 with W1.  W2 is another seed scaled x 1.7 (more cells behind their
ReLU, like test_delta_trunk._net) or W1 + 1e-3 randn in every tensor (a learner step: only bit equality sees a stale cache)."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KINDS = ('reseed', 'step')


def _dims(shape):
    if isinstance(shape, (tuple, list)):
        return int(shape[0]), int(shape[1]), int(shape[2]) if len(shape) > 2 else int(shape[0]) * int(shape[1])
    return int(shape), int(shape), int(shape) * int(shape)


def _module(shape, seed, gain=1.0):
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    rows, cols, acts = _dims(shape)
    torch.manual_seed(seed)
    net = PolicyValueNet(rows) if (rows == cols and acts == rows * cols) else PolicyValueNet(rows, cols, acts)
    if gain != 1.0:
        with torch.no_grad():
            for p in net.parameters():
                p.mul_(gain)
    return net


def _sd(net):
    return {k: v.detach().to('cpu').clone() for k, v in net.state_dict().items()}


def _second(w1, shape, kind, seed):
    """W2 of a kind for the state dict ``w1``."""
    import torch
    if kind == 'reseed':
        return _sd(_module(shape, seed, 1.7))
    gen = torch.Generator().manual_seed(seed)
    return {k: v + 1e-3 * torch.randn(v.shape, generator=gen, dtype=v.dtype) for k, v in w1.items()}


def _with(shape, sd):
    """A torch module holding the state dict ``sd``."""
    net = _module(shape, 0)
    net.load_state_dict(sd)
    return net


def _inputs(shape, n=37, seed=1):
    """Planes in [0, 1] (the domain the split trunk's activation bounds cover): half uniform, half 0 / 1 like the tree's leaves."""
    import torch
    rows, cols, _ = _dims(shape)
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand((n, 4, rows, cols), generator=gen)
    x[n // 2:] = (x[n // 2:] < 0.4).float()
    return x


def _f64(shape, sd, x):
    import torch
    net = copy.deepcopy(_with(shape, sd)).double()
    with torch.no_grad():
        lp, v = net(x.double())
    return lp, v[:, 0]


def _hip(shape, sd, algo=None, heads=None, cap=0, max_boards=64):
    from rlzero_amd.engine import HipNet
    hip = HipNet(shape, 'cuda:0', max_boards=max_boards).load_state_dict(sd)
    if algo is not None:
        hip.set_algo(algo)
    if heads is not None:
        hip.set_heads_algo(heads)
    return hip.set_max_workgroups(cap)


# ------------------------------------------------------------------ a. HipNet: every packed copy follows a reload

SHAPES = [6, 9, 15, (12, 16, 192), (6, 7, 7)]
ALGOS = ('direct', 'winograd_f4', 'split_f16', 'split_f16_tiles')


def _heads(shape, algo):
    rows, cols, _ = _dims(shape)
    small = algo.startswith('split') and rows <= 10 and cols <= 10   # (the trunk runs the FC layers itself: boards of up to 10 rows)
    return ('auto', 'f32') + (('in_trunk', ) if small else ())


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in _dims(s)))
def test_hip_net_reload_equals_a_fresh_build(shape, kind):
    """Every trunk algorithm and heads GEMM, capped and not: W1 (forward and trunk run), then W2 == a fresh net on W2 bit for bit and
    within 1e-4 of torch fp64 on W2; W1 again gives the first bits back."""
    import torch
    w1 = _sd(_module(shape, 21))
    w2 = _second(w1, shape, kind, 22)
    x_cpu = _inputs(shape)
    x = x_cpu.to('cuda:0')
    lp64, v64 = _f64(shape, w2, x_cpu)
    for algo in ALGOS:
        for heads in _heads(shape, algo):
            for cap in ((0, ) if algo == 'direct' else (0, 5)):
                hip = _hip(shape, w1, algo, heads, cap)
                fresh = _hip(shape, w2, algo, heads, cap)
                what = (algo, heads, cap)
                lp1, v1 = hip.forward(x)
                f1 = hip.trunk(x)
                hip.load_state_dict(w2)
                lp2, v2 = hip.forward(x)
                lpf, vf = fresh.forward(x)
                assert torch.equal(lp2, lpf) and torch.equal(v2, vf), what
                assert torch.equal(hip.trunk(x), fresh.trunk(x)), what
                assert not torch.equal(lp2, lp1) and not torch.equal(v2, v1), what
                assert float((lp2.cpu().double() - lp64).abs().max()) <= 1e-4, what
                assert float((v2.cpu().double() - v64).abs().max()) <= 1e-4, what
                hip.load_state_dict(w1)
                lp3, v3 = hip.forward(x)
                assert torch.equal(lp3, lp1) and torch.equal(v3, v1) and torch.equal(hip.trunk(x), f1), what
                hip.check_flags()
                hip.close()
                fresh.close()


def _expand(evaluator, envs, shape):
    """One simulation per game on a fresh engine (the roots' expansion) -> (priors, root values) as bytes."""
    from rlzero_amd.engine import MCTSEngine
    from test_production_routes import _set_roots
    eng = MCTSEngine(shape, 5, n_games=len(envs), n_playout=4, device='cuda:0')
    _set_roots(eng, envs)
    eng.sim_chunk(evaluator, 1)
    pri = eng.root_priors().copy()
    rw = eng.root_stats()[1].copy()
    eng.check()
    eng.close()
    return pri.tobytes() + rw.tobytes()


@pytest.mark.parametrize('kind', KINDS)
def test_fp8_trunk_reload_equals_a_fresh_build(kind):
    """'split_f16_fp8' (positions only, narrower than f32: no fp64 claim here) on 15 x 15: the expansion of a batch of roots after
    W1 -> W2 equals a fresh evaluator's on W2, and W1 again gives the first bits back."""
    from rlzero_amd.engine import HipNetEvaluator
    from test_production_routes import _start_positions
    B = 15
    envs = _start_positions('gomoku', B, 5, 12, seed=3)
    w1 = _sd(_module(B, 23))
    w2 = _second(w1, B, kind, 24)
    net = _with(B, w1)

    def evaluator(module):
        ev = HipNetEvaluator(module, B, 'cuda:0', max_boards=len(envs))
        ev.hip.set_algo('split_f16_fp8')
        ev.resident_search = False
        return ev
    ev = evaluator(net)
    first = _expand(ev, envs, B)
    net.load_state_dict(w2)
    ev.refresh()
    second = _expand(ev, envs, B)
    fresh = evaluator(_with(B, w2))
    assert second == _expand(fresh, envs, B) and second != first
    net.load_state_dict(w1)
    ev.refresh()
    assert _expand(ev, envs, B) == first
    ev.hip.close()
    fresh.hip.close()


# ------------------------------------------------------------------ b. the receptive-field base cache

@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('rows,cols', [(15, 15), (12, 16)])
def test_bases_of_the_old_weights_are_not_used_after_a_reload(rows, cols, kind):
    """Bases built with W1, then W2 loaded: rz_net_delta_leaves without a rebuild gives k_trunk_rows' features on W2 bit for bit --
    for bases of the leaves' own roots and for bases of roots two moves older -- and a rebuild evaluates against W2's bases."""
    import torch
    from test_delta_trunk import _delta_features, _dev, _pairs, _planes
    shape = (rows, cols, rows * cols) if rows != cols else rows
    n = 256
    w1 = _sd(_module(shape, 31, 1.7))
    w2 = _second(w1, shape, kind, 32)
    hip = _hip(shape, w1, max_boards=n)
    rng = np.random.default_rng(rows * 100 + cols)
    pairs = _pairs(rng, rows, cols, n, [1, 2, 2, 3, 1, 4, 0, 2])
    planes = _dev(torch, _planes(pairs['leaf'], pairs['leaf_tm'], pairs['leaf_last'], rows, cols))
    older = dict(pairs)   # the roots two moves back (the same side to move): a subset of the leaf with more changed cells
    roots = []
    for i in range(n):
        seq, d = pairs['cells'][i], int(pairs['depth'][i])
        k = len(seq) - d
        k = k - 2 if k >= 2 else k
        b = np.zeros((2, 4), dtype=np.uint64)
        for j in range(k):
            c = int(seq[j])
            b[j % 2, c >> 6] |= np.uint64(1) << np.uint64(c & 63)
        roots.append(b)
    older['root'] = np.stack(roots)
    fresh = _hip(shape, w2, max_boards=n)
    ref = fresh.trunk(planes)
    for base_pairs in (pairs, older):
        hip.load_state_dict(w1)
        old = _delta_features(torch, hip, base_pairs, rows, cols)          # bases built with W1
        assert torch.equal(old, hip.trunk(planes))
        hip.load_state_dict(w2)
        assert torch.equal(hip.trunk(planes), ref) and not torch.equal(ref, old)
        hip.delta_stats(reset=True)
        got = _delta_features(torch, hip, pairs, rows, cols, rebuild=False)   # the W1 bases are still in the cache
        if not torch.equal(got, ref):
            bad = (got != ref).reshape(n, -1).any(dim=1).sum().item()
            raise AssertionError('%d of %d leaves differ from a fresh build on the new weights (bases of the old weights used)' % (bad, n))
        assert hip.delta_stats()['no_base'] == n   # (a reload leaves no base valid)
        hip.delta_stats(reset=True)
        assert torch.equal(_delta_features(torch, hip, base_pairs, rows, cols), ref)
        assert hip.delta_stats()['delta'] > 0
    hip.close()
    fresh.close()


def _snapshot(eng):
    """The root visits and root values as bytes, then every game's tree as its arena means it (test_deferred._whole_tree: N, the bits of
    W and of the priors of every visited node; child slots that no visit has written hold whatever was there before)."""
    from test_deferred import _whole_tree
    return [eng.root_visits().tobytes(), eng.root_values().tobytes()] + [_whole_tree(eng, g) for g in range(eng.n_games)]


def _resident_select_first_0(kind, reload):
    """15 x 15, k_delta_res: 24 simulations with E(W1), then 16 more continued with select_first = 0 (the first leaf from
    rz_select_step, as test_window_sets drives it) by E(W1) refreshed to W2 (reload) or by a fresh E(W2)."""
    from rlzero_amd.engine import HipNetEvaluator, MCTSEngine, check
    from test_window_sets import _edge_roots, _late_roots
    from test_production_routes import _set_roots
    B = 15
    envs = _edge_roots(B, 12, seed=7) + _late_roots(B, 4, seed=8, n_empty=8)
    w1 = _sd(_module(B, 41))
    w2 = _second(w1, B, kind, 42)
    net = _with(B, w1)
    ev = HipNetEvaluator(net, B, 'cuda:0', max_boards=len(envs))
    eng = MCTSEngine(B, 5, n_games=len(envs), n_playout=40, device='cuda:0', add_noise=True, noise_seed=3)
    assert ev.resident_ok(eng) and ev.resident_delta_ok(eng)
    _set_roots(eng, envs)
    eng.set_noise_keys()
    eng.simulate(ev, 24)
    if reload == 'w1':
        ev2 = ev
    elif reload:
        net.load_state_dict(w2)
        ev.refresh()
        ev2 = ev
    else:
        ev2 = HipNetEvaluator(_with(B, w2), B, 'cuda:0', max_boards=len(envs))
    assert eng._deferred_begin(ev2, 16) == 16
    check(eng.lib.rz_select_step(eng.handle, None, eng.stream()), 'rz_select_step')
    ev2.search_resident(eng, 16, False)
    eng._def_pending += 16
    eng._def_stream = eng.torch.cuda.current_stream(eng.device)
    eng.flush_deferred()
    out = _snapshot(eng)
    eng.check()
    eng.close()
    return out


@pytest.mark.parametrize('kind', KINDS)
def test_a_resident_search_continued_after_a_reload(kind):
    """A resident search (k_delta_res) continued with select_first = 0 after a reload equals the same continuation by a fresh
    evaluator on the new weights."""
    got = _resident_select_first_0(kind, True)
    want = _resident_select_first_0(kind, False)
    assert got == want
    assert got != _resident_select_first_0(kind, 'w1')


# ------------------------------------------------------------------ c. engine routes: refresh == a fresh evaluator

ROUTES = {   # name: (board shape, n_in_row, game, score mode, deferred_priors, resident_search, environment, delta, captures)
    'deferred_delta': (15, 5, 'gomoku', 'uct_ref', True, False, {}, True, True),
    'deferred_full': (15, 5, 'gomoku', 'uct_ref', True, False, {'RZ_NET_DELTA': '0'}, False, True),
    'puct_delta': (15, 5, 'gomoku', 'puct', True, False, {}, True, True),
    'resident_delta': (15, 5, 'gomoku', 'uct_ref', True, True, {}, True, False),
    'resident_rows': (15, 5, 'gomoku', 'uct_ref', True, True, {'RZ_NET_DELTA_RESIDENT': '0'}, False, False),
    'resident_compact_6x6': (6, 4, 'gomoku', 'uct_ref', True, True, {}, False, False),
    'resident_compact_connect4': ((6, 7), 4, 'connect4', 'uct_ref', True, True, {}, False, False),
    'in_step_9x9': (9, 5, 'gomoku', 'uct_ref', False, False, {}, False, True),
    'in_step_15x15': (15, 5, 'gomoku', 'uct_ref', False, False, {}, True, True),
}
K_SIMS, M_SIMS, PER = 24, 24, 8
# what each entry must run: (deferred priors, the resident search, the receptive-field trunk, the compact LDS grid)
TAKEN = {'deferred_delta': (True, False, True, False), 'deferred_full': (True, False, False, False),
         'puct_delta': (False, False, True, False), 'resident_delta': (True, True, True, False), 'resident_rows': (True, True, False, False),
         'resident_compact_6x6': (True, True, False, True), 'resident_compact_connect4': (True, True, False, True),
         'in_step_9x9': (False, False, False, False), 'in_step_15x15': (False, False, True, False)}


def _taken(ev, eng):
    deferred, resident = ev.deferred_ok(eng), ev.resident_ok(eng)
    delta = ev.resident_delta_ok(eng) if resident else ev.delta_ok(eng) if deferred else ev.delta_three_launch_ok(eng)
    return deferred, resident, delta, resident and ev.hip.compact_resident()


def _route_evaluator(route, module):
    from rlzero_amd.engine import HipNetEvaluator
    shape, _, game, _, deferred, resident = ROUTES[route][:6]
    net_shape = (6, 7, 7) if game == 'connect4' else shape
    ev = HipNetEvaluator(module, net_shape, 'cuda:0', max_boards=8)
    ev.deferred_priors = deferred
    ev.resident_search = resident
    return ev


def _route_run(route, w1, w2, mode, use_graph):
    """K_SIMS simulations with E(W1), then M_SIMS more on the same roots: mode 'refresh' (E refreshed to W2), 'fresh' (a fresh E(W2)),
    'w1' (E unchanged).  -> (snapshot, delta_stats of the second search)."""
    from rlzero_amd.engine import MCTSEngine
    from test_production_routes import _set_roots, _start_positions
    shape, n_row, game, score = ROUTES[route][:4]
    net_shape = (6, 7, 7) if game == 'connect4' else shape
    net = _with(net_shape, w1)
    ev = _route_evaluator(route, net)
    eng = MCTSEngine(shape, n_row, n_games=8, n_playout=K_SIMS + M_SIMS, device='cuda:0', game=game, score_mode=score,
                     add_noise=True, noise_seed=5)
    assert _taken(ev, eng) == TAKEN[route], route
    if use_graph:
        eng.reset_games()
        assert eng.warm_graph(ev, PER) is not None
    _set_roots(eng, _start_positions(game, shape, n_row, 8, seed=9))
    eng.set_noise_keys()
    eng.simulate(ev, K_SIMS, use_graph=use_graph, sims_per_graph=PER)
    if mode == 'refresh':
        net.load_state_dict(w2)
        ev.refresh()
        ev2 = ev
    elif mode == 'fresh':
        ev2 = _route_evaluator(route, _with(net_shape, w2))
    else:
        ev2 = ev
    assert _taken(ev2, eng) == TAKEN[route], route
    ev2.hip.delta_stats(reset=True)
    eng.simulate(ev2, M_SIMS, use_graph=use_graph and mode != 'fresh', sims_per_graph=PER)
    out = _snapshot(eng)
    st = ev2.hip.delta_stats()
    eng.check()
    ev2.hip.check_flags()
    eng.close()
    return out, st


CASES = [(r, g) for r in ROUTES for g in ((False, True) if ROUTES[r][8] else (False, ))]


@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('route,use_graph', CASES, ids=['%s-%s' % (r, 'graph' if g else 'eager') for r, g in CASES])
def test_a_search_after_refresh_equals_a_fresh_evaluator(monkeypatch, route, use_graph, kind):
    """simulate(k) with E(W1), refresh to W2, simulate(m) on the same roots == the same with a freshly built E(W2) for the m
    simulations: every node's N, W and priors, the root visits and values, bit for bit; graphs warmed before the reload replayed after
    it.  On the receptive-field routes the second search again evaluates leaves against bases (rebuilt for the new weights)."""
    for k, v in ROUTES[route][6].items():
        monkeypatch.setenv(k, v)
    shape, _, game = ROUTES[route][:3]
    net_shape = (6, 7, 7) if game == 'connect4' else shape
    w1 = _sd(_module(net_shape, 51))
    w2 = _second(w1, net_shape, kind, 52)
    got, st = _route_run(route, w1, w2, 'refresh', use_graph)
    want, _ = _route_run(route, w1, w2, 'fresh', False)
    same, _ = _route_run(route, w1, w2, 'w1', use_graph)
    if got != want:
        bad = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
        raise AssertionError('%s: %d of %d read-outs differ from a fresh evaluator on the new weights (first: %s)'
                             % (route, len(bad), len(got), 'root visits' if bad[0] == 0 else 'root values' if bad[0] == 1 else
                                'the tree of game %d' % (bad[0] - 2)))
    assert got != same
    if ROUTES[route][7]:
        assert st['delta'] > 0, st


# ------------------------------------------------------------------ d. self-play with captured graphs

# (more simulations than legal moves: the reference's rule visits every child once before the values order them)
SELFPLAY = [(15, 5, 240, 1, False), (15, 5, 240, 2, False), (15, 5, 240, 1, None), (6, 4, 48, 1, False)]


@pytest.mark.parametrize('B,n_row,sims,lanes,resident', SELFPLAY, ids=['15x15-1lane', '15x15-2lanes', '15x15-resident', '6x6-1lane'])
def test_selfplay_after_refresh_weights_equals_a_fresh_selfplay(B, n_row, sims, lanes, resident):
    """BatchedSelfPlay with graphs: games, a change of the torch module, refresh_weights(), the next game ids == those ids played by a
    fresh for_network on the changed module (games are keyed by id: slots, lanes and what ran before do not matter)."""
    import torch
    from rlzero_amd.selfplay import BatchedSelfPlay
    w1 = _sd(_module(B, 61))
    w2 = _second(w1, B, 'reseed', 62)
    net = _with(B, w1).to('cuda:0').eval()
    kw = dict(board=B, n_in_row=n_row, n_games=4, n_playout=sims, c_puct=5.0, device='cuda:0', temperature=1.0, seed=13, lanes=lanes,
              use_graph=True, sims_per_graph=8, resident_search=resident)

    def same(a, b):
        assert [t.game_id for t in a] == [t.game_id for t in b]
        for x, y in zip(a, b):
            assert (x.winner, x.moves) == (y.winner, y.moves), x.game_id
            assert np.array_equal(np.asarray(x.pis), np.asarray(y.pis)), x.game_id

    sp = BatchedSelfPlay.for_network(net, **kw)
    old = BatchedSelfPlay.for_network(_with(B, w1).to('cuda:0').eval(), **kw)
    sp.run(range(0, 4))
    with torch.no_grad():
        for name, p in net.named_parameters():
            p.copy_(w2[name].to(p.device))
    sp.refresh_weights()
    got = sp.run(range(4, 8))
    fresh = BatchedSelfPlay.for_network(net, **kw)
    same(got, fresh.run(range(4, 8)))
    assert [(t.moves, np.asarray(t.pis).tobytes()) for t in got] != [(t.moves, np.asarray(t.pis).tobytes()) for t in old.run(range(4, 8))]
    for s in (sp, old, fresh):
        for lane in s.lanes:
            lane.eng.close()


# ------------------------------------------------------------------ e. weights that switch the split route off and on again

def _unbounded(w):
    """Weights without a finite activation bound but with moderate outputs: one conv1 channel has a 2e30 centre tap (bound >= 1e30:
    no split route), and conv2 reads that channel with exact zeros -- its f32 activation is finite and multiplied by 0, so the f32
    kernel and fp64 agree."""
    w = {k: v.clone() for k, v in w.items()}
    w['conv1.weight'][7, 0, 1, 1] = 2e30
    w['conv2.weight'][:, 7] = 0.0
    return w


def test_a_route_flip_drops_the_graphs_and_matches_a_fresh_build():
    """A refresh to weights without a finite bound turns the split route off: forward within 1e-4 of fp64, the graphs captured on the
    deferred route are dropped (simulate(use_graph=True) says so instead of replaying them), the search goes on bit-equal to a fresh
    evaluator; finite weights again bring the split route and its bases back, bit-equal to a fresh build."""
    import torch
    from rlzero_amd.engine import HipError, HipNetEvaluator, MCTSEngine
    from test_production_routes import _set_roots, _start_positions
    B = 15
    w1 = _sd(_module(B, 71))
    wf = _unbounded(w1)
    w3 = _second(w1, B, 'step', 72)
    x_cpu = _inputs(B)
    x = x_cpu.to('cuda:0')
    envs = _start_positions('gomoku', B, 5, 8, seed=9)

    def engine(ev, graph):
        eng = MCTSEngine(B, 5, n_games=8, n_playout=64, device='cuda:0', add_noise=True, noise_seed=5)
        ev.resident_search = False
        if graph:
            eng.reset_games()
            assert eng.warm_graph(ev, PER) is not None
        _set_roots(eng, envs)
        eng.set_noise_keys()
        eng.simulate(ev, K_SIMS, use_graph=graph, sims_per_graph=PER)
        return eng

    net = _with(B, w1)
    ev = HipNetEvaluator(net, B, 'cuda:0', max_boards=8)
    eng = engine(ev, True)
    assert ev.hip.range_info()['split_ok'] and ev.deferred_ok(eng) and ev.delta_ok(eng)
    net.load_state_dict(wf)
    ev.refresh()
    assert not ev.hip.range_info()['split_ok'] and not ev.deferred_ok(eng) and not ev.hip.reads_positions()
    lp, v = ev.hip.forward(x)
    lp64, v64 = _f64(B, wf, x_cpu)
    assert float((lp.cpu().double() - lp64).abs().max()) <= 1e-4 and float((v.cpu().double() - v64).abs().max()) <= 1e-4
    with pytest.raises(HipError, match='evaluation route'):   # the graphs of the deferred route are not replayed on the other route
        eng.simulate(ev, PER, use_graph=True, sims_per_graph=PER)
    eng.simulate(ev, 16)
    ref_eng = engine(HipNetEvaluator(_with(B, w1), B, 'cuda:0', max_boards=8), False)
    ev_f = HipNetEvaluator(_with(B, wf), B, 'cuda:0', max_boards=8)
    ev_f.resident_search = False
    ref_eng.simulate(ev_f, 16)
    assert _snapshot(eng) == _snapshot(ref_eng)
    # finite weights again: the split route (positions, deferred priors, receptive-field bases) is back, bit-equal to a fresh build
    net.load_state_dict(w3)
    ev.refresh()
    assert ev.hip.range_info()['split_ok'] and ev.deferred_ok(eng) and ev.delta_ok(eng)
    fresh = _hip(B, w3)
    lp, v = ev.hip.forward(x)
    lpf, vf = fresh.forward(x)
    assert torch.equal(lp, lpf) and torch.equal(v, vf)
    ev.hip.delta_stats(reset=True)
    eng.simulate(ev, 16)
    assert ev.hip.delta_stats()['delta'] > 0
    ev_3 = HipNetEvaluator(_with(B, w3), B, 'cuda:0', max_boards=8)
    ev_3.resident_search = False
    ref_eng.simulate(ev_3, 16)
    assert _snapshot(eng) == _snapshot(ref_eng)
    eng.check()
    ref_eng.check()
    eng.close()
    ref_eng.close()
    fresh.close()


def test_a_route_flip_drops_the_whole_move_graph():
    """The whole-move graph of a resident lane (warm_move_graph) survives a refresh that keeps the route and is dropped by one that
    changes it: play_move_replay then says so instead of replaying it."""
    import torch
    from rlzero_amd.engine import HipError
    from rlzero_amd.selfplay import BatchedSelfPlay
    B = 15
    w1 = _sd(_module(B, 81))
    net = _with(B, w1).to('cuda:0').eval()
    sp = BatchedSelfPlay.for_network(net, board=B, n_in_row=5, n_games=4, n_playout=16, lanes=1, use_graph=False, seed=3)
    sp.device_attach()
    lane = sp.lanes[0]
    graph = lane.move_graph
    assert graph is not None and lane.evaluator.resident_ok(lane.eng)

    def load(sd):
        with torch.no_grad():
            for name, p in net.named_parameters():
                p.copy_(sd[name].to(p.device))
        sp.refresh_weights()
    load(_second(w1, B, 'step', 82))
    assert lane.eng._move_graph is graph   # (the same route: the graph addresses the same buffers)
    load(_unbounded(w1))
    assert not lane.evaluator.hip.range_info()['split_ok'] and lane.eng._move_graph is None
    with pytest.raises(HipError, match='evaluation route'):
        lane.eng.play_move_replay(graph)
    sp.device_stop()
    lane.eng.close()


# ------------------------------------------------------------------ f. load errors

def test_a_state_dict_of_another_board_or_incomplete_is_refused_before_the_upload(monkeypatch):
    """rz_net_load packs the host arrays at the net's own sizes: a state dict of another board, or one missing a tensor, is refused
    with a ValueError before it is called."""
    from rlzero_amd.engine import HipNet
    hip = HipNet(15, 'cuda:0', max_boards=4)
    calls = []
    real = hip.lib.rz_net_load
    monkeypatch.setattr(hip.lib, 'rz_net_load', lambda *a: calls.append(a) or real(*a))
    with pytest.raises(ValueError, match='act_fc1.weight'):
        hip.load_state_dict(_sd(_module(9, 1)))
    c4 = HipNet((6, 7, 7), 'cuda:0', max_boards=4)
    with pytest.raises(ValueError, match='act_fc1'):
        c4.load_state_dict(_sd(_module(6, 1)))
    missing = _sd(_module(15, 1))
    del missing['val_fc2.bias']
    with pytest.raises(ValueError, match='val_fc2.bias'):
        hip.load_state_dict(missing)
    assert calls == []
    hip.load_state_dict(_sd(_module(15, 1)))   # (the right one goes through)
    assert len(calls) == 1
    hip.close()
    c4.close()


def test_delta_calls_with_a_null_net_return_an_argument_error():
    """The engine-side receptive-field calls check the net handle before anything reads it (RZ_ERR_ARG, nothing launched)."""
    import ctypes
    from rlzero_amd import _hip
    from rlzero_amd.engine import MCTSEngine
    eng = MCTSEngine(15, 5, n_games=2, n_playout=4, device='cuda:0')
    lib = eng.lib
    out = _hip.RzValueHead()
    for call in (lambda: lib.rz_net_delta_bases_engine(None, eng.handle, None),
                 lambda: lib.rz_net_delta_step(None, eng.handle, ctypes.byref(out), None),
                 lambda: lib.rz_net_delta_trunk_engine(None, eng.handle, None)):
        assert lib.rz_net_delta_stats(None, None, 0) == -1 and lib.rz_last_error() == b'NULL argument'   # (another message first)
        assert call() == -1
        assert lib.rz_last_error() == b'net handle is NULL'
    eng.close()
