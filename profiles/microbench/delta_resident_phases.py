"""Cycles per phase of ONE simulation of the resident search with the receptive-field trunk (k_delta_res; wave 0 of the workgroup of
game 0), from a library built with -DRZ_NET_PROFILE (profiles/microbench/build_netprof.sh):

    python profiles/microbench/delta_resident_phases.py [--values] [--backup-rows] [games ...]     (default: 1, 256, 512 games; a whole 800-simulation search each)

--values: the search of policy on demand (k_delta_res<false>: no policy features; the engine here has no move step, so the decision
is forced).
The memo (rz_memo.h; --values only): the share of the timed search's leaves served from it and the entries filled (delta_stats), and
the patch copy's cycles PER HIT -- slot 5 is ticked by a served leaf from the verdict to its two stores (and by conv1 of a pass without
a base: the row is printed only when no leaf went without one), and the share that ran ONE window beside a served one.
RZ_DELTA_MEMO=0 in the environment: the kernel without the memo; =2: the memo without the one-window route; =1: without the twins.
--backup-rows: the library was built with -DRZ_BKP_TICKS=1 (rz_delta.h): the slots of the selection's ticks 1 .. 3 hold the rows of expand +
backup, slot 22 wave 1's conv2.
"""
import ctypes, os, sys
sys.path.insert(0, os.environ.get('GRAFT_REPO_ROOT', '.'))
import rlzero_amd._hip as H
H.library_path = lambda: os.environ.get('RZ_NETPROF_LIB') or os.path.join(os.path.dirname(os.path.abspath(__file__)), 'librlzero_netprof.so')
import rlzero_amd._build as B
B.needs_build = lambda: False
import numpy as np, torch
from rlzero_amd.engine import HipNetEvaluator, MCTSEngine
from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
lib = H.load()
# (since the early release -- ResHook::leaf -- wave 0's rows from the release to conv2 are: 'sel: tail behind the release' + 'verdict' +
# 'requests, ranks' + 'maps; wave 0: planes, conv1' = its arrival at the barrier before conv2, 'bar' behind them its wait there; rows 5 and 6
# are those of the passes without a base; 'selection (up to the release)' ends at the release barrier; the last row is wave 1's)
NAMES = [(0, 'verdict'), (1, 'requests, ranks'), (3, 'maps; wave 0: planes, conv1'), (4, 'bar'), (5, 'conv1'), (6, 'bar'), (7, 'conv2'),
         (9, 'bar + conv3 + heads'), (10, 'bar'), (11, 'features'), (12, 'bar'), (16, 'value layer'), (17, 'expand + backup'),
         # the selection's own rows (-DRZ_SEL_TICKS=<mask>, rz_delta.h: a tick that is off leaves its cycles to the next one taken; 18 = the rest,
         # without any of them the whole selection) and wave 1's pre-scan with the barrier wait behind it
         (2, 'sel: root record'), (8, 'sel: root scan / answer'), (13, 'sel: level-0 cell'), (14, 'sel: deeper levels'), (15, 'sel: tail behind the release'),
         (18, 'selection (up to the release)'), (19, 'wave 1: pre-scan'), (20, 'wave 1: wait behind it'),
         (21, 'wave 1: release -> its arrival at the barrier before conv2')]
FLAGS = ('--values', '--backup-rows')
if '--backup-rows' in sys.argv[1:]:
    BACKUP = {8: 'backup: fetches issued', 13: 'backup: join -> value', 14: 'backup: bookkeeping', 17: 'backup: stores + barrier'}
    NAMES = [(k, BACKUP.get(k, nm)) for k, nm in NAMES] + [(22, 'wave 1: conv2')]
VALUES = '--values' in sys.argv[1:]
if VALUES:
    import rlzero_amd.route as _R
    _R.policy_on_demand = lambda *a, **k: True
sizes = [int(a) for a in sys.argv[1:] if a not in FLAGS] or [1, 256, 512]
for games in sizes:
    torch.manual_seed(0)
    net = PolicyValueNet(15).to('cuda:0')
    ev = HipNetEvaluator(net, 15, 'cuda:0', max_boards=games)
    sims = 800
    eng = MCTSEngine(15, 5, n_games=games, n_playout=sims, device='cuda:0', add_noise=True)
    eng.reset_games()
    assert ev.resident_ok(eng) and ev.resident_delta_ok(eng)
    # a position a few moves into a game (the windows of an empty board's first leaves touch its corner only)
    rng = np.random.default_rng(0)
    for ply in range(6):
        eng.sim_chunk(ev, 40)
        visits = eng.root_visits()
        moves = np.array([int(rng.choice(np.flatnonzero(v > 0))) for v in visits], dtype=np.int32)
        eng.advance(moves)
        eng.step(moves)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev.hip.delta_stats(reset=True)
    a.record(); eng.sim_chunk(ev, sims); b.record(); torch.cuda.synchronize()
    assert (eng.search_launches[True] > 0) == VALUES and (eng.search_launches[False] > 0) != VALUES
    st = ev.hip.delta_stats()
    out = (ctypes.c_longlong * 24)()
    assert lib.rz_net_debug_profile(out) == 0
    us = 1e3 * a.elapsed_time(b) / sims
    total = out[23] / sims
    print('%d games, %d simulations: %.2f us per simulation of a game (events, bases included), %d cycles (%.2f GHz); %.2f conv3 / %.2f conv2 tiles, %.2f changed cells per leaf, %d leaves without a base' % (
        games, sims, us, total, total / us / 1e3, st['tiles3'] / max(1, st['delta'] + st['no_base']), st['tiles2'] / max(1, st['delta'] + st['no_base']),
        st['cells'] / max(1, st['delta'] + st['no_base']), st['no_base']))
    print('   ' + '  '.join('%s=%d' % (nm, out[k] / sims) for k, nm in NAMES) + '  prescans=%d' % st['prescans'], flush=True)
    leaves = max(1, st['delta'] + st['no_base'])
    hits, fills = st.get('memo_hits', 0), st.get('memo_fills', 0)   # (a library from before the memo has neither)
    half = st.get('memo_half', 0)                                   # (one-window leaves: RZ_DELTA_MEMO=2 or a library from before them has none)
    twins = st.get('memo_twins', 0)                                 # (passes that also ran a twin's window: RZ_DELTA_MEMO=3, the default)
    print('   memo: %d of %d leaves served (%.1f %%), %d ran one window (%.1f %%), %d of them with a twin (%.1f %% of leaves), %d entries filled (%.1f a game)' % (
        hits, leaves, 100.0 * hits / leaves, half, 100.0 * half / leaves, twins, 100.0 * twins / leaves, fills, fills / games)
          + ('; game 0, wave 0: patch copy %d cycles per hit (slot 5 / the launch\'s mean hits per game)' % (out[5] / (hits / games))
             if hits and st['no_base'] == 0 else ''), flush=True)
    d1_hits, d1_twins, d1_fills = (st.get(k, 0) for k in ('memo_d1_hits', 'memo_d1_twins', 'memo_d1_fills'))   # (kind D1: RZ_DELTA_MEMO=4, the default)
    print('   memo, kind D1: %d depth-1 leaves served (%.1f %% of leaves), %d depth-1 passes ran a twin (%.1f %%), %d entries filled (%.1f a game)' % (
        d1_hits, 100.0 * d1_hits / leaves, d1_twins, 100.0 * d1_twins / leaves, d1_fills, d1_fills / games), flush=True)
    eng.close(); ev.hip.close()
