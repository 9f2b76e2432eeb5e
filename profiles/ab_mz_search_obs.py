#!/usr/bin/env python3
"""What the search from observations (MuZeroTree.search_from_obs; k_mz_search's ROOTS instantiations) changes for Reanalyse, and that
the launch of ``rz_mz_search`` did not move: one process, HIP events on the launch stream, the routes alternating, medians after warm-up
-- the helpers of profiles/ab_mz_reanalyse.py and profiles/ab_mz_support.py.

  refresh  a buffer staged as profiles/ab_mz_reanalyse.py stages it (CartPole, --envs environments x 48 moves); two MuZeroReanalysers on
           it -- `torch` (initial inference in PyTorch, init_roots, search_fused) and `observations` (one launch per chunk) -- refresh
           256 / 2048 / 16384 drawn positions at --sims simulations with --batch rows per chunk, first event to last
  search   one ``MuZeroTree.search_fused`` launch between two events (fresh roots before it, outside them) at 256 and --envs games: this
           tree, and with --parent DIR (a checkout of the parent commit with its library built) the parent TWICE, as two players; this
           tree counts as unchanged if it lies within the spread of the two parent players

    python profiles/ab_mz_search_obs.py [--out profiles/mz_search_obs/ab.txt] [--reps 30] [--parent DIR]

A report: no figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ab_mz_reanalyse import StageEvents, load_trainer, spread  # noqa: E402
from ab_mz_support import make_player, one_search  # noqa: E402

SIZES = (256, 2048, 16384)


def part_refresh(args, torch, say):
    from rlzero_amd.muzero import CartPoleBatch, MuZeroAgent, MuZeroDeviceReplay, MuZeroReanalyser, MuZeroSelfPlay
    torch.manual_seed(args.seed)
    agent = MuZeroAgent(device='cuda:0')
    env = CartPoleBatch(args.envs, 'cuda:0', seed=args.seed)
    sp = MuZeroSelfPlay(agent.net, env, n_sims=args.sims, seed=args.seed)
    dev = MuZeroDeviceReplay(4, 2, 2000, int(env.max_episode_steps), device='cuda:0', seed=args.seed)
    sp.collect(48, replay=dev)
    sp.close()
    routes = [('torch', MuZeroReanalyser(agent.net, dev, n_sims=args.sims, batch=args.batch, seed=args.seed)),
              ('observations', MuZeroReanalyser(agent.net, dev, n_sims=args.sims, batch=args.batch, seed=args.seed, fused='observations'))]
    for _, rean in routes:
        rean.timer = StageEvents(torch)
    say('refresh: %d episodes held (%d steps), n_sims %d, batch %d; ms per refresh, first event to last, %d repetitions after 3, the routes and '
        'the sizes alternating' % (len(dev), int(dev.lengths().sum()), args.sims, args.batch, args.reps))
    say('  plans: torch %s | observations %s' % (routes[0][1].tree.search_plan(False), routes[1][1].tree.search_plan('observations')))
    got = {(name, n): [] for name, _ in routes for n in SIZES}
    for rep in range(args.reps + 3):
        for n in SIZES:
            for j in range(len(routes)):
                name, rean = routes[(rep + j) % len(routes)]
                rean.reanalyse_sample(n, step=rep)
                ms = rean.timer.take()
                if rep >= 3:
                    got[(name, n)].append(ms)
    for n in SIZES:
        med = {}
        for name, _ in routes:
            rows = got[(name, n)]
            med[name] = statistics.median(r['total'] for r in rows)
            say('  %5d positions (%d chunks)  %-12s %s | medians: positions %.3f, initial inference %.3f, roots + search %.3f, read-out + update %.3f' % (
                n, -(-n // args.batch), name, spread([r['total'] for r in rows]), *[statistics.median(r[k] for r in rows)
                                                                                   for k in ('positions', 'inference', 'search', 'update')]))
        say('  %5d positions  observations / torch = %.3f' % (n, med['observations'] / med['torch']))
    for _, rean in routes:
        rean.close()
    dev.close()


def part_search(args, torch, say, parent):
    import rlzero_amd.muzero as here
    say('search: one rz_mz_search launch (search_fused), CartPole, %d simulations; ms, %d repetitions after 3, the players alternating' % (args.sims, args.reps))
    for n_envs in (256, args.envs):
        routes = [('this tree', here)]
        if parent is not None:
            routes = [('parent (1)', parent)] + routes + [('parent (2)', parent)]
        players = [make_player(mod, torch, 'cartpole', n_envs, args, {}) for _, mod in routes]
        ms = [[] for _ in players]
        for rep in range(args.reps + 3):
            for j in range(len(players)):
                i = (rep + j) % len(players)
                x = one_search(torch, players[i], args.sims)
                if rep >= 3:
                    ms[i].append(x)
        med = {name: statistics.median(xs) for (name, _), xs in zip(routes, ms)}
        for (name, _), xs in zip(routes, ms):
            say('  %5d games  %-11s %s' % (n_envs, name, spread(xs)))
        if parent is not None:
            a, b, c = med['parent (1)'], med['parent (2)'], med['this tree']
            lo, hi = min(a, b), max(a, b)
            say('  %5d games  the two parent players: %.3f and %.3f; this tree: %.3f, %s' % (
                n_envs, a, b, c, 'within their spread' if lo <= c <= hi else 'OUTSIDE their spread by %.3f ms (%.2f %% of the nearer one)' % (
                    (lo - c) if c < lo else (c - hi), 100.0 * ((lo - c) / lo if c < lo else (c - hi) / hi))))
        else:
            say('  parent commit: not measured (no --parent)')
        for sp in players:
            sp.tree.check()
            sp.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_search_obs', 'ab.txt'))
    ap.add_argument('--envs', type=int, default=8192)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--parent', default='', help='a checkout of the parent commit with its library built')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_mz_search_obs.py measures on the GPU: none here')
    parent = None
    if args.parent:
        load_trainer(os.path.abspath(args.parent), 'rlzero_amd_parent')
        parent = sys.modules['rlzero_amd_parent.muzero']
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_mz_search_obs.py: %s; HIP events on the launch stream' % torch.cuda.get_device_name(0))
    part_refresh(args, torch, say)
    part_search(args, torch, say, parent)
    out.close()


if __name__ == '__main__':
    main()
