#!/usr/bin/env python3
"""What the Gumbel search from observations (MuZeroTree.search_gumbel_from_obs; k_mz_search's GUMBEL ROOTS instantiations) changes for a
move, and that the launches it was built beside did not move: one process, HIP events on the launch stream, the routes alternating,
medians after warm-up -- the method and the helpers of profiles/ab_mz_search_obs.py and profiles/ab_mz_support.py.

Acrobot's shapes (6 observations, 3 actions), --sims simulations, 256 and --envs games, value transform on, scalar heads and --support:
  launch   `three steps` -- net.initial_inference, the softmax, the copy of the root states, init_roots, search_gumbel -- against `one
           launch` -- search_gumbel_from_obs -- between two events, the same observations and Gumbel rows
  move     ``collect(16)`` of a MuZeroSelfPlay(search='gumbel') on device moves between two events, ``fused_roots`` off and on
  search   the routes this tree left as they were, scalar heads: one ``search_from_obs`` launch (pUCT) and one ``search_gumbel`` launch
           (fresh roots before it, outside the events) -- this tree, and with --parent DIR [--parent2 DIR] (built checkouts of the parent
           commit) the parent twice, as two players; this tree counts as unchanged if it lies within the spread of the two parent players

    python profiles/ab_mz_search_obs_gumbel.py [--out profiles/mz_search_obs_gumbel/ab.txt] [--reps 30] [--parent DIR] [--parent2 DIR]

A report: no figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ab_mz_env import MOVES, timed  # noqa: E402
from ab_mz_reanalyse import load_trainer, spread  # noqa: E402

D, A = 6, 3


def alternate(torch, routes, reps):
    """-> {name: ms of every repetition after 3}; every round starts one route further on."""
    ms = {name: [] for name, _ in routes}
    for rep in range(reps + 3):
        for j in range(len(routes)):
            name, fn = routes[(rep + j) % len(routes)]
            x = timed(torch, fn)
            if rep >= 3:
                ms[name].append(x)
    return ms


def make_tree(mod, torch, n_games, args, support, gumbel=True):
    torch.manual_seed(args.seed)
    net = mod.MuZeroNet(D, A, 64, value_transform=True, support=support).to('cuda:0').eval()
    tree = mod.MuZeroTree(n_games, A, args.sims, device='cuda:0').set_value_transform(True).set_support(support)
    if gumbel:
        tree.set_gumbel(4)
    tree.load_model(net)
    tree.load_root_model(net)
    hidden = torch.zeros((n_games, tree.slots_per_game, 64), dtype=torch.float32, device='cuda:0')
    gen = torch.Generator(device='cuda:0').manual_seed(args.seed)
    obs = torch.randn((n_games, D), generator=gen, device='cuda:0')
    g = -torch.log(-torch.log(torch.rand((n_games, A), generator=gen, device='cuda:0').clamp_(1e-6, 1.0 - 1e-6))).contiguous()
    return net, tree, hidden, obs, g


def part_launch(args, torch, say):
    import rlzero_amd.muzero as here
    say('launch: one Gumbel search of every game from its observation; ms, %d repetitions after 3, the two routes alternating' % args.reps)
    for support in (None, args.support):
        for n_games in (256, args.envs):
            net, tree, hidden, obs, g = make_tree(here, torch, n_games, args, support)

            def three_steps():
                with torch.no_grad():
                    s0, logits, _ = net.initial_inference(obs)
                    hidden[:, 0] = s0
                    tree.init_roots(torch.softmax(logits, dim=1).contiguous())
                tree.search_gumbel(hidden, args.sims, g)
            ms = alternate(torch, [('three steps', three_steps), ('one launch', lambda: tree.search_gumbel_from_obs(obs, hidden, args.sims, g))], args.reps)
            head = '  %5d games  %-10s' % (n_games, 'support %d' % support if support else 'scalar')
            for name, xs in ms.items():
                say('%s %-11s %s' % (head, name, spread(xs)))
            say('%s one launch / three steps = %.3f   (plan %s)' % (head, statistics.median(ms['one launch']) / statistics.median(ms['three steps']),
                                                                   tree.search_plan('observations_gumbel')))
            tree.check()
            tree.close()


def part_move(args, torch, say):
    import rlzero_amd.muzero as here
    say('move: collect(%d) of Gumbel device moves, Acrobot; ms per %d moves, %d repetitions after 3, fused_roots off and on alternating' % (MOVES, MOVES, args.reps))
    for support in (None, args.support):
        for n_envs in (256, args.envs):
            players = []
            for on in (False, True):
                torch.manual_seed(args.seed)
                net = here.MuZeroNet(D, A, 64, value_transform=True, support=support).to('cuda:0').eval()
                players.append(here.MuZeroSelfPlay(net, here.AcrobotBatch(n_envs, 'cuda:0', seed=args.seed), n_sims=args.sims, seed=args.seed,
                                                   moves_per_launch=MOVES, search='gumbel', fused_roots=on))
            ms = alternate(torch, [('off', lambda: players[0].collect(MOVES)), ('on', lambda: players[1].collect(MOVES))], args.reps)
            head = '  %5d envs   %-10s' % (n_envs, 'support %d' % support if support else 'scalar')
            for name, xs in ms.items():
                say('%s fused_roots %-3s %s' % (head, name, spread(xs)))
            say('%s on / off = %.3f' % (head, statistics.median(ms['on']) / statistics.median(ms['off'])))
            for sp in players:
                sp.close()


def part_search(args, torch, say, parents):
    import rlzero_amd.muzero as here
    mods = [('this tree', here)]
    if parents:
        mods = [('parent (1)', parents[0])] + mods + [('parent (2)', parents[1])]
    say('search: the launches of the parent commit, scalar heads; ms, %d repetitions after 3, the players alternating' % args.reps)
    for what in ('search_from_obs', 'search_gumbel'):
        for n_games in (256, args.envs):
            trees, routes = [], []
            for name, mod in mods:
                _, tree, hidden, obs, g = make_tree(mod, torch, n_games, args, None, gumbel=what == 'search_gumbel')
                trees.append(tree)
                if what == 'search_from_obs':
                    routes.append((name, lambda tree=tree, hidden=hidden, obs=obs: tree.search_from_obs(obs, hidden, args.sims)))
                else:
                    tree.uniform = torch.full((n_games, A), 1.0 / A, dtype=torch.float32, device='cuda:0')

                    def fn(tree=tree, hidden=hidden, g=g):   # (the roots are made outside the events: timed() wraps the search alone)
                        tree.search_gumbel(hidden, args.sims, g)
                    routes.append((name, fn))
            ms = {name: [] for name, _ in routes}
            for rep in range(args.reps + 3):
                for j in range(len(routes)):
                    i = (rep + j) % len(routes)
                    if what == 'search_gumbel':
                        trees[i].init_roots(trees[i].uniform)
                    x = timed(torch, routes[i][1])
                    if rep >= 3:
                        ms[routes[i][0]].append(x)
            for name, xs in ms.items():
                say('  %-15s %5d games  %-11s %s' % (what, n_games, name, spread(xs)))
            if parents:
                a, b, c = (statistics.median(ms[k]) for k in ('parent (1)', 'parent (2)', 'this tree'))
                lo, hi = min(a, b), max(a, b)
                say('  %-15s %5d games  the two parent players: %.3f and %.3f; this tree: %.3f, %s' % (
                    what, n_games, a, b, c, 'within their spread' if lo <= c <= hi else 'OUTSIDE their spread by %.3f ms (%.2f %% of the nearer one)' % (
                        (lo - c) if c < lo else (c - hi), 100.0 * ((lo - c) / lo if c < lo else (c - hi) / hi))))
            else:
                say('  parent commit: not measured (no --parent)')
            for tree in trees:
                tree.check()
                tree.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_search_obs_gumbel', 'ab.txt'))
    ap.add_argument('--envs', type=int, default=8192)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--support', type=int, default=31)
    ap.add_argument('--parent', default='', help='a checkout of the parent commit with its library built')
    ap.add_argument('--parent2', default='', help='a second build of the parent commit (default: --parent again, as a second player)')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_mz_search_obs_gumbel.py measures on the GPU: none here')
    parents = []
    if args.parent:
        for i, path in enumerate((args.parent, args.parent2 or args.parent)):
            name = 'rlzero_amd_parent%d' % (i + 1)
            if i == 1 and not args.parent2:
                parents.append(parents[0])
                continue
            load_trainer(os.path.abspath(path), name)
            parents.append(sys.modules[name + '.muzero'])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, 'w')

    def say(line):
        print(line, flush=True)
        out.write(line + '\n')
        out.flush()
    say('# profiles/ab_mz_search_obs_gumbel.py: %s; HIP events on the launch stream; %d simulations' % (torch.cuda.get_device_name(0), args.sims))
    part_launch(args, torch, say)
    part_move(args, torch, say)
    part_search(args, torch, say, parents)
    out.close()


if __name__ == '__main__':
    main()
