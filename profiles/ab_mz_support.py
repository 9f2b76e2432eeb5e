#!/usr/bin/env python3
"""What the categorical heads cost in the one-launch search (MuZeroNet(value_transform=True, support=S): k_mz_search's CAT
instantiations) against the scalar heads in transformed space (its VT instantiations): one process, HIP events on the launch stream,
the routes alternating, medians after warm-up -- the method and the helpers of profiles/ab_mz_value_transform.py.

Per environment (CartPole, Acrobot) and size (256 and --envs environments), at --sims simulations, every player a MuZeroSelfPlay on
device moves with a net of its own:
  search   one ``MuZeroTree.search_fused`` launch between two events (fresh roots before it, outside them)
  move     ``collect(16)`` between two events: 16 device moves (torch initial inference, root noise, roots, search, k_mz_env_move)
for `scalar` (value_transform=True) | `support` (support=--support as well), and with --parent DIR (a checkout of the parent commit with
its library built) the parent's scalar route TWICE, as two players; the round starts one player further on every time.  The scalar route
counts as unchanged if it lies within the spread of the two parent players; otherwise the file says by how much it does not.

    python profiles/ab_mz_support.py [--out profiles/mz_support/ab.txt] [--reps 30] [--parent DIR] [--support 20]

A report: no figure of this file is asserted anywhere; the README quotes only what the file holds."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from ab_mz_env import MOVES, timed  # noqa: E402
from ab_mz_reanalyse import load_trainer, spread  # noqa: E402


def make_player(mod, torch, kind, n_envs, args, net_kw):
    torch.manual_seed(args.seed)
    env = (mod.CartPoleBatch if kind == 'cartpole' else mod.AcrobotBatch)(n_envs, 'cuda:0', seed=args.seed)
    net = mod.MuZeroNet(env.obs_dim, env.n_actions, **net_kw).to('cuda:0').eval()
    sp = mod.MuZeroSelfPlay(net, env, n_sims=args.sims, seed=args.seed, moves_per_launch=MOVES, fused_moves=False, device_moves=True)
    assert sp.device_moves and sp.fused and getattr(sp.tree, 'support', None) == net_kw.get('support')
    with torch.no_grad():   # the states a lone search starts from
        sp.hidden[:, 0] = net.initial_inference(sp.obs)[0]
    sp.uniform = torch.full((n_envs, env.n_actions), 1.0 / env.n_actions, dtype=torch.float32, device='cuda:0')
    return sp


def one_search(torch, sp, sims):
    sp.tree.init_roots(sp.uniform)
    return timed(torch, lambda: sp.tree.search_fused(sp.hidden, sims))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'mz_support', 'ab.txt'))
    ap.add_argument('--envs', type=int, default=8192)
    ap.add_argument('--sims', type=int, default=50)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--seed', type=int, default=3)
    ap.add_argument('--support', type=int, default=20)
    ap.add_argument('--parent', default='', help='a checkout of the parent commit with its library built')
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('profiles/ab_mz_support.py measures on the GPU: none here')
    import rlzero_amd.muzero as here
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
    say('# profiles/ab_mz_support.py: %s; HIP events on the launch stream; %d simulations, support %d; ms, %d repetitions after 3, the players '
        'of one size and environment alternating (each round starts one player further on)' % (torch.cuda.get_device_name(0), args.sims,
                                                                                             args.support, args.reps))
    for n_envs in (256, args.envs):
        for kind in ('cartpole', 'acrobot'):
            routes = [('scalar', here, dict(value_transform=True)), ('support', here, dict(value_transform=True, support=args.support))]
            if parent is not None:
                routes = [('parent (1)', parent, dict(value_transform=True))] + routes + [('parent (2)', parent, dict(value_transform=True))]
            players = [make_player(mod, torch, kind, n_envs, args, kw) for _, mod, kw in routes]
            for (name, _, _), sp in zip(routes, players):
                say('%5d environments  %-9s %-11s plan: %s' % (n_envs, kind, name, sp.tree.search_plan(False)))
            for what, run in (('search', lambda sp: one_search(torch, sp, args.sims)), ('move x %d' % MOVES, lambda sp: timed(torch, lambda: sp.collect(MOVES)))):
                ms = [[] for _ in players]
                for rep in range(args.reps + 3):
                    for j in range(len(players)):
                        i = (rep + j) % len(players)
                        x = run(players[i])
                        if rep >= 3:
                            ms[i].append(x)
                med = {name: statistics.median(xs) for (name, _, _), xs in zip(routes, ms)}
                for (name, _, _), xs in zip(routes, ms):
                    say('%5d environments  %-9s %-10s %-11s %s' % (n_envs, kind, what, name, spread(xs)))
                say('%5d environments  %-9s %-10s support / scalar = %.3f' % (n_envs, kind, what, med['support'] / med['scalar']))
                if parent is not None:
                    a, b, c = med['parent (1)'], med['parent (2)'], med['scalar']
                    lo, hi = min(a, b), max(a, b)
                    say('%5d environments  %-9s %-10s the two parent players: %.3f and %.3f; scalar: %.3f, %s' % (
                        n_envs, kind, what, a, b, c, 'within their spread' if lo <= c <= hi else 'OUTSIDE their spread by %.3f ms (%.2f %% of the nearer one)' % (
                            (lo - c) if c < lo else (c - hi), 100.0 * ((lo - c) / lo if c < lo else (c - hi) / hi))))
                else:
                    say('  parent commit: not measured (no --parent)')
            for sp in players:
                sp.tree.check()
                sp.close()
    out.close()


if __name__ == '__main__':
    main()
