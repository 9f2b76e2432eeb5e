"""A / B of the Gumbel search against the pUCT search, one process, HIP events on the launch stream, the routes alternating, medians of
30 rounds after 5 warm-up rounds -> profiles/mz_gumbel/ab.txt (python profiles/ab_mz_gumbel.py [--out FILE]).

  1. ``search_fused`` against ``search_gumbel`` from the same roots (init_roots inside the timed region of both), CartPole's and
     Acrobot's shapes (2 / 3 actions), 256 and 8192 environments, 50 and 16 simulations, max_considered 4.
  2. One move on device moves, search='puct' against search='gumbel': ``collect(8)`` of a MuZeroSelfPlay with moves_per_launch 8,
     events around the call, divided by 8 (the read of the finished episodes included, as self-play pays it).
NOT measured here: the pUCT launch of this tree against players of the parent commit (two libraries of different ABI do not load into
one process) and the 60-iteration ``train_muzero.py`` observations."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlzero_amd.muzero import AcrobotBatch, CartPoleBatch, MuZeroNet, MuZeroSelfPlay  # noqa: E402
from rlzero_amd.muzero.tree import MuZeroTree  # noqa: E402

DEV, ROUNDS, WARM = 'cuda:0', 30, 5


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def medians(routes):
    """routes: dict name -> callable; alternating rounds -> dict name -> (median ms, min, max)"""
    events = {k: [] for k in routes}
    for r in range(WARM + ROUNDS):
        for k, fn in routes.items():
            ev = timed(fn)
            if r >= WARM:
                events[k].append(ev)
    torch.cuda.synchronize()
    ms = {k: np.array([a.elapsed_time(b) for a, b in v]) for k, v in events.items()}
    return {k: (float(np.median(v)), float(v.min()), float(v.max())) for k, v in ms.items()}


def searches(out):
    out.append('1. search_fused | search_gumbel from the same roots, ms per search of all environments: median (min .. max) of %d' % ROUNDS)
    for name, obs_dim, A in (('cartpole', 4, 2), ('acrobot', 6, 3)):
        torch.manual_seed(0)
        net = MuZeroNet(obs_dim, A).to(DEV).eval()
        for G in (256, 8192):
            for n_sims in (50, 16):
                tree = MuZeroTree(G, A, n_sims, device=DEV).set_gumbel(4)
                tree.load_model(net)
                hidden = torch.zeros((G, tree.slots_per_game, 64), dtype=torch.float32, device=DEV)
                with torch.no_grad():
                    s0, logits, _ = net.initial_inference(torch.randn(G, obs_dim, device=DEV))
                    hidden[:, 0] = s0
                    probs = torch.softmax(logits, dim=1).contiguous()
                g = -torch.log(-torch.log(torch.rand(G, A, device=DEV).clamp_(1e-7, 1 - 1e-7))).contiguous()

                def puct():
                    tree.init_roots(probs)
                    tree.search_fused(hidden, n_sims)

                def gumbel():
                    tree.init_roots(probs)
                    tree.search_gumbel(hidden, n_sims, g)

                m = medians({'puct': puct, 'gumbel': gumbel})
                tree.check()
                plan = tree.search_plan(False)
                out.append('%-8s G=%-5d n_sims=%-3d trees in %s: puct %.3f (%.3f .. %.3f) | gumbel %.3f (%.3f .. %.3f) | ratio %.2f'
                           % (name, G, n_sims, 'LDS' if plan['tree_in_lds'] else 'HBM', *m['puct'], *m['gumbel'], m['gumbel'][0] / m['puct'][0]))
                tree.close()


def moves(out):
    out.append('2. one move on device moves (collect(8) / 8), ms: median (min .. max) of %d' % ROUNDS)
    for name, cls in (('cartpole', CartPoleBatch), ('acrobot', AcrobotBatch)):
        for G in (256, 8192):
            for n_sims in (50, 16):
                torch.manual_seed(0)
                net = MuZeroNet(cls.obs_dim, cls.n_actions).to(DEV).eval()
                sps = {k: MuZeroSelfPlay(net, cls(G, DEV, seed=1), n_sims=n_sims, seed=1, moves_per_launch=8, fused_moves=False,
                                         device_moves=True, search=k) for k in ('puct', 'gumbel')}
                m = medians({k: (lambda sp=sp: sp.collect(8)) for k, sp in sps.items()})
                out.append('%-8s G=%-5d n_sims=%-3d: puct %.3f (%.3f .. %.3f) | gumbel %.3f (%.3f .. %.3f) | ratio %.2f'
                           % (name, G, n_sims, *(x / 8 for x in m['puct']), *(x / 8 for x in m['gumbel']), m['gumbel'][0] / m['puct'][0]))
                for sp in sps.values():
                    sp.close()


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.abspath(__file__)), 'mz_gumbel', 'ab.txt'))
    args = ap.parse_args()
    lines = ['# profiles/ab_mz_gumbel.py on %s: one process, HIP events, the routes alternating' % torch.cuda.get_device_name(0)]
    searches(lines)
    moves(lines)
    lines.append('Not measured: the pUCT launch against players of the parent commit, and the train_muzero.py observations.')
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    print('\n'.join(lines))
