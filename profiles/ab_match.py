#!/usr/bin/env python3
"""What a network-vs-network match costs on one GPU: 15 x 15 Gomoku at n_playout = 800, 512 pairs in 1024 slots of one engine, two
random-init networks (rlzero_amd/match.py: two resident searches per move, each over the games of its mover, eager enqueue) --
searched simulations/s and finished games/s --, and, from the same process, self-play's rate at 1024 games in flight (the device
loop, one lane) for comparison.

    python profiles/ab_match.py [--out profiles/match/throughput.txt] [--pairs 512] [--selfplay-moves 60]

No figure of this file is asserted anywhere; the README quotes none until the file exists."""
import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'match', 'throughput.txt'))
    ap.add_argument('--board', type=int, default=15)
    ap.add_argument('--playouts', type=int, default=800)
    ap.add_argument('--pairs', type=int, default=512)
    ap.add_argument('--slots', type=int, default=1024)
    ap.add_argument('--openings', type=int, default=64)
    ap.add_argument('--opening-plies', type=int, default=4)
    ap.add_argument('--selfplay-moves', type=int, default=60, help='move steps of the self-play run that is timed')
    ap.add_argument('--seed', type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    from rlzero_amd.match import BatchedMatch, paired_openings, score
    from rlzero_amd.selfplay import BatchedSelfPlay
    nets = []
    for s in (1, 2):
        torch.manual_seed(s)
        nets.append(PolicyValueNet(args.board).to('cuda:0'))
    openings = paired_openings(args.board, 5, args.openings, args.opening_plies, args.seed)
    match = BatchedMatch.for_networks(nets[0], nets[1], args.board, 5, n_games=args.slots, n_playout=args.playouts, device='cuda:0',
                                      seed=args.seed)
    match.run(min(4, args.pairs), openings)                         # warm-up: reservations, the first launches
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    results = match.run(args.pairs, openings)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    m = dict(seconds=dt, games=len(results), moves=match.moves_done, sims=match.sims_done, stalls=match.stalls_resolved,
             a_score=score(results)['a_score'])
    match.close()
    print('match', m, flush=True)

    sp = BatchedSelfPlay.for_network(nets[0], args.board, 5, n_games=args.slots, n_playout=args.playouts, lanes=1, device='cuda:0',
                                     temperature=1.0, seed=args.seed)
    sp.device_attach(queue_capacity=8 * args.slots)
    sp.run_device(range(args.slots), max_moves=3)                   # warm-up
    torch.cuda.synchronize()
    sp.moves_done = sp.sims_done = 0
    t0 = time.perf_counter()
    done = sp.run_device(range(10 ** 6, 10 ** 6 + 8 * args.slots), max_moves=args.selfplay_moves)
    torch.cuda.synchronize()
    dts = time.perf_counter() - t0
    s = dict(seconds=dts, games=len(done), moves=sp.moves_done, sims=sp.sims_done)
    print('selfplay', s, flush=True)

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# %d x %d Gomoku, n_playout %d, one engine of %d slots, one lane; %s\n' % (args.board, args.board, args.playouts, args.slots,
                                                                                       torch.cuda.get_device_name(0)))
        f.write('# match: %d pairs from %d openings of %d plies, two random-init networks, played to the end (eager moves, two searches\n'
                '# per move); self-play: the device loop with its whole-move graph, %d timed move steps, games refilled\n' % (
                    args.pairs, args.openings, args.opening_plies, args.selfplay_moves))
        f.write('%-10s %10s %10s %10s %14s %12s %12s\n' % ('run', 'seconds', 'games', 'moves', 'simulations', 'sims/s', 'games/s'))
        for name, r in (('match', m), ('self-play', s)):
            f.write('%-10s %10.2f %10d %10d %14d %12.0f %12.2f\n' % (name, r['seconds'], r['games'], r['moves'], r['sims'],
                                                                    r['sims'] / r['seconds'], r['games'] / r['seconds']))
        f.write('# match: %d stalls resolved by the host, score of network A %.4f\n' % (m['stalls'], m['a_score']))
    print(open(args.out).read())


if __name__ == '__main__':
    main()
