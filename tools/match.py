"""A match between two checkpoints on one MI355X: is network A stronger than network B, and by how much?

    python tools/match.py CKPT_A CKPT_B --board 15 --n-in-row 5 --playouts 800 --pairs 256 --openings 64 --opening-plies 4 --seed 1

A checkpoint is what ``AlphaZeroAgent.save_model`` writes (a directory holding ``model.th``) or a file holding the state_dict of a
PolicyValueNet.  Pair k plays opening k % OPENINGS twice, the networks exchanging seats, on shared draw uniforms
(rlzero_amd/match.py).  Prints the score from A's side as ONE JSON line: games, wins, losses, ties, the score fraction overall
and by seat, the outcomes of the pairs, and the Elo difference the score amounts to.
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description='network-vs-network match from paired openings (one JSON line)')
    ap.add_argument('ckpt_a')
    ap.add_argument('ckpt_b')
    ap.add_argument('--board', type=int, default=6)
    ap.add_argument('--n-in-row', type=int, default=4)
    ap.add_argument('--playouts', type=int, default=400)
    ap.add_argument('--pairs', type=int, default=64, help='pairs of games (each opening is played twice, seats exchanged)')
    ap.add_argument('--openings', type=int, default=16, help='distinct openings; pair k starts from opening k %% OPENINGS')
    ap.add_argument('--opening-plies', type=int, default=2, help='random plies of an opening (even: player 0 to move)')
    ap.add_argument('--slots', type=int, default=0, help='games in flight (0: every game of the match, at most 1024)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--device', default='cuda:0')
    args = ap.parse_args(argv)
    if args.pairs < 1 or args.openings < 1:
        ap.error('--pairs and --openings must be at least 1')
    if args.opening_plies < 0 or args.opening_plies % 2:
        ap.error('--opening-plies must be even (player 0 to move after the opening)')
    return args


def main(argv=None):
    args = parse_args(argv)
    from rlzero_amd.match import BatchedMatch, load_checkpoint, paired_openings, score
    nets = [load_checkpoint(p, args.board, args.device) for p in (args.ckpt_a, args.ckpt_b)]
    openings = paired_openings(args.board, args.n_in_row, args.openings, args.opening_plies, args.seed)
    slots = args.slots if args.slots > 0 else min(2 * args.pairs, 1024)
    match = BatchedMatch.for_networks(nets[0], nets[1], args.board, args.n_in_row, n_games=slots, n_playout=args.playouts,
                                      device=args.device, seed=args.seed)
    t0 = time.time()
    results = match.run(args.pairs, openings)
    seconds = time.time() - t0
    out = score(results)
    out.update(board=args.board, n_in_row=args.n_in_row, playouts=args.playouts, pairs=args.pairs, openings=args.openings,
               opening_plies=args.opening_plies, seed=args.seed, seconds=round(seconds, 3), moves=match.moves_done,
               stalls_resolved=match.stalls_resolved)
    match.close()
    print(json.dumps(out, sort_keys=True))
    return 0


if __name__ == '__main__':
    sys.exit(main())
