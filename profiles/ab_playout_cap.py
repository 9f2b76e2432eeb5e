#!/usr/bin/env python3
"""What playout cap randomization buys on one GPU: self-play of 15 x 15 Gomoku at n_playout = 800 with 2048 games in flight (the
device loop, one lane, k_delta_res: four rounds of 512 CU halves per search) without a cap, with the cap (100, 0.25) and the
device's longest-first workgroup order, and with the same cap in slot order.

    python profiles/ab_playout_cap.py [--out profiles/playout_cap/ab.txt] [--moves 120] [--repeat 2]

Every configuration runs in a child process of its own under its own time limit (a fresh runtime, nothing shared but the
seed); the parent only collects the JSON lines and writes the table: moves/s, finished games/s and full-budget plies/s -- the
policy samples a trainer gets.  Opt-in extension: none of this enters bench.py's headline number."""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {
    'cap_off': dict(cap=None, longest_first=True),
    'cap_100_0.25_longest_first': dict(cap=(100, 0.25), longest_first=True),
    'cap_100_0.25_identity': dict(cap=(100, 0.25), longest_first=False),
}


def child(name, args):
    sys.path.insert(0, REPO)
    import torch
    from rlzero_amd.games.gomoku.policy_value_net import PolicyValueNet
    from rlzero_amd.selfplay import BatchedSelfPlay
    cfg = CONFIGS[name]
    torch.manual_seed(1)
    net = PolicyValueNet(args.board).to('cuda:0')
    sp = BatchedSelfPlay.for_network(net, args.board, 5, n_games=args.games, n_playout=args.playouts, lanes=1, device='cuda:0',
                                     temperature=1.0, seed=args.seed)
    sp.cap_longest_first = cfg['longest_first']
    if cfg['cap'] is not None:
        sp.set_playout_cap(*cfg['cap'])
    lane = sp.lanes[0]
    assert lane.eng._ask(lane.evaluator)[0].resident_delta, 'this measurement is about k_delta_res'
    sp.device_attach(queue_capacity=8 * args.games)                    # (before the clock: the capture of the move graph)
    sp.run_device(range(args.games), max_moves=3)                      # warm-up: reservations, first replays
    assert lane.move_graph is not None
    torch.cuda.synchronize()
    sp.moves_done = sp.sims_done = sp.full_plies = 0
    ids = range(10 ** 6, 10 ** 6 + 8 * args.games)                     # (more than the timed moves can finish: slots always refill)
    t0 = time.perf_counter()
    done = sp.run_device(ids, max_moves=args.moves)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(config=name, seconds=dt, moves=sp.moves_done, games=len(done), full_plies=sp.full_plies, sims=sp.sims_done,
                          moves_per_s=sp.moves_done / dt, games_per_s=len(done) / dt, full_plies_per_s=sp.full_plies / dt,
                          sims_per_s=sp.sims_done / dt)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'playout_cap', 'ab.txt'))
    ap.add_argument('--board', type=int, default=15)
    ap.add_argument('--playouts', type=int, default=800)
    ap.add_argument('--games', type=int, default=2048)
    ap.add_argument('--moves', type=int, default=120, help='move steps timed per run')
    ap.add_argument('--repeat', type=int, default=2)
    ap.add_argument('--seed', type=int, default=5)
    ap.add_argument('--limit', type=int, default=240, help='seconds a child may take')
    ap.add_argument('--child', default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args)
    rows = []
    for rep in range(args.repeat):
        for name in CONFIGS:   # (alternating: drift of the box hits every configuration alike)
            cmd = [sys.executable, os.path.abspath(__file__), '--child', name] + [x for k in ('board', 'playouts', 'games', 'moves', 'seed')
                                                                                   for x in ('--' + k, str(getattr(args, k)))]
            out = subprocess.run(['timeout', '-k', '10', str(args.limit)] + cmd, capture_output=True, text=True)
            if out.returncode != 0:   # a fault or a time limit: nothing more is started on the GPU
                sys.stderr.write(out.stdout[-2000:] + out.stderr[-4000:])
                sys.exit('%s failed (exit status %d): stopping' % (name, out.returncode))
            rows.append(json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{')][-1]))
            print(rows[-1], flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('# %d x %d Gomoku, n_playout %d, %d games in flight, device loop, %d timed move steps per run\n' % (
            args.board, args.board, args.playouts, args.games, args.moves))
        f.write('%-28s %10s %10s %12s %14s %12s\n' % ('config', 'seconds', 'moves/s', 'games/s', 'full plies/s', 'sims/s'))
        for r in rows:
            f.write('%-28s %10.2f %10.0f %12.2f %14.0f %12.0f\n' % (r['config'], r['seconds'], r['moves_per_s'], r['games_per_s'],
                                                                    r['full_plies_per_s'], r['sims_per_s']))
    print(open(args.out).read())


if __name__ == '__main__':
    main()
