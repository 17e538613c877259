#!/usr/bin/env python3
"""Time per weight reload of a planner: through the host (`Planner.load_state_dict`: one blocking device-to-host copy per tensor, packing
on one host thread, blocking uploads) against packed on the GPU (`Planner.refresh_weights`, csrc/mz_pack.h), for the CartPole MLP, the
TicTacToe MLP, the Gomoku 9 x 9 example net (32 planes x 2 blocks) and the C5 net (128 planes x 8 blocks, 15 x 15) in f32 and bf16x3.
The weights live on the GPU, as a learner's do.  Per net:

    host_ms            wall time around load_state_dict(net.state_dict()) + planner.synchronize()        (median of --reps)
    device_wall_ms     wall time around refresh_weights() + planner.synchronize()
    device_enqueue_ms  wall time of the refresh_weights() call alone (what the training loop's host thread pays)
    device_event_ms    HIP-event time of the pack kernels, between two events on the producer stream, which the refresh orders around them
    first_refresh_ms   the one-off refresh that derives the gather maps (three host commits over probe tensors)
    launches, bytes_read, bytes_written, GB/s = (bytes_read + bytes_written) / device_event_ms

    python tools/reload_bench.py [--reps 20] [--out profiles/device_reload/reload.json]

--host-only times the host path alone: run from a checkout of the parent commit it gives the parent's numbers on the same box."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))

BOARD = dict(discount=1.0, is_board_game=True, known_bounds=(-1.0, 1.0))
NETS = [
    # name, builder, case, planner config
    ('cartpole_mlp', 'mlp', ('cartpole', (4, 5), 2, 512, 31, 31, 64, 11), {}, 'f32'),
    ('tictactoe_mlp', 'mlp', ('tictactoe', (9, 3, 3), 10, 256, 1, 1, 64, 13), BOARD, 'f32'),
    ('gomoku9_example', 'conv', ('g9', 'board', (9, 9, 9), 82, 2, 32, 1, 1, 41), BOARD, 'f32'),
    ('c5', 'conv', ('c5', 'board', (9, 15, 15), 226, 8, 128, 1, 1, 42), BOARD, 'f32'),
    ('c5_bf16x3', 'conv', ('c5', 'board', (9, 15, 15), 226, 8, 128, 1, 1, 42), BOARD, 'bf16x3'),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-only', action='store_true')
    ap.add_argument('--nets', default='')
    ap.add_argument('--out', default='')
    args = ap.parse_args()
    import torch
    from helpers import build_conv, build_mlp
    from muzero_amd import planner as pl

    dev = torch.device('cuda', 0)
    med = lambda xs: round(statistics.median(xs), 4)  # noqa: E731
    out = []
    for name, kind, case, search, precision in NETS:
        if args.nets and name not in args.nets.split(','):
            continue
        net = (build_mlp if kind == 'mlp' else build_conv)(case).to(dev)
        sd = net.state_dict()
        kw = dict(num_envs=8, num_simulations=8, **search)
        if precision != 'f32':
            kw['conv_precision'] = precision
        rec = dict(net=name, tensors=sum(1 for k in sd if not k.endswith('num_batches_tracked')),
                   weight_bytes=sum(4 * v.numel() for k, v in sd.items() if not k.endswith('num_batches_tracked')))
        H = pl.Planner(pl.make_mz_config(net.planner_spec(), None, **kw), 0)
        H.load_state_dict(sd)
        ts = []
        for _ in range(args.reps):
            H.synchronize()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            H.load_state_dict(sd)
            H.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        rec['host_ms'], rec['host_ms_min'] = med(ts), round(min(ts), 4)
        H.close()
        if not args.host_only:
            D = pl.Planner(pl.make_mz_config(net.planner_spec(), None, **kw), 0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            D.bind_device_weights(sd)
            D.refresh_weights()
            D.synchronize()
            rec['first_refresh_ms'] = round((time.perf_counter() - t0) * 1e3, 3)
            wall, enq, evt = [], [], []
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(args.reps):
                D.synchronize()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                D.refresh_weights()
                t1 = time.perf_counter()
                e1.record()
                D.synchronize()
                t2 = time.perf_counter()
                torch.cuda.synchronize()
                wall.append((t2 - t0) * 1e3)
                enq.append((t1 - t0) * 1e3)
                evt.append(e0.elapsed_time(e1))
            st = D.pack_stats()
            rec.update(device_wall_ms=med(wall), device_enqueue_ms=med(enq), device_event_ms=med(evt), device_event_ms_min=round(min(evt), 4), **st)
            rec['GBps'] = round((st['bytes_read'] + st['bytes_written']) / (rec['device_event_ms'] * 1e-3) / 1e9, 1)
            rec['host_over_device_wall'] = round(rec['host_ms'] / rec['device_wall_ms'], 1)
            D.close()
        print(json.dumps(rec), flush=True)
        out.append(rec)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(dict(what='time per planner weight reload, host path against device refresh (tools/reload_bench.py)', reps=args.reps,
                       host_only=args.host_only, gpu=torch.cuda.get_device_name(0), results=out), open(args.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
