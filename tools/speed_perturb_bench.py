#!/usr/bin/env python3
"""What speed perturbation costs on the device (run on the GPU box): aptai_resample_batch_multi next to aptai_resample_batch, and
aptai_warp_targets.

16 clips of 10 s of N(0,1) float32 audio at 48 kHz, already packed on the device, speeds (0.9, 1.0, 1.1):
  single       aptai_resample_batch at 3:1 into the [16][160000] batch                           (the existing launch)
  multi_one    aptai_resample_batch_multi with every row on the 1.0 entry: the same work and the same bits (checked here)
  multi_mixed  aptai_resample_batch_multi with the rows cycling over the three speeds, into [16][177778]
  warp         aptai_warp_targets on the batch's targets: 9 x 16 fp64 tracks and 16 int64 label rows of 499 frames, rows cycling
               over the three speeds (555 / 499 / 454 frames out)
The method is tools/frontend_bench.py's: every case is captured once as a graph of `launches` launches that rotate over `sets`
source / output buffers (together larger than the 256 MiB Infinity Cache for the resampling cases), device events go around
`replays` replays, and the cases alternate round by round inside one process; median, min and max of the rounds.  Whether multi_one
is slower than single is read against the spread of `single` between the rounds of this same call.  One line per figure and a JSON
summary."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aptai_amd import ops
from aptai_amd.frontend import DeviceFrontend
from tools.frontend_bench import _graph, _time

B, SECONDS, RATE, SPEEDS = 16, 10, 48000, (0.9, 1.0, 1.1)


def main(rounds=7, replays=50, sets=8, launches=16):
    g = np.random.RandomState(0)
    fe = DeviceFrontend(RATE, speeds=SPEEDS)
    n = RATE * SECONDS
    one = torch.from_numpy(np.concatenate([g.randn(n).astype(np.float32) for _ in range(B)])).cuda()
    dev = one.device
    off = torch.arange(B + 1, dtype=torch.int64, device=dev) * n
    taps1, first1 = fe._device_tables(dev)
    taps, first, table = fe._device_speed_tables(dev)
    idx = {"multi_one": np.full(B, 1, dtype=np.int32), "multi_mixed": (np.arange(B) % 3).astype(np.int32)}
    idx_d = {k: torch.from_numpy(v).to(dev) for k, v in idx.items()}
    S = {k: int(fe.out_lengths([n] * B, v).max()) for k, v in idx.items()}
    S["single"] = int(fe.out_lengths([n])[0])
    srcs = [one.roll(k * 1001) for k in range(sets)]
    outs = {k: [torch.empty((B, s), device=dev) for _ in range(sets)] for k, s in S.items()}
    assert sets * (one.numel() * 4 + 4 * B * S["single"]) > 256 << 20
    cases = {"single": _graph([(lambda i=i: ops.resample_batch(srcs[i % sets], off, B, taps1, first1, fe.orig, fe.new, fe.Kc, fe.width,
                                                               outs["single"][i % sets], S["single"])) for i in range(launches)])}
    for k in ("multi_one", "multi_mixed"):
        cases[k] = _graph([(lambda i=i, k=k: ops.resample_batch_multi(srcs[i % sets], off, B, taps, first, table, fe._table, idx_d[k], idx[k],
                                                                     outs[k][i % sets], S[k])) for i in range(launches)])
    T_in, R = 499, 10 * B
    n_out = np.array([int(np.ceil(T_in / SPEEDS[i])) for i in idx["multi_mixed"]] * 10)
    trk = torch.randn(9 * B, T_in, device=dev, dtype=torch.float64)
    lab = torch.randint(1, 46, (B, T_in), device=dev)
    n_in_d, n_out_d = torch.full((R,), T_in, device=dev), torch.from_numpy(n_out).to(dev)
    ops.warp_targets(trk, lab, n_in_d, n_out_d, int(n_out.max()))          # the allocator holds the two outputs before the capture
    cases["warp"] = _graph([(lambda: ops.warp_targets(trk, lab, n_in_d, n_out_d, int(n_out.max()))) for _ in range(launches)])
    for graph in cases.values():
        graph.replay()
    torch.cuda.synchronize()
    same = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(outs["single"], outs["multi_one"]))
    print(f"multi_one writes the bits of single: {same}")
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, graph in cases.items():
            t[k].append(_time(graph, replays) / launches)
    summary = {"multi_one_equals_single": same}
    for k in cases:
        med = sorted(t[k])[len(t[k]) // 2]
        print(f"{k}: {med:.1f} us per launch (min {min(t[k]):.1f}, max {max(t[k]):.1f}) over {rounds} rounds of {replays} replays of "
              f"{launches} launches")
        summary[f"{k}_us"], summary[f"{k}_min_us"], summary[f"{k}_max_us"] = round(med, 1), round(min(t[k]), 1), round(max(t[k]), 1)
    print(json.dumps(summary))
    assert same


if __name__ == "__main__":
    main()
