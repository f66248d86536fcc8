#!/usr/bin/env python3
"""What the device audio front end costs next to the host resampler (run on the GPU box).

16 clips of 10 s of N(0,1) audio at 48 kHz and at 44.1 kHz, as float32 and as int16 PCM, already packed on the device:
  resample   aptai_resample_batch into the [16][160000] batch               HBM bytes = B (len_in sizeof(src) + 4 S)
  normalize  aptai_wave_normalize on that batch                             HBM bytes = 12 B S (two reads, one write)
A launch takes of the order of 10 us, less than the Python wrapper needs to enqueue it, and one case's buffers (36-51 MB) would stay
in the 256 MiB Infinity Cache.  So every case is captured ONCE as a graph of `launches` launches that rotate over `sets` separate
source / output buffers (together larger than the cache: a buffer returns after more than 256 MiB of other traffic), and device
events go around `replays` replays of that graph: several milliseconds per timed window, no host work inside it.  The cases
alternate round by round inside one process so that clocks and neighbours hit them alike; median, min and max of the rounds, and the
fraction of the 6.29 TB/s measured HBM roof the HBM bytes alone would give.  For per-kernel times without any of this, run the tool
once under the profiler's kernel trace with statistics, in a run of its own.
Then `hostlogic.resample` (torch conv1d on the CPU) over the same 16 clips, one after the other as a dataset's __getitem__ would,
with the thread count it ran with.  One line per figure and a JSON summary."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from aptai_amd import hostlogic, ops
from aptai_amd.frontend import DeviceFrontend

ROOF = 6.29e12
B, SECONDS = 16, 10


def _graph(fns):
    """One captured graph that runs every launch of `fns` in order on one stream."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for fn in fns:
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for fn in fns:
            fn()
    return g


def _time(graph, replays):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(replays):
        graph.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / replays


def main(rounds=7, replays=50, sets=8, launches=16, host_clips=B):
    g = np.random.RandomState(0)
    cases, host_audio = {}, {}
    for rate in (48000, 44100):
        fe = DeviceFrontend(rate)
        n = rate * SECONDS
        clips = [g.randn(n).astype(np.float32) for _ in range(B)]
        host_audio[rate] = clips
        S = int(fe.out_lengths([n])[0])
        off = torch.arange(B + 1, dtype=torch.int64, device="cuda") * n
        taps, first = fe._device_tables(off.device)
        src = np.concatenate(clips)
        for kind in ("float32", "int16"):
            one = torch.from_numpy(src if kind == "float32" else np.clip(src * 8192, -32768, 32767).astype(np.int16)).cuda()
            bufs = [(one.roll(k * 1001), torch.empty((B, S), device="cuda")) for k in range(sets)]
            fns = [(lambda packed=bufs[i % sets][0], out=bufs[i % sets][1], off=off, taps=taps, first=first, fe=fe, S=S:
                    ops.resample_batch(packed, off, B, taps, first, fe.orig, fe.new, fe.Kc, fe.width, out, S)) for i in range(launches)]
            assert sets * (one.numel() * one.element_size() + 4 * B * S) > 256 << 20
            cases[f"resample_{rate}_{kind}"] = (_graph(fns), launches, B * (n * one.element_size() + 4 * S))
    S16, nsets = 16000 * SECONDS, 4 * sets
    xs = [torch.randn(B, S16, device="cuda") for _ in range(nsets)]
    lens = torch.full((B,), S16, dtype=torch.int64, device="cuda")
    assert nsets * 4 * B * S16 > 256 << 20
    cases["normalize"] = (_graph([(lambda x=x: ops.wave_normalize(x, lens)) for x in xs]), nsets, 12 * B * S16)
    for graph, _, _ in cases.values():
        graph.replay()
    torch.cuda.synchronize()
    t = {k: [] for k in cases}
    for _ in range(rounds):
        for k, (graph, per, _) in cases.items():
            t[k].append(_time(graph, replays) / per)
    summary = {}
    for k, (_, per, nbytes) in cases.items():
        med = sorted(t[k])[len(t[k]) // 2]
        print(f"{k}: {med:.1f} us per launch (min {min(t[k]):.1f}, max {max(t[k]):.1f}) over {rounds} rounds of {replays} replays of "
              f"{per} launches; {nbytes / 1e6:.1f} MB of HBM traffic -> {nbytes / ROOF * 1e6:.1f} us at the roof, "
              f"{nbytes / (med * 1e-6) / ROOF:.2f} of it")
        summary[f"{k}_us"] = round(med, 1)
    threads = torch.get_num_threads()
    for rate, clips in host_audio.items():
        hostlogic.resample(clips[0], rate, 16000)
        t0 = time.perf_counter()
        for c in clips[:host_clips]:
            hostlogic.resample(c, rate, 16000)
        ms = (time.perf_counter() - t0) * 1e3
        print(f"hostlogic.resample {rate} -> 16000, {host_clips} x {SECONDS} s clips one after the other, {threads} torch threads: "
              f"{ms:.1f} ms ({ms / host_clips:.2f} ms per clip)")
        summary[f"host_{rate}_ms"] = round(ms, 1)
    summary["host_threads"] = threads
    print(json.dumps(summary))


if __name__ == "__main__":
    main()
