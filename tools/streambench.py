#!/usr/bin/env python3
"""tools/streambench.py -- end-to-end frames/s from HOST memory, GPU box.
One 4K C2 frame = 99.5 MB up, 24.9 MB down: PCIe-bound.  Compares the synchronous entry
(h2y_convert_frame: upload, convert, download one after the other, pageable numpy buffers) with the
pinned ring of h2y_stream_* (the three overlapped).

`streambench.py inverse`: the .yuv -> G,B,R flow on 4K frames instead.
  1. kernel us per frame (HIP events, h2y_last_kernel_ms) and wall time per frame (host clock, every call synchronous) of
     h2y_inverse_batch at 64 frames per call, next to the single-frame entries (h2y_inverse_420 / h2y_matrix_inverse) called
     64 times, in the same process: 4:2:0 FIR, 4:2:0 replication, 4:4:4;
  2. frames/s from host memory, 4:2:0 FIR: h2y_inverse_frame (pageable, serial) against the inverse stream (depth 3).
Prints one line per figure, then one JSON line with all of them."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import hdr2yuv_amd as h
from hdr2yuv_amd.synth import synth_frame


def inverse_main():
    import json

    import torch

    w, hh, nb, reps = 3840, 2160, 64, 7
    n = w * hh
    rng = np.random.default_rng(4096)
    ctx = h.Context(0)
    res = {"width": w, "height": hh, "frames_per_call": nb, "reps": reps, "stat": "median over reps"}
    for name, chroma, alg in (("420_fir", 1, 1), ("420_replicate", 1, 0), ("444", 3, 0)):
        nc = n // 4 if chroma == 1 else n
        srcs = [[torch.from_numpy(rng.integers(0, 4096, m).astype(np.uint16).view(np.int16)).cuda() for m in (n, nc, nc)] for _ in range(8)]
        frames_in = [srcs[k % 8] for k in range(nb)]  # eight distinct inputs, 64 distinct outputs
        frames_out = [[torch.empty(n, dtype=torch.int16, device="cuda") for _ in range(3)] for _ in range(nb)]
        torch.cuda.synchronize()
        single_k, single_w, batch_k, batch_w = [], [], [], []
        for rep in range(reps + 1):  # rep 0 warms up
            ks = 0.0
            t0 = time.perf_counter()
            for f in range(nb):
                if chroma == 1:
                    ctx.inverse_420(w, hh, 12, 0, 1, 16, alg, frames_in[f], frames_out[f])
                else:
                    ctx.matrix_inverse(w, hh, 12, 0, 1, 16, frames_in[f], frames_out[f])
                ks += ctx.last_kernel_ms()[0]
            tw = time.perf_counter() - t0
            t0 = time.perf_counter()
            ctx.inverse_batch(w, hh, chroma, 12, 0, 1, 16, alg, frames_in, frames_out)
            bw = time.perf_counter() - t0
            if rep:
                single_k.append(ks / nb * 1e3)
                single_w.append(tw / nb * 1e6)
                batch_k.append(ctx.last_kernel_ms()[0] / nb * 1e3)
                batch_w.append(bw / nb * 1e6)
        r = {k: round(float(np.median(v)), 1) for k, v in (("single_kernel_us", single_k), ("single_wall_us", single_w),
                                                            ("batch_kernel_us", batch_k), ("batch_wall_us", batch_w))}
        res[name] = r
        print(f"{name:14s} us/frame  single: kernel {r['single_kernel_us']:7.1f} wall {r['single_wall_us']:7.1f}   "
              f"batch of {nb}: kernel {r['batch_kernel_us']:7.1f} wall {r['batch_wall_us']:7.1f}", flush=True)
        del srcs, frames_in, frames_out
        torch.cuda.empty_cache()

    # host memory, 4:2:0 FIR, BT.709 12 -> 16 bits
    nf = int(os.environ.get("N", "120"))
    depth = int(os.environ.get("DEPTH", "3"))
    planes = [rng.integers(0, 4096, m).astype(np.uint16) for m in (n, n // 4, n // 4)]
    ctx.inverse_frame(w, hh, 1, 12, 0, 1, 16, 1, planes)
    t0 = time.perf_counter()
    for _ in range(nf // 4):
        ctx.inverse_frame(w, hh, 1, 12, 0, 1, 16, 1, planes)
    dt = (time.perf_counter() - t0) / (nf // 4)
    res["host_inverse_frame_ms"] = round(dt * 1e3, 2)
    print(f"h2y_inverse_frame (pageable host buffers, serial): {dt*1e3:7.2f} ms/frame  {1/dt:7.1f} frames/s", flush=True)
    ctx.inverse_stream_open(w, hh, 1, 12, 0, 1, 16, 1, depth)
    inflight = 0
    t0 = time.perf_counter()
    for _ in range(nf):
        dst = ctx.stream_input()
        for c in range(3):
            dst[c][:] = planes[c]  # a memcpy standing in for the file read
        ctx.stream_submit()
        inflight += 1
        if inflight == depth - 1:
            ctx.stream_output()
            inflight -= 1
    while inflight:
        ctx.stream_output()
        inflight -= 1
    dt = (time.perf_counter() - t0) / nf
    ctx.stream_close()
    gb = (n * 3 + n * 6) / 1e9  # 1.5 samples up, 3 down, 2 bytes each
    res["host_inverse_stream_ms"] = round(dt * 1e3, 2)
    res["host_inverse_stream_depth"] = depth
    print(f"inverse stream depth {depth} + host copy into the slot:   {dt*1e3:7.2f} ms/frame  {1/dt:7.1f} frames/s  ({gb/dt:5.1f} GB/s over PCIe)", flush=True)
    ctx.close()
    print(json.dumps({"streambench_inverse": res}), flush=True)


def main():
    n = int(os.environ.get("N", "200"))  # long enough for the start-up (three slots filled by host copies) not to weigh
    depth = int(os.environ.get("DEPTH", "3"))
    w, hh = 3840, 2160
    d = h.make_desc(w, hh, dst_depth=12, dst_matrix=9, resampler=0)
    planes = synth_frame(w, hh, 0)
    ctx = h.Context(0)
    ctx.convert_frame(d, planes)
    t0 = time.perf_counter()
    for _ in range(n // 4):
        ctx.convert_frame(d, planes)
    dt = (time.perf_counter() - t0) / (n // 4)
    print(f"h2y_convert_frame (pageable host buffers, serial):   {dt*1e3:7.2f} ms/frame  {1/dt:7.1f} frames/s", flush=True)

    ctx.stream_open(d, depth)
    for fill in (False, True):
        # fill=True also pays for writing the input into the pinned slot (a memcpy standing in for the file read)
        inflight = 0
        done = 0
        t0 = time.perf_counter()
        for _ in range(n):
            dst = ctx.stream_input()
            if fill or done + inflight < depth:
                for c in range(3):
                    dst[c][:] = planes[c]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                ctx.stream_output()
                inflight -= 1
                done += 1
        while inflight:
            ctx.stream_output()
            inflight -= 1
            done += 1
        dt = (time.perf_counter() - t0) / n
        gb = (3 * w * hh * 4 + h.frame_bytes(d)) / 1e9
        print(f"h2y_stream_* depth {depth}{' + host copy into the slot' if fill else '':28s}: {dt*1e3:7.2f} ms/frame  {1/dt:7.1f} frames/s  ({gb/dt:5.1f} GB/s over PCIe)", flush=True)
    ctx.stream_close()
    ctx.close()


if __name__ == "__main__":
    inverse_main() if sys.argv[1:] == ["inverse"] else main()
