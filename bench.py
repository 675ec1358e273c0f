#!/usr/bin/env python3
"""bench.py -- throughput of the hdr2yuv convert hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--full]

A *step* is one pass of the hot path (pic_stats -> matrix_convert/PQ -> convert
-> write_yuv arithmetic) over one batch of --frames synthetic frames per GPU,
inputs already resident in HBM, outputs left in HBM in .yuv layout.  Workload =
BASELINE.json configs[1] ("C2"): 3840x2160 fp32 RGB -> PQ -> 12-bit BT.2020nc
YCbCr 4:2:0 (video range), chroma by the 2x2 box (the north_star's fused kernel).

A plain run does only what the headline needs: it sets up, warms up, times the K
steps, checks frame 0 against its known answer, writes --dump-outputs and prints
the line.  --full adds everything else: a device-to-device copy for context, at
N = 1 shorter passes over the FIR resampler (make.sh's example, the CLI's default),
configs[0] / [2] / [3] (C1, C3, C4), the other transfer pairs, the inverse flow
and darker / letterboxed pictures, each with its own roofline fraction and md5
self-check, and the CPU baseline, whose frames 40 of the GPU's output frames are
compared with.

N > 1: one process per GPU.  Started under `python -m torch.distributed.run` the
ranks come from the environment; started as plain `python bench.py --gpus N` this
process launches that command itself BEFORE anything touches the GPU, and exits
with its code.  Frames shard by frame index: rank r owns frames [r*F, (r+1)*F) --
no data-path collective; RCCL carries one all-reduce / all-gather of the counters
(weak scaling).  Fewer than N visible devices is an error, never a silent N = 1.

The output bytes of frame 0 on rank 0 are the SURVEY 8c known-answer frame: their
md5 is checked against tests/golden/known_md5.json after the timed loop
("verified"); a mismatch fails the run.

--dump-outputs DIR writes what the timed path computed in its last step -- the output frames a caller of
h2y_convert_batch receives -- as DIR/*.npy (float32 code values), so that two builds can be compared output for
output on the same inputs (the synthetic frames depend on the arguments alone).  All of the frames when they fit
in 64 MB, else a fixed seeded sample of their samples with its indices (dump_plan).

Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import ctypes as C
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: HBM3E peak (spec); 6290 measured with a plain float4 copy (0.79)

WORKLOADS = {
    # name: (desc kwargs, algorithmic bytes per pixel: read input once + write output once, text, known-answer stem)
    "C2": (dict(width=3840, height=2160, dst_depth=12, dst_matrix=9), 15.0,
           "3840x2160 fp32 RGB -> PQ -> 12-bit BT.2020nc YCbCr 4:2:0", "C2_4k_2020_12b"),
    "C3": (dict(width=3840, height=2160, dst_depth=16, dst_matrix=11, chroma=3), 18.0,
           "3840x2160 fp32 XYZ -> PQ -> 16-bit YDzDx 4:4:4", "C3_4k_ydzdx_16b_444"),
    "C4": (dict(width=7680, height=4320, sample=3, dst_depth=10, dst_matrix=9), 9.0,
           "7680x4320 fp16 RGB -> PQ -> 10-bit BT.2020nc YCbCr 4:2:0", "C4_8k_f16_2020_10b"),
    "C1": (dict(width=1920, height=1080, dst_depth=10, dst_matrix=1), 15.0,
           "1920x1080 fp32 RGB -> PQ -> 10-bit BT.709 YCbCr 4:2:0", "C1_1080p_709_10b"),
}
# the other transfer pairs of the same dispatch point (convert.cpp:1024-1109) on the C2 picture and output format
TF_PAIRS = {"tf_linear_to_bt709": (8, 1, 1), "tf_pq_to_linear": (16, 8, 1), "tf_bt709_to_pq": (1, 16, 2), "tf_pq_to_bt709": (16, 1, 2)}  # src, dst, stages
for _name, (_s, _d, _n) in TF_PAIRS.items():
    WORKLOADS[_name] = (dict(width=3840, height=2160, dst_depth=12, dst_matrix=9, src_transfer=_s, dst_transfer=_d), 15.0,
                        f"3840x2160 fp32 RGB, transfer {_s} -> {_d} ({_n} table stage{'s' if _n > 1 else ''}) -> 12-bit BT.2020nc YCbCr 4:2:0", None)
TRAFFIC_FILE = os.path.join("profiles", "r03_pmc_traffic.json")
DUMP_BYTES = 64_000_000  # --dump-outputs: the files of all ranks together, .npy headers included
DUMP_SEED = 20261015


def positive_int(text):
    v = int(text)
    if v < 1:
        raise argparse.ArgumentTypeError(f"must be at least 1, not {v}")
    return v


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=positive_int, default=20, help="timed steps of the main measurement (ms_per_step is their mean)")
    ap.add_argument("--warmup", type=int, default=10)  # the card clocks up during the first ~10 launches
    ap.add_argument("--frames", type=int, default=128, help="frames per GPU per step (128 x 124 MB = 16 GB of the 288; one launch: the library splits "
                    "longer batches.  Rounds 1-3 measured 64: a launch's fixed costs -- tables staged per block, the blocks' finish spread, "
                    "the FIR path's row segments -- weigh half as much at 128: box +0.5 %% on the kernel and +1.2 %% on value, FIR +1.5 %% / +1.8 %%)")
    ap.add_argument("--workload", default="C2", choices=sorted(WORKLOADS))
    ap.add_argument("--resampler", default="box", choices=["box", "fir"])
    ap.add_argument("--full", action="store_true", help="besides the headline, measure and check everything else: the device copy figure, "
                    "the secondary passes and the CPU baseline (a plain run does none of them)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline and the comparison of frames with it")
    ap.add_argument("--no-extra", action="store_true", help="with --full: skip the secondary measurements (other resampler, C1/C3/C4, ...)")
    ap.add_argument("--cpu-frames", type=int, default=0, help="frames for the CPU baseline sample (0 = auto ~15 s)")
    ap.add_argument("--lib", default=None, help="load this build of libhdr2yuv_hip.so instead of the in-tree one (recorded in the JSON)")
    ap.add_argument("--allow-experiment", action="store_true", help="with --lib: accept a -DH2Y_EXPERIMENT build (timing variants that may write wrong "
                                                                     "bytes); the JSON line then says experiment_build: true and verified: false")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE", help="h2y_ctx_set_option knobs (A/B timing), e.g. fir=twopass")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="process-group backend (nccl = RCCL; gloo only to rehearse N > 1)")
    ap.add_argument("--share-gpu", action="store_true", help="rehearsal: every rank uses cuda:0 (needs --backend gloo)")
    ap.add_argument("--content", default="uniform", choices=["uniform", "bars", "squared", "pow3", "pow4", "pow6"],
                    help="synthetic picture content (fp32 workloads): uniform = the SURVEY 8c generator (the headline; md5-checked); bars = the same "
                         "with the top and bottom 12.8 %% of the rows exactly zero (a 2.39:1 picture letterboxed in 16:9); squared = every sample "
                         "squared (darker).  Not md5-checked; no secondary passes even with --full")
    ap.add_argument("--placement", default="separate", choices=["arena", "separate"],
                    help="arena: the batch's input planes in one allocation back to back and its output frames in another (the .yuv's own "
                         "layout); separate (default): one allocation per plane / frame.  Where the planes lie decides how often the kernels' streams meet in "
                         "a DRAM bank: either way a launch's time moves by several per cent from process to process (DESIGN.md 7.2)")
    ap.add_argument("--no-pipeline", action="store_true", help="finish every step before the next is enqueued (A/B against two batches in flight)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write the main measurement's output frames of its last step to DIR/*.npy (float32; all "
                         "of them when they fit in 64 MB, else a fixed seeded sample of their samples with the samples' indices)")
    ap.add_argument("--rehearse", action="store_true",
                    help="CPU rehearsal of the N-rank launch: ranks rendezvous (gloo), shard the frame indices and reduce made-up counters; "
                         "no device, no conversion, nothing measured")
    return ap.parse_args(argv)


# ---------------------------------------------------------------------------------------------
# N > 1 from a plain `python bench.py --gpus N`: this process only launches the ranks
# ---------------------------------------------------------------------------------------------
def visible_gpus():
    """GPUs this process tree would see, counted WITHOUT any HIP / torch call: the entries of the visibility variables when
    one is set, else the KFD topology nodes that have SIMDs (CPU nodes have none).  None when neither is readable."""
    for var in ("HIP_VISIBLE_DEVICES", "CUDA_VISIBLE_DEVICES", "ROCR_VISIBLE_DEVICES"):
        v = os.environ.get(var)
        if v is not None:
            return len([x for x in v.split(",") if x.strip() != ""])
    top = "/sys/class/kfd/kfd/topology/nodes"
    try:
        n = 0
        for node in os.listdir(top):
            with open(os.path.join(top, node, "properties")) as f:
                props = dict(ln.split()[:2] for ln in f if len(ln.split()) >= 2)
            if int(props.get("simd_count", "0")) > 0:
                n += 1
        return n
    except OSError:
        return None


def launch_ranks(args) -> int:
    """Parent of the N ranks.  Never makes a HIP call -- it does not even import torch: the devices are counted from the
    environment / sysfs (visible_gpus) -- and the ranks are fresh processes started by torch.distributed.run.  Where the
    count cannot be read the ranks decide: each refuses to run without its own device."""
    n = args.gpus
    if not args.rehearse:
        have = visible_gpus()
        need = 1 if args.share_gpu else n
        if have is not None and have < need:
            print(f"[bench] --gpus {n} asked for but only {have} GPU(s) visible: refusing to measure fewer silently", file=sys.stderr)
            return 2
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


# ---------------------------------------------------------------------------------------------
# synthetic input on the device (SURVEY 8c/8d generator; hdr2yuv_amd/synth.py is the host form)
# ---------------------------------------------------------------------------------------------
class DeviceSynth:
    """uint32 s = 12345 + frame; per sample s = s*1664525 + 1013904223; v = (s >> 8) / 2^24; plane[0] = 0, plane[1] = 1.
    Closed form of the LCG in 64-bit integers on the device (wrap-around multiplication keeps the low 32 bits exact)."""

    def __init__(self, n_samples, dev):
        import torch

        a = torch.full((n_samples,), 1664525, dtype=torch.int64, device=dev)
        self.ai = torch.cumprod(a, 0) & 0xFFFFFFFF                                # a^(i+1) mod 2^32
        del a
        geo = torch.cat([torch.ones(1, dtype=torch.int64, device=dev), self.ai[:-1]])
        self.geo_c = ((torch.cumsum(geo, 0) & 0xFFFFFFFF) * 1013904223) & 0xFFFFFFFF  # c * sum_{j<=i} a^j
        del geo

    def frame(self, width, height, k, f16, into=None):
        """Frame k's three planes; `into` = three preallocated tensors (views of the batch's one allocation) to fill."""
        import torch

        n = width * height
        s = (self.ai * (12345 + k) + self.geo_c) & 0xFFFFFFFF
        v = (s >> 8).to(torch.float32) * (1.0 / 16777216.0)
        planes = []
        for c in range(3):
            p = v[c * n:(c + 1) * n]
            if into is not None:
                q = into[c]
                q.copy_(p)  # (converts to half where the plane is half)
            else:
                q = p.to(torch.float16) if f16 else p.clone()
            q[0], q[1] = 0.0, 1.0
            planes.append(q.view(torch.int16) if f16 else q)
        return planes


def dump_plan(n_frames, frame_samples, budget_bytes):
    """Which output samples --dump-outputs writes: None = every one ((n_frames, frame_samples) float32 fits the budget), else
    the sorted global indices (frame * frame_samples + offset) of a fixed seeded sample, sized so that its values (float32) and
    its indices (float64) fit together.  Depends on its arguments alone: two runs with the same arguments write the same samples."""
    import numpy as np

    total = n_frames * frame_samples
    if total * 4 + 4096 <= budget_bytes:
        return None
    n = (budget_bytes - 8192) // 12
    return np.unique(np.random.default_rng(DUMP_SEED).integers(0, total, n, dtype=np.int64))


def dump_frames(dirname, outs_t, frame_samples, budget_bytes, prefix=""):
    """Write the output frames `outs_t` (device int16 tensors of uint16 code values) as dump_plan says; returns what was written."""
    import numpy as np
    import torch

    os.makedirs(dirname, exist_ok=True)
    idx = dump_plan(len(outs_t), frame_samples, budget_bytes)
    if idx is None:
        vals = np.stack([t.cpu().numpy().view(np.uint16) for t in outs_t]).astype(np.float32)
        files = {f"{prefix}yuv_frames": vals}
    else:
        parts = []
        for f, t in enumerate(outs_t):
            lo, hi = np.searchsorted(idx, [f * frame_samples, (f + 1) * frame_samples])
            if hi > lo:
                offs = torch.from_numpy(idx[lo:hi] - f * frame_samples).to(t.device)
                parts.append(t.index_select(0, offs).cpu().numpy().view(np.uint16))
        vals = np.concatenate(parts).astype(np.float32)
        files = {f"{prefix}yuv_sample": vals, f"{prefix}yuv_sample_index": idx.astype(np.float64)}
    for name, a in files.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    return {"dir": dirname, "files": sorted(n + ".npy" for n in files), "frames": len(outs_t), "samples_per_frame": frame_samples,
            "samples": int(vals.size), "of_samples": len(outs_t) * frame_samples, "seed": None if idx is None else DUMP_SEED,
            "what": "output frames of the main measurement's last timed step as float32 code values" +
                    ("" if idx is None else ", a fixed seeded sample; yuv_sample_index = frame * samples_per_frame + offset in the frame")}


def run_steps(ctx, d, n_frames, ins, outs, steps, warmup, barrier, pipeline=True):
    """W untimed + K timed steps. Returns (seconds for K steps, mean kernel ms per step, redone frames, launches per step)."""
    import torch

    for _ in range(warmup):
        ctx.convert_batch_enqueue_raw(d, n_frames, ins, outs)
        ctx.batch_finish()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    kms = 0.0
    redone = 0
    launches = 0
    per_step = []
    # two batches in flight: step k+1 is queued behind step k before step k's statistics are looked at, so the
    # launches follow each other without a gap (same stream: the kernels never overlap, each one's HIP events are its own)
    for k in range(steps):
        ctx.convert_batch_enqueue_raw(d, n_frames, ins, outs)
        if k > 0 or not pipeline:
            redone += ctx.batch_finish()
            ms, launches = ctx.last_kernel_ms()
            kms += ms
            per_step.append(ms)
    if steps > 0 and pipeline:
        redone += ctx.batch_finish()
        ms, launches = ctx.last_kernel_ms()
        kms += ms
        per_step.append(ms)
    torch.cuda.synchronize()
    barrier()
    t1 = time.perf_counter()
    run_steps.last_per_step = per_step  # (diagnostics: every timed step's kernel ms)
    return t1 - t0, kms / max(steps, 1), redone, launches


def cpu_baseline(desc_kw, resampler, n_frames_hint):
    """The reference CPU path timed on this box's host cores, single thread (the
    reference is single-threaded): oracle/_ref (the reference's own object code)
    when that prebuilt library travelled with the repo, else our C restatement.
    Converts frames 0, 1, ... (seed 12345 + k each) and keeps the md5 of every .yuv
    frame it produced: ({figures}, {frame index: md5})."""
    from hdr2yuv_amd.synth import synth_frame
    from oracle import binding as ob

    kind = "port"
    impl = None
    try:
        impl = ob.Ref(build=False)
        kind = "reference"
    except Exception:
        impl = ob.Oracle()
    kw = dict(desc_kw)
    kw["resampler"] = 1 if resampler == "fir" else 0
    od = ob.make_desc(**kw)
    w, h = kw["width"], kw["height"]
    f16 = kw.get("sample") == 3
    md5s = {}
    planes = synth_frame(w, h, 0, f16=f16)
    t0 = time.perf_counter()
    md5s[0] = hashlib.md5(impl.convert_frame(od, planes).tobytes()).hexdigest()
    one = time.perf_counter() - t0
    n = n_frames_hint or max(1, min(8, int(15.0 / max(one, 1e-3))))
    inputs = [synth_frame(w, h, k, f16=f16) for k in range(n)]
    t0 = time.perf_counter()
    outs = [impl.convert_frame(od, planes) for planes in inputs]
    dt = time.perf_counter() - t0
    for k, o in enumerate(outs):
        md5s[k] = hashlib.md5(o.tobytes()).hexdigest()
    return {
        "value": round(n * w * h / dt / 1e6, 3),
        "unit": "Mpixels/s",
        "cores": 1,
        "kind": kind,
        "sample": f"frames 0..{n - 1} of the same {w}x{h} workload ({resampler}), {dt:.1f} s, single thread, "
                  f"pic_stats+matrix_convert+convert+write_yuv arithmetic",
    }, md5s


def cpu_baseline_parallel(desc_kw, resampler, indices):
    """Frame-parallel run of the same CPU path: one single-threaded process per host core, the frames `indices` dealt
    round-robin between them (SURVEY 8d asks for both figures; the reference itself is one process per frame).
    ({figures}, {frame index: md5}) or (None, {})."""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    cores = max(1, min(cores, 16, len(indices)))  # a one-GPU box's CPU share is 16 cores, whatever the affinity mask says
    kw = dict(desc_kw)
    if kw.get("sample") == 3 or kw.get("chroma", 1) != 1 or not indices:
        return None, {}  # the helper script covers the fp32 4:2:0 workloads
    base = [sys.executable, os.path.join(ROOT, "oracle", "cpu_bench.py")]
    for key in ("src_transfer", "dst_transfer"):
        if key in kw:
            base += ["--" + key.replace("_", "-"), str(kw[key])]
    base += [str(kw["width"]), str(kw["height"]), "1" if resampler == "fir" else "0", str(kw["dst_depth"]), str(kw["dst_matrix"])]
    t0 = time.perf_counter()
    procs = [subprocess.Popen(base + [str(k) for k in indices[c::cores]], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True) for c in range(cores)]
    kinds = set()
    md5s = {}
    for p in procs:
        out, _ = p.communicate(timeout=900)
        if p.returncode != 0:
            return None, {}
        lines = out.splitlines()
        kinds.add(lines[0].split()[0])
        for ln in lines[1:]:
            tag, k, digest = ln.split()
            md5s[int(k)] = digest
    dt = time.perf_counter() - t0  # includes the start-up of the processes: a lower bound of the rate
    return {"value": round(len(indices) * kw["width"] * kw["height"] / dt / 1e6, 2), "unit": "Mpixels/s", "cores": cores,
            "kind": "reference" if kinds == {"reference"} else "port",
            "sample": f"{cores} processes, {len(indices)} distinct frames between them, {dt:.1f} s wall including process start-up"}, md5s


def sources_sha256():
    """sha256 over the library's sources (kernels, shim, headers): what a counter file under profiles/ is valid for --
    a rebuild of the same sources gives another binary (build id) but the same kernels."""
    hsh = hashlib.sha256()
    src = os.path.join(ROOT, "hdr2yuv_amd", "csrc")
    for name in sorted(os.listdir(src)) + [os.path.join("..", "..", "include", "hdr2yuv_hip.h")]:
        if name.endswith((".hip", ".h", "Makefile")):
            with open(os.path.join(src, name), "rb") as f:
                hsh.update(name.encode() + b"\0" + f.read())
    return hsh.hexdigest()


def known_md5(stem, is420, resampler):
    if stem is None:
        return "none (no known answer: compared with the CPU reference's frames of this run)", None
    name = stem if not is420 else f"{stem}_{resampler}"
    with open(os.path.join(ROOT, "tests", "golden", "known_md5.json")) as f:
        case = json.load(f)["cases"].get(name)
    return name, (case or {}).get("md5")


def rehearse(args, world, rank):
    """--rehearse: what the ranks do around the measurement, with nothing measured (CPU, gloo)."""
    import torch
    import torch.distributed as dist

    from hdr2yuv_amd.shard import frames_for_rank

    if world > 1:
        dist.init_process_group(backend="gloo")
    F = args.frames
    mine = frames_for_rank(world * F, rank, world)
    desc_kw = WORKLOADS[args.workload][0]
    px = float(len(mine)) * desc_kw["width"] * desc_kw["height"] * args.steps
    secs = 1.0 + 0.25 * rank  # made up: the slowest rank sets the job's time
    mine_t = torch.tensor([secs, px, float(mine.start), float(mine.stop)], dtype=torch.float64)
    allr = [torch.zeros_like(mine_t) for _ in range(world)]
    if world > 1:
        dist.all_gather(allr, mine_t)
    else:
        allr = [mine_t]
    tmax = max(float(t[0]) for t in allr)
    total = sum(float(t[1]) for t in allr)
    out = {"rehearsal": True, "metric": "none (launch rehearsal: nothing measured)", "value": None, "n_gpus": world, "steps": args.steps,
           "warmup": args.warmup, "backend": "gloo", "pixels_total": total, "seconds_max": tmax,
           "per_rank": [{"rank": r, "frames": [int(t[2]), int(t[3])], "seconds": float(t[0])} for r, t in enumerate(allr)]}
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out), flush=True)
    return 0


def main() -> int:
    args = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus > 1 and env_world is None:
        return launch_ranks(args)  # parent: no GPU call before or after
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if rank == 0:
            print(f"[bench] --gpus {args.gpus} but WORLD_SIZE={world}: refusing to report a different N than asked for", file=sys.stderr)
        return 2
    if args.rehearse:
        return rehearse(args, world, rank)

    import torch
    import torch.distributed as dist

    import hdr2yuv_amd as h
    from hdr2yuv_amd import api as h_api
    from hdr2yuv_amd.shard import frames_for_rank

    if args.lib:
        h_api.set_library_path(args.lib, allow_experiment=args.allow_experiment)
    if args.share_gpu:
        if args.backend != "gloo":
            print("[bench] --share-gpu needs --backend gloo", file=sys.stderr)
            return 2
        local_rank = 0
    elif torch.cuda.device_count() <= local_rank:
        print(f"[bench] rank {rank}: no GPU {local_rank} (visible: {torch.cuda.device_count()})", file=sys.stderr)
        return 2
    if world > 1:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        torch.cuda.set_device(local_rank)
        if args.backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend="gloo")
    else:
        torch.cuda.set_device(0)
        local_rank = 0

    def barrier():
        if world > 1:
            dist.barrier()

    dev = torch.device("cuda", local_rank)
    red_dev = dev if args.backend == "nccl" else torch.device("cpu")
    ctx = h.Context(local_rank)
    for kv in args.option:
        name, _, value = kv.partition("=")
        ctx.set_option(name, value)
    lib_path = h.library_path()
    with open(lib_path, "rb") as f:
        lib_sha = hashlib.sha256(f.read()).hexdigest()

    synth_cache = {}

    def device_frames(desc_kw, indices):
        w, hh = desc_kw["width"], desc_kw["height"]
        f16 = desc_kw.get("sample") == 3
        key = 3 * w * hh
        if key not in synth_cache:
            synth_cache.clear()
            synth_cache[key] = DeviceSynth(key, dev)
        indices = list(indices)
        if args.placement == "separate":
            return [synth_cache[key].frame(w, hh, k, f16) for k in indices]
        # one allocation for the batch's input planes, back to back (frame after frame, G B R): where planes lie in memory
        # relative to each other decides how often the kernels' streams meet in a DRAM bank
        n = w * hh
        arena = torch.empty(len(indices) * 3 * n, dtype=torch.float16 if f16 else torch.float32, device=dev)
        return [synth_cache[key].frame(w, hh, k, f16, into=[arena[(i * 3 + c) * n:(i * 3 + c + 1) * n] for c in range(3)]) for i, k in enumerate(indices)]

    def measure(wl, resampler, frames_in, F, steps, warmup, check=(), known=True, dump_dir=None):
        """One timed pass of workload `wl` over F frames per step (frames_in may hold fewer DISTINCT inputs: they repeat;
        every frame has its own output).  Returns a dict of figures; all ranks call it together.  `check`: output frames whose
        md5 rank 0 takes after the timed loop (r["md5_frames"]), to be held against the CPU reference's frames of the same index.
        `dump_dir`: every rank writes its output frames of the last timed step there (dump_frames; r["dump"])."""
        desc_kw, bytes_per_px, wl_name, stem = WORKLOADS[wl]
        is420 = desc_kw.get("chroma", 1) == 1
        w, hh = desc_kw["width"], desc_kw["height"]
        d = h.make_desc(**dict(desc_kw, resampler=1 if resampler == "fir" else 0))
        nb = h.frame_bytes(d)
        if args.placement == "separate":
            outs_t = [torch.empty(nb // 2, dtype=torch.int16, device=dev) for _ in range(F)]
        else:  # the batch's output frames in one allocation, back to back: the bytes of the .yuv file, in its order
            out_arena = torch.empty(F * (nb // 2), dtype=torch.int16, device=dev)
            outs_t = [out_arena[f * (nb // 2):(f + 1) * (nb // 2)] for f in range(F)]
        ins = (C.c_void_p * (3 * F))(*[t.data_ptr() for i in range(F) for t in frames_in[i % len(frames_in)]])
        outs = (C.c_void_p * F)(*[t.data_ptr() for t in outs_t])
        secs, kernel_ms, redone, launches = run_steps(ctx, d, F, ins, outs, steps, warmup, barrier, not args.no_pipeline)
        per_step = list(run_steps.last_per_step)
        mine = torch.tensor([secs, float(F) * w * hh * steps], dtype=torch.float64, device=red_dev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        if world > 1:
            dist.all_gather(allr, mine)  # RCCL over xGMI: two doubles per rank
        else:
            allr = [mine]
        tmax = max(float(t[0]) for t in allr)
        total_px = sum(float(t[1]) for t in allr)
        variant = ctx.last_kernel_variant()
        kernel = ctx.last_kernel_name() + ("+k_fir420" if "+k_fir420" in variant else "")
        # self-check: rank 0's frame 0 is the SURVEY 8c known-answer frame of this workload
        verified, vname, got_md5 = None, None, None
        if rank == 0:
            vname, want = known_md5(stem, is420, resampler)
            if args.content != "uniform" or not known:
                vname, want = f"none (content {args.content if known else 'changed'})", None
            if want:
                got_md5 = hashlib.md5(outs_t[0].cpu().numpy().tobytes()).hexdigest()
                verified = got_md5 == want
        md5_frames = {}
        if rank == 0 and args.content == "uniform":
            for f in check:
                if 0 <= f < F and f < len(frames_in):  # (output f was made from the generator's frame f)
                    md5_frames[f] = hashlib.md5(outs_t[f].cpu().numpy().tobytes()).hexdigest()
        dump = None
        if dump_dir is not None:
            dump = dump_frames(dump_dir, outs_t, nb // 2, DUMP_BYTES // world, f"rank{rank}_" if world > 1 else "")
        del outs_t
        alg_bytes = bytes_per_px * w * hh * F  # per step
        ach_kernel = alg_bytes / (kernel_ms / 1e3) / 1e9 if kernel_ms > 0 else 0.0
        ach_wall = alg_bytes / (secs / steps) / 1e9
        return dict(workload=wl, text=wl_name, resampler=resampler if is420 else "none", is420=is420, secs=tmax, pixels=total_px, steps=steps,
                    per_rank=[float(t[1]) / float(t[0]) / 1e6 for t in allr], kernel_ms=kernel_ms, launches=launches, redone=redone,
                    kernel=kernel, variant=variant, verified=verified, verify_case=vname, md5=got_md5, alg_bytes=alg_bytes,
                    ach_kernel=ach_kernel, ach_wall=ach_wall, w=w, h=hh, frames=F, per_step=per_step, md5_frames=md5_frames, dump=dump)

    def roofline_of(r, traffic=None, traffic_source=None):
        """Dominant kernel of the pass.  Box / 4:4:4 and the fused FIR path run ONE kernel per launch: `achieved` is its
        algorithmic bytes over its HIP-event time on its own stream.  The two-pass FIR form (fused kernel + k_fir420 on a
        second stream) has no single dominant kernel: its figure is over the wall time of a step and says so."""
        two_pass = r["kernel"].endswith("+k_fir420")
        ach = r["ach_wall"] if two_pass else r["ach_kernel"]
        out = {"bound": "hbm", "kernel": r["kernel"], "variant": r["variant"], "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": traffic, "traffic_source": traffic_source,
               "timed_by": "wall time of a step (two kernels on two streams)" if two_pass else "HIP events around the kernel, on its stream",
               "algorithmic_bytes_per_launch": r["alg_bytes"] / max(r["launches"], 1), "launches_per_step": r["launches"],
               "kernel_ms_per_step": round(r["kernel_ms"], 4),
               # every timed step's kernel time: where the allocator put this run's planes moves the mean by 3-10 % from one process to
               # the next while the steps of ONE run agree to about 1 % -- a wide spread here means something else
               "kernel_ms_min_max": [round(min(r["per_step"]), 4), round(max(r["per_step"]), 4)] if r["per_step"] else None,
               "kernel_ms_spread": round((max(r["per_step"]) - min(r["per_step"])) / (sum(r["per_step"]) / len(r["per_step"])), 4) if r["per_step"] else None}
        return out

    # ---- main measurement -----------------------------------------------------------------
    desc_kw, bytes_per_px, wl_name, stem = WORKLOADS[args.workload]
    is420 = desc_kw.get("chroma", 1) == 1
    F = args.frames
    w, hh = desc_kw["width"], desc_kw["height"]
    frames_in = device_frames(desc_kw, frames_for_rank(world * F, rank, world))  # this rank's contiguous block of the global frame sequence
    if args.content != "uniform":
        if desc_kw.get("sample", 2) != 2:
            raise SystemExit("--content applies to the fp32 workloads")
        args.no_extra = True
        bar = int(round(0.128 * hh))
        for fr in frames_in:
            for p in fr:
                if args.content == "squared":
                    p.mul_(p)
                elif args.content.startswith("pow"):  # darker still: 0.4 % / 1.6 % / 6 % of the samples below the kernels' tables
                    p.pow_(int(args.content[3:]))
                else:
                    p[: bar * w] = 0.0
                    p[(hh - bar) * w:] = 0.0
                    p[bar * w + 1] = 1.0  # (the planted 1.0 of the generator sat in the first row: ceiling 1 again)
    torch.cuda.synchronize()

    # --full: a plain device-to-device copy of 1 GiB on this very box (30 times): context only, it swings by +-10 % between runs.
    # A plain run takes and frees the same two buffers without copying: the main pass's output frames are then cut from the
    # same two cached blocks either way, and where the frames lie moves a launch's time by several per cent
    copy_gbs = None
    try:
        src_t = torch.empty(1 << 28, dtype=torch.float32, device=dev)
        dst_t = torch.empty_like(src_t)
        if args.full:
            for _ in range(2):
                dst_t.copy_(src_t)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(30):
                dst_t.copy_(src_t)
            e1.record()
            torch.cuda.synchronize()
            copy_gbs = 30 * 2 * src_t.numel() * 4 / (e0.elapsed_time(e1) / 1e3) / 1e9
        del src_t, dst_t
    except Exception:
        copy_gbs = None

    # frames whose bytes are compared with the CPU reference's (N = 1): 0..7 (the single-thread baseline converts those anyway) and 32
    # more spread over the rest of the batch, the last one included (the frame-parallel baseline converts those): both frame groups,
    # every block's slice range, the first and the last launch split
    do_cpu = rank == 0 and world == 1 and args.full and not args.no_cpu_baseline
    extras = world == 1 and args.full and not args.no_extra
    check = sorted(set(range(min(8, F))) | {8 + (i * (F - 9)) // 31 for i in range(32) if F > 9}) if do_cpu and args.content == "uniform" else []
    main_r = measure(args.workload, args.resampler, frames_in, F, args.steps, args.warmup, check, dump_dir=args.dump_outputs)
    value = main_r["pixels"] / main_r["secs"] / 1e6
    ms_per_step = main_r["secs"] / args.steps * 1e3

    out = {
        "metric": "Mpixels/s, 4K RGB->YUV420 PQ convert path (in-memory, HBM-resident)",
        "value": round(value, 1),
        "unit": "Mpixels/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32+f64",
        "data": "synthetic" if args.content == "uniform" else f"synthetic ({args.content})",
        "config": {
            "workload": f"{args.workload}: {wl_name}, chroma {args.resampler}" if is420 else f"{args.workload}: {wl_name}",
            "frames_per_gpu_per_step": F,
            "frame_shard": "frame index, contiguous block per rank",
            "placement": "input planes of a rank's batch back to back in one allocation, output frames in another" if args.placement == "arena"
                         else "one allocation per plane / output frame",
            "resampler": args.resampler if is420 else "none",
        },
        "frames_per_s": round(value * 1e6 / (w * hh), 1),
        "per_rank_mpixels_s": [round(v, 1) for v in main_r["per_rank"]],
        "verified": main_r["verified"],
        "verified_frames": [],
        "verify": {"case": main_r["verify_case"], "md5": main_r["md5"],
                   "what": "md5 of rank 0's output frame 0 after the timed loop vs tests/golden/known_md5.json; verified_frames (--full): output frames whose md5 "
                           "equals the CPU reference's frame of the same index, converted in this run (cpu_baseline)"},
        "library": {"path": os.path.relpath(lib_path, ROOT) if lib_path.startswith(ROOT) else lib_path, "sha256": lib_sha,
                    "sources_sha256": sources_sha256()},
        "options": args.option,
    }
    if h_api.is_experiment_build():  # only reachable with --lib ... --allow-experiment
        out["experiment_build"] = True
        out["verified"] = False
    traffic, traffic_source = None, None
    tpath = os.path.join(ROOT, TRAFFIC_FILE)
    if os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            ent = tj.get(f"{args.workload}_{args.resampler}_F{F}")
            if ent and not args.lib and tj.get("sources_sha256") == sources_sha256():
                traffic = ent.get("hbm_bytes_per_launch")
                traffic_source = f"{TRAFFIC_FILE} (rocprofv3 --pmc passes over these very sources; static, not this run)"
            elif ent:
                traffic_source = f"{TRAFFIC_FILE} holds counters of other sources: not quoted"
        except Exception:
            traffic = None
    out["roofline"] = roofline_of(main_r, traffic, traffic_source)
    if args.full:
        out["roofline"]["device_copy_gbs"] = None if copy_gbs is None else round(copy_gbs, 1)
    out["frames_redone"] = main_r["redone"]
    if main_r["dump"] is not None:
        out["dump_outputs"] = main_r["dump"]
    failed = main_r["verified"] is False

    # ---- secondary passes (--full, N = 1): the other resampler and the other BASELINE configs -------
    if extras:
        others = {}
        other_md5 = {}
        sec_steps, sec_warm = max(10, args.steps // 2), max(8, args.warmup)  # (the XCD weights settle within the first few launches)
        plan = []
        if is420:
            plan.append((args.workload, "fir" if args.resampler == "box" else "box", F))
        # frames per launch of the passes beside the headline: what a launch pays once weighs less in a longer one (C3 64 -> 128 frames
        # +0.9 %, C1 64 -> 256 small frames +9 %, C4 FIR 16 -> 32 +3 %; C4 box is no faster at 32: tools/framesweep2.sh)
        for wl, nf in (("C3", 128), ("C1", 256), ("C4", 16)):
            if wl != args.workload:
                plan.append((wl, "box", nf))
        if args.workload != "C4":
            plan.append(("C4", "fir", 32))
        if args.workload == "C2":
            for name in TF_PAIRS:
                plan.append((name, "box", F))
        for wl, res, nf in plan:
            kw2 = WORKLOADS[wl][0]
            same_input = (kw2["width"], kw2["height"], kw2.get("sample", 2)) == (w, hh, desc_kw.get("sample", 2))
            if same_input:
                fin = frames_in  # C3 reads the very frames C2 reads (fp32 4K planes)
            else:
                ndist = nf  # every frame of a step its own input (8K: 16 x 199 MB; four inputs read four times each let frame groups
                            # that happened to read the same planes at the same time hit in the caches: 0.72 instead of 0.67)
                fin = device_frames(kw2, range(ndist))
            key = wl if (WORKLOADS[wl][0].get("chroma", 1) != 1 or wl in TF_PAIRS) else f"{wl}_{res}"
            chk = check if (wl == args.workload and nf == F) else ([0, 1, nf - 1] if wl in TF_PAIRS and do_cpu else [])
            r = measure(wl, res, fin, nf, sec_steps, sec_warm, chk)
            hiccup = None
            if r["per_step"] and max(r["per_step"]) > 3.0 * sorted(r["per_step"])[len(r["per_step"]) // 2]:
                # one launch of the pass took several times the others (seen once in a few runs, on the first timed launch after a pass
                # allocated gigabytes: 25 ms against 0.9): not the kernel's speed.  The pass is measured again, the first try reported
                hiccup = [round(x, 3) for x in r["per_step"]]
                r = measure(wl, res, fin, nf, sec_steps, sec_warm, chk)
            if chk:
                other_md5[key] = (res, r["md5_frames"], WORKLOADS[wl][0])
            rf = roofline_of(r)
            others[key] = {"value": round(r["pixels"] / r["secs"] / 1e6, 1), "unit": "Mpixels/s", "ms_per_step": round(r["secs"] / r["steps"] * 1e3, 4),
                           "frames_per_step": nf, "distinct_input_frames": len(fin), "steps": r["steps"], "kernel": r["kernel"], "variant": r["variant"],
                           "frac": rf["frac"], "kernel_ms_min_max": [round(min(r["per_step"]), 4), round(max(r["per_step"]), 4)] if r["per_step"] else None,
                           "kernel_ms_steps": [round(x, 3) for x in r["per_step"]] if r["per_step"] and max(r["per_step"]) > 1.5 * min(r["per_step"]) else None,
                           "frames_redone": r["redone"], "achieved_gbs": rf["achieved"], "timed_by": rf["timed_by"], "bytes_per_pixel": WORKLOADS[wl][1],
                           "verified": r["verified"], "verify_case": r["verify_case"], "workload": r["text"] + (f", chroma {res}" if r["is420"] else "")}
            if hiccup:
                others[key]["measured_again_after_kernel_ms_steps"] = hiccup
            failed = failed or r["verified"] is False
            if fin is not frames_in:
                del fin
                # (no torch.cuda.empty_cache() here: returning gigabytes to the driver in the middle of the run was followed, one
                # run in eight, by a single 12-18 ms launch in the NEXT pass -- the card has 288 GB, the blocks stay cached)
        # the .yuv 4:2:0 -> RGB flow (h2y_inverse_420: Subsample420to444 of both chroma planes + matrix_inverse in one
        # kernel), one 4K frame per call as the entry takes it: 12-bit BT.709 in, 16-bit G,B,R planes out, FIR upsampler
        try:
            import numpy as np

            rng = np.random.default_rng(420)
            n = w * hh
            host = [rng.integers(0, 4096, n if c == 0 else n // 4, dtype=np.uint16) for c in range(3)]
            din = [torch.from_numpy(p.view(np.int16)).to(dev) for p in host]
            dout = [torch.zeros(n, dtype=torch.int16, device=dev) for _ in range(3)]
            torch.cuda.synchronize()
            times = []
            for k in range(5 + sec_steps):
                ctx.inverse_420(w, hh, 12, 0, 1, 16, 1, din, dout)
                if k >= 5:
                    times.append(ctx.last_kernel_ms()[0])
            ms = sum(times) / len(times)
            inv = {"value": round(n / ms / 1e3, 1), "unit": "Mpixels/s", "kernel": ctx.last_kernel_name(), "variant": ctx.last_kernel_variant(),
                   "kernel_ms_per_frame": round(ms, 5), "kernel_ms_min_max": [round(min(times), 5), round(max(times), 5)], "bytes_per_pixel": 9.0,
                   "achieved_gbs": round(9.0 * n / ms / 1e6, 1), "frac": round(9.0 * n / ms / 1e6 / HBM_PEAK_GBS, 4), "frames_per_call": 1,
                   "workload": "3840x2160 12-bit BT.709 Y'CbCr 4:2:0 -> 16-bit G,B,R planes (Subsample420to444 FIR + matrix_inverse)",
                   "timed_by": "HIP events around the kernel, on its stream", "verified": None}
            if do_cpu:
                from oracle import binding as ob

                orc = ob.Oracle()
                full = [host[0], orc.up444(host[1], w, hh, 1, 0, 4095).reshape(-1), orc.up444(host[2], w, hh, 1, 0, 4095).reshape(-1)]
                want = orc.matrix_inverse(w, hh, 12, 0, 1, 16, full)
                inv["verified"] = all(np.array_equal(dout[c].cpu().numpy().view(np.uint16), want[c]) for c in range(3))
                inv["verify_case"] = "all three output planes against the oracle's Subsample420to444 + matrix_inverse of the same frame"
                failed = failed or not inv["verified"]
            others["inverse_420"] = inv
            del din, dout
        except Exception as e:  # a secondary figure never costs the main line
            others["inverse_420"] = {"value": None, "error": str(e)}
        # pictures unlike the headline's (SURVEY 8d's extra distributions): "squared" = every sample squared (dark-heavy, as HDR
        # masters are: 0.03 % of the samples fall below the kernels' LDS tables), "bars" = a 2.39:1 letterbox (a quarter of the rows
        # exact zeros).  Box and FIR each; frame 0 of each pass against the CPU reference's conversion of the same changed frame.
        if args.workload == "C2" and args.content == "uniform":
            def change(planes, content, xp):
                bar = int(round(0.128 * hh))
                for p_ in planes:
                    if content == "squared":
                        p_ *= p_
                    else:
                        p_[: bar * w] = 0.0
                        p_[(hh - bar) * w:] = 0.0
                        p_[bar * w + 1] = 1.0  # (the planted 1.0 of the generator sat in the first row: ceiling 1 again)
            for content in ("squared", "bars"):
                try:
                    fin = device_frames(desc_kw, range(F))
                    for fr in fin:
                        change(fr, content, torch)
                    torch.cuda.synchronize()
                    want = {}
                    if do_cpu:
                        from hdr2yuv_amd.synth import synth_frame
                        from oracle import binding as ob

                        try:
                            impl = ob.Ref(build=False)
                        except Exception:
                            impl = ob.Oracle()
                        planes = synth_frame(w, hh, 0)
                        change(planes, content, None)
                        for res in ("box", "fir"):
                            od = ob.make_desc(width=w, height=hh, dst_depth=desc_kw["dst_depth"], dst_matrix=desc_kw["dst_matrix"], resampler=1 if res == "fir" else 0)
                            want[res] = hashlib.md5(impl.convert_frame(od, planes).tobytes()).hexdigest()
                    for res in ("box", "fir"):
                        r = measure("C2", res, fin, F, sec_steps, sec_warm, [0] if do_cpu else [], known=False)
                        rf = roofline_of(r)
                        ok = (r["md5_frames"].get(0) == want[res]) if do_cpu else None
                        others[f"C2_{res}_{content}"] = {"value": round(r["pixels"] / r["secs"] / 1e6, 1), "unit": "Mpixels/s", "frames_per_step": F, "steps": r["steps"],
                                                        "kernel": r["kernel"], "variant": r["variant"], "frac": rf["frac"], "achieved_gbs": rf["achieved"],
                                                        "kernel_ms_min_max": [round(min(r["per_step"]), 4), round(max(r["per_step"]), 4)] if r["per_step"] else None,
                                                        "frames_redone": r["redone"], "timed_by": rf["timed_by"], "verified": ok,
                                                        "verify_case": "output frame 0 against the CPU reference's conversion of the same changed frame" if do_cpu else None,
                                                        "workload": r["text"] + f", chroma {res}, content {content}"}
                        failed = failed or ok is False
                    del fin
                except Exception as e:  # a secondary figure never costs the main line
                    others[f"C2_{content}"] = {"value": None, "error": str(e)}
        out["others"] = others
        if is420 and args.resampler == "box" and f"{args.workload}_fir" in others:  # round-1 field names, kept
            out["fir_value"] = others[f"{args.workload}_fir"]["value"]
            out["fir_ms_per_step"] = others[f"{args.workload}_fir"]["ms_per_step"]

    if do_cpu:
        def compare(gpu_md5, cpu_md5):
            both = sorted(set(gpu_md5) & set(cpu_md5))
            return [k for k in both if gpu_md5[k] == cpu_md5[k]], [k for k in both if gpu_md5[k] != cpu_md5[k]]

        try:
            out["cpu_baseline"], cpu_md5 = cpu_baseline(desc_kw, args.resampler, args.cpu_frames)
            par, par_md5 = cpu_baseline_parallel(desc_kw, args.resampler, [k for k in check if k not in cpu_md5])
            if par:
                out["cpu_baseline_all_cores"] = par
                cpu_md5.update(par_md5)
            good, bad = compare(main_r["md5_frames"], cpu_md5)
            out["verified_frames"] = good
            if bad:
                out["verified"] = False
                out["verify"]["mismatched_frames"] = bad
                failed = True
            for key, (res, gmd5, okw) in (other_md5 if extras else {}).items():
                par, par_md5 = cpu_baseline_parallel(okw, res, sorted(gmd5))
                good, bad = compare(gmd5, par_md5)
                out["others"][key]["verified_frames"] = good
                if out["others"][key]["verified"] is None:
                    out["others"][key]["verified"] = bool(good) and not bad
                if par:
                    out["others"][key]["cpu_baseline_all_cores"] = par
                if bad:
                    out["others"][key]["verified"] = False
                    out["others"][key]["mismatched_frames"] = bad
                    failed = True
        except Exception as e:  # the baseline is a reported number, never a reason to lose the GPU line
            out["cpu_baseline"] = {"value": None, "unit": "Mpixels/s", "cores": 1, "kind": "port", "sample": f"failed: {e}"}
    ctx.close()
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        print(json.dumps(out), flush=True)
        if failed:
            print("[bench] output bytes do not match the known answer: the figures above are void", file=sys.stderr)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
