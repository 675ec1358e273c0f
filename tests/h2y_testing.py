"""What the tests share: the one loop that drives an opened ring, the launcher of the hdr2yuv program, the upload of numpy arrays to
the device, and a few small helpers.  Plain functions, imported as `import h2y_testing as ht`; a helper that serves one feature stays
in that feature's test file.  test_h2y_testing.py tests the ring loop and the banner parser on the CPU."""
import hashlib
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESULTS = ("compare", "ssim", "deltae", "histogram", "light", "lightdist", "scenesig")


# ---- the ring -------------------------------------------------------------------------------------------------------------

def drive_ring(ctx, inputs, depth, *, refs=None, results=()):
    """Every frame of inputs through the ring that ctx has open (and armed), with depth - 1 frames in flight; closes the ring.
    inputs[k]: one entry per plane of stream_input()'s slot, an array (dst[:] = src) or a callable src(dst); or one callable
    fill(slots).  refs[k] is written to stream_reference() before frame k's submit.  results: which stream_<name>_result() to
    collect with each output, from RESULTS ("histogram": the stats and a copy of the bins; "lightdist": the stats and a copy of
    stream_lightdist_bins(); "light" and "lightdist" are also what a light-only ring returns).  Returns per frame, in output order,
    {"out": a copy or None, <name>: the result}."""
    assert depth >= 2 and set(results) <= set(RESULTS), (depth, results)
    recs, inflight = [], 0

    def take():
        o = ctx.stream_output()
        rec = {"out": None if o is None else o.copy()}
        for name in results:
            r = getattr(ctx, f"stream_{name}_result")()
            if name == "histogram":
                r = (r[0], r[1].copy())  # the bins are the ring's own memory
            elif name == "lightdist":
                r = (r, ctx.stream_lightdist_bins().copy())
            rec[name] = r
        recs.append(rec)

    try:
        for k, inp in enumerate(inputs):
            slots = ctx.stream_input()
            if callable(inp):
                inp(slots)
            else:
                for dst, src in zip(slots, inp):
                    if callable(src):
                        src(dst)
                    else:
                        dst[:] = src
            if refs is not None:
                ctx.stream_reference()[:] = refs[k]
            ctx.stream_submit()
            inflight += 1
            if inflight == depth - 1:
                take()
                inflight -= 1
        while inflight:
            take()
            inflight -= 1
    finally:
        ctx.stream_close()
    assert len(recs) == len(inputs)
    return recs


# ---- the command line -----------------------------------------------------------------------------------------------------

def exe():
    """the hdr2yuv program's path; built first where a clean tree has none"""
    path = os.path.join(ROOT, "hdr2yuv_amd", "hdr2yuv")
    if not os.path.exists(path):
        subprocess.run(["make", "-C", os.path.join(ROOT, "hdr2yuv_amd", "cli"), "--no-print-directory"], check=True)
    return path


def run_cli(args, *, timeout, dry=False):
    """the finished run of hdr2yuv with args (dry: and --dry_run 1); asserts nothing"""
    argv = [exe()] + [str(a) for a in args] + (["--dry_run", "1"] if dry else [])
    return subprocess.run(argv, capture_output=True, text=True, timeout=timeout)


def cli_ok(args, rc=0, timeout=600):
    r = run_cli(args, timeout=timeout)
    assert r.returncode == rc, r.stdout + r.stderr
    return r


def banner(stdout):
    """{key: value} of the 'key: value' lines a run prints; its WARNING and ERROR lines are no such lines"""
    kv = {}
    for ln in stdout.splitlines():
        if ": " in ln and not ln.startswith(("WARNING", "ERROR")):
            k, v = ln.split(": ", 1)
            kv[k] = v
    return kv


def lines_with(stdout, prefixes):
    """stdout's lines that start with prefixes (a string or a tuple of them)"""
    return [ln for ln in stdout.splitlines() if ln.startswith(prefixes)]


# ---- the device -----------------------------------------------------------------------------------------------------------

def dev(x):
    """a copy of x on the device, contiguous: the same bytes and shape; an unsigned type wider than a byte, which torch
    lacks or half supports, as the signed type of its size"""
    import torch

    x = np.ascontiguousarray(x)
    if not x.flags.writeable:  # torch.from_numpy wants one; the upload is the copy otherwise
        x = x.copy()
    if x.dtype.kind == "u" and x.dtype.itemsize > 1:
        x = x.view(f"i{x.dtype.itemsize}")
    return torch.from_numpy(x).cuda()


def host(t, dtype):
    """the tensor's bytes as a numpy array of dtype"""
    return t.cpu().numpy().view(dtype)


def dev_zeros(n, dtype):
    return dev(np.zeros(n, dtype))


# ---- small ones -----------------------------------------------------------------------------------------------------------

def zero_file(path, nbytes):
    with open(path, "wb") as f:
        f.write(bytes(nbytes))
    return path


def plane_sizes(w, hh, chroma):
    """samples in the three planes of a frame: 4:2:0 (chroma 1) or full-size chroma"""
    nc = (w >> 1) * (hh >> 1) if chroma == 1 else w * hh
    return [w * hh, nc, nc]


def noisy(x, depth, rng, amp=3):
    """x with every code moved by up to amp and clipped to depth bits, so that no PSNR is infinite"""
    return np.clip(x.astype(np.int64) + rng.integers(-amp, amp + 1, x.size), 0, (1 << depth) - 1).astype(np.uint16)


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def descs(w, hh, **kw):
    """(the library's descriptor, the oracle's) from the same keywords; their bytes are equal"""
    import hdr2yuv_amd as h
    from oracle import binding as ob

    d, od = h.make_desc(w, hh, **kw), ob.make_desc(w, hh, **kw)
    assert bytes(d) == bytes(od)
    return d, od
