"""The helpers the tests share (h2y_testing.py), on the CPU: the ring loop against a context that only records what is called on
it, and the banner parser against a captured banner."""
import numpy as np
import pytest

import h2y_testing as ht

PLANES = 3


class FakeRing:
    """What drive_ring needs of a context.  A frame's output is the sum of its slot; every result names the frame it belongs to;
    taking an output with nothing in flight, or with more than depth - 1 in flight, fails."""

    def __init__(self, depth, has_output=True):
        self.depth, self.has_output = depth, has_output
        self.slots = [[np.zeros(4, np.int64) for _ in range(PLANES)] for _ in range(depth)]
        self.ref = np.zeros(2, np.int64)
        self.calls, self.queue, self.most = [], [], 0
        self.submitted = self.taken = self.closed = 0
        self.last = None

    def stream_input(self):
        self.calls.append("input")
        return self.slots[self.submitted % self.depth]

    def stream_reference(self):
        self.calls.append("reference")
        return self.ref

    def stream_submit(self):
        self.calls.append("submit")
        slot = self.slots[self.submitted % self.depth]
        self.queue.append((self.submitted, sum(int(p.sum()) for p in slot), int(self.ref[0])))
        self.submitted += 1
        assert len(self.queue) <= self.depth - 1, "more frames in flight than the ring has slots for"
        self.most = max(self.most, len(self.queue))

    def stream_output(self):
        self.calls.append("output")
        self.last = self.queue.pop(0)
        self.taken += 1
        return np.array([self.last[1]]) if self.has_output else None

    def _result(self, name):
        self.calls.append(name)
        return (name, self.last[0], self.last[2])

    def stream_compare_result(self):
        return self._result("compare")

    def stream_ssim_result(self):
        return self._result("ssim")

    def stream_light_result(self):
        return self._result("light")

    def stream_deltae_result(self):
        return self._result("deltae")

    def stream_scenesig_result(self):
        return self._result("scenesig")

    def stream_lightdist_result(self):
        return self._result("lightdist")

    def stream_lightdist_bins(self):
        self.calls.append("lightdist_bins")
        self.dist_bins = np.full(3, self.last[0])
        return self.dist_bins

    def stream_histogram_result(self):
        self.calls.append("histogram")
        self.bins = np.full(2, self.last[0])
        return ("histogram", self.last[0]), self.bins

    def stream_close(self):
        self.closed += 1


def _frames(n):
    """frame k: an array, a callable and an array again, which sum to 100 k + 8"""
    def second(k):
        def fill(dst):
            dst[:] = 2
            dst[0] = 100 * k - 3
        return fill

    return [[np.full(4, 1), second(k), np.array([0, 0, 0, 1])] for k in range(n)]


@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_drive_ring_order_and_frames_in_flight(depth, n):
    ring = FakeRing(depth)
    recs = ht.drive_ring(ring, _frames(n), depth)
    assert [int(r["out"][0]) for r in recs] == [100 * k + 8 for k in range(n)]  # submission order, and every fill applied
    assert all(set(r) == {"out"} for r in recs)
    assert ring.most == min(n, depth - 1)  # never more than depth - 1 in flight, and that many once there are enough frames
    assert ring.submitted == ring.taken == n and ring.closed == 1
    assert "reference" not in ring.calls and not set(ht.RESULTS) & set(ring.calls)
    # an output is taken exactly when depth - 1 are in flight; the rest are drained behind the last submit
    early = max(0, n - (depth - 2))
    want = ["input", "submit"] * min(n, depth - 2) + ["input", "submit", "output"] * early + ["output"] * (n - early)
    assert ring.calls == want


@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_drive_ring_references_and_results(depth, n):
    ring = FakeRing(depth, has_output=False)
    refs = [np.array([7 + k, 0]) for k in range(n)]
    recs = ht.drive_ring(ring, _frames(n), depth, refs=refs, results=("compare", "histogram"))
    assert ring.closed == 1 and len(recs) == n
    for k, r in enumerate(recs):
        assert set(r) == {"out", "compare", "histogram"} and r["out"] is None
        assert r["compare"] == ("compare", k, 7 + k)  # frame k's reference was in place at frame k's submit
        assert r["histogram"][0] == ("histogram", k) and list(r["histogram"][1]) == [k, k]
        assert r["histogram"][1] is not ring.bins  # a copy: the ring's bins are overwritten by the next frame
    assert ring.calls.count("compare") == ring.calls.count("histogram") == n  # once per output, and only what was asked for
    assert "ssim" not in ring.calls and "light" not in ring.calls
    at = [i for i, c in enumerate(ring.calls) if c in ("reference", "submit")]
    assert [ring.calls[i] for i in at] == ["reference", "submit"] * n
    for i, c in enumerate(ring.calls):  # the results follow their output
        if c == "output":
            assert ring.calls[i + 1:i + 3] == ["compare", "histogram"]


@pytest.mark.parametrize("depth", [2, 3, 4])
@pytest.mark.parametrize("n", [1, 2, 5])
def test_drive_ring_every_result(depth, n):
    """all of RESULTS at once, in the caller's order; the light distribution comes with a copy of its bins, as the histogram does"""
    assert set(ht.RESULTS) == {"compare", "ssim", "deltae", "histogram", "light", "lightdist", "scenesig"}
    ring = FakeRing(depth, has_output=False)
    refs = [np.array([7 + k, 0]) for k in range(n)]
    names = ("scenesig", "lightdist", "deltae", "light", "compare", "ssim", "histogram")
    recs = ht.drive_ring(ring, _frames(n), depth, refs=refs, results=names)
    assert ring.closed == 1 and len(recs) == n
    for k, r in enumerate(recs):
        assert set(r) == {"out", *names} and r["out"] is None
        for name in ("scenesig", "deltae", "light", "compare", "ssim"):
            assert r[name] == (name, k, 7 + k)  # frame k's result, and frame k's reference was in place at its submit
        assert r["lightdist"][0] == ("lightdist", k, 7 + k) and list(r["lightdist"][1]) == [k, k, k]
        assert r["lightdist"][1] is not ring.dist_bins  # a copy, whatever the ring does with its own
        assert r["histogram"][0] == ("histogram", k) and list(r["histogram"][1]) == [k, k]
        assert r["histogram"][1] is not ring.bins
    for name in names + ("lightdist_bins",):
        assert ring.calls.count(name) == n, name
    for i, c in enumerate(ring.calls):  # the results follow their output, in the order asked for, the bins with their distribution
        if c == "output":
            assert ring.calls[i + 1:i + 9] == ["scenesig", "lightdist", "lightdist_bins", "deltae", "light", "compare", "ssim", "histogram"]


def test_drive_ring_light_only_ring_results():
    """a light-only ring has no output and no reference: light and the distribution are collected all the same"""
    ring = FakeRing(3, has_output=False)
    recs = ht.drive_ring(ring, _frames(4), 3, results=("light", "lightdist", "scenesig"))
    assert "reference" not in ring.calls
    for k, r in enumerate(recs):
        assert r["out"] is None and r["light"][:2] == ("light", k) and r["scenesig"][:2] == ("scenesig", k)
        assert r["lightdist"][0][:2] == ("lightdist", k) and list(r["lightdist"][1]) == [k] * 3


def test_drive_ring_whole_slot_callable():
    ring, seen = FakeRing(3), []

    def fill(k):
        def into(slots):
            assert len(slots) == PLANES
            seen.append(k)
            for p in slots:
                p[:] = k
        return into

    recs = ht.drive_ring(ring, [fill(k) for k in range(4)], 3, results=["light", "ssim"])
    assert seen == [0, 1, 2, 3] and [int(r["out"][0]) for r in recs] == [12 * k for k in range(4)]
    assert [r["light"][:2] for r in recs] == [("light", k) for k in range(4)]
    assert [r["ssim"][:2] for r in recs] == [("ssim", k) for k in range(4)]


@pytest.mark.parametrize("depth", [2, 3, 4])
def test_drive_ring_closes_when_a_fill_raises(depth):
    ring = FakeRing(depth)

    def bad(dst):
        raise RuntimeError("no such file")

    frames = _frames(3)
    frames[1][2] = bad
    with pytest.raises(RuntimeError, match="no such file"):
        ht.drive_ring(ring, frames, depth)
    assert ring.closed == 1 and ring.submitted == 1


def test_drive_ring_refuses_unknown_results():
    ring = FakeRing(3)
    with pytest.raises(AssertionError):
        ht.drive_ring(ring, _frames(1), 3, results=("psnr",))
    assert ring.calls == []


BANNER = """\
src_filename: /tmp/in file.yuv
WARNING: reference file /tmp/r.yuv holds 1 frames, the run produces 2
dst_matrix_coeffs: 9
gpus: 3 (devices 0 1 2)
ERROR (device 0, frames 0..4): no HIP device (100): this library has no CPU path
compare: yuv 16x8 chroma_format_idc 1 bit_depth 10 planes Y,Cb,Cr, 2 frames against /tmp/r.yuv, sigma 4, output none
frame 0 psnr Y inf
key:no space
note: a: b
"""


def test_banner():
    kv = ht.banner(BANNER)
    assert kv == {
        "src_filename": "/tmp/in file.yuv",
        "dst_matrix_coeffs": "9",
        "gpus": "3 (devices 0 1 2)",
        "compare": "yuv 16x8 chroma_format_idc 1 bit_depth 10 planes Y,Cb,Cr, 2 frames against /tmp/r.yuv, sigma 4, output none",
        "note": "a: b",
    }
    assert ht.banner("") == {}
    assert ht.lines_with(BANNER, ("WARNING", "ERROR")) == [BANNER.splitlines()[1], BANNER.splitlines()[4]]
    assert ht.lines_with(BANNER, "frame ") == ["frame 0 psnr Y inf"]


def test_small_helpers(tmp_path):
    assert ht.plane_sizes(35, 19, 1) == [665, 153, 153] and ht.plane_sizes(35, 19, 3) == [665] * 3
    p = ht.zero_file(tmp_path / "z.yuv", 10)
    assert p == tmp_path / "z.yuv" and p.read_bytes() == bytes(10)
    x = np.arange(0, 1024, 8, dtype=np.uint16)
    y = ht.noisy(x, 10, np.random.default_rng(0), 3)
    assert y.dtype == np.uint16 and y.max() <= 1023 and 0 < np.abs(y.astype(int) - x).max() <= 3
    assert ht.md5(np.zeros(4, np.uint8)) == "f1d3ff8443297732862df21dc4e57262"
