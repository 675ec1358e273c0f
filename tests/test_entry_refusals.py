"""The refusals that the shim's entries share, pinned in one table: the code and the literal text of each, and which of two bad
arguments is reported first.  Every refusal comes before any launch, so no row computes anything and no number is measured.

The pair family (compare, SSIM, regions) works on 16x16 10-bit 4:2:0 frames (SSIM needs 8x8 chroma planes), the pass family
(gamut, tone map, LUT, HLG, ICtCp) on 16x4 planes.  The rings are forward rings on 16x16 F32 planes, a compare-only ring and a
light-only ring."""
import ctypes as C

import numpy as np
import pytest

import h2y_testing as ht
import hdr2yuv_amd as h
from hdr2yuv_amd import api

pytestmark = pytest.mark.gpu

EINVAL, EUNSUPPORTED = api.H2Y_EINVAL, api.H2Y_EUNSUPPORTED
F32, F16 = api.SAMPLE_F32, api.SAMPLE_F16
W, HH = 16, 16      # the pair family's frames and the rings'
PW, PH = 16, 4      # the pass family's planes
STARTED = "arm the ring before its first input"
NO_OUTPUT = "no output taken yet: h2y_stream_output first"
BUSY = "a batch is pending or a stream is open"
HALF_IN_PLACE = "frame 0: plane 0 in place: half planes are widened, the float planes need room of their own"
CUBE = "LUT_3D_SIZE 2\n" + "".join(f"{r} {g} {b}\n" for b in (0, 1) for g in (0, 1) for r in (0, 1))


@pytest.fixture(scope="module")
def env():
    """one context for the file (a refusal leaves it as it was; every row closes the ring it opened), the device buffers and the LUT"""
    c = h.Context(0)
    e = type("Env", (), {})()
    e.ctx = c
    e.a, e.b = (ht.dev_zeros(W * HH * 3 // 2 + 8, np.uint16) for _ in range(2))  # eight samples past the frame: a + 4 bytes stays inside
    e.src32 = [ht.dev_zeros(PW * PH + 4, np.float32) for _ in range(3)]
    e.dst32 = [ht.dev_zeros(PW * PH + 4, np.float32) for _ in range(3)]
    e.half = [ht.dev_zeros(PW * PH, np.float16) for _ in range(3)]
    e.lut = api.Lut3d(CUBE)
    e.cd = h.make_codelight_desc(W, HH, 1, 10, 0, 9, 1)
    yield e
    c.stream_close()
    e.lut.close()
    c.close()


def refused(code, text, call):
    with pytest.raises(api.H2YError) as ei:
        call()
    assert (ei.value.code, str(ei.value)) == (code, f"hdr2yuv_hip error {code}: {text}")


def ptr(t, byte_offset=0):
    return int(t.data_ptr()) + byte_offset


# ---- the batch entries of the pair family ---------------------------------------------------------------------------------------

PAIR = {
    "compare": lambda c, a, b, w=W: c.compare_batch(w, HH, 1, 0, a, b),
    "ssim": lambda c, a, b, w=W: c.ssim_batch(w, HH, 1, 10, a, b),
    "regions": lambda c, a, b, w=W: c.regions_batch(w, HH, 1, 4, 1, a, b),
}
PAIR_ROWS = {
    "n_frames": ("n_frames must be >= 1", lambda e: ([], [])),
    "misaligned": ("frame 0: a frame is not 16-byte aligned", lambda e: ([ptr(e.a, 4)], [ptr(e.b)])),
    "null": ("frame 0: a frame is null", lambda e: ([ptr(e.a)], [0])),
    "null_before_misaligned": ("frame 0: a frame is null", lambda e: ([ptr(e.a, 4)], [0])),
}


@pytest.mark.parametrize("row", PAIR_ROWS)
@pytest.mark.parametrize("entry", PAIR)
def test_pair_batch(env, entry, row):
    text, frames = PAIR_ROWS[row]
    refused(EINVAL, text, lambda: PAIR[entry](env.ctx, *frames(env)))


@pytest.mark.parametrize("entry", PAIR)
def test_pair_batch_beside_a_stream(env, entry):
    env.ctx.compare_stream_open(W, HH, 1, 0, 2)
    try:
        refused(EINVAL, BUSY, lambda: PAIR[entry](env.ctx, [ptr(env.a)], [ptr(env.b)]))
    finally:
        env.ctx.stream_close()


@pytest.mark.parametrize("entry", PAIR)
def test_pair_batch_size_before_n_frames(env, entry):
    """two bad arguments: the picture's size is reported before n_frames"""
    refused(EINVAL, "bad picture size", lambda: PAIR[entry](env.ctx, [], [], 0))


# ---- the batch entries of the pass family ---------------------------------------------------------------------------------------

PASS = {
    "gamut": lambda e, s, src, dst: e.ctx.gamut_batch(PW, PH, s, 1, 9, 1, src, dst),
    "tonemap": lambda e, s, src, dst: e.ctx.tonemap_batch(PW, PH, s, 4000, 1000, 0, src, dst),
    "lut3d": lambda e, s, src, dst: e.ctx.lut3d_batch(PW, PH, s, e.lut, 1, 1, 10, 0, 9, src, dst),
    "hlg": lambda e, s, src, dst: e.ctx.hlg_batch(PW, PH, s, 1000, 0, 10, 0, 9, src, dst),
    "ictcp": lambda e, s, src, dst: e.ctx.ictcp_batch(PW, PH, s, 10, 0, src, dst),
}
WIDENS = ("lut3d", "hlg", "ictcp")  # half planes come out as float planes: lut3d in signal mode, as PASS calls it


def planes(e, bad=None, value=None):
    src = [ptr(t) for t in e.src32]
    if bad is not None:
        src[bad] = value(e.src32[bad])
    return [src], [[ptr(t) for t in e.dst32]]


PASS_ROWS = {
    "n_frames": ("n_frames must be >= 1", lambda e: ([], [])),
    "misaligned": ("frame 0: plane 1 is not 16-byte aligned", lambda e: planes(e, 1, lambda t: ptr(t, 4))),
    "null": ("frame 0: plane 1 is null", lambda e: planes(e, 1, lambda t: 0)),
    # two bad planes: the planes are checked in their order, each for null and then for alignment
    "plane_order": ("frame 0: plane 0 is not 16-byte aligned", lambda e: ([[ptr(e.src32[0], 4), 0, ptr(e.src32[2])]], planes(e)[1])),
}


@pytest.mark.parametrize("row", PASS_ROWS)
@pytest.mark.parametrize("entry", PASS)
def test_pass_batch(env, entry, row):
    text, frames = PASS_ROWS[row]
    refused(EINVAL, text, lambda: PASS[entry](env, F32, *frames(env)))


@pytest.mark.parametrize("entry", PASS)
def test_pass_batch_beside_a_stream(env, entry):
    env.ctx.compare_stream_open(W, HH, 1, 0, 2)
    try:
        refused(EINVAL, BUSY, lambda: PASS[entry](env, F32, *planes(env)))
    finally:
        env.ctx.stream_close()


@pytest.mark.parametrize("entry", PASS)
def test_pass_batch_half_in_place(env, entry):
    """the passes that widen half planes refuse them in place; gamut and tone map write halves and take them"""
    src = [[ptr(t) for t in env.half]]
    if entry in WIDENS:
        refused(EINVAL, HALF_IN_PLACE, lambda: PASS[entry](env, F16, src, src))
    else:
        PASS[entry](env, F16, src, src)


# ---- arming a ring after its first input ----------------------------------------------------------------------------------------

def forward(e, depth=2):
    e.ctx.stream_open(h.make_desc(W, HH, dst_transfer=16, stats=[(0, 1)] * 3), depth)


def forward_compared(e):
    forward(e)
    e.ctx.stream_compare(0, 1)


ARM = {  # entry: (the ring it is armed on, the call)
    "compare": (forward, lambda e: e.ctx.stream_compare(0, 1)),
    "ssim": (forward_compared, lambda e: e.ctx.stream_ssim(-1)),
    "regions": (forward_compared, lambda e: e.ctx.stream_regions(4, 1)),
    "deltae": (forward_compared, lambda e: e.ctx.stream_deltae(e.cd, 1.0)),
    "light": (forward, lambda e: e.ctx.stream_light()),
    "lightdist": (forward, lambda e: e.ctx.stream_lightdist()),
    "scenesig": (forward, lambda e: e.ctx.stream_scenesig()),
    "histogram": (forward, lambda e: e.ctx.stream_histogram(0)),
    "histogram_ex": (forward, lambda e: e.ctx.stream_histogram(0, 10, 0, 0)),
    "scale": (forward, lambda e: e.ctx.stream_scale(8, 8, 3)),
    "gamut": (forward, lambda e: e.ctx.stream_gamut(1, 9, 1)),
    "tonemap": (forward, lambda e: e.ctx.stream_tonemap(4000, 1000, 0)),
    "lut3d": (forward, lambda e: e.ctx.stream_lut3d(e.lut, 1, 0)),
    "hlg": (forward, lambda e: e.ctx.stream_hlg(1000, 0)),
    "ictcp": (forward, lambda e: e.ctx.stream_ictcp()),
    "dither": (forward, lambda e: e.ctx.stream_dither(8, 1)),
    "pack": (forward, lambda e: e.ctx.stream_pack(api.PACK_P010)),
    "unpack": (lambda e: e.ctx.compare_stream_open(W, HH, 1, 0, 2), lambda e: e.ctx.stream_unpack(api.PACK_PLANAR8)),
    "unpack_ex": (lambda e: e.ctx.compare_stream_open(W, HH, 1, 0, 2), lambda e: e.ctx.stream_unpack(api.PACK_P010, 10)),
}


@pytest.mark.parametrize("entry", ARM)
def test_arm_after_first_input(env, entry):
    open_ring, arm = ARM[entry]
    open_ring(env)
    try:
        env.ctx.stream_input()
        refused(EINVAL, STARTED, lambda: arm(env))
    finally:
        env.ctx.stream_close()


ARM_ORDER = {  # two refusals at once: (the ring, what is done to it first, the call, the code and text that win)
    "ssim_comparison_before_started": (forward, lambda e: e.ctx.stream_input(), lambda e: e.ctx.stream_ssim(-1), EINVAL,
                                       "the ring is not armed for comparison: h2y_stream_compare first"),
    "ssim_scaling_before_comparison": (forward, lambda e: e.ctx.stream_scale(8, 8, 3), lambda e: e.ctx.stream_ssim(-1), EUNSUPPORTED,
                                       "a ring that scales computes no SSIM: compare the written file instead"),
    "tonemap_ring_kind_before_started": (lambda e: e.ctx.compare_stream_open(W, HH, 1, 0, 2), lambda e: e.ctx.stream_input(),
                                         lambda e: e.ctx.stream_tonemap(4000, 1000, 0), EINVAL, "tone mapping works on the forward rings only"),
    "gamut_armed_before_started": (lambda e: (forward(e), e.ctx.stream_gamut(1, 9, 1)), lambda e: e.ctx.stream_input(),
                                   lambda e: e.ctx.stream_gamut(1, 9, 1), EINVAL, "the ring converts primaries already"),
}


@pytest.mark.parametrize("row", ARM_ORDER)
def test_arm_first_refusal_wins(env, row):
    open_ring, first, arm, code, text = ARM_ORDER[row]
    open_ring(env)
    try:
        first(env)
        refused(code, text, lambda: arm(env))
    finally:
        env.ctx.stream_close()


# ---- a result before the first output -------------------------------------------------------------------------------------------

def armed_forward(e):
    forward(e)
    c = e.ctx
    c.stream_light(), c.stream_lightdist(), c.stream_scenesig()
    c.stream_compare(0, 1), c.stream_ssim(-1), c.stream_regions(4, 1), c.stream_deltae(e.cd, 1.0)
    c.stream_histogram(0)


def light_only(e):
    e.ctx.codelight_stream_open(e.cd, 1, 2)


RESULT = {
    "compare": (armed_forward, lambda c: c.stream_compare_result()),
    "ssim": (armed_forward, lambda c: c.stream_ssim_result()),
    "regions": (armed_forward, lambda c: c.stream_regions_result()),
    "deltae": (armed_forward, lambda c: c.stream_deltae_result()),
    "light": (armed_forward, lambda c: c.stream_light_result()),
    "lightdist": (armed_forward, lambda c: c.stream_lightdist_result()),
    "lightdist_bins": (armed_forward, lambda c: c.stream_lightdist_bins()),
    "scenesig": (armed_forward, lambda c: c.stream_scenesig_result()),
    "histogram": (armed_forward, lambda c: c.stream_histogram_result()),
    "codelight_light": (light_only, lambda c: c.stream_light_result()),
    "codelight_lightdist": (light_only, lambda c: c.stream_lightdist_result()),
    "codelight_lightdist_bins": (light_only, lambda c: c.stream_lightdist_bins()),
}


@pytest.mark.parametrize("entry", RESULT)
def test_result_before_first_output(env, entry):
    open_ring, result = RESULT[entry]
    open_ring(env)
    try:
        refused(EINVAL, NO_OUTPUT, lambda: result(env.ctx))
    finally:
        env.ctx.stream_close()


NOT_ARMED = {  # on an open ring without the stage, and no output taken either: the missing stage is reported
    "compare": "no armed stream open",
    "ssim": "no stream open that computes SSIM",
    "regions": "no stream open that measures flat and busy areas",
    "deltae": "no stream open that computes Delta E",
    "light": "no stream open that measures content light",
    "lightdist": "no stream open that measures the light distribution",
    "lightdist_bins": "no stream open that measures the light distribution",
    "scenesig": "no stream open that measures the scene signature",
    "histogram": "no stream open that counts histograms",
}


@pytest.mark.parametrize("entry", NOT_ARMED)
def test_result_stage_before_output(env, entry):
    forward(env)
    try:
        refused(EINVAL, NOT_ARMED[entry], lambda: RESULT[entry][1](env.ctx))
    finally:
        env.ctx.stream_close()


def test_result_null_argument_first(env):
    """a null result and no ring at all, through the C entry itself: the null argument is reported"""
    lib, ctx = env.ctx.lib, env.ctx
    for name in ("compare", "ssim", "regions", "deltae", "light", "lightdist", "scenesig"):
        entry = getattr(lib, f"h2y_stream_{name}_result")
        assert entry(ctx.h, None) == EINVAL, name
        assert lib.h2y_last_error(ctx.h) == b"null argument", name
    assert lib.h2y_stream_lightdist_bins(ctx.h, None) == EINVAL
    assert lib.h2y_last_error(ctx.h) == b"null argument"
    assert lib.h2y_stream_histogram_result(ctx.h, None, None) == EINVAL
    assert lib.h2y_last_error(ctx.h) == b"null argument"
