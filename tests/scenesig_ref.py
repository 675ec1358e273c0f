"""A numpy / Python-int restatement of "scene signature and scene cuts" of include/hdr2yuv_hip.h, for the tests: the per-pixel light is
light_ref.py's and codelight_ref.py's, the bin lightdist_ref.py's; here the signature of a frame, the distance of two signatures,
the cuts, the figures of a scene merged from its frames' figures and bins, the text of h2y_lightdist_json_scenes and the command
line's scene: lines.  Sums are Python ints: no width to overflow."""
import numpy as np

import codelight_ref as cr
import lightdist_ref as ldr

COLS, ROWS = 16, 9
CELLS = COLS * ROWS


def signature_of_m(m, width, height):
    """the signature (a dict: cell, a list of 144 ints; pixels) of a frame from its pixels' m (flat binary32, raster order)"""
    b = ldr.bin_of(np.asarray(m, np.float32).reshape(-1).view(np.uint32)).astype(np.int64)
    assert b.size == width * height
    y, x = np.divmod(np.arange(b.size, dtype=np.int64), width)
    cell = (y * ROWS // height) * COLS + x * COLS // width
    sums = np.zeros(CELLS, np.int64)  # a cell of 2^28 pixels stays below 2^42
    np.add.at(sums, cell, b)
    return dict(cell=[int(v) for v in sums], pixels=int(b.size))


def signature(planes, width, height, sample, src_transfer, src_depth=16, override=None, to_linear_fn=None):
    """the signature of one frame of the forward flow (planes: G, B, R arrays as uploaded); override: (floor, ceiling) lists"""
    import light_ref as lr

    fl, ce = override if override is not None else lr.pic_stats(planes, sample, src_depth)
    return signature_of_m(lr.light_m(planes, fl, ce, src_transfer, to_linear_fn), width, height)


def code_signature(oracle, planes, width, height, chroma, depth, full_range, matrix, form=cr.FIR):
    """the signature of one frame of PQ codes (planes as codelight_ref.stats takes them)"""
    ls = cr.lights(oracle, cr.planes444(oracle, planes, width, height, chroma, depth, form), depth, full_range, matrix)
    return signature_of_m(np.maximum(np.maximum(ls[0], ls[1]), ls[2]), width, height)


def distance(a, b):
    """h2y_scene_distance: S / (512 x pixels) in binary64, S the exact sum of the cells' absolute differences; -1 for zero or
    differing pixels"""
    if not a["pixels"] or a["pixels"] != b["pixels"]:
        return -1.0
    s = sum(abs(x - y) for x, y in zip(a["cell"], b["cell"]))
    return float(s) / (512.0 * float(a["pixels"]))


def cuts(sigs, threshold):
    """h2y_scene_cuts: the scene id of every frame"""
    ids = [0]
    for f in range(1, len(sigs)):
        ids.append(ids[-1] + (distance(sigs[f - 1], sigs[f]) > threshold))
    return ids


def ids_of_cut_list(first_frames, n):
    """the scene ids of n frames from the scenes' first frames (0 optional)"""
    starts = set(first_frames) | {0}
    ids, s = [], -1
    for f in range(n):
        s += f in starts
        ids.append(s)
    return ids


def merge(stats, scene_id):
    """h2y_scene_merge: the scenes (dicts) of frames whose stats dicts carry their bins (lightdist_ref.stats_of_planes)"""
    scenes = []
    for f, (st, s) in enumerate(zip(stats, scene_id)):
        if s == len(scenes):
            scenes.append(dict(first_frame=f, n_frames=0, maxscl_bits=[0, 0, 0], max_bits=0, sum_q=0, pixels=0, below_100=0,
                               bins=[0] * ldr.BINS))
        o = scenes[s]
        o["n_frames"] += 1
        o["maxscl_bits"] = [max(a, b) for a, b in zip(o["maxscl_bits"], st["maxscl_bits"])]
        o["max_bits"] = max(o["max_bits"], st["max_bits"])
        o["sum_q"] += int(st["sum_q"])
        o["pixels"] += int(st["pixels"])
        o["below_100"] += int(st["below_100"])
        o["bins"] = [a + int(b) for a, b in zip(o["bins"], st["bins"])]
    for o in scenes:
        pct, cum, i = [], 0, 0
        for k, c in enumerate(o["bins"]):
            cum += c
            while i < len(ldr.PCT) and cum * 10000 >= ldr.PCT[i] * o["pixels"]:  # the smallest such k
                pct.append(ldr.edge_bits(k))
                i += 1
        o["pct_bits"] = pct
    return scenes


def _entry_head(s):
    """the text of a scene's LuminanceParameters, as every entry of the scene carries it"""
    p, scl = s["pct_bits"], s["maxscl_bits"]
    avg = int(np.rint(((100000.0 * float(s["sum_q"])) * 2.0 ** -32) / float(s["pixels"])))  # float(int): correctly rounded
    values = [ldr.units(p[0]), ldr.units(p[9]), 100 * s["below_100"] // s["pixels"]] + [ldr.units(x) for x in p[3:9]]
    return ('{"LuminanceParameters": {"AverageRGB": %d, "LuminanceDistributions": {"DistributionIndex": [1, 5, 10, 25, 50, 75, 90, '
            '95, 99], "DistributionValues": [%s]}, "MaxScl": [%d, %d, %d]}, "NumberOfWindows": 1, '
            '"TargetedSystemDisplayMaximumLuminance": 400, ' % (avg, ", ".join(str(v) for v in values), ldr.units(scl[2]),
                                                                 ldr.units(scl[0]), ldr.units(scl[1])))


def json_text(scenes, first=0):
    """h2y_lightdist_json_scenes' text for a list of scene dicts"""
    out = ['{"JSONInfo": {"HDR10plusProfile": "A", "Version": "1.0"},\n"SceneInfo": [\n']
    total = sum(s["n_frames"] for s in scenes)
    for i, s in enumerate(scenes):
        head = _entry_head(s)
        for k in range(s["n_frames"]):
            f = s["first_frame"] + k
            out.append('%s"SceneFrameIndex": %d, "SceneId": %d, "SequenceFrameIndex": %d}%s\n' % (head, k, i, first + f,
                                                                                                   "," if f + 1 < total else ""))
    out.append('],\n"SceneInfoSummary": {"SceneFirstFrameIndex": [%s], "SceneFrameNumbers": [%s]},\n'
               '"ToolInfo": {"Tool": "hdr2yuv", "Version": "1.0"}}\n'
               % (", ".join(str(first + s["first_frame"]) for s in scenes), ", ".join(str(s["n_frames"]) for s in scenes)))
    return "".join(out)


def report_lines(scenes, n_frames, sigs=None, threshold=None):
    """the CLI's scene: lines (hdr2yuv.cpp); sigs and threshold: the detected case, with its distance lines"""
    lines = []
    if sigs is not None:
        for k in range(1, len(sigs)):
            d = distance(sigs[k - 1], sigs[k])
            lines.append("scene: frame %d distance %.6f%s" % (k, d, " cut" if d > threshold else ""))
    for i, s in enumerate(scenes):
        scl = s["maxscl_bits"]
        avg = ((10000.0 * float(s["sum_q"])) * 2.0 ** -32) / float(s["pixels"])
        lines.append("scene: %d first %d frames %d maxscl %.4f %.4f %.4f average %.4f percentiles %s below_100 %.4f"
                     % (i, s["first_frame"], s["n_frames"], 10000.0 * ldr._f(scl[2]), 10000.0 * ldr._f(scl[0]), 10000.0 * ldr._f(scl[1]), avg,
                        " ".join("%.4f" % (10000.0 * ldr._f(b)) for b in s["pct_bits"]), 100.0 * float(s["below_100"]) / float(s["pixels"])))
    lines.append("scene: summary scenes %d frames %d" % (len(scenes), n_frames))
    return lines


def qpfile_text(scenes):
    """the text --scene_qpfile writes: one line per scene start"""
    return "".join("%d I\n" % s["first_frame"] for s in scenes)
