"""A small .cube writer for the tests of the 3D LUT: the text h2y_lut3d_parse reads.  A node is written with nine significant digits,
which is enough for the parser to read back the same binary32 value."""
import numpy as np


def _num(v):
    return "%.9g" % float(np.float32(v))


def write_cube(nodes, lo=None, hi=None, title=None, *, eol="\n", sep=" ", comments=True, input_range=None, size_first=False):
    """The text of a .cube file.  nodes: float32 (n, n, n, 3), indexed [b][g][r][channel r, g, b] -- the file's order, r fastest.
    lo / hi: DOMAIN_MIN / DOMAIN_MAX triples (left out when None); input_range: Resolve's LUT_3D_INPUT_RANGE pair instead."""
    nodes = np.asarray(nodes, np.float32)
    n = nodes.shape[0]
    assert nodes.shape == (n, n, n, 3)
    head = []
    if comments:
        head += ["# a test table", ""]
    if size_first:
        head.append(f"LUT_3D_SIZE{sep}{n}")
    if title is not None:
        head.append(f'TITLE{sep}"{title}"')
    if lo is not None:
        head.append("DOMAIN_MIN" + sep + sep.join(_num(v) for v in lo))
    if hi is not None:
        head.append("DOMAIN_MAX" + sep + sep.join(_num(v) for v in hi))
    if input_range is not None:
        head.append("LUT_3D_INPUT_RANGE" + sep + sep.join(_num(v) for v in input_range))
    if not size_first:
        head.append(f"LUT_3D_SIZE{sep}{n}")
    if comments:
        head += ["", "# the nodes"]
    rows = [sep.join("%.9g" % v for v in row) for row in nodes.reshape(-1, 3).astype(np.float64)]
    return eol.join(head + rows) + eol


def random_nodes(rng, n, lo=-0.5, hi=1.5):
    """a random table with values in [lo, hi]"""
    return rng.uniform(lo, hi, (n, n, n, 3)).astype(np.float32)


def identity_nodes(n, lo=(0, 0, 0), hi=(1, 1, 1)):
    """the table that returns its input (up to rounding): node (r, g, b) holds its own position in the domain"""
    ax = [np.linspace(lo[c], hi[c], n) for c in range(3)]
    b, g, r = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([r, g, b], axis=-1).astype(np.float32)
