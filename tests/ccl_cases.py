"""The volumes the connected-component tests label (tests/test_components_cpu.py, tests/test_gpu_components.py): the
contents on which a union-find goes wrong, for any (D, H, W)."""
import functools

import numpy as np

NEIGHBOURHOODS = [(1, 0), (2, 0), (3, 0), (1, 1), (2, 1)]      # (connectivity, in_plane): 6, 18, 26, 4 and 8 neighbours
SMALL_SHAPES = [(1, 1, 1), (1, 9, 70), (5, 37, 70), (3, 3, 300), (3, 300, 3), (70, 5, 9), (2, 64, 64)]
BLOBS = (3, 256, 256)
CONTENTS = ["empty", "full", "corners", "checker", "diag_plane", "diag_volume", "serpentine", "u", "comb",
            "comb_mirror", "spirals", "slabs", "random_0.01", "random_0.25", "random_0.31", "random_0.5", "random_0.6"]


def spiral(H, W, inset):
    """bool (H, W): a rectangular spiral path one voxel wide with a pitch of 4, wound inwards from (inset, inset).  Two
    of them with insets 0 and 2 interleave and stay two voxels apart."""
    g = np.zeros((H, W), bool)
    top, left, bottom, right = inset, inset, H - 1 - inset, W - 1 - inset
    start = left                                    # the first row of a turn begins where the last column went up
    while top <= bottom and start <= right:
        g[top, start:right + 1] = True              # right along the top
        g[top:bottom + 1, right] = True             # down the right edge
        if bottom - top < 4 or right - left < 4:
            break
        g[bottom, left:right + 1] = True            # left along the bottom
        g[top + 4:bottom + 1, left] = True          # up the left edge, as far as the next turn's first row
        start, top, left, bottom, right = left, top + 4, left + 4, bottom - 4, right - 4
    return g


@functools.lru_cache(maxsize=None)
def volume(shape, name):
    """bool (D, H, W), read-only"""
    rng = np.random.default_rng(sum(shape) + len(name))
    D, H, W = shape
    a = np.zeros(shape, bool)
    zz, yy, xx = np.indices(shape)
    if name == "full":
        a[:] = True
    elif name == "corners":
        a[0, 0, 0] = a[-1, -1, -1] = True
    elif name == "checker":                         # singletons at rank 1, one component at rank 3
        a = (zz + yy + xx) % 2 == 0
    elif name == "diag_plane":                      # a diagonal inside the middle slice
        a = (zz == D // 2) & (yy == xx)
    elif name == "diag_volume":                     # the space diagonal: joined at rank 3 in the volume only
        a = (zz == yy) & (yy == xx)
    elif name == "serpentine":                      # one path through every slice: full rows joined at alternating ends
        a = (yy % 2 == 0) | ((yy % 4 == 1) & (xx == W - 1)) | ((yy % 4 == 3) & (xx == 0))
    elif name == "u":                               # two columns joined along the last row
        a = (xx == 0) | (xx == W - 1) | (yy == H - 1)
    elif name in ("comb", "comb_mirror"):           # teeth joined along the LAST row only: a late merge of every root
        a = (xx % 3 == 0) | (yy == H - 1)
        if name == "comb_mirror":
            a = a[:, :, ::-1]
    elif name == "spirals":                         # two spirals interleaved without touching
        a[:] = spiral(H, W, 0) | spiral(H, W, 2)
    elif name == "slabs":                           # first and last slice, joined by one column of single voxels
        a = (zz == 0) | (zz == D - 1) | ((yy == H // 2) & (xx == W // 2))
    elif name.startswith("random_"):
        a = rng.uniform(size=shape) < float(name[7:])
    elif name.startswith("blobs"):
        for _ in range(40):
            c = rng.uniform(size=3) * shape
            r = rng.uniform(2, 14)
            a |= ((zz - c[0]) * 3.0) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2 < r * r
    elif name != "empty":
        raise KeyError(name)
    a = np.ascontiguousarray(a)
    a.setflags(write=False)
    return a
