"""Case table of tests/test_gpu_deconv_tiles.py: the fused forward transposed-convolution kernel (csrc/deconv_fwd.hip) PAST
ONE TILE PER WORKGROUP.  Pure Python, no device: tests/test_deconv_tiles_cpu.py checks the builder for several grids.

The kernel is persistent: workgroup x walks the 32-pixel tiles x, x + gridDim.x, ...; its first tile runs the plain body,
every later one the scheduled body that stores the previous tile inside the MFMA stream and stages the next one into the
other half of the double buffer.  What a launch exercises is therefore a function of tiles and gridDim.x alone, and
gridDim.x = min(CUs * workgroups per CU / gridDim.y, tiles) belongs to the device.  So the table holds SHAPES (ROWS) and
the batch of every launch is computed from the device's own numbers (depgan_debug_deconv_fwd_plan): batches() below.
"""
import math
from collections import namedtuple

Row = namedtuple("Row", "name Cin Cout H W")
MT = {64: 2, 96: 3, 128: 2}            # 32-channel tiles per wave (deconv_fwd.hip mt_for)

# Two tiles per sample everywhere but the last of the first block, so that every even tile count is a whole batch:
#   W = 32 (WIDE: a tile lies inside a row; H = 2 so that the row index changes from tile to tile),
#   W = 16 (narrow: a tile spans two rows, its four 8-pixel passes take pass_base one by one),
#   H W = 16 (narrow: a tile spans two samples).
ROWS = [Row("c%d_%s" % (c, "wide" if w == 32 else "narrow"), c, c, h, w) for c in (64, 96, 128) for h, w in ((2, 32), (4, 16))]
ROWS += [Row("c64_two_samples_per_tile", 64, 64, 2, 8)]
# Cin != Cout and gridDim.y > 1: the `% Cout` of the folded bias and of the weight scale, a tap change inside a wave's tiles
ROWS += [Row("c64_to_128_wide", 64, 128, 2, 32), Row("c64_to_192_narrow", 64, 192, 4, 16),
         Row("c96_to_192_wide", 96, 192, 2, 32), Row("c128_to_64_narrow", 128, 64, 4, 16)]
LAUNCHES = ("one_extra", "two_each", "uneven")
BIG_B = 16384                          # the plan of this batch has more tiles than any grid: gridDim.x uncapped


def grid_y(r):
    return 4 * r.Cout // (128 * MT[r.Cin])


def instantiation(r):
    """(Cin, WIDE): the six kernel instantiations"""
    return (r.Cin, r.W >= 32)


def batch_step(H, W):
    """batches are multiples of this: B H W % 32 == 0"""
    return 32 // math.gcd(H * W, 32)


def tiles_of(B, H, W):
    assert (B * H * W) % 32 == 0
    return B * H * W // 32


def _smallest(H, W, ok):
    step = batch_step(H, W)
    B = step
    while not ok(tiles_of(B, H, W)):
        B += step
    return B


def batches(gx, gy, H, W):
    """The three launch sizes of a row on a device whose uncapped grid is (gx, gy): the smallest batch with
      one_extra  tiles >= gx + 1: tiles - gx workgroups run the scheduled body once, the others not at all
      two_each   tiles >= 2 gx:   every workgroup runs it (exactly 2 gx wherever 2 gx tiles are whole samples)
      uneven     tiles >= 3 gx + 1 and tiles % gx != 0: the first staging buffer is written a second time, and some
                 workgroups make one trip more than the others
    gy does not enter: it is part of the signature because the grid is (gx, gy) and the caller has both."""
    assert gx >= 2 and gy >= 1
    return {"one_extra": _smallest(H, W, lambda t: t >= gx + 1),
            "two_each": _smallest(H, W, lambda t: t >= 2 * gx),
            "uneven": _smallest(H, W, lambda t: t >= 3 * gx + 1 and t % gx != 0)}


def trips(tiles, gx):
    """(fewest, most) tiles a workgroup of the launch walks"""
    g = min(gx, tiles)
    return tiles // g, -(-tiles // g)


def sub_batch(gx, H, W):
    """the largest batch whose launch gives every workgroup one tile (tiles <= gx)"""
    step = batch_step(H, W)
    B = (gx * 32 // (H * W)) // step * step
    assert B >= step, "one tile per workgroup needs a grid of at least one sample group"
    return B


def coverage(launches):
    """launches: iterable of (row, tiles, gx, gy, sliced).  The properties the file exists for, as a dict of sets /
    flags that test_case_table_reaches_every_loop_form asserts on the DEVICE's numbers."""
    two, three, uneven, ys, outs, small = set(), set(), set(), set(), set(), False
    for r, tiles, gx, gy, sliced in launches:
        lo, hi = trips(tiles, gx)
        if hi == 2 or lo == 2:
            two.add(instantiation(r))
        if hi >= 3:
            three.add(instantiation(r))
            outs.add((instantiation(r), bool(sliced)))
            if lo != hi:
                uneven.add(instantiation(r))
        ys.add(gy)
        small |= r.H * r.W < 32 and hi >= 2
    return {"two": two, "three": three, "uneven": uneven, "grid_y": ys, "three_by_output": outs, "small_image": small}


ALL_SIX = {(c, w) for c in (64, 96, 128) for w in (False, True)}


def check_coverage(cov):
    assert cov["two"] == ALL_SIX, cov["two"]
    assert cov["three"] == ALL_SIX, cov["three"]
    assert cov["uneven"] == ALL_SIX, cov["uneven"]
    assert cov["three_by_output"] == {(i, s) for i in ALL_SIX for s in (False, True)}
    assert cov["grid_y"] >= {1, 2, 3}, cov["grid_y"]
    assert cov["small_image"]
