"""The case table of tests/test_gpu_wgrad_tiles.py (GPU) and tests/test_wgrad_plan_cpu.py (CPU), and what both need to
read it: a Python restatement of the weight-gradient launchers' chunking, the plan properties a case exists for, the
operands, and a numpy emulation that walks the tiles chunk by chunk as the kernels do.

Every weight-gradient kernel gives a workgroup a contiguous range of pixel tiles (the transposed-convolution kernel: of
k-steps of 4 pixels) whose length the host picks so that a launch is one round of resident workgroups.  A case is in the
table because its PLAN has a property that the smaller operator cases never reach:

  t3   three or more tiles per workgroup: the steady state (prefetch under the MFMAs, counted vmcnt, reuse of LDS
       buffer 0 by the third tile)
  a    a last chunk shorter than the others (t1 = min(t0 + tilesPerChunk, nTiles))
  b    a chunk holding tiles of two samples (the incremental tile / row / sample advance, the sample tag)
  c    three or more tile columns and rows, and one chunk in which a border tile follows an interior one and an interior
       tile a border one
  d    column sums over the samples b < colB with 1 <= colB < B, the boundary inside a chunk
  r3   transposed convolution: 12 or more k-steps per workgroup (three rounds of the ring of 4 fragment stages)
  r2   transposed convolution: exactly 8 k-steps per workgroup (two rounds: the one refill that is multiplied)

On the device the plan comes from depgan_debug_wgrad_plan (the launchers' own functions); plan() below restates them for
a device of CUS compute units so that the table is checked on a machine without one.
"""
import collections

import numpy as np

CUS = 256                                   # MI355X; chunking() of wgrad.hip has the number as a literal
K_F32, K_EDGE, K_BF16, K_BF16S, K_DECONV = range(5)     # `kernel` of depgan_debug_wgrad_plan
DEPTH = 4                                   # deconv_wgrad.hip: fragment stages in flight


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------------------------------
# the launchers' chunking, restated
# ---------------------------------------------------------------------------------------------------------------------
def f32_variant(KS, Cin, Cout):
    """pick_variant of wgrad.hip (default build): MF, TPW, TH of the wgrad_dma_kernel instantiation."""
    MF = 32 if (Cin % 32 == 0 and Cout % 32 == 0) else 16
    TPW, TH = KS * KS, 16
    if KS == 5 and MF == 32:
        TPW, TH = 5, 4
    if KS == 3 and MF == 32:
        TH = 8
    return MF, TPW, TH


def _f32_lds(MF, KS, TPW, TH):
    """WDmaCfg<MF, KS, TPW, TH>::LDS_BYTES"""
    TW, THH, V = 16 + KS - 1, TH + KS - 1, MF // 4
    XTOT, DTOT = THH * TW * V, TH * 16 * V
    BUF = cdiv(XTOT, 256) * 256 * 4 + DTOT * 4
    two = (MF == 32 and KS == 3 and TH == 8) or (MF == 32 and KS == 5 and TH == 4)
    RT = (3 if KS == 3 else 1) if two else TPW
    return max(2 * BUF * 4, RT * 4 * MF * MF * 4)


def edge_is_mfma(KS, Cin, Cout):
    """dg_wgrad_small: wgrad_edge_kernel (MFMA) or wgrad_small_kernel (VALU), for dense or 4-float-strided dy"""
    return KS * KS * Cin <= 32 and Cout in (16, 32)


def tile_h(kernel, KS, Cin, Cout):
    return f32_variant(KS, Cin, Cout)[2] if kernel == K_F32 else 16


def variant(kernel, KS, Cin, Cout):
    """name of the kernel instantiation a case runs"""
    if kernel == K_F32:
        MF, TPW, TH = f32_variant(KS, Cin, Cout)
        return "wgrad_dma_kernel<%d,%d,%d,%d>" % (MF, KS, TPW, TH)
    if kernel == K_EDGE:
        return ("wgrad_edge_kernel<%d>" if edge_is_mfma(KS, Cin, Cout) else "wgrad_small_kernel<%d>") % KS
    if kernel == K_BF16:
        return "wgrad_bf16_kernel<%d>" % KS
    if kernel == K_BF16S:
        return "wgrad_bf16s_kernel<%d>" % KS
    return "deconv_wgrad_kernel<%s>" % {64: "4,4", 96: "6,6", 128: "8,4"}[Cin]


def plan(kernel, KS, B, H, W, Cin, Cout, cus=CUS):
    """(tiles, tiles per workgroup, chunks, gridDim.y) as depgan_debug_wgrad_plan reports them on a device of `cus`
    compute units (kernel 4: k-steps, k-steps per workgroup, workgroups along x, gridDim.y)."""
    if kernel == K_DECONV:
        ny = 2 if Cin == 128 else 1
        total = B * H * W // 4
        n = next(n for n in range(2 * cus // ny, 0, -1) if total % (n * DEPTH) == 0)
        return total, total // n, n, ny
    th = tile_h(kernel, KS, Cin, Cout)
    nT = B * cdiv(W, 16) * cdiv(H, th)
    if kernel == K_EDGE:
        want, gy = min(max(nT // 6, 1024), 8192), 1
    elif kernel == K_F32:
        MF, TPW, TH = f32_variant(KS, Cin, Cout)
        gy = cdiv(Cin, MF) * cdiv(Cout, MF) * (KS * KS // TPW)
        per_cu = 2 if 2 * _f32_lds(MF, KS, TPW, TH) <= 160 * 1024 else 1
        want = 256 * per_cu // gy             # the literal of wgrad.hip, not `cus`
    else:
        gy = cdiv(Cin, 32) * cdiv(Cout, 32)
        want = cus * (1 if KS == 5 else 2) // gy
    want = min(max(want, 1), nT)
    tpc = cdiv(nT, want)
    return nT, tpc, cdiv(nT, tpc), gy


def interior(tile, B, H, W, KS, th):
    """wgrad_dma_kernel's test: the halo tile lies inside the image (no per-piece bounds test while staging)"""
    tX, tY, p = cdiv(W, 16), cdiv(H, th), KS // 2
    tx0, ty0 = (tile % tX) * 16, (tile // tX % tY) * th
    return ty0 >= p and ty0 + th + p <= H and tx0 >= p and tx0 + 16 + p <= W


def properties(kernel, KS, B, H, W, Cin, Cout, colB, pl):
    """The properties the plan `pl` gives the shape.  Exactly what both test files assert for every row."""
    nT, tpc, nch, gy = pl
    if kernel == K_DECONV:
        assert nT == B * H * W // 4 and tpc * nch == nT and tpc % DEPTH == 0
        return {p for p, ok in (("r3", tpc >= 3 * DEPTH), ("r2", tpc == 2 * DEPTH)) if ok}
    th = tile_h(kernel, KS, Cin, Cout)
    tX, tY = cdiv(W, 16), cdiv(H, th)
    tps = tX * tY
    assert nT == B * tps and nch == cdiv(nT, tpc)
    chunks = [range(c * tpc, min((c + 1) * tpc, nT)) for c in range(nch)]
    got = set()
    if tpc >= 3:
        got.add("t3")
    if nch > 1 and len(chunks[-1]) < tpc:
        got.add("a")
    if any(c[0] // tps != c[-1] // tps for c in chunks):
        got.add("b")
    if tX >= 3 and tY >= 3:
        for c in chunks:
            inner = [interior(t, B, H, W, KS, th) for t in c]
            steps = set(zip(inner, inner[1:]))
            if (True, False) in steps and (False, True) in steps:
                got.add("c")
    if 1 <= colB < B and (colB * tps) % tpc != 0:
        got.add("d")
    return got


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
# shape = (B, H, W, Cin, Cout, KS).  The entry follows from the kernel: depgan_op_conv2d_wgrad_ex with bf16 = 0 (kernels 0
# and 1) or 1 (kernel 2), depgan_op_conv2d_wgrad_bf16s (3), depgan_op_deconv2x2_wgrad (4; shape is that of its input).
# colB 0: no column sums; bf16s and deconv have colB = B, their entries know no other form.  scale / raw / acc / oi: the
# extras of depgan_op_conv2d_wgrad_ex (oi also of bf16s); grid: dy is the (gy, gx) strided grid of a (2H, 2W) buffer.
Case = collections.namedtuple("Case", "name kernel shape props colB scale raw acc oi grid")


def _c(name, kernel, shape, props, colB=0, scale=0, raw=0, acc=0, oi=0, grid=None):
    return Case(name, kernel, tuple(shape), frozenset(props.split()), colB, scale, raw, acc, oi, grid)


CASES = [
    # ---- fp32 MFMA kernel: one row per default instantiation
    # 170 tiles of 8 rows (85 per sample), 4 per chunk, 43 chunks, the last one holds 2
    _c("f32-3x3-mf32", K_F32, (2, 133, 70, 96, 96, 3), "t3 a b c d", colB=1, scale=1, raw=1),
    _c("f32-3x3-mf16", K_F32, (5, 100, 39, 72, 44, 3), "t3 a b c d", colB=2, acc=1, oi=1),
    # 90 tiles of 4 rows, 4 per chunk, 23 chunks: the last one holds 2
    _c("f32-5x5-mf32", K_F32, (3, 40, 40, 64, 64, 5), "t3 a b c d", colB=1, scale=1, acc=1),
    _c("f32-5x5-mf16", K_F32, (5, 85, 38, 48, 48, 5), "t3 a b c d", colB=3, raw=1, oi=1),
    _c("f32-1x1-mf32", K_F32, (2, 53, 70, 128, 128, 1), "t3 a b c d", colB=1, scale=1, raw=1, oi=1, grid=(1, 0)),
    # 75 tiles, 8 per chunk, the last one holds 3
    _c("f32-1x1-mf32-tail", K_F32, (3, 70, 67, 160, 160, 1), "t3 a b c", acc=1, grid=(0, 1)),
    _c("f32-1x1-mf16", K_F32, (2, 69, 71, 72, 72, 1), "t3 a b c d", colB=1),
    # ---- bf16 matrix pipe, fp32 staging (KS 1, 3, 5)
    _c("bf16-1x1", K_BF16, (2, 55, 53, 192, 192, 1), "t3 a b c d", colB=1, scale=1, oi=1, grid=(1, 1)),
    _c("bf16-1x1-tail", K_BF16, (3, 71, 66, 152, 136, 1), "t3 a b c d", colB=1, raw=1, acc=1),
    _c("bf16-3x3", K_BF16, (5, 101, 38, 128, 128, 3), "t3 a b c d", colB=2, scale=1, raw=1),
    _c("bf16-5x5", K_BF16, (2, 70, 69, 128, 128, 5), "t3 a b c d", colB=1, acc=1, oi=1),
    # ---- bf16 matrix pipe, bf16 staging (KS 1, 3); its entry sums the columns over all samples
    _c("bf16s-1x1", K_BF16S, (3, 69, 72, 152, 136, 1), "t3 a b c", colB=3, oi=1, grid=(0, 1)),
    # 128 tiles, 3 per chunk, 43 chunks: the last one holds 2
    _c("bf16s-3x3", K_BF16S, (2, 125, 122, 160, 64, 3), "t3 a b", colB=2),
    _c("bf16s-3x3-rows", K_BF16S, (5, 101, 38, 128, 128, 3), "t3 a b c", colB=5, oi=1),
    # ---- edge-layer kernels: 3 tiles per block only past 2048 tiles, 4 past 3072.  With 3 tile columns and 3 tiles per
    # block the blocks never leave a tile row, so c and b meet only at 4 tiles per block.  Their column sums are a
    # streaming pass of their own (dg_colsum): d says that the entry's colB < B form runs next to a multi-tile launch.
    _c("edge-3x3", K_EDGE, (342, 35, 33, 2, 16, 3), "t3 a b c d", colB=171, scale=1, raw=1),
    _c("edge-5x5", K_EDGE, (229, 40, 37, 1, 32, 5), "t3 c", acc=1, oi=1),
    _c("small-3x3", K_EDGE, (229, 37, 40, 1, 6, 3), "t3 c", scale=1),
    _c("small-5x5", K_EDGE, (130, 49, 50, 2, 16, 5), "t3 a b", raw=1),
    # ---- transposed convolution: r3 and r2 for each of the three instantiations
    _c("deconv-64-r3", K_DECONV, (9, 32, 64, 64, 64, 1), "r3", colB=9),
    _c("deconv-64-r2", K_DECONV, (9, 32, 32, 64, 64, 1), "r2", colB=9),
    _c("deconv-96-r3", K_DECONV, (9, 32, 64, 96, 96, 1), "r3", colB=9),
    _c("deconv-96-r2", K_DECONV, (9, 32, 32, 96, 96, 1), "r2", colB=9),
    _c("deconv-128-r3", K_DECONV, (9, 32, 32, 128, 128, 1), "r3", colB=9),
    _c("deconv-128-r2", K_DECONV, (8, 32, 32, 128, 128, 1), "r2", colB=8),
]
BY_NAME = {c.name: c for c in CASES}
TILE_CASES = [c for c in CASES if c.kernel != K_DECONV]
DECONV_CASES = [c for c in CASES if c.kernel == K_DECONV]

# what the table as a whole has to hold (tests/test_wgrad_plan_cpu.py)
TILE_VARIANTS = ["wgrad_dma_kernel<32,3,9,8>", "wgrad_dma_kernel<16,3,9,16>", "wgrad_dma_kernel<32,5,5,4>",
                 "wgrad_dma_kernel<16,5,25,16>", "wgrad_dma_kernel<32,1,1,16>", "wgrad_dma_kernel<16,1,1,16>",
                 "wgrad_bf16_kernel<1>", "wgrad_bf16_kernel<3>", "wgrad_bf16_kernel<5>", "wgrad_bf16s_kernel<1>",
                 "wgrad_bf16s_kernel<3>", "wgrad_edge_kernel<3>", "wgrad_edge_kernel<5>", "wgrad_small_kernel<3>",
                 "wgrad_small_kernel<5>"]
FAMILIES = {"fp32": (K_F32,), "bf16": (K_BF16, K_BF16S), "edge": (K_EDGE,)}


def case_plan_cpu(c):
    B, H, W, ci, co, k = c.shape
    return plan(c.kernel, k, B, H, W, ci, co)


def check_plan(c, pl):
    """The coverage property the row exists for, asserted on a plan (restated, or read from the device)."""
    B, H, W, ci, co, k = c.shape
    got = properties(c.kernel, k, B, H, W, ci, co, c.colB, pl)
    assert c.props <= got, "%s: plan %s gives %s, the row is there for %s" % (c.name, tuple(pl), sorted(got), sorted(c.props))


# ---------------------------------------------------------------------------------------------------------------------
# operands
# ---------------------------------------------------------------------------------------------------------------------
# exact operands: dy of the samples the column sums must ignore is a multiple of BIG, up to 8 BIG (of BIG / 2, / 4, ...
# down to 4 where every partial sum would not stay below SUM_BOUND otherwise)
BIG = 64.0
SUM_BOUND = 2.0 ** 24


def operands(c, kind):
    """x (B, H, W, Cin), dyf (the buffer dy is a view of), dy, for kind 'exact' (small integers, bf16-representable,
    drawn independently per element, so per tile) or 'real' (standard normal).  The samples at index colB and above hold
    large dy values where the case has column sums over fewer samples than B.  Deconv: dy is the (2H, 2W) gradient."""
    B, H, W, ci, co, k = c.shape
    rng = np.random.default_rng([c.kernel, B, H, W, ci, co, k, kind == "exact"])
    ex = kind == "exact"
    gen = (lambda s: rng.integers(-2, 3, s).astype(np.float32)) if ex else (lambda s: rng.standard_normal(s).astype(np.float32))
    x = gen((B, H, W, ci))
    gh, gw = (2 * H, 2 * W) if (c.grid or c.kernel == K_DECONV) else (H, W)
    dyf = gen((B, gh, gw, co))
    view = lambda a: a[:, c.grid[0]::2, c.grid[1]::2] if c.grid else a   # noqa: E731
    if 1 <= c.colB < B and not ex:
        dyf[c.colB:] *= 1e4
    if 1 <= c.colB < B and ex:
        big, m = rng.integers(-8, 9, dyf[c.colB:].shape).astype(np.float32), BIG
        dyf[c.colB:] = big * m
        while sum_bound(x, view(dyf)) >= SUM_BOUND and m > 4:      # the edge kernels' 300k pixels: 8 BIG is too much
            m /= 2
            dyf[c.colB:] = big * m
    return x, dyf, view(dyf)


def sum_bound(x, dy):
    """An upper bound of every partial sum any summation order can form: max |x| times the largest column sum of |dy|."""
    return float(np.abs(x).max()) * float(np.abs(dy).astype(np.float64).sum(axis=(0, 1, 2)).max())


# ---------------------------------------------------------------------------------------------------------------------
# numpy emulation of the tile walk, and its mutants
# ---------------------------------------------------------------------------------------------------------------------
# mutant -> the properties whose cases must see it
MUTANTS_TILE = {"skip_last": {"t3", "a"}, "stale_dy": {"t3"}, "prev_sample_tag": {"d"}, "border_as_interior": {"c"}}
MUTANTS_DECONV = {"last_step_twice": {"r2", "r3"}, "drop_second_round": {"r2", "r3"}}


def _gather(flat, b, y0, x0, nh, nw, H, W, check):
    """(nh, nw, C) pixels from (y0, x0) of sample b out of a dense (B H W, C) array, addressed as the kernels do: one
    linear offset, no wrap at a row's end.  check: pixels outside the image read 0 (the border path); without it
    (the interior path taken for a border tile) they read whatever the address holds."""
    iy, ix = np.arange(y0, y0 + nh)[:, None], np.arange(x0, x0 + nw)[None, :]
    lin = (b * H + iy) * W + ix
    v = flat[lin % flat.shape[0]].astype(np.float32)
    if check:
        v[~((iy >= 0) & (iy < H) & (ix >= 0) & (ix < W))] = 0
    return v


def emulate_tiles(x, dy, k, th, tpc, colB=0, mutant=None):
    """dw (k, k, Cin, Cout) and the column sums over the samples b < colB, tile by tile and chunk by chunk: every tile
    is a halo tile of x and a th x 16 tile of dy, multiplied tap by tap.  Exact operands only (float32 products summed
    in float64).  mutant: one of MUTANTS_TILE."""
    B, H, W, ci = x.shape
    co, p = dy.shape[3], k // 2
    tX, tY = cdiv(W, 16), cdiv(H, th)
    nT = B * tX * tY
    xf, df = x.reshape(-1, ci), np.ascontiguousarray(dy).reshape(-1, co)
    dw, col = np.zeros((k, k, ci, co)), np.zeros(co)
    for t0 in range(0, nT, tpc):
        tiles = list(range(t0, min(t0 + tpc, nT)))
        if mutant == "skip_last":
            tiles = tiles[:-1]
        staged = []
        for i, t in enumerate(tiles):
            b, ty0, tx0 = t // (tX * tY), (t // tX % tY) * th, (t % tX) * 16
            inner = interior(t, B, H, W, k, th)
            check = not inner
            if mutant == "border_as_interior" and i > 0 and staged[-1][3] and not inner:
                check = False
            xs = _gather(xf, b, ty0 - p, tx0 - p, th + 2 * p, 16 + 2 * p, H, W, check)
            ds = _gather(df, b, ty0, tx0, th, 16, H, W, check)
            staged.append((xs, ds, b, inner))
        for i, (xs, ds, b, _) in enumerate(staged):
            if mutant == "stale_dy" and i >= 2:
                ds = staged[i - 2][1]
            tag = staged[i - 1][2] if (mutant == "prev_sample_tag" and i > 0) else b
            if tag < colB:
                col += ds.sum(axis=(0, 1), dtype=np.float64)
            d2 = ds.reshape(-1, co)
            for ty in range(k):
                for tx in range(k):
                    dw[ty, tx] += xs[ty:ty + th, tx:tx + 16].reshape(-1, ci).T @ d2
    return dw, col


def emulate_deconv(x, dout, steps, mutant=None):
    """dw (2, 2, Cout, Cin) and the column sums of dout, walking the k-steps of 4 input pixels chunk by chunk with a ring
    of DEPTH stages: round r of a chunk multiplies its steps 4r .. 4r + 3, the refills past the chunk's end re-read its
    last step and are never multiplied.  mutant: one of MUTANTS_DECONV."""
    B, H, W, ci = x.shape
    co = dout.shape[3]
    total = B * H * W // 4
    mult = np.ones(total)
    for s0 in range(0, total, steps):
        if mutant == "last_step_twice":
            mult[s0 + steps - 1] += 1
        if mutant == "drop_second_round":
            mult[s0 + DEPTH:s0 + 2 * DEPTH] = 0
    m = np.repeat(mult, 4)[:, None]
    xf = x.reshape(-1, ci).astype(np.float64)
    dw, col = np.zeros((2, 2, co, ci)), np.zeros(co)
    for di in range(2):
        for dj in range(2):
            d = dout[:, di::2, dj::2].reshape(-1, co).astype(np.float64) * m
            dw[di, dj] = d.T @ xf
            col += d.sum(axis=0)
    return dw, col


def deconv_ref(x, dout):
    """float64 reference of depgan_op_deconv2x2_wgrad: dw[di][dj][co][ci] and the column sums of dout"""
    B, H, W, ci = x.shape
    co = dout.shape[3]
    xf = x.reshape(-1, ci).astype(np.float64)
    dw = np.stack([np.stack([dout[:, di::2, dj::2].reshape(-1, co).astype(np.float64).T @ xf for dj in range(2)])
                   for di in range(2)])
    return dw, dout.astype(np.float64).sum(axis=(0, 1, 2))
