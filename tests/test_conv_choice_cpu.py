"""CPU: which kernel a convolution takes and with what geometry (dg_conv_prepare, csrc/conv_select.hip) through
depgan_debug_conv_choice.

The rule is restated here -- the plan of a layer (with the 1536-item rule for 8-channel chunks), the family chain, the tile
instantiation by (MF, KS, CK) and its fused-head variant, the persistent caps of igemm_grid, the item / slot thresholds and
per-shape defaults of the weight-stationary 5x5 kernel, the Winograd form and epilogue class -- and held against the export
for every convolution launch of the canonical step (generator trunk forward and backward-data at batch 32 with 1 and 2 input
channels, gen_17 with the fused head, the three transposed convolutions grouped and gathered, both critics at batch 96 and
32) at 256 x 256, and again at 16 x 16 and 32 x 48 with batch 2; in fp32 with and without Winograd, bf16, and split 3 / 6.
With no device the library answers 256 CUs, the MI355X's count: the thresholds here are the GPU's.
"""
import ctypes as C
import os

import pytest

from dep_gan_im_amd import _lib

K = _lib._K
BIAS, AFFINE, FILM, RELU, PRE, RES, MASK, POOL, ACCUM, HEAD = (
    K["DEPGAN_EPF_" + n] for n in ("BIAS", "AFFINE", "FILM", "RELU", "PRE", "RES", "MASK", "POOL", "ACCUM", "HEAD"))
BAR = BIAS | AFFINE | RELU
CUS, LDS_MAX = 256, 160 * 1024
# switches the library reads once per process: the rule below is the default's
READ_ONCE = ("DEPGAN_IGEMM_WP", "DEPGAN_IGEMM_WS5", "DEPGAN_IGEMM_WS5_WAVES", "DEPGAN_WINO_MT", "DEPGAN_EPI_CLASSES",
             "DEPGAN_BF16_N16_VARIANT")
MODES = {"fp32": (0, 0, 1), "fp32-nowino": (0, 0, 0), "bf16": (0, 1, 1), "split3": (3, 0, 1), "split6": (6, 0, 1)}


def cdiv(a, b):
    return -(-a // b)


# ---- plans (dg_conv_plan) ----
def plan_tile(KS, Cin, Cout):
    MF = 32 if Cout % 32 == 0 else 16
    if Cin < 8 or Cin % 4 or Cout < 8 or KS not in (1, 3, 5):
        return dict(family="direct")
    CK = 8 if (MF, KS) == (32, 5) else 32 if (MF, KS) == (32, 1) else 16
    return dict(family="tile", MF=MF, KS=KS, CK=CK, Cin=Cin, Cout=Cout)


def plan(mode, KS, Cin, Cout, N, H, W):
    split, bf16, wino = MODES[mode]
    p = plan_tile(KS, Cin, Cout)
    pipe = p["family"] == "tile" and Cin >= 8 and Cin % 4 == 0
    if split:
        return dict(p, family="split", planes=3 if split == 6 else 2, MF=32, CK=16) if pipe and Cout % 16 == 0 else p
    if bf16:
        return dict(p, family="bf16", MF=32, CK=32) if pipe and Cout % 32 == 0 else p
    if wino and KS == 3 and not (H | W) & 1 and p["family"] == "tile" and Cin % 8 == 0 and Cout % 32 == 0:
        return dict(p, family="wino", CK=8)
    items = N * cdiv(H, 16) * cdiv(W, 16) * cdiv(Cout, 32)
    if p["family"] == "tile" and KS == 3 and p["MF"] == 32 and Cin % 8 == 0 and items >= 1536:
        p["CK"] = 8
    return p


# ---- the launch of each family: (name, workgroups, threads, lds, attribute, work items) or a refusal status ----
def direct(KS, B, H, W, Cin, Cout, flags, groups, runs):
    if flags & (POOL | HEAD) or groups > 1 or runs:
        return 3
    tiles = cdiv(W, 16) * cdiv(H, 16) * B
    if Cin <= 2 and Cout in (16, 32) and KS in (3, 5):
        return "conv_direct", cdiv(W, 16) * cdiv(H, 8 if Cout == 32 else 16) * B, 256, 0, 0, 0
    if Cout == 1 and Cin >= 4 and KS in (3, 5):
        lds = (8 * (32 + KS - 1) * 40 + 8 * KS * 8) * 4
        return "conv_direct", cdiv(W, 32) * cdiv(H, 32) * B, 256, lds, lds, 0
    per_wg = 1 if Cout == 1 else 16 if Cout <= 16 else 32
    lds = (8 * (16 + KS - 1) ** 2 + KS * KS * 8 * per_wg) * 4
    return "conv_direct", tiles * cdiv(Cout, per_wg), 256, lds, lds, 0      # no logical grid: a workgroup per tile


def pipe_lds(KS, taps, rowb, planes=1):
    return max(planes * ((16 + KS - 1) ** 2 + taps * 32) * rowb, 4 * 64 * 36 * 4)


def bf16_pipe(p, B, H, W, Cout, groups):
    KS, taps = p["KS"], {1: 1, 3: 9, 5: 5}[p["KS"]]
    total = cdiv(W, 16) * cdiv(H, 16) * B * cdiv(Cout, 32) * max(groups, 1)
    if p["family"] == "bf16":
        lds = pipe_lds(KS, taps, 80)
        return "igemm_bf16_kernel", total, 256, lds, lds, total
    lds = pipe_lds(KS, taps, 32 if p["planes"] == 3 else 48, p["planes"])
    return "igemm_split_kernel", min(total, CUS * min(2, max(1, LDS_MAX // lds))), 256, lds, lds, total


def wino(lib, B, H, W, Cout, flags, runs):
    head = bool(flags & HEAD)
    if head and (Cout != 32 or flags & POOL or runs):
        return 1
    mt = 2 if head else 1
    total = cdiv(W, 16) * cdiv(H, 8 * mt) * B * (Cout // 32)
    cap = (2 if head else 3) * CUS
    pers = "true" if total > cap else "false"
    ec = lib.depgan_wino_epilogue_class(flags, 1 if head else 3 if runs else 0)
    name = ("wino_conv_head_kernel<%s,%d>" % (pers, ec) if head else "wino_conv_gathered_kernel<1,%s>" % pers if runs
            else "wino_conv_kernel<1,%s,%d>" % (pers, ec))
    return name, min(total, cap), 256, None, None, total        # the LDS of a form is WnCfg's: held by the attribute checks only


def ws5(p, B, H, W, Cin, Cout, flags, groups, runs):
    """None where the weight-stationary kernel is not taken"""
    MF = p["MF"]
    if p["KS"] != 5 or Cout != MF or Cin not in (16, 32) or groups > 1 or runs or flags & HEAD:
        return None
    wave = 1280 if MF == 32 else 2560                   # floats of a wave's halo chunk (8 x 20 pixels x CK) or its transpose
    nw = min((LDS_MAX // 4 - Cin * 25 * MF) // wave, 16, 16 if MF == 32 else 12)
    items, slots = B * cdiv(H, 4) * cdiv(W, 16), CUS * nw
    if items < 2 * slots or (Cin, Cout) == (32, 16) or ((Cin, Cout) == (32, 32) and items < 4 * slots):
        return None
    groups_ = cdiv(B * cdiv(H, 16) * cdiv(W, 16) * 4, nw)
    return ("igemm_ws5_kernel<%d,%d>" % (MF, p["CK"]), min(CUS, groups_), nw * 64, (Cin * 25 * MF + nw * wave) * 4, LDS_MAX,
            groups_)


def tile(p, B, H, W, Cout, flags, groups):
    MF, KS, CK = p["MF"], p["KS"], p["CK"]
    if flags & HEAD and ((MF, KS, CK) != (32, 3, 8) or Cout != 32 or groups > 1 or flags & POOL):
        return 1
    lds = max(((16 + KS - 1) ** 2 + KS * KS * MF) * (CK + 4) * 4, 4 * 64 * (MF + 4) * 4)
    total = cdiv(W, 16) * cdiv(H, 16) * B * cdiv(Cout, MF) * max(groups, 1)
    per_cu = 0 if KS == 1 else min(LDS_MAX // lds, (4 if CK == 8 else 3) if KS == 3 else 2)
    pers = per_cu > 0 and total > CUS * per_cu
    name = ("igemm_conv_head_kernel<%s>" if flags & HEAD else "igemm_conv_kernel<%d,%d,%d,%d,%%s>" % (MF, KS, CK, KS * KS))
    return name % ("true" if pers else "false"), CUS * per_cu if pers else total, 256, lds, lds, total


def rule(lib, mode, KS, planN, B, H, W, Cin, Cout, flags, groups, runs):
    p = plan(mode, KS, Cin, Cout, planN, H, W)
    if p["family"] == "direct":
        return direct(KS, B, H, W, Cin, Cout, flags, groups, runs)
    if runs and Cin % (runs * p["CK"]):
        return 3
    head_ok = ((p["family"] == "tile" and (p["KS"], p["CK"]) == (3, 8)) or p["family"] == "wino") and Cout == 32 and \
        groups <= 1 and not flags & (POOL | ACCUM) and not runs
    if (flags & POOL and ((H | W) & 1 or groups > 1)) or (flags & HEAD and not head_ok):
        return 1
    if p["family"] in ("bf16", "split"):
        return bf16_pipe(p, B, H, W, Cout, groups)
    if p["family"] == "wino":
        return wino(lib, B, H, W, Cout, flags, runs)
    return ws5(p, B, H, W, Cin, Cout, flags, groups, runs) or tile(p, B, H, W, Cout, flags, groups)     # wave-private 3x3: opt-in


# ---- the convolution launches of the canonical step (kTrunk, kDis and the passes of model.hip) ----
TRUNK = [("c", -1, 1), ("f", 1, 1), ("c", 1, 1), ("p",), ("c", 1, 2), ("f", 2, 2), ("c", 2, 2), ("p",), ("c", 2, 3),
         ("f", 3, 3), ("c", 3, 3), ("p",), ("c", 3, 4), ("f", 4, 4), ("c", 4, 4), ("d", 4, 4), ("c", 7, 3), ("f", 3, 3),
         ("c", 3, 3), ("d", 3, 3), ("c", 5, 2), ("f", 2, 2), ("c", 2, 2), ("d", 2, 2), ("c", 3, 1), ("f", 1, 1), ("c", 1, 1)]
DIS = [(5, 1, 16, 0), (5, 16, 16, 1), (5, 16, 32, 0), (5, 32, 32, 1), (3, 32, 64, 0), (3, 64, 64, 1), (3, 64, 128, 0),
       (3, 128, 128, 1), (3, 128, 256, 0), (3, 256, 256, 0), (3, 256, 256, 0)]
BWD_SETS = (RES | MASK, MASK, 0)


def step_launches(B, H, W, fm=32):
    """(KS, planN, B, H, W, Cin, Cout, flags, groups, runs) of every convolution launch, each once"""
    out = set()
    for nicg in (1, 2):
        h, w = H, W
        for i, e in enumerate(TRUNK):
            if e[0] == "p":
                h, w = h // 2, w // 2
                continue
            ci, co = (nicg if e[1] < 0 else e[1] * fm), e[2] * fm
            if e[0] == "d":
                out.add((1, 0, B, h, w, ci, co, BAR, 4, 0))                          # forward: the four taps, grouped
                out.add((1, 0, B, h, w, 4 * co, ci, MASK, 0, 4))                     # backward-data: gathered K
                for acc in (0, ACCUM):
                    out.add((1, 0, B, h, w, co, ci, MASK | acc, 0, 0))               # ... or one launch per tap
                h, w = 2 * h, 2 * w
                continue
            pool = POOL if i + 1 < len(TRUNK) and TRUNK[i + 1][0] == "p" else 0
            fwd = [BAR | FILM | RES, BAR | FILM | RES | PRE] if e[0] == "f" else [BAR | pool]
            if i == len(TRUNK) - 1:
                fwd.append(BAR | HEAD)                                               # gen_17 + gen_segmentation
            for f in fwd:
                out.add((3, 32, B, h, w, ci, co, f, 0, 0))
            if e[1] > 0:
                for f in BWD_SETS:
                    out.add((3, 32, B, h, w, co, ci, f, 0, 0))
    for batch in (3 * B, B):                                                         # [real | fake | mixed], and one of them
        h, w = H, W
        for k, ci, co, pool in DIS:
            out.add((k, 96, batch, h, w, ci, co, BIAS | RELU | (POOL if pool else 0), 0, 0))
            out.add((k, 96, batch, h, w, co, ci, MASK, 0, 0))
            out.add((k, 96, batch, h, w, co, ci, 0, 0, 0))
            if pool:
                h, w = h // 2, w // 2
    return sorted(out)


SIZES = [(32, 256, 256), (2, 16, 16), (2, 32, 48)]


def ask(lib, mode, case):
    name, out = C.create_string_buffer(b"untouched", 64), (C.c_long * 5)(*[-7] * 5)
    KS, planN, *rest = case
    status = lib.depgan_debug_conv_choice(*MODES[mode], KS, planN, *rest, name, 64, out)
    return status, name.value.decode(), list(out)


@pytest.fixture(scope="module")
def answers(lib):
    """every launch of every mode and size, asked once: {(mode, case): (status, name, out)}"""
    assert not [v for v in READ_ONCE if v in os.environ], "this test states the default rule: unset " + ", ".join(READ_ONCE)
    saved = {v: os.environ.pop(v, None) for v in ("DEPGAN_IGEMM_PERSIST", "DEPGAN_IGEMM_CK8")}     # read at every call
    try:
        return {(m, c): ask(lib, m, c) for m in MODES for size in SIZES for c in step_launches(*size)}
    finally:
        os.environ.update({k: v for k, v in saved.items() if v is not None})


@pytest.mark.parametrize("mode", list(MODES))
def test_choice_is_the_rule(lib, answers, mode):
    seen = set()
    for (m, case), (status, name, out) in answers.items():
        if m != mode:
            continue
        want = rule(lib, mode, *case)
        if isinstance(want, int):
            assert (status, name, out) == (want, "untouched", [-7] * 5), (case, lib.depgan_last_error())
            continue
        assert status == 0, (case, lib.depgan_last_error())
        wname, grid, block, lds, attr, total = want
        assert (name, out[0], out[1]) == (wname, grid, block), (case, out)
        if lds is not None:
            assert out[2:4] == [lds, attr], (case, name, out)
        assert out[4] == int(grid < total), (case, out)            # persistent: the workgroups walk more than one item each
        seen.add(name.split("<")[0])
    families = {"fp32": {"wino_conv_kernel", "wino_conv_head_kernel", "igemm_ws5_kernel", "igemm_conv_kernel", "conv_direct"},
                "fp32-nowino": {"igemm_conv_kernel", "igemm_conv_head_kernel", "igemm_ws5_kernel", "conv_direct"},
                "bf16": {"igemm_bf16_kernel", "igemm_ws5_kernel", "igemm_conv_kernel", "conv_direct"},
                "split3": {"igemm_split_kernel", "conv_direct"}, "split6": {"igemm_split_kernel", "conv_direct"}}
    assert seen == families[mode]


def test_the_thresholds_are_crossed_by_the_step(lib, answers):
    """both sides of the 1536-item rule, of the persistent caps and of the 5x5 kernel's defaults occur"""
    names = {(m, c): a[1] for (m, c), a in answers.items() if a[0] == 0}
    got = set(names.values())
    for n in ("igemm_conv_kernel<32,3,8,9,true>", "igemm_conv_kernel<32,3,16,9,true>", "igemm_conv_kernel<32,3,16,9,false>",
              "igemm_conv_kernel<32,5,8,25,true>", "igemm_conv_kernel<16,5,16,25,false>", "igemm_conv_kernel<32,1,32,1,false>",
              "igemm_ws5_kernel<32,8>", "igemm_ws5_kernel<16,16>", "wino_conv_kernel<1,true,1>", "wino_conv_kernel<1,false,1>",
              "wino_conv_head_kernel<true,10>", "igemm_conv_head_kernel<true>"):
        assert n in got, n
    # 32 -> 32 5x5 at 128 x 128: the weight-stationary kernel at batch 96, the tile kernel at batch 32; 32 -> 16 never
    assert names[("fp32", (5, 96, 96, 128, 128, 32, 32, BIAS | RELU | POOL, 0, 0))] == "igemm_ws5_kernel<32,8>"
    assert names[("fp32", (5, 96, 32, 128, 128, 32, 32, BIAS | RELU | POOL, 0, 0))] == "igemm_conv_kernel<32,5,8,25,true>"
    assert names[("fp32", (5, 96, 96, 128, 128, 32, 16, MASK, 0, 0))] == "igemm_conv_kernel<16,5,16,25,true>"


def test_every_kernel_has_one_attribute_that_covers_all_its_launches(answers):
    attr = {}
    for (mode, case), (status, name, out) in answers.items():
        if status:
            continue
        assert 0 <= out[2] <= out[3] <= LDS_MAX and (out[3] > 0 or out[2] == 0), (mode, case, name, out)
        if name != "conv_direct":                               # one name for every direct instantiation
            key = (name, case[0])                               # igemm_bf16_kernel / igemm_split_kernel: one bare name per KS
            assert attr.setdefault(key, out[3]) == out[3], (mode, case, name, out)
    assert attr[("igemm_ws5_kernel<32,8>", 5)] == attr[("igemm_ws5_kernel<16,16>", 5)] == LDS_MAX
    lds = {out[2] for (_, _), (status, name, out) in answers.items() if status == 0 and name == "igemm_ws5_kernel<32,8>"}
    assert len(lds) > 1 and max(lds) <= LDS_MAX                 # launches of one entry differ in size: the attribute is the entry's


def test_winograd_names_are_the_name_entrys(lib, answers):
    buf, n = C.create_string_buffer(64), 0
    for (mode, case), (status, name, out) in answers.items():
        KS, planN, B, H, W, Cin, Cout, flags, groups, runs = case
        if status == 0 and name.startswith("wino_") and not runs:
            assert lib.depgan_op_conv3x3_wino_kernel_name(flags, B, H, W, Cin, Cout, buf, 64) == 0
            assert buf.value.decode() == name, case
            n += 1
    assert n > 50


def test_refusals_write_nothing(lib):
    ok = dict(split=0, bf16=0, wino=1, KS=3, planN=32, B=2, H=16, W=16, Cin=32, Cout=32, flags=BAR, groups=0, runs=0)
    name, out = C.create_string_buffer(b"untouched", 64), (C.c_long * 5)(*[-7] * 5)

    def call(name_=name, cap=64, out_=out, **kw):
        a = dict(ok, **kw)
        return lib.depgan_debug_conv_choice(a["split"], a["bf16"], a["wino"], a["KS"], a["planN"], a["B"], a["H"], a["W"], a["Cin"],
                                            a["Cout"], a["flags"], a["groups"], a["runs"], name_, cap, out_)
    assert call() == 0 and name.value.startswith(b"wino_conv_kernel<1,false,") and out[1] == 256
    name.value, out[:] = b"untouched", [-7] * 5
    refused = [
        (dict(B=0), 1), (dict(H=0), 1), (dict(W=-1), 1), (dict(Cin=0), 1), (dict(Cout=0), 1), (dict(planN=-1), 1),      # sizes
        (dict(split=2), 1), (dict(bf16=2), 1), (dict(wino=-1), 1), (dict(groups=3), 1), (dict(runs=5), 1),              # modes
        (dict(flags=1024), 1), (dict(flags=BAR | 4096), 1),                                                            # flags
        (dict(name_=None), 1), (dict(cap=0), 1), (dict(out_=None), 1),
        (dict(flags=BAR | HEAD, Cout=64), 1), (dict(flags=BAR | HEAD, bf16=1), 1), (dict(flags=BAR | HEAD, split=3), 1),
        (dict(flags=BAR | HEAD, wino=0, planN=0), 1), (dict(flags=BAR | HEAD | POOL), 1),                                # head
        (dict(flags=BAR | POOL, H=15, wino=0), 1),                                                                     # odd pool
        (dict(KS=7), 3), (dict(Cin=1, flags=BAR | POOL), 3), (dict(Cin=1, groups=4), 3), (dict(Cin=32, runs=3), 3),      # uncovered
    ]
    for kw, status in refused:
        assert call(**kw) == status, kw
        assert lib.depgan_last_error(), kw
        assert name.value == b"untouched" and list(out) == [-7] * 5, kw
    assert b"head" in (call(flags=BAR | HEAD, Cout=64) and lib.depgan_last_error())
