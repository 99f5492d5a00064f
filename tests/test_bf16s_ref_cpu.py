"""CPU: what tests/test_gpu_bf16s_exact.py rests on, proved without a GPU.

  * fused_ref.rne_bf16 (integer arithmetic on the bits) is torch's float32 -> bfloat16 conversion, bit for bit;
  * for every exact case of the GPU case table (tests/bf16s_cases.py) the operands the kernels read as bf16 ARE bf16
    values and every stage in front of the store is a multiple of 2^-7 below 2^15 (fused_ref.bounds_hold): no fp32
    operation of the kernel rounds, the value in front of the store is known exactly, and the stored bf16 is its
    round-to-nearest-even -- one bit pattern.  The fused head's sum over the STORED values is exact in float32 in any
    order, the weight gradients and column sums are integers below 2^24;
  * the operands can SEE the bugs the bound-only tests let through: for each mutant of the contract the reference of
    at least one case changes, in a counted number of elements (printed per mutant and case: run with -s);
  * the case table holds every cell of the coverage list.
"""
import functools
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16s_cases as bc  # noqa: E402
import fused_ref as fr  # noqa: E402


def _torch_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_rne_bf16_is_torchs_conversion_bit_for_bit():
    rng = np.random.default_rng(5)
    n = 1 << 20
    # a random 24-bit significand in each of 40 binades (2^-20 .. 2^19), both signs: 1 M values and more
    mant = rng.integers(0, 1 << 23, n).astype(np.uint32)
    expo = (127 - 20 + (np.arange(n) % 40)).astype(np.uint32)
    sign = (rng.integers(0, 2, n).astype(np.uint32)) << 31
    v = (sign | (expo << 23) | mant).view(np.float32)
    assert len(np.unique(np.frexp(np.abs(v))[1])) == 40 and (v < 0).any() and (v > 0).any()
    assert _same_bits(fr.rne_bf16(v), _torch_bf16(v))
    # the same with the low 16 bits forced onto and next to the tie
    for low in (0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF):
        t = ((v.view(np.uint32) & 0xFFFF0000) | low).view(np.float32)
        assert _same_bits(fr.rne_bf16(t), _torch_bf16(t)), hex(low)
    assert (fr.trunc_bf16(v) != fr.rne_bf16(v)).any() and (fr.half_away_bf16(v) == fr.rne_bf16(v)).mean() > 0.99


def test_rne_bf16_hand_table():
    f = lambda bits: np.array(bits, np.uint32).view(np.float32)   # noqa: E731
    table = [  # float32 bits -> bf16 bits (upper half)
        (0x3F808000, 0x3F80),   # 1 + 2^-8: tie between 1.0 (even) and 1.0078125 (odd) -> down, to even
        (0x3F818000, 0x3F82),   # 1.0078125 + 2^-8: tie between odd and even -> up, to even
        (0xBF808000, 0xBF80), (0xBF818000, 0xBF82),          # the same, negative: ties do not depend on the sign
        (0x3F807FFF, 0x3F80), (0x3F808001, 0x3F81),          # next to the tie, either side
        (0x3F817FFF, 0x3F81), (0x3F818001, 0x3F82),
        (0x3FFF8000, 0x4000),   # 1.99609375 + 2^-8: tie at the binade's end, odd neighbour -> up into the next binade (2.0)
        (0x3FFE8000, 0x3FFE),   # 1.98828125 + 2^-8: the tie below it, even neighbour -> stays
        (0x3FFF7FFF, 0x3FFF), (0x3FFF8001, 0x4000),
        (0x00000000, 0x0000), (0x80000000, 0x8000),          # +0, -0 keep their sign
        (0x7F7F0000, 0x7F7F),   # the largest finite bf16
        (0x7F7F7FFF, 0x7F7F),   # just below the tie to infinity
        (0x3F800000, 0x3F80), (0x40490FDB, 0x4049),          # 1.0; pi -> 3.140625
    ]
    src = f([s for s, _ in table])
    want = np.array([w for _, w in table], np.uint32) << 16
    assert np.array_equal(fr.rne_bf16(src).view(np.uint32), want)
    assert _same_bits(fr.rne_bf16(src), _torch_bf16(src))
    # the mutants differ from it exactly where they should
    assert fr.trunc_bf16(f(0x3F818000)).view(np.uint32) == 0x3F810000          # tie: truncation stays below
    assert fr.trunc_bf16(f(0x3F808001)).view(np.uint32) == 0x3F800000          # above the tie: still below
    assert fr.half_away_bf16(f(0x3F808000)).view(np.uint32) == 0x3F810000      # tie with an even lower neighbour: goes up
    assert fr.half_away_bf16(f(0xBF808000)).view(np.uint32) == 0xBF810000      # ... away from zero
    assert fr.half_away_bf16(f(0x3F818000)).view(np.uint32) == 0x3F820000      # agrees with RNE on the other ties
    assert fr.is_bf16(fr.rne_bf16(src)) and fr.is_bf16(fr.MASKS_BF16) and fr.MASKS_BF16[3] > 0
    assert np.array_equal(fr.pack_dec(np.array([1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 1], bool)), [0x01, 0x82])


# ---------------------------------------------------------------------------------------------------------------------
# exactness, case by case
# ---------------------------------------------------------------------------------------------------------------------
ALL_CONV = bc.CONV_CASES + bc.HEAD_CASES + [("film", s + (3,), "train") for s in bc.TRAIN_CASES]


@functools.lru_cache(maxsize=None)
def _conv_ref(case):
    o, pool, head = bc.conv_ops(case, "exact")
    return o, pool, head, fr.reference_bf16s(o)


def _ties(exact):
    """elements of a float32-exact array that sit exactly between two bf16 values / that are not bf16 values"""
    low = np.ascontiguousarray(exact, np.float32).view(np.uint32) & 0xFFFF
    return int((low == 0x8000).sum()), int((low != 0).sum())


def test_exact_operands_are_exact_for_every_conv_head_and_train_case():
    ties_by_feat = {}
    for case in ALL_CONV:
        o, pool, head, r = _conv_ref(case)
        for n in ("x", "w", "res"):               # what the kernel reads as bf16 (the weights: packed to bf16 inside)
            assert fr.is_bf16(getattr(o, n)), (case, n)
        assert fr.bounds_hold(r["stages"]), case
        assert fr.is_bf16(r["out"]) and fr.is_bf16(r["u"])
        t, nr = _ties(r["out_exact"])
        ties_by_feat[case[0]] = ties_by_feat.get(case[0], 0) + t
        print("%-40s %5.1f %% of the outputs round at the store, %4.1f %% are ties" % (
            bc.cid(case), 100.0 * nr / r["out"].size, 100.0 * t / r["out"].size))
        if pool:
            assert not (case[1][1] | case[1][2]) & 1 and "pool" in r
        if o.fmul is not None:
            z = fr.ZERO_FILM_CHANNEL                # the forced zero channel: FiLM value 0, decision 0, out = RNE(res)
            assert not r["dec"][..., z].any() and np.array_equal(r["out"][..., z], o.res[..., z])
            assert r["dec"].any() and (o.fmul[0, :3] == (-1.25, 0.0, 2.0)).all()
        if head:
            # the head over the STORED values: float32 in two orders == float64
            p = (r["out"].astype(np.float32) * o.head_w).astype(np.float32)
            assert np.array_equal(p.astype(np.float64), r["out"].astype(np.float64) * o.head_w)
            seq = np.zeros(p.shape[:-1], np.float32)
            for c in range(32):
                seq = (seq + p[..., c]).astype(np.float32)
            part = [np.zeros(p.shape[:-1], np.float32) for _ in range(4)]
            for q in range(4):                      # the kernel's order: 8 channels per lane, then lanes xor 2, xor 1
                for k in range(8):
                    part[q] = (part[q] + p[..., 8 * q + k]).astype(np.float32)
            tree = ((part[0] + part[2]).astype(np.float32) + (part[1] + part[3]).astype(np.float32)).astype(np.float32)
            s64 = (r["out"].astype(np.float64) * o.head_w).sum(-1)
            assert np.array_equal(seq, s64) and np.array_equal(tree, s64)
            assert np.array_equal((tree + o.head_b[0]).astype(np.float32), r["head"])
            assert np.abs(s64).max() < 2.0 ** 17
    for feat, t in ties_by_feat.items():
        assert t > 100, (feat, t)                   # the rounding rule meets ties in every feature set


def test_exact_operands_are_exact_for_the_remaining_entries():
    for case in bc.DECONV_CASES:
        x, wt, o = bc.deconv_ops(case, "exact")
        assert fr.is_bf16(x) and fr.is_bf16(wt)
        acc = fr.deconv2x2(x, wt)
        assert fr.bounds_hold([acc, fr.affine(acc, o, np.float64)])
    for case in bc.EDGE_CASES:
        x, w, o = bc.edge_ops(case, "exact")
        acc = fr.conv_acc(x, w)
        assert fr.bounds_hold([acc, fr.affine(acc, o, np.float64)])
        assert np.array_equal(fr.affine(acc, o, np.float64), fr.affine(acc, o, np.float32, "mfma"))
    for case in bc.BWD_CASES:
        o = bc.bwd_ops(case, "exact")
        assert fr.is_bf16(o.x) and fr.is_bf16(o.w) and fr.is_bf16(o.mask)
        assert fr.bounds_hold(fr.reference(o)["stages"])
        if o.mask is not None:
            assert set(np.unique(o.mask.view(np.uint32))) == set(fr.MASKS_BF16.view(np.uint32))    # -0.0 and the tiny one included
    for case in bc.BWD_DECONV_CASES:
        dy, wt, r, m = bc.bwd_deconv_ops(case, "exact")
        assert fr.is_bf16(dy) and fr.is_bf16(wt) and fr.is_bf16(m)
        g = fr.deconv2x2_bwd_data(dy, wt)
        assert fr.bounds_hold([g, g + (0 if r is None else r)])
    for case in bc.WGRAD_CASES:
        x, dyf, dy = bc.wgrad_ops(case, "exact")
        assert fr.is_bf16(x) and fr.is_bf16(dy)
        g = fr.wgrad(x, dy, case[5])
        col = dy.astype(np.float64).sum(axis=(0, 1, 2))
        assert np.abs(g).max() < 2 ** 24 and np.abs(col).max() < 2 ** 24
        assert np.array_equal(g, np.round(g)) and np.array_equal(col, np.round(col))
    for case in bc.UNPOOL_CASES:
        dpool, a, sk = bc.unpool_ops(case)
        assert fr.is_bf16(a)
        assert fr.bounds_hold([fr.unpool_mask(dpool, a, sk)])


# ---------------------------------------------------------------------------------------------------------------------
# sensitivity: each mutant of the contract changes the reference of some case
# ---------------------------------------------------------------------------------------------------------------------
def _chain(o, r, mutant=None):
    """the epilogue after out_pre in float64 (exact on these operands), with one deliberate mistake"""
    b4 = lambda a: a.astype(np.float64)[:, None, None, :]   # noqa: E731
    v = r["out_pre"]
    res = 0.0 if o.res is None else o.res.astype(np.float64)
    film = None
    if mutant == "res_before_film":
        v = v + res
    if o.fmul is not None:
        fm, fa = b4(o.fmul), b4(o.fadd)
        if mutant == "film_row_of_sample_b_minus_1":
            fm, fa = np.roll(fm, 1, axis=0), np.roll(fa, 1, axis=0)
        v = film = v * fm + fa
    if mutant == "relu_after_res":
        v = np.maximum(v + res, 0) if o.relu else v + res
    else:
        if o.relu:
            v = np.maximum(v, 0)
        if mutant != "res_before_film":
            v = v + res
    assert np.array_equal(v.astype(np.float32).astype(np.float64), v)
    return fr.rne_bf16(v.astype(np.float32)), film


def _report(name, rows):
    """rows: (case id, differing elements, elements).  Prints them; at least one case must differ."""
    for c, d, n in rows:
        print("mutant %-32s %-44s %7d of %7d elements differ" % (name, c, d, n))
    assert rows and max(d for _, d, _ in rows) > 0, name
    caught = {}
    for c, d, _ in rows:                       # per feature set (the first word of the case id): some case catches it
        caught[c.split("-")[0]] = caught.get(c.split("-")[0], 0) + d
    assert all(caught.values()), (name, caught)
    return sum(d > 0 for _, d, _ in rows)


def test_sensitivity_of_the_store_and_the_epilogue_order():
    for name, rnd in (("truncation_at_the_store", fr.trunc_bf16), ("half_away_at_the_store", fr.half_away_bf16)):
        rows = []
        for case in ALL_CONV:
            o, pool, head, r = _conv_ref(case)
            m = fr.reference_bf16s(o, rnd)["out"]
            rows.append((bc.cid(case), int((m != r["out"]).sum()), m.size))
        # every feature set has cases with values that round, and ties; bias alone at Cin 48, 1x1 has neither (its
        # outputs are small multiples of 1/8: bf16 values) and is there for the addressing
        assert _report(name, rows) >= len(rows) - 1
    for name, needs in (("relu_after_res", "res"), ("res_before_film", "fmul"), ("film_row_of_sample_b_minus_1", "fmul")):
        rows = []
        for case in ALL_CONV:
            o, pool, head, r = _conv_ref(case)
            if getattr(o, needs) is None or (name == "film_row_of_sample_b_minus_1" and o.x.shape[0] == 1):
                continue
            m, _ = _chain(o, r, name)
            assert np.array_equal(_chain(o, r)[0], r["out"])      # the unmutated chain is the reference
            rows.append((bc.cid(case), int((m != r["out"]).sum()), m.size))
        assert _report(name, rows) == len(rows)


def test_pooling_before_the_rounding_cannot_be_told_apart():
    """RNE is monotone (a <= b implies rne(a) <= rne(b)), so rne(max(a, b, c, d)) == max(rne(a), ..., rne(d)): a kernel
    that pools the unrounded values and rounds the maximum stores the same bits.  Asserted, not assumed -- and the
    truncating and half-away stores are monotone too, so for them the same holds; what the pool test can see is a pool
    of OTHER values (the pre-residual ones, below)."""
    n = 0
    for case in ALL_CONV:
        o, pool, head, r = _conv_ref(case)
        if not pool:
            continue
        early = fr.rne_bf16(fr.pool2(r["out_exact"]).astype(np.float32))
        assert np.array_equal(early, r["pool"]), case
        if o.res is not None:      # distinguishable: the maximum taken before the residual is added
            pre_res = fr.pool2(fr.rne_bf16((r["out_exact"] - o.res).astype(np.float32)))
            d = int((pre_res != r["pool"]).sum())
            print("mutant %-32s %-44s %7d of %7d elements differ" % ("pool_before_the_residual", bc.cid(case), d, early.size))
            assert d > 0
        n += 1
    assert n >= 4


def test_sensitivity_of_the_training_outputs():
    rows_dec, rows_u = [], []
    for shape in bc.TRAIN_CASES:
        case = ("film", shape + (3,), "train")
        o, _, _, r = _conv_ref(case)
        _, film = _chain(o, r)
        dec_after_relu = np.maximum(film, 0) >= 0
        rows_dec.append((bc.cid(case), int((fr.pack_dec(dec_after_relu) != r["dec_bits"]).sum()), r["dec_bits"].size))
        u_after_film = fr.rne_bf16(film.astype(np.float32))
        rows_u.append((bc.cid(case), int((u_after_film != r["u"]).sum()), r["u"].size))
        assert np.array_equal(np.unpackbits(r["dec_bits"], bitorder="little").reshape(r["dec"].shape), r["dec"])
    assert _report("decision_after_the_relu (>= 0)", rows_dec) == len(rows_dec)
    assert _report("u_stored_after_film", rows_u) == len(rows_u)


def test_sensitivity_of_unpool_and_weight_gradient():
    rows = []
    for case in bc.UNPOOL_CASES:
        dpool, a, sk = bc.unpool_ops(case)
        ref, last = fr.unpool_mask(dpool, a, sk), fr.unpool_mask(dpool, a, sk, last=True)
        rows.append((bc.cid(case), int((ref != last).sum()), ref.size))
    assert _report("argmax_takes_the_last_maximum", rows) == len(rows)
    rows = []
    for case in bc.WGRAD_CASES:
        if not case[6]:
            continue
        x, dyf, dy = bc.wgrad_ops(case, "exact")
        g = fr.wgrad(x, dy, case[5])
        oi = np.ascontiguousarray(g.transpose(0, 1, 3, 2))
        rows.append((bc.cid(case), int((oi.ravel() != g.ravel()).sum()), g.size))
    assert _report("weight_gradient_in_IO_order_where_OI_was_asked", rows) == len(rows)


# ---------------------------------------------------------------------------------------------------------------------
def test_the_case_table_covers_the_coverage_list():
    cv = bc.COVERAGE
    conv = {(f, s) for f, s, v in bc.CONV_CASES}
    for f in cv["conv_feats"]:
        assert any(c[0] == f for c in conv), f
    for s in cv["conv_shapes"]:
        assert any(c[1] == s for c in conv), s
    for f, s, v in bc.CONV_CASES:
        if "pool" in f:
            assert not (s[1] | s[2]) & 1, (f, s)
        if v:                                       # the sB = 0 cases run with per-sample FiLM rows
            assert "film" in f and s[0] > 1
    # at least 8 pixel tiles in a count that is no multiple of 8, also with the pool
    for f in ("bias", "film", "film_pool"):
        assert any(c[0] == f and (-(-c[1][1] // 16) * -(-c[1][2] // 16) * c[1][0]) % 8 and
                   -(-c[1][1] // 16) * -(-c[1][2] // 16) * c[1][0] >= 8 for c in conv), f
    tiles = lambda s: -(-s[1] // 16) * -(-s[2] // 16) * s[0]   # noqa: E731
    assert any(tiles(s) % 8 == 0 for _, s in conv) and any(tiles(s) == 2 for _, s in conv)      # both item orders, one tile per sample
    assert {v for _, _, v in bc.CONV_CASES if v} == set(cv["conv_views"])
    for f in cv["head_feats"]:
        for s in cv["head_shapes"]:
            assert (f, s, "") in bc.HEAD_CASES, (f, s)
    assert any(bc.FEATS[f].get("film") and bc.FEATS[f].get("res") for f, _, _ in bc.HEAD_CASES)
    assert bc.TRAIN_CASES == cv["train_shapes"] and bc.DECONV_CASES == cv["deconv_shapes"]
    assert {(c[3], c[4]) for c in bc.EDGE_CASES} == {(i, o) for i in cv["edge_cin"] for o in cv["edge_cout"]}
    for sz in cv["edge_sizes"]:
        assert {(c[3], c[4]) for c in bc.EDGE_CASES if c[:3] == sz} == {(i, o) for i in cv["edge_cin"] for o in cv["edge_cout"]}
    for s in cv["bwd_shapes"]:
        assert {c[5:] for c in bc.BWD_CASES if c[:5] == s} == {(0, 0), (0, 1), (1, 0), (1, 1)}, s
    assert {c[:5] for c in bc.BWD_DECONV_CASES} == set(cv["bwd_deconv_shapes"])
    for s in cv["wgrad_shapes"]:
        assert {c[8] for c in bc.WGRAD_CASES if c[:6] == s} == {0, 1}, s
    assert any(c[7] is not None and c[6] == 1 for c in bc.WGRAD_CASES)      # the transposed-convolution form
    for s in cv["unpool_shapes"]:
        assert {c[4] for c in bc.UNPOOL_CASES if c[:4] == s} == {0, 1}, s
    assert bc.REFUSALS == cv["refusals"]
    # every refusal and every case list has its test in the GPU file
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_bf16s_exact.py")).read()
    for name in cv["refusals"]:
        assert "def _refuse_%s(" % name in src, name
    for table in ("CONV_CASES", "HEAD_CASES", "TRAIN_CASES", "DECONV_CASES", "EDGE_CASES", "BWD_CASES",
                  "BWD_DECONV_CASES", "WGRAD_CASES", "UNPOOL_CASES", "REFUSALS"):
        assert "bc." + table in src, table
