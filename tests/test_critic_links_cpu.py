"""CPU: the float64 link functions of tests/critic_links_ref.py, before the GPU test relies on them.

(a) the site table sites() against what the library chooses, launch by launch, through depgan_debug_conv_choice and
    depgan_debug_wgrad_choice (no device);
(b) the link functions against a float32 run of the same site model (simulate): every link within 1e-5 S -- the
    references and the layout agree with a second evaluation that shares only the primitives -- and at every bf16 site
    the reference with the operand rounding and the one without are at least 5e-4 S apart: the condition under which
    the GPU gate of 1e-4 S also pins WHERE the library rounds."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import critic_links_ref as R  # noqa: E402

from dep_gan_im_amd import _lib  # noqa: E402
from oracle import depgan_oracle as O  # noqa: E402

K = _lib._K
BIAS, RELU, MASK, POOL = (K["DEPGAN_EPF_" + n] for n in ("BIAS", "RELU", "MASK", "POOL"))


def _conv_name(lib, k, B, H, W, ci, co, flags):
    name, out = C.create_string_buffer(64), (C.c_long * 5)()
    assert lib.depgan_debug_conv_choice(0, 1, 1, k, 96, B, H, W, ci, co, flags, 0, 0, name, 64, out) == 0, \
        lib.depgan_last_error()
    return name.value.decode()


def _n16(k, ci, co, base):
    """dg_plan_conv_bf16_n16 (common.h) as build_critics takes it: a 5x5 launch with Cout % 16 == 0, Cin >= 8,
    Cin % 4 == 0 whose plan is on the fp32 matrix pipe"""
    return (k == 5 and co % 16 == 0 and ci >= 8 and ci % 4 == 0 and not base.startswith("igemm_bf16")
            and base != "conv_direct")


@pytest.mark.parametrize("size", [(2, 64, 64), (3, 48, 80), (32, 256, 256)], ids=lambda s: "x".join(map(str, s)))
def test_site_table_is_the_library_s_choice(lib, size):
    B, H0, W0 = size
    got = {(c16, wg): {n: dict(fwd=None, bwd=None, wgrad=None) for n in R.LAYERS} for c16 in (0, 1) for wg in (0, 1)}
    H, W = H0, W0
    for li, (name, k, ci, co, pool) in enumerate(R.DIS_TRUNK):
        f = _conv_name(lib, k, 3 * B, H, W, ci, co, BIAS | RELU | (POOL if pool and ci >= 8 else 0))
        u = _conv_name(lib, k, B, H, W, ci, co, MASK)                              # the u-forward: the same plan
        b = _conv_name(lib, k, 3 * B, H, W, co, ci, 0 if (li > 0 and R.DIS_TRUNK[li - 1][4]) else MASK) if li else "none"
        assert f.startswith("igemm_bf16") == u.startswith("igemm_bf16"), name
        for c16 in (0, 1):
            for wg in (0, 1):
                out = (C.c_long * 4)()
                assert lib.depgan_debug_wgrad_choice(k, 3 * B, H, W, ci, co, wg, 0, out) == 0, lib.depgan_last_error()
                got[(c16, wg)][name] = {"fwd": f.startswith("igemm_bf16") or bool(c16 and _n16(k, ci, co, f)),
                                        "bwd": li > 0 and (b.startswith("igemm_bf16") or bool(c16 and _n16(k, co, ci, b))),
                                        "wgrad": out[0] == 2}
        if pool:
            H, W = H // 2, W // 2
    for (c16, wg), table in got.items():
        assert R.sites(bool(c16), bool(wg)) == table, (c16, wg)
    # the critic16 switch adds exactly four launches (dis_0b forward and u-forward are one column)
    on, off = R.sites(True, True), R.sites(False, True)
    added = sorted((n, c) for n in R.LAYERS for c in ("fwd", "bwd", "wgrad") if on[n][c] != off[n][c])
    assert added == [("dis_0b", "bwd"), ("dis_0b", "fwd"), ("dis_1a", "bwd")] and all(on[n][c] for n, c in added)
    assert not any(R.sites(True, True)["dis_0a"].values())                      # dis_0a: never
    assert not any(v for row in R.sites(True, True, bf16_mfma=False).values() for v in row.values())
    assert all(row["wgrad"] == (n != "dis_0a") for n, row in on.items())
    assert not any(row["wgrad"] for row in R.sites(True, False).values())


def critic_real_fake(which, x, y2, attr):
    y1 = x[..., 0:1]
    return (y2, (y1 + attr).astype(np.float32)) if which == "D_y2" else ((y2 - y1).astype(np.float32), attr)


_cache = {}


def _case(H, W, B, seed):
    """inputs and the generator output of a bf16 context, from the oracle (once per case)"""
    key = (H, W, B, seed)
    if key not in _cache:
        PG, PD1, PD2, x, y2, z, ep = R.case_inputs(H, W, B, seed)
        with O.bf16_activations():
            attr = O.g_predict(O.round_kernels_bf16(PG), x, z, nicg=2).astype(np.float32)
        _cache[key] = (PD1, PD2, x, y2, ep, attr)
    return _cache[key]


CASES = [(64, 64, 2, 57, "D_y2", True), (64, 64, 2, 57, "D_dem", True), (48, 80, 3, 57, "D_y2", True),
         (48, 80, 3, 57, "D_dem", True), (64, 64, 2, 57, "D_y2", False)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-b%d-%s-%s" % (c[0], c[1], c[2], c[4], "c16" if c[5] else "plain"))
def test_links_against_a_float32_run_and_the_roundings_are_visible(case):
    H, W, B, seed, which, c16 = case
    PD1, PD2, x, y2, ep, attr = _case(H, W, B, seed)
    Kd = R.compute_kernels(PD1 if which == "D_y2" else PD2, True)
    real, fake = critic_real_fake(which, x, y2, attr)
    st = R.sites(c16, True)
    t = R.simulate(Kd, real, fake, ep, st, dt=torch.float32)
    worst, sep, n_sites = {}, {}, 0
    for ln in R.critic_links(Kd, t, B):
        site, S, e, e_other, d = R.link_errors(ln, st)
        what = "%s %s %s" % (ln.kind, ln.layer, ln.tag)
        if ln.exact:
            assert np.array_equal(ln.got, ln.ref_f), what
            continue
        assert np.isfinite(e) and e <= 1e-5, (what, e, S)
        worst[ln.kind] = max(worst.get(ln.kind, 0.0), e)
        if site:
            n_sites += 1
            assert ln.ref_q is not ln.ref_f
            sep[ln.kind] = min(sep.get(ln.kind, np.inf), d)
            assert d >= R.SEP, (what, d, S)
    print("links %s: worst float32-run error per kind (units of S) %s" % (case, {k: "%.1e" % v for k, v in worst.items()}))
    print("links %s: smallest |ref_rounded - ref_unrounded| / S per kind over %d bf16 sites %s" % (
        case, n_sites, {k: "%.1e" % v for k, v in sep.items()}))
    # forward (2 passes' links per layer), backward-data (2), u-forward (1), weight gradient (1) of every site
    want = sum(2 * r["fwd"] + 2 * r["bwd"] + r["fwd"] + r["wgrad"] for r in st.values())
    assert n_sites == want and set(sep) == {"forward", "backward-data", "u-forward", "weight-gradient"}
