"""GPU: depgan_op_softmax_ce_census, the softmax + cross-entropy kernel with the class census on, at operator level.

Every check is exact.  The census moves integers only: its table is compared with a NumPy count of the arg-max of the
probabilities the same call returned, and probs, dz and the loss sum are compared bit for bit with depgan_op_softmax_ce
on the same inputs.  P = 1 is one thread, 255 a ragged block, 3219 a ragged grid of 13 blocks, 262181 is 37 pixels past
the 1024-block cap where the grid-stride loop takes over."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CLASSES = [2, 3, 4, 5, 8]
PIXELS = [1, 255, 3219, 262181]


def P_(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _u32(t):
    return np.ascontiguousarray(t.cpu().numpy(), np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(Cc, P):
    """(logits (P, Cc) float32, codes (P,) uint8, tie rows, the lower tied position per tie row).  Row r mod 7: 1 = the
    maximum tied between two positions (every pair of positions in turn, both written as the same float), 2 = all
    entries equal, 3 = a spread of +-100, else standard normal.  One class is rare (about 1 % of the pixels)."""
    rng = np.random.default_rng(1000 * Cc + P % 997)
    z = rng.standard_normal((P, Cc)).astype(np.float32)
    r = np.arange(P)
    pairs = [(a, b) for a in range(Cc) for b in range(a + 1, Cc)]
    tie = r[r % 7 == 1]
    lo = np.array([pairs[i % len(pairs)][0] for i in range(len(tie))], np.int64)
    hi = np.array([pairs[i % len(pairs)][1] for i in range(len(tie))], np.int64)
    top = (z[tie].max(-1) + np.float32(0.75)).astype(np.float32)
    z[tie, lo] = top
    z[tie, hi] = top
    z[r % 7 == 2] = np.float32(0.3125)
    z[r % 7 == 3] *= np.float32(100.0)
    share = np.full(Cc, 0.99 / (Cc - 1))
    share[Cc - 1] = 0.01
    codes = rng.choice(Cc, size=P, p=share).astype(np.uint8)
    return z, codes, tie, lo


def _run(lib, entry, z, onehot, codes, Cc, census=None):
    """One call of depgan_op_softmax_ce (census None) or depgan_op_softmax_ce_census into fresh NaN-filled outputs."""
    P = len(z)
    zd = torch.from_numpy(z).cuda()
    od = torch.from_numpy(onehot).cuda() if onehot is not None else None
    cd = torch.from_numpy(codes).cuda() if codes is not None else None
    probs = torch.full((P, Cc), float("nan"), device="cuda:0")
    dz = torch.full((P, Cc), float("nan"), device="cuda:0")
    loss = torch.full((1,), float("nan"), device="cuda:0")
    if census is None:
        rc = lib.depgan_op_softmax_ce(P_(zd), P_(od), P_(cd), P_(probs), P_(dz), P_(loss), P, Cc, None)
    else:
        rc = lib.depgan_op_softmax_ce_census(P_(zd), P_(od), P_(cd), P_(probs), P_(dz), P_(loss), census, P, Cc, None)
    torch.cuda.synchronize()
    return rc, probs, dz, loss


def _table(census, Cc):
    return np.array(census[:Cc * Cc], np.int64).reshape(Cc, Cc)


def _numpy_table(codes, probs, Cc):
    keep = codes < Cc
    cm = np.zeros((Cc, Cc), np.int64)
    np.add.at(cm, (codes[keep].astype(np.int64), np.argmax(probs[keep], -1)), 1)
    return cm


@pytest.mark.parametrize("P", PIXELS)
@pytest.mark.parametrize("Cc", CLASSES)
def test_census_table_and_unchanged_floats(lib, Cc, P):
    z, codes, tie, lo = _case(Cc, P)
    onehot = np.eye(Cc, dtype=np.float32)[codes]
    cen = (C.c_longlong * 64)(*([-7] * 64))
    rc, probs, dz, loss = _run(lib, "census", z, None, codes, Cc, cen)
    assert rc == 0, lib.depgan_last_error()
    got = _table(cen, Cc)
    pn = probs.cpu().numpy()
    # the table is the NumPy count of the arg-max of what probs received
    assert np.array_equal(got, _numpy_table(codes, pn, Cc)), (got, _numpy_table(codes, pn, Cc))
    assert int(got.sum()) == P
    assert list(cen[Cc * Cc:]) == [-7] * (64 - Cc * Cc)                  # nothing is written past C*C entries
    # the tie rows kept their tie through the softmax, so their prediction is the lower index
    if len(tie):
        hi_val = pn[tie].max(-1)
        assert np.array_equal(pn[tie, lo], hi_val) and np.array_equal(np.argmax(pn[tie], -1), lo)
        assert ((pn[tie] == hi_val[:, None]).sum(-1) >= 2).all()
    # probs, dz and the loss sum are those of the entry without the census, for both label kinds
    for oh, cd in ((None, codes), (onehot, None)):
        rc0, p0, d0, l0 = _run(lib, "plain", z, oh, cd, Cc)
        assert rc0 == 0, lib.depgan_last_error()
        cen2 = (C.c_longlong * 64)(*([-7] * 64))
        rc1, p1, d1, l1 = _run(lib, "census", z, oh, cd, Cc, cen2)
        assert rc1 == 0, lib.depgan_last_error()
        assert np.array_equal(_u32(p0), _u32(p1)) and np.array_equal(_u32(d0), _u32(d1))
        assert np.array_equal(_u32(l0), _u32(l1)) and np.isfinite(l1.cpu().numpy()).all()
        # the one-hot call counts what the codes call counts
        assert np.array_equal(_table(cen2, Cc), got)
    assert np.array_equal(_u32(p1), _u32(probs)) and np.array_equal(_u32(d1), _u32(dz))


@pytest.mark.parametrize("P", [3219, 262181])
@pytest.mark.parametrize("Cc", [3, 8])
def test_out_of_range_codes_are_in_no_bin(lib, Cc, P):
    z, codes, _, _ = _case(Cc, P)
    rng = np.random.default_rng(5 * Cc + P)
    bad = codes.copy()
    where = rng.choice(P, size=min(P, 41), replace=False)
    bad[where] = np.array([Cc, Cc + 1, 255], np.uint8)[np.arange(len(where)) % 3]
    cen = (C.c_longlong * 64)()
    rc, probs, dz, loss = _run(lib, "census", z, None, bad, Cc, cen)
    assert rc == 1
    msg = lib.depgan_last_error()
    assert b"%d of %d" % (len(where), P) in msg and b"[0, %d)" % Cc in msg, msg
    got = _table(cen, Cc)
    assert np.array_equal(got, _numpy_table(bad, probs.cpu().numpy(), Cc))
    assert int(got.sum()) + len(where) == P
    # and the floats are those of the entry without the census on the same bad codes
    rc0, p0, d0, l0 = _run(lib, "plain", z, None, bad, Cc)
    assert rc0 == 1
    assert np.array_equal(_u32(p0), _u32(probs)) and np.array_equal(_u32(d0), _u32(dz)) and np.array_equal(_u32(l0), _u32(loss))


@pytest.mark.parametrize("Cc,P", [(4, 3219), (8, 262181), (3, 255)])
def test_a_second_call_into_the_same_buffers_repeats_the_table(lib, Cc, P):
    """No stale partial and no dependence on zeroing: same device buffers, same host table, other inputs in between."""
    z, codes, _, _ = _case(Cc, P)
    zd, cd = torch.from_numpy(z).cuda(), torch.from_numpy(codes).cuda()
    probs, dz, loss = torch.empty((P, Cc), device="cuda:0"), torch.empty((P, Cc), device="cuda:0"), torch.empty(1, device="cuda:0")
    cen = (C.c_longlong * 64)()
    call = lambda c_dev: lib.depgan_op_softmax_ce_census(P_(zd), None, P_(c_dev), P_(probs), P_(dz), P_(loss), cen, P, Cc,  # noqa: E731
                                                         None)
    assert call(cd) == 0, lib.depgan_last_error()
    first = _table(cen, Cc).copy()
    other = torch.from_numpy(((codes.astype(np.int64) + 1) % Cc).astype(np.uint8)).cuda()
    assert call(other) == 0
    assert not np.array_equal(_table(cen, Cc), first) or P == 1
    assert call(cd) == 0
    assert np.array_equal(_table(cen, Cc), first) and int(first.sum()) == P
