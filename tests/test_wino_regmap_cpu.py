"""No GPU: the lane mapping and the LDS slot function of the Winograd kernel (csrc/igemm_wino.hip), restated in Python
and enumerated for both tile forms (MT = 1: 32 Winograd tiles per workgroup, MT = 2: 64).

The kernel keeps the transformed input V in registers: transform task i of a lane must produce exactly the A operands
that lane hands to its MFMAs of row tile mt = i.  v_mfma_f32_32x32x2_f32 takes A[row][k] from lane row + 32 k, and the
kernel issues it four times per frequency, j = 0..3, on channel 4 k + j of the 8-channel chunk: lane (r, h) supplies
V_f[tile 32 mt + r][channel 4 h + j].  The raw halo chunk the transform reads is an unpadded [pixel][8] image filled by
DMA, lane-linearly; its 16-byte slots are permuted (rslot) so that the lanes the LDS serves together on a b128 read hit
different slots of the bank window.  Two models of "together" are enumerated: eight consecutive lanes over 128 bytes
(what the kernel's counters were read against) and the four 16-lane groups over 256 bytes.

Checked: ownership, the slot bijection and its inverse, padding -> sentinel, conflict freedom of every read, and -- by
running the staging and the transform on an integer image in numpy -- that every lane ends up with the values of
B^T d B its MFMAs need.  The old task mapping and slot functions without (or with the old) XOR must fail.
"""
import numpy as np
import pytest

TW = 18            # halo columns of a 16-pixel-wide tile
CK = 8             # channels per chunk: two 16-byte halves per pixel
ROWS = {0: (0, 2, -1.0), 1: (1, 2, 1.0), 2: (2, 1, -1.0), 3: (1, 3, -1.0)}      # row a of B^T d = d[x] + s d[y]
BT = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
SENT = None        # what a padding slot fetches (the kernel: an out-of-range offset, zeros)
GROUPS8 = [list(range(8 * k, 8 * k + 8)) for k in range(8)]
_G16 = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]]
GROUPS16 = _G16 + [[l + 32 for l in g] for g in _G16]


class Mapping:
    """The kernel's: task i of a lane is (tile 32 i + (lane & 31), half lane >> 5); slot = linear ^ ((column >> 2) & 3)."""

    def task(self, lane, i):
        return 32 * i + (lane & 31), lane >> 5

    def rslot(self, pix, half):
        return (2 * pix + half) ^ (((pix % TW) >> 2) & 3)

    def rslot_inv(self, q):
        return q ^ ((((q >> 1) % TW) >> 2) & 3)


class OldTasks(Mapping):
    """MUTANT: the mapping of the LDS-V kernel (q = lane + 64 i -> tile q >> 1, half q & 1)."""

    def task(self, lane, i):
        q = lane + 64 * i
        return q >> 1, q & 1


class NoXor(Mapping):
    """MUTANT: the linear image."""

    def rslot(self, pix, half):
        return 2 * pix + half

    def rslot_inv(self, q):
        return q


class OldXor(Mapping):
    """MUTANT: the slot function that served four tiles x two halves per eight lanes."""

    def rslot(self, pix, half):
        return (2 * pix + half) ^ (((pix >> 2) & 1) << 1)

    def rslot_inv(self, q):
        return q ^ (((q >> 3) & 1) << 1)


class WrongInverse(Mapping):
    """MUTANT: a stated inverse that is none (keyed by the slot's own low bits)."""

    def rslot_inv(self, q):
        return q ^ ((q >> 2) & 3)


def geometry(MT):
    pixt = (8 * MT + 2) * TW
    xtot = 2 * pixt
    nxp = (xtot + 255) // 256
    return pixt, xtot, nxp * 256


def mfma_demand(MT):
    """{(lane, mt): (tile, half)} from the operand layout alone: A[row][k] comes from lane row + 32 k."""
    return {(row + 32 * k, mt): (32 * mt + row, k) for mt in range(MT) for row in range(32) for k in range(2)}


def check_ownership(m, MT):
    got = {(lane, i): m.task(lane, i) for lane in range(64) for i in range(MT)}
    owners = {}
    for key, task in got.items():
        owners.setdefault(task, []).append(key)
    want = {(T, half) for T in range(32 * MT) for half in range(2)}
    assert set(owners) == want and all(len(v) == 1 for v in owners.values()), "every (tile, half) owned exactly once"
    assert got == mfma_demand(MT), "task i of a lane = what its MFMAs of row tile i take from it"


def check_slots(m, MT):
    pixt, xtot, nslots = geometry(MT)
    image = [m.rslot(p, h) for p in range(pixt) for h in range(2)]
    assert sorted(image) == list(range(xtot)), "a bijection on the pieces of a chunk"
    for p in range(pixt):
        for h in range(2):
            assert m.rslot_inv(m.rslot(p, h)) == 2 * p + h, "the stated inverse inverts it"
    for q in range(nslots):
        lq = m.rslot_inv(q)
        assert (lq >= xtot) == (q >= xtot), "padding slots fetch the sentinel, and only they"
        assert 0 <= lq < nslots


def reads(m, MT):
    """every b128 read of the transform: (wave = a, task i, row, j) -> slot per lane"""
    for a, (ra, rb, _) in ROWS.items():
        for i in range(MT):
            for row in (ra, rb):
                for j in range(4):
                    slots = []
                    for lane in range(64):
                        T, half = m.task(lane, i)
                        slots.append(m.rslot((2 * (T >> 3) + row) * TW + 2 * (T & 7) + j, half))
                    yield (a, i, row, j), slots


def check_conflicts(m, MT, groups, window):
    for what, slots in reads(m, MT):
        for g in groups:
            hit = {}
            for lane in g:
                hit.setdefault(slots[lane] % window, set()).add(slots[lane])
            assert all(len(v) == 1 for v in hit.values()), (what, g[0], "two addresses on one 16-byte bank slot")


def staged_image(m, MT, halo):
    """the LDS image after the DMA: slot q holds logical piece rslot_inv(q) of halo[pixel][8], padding zeros"""
    pixt, xtot, nslots = geometry(MT)
    lds = np.zeros((nslots, 4))
    for q in range(nslots):
        lq = m.rslot_inv(q)
        if lq < xtot:
            lds[q] = halo[lq >> 1, 4 * (lq & 1):4 * (lq & 1) + 4]
    return lds


def check_values(m, MT):
    """stage an integer halo, run every lane's transform tasks, compare with B^T d B of the tile the MFMA wants"""
    pixt, _, _ = geometry(MT)
    halo = np.random.default_rng(MT).integers(-8, 9, (pixt, CK)).astype(np.float64)
    lds = staged_image(m, MT, halo)
    d = halo.reshape(8 * MT + 2, TW, CK)
    demand = mfma_demand(MT)
    for a, (ra, rb, s) in ROWS.items():                  # wave a
        for lane in range(64):
            for i in range(MT):
                T, half = m.task(lane, i)
                ty, tx = T >> 3, T & 7
                tc = [lds[m.rslot((2 * ty + ra) * TW + 2 * tx + j, half)] + s * lds[m.rslot((2 * ty + rb) * TW + 2 * tx + j, half)]
                      for j in range(4)]
                vr = [tc[0] - tc[2], tc[1] + tc[2], tc[2] - tc[1], tc[1] - tc[3]]          # b = 0..3, four channels each
                wt, wh = demand[(lane, i)]
                tile = d[2 * (wt >> 3):2 * (wt >> 3) + 4, 2 * (wt & 7):2 * (wt & 7) + 4, 4 * wh:4 * wh + 4]
                V = np.einsum("ay,yxc,bx->abc", BT, tile, BT)
                assert np.array_equal(np.array(vr), V[a]), (a, lane, i)


CHECKS = {
    "ownership": check_ownership,
    "slots": check_slots,
    "conflicts8": lambda m, MT: check_conflicts(m, MT, GROUPS8, 8),
    "conflicts16": lambda m, MT: check_conflicts(m, MT, GROUPS16, 16),
    "values": check_values,
}


@pytest.mark.parametrize("MT", [1, 2])
@pytest.mark.parametrize("check", list(CHECKS))
def test_kernel_mapping(check, MT):
    CHECKS[check](Mapping(), MT)


@pytest.mark.parametrize("MT", [1, 2])
@pytest.mark.parametrize("mutant,caught_by", [
    (OldTasks, ("ownership", "values")),            # every tile still owned once, but by the wrong lane
    (NoXor, ("conflicts8", "conflicts16")),
    (OldXor, ("conflicts8", "conflicts16")),
    (WrongInverse, ("slots", "values")),
])
def test_wrong_mappings_fail(mutant, caught_by, MT):
    for name in caught_by:
        with pytest.raises(AssertionError):
            CHECKS[name](mutant(), MT)


def test_lds_footprint_is_the_z_exchange():
    """WnCfg::LDS = max(2 RAW, Z): the two raw buffers fit under the epilogue's Z planes in both forms."""
    for MT, kb in ((1, 37), (2, 73)):
        _, _, nslots = geometry(MT)
        raw2 = 2 * nslots * 16
        z = 8 * (32 * MT * 36 + 32) * 4
        assert raw2 < z and z // 1024 == kb
