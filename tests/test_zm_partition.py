"""The balanced cutting of the z-marching CostRegNet layers (csrc/zm_common.hpp) through the library's host entry points
cds_zm_partition / cds_zm_partition_all / cds_zm_plan: no GPU call.

A layer is cols columns of `stages` stages; workgroup wg of nwg owns one contiguous range of the column-major (column, stage)
sequence, cut at the column boundaries into pieces.  Swept: cols 1..40 x stages 1..64 x nwg in NWG, in the units of both kernel
families (cell planes, min_len 3; stages of G output planes over a depth that is not a multiple of G, min_len 4).  Checked for every
combination: every (column, plane) is covered exactly once; a piece starts on a multiple of the unit and ends on one or at the
column's end; a workgroup has no more pieces than a range of ceil(T / nwg) slots can touch; no piece is shorter than min_len stages
unless it is a whole column."""
import ctypes

import numpy as np
import pytest

NWG = (1, 2, 3, 5, 7, 16, 31, 256, 1000)
MAX_PIECES = 8            # ZM_MAX_PIECES
CAP = 40                  # pieces per workgroup the sweep can hold: nwg = 1 owns all 40 columns


@pytest.fixture(scope="module")
def lib():
    from cds_mvsnet_amd import _lib
    return _lib.load()


def _pieces(lib, cols, planes, unit, nwg, min_len, buf):
    rc = lib.cds_zm_partition_all(cols, planes, unit, nwg, min_len, CAP, buf.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return buf[:nwg * (1 + 3 * CAP)].reshape(nwg, 1 + 3 * CAP)


def _check(tab, cols, planes, unit, nwg, min_len):
    what = (cols, planes, unit, nwg, min_len)
    stages = -(-planes // unit)
    n = tab[:, 0]
    assert n.min() >= 0 and n.max() <= CAP, what
    # the pieces per workgroup stay within what a range of L slots can touch
    L = -(-cols * stages // nwg)
    assert n.max() <= (L - 2) // stages + 2, (what, int(n.max()))
    tri = tab[:, 1:].reshape(nwg, CAP, 3)
    live = np.arange(CAP)[None, :] < n[:, None]
    col, z0, z1 = tri[..., 0][live], tri[..., 1][live], tri[..., 2][live]      # in workgroup order, then piece order
    assert ((col >= 0) & (col < cols) & (z0 >= 0) & (z0 < z1) & (z1 <= planes)).all(), what
    # whole multiples of the unit
    assert (z0 % unit == 0).all() and ((z1 % unit == 0) | (z1 == planes)).all(), what
    # every (column, plane) exactly once
    cover = np.zeros(cols * planes + 1, dtype=np.int64)
    np.add.at(cover, col * planes + z0, 1)
    np.add.at(cover, col * planes + z1, -1)
    assert (np.cumsum(cover)[:-1] == 1).all(), what
    # and in order: workgroup after workgroup, piece after piece, the column-major sequence without a gap
    start, end = col * planes + z0, col * planes + z1
    assert start[0] == 0 and end[-1] == cols * planes and (start[1:] == end[:-1]).all(), what
    # no piece below the minimum unless it is a whole column
    nst = -(-(z1 - z0) // unit)
    assert ((nst >= min_len) | ((z0 == 0) & (z1 == planes))).all(), what
    return int(n.max())


@pytest.mark.parametrize("family", ["cell", "zmg"])
def test_partition_sweep(lib, family):
    buf = np.zeros(max(NWG) * (1 + 3 * CAP), dtype=np.int32)
    one = (ctypes.c_int * (3 * MAX_PIECES))()
    seen = set()
    for cols in range(1, 41):
        for stages in range(1, 65):
            if family == "cell":
                unit, planes, min_len = 1, stages, 3
            else:                                   # G = 1 or 3, the depth one or two planes short of a multiple of G
                unit = 1 + 2 * (cols & 1)
                planes, min_len = stages * unit - (unit - 1) * (stages & 1), 4
            for nwg in NWG:
                tab = _pieces(lib, cols, planes, unit, nwg, min_len, buf)
                nmax = _check(tab, cols, planes, unit, nwg, min_len)
                seen.add(min(nmax, MAX_PIECES + 1))
                # the single-workgroup entry agrees with the table (first, last and a middle workgroup), and beyond the compile-time
                # bound the launch keeps the uniform cutting even when the balanced one is forced
                for wg in {0, nwg // 2, nwg - 1}:
                    got = lib.cds_zm_partition(cols, planes, unit, nwg, wg, min_len, one)
                    assert got == tab[wg, 0]
                    k = 3 * min(got, MAX_PIECES)
                    assert list(one[:k]) == list(tab[wg, 1:1 + k])
                plan = (ctypes.c_int * 4)()
                fam = 2 if family == "cell" else 0
                assert lib.cds_zm_plan(fam, cols, planes, unit, 1, nwg, 2, plan) == 0
                assert plan[0] == (1 if nmax <= MAX_PIECES else 0), (cols, planes, unit, nwg, nmax, list(plan))
    assert seen >= set(range(1, MAX_PIECES + 2)), seen      # the sweep reaches every piece count and the fallback


def test_partition_examples(lib):
    """Hand-checked cuttings: a range that ends exactly on a column boundary, a short piece that goes to its neighbour on either side,
    empty workgroups where there are more of them than slots."""
    def P(cols, planes, unit, nwg, min_len):
        out = []
        for wg in range(nwg):
            o = (ctypes.c_int * (3 * MAX_PIECES))()
            n = lib.cds_zm_partition(cols, planes, unit, nwg, wg, min_len, o)
            out.append([tuple(o[3 * i:3 * i + 3]) for i in range(n)])
        return out
    # 9 columns x 11 stages over 3 workgroups: 33 slots each = three whole columns
    assert P(9, 11, 1, 3, 4) == [[(0, 0, 11), (1, 0, 11), (2, 0, 11)], [(3, 0, 11), (4, 0, 11), (5, 0, 11)], [(6, 0, 11), (7, 0, 11), (8, 0, 11)]]
    # 3 x 10 over 4: the raw cuts 7 | 15 | 22 leave pieces of 3 at [7, 10) and 2 at [20, 22): both go to the neighbour (min_len 4)
    assert P(3, 10, 1, 4, 4) == [[(0, 0, 10)], [(1, 0, 5)], [(1, 5, 10)], [(2, 0, 10)]]
    # the same with min_len 3: [7, 10) is long enough to stay
    assert P(3, 10, 1, 4, 3) == [[(0, 0, 7)], [(0, 7, 10), (1, 0, 5)], [(1, 5, 10)], [(2, 0, 10)]]
    # more workgroups than slots: cuts at the multiples of min_len only, most workgroups empty; G = 3 over 11 planes = 4 stages
    cut = P(2, 11, 3, 50, 4)
    assert [p for wg in cut for p in wg] == [(0, 0, 11), (1, 0, 11)] and sum(1 for wg in cut if not wg) == 48


# The M1 step (640 x 512, D = 192, 8 channels) on 256 CUs: (family, columns, planes, planes per stage, cout splits) of every z-march
# layer and what the default (CDS_ZM_BALANCE=1) chooses: profiles/zm_balance.md reports the same table.  conv5 and conv6: the
# model would balance them, their kernels have no registers left for the walk and keep the uniform cutting (ZgConv5F16 /
# ZgConv6F16::BALANCED in csrc/conv3d_zmg.hip); that is decided by the configuration, not by this plan.  The tail: the model
# promises 6 %, measured none: below the margin the tail asks for.
M1 = {
    "conv0": ((0, 1280, 192, 3, 1), 0), "conv1": ((0, 640, 96, 1, 1), 0), "conv2": ((0, 320, 96, 1, 1), 1),
    "conv3": ((0, 320, 48, 1, 1), 1), "conv4": ((0, 320, 48, 1, 1), 1), "conv5": ((0, 160, 24, 1, 1), 1),
    "conv6": ((0, 160, 24, 1, 2), 1), "conv7": ((1, 80, 24, 1, 2), 1), "conv9": ((1, 160, 48, 1, 1), 1),
    "tail": ((2, 473, 96, 1, 1), 0),
}


@pytest.mark.parametrize("layer", sorted(M1))
def test_chooser_at_m1(lib, layer):
    (fam, cols, planes, unit, ys), want = M1[layer]
    out = (ctypes.c_int * 4)()
    assert lib.cds_zm_plan(fam, cols, planes, unit, ys, 256, 1, out) == 0
    print(f"{layer}: balanced {out[0]}, uniform nseg {out[1]}, model cost uniform {out[2] / 1000} balanced {out[3] / 1000}")
    assert out[0] == want
    # CDS_ZM_BALANCE=0 is the uniform cutting whatever the model says
    assert lib.cds_zm_plan(fam, cols, planes, unit, ys, 256, 0, out) == 0 and out[0] == 0
