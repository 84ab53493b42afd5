"""The balanced cutting of the z-marching CostRegNet kernels (csrc/zm_common.hpp) computes the bits of the uniform one: outputs and
published bounds of CDS_ZM_BALANCE=0 (columns x z segments, as before) against CDS_ZM_BALANCE=2 (one contiguous range per workgroup,
walked piece by piece), with CDS_ZM_NCU forcing workgroup counts that give workgroups of one, two, three and more pieces, ranges that
end exactly on a column boundary, short pieces that move to their neighbour and empty workgroups (more workgroups than stages).
Every comparison is two calls in this process on the same inputs."""
import contextlib
import ctypes
import functools
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
VOL = (11, 19, 70)                     # D x H x W of the convolutions' input: a few columns in x and y, D no multiple of G = 3
ZMG_NCU = (3, 4, 7, 200)
# layer -> (Cin, Cout, stride code, (TXO, TYO, G, YS) of its z-march configuration, may run balanced)
PAIR = 101
ZMG = {
    "pair8": (8, 8, PAIR, (32, 8, 3, 1), True), "conv1": (8, 16, 2, (16, 8, 1, 1), True), "conv2": (16, 16, 1, (32, 8, 1, 1), True),
    "conv3": (16, 32, 2, (16, 4, 1, 1), True), "conv4": (32, 32, 1, (16, 4, 1, 1), True),
    "conv5": (32, 64, 2, (16, 2, 1, 1), False), "conv6": (64, 64, 1, (16, 2, 1, 2), False),
}
ZMG_CASES = [(n, True) for n in ZMG] + [(n, False) for n in ("conv1", "conv2", "conv3")]


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from cds_mvsnet_amd import ops as o
    assert o.version() >= 100
    return o


def _plan(family, cols, planes, unit, ys, ncu):
    """(balanced under CDS_ZM_BALANCE=2?, pieces of every workgroup) from the library's host entry points."""
    from cds_mvsnet_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 4)()
    assert lib.cds_zm_plan(family, cols, planes, unit, ys, ncu, 2, out) == 0
    nwg, one = max(1, ncu // ys), (ctypes.c_int * 24)()
    counts = [lib.cds_zm_partition(cols, planes, unit, nwg, wg, 4 if family == 0 else 3, one) for wg in range(nwg)]
    return bool(out[0]), counts


def _both(call, ncu):
    """The same call under the uniform and under the forced balanced cutting."""
    res = []
    for balance in (0, 2):
        with _env(CDS_ZM_BALANCE=balance, CDS_ZM_NCU=ncu, CDS_ZMG_NSEG=None, CDS_DZM_NSEG=None, CDS_DPZ_NSEG=None):
            res.append(call())
    torch.cuda.synchronize()
    return res


@functools.lru_cache(maxsize=None)
def _zmg_inputs(name, f16):
    from cds_mvsnet_amd import ops
    cin, cout, stride, _, _ = ZMG[name]
    g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + (stride % 7))
    x_cl = (torch.randn(*VOL, cin, generator=g) * torch.exp(0.5 * torch.randn(cin, generator=g))).to(DEV)
    w = torch.randn(cout, cin, 3, 3, 3, generator=g) / (27 * cin) ** 0.5
    b = torch.randn(cout, generator=g).to(DEV)
    pack = ops.split_pack_conv3d_pair if stride == PAIR else ops.split_pack_conv3d
    wh, w_inv = pack(w.to(DEV), f16=True) if f16 else (pack(w.to(DEV)), 1.0)
    return x_cl, wh, w_inv, b, x_cl.abs().amax().reshape(1)


@pytest.mark.parametrize("ncu", ZMG_NCU)
@pytest.mark.parametrize("name,f16", ZMG_CASES)
def test_conv3d_zmg_balanced_is_bit_identical(name, f16, ncu, ops):
    if f16 and not ops.USE_SPLIT_F16:
        pytest.skip("CDS_SPLIT_F16=0: the split-f16 convolution entry is switched off")
    cin, cout, stride, (txo, tyo, G, ys), may = ZMG[name]
    x_cl, wh, w_inv, b, in_bound = _zmg_inputs(name, f16)
    s = 2 if stride == 2 else 1
    Do, Ho, Wo = ((v - 1) // s + 1 for v in VOL)
    balanced, counts = _plan(0, -(-Wo // txo) * -(-Ho // tyo), Do, G, ys, ncu)
    print(f"{name} f16 {int(f16)} ncu {ncu}: balanced {int(balanced and may)}, pieces per workgroup {sorted(set(counts))}")

    def call():
        ob = torch.zeros(1, device=DEV) if f16 else None
        kw = dict(in_bound=in_bound, w_inv_scale=w_inv, out_bound=ob) if f16 else {}
        return ops.conv3d_sbf(x_cl, wh, b, cout, stride=stride, relu=True, **kw), ob

    with _env(CDS_ZMG_DEEP=2, CDS_ZMG=None):
        (u, ub), (v, vb) = _both(call, ncu)
    assert u.shape == (Do, Ho, Wo, cout) and torch.isfinite(u).all() and float(u.abs().max()) > 0
    assert torch.equal(u, v)
    if f16:
        assert float(ub) == float(u.abs().max()) and torch.equal(ub, vb)


def test_zmg_cases_reach_the_piece_counts():
    """What the workgroup counts above do to the 9 columns of conv2 (11 stages) and of pair8 (4 stages of 3 planes, the last one of
    2): workgroups of one, two and three pieces, ranges that end on a column boundary, empty workgroups."""
    seen = set()
    for ncu in ZMG_NCU:
        for planes, unit in ((11, 1), (11, 3)):
            balanced, counts = _plan(0, 9, planes, unit, 1, ncu)
            assert balanced
            seen |= set(counts)
    assert seen >= {0, 1, 2, 3}, seen
    assert _plan(0, 9, 11, 1, 1, 3)[1] == [3, 3, 3]          # 33 slots each: three whole columns


@functools.lru_cache(maxsize=None)
def _deconv_inputs(cin, cout, shape):
    D, H, W = shape
    g = torch.Generator().manual_seed(cin * 100 + cout)
    x_cl = (torch.randn(D, H, W, cin, generator=g) * torch.exp(0.5 * torch.randn(cin, generator=g))).to(DEV)
    w = torch.randn(cin, cout, 3, 3, 3, generator=g) / (27 * cin / 8) ** 0.5
    b = torch.randn(cout, generator=g).to(DEV)
    skip = torch.randn(2 * D, 2 * H, 2 * W, cout, generator=g).to(DEV)
    return x_cl, w.to(DEV), b, skip, x_cl.abs().amax().reshape(1)


@pytest.mark.parametrize("ncu", ZMG_NCU)
@pytest.mark.parametrize("f16", [True, False])
def test_conv9_balanced_is_bit_identical(f16, ncu, ops):
    """deconv3d_zm (32 -> 16) at 9 x 13 x 37 cells: 3 x 2 columns of 9 cell planes."""
    x_cl, w, b, skip, in_bound = _deconv_inputs(32, 16, (9, 13, 37))
    wcls, w_inv = ops.split_pack_deconv_cls(w, f16=True) if f16 else (ops.split_pack_deconv_cls(w), 1.0)
    balanced, counts = _plan(1, 6, 9, 1, 1, ncu)
    print(f"conv9 f16 {int(f16)} ncu {ncu}: balanced {int(balanced)}, pieces per workgroup {sorted(set(counts))}")
    assert balanced

    def call():
        ob = torch.zeros(1, device=DEV) if f16 else None
        kw = dict(in_bound=in_bound, w_inv_scale=w_inv, out_bound=ob) if f16 else {}
        return ops.deconv3d_zm(x_cl, wcls, b, relu=True, skip=skip, **kw), ob

    (u, ub), (v, vb) = _both(call, ncu)
    assert torch.isfinite(u).all() and float(u.abs().max()) > 0
    assert torch.equal(u, v)
    if f16:
        assert float(ub) == float(u.abs().max()) and torch.equal(ub, vb)


@pytest.mark.parametrize("ncu", ZMG_NCU)
def test_conv7_balanced_is_bit_identical(ncu, ops):
    """deconv3d_sbf (64 -> 32, split-f16) on its z-march (CDS_DZM_DEEP=2) at 9 x 13 x 37 cells: 3 x 4 columns, two cout blocks, each
    cut over half of the workgroups (one workgroup would have 12 pieces: the uniform cutting stays)."""
    if not ops.USE_SPLIT_F16:
        pytest.skip("CDS_SPLIT_F16=0: the split-f16 entry is switched off")
    x_cl, w, b, skip, in_bound = _deconv_inputs(64, 32, (9, 13, 37))
    wh, w_inv = ops.split_pack_deconv3d(w, f16=True)
    balanced, counts = _plan(1, 12, 9, 1, 2, ncu)
    print(f"conv7 ncu {ncu}: balanced {int(balanced)}, pieces per workgroup {sorted(set(counts))}")
    assert balanced == (ncu != 3)

    def call():
        ob = torch.zeros(1, device=DEV)
        return ops.deconv3d_sbf(x_cl, wh, b, 32, relu=True, skip=skip, in_bound=in_bound, w_inv_scale=w_inv, out_bound=ob), ob

    with _env(CDS_DZM_DEEP=2):
        (u, ub), (v, vb) = _both(call, ncu)
    assert torch.isfinite(u).all() and float(u.abs().max()) > 0
    assert torch.equal(u, v)
    assert float(ub) == float(u.abs().max()) and torch.equal(ub, vb)


@functools.lru_cache(maxsize=None)
def _tail_inputs():
    D, H, W = 5, 19, 91                # 4 x 4 columns of 30 x 6 cells
    g = torch.Generator().manual_seed(5 * 1000 + 19 * 10 + 91)
    x_cl = (torch.randn(D, H, W, 16, generator=g) * torch.exp(0.5 * torch.randn(16, generator=g))).to(DEV)
    skip = torch.randn(2 * D, 2 * H, 2 * W, 8, generator=g).to(DEV)
    w11 = (torch.randn(16, 8, 3, 3, 3, generator=g) / (27 * 2) ** 0.5).to(DEV)
    b11 = torch.randn(8, generator=g).to(DEV)
    wp = (torch.randn(1, 8, 3, 3, 3, generator=g) / 27 ** 0.5).to(DEV)
    return x_cl, skip, w11, b11, wp


@pytest.mark.parametrize("ncu", (3, 6, 16, 50))
@pytest.mark.parametrize("form", ["sbf", "sf16_valu", "sf16_mfma"])
def test_tail_balanced_is_bit_identical(form, ncu, ops):
    """The fused tail's three instantiations (split-bf16; split-f16 with prob on the VALU; with prob on the matrix cores) at
    5 x 19 x 91 cells: 16 columns of 5 cell planes."""
    x_cl, skip, w11, b11, wp = _tail_inputs()
    balanced, counts = _plan(2, 16, 5, 1, 1, ncu)
    print(f"tail {form} ncu {ncu}: balanced {int(balanced)}, pieces per workgroup {sorted(set(counts))}")
    assert balanced
    table = ops.pack_prob_table(wp)
    if form == "sbf":
        wh = ops.split_pack_deconv_prob(w11)
        call = lambda: ops.deconv_prob_zm(x_cl, wh, b11, skip, table)
    else:
        wh, w_inv = ops.split_pack_deconv_prob(w11, f16=True)
        wm, wms = ops.split_pack_prob(wp, f16=True)
        in_bound, skip_bound = x_cl.abs().amax().reshape(1), skip.abs().amax().reshape(1)
        gain = ops.deconv_prob_gain(wh, w_inv)
        call = lambda: ops.deconv_prob_zm(x_cl, wh, b11, skip, table, in_bound=in_bound, w_inv_scale=w_inv, prob_mfma=wm,
                                          prob_inv_scale=wms, skip_bound=skip_bound, y_gain=gain)
    with _env(CDS_DPZ_PROB_MFMA="0" if form == "sf16_valu" else None):
        u, v = _both(call, ncu)
    assert torch.isfinite(u).all() and float(u.abs().max()) > 0
    assert torch.equal(u, v)


def test_tail_cases_reach_the_piece_counts():
    seen = set()
    for ncu in (3, 6, 16, 50):
        seen |= set(_plan(2, 16, 5, 1, 1, ncu)[1])
    assert seen >= {0, 1, 2, 3}, seen
