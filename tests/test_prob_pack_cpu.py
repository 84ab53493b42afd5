"""Host side of prob on the matrix cores (csrc/deconv_prob_zm.hip): the operands of ops.split_pack_prob.

One 16 x 32 MFMA operand per (rotation r, ky) in lane order (lane = 16 k-group + row, 8 channels each): row 4 kz + kx holds tap
((kz + r) mod 3, ky, kx); the k-groups are w_hi | w_hi | w_lo | spare, which the kernel multiplies with y_hi | y_lo | y_hi | anything."""
import pytest
import torch

from cds_mvsnet_amd import ops


def _operands(seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(1, 8, 3, 3, 3, generator=g) * scale / 27 ** 0.5
    packed, inv = ops.split_pack_prob(w, f16=True)
    assert packed.dtype == torch.int16 and tuple(packed.shape) == (3, 3, 64, 8) and packed.is_contiguous()
    return w, packed.view(torch.float16).double().reshape(3, 3, 4, 16, 8), inv       # [r][ky][k-group][row][c]


@pytest.mark.parametrize("scale", [1.0, 3e-4, 700.0])
def test_split_pack_prob_round_trip(scale):
    """hi + lo reproduces w x scale to 2^-22 (relative), the scale is the power of two that puts max |w| into (2^14, 2^15], and
    k-groups 0 and 1 are the same high term."""
    w, a, inv = _operands(1, scale)
    s = 1.0 / inv
    assert s == 2.0 ** round(torch.log2(torch.tensor(s)).item())
    assert 2.0 ** 14 < w.abs().max().item() * s <= 2.0 ** 15
    assert torch.equal(a[:, :, 0], a[:, :, 1])
    wd = w.double()[0] * s                                                            # [c][kz][ky][kx]
    for r in range(3):
        for ky in range(3):
            for kz in range(3):
                for kx in range(3):
                    want = wd[:, (kz + r) % 3, ky, kx]
                    got = a[r, ky, 0, 4 * kz + kx] + a[r, ky, 2, 4 * kz + kx]
                    assert ((got - want).abs() <= 2.0 ** -22 * want.abs()).all(), (r, ky, kz, kx)


def test_split_pack_prob_rows_are_rotated_taps():
    """Row 4 kz + kx of the rotation r operand holds tap ((kz + r) mod 3, ky, kx): its high term is RN16(w x scale) of that tap."""
    w, a, inv = _operands(2)
    hi = (w[0] / inv).to(torch.float16).double()                                      # [c][kz][ky][kx]
    for r in range(3):
        for ky in range(3):
            for kz in range(3):
                for kx in range(3):
                    assert torch.equal(a[r, ky, 0, 4 * kz + kx], hi[:, (kz + r) % 3, ky, kx]), (r, ky, kz, kx)
    # the three rotations hold the same 27 taps
    for r in (1, 2):
        for kz in range(3):
            assert torch.equal(a[r, :, :, 4 * kz:4 * kz + 3], a[0, :, :, 4 * ((kz + r) % 3):4 * ((kz + r) % 3) + 3])


def test_split_pack_prob_unused_rows_and_spare_slot_are_zero():
    _, a, _ = _operands(3)
    assert (a[:, :, 3] == 0).all()                                                    # the spare K slot
    for row in (3, 7, 11, 12, 13, 14, 15):
        assert (a[:, :, :, row] == 0).all(), row
    assert (a[:, :, 0, [0, 1, 2, 4, 5, 6, 8, 9, 10]] != 0).any()


def test_split_pack_prob_rejects_other_forms():
    with pytest.raises(ValueError):
        ops.split_pack_prob(torch.zeros(1, 8, 3, 3, 3), f16=False)
    with pytest.raises(ValueError):
        ops.split_pack_prob(torch.zeros(1, 16, 3, 3, 3))
