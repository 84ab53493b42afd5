"""The numpy restatement of the photometric score (photo_ref.py) against independent statements of the same
quantities: the separable window against a direct 121-term sum, identical images, a constant offset, and what a held-out score is
for: it prefers the textured render to the vertex colours, and it falls when the surface is in the wrong place.  No GPU."""
import math

import numpy as np

import photo_ref as P
import texture_ref as T


def test_gauss_table_sums_to_one_and_is_symmetric():
    g = P.gauss_table()
    assert g.shape == (11,) and abs(g.sum() - 1.0) < 1e-15 and np.array_equal(g, g[::-1]) and g.argmax() == 5


def test_separable_window_equals_the_direct_sum():
    """Both are sums of the same 121 products g_i g_j m; they differ by their roundings only, at most 121 2^-52 sum |terms|."""
    g = P.gauss_table()
    a = T.view_images(1, 23, 29)[0, :, :, 0].astype(np.float64)
    for m in (a, a * a):
        got = P.window_means(m, g)
        assert got.shape == (13, 19)
        worst = 0.0
        for y in range(got.shape[0]):
            for x in range(got.shape[1]):
                terms = np.outer(g, g) * m[y:y + 11, x:x + 11]
                bound = 121 * 2.0 ** -52 * np.abs(terms).sum()
                err = abs(got[y, x] - math.fsum(terms.ravel().tolist()))
                assert err <= bound, (y, x, err, bound)
                worst = max(worst, err / bound)
        print(f"separable against direct: worst error {worst:.3f} of the bound")


def test_window_counts_is_the_all_of_121():
    rs = np.random.RandomState(3)
    mask = (rs.rand(30, 27) > 0.01).astype(np.uint8) * 7
    want = np.array([[bool((mask[y:y + 11, x:x + 11] != 0).all()) for x in range(17)] for y in range(20)])
    got = P.window_counts(mask)
    assert np.array_equal(got, want) and want.any() and not want.all()


def test_identical_images_give_ssim_one_and_psnr_inf():
    a = T.view_images(2, 20, 31)
    mask = np.ones((2, 20, 31), np.uint8)
    s = P.scores(a, a, mask)
    assert (s["ssim_map"] == 1.0).all() and (s["ssim"] == 1.0).all() and np.isinf(s["psnr"]).all() and (s["psnr"] > 0).all()
    assert (s["sse"] == 0).all() and (s["n_px"] == 20 * 31).all() and (s["n_win"] == 10 * 21).all() and (s["coverage"] == 1.0).all()


def test_psnr_of_a_constant_offset():
    a = (T.view_images(1, 16, 18) // 2).astype(np.uint8)                                      # <= 127: a + k does not wrap
    for k in (1, 7, 100):
        s = P.scores(a, (a + k).astype(np.uint8), np.ones((1, 16, 18), np.uint8))
        assert abs(s["psnr"][0] - 20.0 * math.log10(255.0 / k)) < 1e-12, (k, s["psnr"])


def test_mask_limits_the_pixels_and_the_windows():
    a, b, mask = P.image_pair(1, 24, 30)
    s = P.scores(a, b, mask)
    assert s["n_px"][0] == 24 * 30 - 2 and 0 < s["n_win"][0] < 14 * 20
    assert np.isnan(s["ssim_map"]).sum() == 3 * (14 * 20 - s["n_win"][0])
    none = P.scores(a, b, np.zeros_like(mask))
    assert none["n_px"][0] == 0 and np.isnan(none["psnr"][0]) and np.isnan(none["ssim"][0]) and none["coverage"][0] == 0.0
    small = P.scores(a[:, :10], b[:, :10], mask[:, :10])
    assert small["n_win"][0] == 0 and small["ssim_map"].shape == (1, 3, 0, 0) and np.isnan(small["ssim"][0])
    assert np.isfinite(small["psnr"][0])


def test_held_out_view_prefers_the_texture_and_punishes_a_moved_surface():
    """The analytic-pattern plane, four views texture it and the fifth is held out.  The pattern has several periods across a
    face, so interpolated vertex colours cannot show it and the atlas can; a surface moved along its normal is textured from
    the wrong pixels and rendered at the wrong place, and the held-out score falls.  The camera centres lie 1.2 and 2.5 apart from
    the held-out one at focal length 120 and depth 5: 0.4 along z is 120 x 1.2 x 0.4 / 25 = 2.4 to 4.8 pixels of parallax."""
    tex, vert, moved = P.holdout_scores(0.0), P.holdout_scores(0.0, "vertex"), P.holdout_scores(0.4)
    print(f"held out: textured {tex['psnr'][0]:.2f} dB ssim {tex['ssim'][0]:.4f}; vertex colours {vert['psnr'][0]:.2f} dB ssim "
          f"{vert['ssim'][0]:.4f}; moved by 0.4 {moved['psnr'][0]:.2f} dB ssim {moved['ssim'][0]:.4f}; coverage {tex['coverage'][0]:.3f}")
    assert tex["coverage"][0] > 0.3 and tex["n_win"][0] > 0
    assert tex["psnr"][0] > vert["psnr"][0] and tex["ssim"][0] > vert["ssim"][0]
    assert moved["psnr"][0] < tex["psnr"][0] and moved["ssim"][0] < tex["ssim"][0]
