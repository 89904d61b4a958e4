"""k_resize_lds tile edges, workgroup orders, scales and caller-owned level 0: every level of every image bit-exact against
oracle.pyramid (OpenCV 3.3 fixed point). Images are cheap patterns: image i of a batch is pattern i mod 5 (seeded noise, ramp,
all 0, all 255, 0/255 checkerboard -- the last one reaches the largest intermediate values of the blend) rolled by i pixels,
so a wrong image index shows."""
import numpy as np
import pytest

import oracle
from trackingbench_slam_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _patterns(w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    return [np.random.default_rng(1234).integers(0, 256, (h, w), dtype=np.uint8),
            ((xx * 3 + yy * 7) & 255).astype(np.uint8),
            np.zeros((h, w), np.uint8),
            np.full((h, w), 255, np.uint8),
            (((xx + yy) & 1) * 255).astype(np.uint8)]


def _batch(w, h, n):
    pats = _patterns(w, h)
    return np.stack([np.roll(pats[i % 5], i, axis=1) for i in range(n)])


_EXPECTED = {}


def _expected(w, h, n, nl, scale):
    """oracle pyramids of the batch, computed once per geometry and left unchanged"""
    key = (w, h, n, nl, scale)
    if key not in _EXPECTED:
        _EXPECTED[key] = [oracle.pyramid(img, nl, scale)[0] for img in _batch(w, h, n)]
    return _EXPECTED[key]


def _check(ex, exp, n, nl):
    for i in range(n):
        for l in range(nl):
            got = ex.get_level(i, l)
            assert got.shape == exp[i][l].shape, (i, l)
            assert np.array_equal(got, exp[i][l]), "image %d level %d" % (i, l)


def _run_host(ctx, w, h, n, nl, scale):
    ex = capi.Extractor(ctx, w, h, nl, scale, n, 100)
    try:
        ex.set_images_host(_batch(w, h, n))
        ex.build_pyramid(n)
        _check(ex, _expected(w, h, n, nl, scale), n, nl)
    finally:
        ex.close()


@pytest.mark.parametrize("n", [3, 64, 70])
def test_workgroup_orders(ctx, n):
    """n = 3: 3-D grid; n = 64: one image per XCD slot; n = 70: a last XCD group that is not full"""
    _run_host(ctx, 333, 41, n, 3, 0.8)


@pytest.mark.parametrize("w", [255, 256, 257, 320, 321, 333])
def test_tile_edges_width(ctx, w):
    _run_host(ctx, w, 41, 3, 3, 0.8)


@pytest.mark.parametrize("w,h,nl,n", [(640, 480, 8, 3), (40, 30, 3, 3), (1241, 376, 5, 64)])
def test_tile_edges_levels(ctx, w, h, nl, n):
    _run_host(ctx, w, h, n, nl, 0.8)


@pytest.mark.parametrize("w,h,nl,scale", [(333, 241, 5, 0.6), (400, 300, 4, 0.5), (300, 200, 4, 0.9)])
def test_other_scales(ctx, w, h, nl, scale):
    _run_host(ctx, w, h, 3, nl, scale)


@pytest.mark.parametrize("stride", [640, 644, 641])
def test_caller_owned_level0(ctx, stride):
    """level 0 stays in the caller's device tensor: stride = w (16-byte staging), a multiple of 4 but not of 16 (dword
    staging), and an odd one (generic k_resize)"""
    import torch
    w, h, n, nl = 640, 60, 3, 4
    imgs = _batch(w, h, n)
    padded = np.full((n, h, stride), 0xAB, np.uint8)      # row padding the kernel may read but must never use
    padded[:, :, :w] = imgs
    dev = torch.from_numpy(padded).cuda()
    ex = capi.Extractor(ctx, w, h, nl, 0.8, n, 100)
    try:
        ex.set_images_dev(dev.data_ptr(), n, stride, h * stride)
        ex.build_pyramid(n)
        torch.cuda.synchronize()
        _check(ex, _expected(w, h, n, nl, 0.8), n, nl)
    finally:
        ex.close()
