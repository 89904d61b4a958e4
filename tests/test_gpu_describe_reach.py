"""GPU parity of the descriptor kernel on inputs that reach its corners (pytest -m gpu): keypoint records and descriptors byte for
byte against oracle.orb_extract, on image sets whose ORACLE keypoints -- asserted here, so that no case can be left out -- take all
four sub-dword phases of the patch origin, sit 19..22 px from every level border (reflect path and both sides of the interior
boundary), rotate a tap to row +-18 and to column +-18, and lie over saturated and all-zero regions (tests/describe_reach_cases.py).
Both launch orders of k_describe: fewer than 64 images, and 66 tiled images (an image per XCD at a time)."""
import numpy as np
import pytest

import oracle
from trackingbench_slam_amd import capi
import describe_reach_cases as dc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs():
    """name -> (images, [(keypoints, descriptors)]): the oracle's output per distinct image, computed once, coverage asserted."""
    out = {}
    for name, (w, h, seeds) in dc.SETS.items():
        imgs, lvs, res = [], [], []
        for s in seeds:
            img = dc.image(s, w, h)
            lv, sf = oracle.pyramid(img, dc.NLEVELS, dc.SCALE)
            k, d, _ = oracle.orb_extract(lv, sf, dc.TARGET, dc.INI_TH, dc.MIN_TH)
            imgs.append(img); lvs.append(lv); res.append((k, d))
        dc.check_coverage(dc.coverage(lvs, sf, [k for k, _ in res]))
        out[name] = (imgs, res)
    return out


def _eq_struct(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.shape, b.shape)
    for f in a.dtype.names:
        assert np.array_equal(a[f], b[f]), f


@pytest.mark.parametrize("n", [3, 66])
@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_describe_matches_oracle_byte_for_byte(ctx, refs, name, n):
    w, h, _ = dc.SETS[name]
    distinct, res = refs[name]
    imgs = np.stack([distinct[i % len(distinct)] for i in range(n)])
    ex = capi.Extractor(ctx, w, h, dc.NLEVELS, dc.SCALE, n, dc.TARGET)
    assert ex.set_images_host(imgs) == n
    ex.build_pyramid(n)
    ex.orb(n, dc.TARGET, dc.INI_TH, dc.MIN_TH)
    cnt = ex.counts(n)
    for b in range(n):
        ko, do = res[b % len(distinct)]
        k, d = ex.results(b)
        assert cnt[b] == len(ko)
        _eq_struct(k, ko)
        assert np.array_equal(d, do), (b, int((d != do).any(axis=1).sum()))
    ex.close()


@pytest.mark.parametrize("name", sorted(dc.SETS))
def test_describe_single_frame_entry_matches_oracle(ctx, refs, name):
    """tb_orb_extract on caller-owned levels: tight rows, so the odd width's levels come with strides that are no multiple of 4."""
    distinct, res = refs[name]
    for img, (ko, do) in zip(distinct, res):
        lv, sf = oracle.pyramid(img, dc.NLEVELS, dc.SCALE)
        k, d, _ = ctx.orb_extract(lv, sf, dc.TARGET, dc.INI_TH, dc.MIN_TH)
        _eq_struct(k, ko)
        assert np.array_equal(d, do)
