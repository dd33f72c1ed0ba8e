"""The speckle filter's definition (tests/speckle_model.py) against an independent scalar restatement - cv::filterSpeckles as
OpenCV walks it: raster order, an explicit stack, in place - and against known answers.  No GPU."""
import numpy as np
import pytest

import speckle_model as M


def scalar_filter_speckles(img, new_val, max_size, max_diff):
    """filterSpeckles on a copy, the way OpenCV's flood fill goes: pixels in raster order; an unlabelled pixel that is not new_val
    starts a region and grows it over 4-neighbours that are not new_val, are unlabelled and differ from the pixel they are reached
    from by at most max_diff; a region of at most max_size pixels is marked small and its seed is rewritten at once, and a pixel
    met later whose label is a small region's is rewritten when the walk reaches it.  -> (filtered, sizes per pixel)."""
    img = np.array(img, dtype=np.int16, copy=True)
    H, W = img.shape
    labels = np.zeros((H, W), np.int64)
    small = {}                                      # region label -> bool
    count = {}
    cur = 0
    for i in range(H):
        for j in range(W):
            if int(img[i, j]) == new_val:
                continue
            if labels[i, j]:
                if small[labels[i, j]]:
                    img[i, j] = new_val
                continue
            cur += 1
            labels[i, j] = cur
            stack, n = [(i, j)], 0
            while stack:
                y, x = stack.pop()
                n += 1
                d = int(img[y, x])
                for yy, xx in ((y, x + 1), (y, x - 1), (y + 1, x), (y - 1, x)):
                    if 0 <= yy < H and 0 <= xx < W and not labels[yy, xx]:
                        e = int(img[yy, xx])
                        if e != new_val and abs(e - d) <= max_diff:
                            labels[yy, xx] = cur
                            stack.append((yy, xx))
            count[cur] = n
            small[cur] = n <= max_size
            if small[cur]:
                img[i, j] = new_val
    sizes = np.zeros((H, W), np.int32)
    for i in range(H):
        for j in range(W):
            if labels[i, j]:
                sizes[i, j] = count[labels[i, j]]
    return img, sizes


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("seed", range(6))
@pytest.mark.parametrize("max_diff", [0, 1, 16, 40])
def test_model_equals_the_raster_order_flood_fill(seed, max_diff):
    rng = np.random.default_rng(seed)
    H, W = int(rng.integers(1, 24)), int(rng.integers(1, 40))
    levels = np.array([-16, 0, 16, 17, 48, 300], np.int16)[: int(rng.integers(2, 7))]
    img = levels[rng.integers(0, levels.size, (H, W))]
    for new_val in (-16, 16):
        for max_size in (0, 1, 3, 10, H * W):
            got = M.filter_speckles(img, new_val, max_size, max_diff)
            want = scalar_filter_speckles(img, new_val, max_size, max_diff)
            assert same(got[0], want[0]) and same(got[1], want[1]), (H, W, new_val, max_size, max_diff)


def test_chain_connects_through_its_middle():
    img = np.array([[0, 512, 1024]], np.int16)
    out, sizes = M.filter_speckles(img, -16, 2, 512)
    assert sizes.tolist() == [[3, 3, 3]] and same(out, img)
    out, sizes = M.filter_speckles(img, -16, 3, 512)
    assert out.tolist() == [[-16, -16, -16]]
    out, sizes = M.filter_speckles(img, -16, 1, 511)
    assert sizes.tolist() == [[1, 1, 1]] and out.tolist() == [[-16, -16, -16]]


def test_exactly_max_size_goes_one_more_stays():
    img = np.full((5, 9), -16, np.int16)
    img[1, 1:5] = 32                               # 4 pixels
    img[3, 1:6] = 32                               # 5 pixels
    out, sizes = M.filter_speckles(img, -16, 4, 0)
    assert (out[1] == -16).all() and (out[3, 1:6] == 32).all()
    assert sizes[1, 1:5].tolist() == [4] * 4 and sizes[3, 1:6].tolist() == [5] * 5 and sizes.sum() == 16 + 25


def test_int16_extremes_do_not_wrap():
    img = np.array([[32767, -32768], [-32768, 32767]], np.int16)
    for md in (0, 1, 32767, 65534):
        out, sizes = M.filter_speckles(img, 0, 0, md)
        assert (sizes == 1).all() and same(out, img)
    assert (M.filter_speckles(img, 0, 0, 65535)[1] == 4).all()


def test_all_new_val_and_max_size_zero():
    img = np.full((7, 11), -16, np.int16)
    out, sizes = M.filter_speckles(img, -16, 100, 512)
    assert same(out, img) and not sizes.any()
    rng = np.random.default_rng(1)
    img = rng.integers(-20, 20, (13, 17)).astype(np.int16)
    out, sizes = M.filter_speckles(img, -16, 0, 3)
    assert same(out, img) and ((sizes > 0) == (img != -16)).all()


def test_sgbm_parameters():
    img = np.full((4, 4), 160, np.int16)
    assert M.sgbm_speckle(img, 0, 32)[1] is None and same(M.sgbm_speckle(img, 0, 32)[0], img)
    assert (M.sgbm_speckle(img, 16, 0)[0] == -16).all() and same(M.sgbm_speckle(img, 15, 0)[0], img)


# computed from tests/golden/{cones,teddy}_sgm.npz["disp"] with the reference's (-16, 100, 512)
@pytest.mark.parametrize("name,ncomp,largest,removed", [("cones", 104, 152415, 759), ("teddy", 279, 149420, 1674)])
def test_goldens(golden, name, ncomp, largest, removed):
    disp = golden(f"{name}_sgm.npz")["disp"]
    lab, n = M.components(disp, -16, 512)
    out, sizes = M.filter_speckles(disp, -16, 100, 512)
    assert n == ncomp
    assert int(sizes.max()) == largest
    assert int(np.count_nonzero(out != disp)) == removed
    assert ((out == disp) | (out == -16)).all() and ((sizes > 0) == (disp != -16)).all()
