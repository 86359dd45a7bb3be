"""CPU: the two numpy restatements of cv::remap agree on every directed case, the weight-table
claims behind the closed form hold by exhaustion, the directed constructs all occur, and the host
helpers of include/orbx_frame.h (orbx_remap_fixed_point, orbx_init_undistort_rectify_map) equal
the restatements bit for bit (tests/remap_cases.py)."""
import ctypes
import pathlib

import numpy as np
import pytest

import remap_cases as rc

ROOT = pathlib.Path(__file__).resolve().parents[1]
EUROC_YAML = str(ROOT / "tests" / "golden" / "euroc_stereo.yaml")


@pytest.fixture(scope="module")
def cases(orbx_lib):
    from my_orb_slam2_amd import rectify
    chunk = rectify.images_per_chunk()
    assert chunk >= 1
    pairs = rc.build_stereo_cases(chunk)
    return rc.build_cases(chunk) + [c for p in pairs for c in p]


def test_literal_equals_closed(cases):
    stats = {}
    for c in cases:
        lit = rc.remap_literal(c["src"], c["map1"], c["map2"], stats)
        assert np.array_equal(lit, rc.remap_closed(c["src"], c["map1"], c["map2"])), c["name"]
    assert stats.get("inlier", 0) > 0 and stats.get("border", 0) > 0, stats


def test_specials_give_zero(cases):
    c = next(c for c in cases if c["name"] == "specials")
    assert c["src"].min() > 0
    assert not rc.remap_closed(c["src"], c["map1"], c["map2"]).any()


def test_entry_00_returns_v00():
    """(32767 * p + q + 16384) >> 15 == p for all bytes p, q: entry (0, 0), whose weight 32768
    saturates to 32767, gives v00 wherever the fix-up puts the missing 1."""
    tab = rc.weight_table()
    assert tab[0].max() == 32767 and tab[0].sum() == 32768 and sorted(tab[0])[:3] == [0, 0, 1]
    p, q = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64))
    assert np.array_equal((32767 * p + q + 16384) >> 15, p)


def test_weight_table_is_32_times_the_integer_product():
    tab = rc.weight_table()
    for b in range(32):
        for a in range(32):
            if (a, b) == (0, 0):
                continue
            want = [32 * (32 - a) * (32 - b), 32 * a * (32 - b), 32 * (32 - a) * b, 32 * a * b]
            assert list(tab[b * 32 + a]) == want, (a, b)


def test_census(cases):
    cn = rc.census(cases)
    must = ["inlier", "border_path", "X=-1", "X=sw-1", "Y=-1", "Y=sh-1", "X=-2", "X=sw", "Y=sh",
            "corner_tl", "corner_tr", "corner_bl", "corner_br", "all_outside", "partial",
            "neg_shift_a31", "nan", "+inf", "-inf", "1e+09", "-1e+09", "3e+09", f"{2.0 ** 26:g}",
            "40000", "sum%1024==0", "sum%1024==1023", "sum%1024==512", "sum%1024==511",
            "batch1", "batch2", "batch3", "batchchunk+", "src!=dst", "src_pad", "dst_stride%4",
            "dst_odd_base", "image_gap", "src1x1", "src2x2"]
    must += [k for k in cn if k.startswith("tie")]
    assert len([k for k in cn if k.startswith("tie")]) == 4
    must += [f"w{w}" for w in rc.WIDTHS] + [f"h{h}" for h in rc.HEIGHTS]
    missing = [k for k in must if cn.get(k, 0) <= 0]
    assert not missing, (missing, cn)
    # all 1024 (a, b) pairs
    c = next(c for c in cases if c["name"] == "ab_grid")
    _, _, a, b = rc.fixed_point_np(c["map1"], c["map2"])
    assert len(set((b * 32 + a).ravel().tolist())) == 1024


def test_census_of_kernel_forms(cases):
    """Both forms of k_remap (the 8-column x 3-row window and the byte gather) and each side of
    every limit between them occur in the directed cases."""
    tot = {}
    for c in cases:
        for k, v in rc.group_forms(c).items():
            tot[k] = tot.get(k, 0) + v
    missing = [k for k, v in tot.items() if v <= 0]
    assert not missing, (missing, tot)


def test_fixed_point_helper_equals_numpy(cases):
    from my_orb_slam2_amd import rectify
    for c in cases:
        xy, a = rectify.remap_fixed_point(c["map1"], c["map2"])
        xy_o, a_o = rc.fixed_point_cv(c["map1"], c["map2"])
        assert np.array_equal(xy, xy_o) and np.array_equal(a, a_o), c["name"]
        # the scalar and the vectorised restatement agree too
        X, Y, aa, bb = rc.fixed_point_np(c["map1"], c["map2"])
        for (y, x) in ((0, 0), (-1, -1)):
            assert rc.fixed_point_scalar(c["map1"][y, x], c["map2"][y, x]) == \
                (X[y, x], Y[y, x], aa[y, x], bb[y, x])


def _bits(m):
    return np.ascontiguousarray(m, np.float32).view(np.uint32)


@pytest.mark.parametrize("side", ["left", "right"])
def test_init_map_euroc(orbx_lib, side):
    from my_orb_slam2_amd import rectify
    ml, mr, s = rc.euroc_maps(EUROC_YAML)
    want = ml if side == "left" else mr
    c = s[side]
    assert (c["width"], c["height"]) == (rc.EUROC_W, rc.EUROC_H)
    m1, m2 = rectify.init_undistort_rectify_map(c["K"], c["D"], c["R"], c["P"], c["width"],
                                                c["height"])
    assert np.array_equal(_bits(m1), _bits(want[0])) and np.array_equal(_bits(m2), _bits(want[1]))


@pytest.mark.parametrize("ndist", [4, 5, 8])
@pytest.mark.parametrize("with_r", [False, True])
def test_init_map_variants(orbx_lib, ndist, with_r):
    from my_orb_slam2_amd import rectify
    K = [[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]]
    D = [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0123, 0.011, -0.02, 0.003][:ndist]
    R = [[0.999966347530033, -0.001422739138722922, 0.008079580483432283],
         [0.001365741834644127, 0.9999741760894847, 0.007055629199258132],
         [-0.008089410156878961, -0.007044357138835809, 0.9999424675829176]] if with_r else None
    P = [[435.2, 0, 367.45, -47.9], [0, 436.1, 252.2, 0], [0, 0, 1, 0]]
    w1, w2 = rc.init_map_np(K, D, R, P, 97, 33)
    m1, m2 = rectify.init_undistort_rectify_map(K, D, R, P, 97, 33)
    assert np.array_equal(_bits(m1), _bits(w1)) and np.array_equal(_bits(m2), _bits(w2))


def test_init_map_refuses_thin_prism(orbx_lib):
    from my_orb_slam2_amd import OrbxError, rectify
    with pytest.raises(OrbxError) as e:
        rectify.init_undistort_rectify_map(np.eye(3), np.zeros(12), None, np.eye(3), 8, 8)
    assert e.value.code == -4     # ORBX_ERR_UNSUPPORTED


def test_load_stereo_settings():
    from my_orb_slam2_amd.rectify import load_stereo_settings
    s = load_stereo_settings(EUROC_YAML)
    assert s["bf"] == 47.90639384423901 and s["fx"] == 435.2046959714599
    L, R = s["left"], s["right"]
    assert (L["width"], L["height"], R["width"], R["height"]) == (752, 480, 752, 480)
    assert L["K"].tolist() == [[458.654, 0.0, 367.215], [0.0, 457.296, 248.375], [0.0, 0.0, 1.0]]
    assert L["D"].tolist() == [-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.0]
    assert R["D"].tolist() == [-0.28368365, 0.07451284, -0.00010473, -3.555907e-05, 0.0]
    assert R["K"].tolist() == [[457.587, 0.0, 379.999], [0.0, 456.134, 255.238], [0.0, 0.0, 1.0]]
    assert L["R"][0].tolist() == [0.999966347530033, -0.001422739138722922, 0.008079580483432283]
    assert R["R"][2].tolist() == [-0.007729688520722713, 0.007064130529506649, 0.999945173484644]
    assert L["P"].shape == (3, 4) and R["P"].shape == (3, 4)
    assert R["P"][0].tolist() == [435.2046959714599, 0.0, 367.4517211914062, -47.90639384423901]
    assert L["P"][1].tolist() == [0.0, 435.2046959714599, 252.2008514404297, 0.0]


def test_euroc_maps_touch_the_border_on_the_right_only_partially():
    ml, mr, _ = rc.euroc_maps(EUROC_YAML)
    partial = {}
    for name, (m1, m2) in (("left", ml), ("right", mr)):
        X, Y, _, _ = rc.fixed_point_np(m1, m2)
        okx = [(X + o >= 0) & (X + o < rc.EUROC_W) for o in (0, 1)]
        oky = [(Y + o >= 0) & (Y + o < rc.EUROC_H) for o in (0, 1)]
        ntaps = sum((ox & oy).astype(int) for ox in okx for oy in oky)
        assert (ntaps > 0).all(), f"{name}: a pixel lies entirely outside the source"
        partial[name] = int(((ntaps > 0) & (ntaps < 4)).sum())
    assert partial["right"] >= 1, partial


def test_rectifier_without_gpu_fails_loudly(orbx_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import my_orb_slam2_amd as m
    ident = np.zeros((4, 4), np.float32)
    with pytest.raises(m.OrbxError) as e:
        m.Rectifier(ident, ident)
    assert e.value.code == -2     # ORBX_ERR_DEVICE


def test_rectifier_argument_statuses_need_no_gpu(orbx_lib):
    """ORBX_ERR_INVALID / ORBX_ERR_UNSUPPORTED are decided before the device is touched."""
    h = ctypes.c_void_p()
    m = np.zeros((2, 2), np.float32)
    p = ctypes.c_void_p(m.ctypes.data)
    L = orbx_lib
    assert L.orbx_rectifier_create(None, p, 2, 2, 2, 2, 0, ctypes.byref(h)) == -1
    assert L.orbx_rectifier_create(p, p, 0, 2, 2, 2, 0, ctypes.byref(h)) == -1
    assert L.orbx_rectifier_create(p, p, 2, 2, 2, -1, 0, ctypes.byref(h)) == -1
    assert L.orbx_rectifier_create(p, p, 2, 2, 32768, 2, 0, ctypes.byref(h)) == -4
    assert L.orbx_rectifier_create(p, p, 2, 2, 2, 32768, 0, ctypes.byref(h)) == -4
    assert L.orbx_remap_batch_device(None, p, 2, 4, p, 2, 4, 1, None) == -1
    assert L.orbx_remap(None, p, 2, p, 2) == -1
