"""CPU: the RGB-D restatements (tests/rgbd_cases.py) give every directed case its planted
outcome, the closed form of the close-point pass' visited count equals the literal loop, the
library declares and exports the RGB-D entry points, the host forms fail loudly without a GPU,
and extracted keypoints always truncate to a pixel inside the image (what the depth sampling's
bounds guard relies on never firing for real keypoints)."""
import ctypes
import pathlib
import re

import numpy as np
import pytest

import rgbd_cases as rc
from my_orb_slam2_amd import synth
from my_orb_slam2_amd.features import DEPTH_F32, DEPTH_U16

ROOT = pathlib.Path(__file__).resolve().parents[1]
f32 = np.float32
NEW_FUNCTIONS = ["orbx_compute_stereo_from_rgbd_batch_device", "orbx_compute_stereo_from_rgbd",
                 "orbx_rgbd_frame_geometry_batch_device", "orbx_unproject_stereo_batch_device",
                 "orbx_unproject_stereo", "orbx_close_points_batch_device", "orbx_close_points"]


def test_depth_rule_multiplies_as_the_reference_does():
    one5, one2 = rc.FACTORS["one+5e-6"], rc.FACTORS["one+2e-5"]
    assert one5 != f32(1.0) and one2 != f32(1.0)
    # f32 image, factor within 1e-5 of 1: the reference does not convert at all
    assert not rc.scales(DEPTH_F32, f32(1.0)) and not rc.scales(DEPTH_F32, one5)
    assert rc.scales(DEPTH_F32, one2) and rc.scales(DEPTH_F32, rc.TUM_FACTOR)
    # a u16 image is always converted
    assert all(rc.scales(DEPTH_U16, f) for f in rc.FACTORS.values())
    x = f32(2.7182817)
    assert rc.depth_rule(x, DEPTH_F32, one5).tobytes() == x.tobytes()
    assert rc.depth_rule(x, DEPTH_F32, one2) == f32(x * one2) != x
    assert rc.depth_rule(12345, DEPTH_U16, one5) == f32(f32(12345) * one5) != f32(12345)
    assert rc.depth_rule(5000, DEPTH_U16, rc.TUM_FACTOR) == f32(f32(5000) * rc.TUM_FACTOR)
    # denormals survive, -0.0 and NaN are not > 0
    tiny = np.nextafter(f32(0), f32(1))
    assert rc.depth_rule(tiny, DEPTH_F32, f32(1.0)) == tiny > 0
    assert not rc.depth_rule(f32(-0.0), DEPTH_F32, f32(1.0)) > 0
    assert not rc.depth_rule(f32(np.nan), DEPTH_F32, one2) > 0


def test_truncation_is_x86():
    assert rc.trunc_x86(f32(-0.5)) == 0 and rc.trunc_x86(f32(-1.0)) == -1
    assert rc.trunc_x86(np.nextafter(f32(17), f32(0))) == 16
    assert rc.trunc_x86(f32(np.nan)) == rc.INT_MIN == rc.trunc_x86(f32(3e9)) == rc.trunc_x86(f32(-3e9))


def test_depth_cases_hold_their_planted_outcomes():
    classes, styles, raws = set(), set(), {DEPTH_U16: set(), DEPTH_F32: set()}
    for c in rc.depth_cases():
        n = len(c["kps"])
        # the allocation has a spare row and column of valid depth and a padded stride
        assert c["alloc"].shape == (rc.H + 1, rc.ROW_ELEMS) and rc.ROW_ELEMS > rc.W + 1
        assert np.shares_memory(c["img"], c["alloc"]) and c["img"].shape == (rc.H, rc.W)
        ur, de = rc.compute_stereo_from_rgbd(c["img"], c["depth_type"], c["factor"], c["mbf"],
                                             c["kps"], c["kps_un"])
        assert len(ur) == len(de) == n
        for i in range(n):
            cls = c["cls"][i]
            classes.add(cls)
            styles.add(c["style"][i])
            if cls in ("oob", "invalid"):
                assert ur[i] == -1 and de[i] == -1, (c["factor_name"], i, c["style"][i])
                continue
            r, col = c["pixel"][i]
            assert (rc.trunc_x86(c["kps"]["y"][i]), rc.trunc_x86(c["kps"]["x"][i])) == (r, col)
            raws[c["depth_type"]].add(repr(c["raw"][i]))
            d = rc.depth_rule(c["img"][r, col], c["depth_type"], c["factor"])
            assert d > 0 and de[i].tobytes() == d.tobytes()
            with np.errstate(all="ignore"):
                want = f32(c["kps_un"]["x"][i] - f32(c["mbf"] / d))
            assert ur[i].tobytes() == want.tobytes()
            assert c["kps_un"]["x"][i] != c["kps"]["x"][i]
    assert classes == {"oob", "invalid", "valid"}
    assert styles == {"trunc-to-zero", "integral", "below-next", "frac"} | {n for n, _ in rc.OOB}
    # the special values reach the valid class where they are valid
    assert {"1", "65535"} <= raws[DEPTH_U16] and "0" not in raws[DEPTH_U16]
    assert {repr(f32(np.inf)), repr(f32(1e-41)), repr(np.nextafter(f32(0), f32(1)))} <= raws[DEPTH_F32]


def test_below_next_integer_truncates_to_the_pixel_before():
    c = rc.depth_case(5, DEPTH_U16, "tum", 64)
    i = c["style"].index("below-next")
    r, col = c["pixel"][i]
    assert c["kps"]["x"][i] < col + 1 and round(float(c["kps"]["x"][i])) == col + 1
    assert rc.trunc_x86(c["kps"]["x"][i]) == col


def test_unprojection_identity_pose():
    F = rc.pose(None)
    p = rc.unproject(F, F["cx"] + f32(10), F["cy"], f32(2.0))
    assert p[2] == f32(2.0) and p[1] == 0
    assert p[0] == f32(f32(f32(10) * f32(2.0)) * f32(f32(1) / F["fx"]))
    # a rotated pose: agrees with the double evaluation to float precision
    F = rc.pose(4)
    p = rc.unproject(F, 100.5, 200.25, 1.75).astype(np.float64)
    R = F["Rcw"].reshape(3, 3).astype(np.float64)
    c = np.array([(100.5 - F["cx"]) * 1.75 / F["fx"], (200.25 - F["cy"]) * 1.75 / F["fy"], 1.75])
    np.testing.assert_allclose(p, R.T @ c + F["Ow"], rtol=0, atol=2e-6)


def _literal_visited(depth, th, min_points):
    """Tracking.cc:862-912 with nothing but its control flow."""
    v = sorted((float(z), i) for i, z in enumerate(depth) if z > 0)
    n_points = visited = 0
    for z, _ in v:
        visited += 1
        n_points += 1
        if z > float(th) and n_points > min_points:
            break
    return len(v), visited


def test_visited_closed_form_equals_the_literal_loop():
    seen = set()
    for c in rc.close_cases() + [rc.close_size_case(n) for n in rc.CLOSE_SIZES[:7]]:
        M, V = _literal_visited(c["depth"], c["th"], 100)
        assert M == c["M"]
        assert V == rc.visited_closed_form(c["M"], c["L"]), c["name"]
        seen.add("break" if V < M else "all")
    assert seen == {"break", "all"}
    for seed in range(200):
        depth, th, mp = rc.random_close_frame(seed)
        M, V = _literal_visited(depth, th, mp)
        L = int(((depth > 0) & ~(depth > th)).sum())
        assert V == rc.visited_closed_form(M, L, mp), (seed, M, L, mp)


def test_close_cases_hold_their_planted_outcomes():
    names = {}
    for c in rc.close_cases():
        order, counts, create, x3d = rc.close_points_ref(c["F"], c["keys"], c["depth"], c["th"],
                                                         c["has_point"], c["tracked"])
        M, V, n_tr, n_ntr = (int(v) for v in counts)
        names[c["name"]] = (M, V, c["L"])
        assert M == c["M"] == len(order) and V == rc.visited_closed_form(M, c["L"])
        assert n_tr + n_ntr == c["n_close"]
        assert len(create) == V and x3d.shape == (V, 3)
        z = c["depth"][order]
        assert (z > 0).all() and (z[1:] >= z[:-1]).all()
        ties = np.nonzero(z[1:] == z[:-1])[0]
        assert (np.diff(order)[ties] > 0).all()          # equal z: the lower index first
        if c["has_point"] is None:
            assert create.all() and n_tr == 0
        else:
            np.testing.assert_array_equal(create, 1 - c["has_point"][order[:V]])
    assert [names[f"M={m}"][:2] for m in (0, 1, 99, 100, 101, 102)] == [
        (0, 0), (1, 1), (99, 99), (100, 100), (101, 101), (102, 101)]
    assert names["L<100<M"] == (150, 101, 50) and names["L=100"] == (150, 101, 100)
    assert names["L=101"] == (150, 102, 101) and names["L=M>100"] == (130, 130, 130)
    assert names["all-far"] == (150, 101, 0)
    # z == th_depth counts into L (no break there) but not into the close counts
    c = next(c for c in rc.close_cases() if c["name"] == "at-threshold")
    assert (c["L"], c["n_close"], names["at-threshold"][1]) == (103, 98, 104)
    # the tie runs straddle sorted position 100 / the threshold
    c = next(c for c in rc.close_cases() if c["name"] == "tie-across-100")
    z = np.sort(c["depth"][c["depth"] > 0])
    assert z[95] == z[100] == z[106] == f32(4.25) and names["tie-across-100"][1] == 101
    c = next(c for c in rc.close_cases() if c["name"] == "tie-across-th")
    assert c["L"] == 104 and c["n_close"] == 98 and names["tie-across-th"][1] == 105
    c = next(c for c in rc.close_cases() if c["name"] == "inf-denormal")
    order, *_ = rc.close_points_ref(c["F"], c["keys"], c["depth"], c["th"])
    z = c["depth"][order]
    assert 0 < z[0] == z[1] * 0 + np.nextafter(f32(0), f32(1)) and np.isinf(z[-2:]).all()
    assert names["th=inf"][0] == names["th=inf"][1] == 142


def test_positive_floats_order_as_their_bit_patterns():
    z = np.array([np.inf, 1e-41, 1.0, np.nextafter(f32(0), f32(1)), 3.0, 2.9999998, 65535.0], f32)
    assert np.array_equal(np.argsort(z, kind="stable"), np.argsort(z.view(np.uint32), kind="stable"))


def test_headers_declare_and_library_exports_the_rgbd_entry_points(orbx_lib):
    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "orbx_frame.h").read_text(), flags=re.S)
    declared = set(re.findall(r"\b(orbx_[a-z0-9_]+)\s*\(", text))
    lib = ctypes.CDLL(str(ROOT / "my_orb_slam2_amd" / "liborbx.so"))
    for name in NEW_FUNCTIONS:
        assert name in declared, name
        assert hasattr(lib, name), name
    assert re.search(r"ORBX_DEPTH_U16\s*=\s*0", text) and re.search(r"ORBX_DEPTH_F32\s*=\s*1", text)
    import my_orb_slam2_amd as m
    assert m.RGBDTrackBatch.__mro__[1] is m.MonoTrackBatch


def test_host_forms_fail_loudly_without_a_gpu(orbx_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd import features as ft
    c = rc.depth_case(1, DEPTH_U16, "tum", 8)
    with pytest.raises(m.OrbxError):
        ft.compute_stereo_from_rgbd(c["img"], c["factor"], c["mbf"], c["kps"], c["kps_un"])
    cc = rc.close_cases()[2]
    with pytest.raises(m.OrbxError):
        ft.unproject_stereo(cc["F"], cc["keys"], cc["depth"])
    with pytest.raises(m.OrbxError):
        ft.close_points(cc["F"], cc["keys"], cc["depth"], cc["th"])


def test_argument_checks_need_no_gpu(orbx_lib):
    """Refusals are decided on the host: unknown depth types and more than 8192 features."""
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd import features as ft
    c = rc.depth_case(1, DEPTH_U16, "tum", 8)
    with pytest.raises(m.OrbxError) as e:
        ft.compute_stereo_from_rgbd(c["img"], c["factor"], c["mbf"], c["kps"], c["kps_un"],
                                    depth_type=7)
    assert e.value.code == -4
    n = ft.CLOSE_MAX_FEATURES + 1
    keys = np.zeros(n, m.KEYPOINT_DTYPE)
    with pytest.raises(m.OrbxError) as e:
        ft.close_points(rc.pose(None), keys, np.ones(n, f32), 3.0)
    assert e.value.code == -4


@pytest.mark.parametrize("w,h", [(640, 480), (1241, 376), (97, 83)])
def test_extracted_keypoints_truncate_to_pixels_in_the_image(oracle_mod, w, h):
    mx = my = 0
    for seed in (1, 2, 3):
        k, _ = oracle_mod.OracleExtractor(1000, 1.2, 8, 20, 7)(synth.frame(seed, w, h))
        assert len(k) > 0
        cols = [rc.trunc_x86(v) for v in k["x"]]
        rows = [rc.trunc_x86(v) for v in k["y"]]
        assert min(cols) >= 0 and max(cols) < w and min(rows) >= 0 and max(rows) < h
        mx, my = max(mx, max(cols)), max(my, max(rows))
    print(f"{w}x{h}: largest truncated column / row {mx} / {my}")
