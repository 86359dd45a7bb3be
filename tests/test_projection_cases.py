"""CPU: the projection loops of the six projection searches orbx_project_map_points* runs
(tests/projection_cases.py).  The numpy restatement against the cv::Mat restatement of
tests/native/project_ref.cpp, bit for bit, on every directed and random case of every mode; the
census of what the cases contain; every single-decision variant of the restatement changes a
case; the C ABI's argument checks, which need no GPU."""
import ctypes
import subprocess

import numpy as np
import pytest

import projection_cases as pc
from my_orb_slam2_amd.features import (PROJ_FUSE, PROJ_JOB_DTYPE, PROJ_KEYFRAME, PROJ_KF_SCW,
                                       PROJ_LAST_FRAME, PROJ_QUERY_DTYPE, PROJ_SIM3)

f32 = np.float32
MODE_IDS = [pc.MODE_NAMES[m] for m in pc.MODES]


@pytest.fixture(scope="module")
def project_ref():
    from my_orb_slam2_amd import build as b
    return b.build_project_ref()


def run_ref(binary, cases, tmp_path):
    """The C++ restatement on a list of cases -> [(queries, nactive)]."""
    src, dst = tmp_path / "cases.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for c in cases:
            n = len(c["mps"])
            f.write(np.array([c["mode"], n, c["keys"] is not None, c["skip"] is not None],
                             np.int32).tobytes())
            f.write(np.asarray(c["job"], PROJ_JOB_DTYPE).tobytes())
            f.write(c["mps"].tobytes())
            if c["keys"] is not None:
                f.write(c["keys"].tobytes())
            if c["skip"] is not None:
                f.write(c["skip"].tobytes())
    subprocess.run([str(binary), str(src), str(dst)], check=True, timeout=120)
    raw = dst.read_bytes()
    out, o = [], 0
    for c in cases:
        n = len(c["mps"])
        q = np.frombuffer(raw, PROJ_QUERY_DTYPE, n, o)
        o += 32 * n
        out.append((q, int(np.frombuffer(raw, np.int32, 1, o)[0])))
        o += 4
    assert o == len(raw)
    return out


def test_job_record_layout():
    assert PROJ_JOB_DTYPE.itemsize == 240 and PROJ_JOB_DTYPE.itemsize % 16 == 0
    assert PROJ_JOB_DTYPE.fields["pre_R"][1] == 168 and PROJ_JOB_DTYPE.fields["th"][1] == 220


@pytest.mark.parametrize("mode", pc.MODES, ids=MODE_IDS)
def test_numpy_equals_cv_mat_restatement(project_ref, tmp_path, mode):
    cases = pc.all_cases(mode)
    assert all(len(c["mps"]) <= 300 for c in cases if "random" not in c["name"])
    for c, (q_ref, n_ref) in zip(cases, run_ref(project_ref, cases, tmp_path)):
        q, n, _ = pc.reference(c)
        bad = np.nonzero((q.view(np.uint8).reshape(-1, 32) != q_ref.view(np.uint8).reshape(-1, 32)).any(1))[0]
        assert bad.size == 0, f"{c['name']}: queries differ at points {bad[:8]}"
        assert n == n_ref == int((q["radius"] >= 0).sum()), c["name"]


def _census(mode):
    out = dict(outcome=set(), window=set(), clamp=set())
    for c in pc.all_cases(mode):
        _, _, info = pc.reference(c)
        for k in out:
            out[k] |= set(info[k])
    return out


@pytest.mark.parametrize("mode", pc.MODES, ids=MODE_IDS)
def test_census_every_outcome_occurs(mode):
    cen = _census(mode)
    assert cen["outcome"] >= set(pc.outcomes_of(mode)), set(pc.outcomes_of(mode)) - cen["outcome"]
    assert cen["outcome"] <= set(pc.outcomes_of(mode))
    if mode == PROJ_LAST_FRAME:
        assert cen["window"] >= set(pc.WINDOWS)
    else:
        assert cen["clamp"] >= set(pc.CLAMPS)
    # the random scenes alone reach every outcome too
    rnd = set()
    for c in pc.random_cases(mode):
        rnd |= set(pc.reference(c)[2]["outcome"])
    assert rnd >= set(pc.outcomes_of(mode)), set(pc.outcomes_of(mode)) - rnd


def _case(mode, name):
    (c,) = [c for c in pc.all_cases(mode) if c["name"].endswith("/" + name)]
    return c, pc.reference(c)


@pytest.mark.parametrize("mode", pc.MODES, ids=MODE_IDS)
def test_census_named_constructs(mode):
    frame = mode in pc.FRAME_MODES
    # bounds: both ends and one float either side; a Frame keeps both ends, IsInImage drops max
    c, (q, _, info) = _case(mode, "bounds")
    u, v, act = info["u"], info["v"], np.array(info["outcome"]) == "active"
    up = lambda a: np.nextafter(f32(a), f32(np.inf))
    dn = lambda a: np.nextafter(f32(a), f32(-np.inf))
    assert [float(x) for x in u[:6]] == [float(x) for x in (dn(64), 64, up(64), dn(320), 320, up(320))]
    assert [float(x) for x in v[6:12]] == [float(x) for x in (dn(32), 32, up(32), dn(288), 288, up(288))]
    assert act[:6].tolist() == [False, True, True, True, frame, False]
    assert act[6:12].tolist() == [False, True, True, True, frame, False]
    assert info["outcome"][0] == "bounds_u" and info["outcome"][6] == "bounds_v"

    # depth values
    c, (q, _, info) = _case(mode, "depth")
    z, out = info["z"], info["outcome"]
    negzero = (z == 0) & np.signbit(z)
    poszero = (z == 0) & ~np.signbit(z)
    assert negzero.any() and poszero.any() and np.isnan(z).any()
    assert (z < 0).sum() >= 4 and ((z < 0) & (z > -1e-20)).any()
    i = int(np.nonzero(negzero)[0][0])
    if mode == PROJ_LAST_FRAME:
        assert out[i] == "depth"                       # invz = -inf
        j = int(np.nonzero(poszero)[0][0])             # xc = 0: NaN u passes the Frame bounds
        assert out[j] == "active" and np.isnan(q["u"][j])
    elif mode == PROJ_KEYFRAME:
        neg_in = [k for k in range(len(z)) if z[k] < 0 and out[k] == "active"]
        assert neg_in, "KEYFRAME: a negative z in bounds stays active"
    else:
        assert out[i] == "bounds_u"                    # passes z < 0, fails IsInImage
        assert all(out[k] == "depth" for k in range(len(z)) if z[k] < 0)
    tz = [pc.reference(c)[2]["z"] for c in pc.all_cases(mode) if "/depth_tz" in c["name"]]
    assert len(tz) == 6 and any(((a == 0) & np.signbit(a)).any() for a in tz)
    # (SIM3's two gemms turn an infinite P.z into NaN; tcw.z = inf reaches an infinite depth)
    assert any(np.isposinf(a).any() for a in tz) and any(np.isnan(a).all() for a in tz)

    if mode != PROJ_LAST_FRAME:
        # d at 0.8f*min / 1.2f*max and one float outside
        c, (q, _, info) = _case(mode, "range")
        d, out, m = info["d"], info["outcome"], c["mps"]
        lo, hi = f32(0.8) * m["min_dist"], f32(1.2) * m["max_dist"]
        eq_lo, eq_hi = np.nonzero(d == lo)[0], np.nonzero(d == hi)[0]
        assert len(eq_lo) >= 3 and len(eq_hi) >= 3
        assert all(out[k] not in ("range_low", "range_high") for k in list(eq_lo) + list(eq_hi))
        assert any(d[k] == dn(lo[k]) and out[k] == "range_low" for k in range(len(d)))
        assert any(d[k] == up(hi[k]) and out[k] == "range_high" for k in range(len(d)))
        # PredictScale
        for nl in (1, 8, 16):
            c, (q, _, info) = _case(mode, f"predict_scale_nl{nl}")
            assert "below" in info["clamp"] and "above" in info["clamp"]
            assert nl == 1 or "inside" in info["clamp"]
            assert q["pred_level"].max() == nl - 1
            k = int(np.nonzero(np.isnan(c["mps"]["max_dist"]))[0][0])      # NaN ratio -> INT_MIN -> 0
            assert info["outcome"][k] == "active" and q["pred_level"][k] == 0 and info["clamp"][k] == "below"
        c, (q, _, info) = _case(mode, "predict_scale_1.2")
        assert q["pred_level"][:3].tolist() == [1, 0, 7]       # quotient exactly 1, exactly 0, far above
        assert sorted(set(q["pred_level"][3:].tolist())) == list(range(8))
    if mode in pc.NORMAL_MODES:
        c, (q, _, info) = _case(mode, "normal")
        dot, d, out = info["dot"], info["d"], info["outcome"]
        assert dot[0] == 0.5 * float(d[0]) and out[0] == "active"
        assert dot[1] == np.nextafter(2.0, 0.0) and d[1] == 4 and out[1] == "normal"
        assert f32(dot[1]) == f32(0.5) * d[1]          # float32 would keep it
    if mode == PROJ_LAST_FRAME:
        want = {"tlc==mb": "default", "tlc>mb": "forward", "-tlc==mb": "default",
                "-tlc>mb": "backward", "mono_fwd": "default", "mono_bwd": "default",
                "tlc_nan": "default", "tlc0": "default"}
        for name, kind in want.items():
            c, (q, _, info) = _case(mode, "window_" + name)
            assert set(info["window"]) == {kind}, name
            o = c["keys"]["octave"]
            exp = {"default": (o - 1, o + 1), "forward": (o, 0 * o - 1), "backward": (0 * o, o)}[kind]
            assert (q["min_level"] == exp[0]).all() and (q["max_level"] == exp[1]).all()
            assert (q["pred_level"] == o).all() and (q["angle"] == c["keys"]["angle"]).all()
        c, (q, _, info) = _case(mode, "window_tlc==mb")
        assert q["min_level"][0] == -1 and info["tlc_z"] == f32(0.5)
        c, (q, _, info) = _case(mode, "octaves_nl16")
        assert q["pred_level"].tolist() == list(range(16))
    # th and the skip flags
    for th in (1, 3, 7, 10, 15):
        c, (q, n, _) = _case(mode, f"th{th}")
        assert n == 8
        assert (q["radius"] == f32(th) * c["job"]["cam"]["scale"][q["pred_level"]]).all()
    c, (q, n, info) = _case(mode, "skip")
    sk = c["skip"].astype(bool)
    assert (np.array(info["outcome"])[sk] == "skipped").all() and (q["radius"][sk] == -1).all()
    assert (q["radius"][~sk] > 0).all() and n == int((~sk).sum())
    for nl in (0, 17, -3):
        c, (q, n, _) = _case(mode, f"nlevels{nl}")
        assert n == 0 and (q["radius"] == -1).all()
    # the query conventions of the mode
    c, (q, _, _) = _case(mode, "th3")
    if mode == PROJ_KEYFRAME:
        assert (q["min_level"] == q["pred_level"] - 1).all() and (q["max_level"] == q["pred_level"] + 1).all()
    elif mode != PROJ_LAST_FRAME:
        assert (q["min_level"] == -1).all() and (q["max_level"] == -1).all() and (q["angle"] == 0).all()
    assert (q["ur"] != 0).all() if mode in pc.UR_MODES else (q["ur"] == 0).all()


@pytest.mark.parametrize("variant", sorted(pc.VARIANTS))
def test_every_variant_changes_a_case(variant):
    """Each decision of the restatement is pinned: switching it changes at least one case of
    every mode it applies to."""
    for mode in pc.VARIANTS[variant]:
        changed = []
        for c in pc.all_cases(mode):
            if "random11" in c["name"]:
                continue                       # one random scene is enough here
            q, _, _ = pc.reference(c)
            qv, _, _ = pc.project_np(mode, c["job"], c["mps"], c["keys"], c["skip"], variant)
            if q.tobytes() != qv.tobytes():
                changed.append(c["name"])
        assert changed, f"{variant} changes nothing in {pc.MODE_NAMES[mode]}"


def test_directed_variant_pins():
    """The directed cases, not only the random ones, pin the decisions they were built for."""
    def differs(mode, name, variant):
        c, (q, _, _) = _case(mode, name)
        return q.tobytes() != pc.project_np(mode, c["job"], c["mps"], c["keys"], c["skip"], variant)[0].tobytes()
    for mode in pc.FRAME_MODES:
        assert differs(mode, "bounds", "frame_min_strict") and differs(mode, "bounds", "frame_max_strict")
        assert differs(mode, "th3", "max_level_L") or mode == PROJ_LAST_FRAME
    for mode in (PROJ_KF_SCW, PROJ_FUSE, PROJ_SIM3):
        assert differs(mode, "bounds", "kf_min_strict") and differs(mode, "bounds", "kf_max_inclusive")
    for mode in pc.MODES:
        assert differs(mode, "depth", "depth_flip"), pc.MODE_NAMES[mode]
    for mode in pc.NORMAL_MODES:
        assert differs(mode, "normal", "dot_f32") and differs(mode, "normal", "half_d_f32")
    assert differs(PROJ_LAST_FRAME, "window_tlc==mb", "threshold_nonstrict")
    assert differs(PROJ_LAST_FRAME, "window_-tlc==mb", "threshold_nonstrict")
    assert differs(PROJ_LAST_FRAME, "window_tlc>mb", "windows_swapped")
    assert differs(PROJ_LAST_FRAME, "window_tlc0", "max_level_L")


# ---- the C ABI without a GPU --------------------------------------------------------------------

def _abi_args(n=4):
    job = pc.exact_job(PROJ_FUSE)
    mps = np.zeros(n, pc.MAP_POINT_DTYPE)
    keys = np.zeros(n, pc.KEYPOINT_DTYPE)
    q = np.zeros(n, PROJ_QUERY_DTYPE)
    return job, mps, keys, q


def test_symbols_and_argument_statuses_need_no_gpu(orbx_lib):
    """ORBX_ERR_INVALID is decided before the device is touched."""
    L = orbx_lib
    assert hasattr(L, "orbx_project_map_points") and hasattr(L, "orbx_project_map_points_batch_device")
    job, mps, keys, q = _abi_args()
    P = lambda a: ctypes.c_void_p(a.ctypes.data)
    na = ctypes.c_int32(-5)
    host = lambda mode, n, k: L.orbx_project_map_points(mode, P(job), P(mps), n, k, None, P(q),
                                                        ctypes.byref(na), 0)
    for bad in (0, 7, -1, 100):                       # FRAME_MAPPOINTS is orbx_is_in_frustum's
        assert host(bad, 4, P(keys)) == -1
        assert L.orbx_project_map_points_batch_device(bad, P(job), 1, P(mps), P(mps), 4, P(keys),
                                                      None, P(q), None, None) == -1
    for mode in (PROJ_LAST_FRAME, PROJ_KEYFRAME):     # src_keys is required
        assert host(mode, 4, None) == -1
        assert L.orbx_project_map_points_batch_device(mode, P(job), 1, P(mps), P(mps), 4, None,
                                                      None, P(q), None, None) == -1
    assert host(PROJ_FUSE, (1 << 24) + 1, None) == -1     # more than 1 << 24 points
    assert host(PROJ_FUSE, -1, None) == -1
    assert L.orbx_project_map_points_batch_device(PROJ_FUSE, P(job), 1, P(mps), P(mps),
                                                  (1 << 24) + 1, None, None, P(q), None, None) == -1
    assert L.orbx_project_map_points_batch_device(PROJ_FUSE, P(job), 65536, P(mps), P(mps), 4,
                                                  None, None, P(q), None, None) == -1
    assert L.orbx_project_map_points_batch_device(       # records move as 16-byte accesses
        PROJ_FUSE, P(job), 1, ctypes.c_void_p(mps.ctypes.data + 4), P(mps), 3, None, None, P(q),
        None, None) == -1
    assert L.orbx_project_map_points(PROJ_FUSE, None, P(mps), 4, None, None, P(q), None, 0) == -1
    assert L.orbx_project_map_points(PROJ_FUSE, P(job), None, 4, None, None, P(q), None, 0) == -1
    # nothing to do: no device needed either
    assert host(PROJ_SIM3, 0, None) == 0 and na.value == 0
    assert L.orbx_project_map_points_batch_device(PROJ_SIM3, None, 0, None, None, 0, None, None,
                                                  None, None, None) == 0


def test_without_gpu_the_host_form_fails_loudly(orbx_lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    import my_orb_slam2_amd as m
    job, mps, keys, _ = _abi_args()
    with pytest.raises(m.OrbxError) as e:
        m.project_map_points(m.PROJ_SIM3, job, mps)
    assert e.value.code == -2     # ORBX_ERR_DEVICE
