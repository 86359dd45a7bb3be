"""Frame::isInFrustum + MapPoint::PredictScale (src/Frame.cc:285-349, MapPoint.cc:430-444) and
the SearchByProjection window built from them (ORBmatcher.cc:55-80): the projection half of
Tracking::SearchLocalPoints (Tracking.cc:1297-1347).

CPU: the C++ restatement (oracle/orb_frame_oracle.cpp) against a second, numpy restatement of
the same statements; the synthetic local map exercises every rejection.  GPU: k_frustum
(orbx_is_in_frustum / _batch_device) bit for bit against the C++ restatement, one frame and the
256-frame EuRoC batch bench.py --workload euroc times."""
import ctypes
import math

import numpy as np
import pytest

from frame_cases import numpy_is_in_frustum
from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import MAP_POINT_DTYPE, PROJ_QUERY_DTYPE, frame_pose

_libm = ctypes.CDLL("libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
_libm.ceilf.restype = ctypes.c_float
_libm.ceilf.argtypes = [ctypes.c_float]
f32 = np.float32


def _keys(seed, n=800, w=752, h=480):
    rng = np.random.default_rng(seed)
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"] = rng.uniform(20, w - 20, n)
    k["y"] = rng.uniform(20, h - 20, n)
    k["octave"] = rng.integers(0, 8, n)
    return k, rng.integers(0, 256, (n, 32), dtype=np.uint8)


def _scene(seed, n=2000):
    K4, _ = synth.EUROC_CAM
    bounds = (0.0, 752.0, 0.0, 480.0)
    keys, desc = _keys(seed)
    return synth.local_map_points(seed, keys, desc, n, K4, bounds, mbf=40.0)


def test_log_scale_factor_is_glibc_logf():
    F = frame_pose(np.eye(3), np.zeros(3), (1, 1, 0, 0), (0, 1, 0, 1), np.ones(8))
    assert F["log_scale_factor"] == _libm.logf(f32(1.2))


@pytest.mark.parametrize("seed", [3, 11])
def test_oracle_matches_numpy_restatement(oracle_mod, seed):
    from oracle import matcher as om
    F, mps, _, skip = _scene(seed, 600)
    qo, no = om.is_in_frustum(F, mps, skip)
    qn, nn = numpy_is_in_frustum(F, mps, skip)
    assert no == nn
    assert qo.tobytes() == qn.tobytes()
    # every kind of outcome occurs: both radii, several levels, rejections and skips
    qv = qo.view(PROJ_QUERY_DTYPE)
    vis = qv["radius"] > 0
    assert 0.55 < vis.mean() < 0.95
    assert len(set(qv["pred_level"][vis].tolist())) >= 6
    r0 = qv["radius"][vis] / F["scale"][qv["pred_level"][vis]]
    assert set(np.round(r0, 3).tolist()) == {2.5, 4.0}
    # th != 1 scales the radius (RGB-D th = 3, Tracking.cc:1340-1343)
    q3, _ = om.is_in_frustum(F, mps, skip, 0.5, 3.0)
    qn3, _ = numpy_is_in_frustum(F, mps, skip, 0.5, 3.0)
    assert q3.tobytes() == qn3.tobytes()


def test_inliers_predict_their_level(oracle_mod):
    """The synthetic map's MapPoints that observe a feature project onto it at the level the
    generator asked for (PredictScale inverts mfMaxDistance = dist * 1.2^(level - 1/2))."""
    from oracle import matcher as om
    K4, _ = synth.EUROC_CAM
    keys, desc = _keys(5)
    F, mps, _, skip = synth.local_map_points(5, keys, desc, 500, K4, (0.0, 752.0, 0.0, 480.0),
                                             inlier_frac=1.0, outside_frac=0.0, skip_frac=0.0)
    q, n = om.is_in_frustum(F, mps, None)
    qv = q.view(PROJ_QUERY_DTYPE)
    assert n >= 0.97 * len(mps)
    vis = qv["radius"] > 0
    # every projection lands near some feature
    d = np.hypot(qv["u"][vis, None] - keys["x"][None, :], qv["v"][vis, None] - keys["y"][None, :])
    assert np.median(d.min(1)) < 1.5


def test_skip_and_empty(oracle_mod):
    from oracle import matcher as om
    F, mps, _, _ = _scene(7, 50)
    q, n = om.is_in_frustum(F, mps, np.ones(len(mps), np.uint8))
    assert n == 0 and (q.view(PROJ_QUERY_DTYPE)["radius"] == -1).all()
    q, n = om.is_in_frustum(F, mps[:0], None)
    assert n == 0 and len(q) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("seed", [3, 11, 29])
def test_gpu_frustum_one_frame(oracle_mod, orbx_lib, gpu, seed):
    from oracle import matcher as om
    from my_orb_slam2_amd.features import is_in_frustum
    F, mps, _, skip = _scene(seed, 3000)
    qg, ng = is_in_frustum(F, mps, skip)
    qo, no = om.is_in_frustum(F, mps, skip)
    assert ng == no
    bad = np.nonzero(qg.view(np.uint8).reshape(-1, 32) != qo.reshape(-1, 32))[0]
    assert bad.size == 0, f"queries differ at MapPoints {np.unique(bad)[:8]}"
    q3, _ = is_in_frustum(F, mps, skip, 0.5, 3.0)
    qo3, _ = om.is_in_frustum(F, mps, skip, 0.5, 3.0)
    assert q3.tobytes() == qo3.tobytes()
    qe, ne = is_in_frustum(F, mps[:0])
    assert ne == 0 and len(qe) == 0


@pytest.mark.gpu
def test_gpu_frustum_host_form_sentinels(orbx_lib, gpu):
    """orbx_is_in_frustum on three MapPoints, one skipped, the outputs inside sentinel-filled
    allocations: the three queries and the count are the restatement's (the skipped point's query
    is the not-in-view record), nothing else is written."""
    import host_array_cases as hc
    c = hc.case("frustum")
    r = c.call()
    assert r["q"].guards_intact() and r["nvisible"].guards_intact()
    want, n = numpy_is_in_frustum(c.F, c.mps, c.skip)
    assert n >= 1 and want["radius"][1] == -1.0
    assert r["q"].a.tobytes() == want.tobytes()
    assert int(r["nvisible"].a[0]) == n
