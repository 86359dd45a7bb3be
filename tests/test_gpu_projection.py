"""GPU: k_project (orbx_project_map_points / _batch_device) bit for bit against the numpy
restatement of tests/projection_cases.py on every directed and random case of every mode, the
launch shapes, the library-defined out-of-range octave, and end to end: device-made queries
through the projection searches against the CPU oracle search on restated queries, and
MonoTrackBatch / RGBDTrackBatch.track_with_motion_model against single-frame calls."""
import numpy as np
import pytest

import projection_cases as pc
from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import (MAP_POINT_DTYPE, PROJ_FRAME_MAPPOINTS, PROJ_FUSE,
                                       PROJ_FUSE_SCW, PROJ_JOB_DTYPE, PROJ_KEYFRAME, PROJ_KF_SCW,
                                       PROJ_LAST_FRAME, PROJ_QUERY_DTYPE, PROJ_SIM3, FeatureSet,
                                       assign_features_to_grid, project_map_points,
                                       project_map_points_batch_device)

pytestmark = pytest.mark.gpu
f32 = np.float32
MODE_IDS = [pc.MODE_NAMES[m] for m in pc.MODES]
PAD = 5            # records in front of the first job and behind the last one
SENT = 0xA5


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(gpu)


def _rows(q):
    return np.ascontiguousarray(q).view(np.uint8).reshape(-1, 32)


def _assert_queries(got, want, what):
    bad = np.nonzero((_rows(got) != _rows(want)).any(1))[0]
    assert bad.size == 0, f"{what}: queries differ at points {bad[:8]}"


def run_batch(mode, jobs, mps_list, keys_list, skip_list, gpu, with_skip=True, with_nactive=True,
              max_mps=None):
    """One batched call over the given jobs, every array with PAD records in front and behind;
    returns (per-job queries, nactive or None) after checking the sentinels."""
    import torch
    sizes = [len(m) for m in mps_list]
    total = sum(sizes)
    off = (PAD + np.concatenate([[0], np.cumsum(sizes)])).astype(np.int32)
    mps = np.zeros(total + 2 * PAD, MAP_POINT_DTYPE)
    keys = np.zeros(total + 2 * PAD, KEYPOINT_DTYPE)
    skip = np.zeros(total + 2 * PAD, np.uint8)
    for j, m in enumerate(mps_list):
        mps[off[j]:off[j + 1]] = m
        if keys_list[j] is not None:
            keys[off[j]:off[j + 1]] = keys_list[j]
        if skip_list[j] is not None:
            skip[off[j]:off[j + 1]] = skip_list[j]
    d_q = torch.full(((total + 2 * PAD) * 32,), SENT, dtype=torch.uint8, device=gpu)
    d_na = torch.full((len(jobs) + 2,), -77, dtype=torch.int32, device=gpu)
    project_map_points_batch_device(
        mode, _dev(np.stack(jobs).astype(PROJ_JOB_DTYPE), gpu), len(jobs), _dev(mps, gpu),
        _dev(off, gpu), max(sizes) if max_mps is None else max_mps,
        _dev(keys, gpu) if mode in pc.FRAME_MODES else None, _dev(skip, gpu) if with_skip else None,
        d_q, d_na[1:1 + len(jobs)] if with_nactive else None)
    torch.cuda.synchronize()
    raw = d_q.cpu().numpy()
    assert (raw[:PAD * 32] == SENT).all(), "wrote in front of the first job"
    assert (raw[(PAD + total) * 32:] == SENT).all(), "wrote behind the last job"
    na = d_na.cpu().numpy()
    assert na[0] == -77 and na[-1] == -77
    q = raw.view(PROJ_QUERY_DTYPE)
    return [q[off[j]:off[j + 1]] for j in range(len(jobs))], (na[1:-1] if with_nactive else None)


@pytest.mark.parametrize("mode", pc.MODES, ids=MODE_IDS)
def test_every_case_both_entry_points(orbx_lib, gpu, mode):
    cases = pc.all_cases(mode)
    refs = [pc.reference(c) for c in cases]
    for c, (q_ref, n_ref, _) in zip(cases, refs):        # the host form, one case per call
        q, n = project_map_points(mode, c["job"], c["mps"], c["keys"], c["skip"])
        _assert_queries(q, q_ref, c["name"])
        assert n == n_ref, c["name"]
    # the batched form: every case of the mode is one job of a single call
    qs, na = run_batch(mode, [c["job"] for c in cases], [c["mps"] for c in cases],
                       [c["keys"] for c in cases], [c["skip"] for c in cases], gpu)
    for c, (q_ref, n_ref, _), q, n in zip(cases, refs, qs, na):
        _assert_queries(q, q_ref, "batch " + c["name"])
        assert n == n_ref, c["name"]


@pytest.fixture(scope="module")
def pools():
    """1000 points per mode and three jobs differing in th (and window), with their references."""
    out = {}
    for mode in (PROJ_FUSE, PROJ_LAST_FRAME):
        c = pc.random_cases(mode, seeds=(5,), n=1000)[0]
        jobs = []
        for k, th in enumerate((3.0, 7.0, 15.0)):
            j = c["job"].copy()
            j["th"] = th
            j["mono"] = k == 1
            jobs.append(j)
        refs = [pc.project_np(mode, j, c["mps"], c["keys"], None)[0] for j in jobs]
        out[mode] = (c, jobs, refs)
    return out


@pytest.mark.parametrize("mode", [PROJ_FUSE, PROJ_LAST_FRAME], ids=["FUSE", "LAST_FRAME"])
@pytest.mark.parametrize("shape", ["one_job", "three_jobs", "many_jobs"])
def test_launch_shapes(orbx_lib, gpu, pools, mode, shape):
    c, jobs, refs = pools[mode]
    inactive = np.zeros(1, PROJ_QUERY_DTYPE)
    inactive["radius"], inactive["min_level"], inactive["max_level"], inactive["pred_level"] = -1, -1, -1, -1

    def check(layout, with_skip, with_nactive, max_mps=None):
        # layout: [(job variant, point indices)]
        idx = [np.asarray(ix, np.int64) for _, ix in layout]
        skips = [(ix % 4 == 1).astype(np.uint8) for ix in idx]
        qs, na = run_batch(mode, [jobs[v] for v, _ in layout], [c["mps"][ix] for ix in idx],
                           [c["keys"][ix] if c["keys"] is not None else None for ix in idx],
                           skips if with_skip else [None] * len(idx), gpu, with_skip, with_nactive,
                           max_mps)
        for k, ((v, _), ix, q) in enumerate(zip(layout, idx, qs)):
            want = refs[v][ix].copy()
            if with_skip:
                want[skips[k] != 0] = inactive
            _assert_queries(q, want, f"{shape} job {k} ({len(ix)} points)")
            if with_nactive:
                assert na[k] == int((want["radius"] >= 0).sum())

    if shape == "one_job":
        for n in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
            check([(0, np.arange(n))], with_skip=n % 2 == 1, with_nactive=n != 64)
        check([(1, np.arange(300))], False, True, max_mps=1000)      # max_mps above the job's count
    elif shape == "three_jobs":
        for mid in (0, 1):
            check([(0, np.arange(257)), (1, np.arange(mid)), (2, np.arange(300, 365))], True, True)
            check([(2, np.arange(65)), (0, np.arange(mid)), (1, np.arange(500, 1000))], False, False)
    else:
        lay = [(k % 3, (7 * k + np.arange(7)) % 1000) for k in range(256)]
        check(lay, True, True)
        check(lay, False, False)


def test_out_of_range_octave_is_inactive(orbx_lib, gpu):
    """Library-defined: the reference indexes mvScaleFactors[nLastOctave] unchecked; here such a
    point yields an inactive query and its neighbours are untouched."""
    c = [c for c in pc.all_cases(PROJ_LAST_FRAME) if c["name"].endswith("/th7")][0]
    for nl in (8, 1, 16):
        job = c["job"].copy()
        job["cam"]["nlevels"] = nl
        job["cam"]["scale"] = synth.scale_tables(16)[0]
        keys = c["keys"].copy()
        keys["octave"] = np.arange(len(keys)) % nl
        bad = {1: -1, 3: nl, 4: 100, 6: -2 ** 31, 7: 2 ** 31 - 1}
        want, _, _ = pc.project_np(PROJ_LAST_FRAME, job, c["mps"], keys,
                                   np.isin(np.arange(len(keys)), list(bad)))
        for i, o in bad.items():
            keys["octave"][i] = o
        q, n = project_map_points(PROJ_LAST_FRAME, job, c["mps"], keys)
        _assert_queries(q, want, f"nlevels {nl}")
        assert n == len(keys) - len(bad) and (q["radius"][list(bad)] == -1).all()
        (qb,), na = run_batch(PROJ_LAST_FRAME, [job], [c["mps"]], [keys], [None], gpu)
        _assert_queries(qb, want, f"batch nlevels {nl}")
        assert na[0] == n


# ---- end to end: device-made queries through the projection searches ----------------------------

K4 = synth.EUROC_CAM[0]
BOUNDS = (0.0, 752.0, 0.0, 480.0)


def _e2e_scene(mode, seed, f_src, f_dst, truth):
    """MapPoints observed as f_src's features that project onto their f_dst copies."""
    pose = pc.random_pose(seed, K4, BOUNDS)
    mps = pc.mappoints_onto(seed, pose, f_dst.keys, truth)
    job = pc.job_from_pose(mode, pose, seed)
    skip = (np.random.default_rng(seed).random(len(mps)) < 0.05).astype(np.uint8)
    keys = f_src.keys if mode in pc.FRAME_MODES else None
    q_np, n_np, _ = pc.project_np(mode, job, mps, keys, skip)
    q_gpu, n_gpu = project_map_points(mode, job, mps, keys, skip)
    assert n_gpu == n_np and n_np > 0.8 * (skip == 0).sum()
    return q_gpu, q_np


@pytest.mark.parametrize("mode", [PROJ_KF_SCW, PROJ_LAST_FRAME, PROJ_KEYFRAME, PROJ_FUSE,
                                  PROJ_FUSE_SCW], ids=["KF_SCW", "LAST_FRAME", "KEYFRAME", "FUSE",
                                                       "FUSE_SCW"])
def test_end_to_end_search(oracle_mod, orbx_lib, gpu, mode):
    from oracle import matcher as om
    from my_orb_slam2_amd import ORBmatcher
    f1, f2, truth = synth.feature_pair(60 + mode, n1=500, n2=500)
    q_gpu, q_np = _e2e_scene(mode, 60 + mode, f1, f2, truth)
    claimed = np.random.default_rng(mode).random(f2.n) < 0.1
    _, _, isg = synth.scale_tables()
    n_g, m_g = ORBmatcher(0.8, True).search_by_projection(mode, f2, q_gpu, f1.desc, claimed, isg,
                                                          orb_dist=64)
    n_o, m_o = om.search_by_projection(mode, f2, q_np, f1.desc, claimed, isg, orb_dist=64,
                                       nnratio=0.8)
    assert n_g == n_o and n_o > 50
    np.testing.assert_array_equal(m_g, m_o)


def test_end_to_end_sim3(oracle_mod, orbx_lib, gpu):
    from oracle import matcher as om
    from my_orb_slam2_amd import ORBmatcher
    f1, f2, _, _, truth = synth.keyframe_pair(71, n1=500, n2=480)
    inv = np.full(f2.n, -1, np.int64)
    inv[truth[truth >= 0]] = np.nonzero(truth >= 0)[0]
    q12_g, q12_n = _e2e_scene(PROJ_SIM3, 71, f1, f2, truth)      # KF1's MapPoints into KF2
    q21_g, q21_n = _e2e_scene(PROJ_SIM3, 72, f2, f1, inv)        # KF2's MapPoints into KF1
    n_g, m_g = ORBmatcher(0.75, True).SearchBySim3(f1, f2, f1.desc, q12_g, f2.desc, q21_g)
    n_o, m_o = om.search_by_sim3(f1, f2, f1.desc, q12_n, f2.desc, q21_n)
    assert n_g == n_o and n_o > 50
    np.testing.assert_array_equal(m_g, m_o)


# ---- TrackWithMotionModel on the batched front-ends -------------------------------------------

TW, TH_, TB = 320, 240, 4
TK4, TDIST = (230.0, 231.0, 161.5, 118.5), (-0.12, 0.03, 0.0005, -0.0003)


def _track_inputs(mt, nkp, ku, desc, mono, depth=None):
    """Per frame: the last frame's MapPoints taken from the frame's own features (three quarters
    of them, the rest empty slots), the LAST_FRAME job and the restated queries."""
    per = []
    for j in range(TB):
        n = int(nkp[j])
        rng = np.random.default_rng(90 + j)
        cam = pc.random_pose(90 + j, TK4, mt.bounds, mbf=getattr(mt, "mbf", 0.0))
        target = np.where(rng.random(n) < 0.75, rng.permutation(n), -1)
        mps = pc.mappoints_onto(j, cam, ku[j, :n], target, depth=None if depth is None else depth[j, :n])
        skip = (target < 0).astype(np.uint8)                 # no MapPoint in the slot
        src = ku[j, :n].copy()
        ti = np.maximum(target, 0)
        src["octave"] = np.clip(src["octave"][ti] + rng.integers(-1, 2, n), 0, 7)
        src["angle"] = src["angle"][ti]
        # the last frame's pose, placed so that tlc.z is about -2, 0.01, 2, -2 against mb = 0.08
        Rlw, tlw = synth._rot(rng, 5.0), rng.normal(0, 0.3, 3)
        tlw[2] = (-2.0, 0.01, 2.0, -2.0)[j] - (Rlw @ cam["Ow"].astype(np.float64))[2]
        job = pc.proj_job(cam, 7.0 if mono else 15.0, Rlw, tlw, mb=0.08, mono=mono)
        qd = synth._flip(rng, desc[j, :n][ti], rng.integers(0, 16, n))
        q_np, _, info = pc.project_np(PROJ_LAST_FRAME, job, mps, src, skip)
        per.append(dict(n=n, mps=mps, skip=skip, src=src, job=job, qdesc=qd, q_np=q_np,
                        window=info["window"]))
    return per


def _track_check(mt, per, ku, desc, u_right, gpu):
    import torch
    from oracle import matcher as om
    kc = mt.kp_cap
    off = np.concatenate([[0], np.cumsum([p["n"] for p in per])]).astype(np.int32)
    total, max_mps = int(off[-1]), max(p["n"] for p in per)
    cat = lambda k: np.concatenate([p[k] for p in per])
    d_q = torch.full((total * 32,), SENT, dtype=torch.uint8, device=gpu)
    d_match = torch.full((total,), -7, dtype=torch.int32, device=gpu)
    d_cnt = torch.full((TB,), -7, dtype=torch.int32, device=gpu)
    d_na = torch.full((TB,), -7, dtype=torch.int32, device=gpu)
    d_off = torch.from_numpy(off).to(gpu)
    mt.track_with_motion_model(_dev(np.stack([p["job"] for p in per]), gpu), _dev(cat("mps"), gpu),
                               d_off, max_mps, _dev(cat("src"), gpu), _dev(cat("skip"), gpu), d_q,
                               _dev(cat("qdesc"), gpu), d_match, d_cnt, None, d_na)
    mt.matcher.sync()
    q = d_q.cpu().numpy().view(PROJ_QUERY_DTYPE)
    match, cnt, na = d_match.cpu().numpy(), d_cnt.cpu().numpy(), d_na.cpu().numpy()
    claimed = np.zeros((TB, kc), np.uint8)
    fsets = []
    for j, p in enumerate(per):
        n, sl = p["n"], slice(off[j], off[j + 1])
        _assert_queries(q[sl], p["q_np"], f"frame {j}")
        assert na[j] == int((p["q_np"]["radius"] >= 0).sum()) > 0.5 * n
        fs = FeatureSet(ku[j, :n].copy(), desc[j, :n].copy(),
                        None if u_right is None else u_right[j, :n].copy(), None,
                        assign_features_to_grid(ku[j, :n], *mt.bounds))
        fsets.append(fs)
        # four single-frame calls: the host projection and the single search
        q1, _ = project_map_points(PROJ_LAST_FRAME, p["job"], p["mps"], p["src"], p["skip"])
        n1, m1 = mt.matcher.search_by_projection(PROJ_LAST_FRAME, fs, q1, p["qdesc"])
        # the oracle search on the restated queries
        n_o, m_o = om.search_by_projection(PROJ_LAST_FRAME, fs, p["q_np"], p["qdesc"], None, None,
                                           nnratio=0.8)
        assert cnt[j] == n1 == n_o and n_o > 0.3 * n, (j, cnt[j], n1, n_o)
        np.testing.assert_array_equal(match[sl], m1)
        np.testing.assert_array_equal(match[sl], m_o)
        claimed[j, m_o[m_o >= 0]] = 1
    # the claimed mask of the device run, fed into SearchLocalPoints, against host-made queries
    d_claimed = torch.zeros((TB * kc,), dtype=torch.uint8, device=gpu)
    feat = d_match.long() + torch.repeat_interleave(
        torch.arange(TB, device=gpu) * kc, torch.from_numpy(np.diff(off).astype(np.int64)).to(gpu))
    d_claimed[feat[d_match >= 0]] = 1
    assert np.array_equal(d_claimed.cpu().numpy().reshape(TB, kc), claimed)
    qs, ds, refs = [], [], []
    for j, p in enumerate(per):
        n = p["n"]
        ql, dl = synth.local_map_queries(j, ku[j, :n], desc[j, :n], 600, TW, TH_)
        if u_right is not None:      # a stereo frame: the projected right coordinate of the
            near = np.argmin((ql["u"][:, None] - ku[j, :n]["x"][None, :]) ** 2 +       # nearest feature
                             (ql["v"][:, None] - ku[j, :n]["y"][None, :]) ** 2, axis=1)
            ql["ur"] = u_right[j, :n][near]
        refs.append(om.search_by_projection(PROJ_FRAME_MAPPOINTS, fsets[j], ql, dl, claimed[j, :n],
                                            None, nnratio=0.8))
        qs.append(ql)
        ds.append(dl)
    q_off = (600 * np.arange(TB + 1)).astype(np.int32)
    out = torch.full((600 * TB,), -7, dtype=torch.int32, device=gpu)
    cnt2 = torch.full((TB,), -7, dtype=torch.int32, device=gpu)
    mt.search_local_points(_dev(np.concatenate(ds), gpu), _dev(np.concatenate(qs), gpu),
                           torch.from_numpy(q_off).to(gpu), out, cnt2, d_claimed)
    mt.matcher.sync()
    out, cnt2 = out.cpu().numpy(), cnt2.cpu().numpy()
    for j, (n_o, m_o) in enumerate(refs):
        assert cnt2[j] == n_o and n_o > 0
        np.testing.assert_array_equal(out[q_off[j]:q_off[j + 1]], m_o)


def test_mono_track_with_motion_model(oracle_mod, orbx_lib, gpu):
    import torch
    from my_orb_slam2_amd.tracking import MonoTrackBatch
    imgs = np.stack([synth.frame(800 + i, TW, TH_) for i in range(TB)])
    mt = MonoTrackBatch(TB, TW, TH_, TK4, TDIST, nfeatures=500, device=gpu.index or 0)
    mt.frames(torch.from_numpy(imgs).to(gpu))
    nkp, ku, desc = mt.fetch_undistorted()
    assert (nkp > 200).all()
    per = _track_inputs(mt, nkp, ku, desc, mono=True)
    assert {w for p in per for w in p["window"]} == {"", "default"}
    _track_check(mt, per, ku, desc, None, gpu)


def test_rgbd_track_with_motion_model(oracle_mod, orbx_lib, gpu):
    import torch
    from my_orb_slam2_amd.tracking import RGBDTrackBatch
    imgs = np.stack([synth.frame(820 + i, TW, TH_) for i in range(TB)])
    yy, xx = np.mgrid[0:TH_, 0:TW]
    depth = np.stack([(5000.0 * (3.0 + np.sin(xx / 60.0 + i) + 0.8 * np.cos(yy / 45.0))).astype(np.uint16)
                      for i in range(TB)])
    mt = RGBDTrackBatch(TB, TW, TH_, TK4, TDIST, 40.0, depth_factor=float(f32(1.0) / f32(5000.0)),
                        nfeatures=500, device=gpu.index or 0)
    mt.frames(torch.from_numpy(imgs).to(gpu), torch.from_numpy(depth.view(np.int16)).to(gpu))
    nkp, ku, desc = mt.fetch_undistorted()
    ur, de = mt.fetch_stereo()
    assert (nkp > 200).all() and (ur[0, :nkp[0]] > -1).all()
    per = _track_inputs(mt, nkp, ku, desc, mono=False, depth=de)
    # stereo: the forward and the backward window and the default one all occur
    assert {w for p in per for w in p["window"]} == {"", "default", "forward", "backward"}
    _track_check(mt, per, ku, desc, ur, gpu)


def test_host_form_sentinels(orbx_lib, gpu):
    """orbx_project_map_points (LAST_FRAME, so that src_keys is staged) on three MapPoints, one
    skipped, the outputs inside sentinel-filled allocations: the three queries and the count are
    the restatement's, nothing else is written."""
    import host_array_cases as hc
    c = hc.case("project")
    r = c.call()
    assert r["q"].guards_intact() and r["nactive"].guards_intact()
    want, n, _ = pc.project_np(PROJ_LAST_FRAME, c.job, c.mps, c.src_keys, c.skip)
    assert n >= 1 and want["radius"][1] == -1.0
    _assert_queries(r["q"].a, want, "host form")
    assert int(r["nactive"].a[0]) == n
