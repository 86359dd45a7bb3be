"""GPU: k_pose_opt (orbx_pose_optimization / _batch_device) bit for bit against the numpy
restatement of tests/poseopt_cases.py (which tests/test_poseopt_cases.py holds against the C++
one) on every case through both entry points, the launch shapes, the refusals, k_match_scatter,
and MonoTrackBatch / RGBDTrackBatch.track_with_motion_model_and_optimize against the oracle
search followed by the restatement, its poses fed on into project_local_map."""
import numpy as np
import pytest

import poseopt_cases as pc
import projection_cases as prj
from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import (FRAME_POSE_DTYPE, MAP_POINT_DTYPE, PROJ_LAST_FRAME,
                                       PROJ_QUERY_DTYPE, FeatureSet, assign_features_to_grid,
                                       matches_to_features_batch_device, pose_optimization,
                                       pose_optimization_batch_device)

pytestmark = pytest.mark.gpu
f32 = np.float32
PAD = 3
SENT = 0xA5


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(gpu)


def _expect(case, max_feat):
    """The restatement's result; a case run under another max_feat than its own is recomputed."""
    if len(case["keys"]) > case["max_feat"] and len(case["keys"]) <= max_feat:
        return pc.pose_optimization_np(dict(case, max_feat=max_feat))
    return pc.reference(case)


def run_batch(cases, gpu, alias=False, max_feat=None, mono_null=False):
    """One launch over the cases, every array with PAD records of sentinel in front and behind;
    returns [(pose, outlier, ngood, info)] after checking the sentinels."""
    import torch
    nf = len(cases)
    ns = [len(c["keys"]) for c in cases]
    ms = [len(c["mps"]) for c in cases]
    fo = (PAD + np.concatenate([[0], np.cumsum(ns)])).astype(np.int32)
    mo = (PAD + np.concatenate([[0], np.cumsum(ms)])).astype(np.int32)
    keys = np.zeros(fo[-1] + PAD, KEYPOINT_DTYPE)
    keys["octave"] = 1 << 20                      # reading a pad slot's scale would fault the test
    ur = np.full(fo[-1] + PAD, -1, f32)
    mpf = np.full(fo[-1] + PAD, 1 << 28, np.int32)
    mps = np.zeros(mo[-1] + PAD, MAP_POINT_DTYPE)
    mps["pos"] = np.nan
    flag = np.full(fo[-1] + PAD, SENT, np.uint8)
    poses = np.zeros(nf + 2 * PAD, FRAME_POSE_DTYPE)
    for j, c in enumerate(cases):
        sl = slice(fo[j], fo[j + 1])
        keys[sl], mpf[sl], flag[sl] = c["keys"], c["mp_of_feat"], c["outlier_in"]
        if c["ur"] is not None:
            ur[sl] = c["ur"]
        mps[mo[j]:mo[j + 1]] = c["mps"]
        poses[PAD + j] = c["pose"]
    d_poses = _dev(poses, gpu)
    d_out = d_poses if alias else torch.full_like(d_poses, SENT)
    d_flag = _dev(flag, gpu)
    d_ng = torch.full((nf + 2 * PAD,), -77, dtype=torch.int32, device=gpu)
    d_info = torch.full((nf + 2 * PAD,), -77, dtype=torch.int32, device=gpu)
    ps = FRAME_POSE_DTYPE.itemsize
    pose_optimization_batch_device(
        d_poses[PAD * ps:], nf, _dev(keys, gpu), None if mono_null else _dev(ur, gpu),
        _dev(fo, gpu), max(ns) if max_feat is None else max_feat, _dev(mpf, gpu), _dev(mps, gpu),
        _dev(mo, gpu), d_out[PAD * ps:], d_flag, d_ng[PAD:], d_info[PAD:])
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(FRAME_POSE_DTYPE)
    flag_o, ng, info = d_flag.cpu().numpy(), d_ng.cpu().numpy(), d_info.cpu().numpy().view(np.uint32)
    edge = np.r_[0:PAD, nf + PAD:nf + 2 * PAD]
    assert (ng[edge] == -77).all() and (d_info.cpu().numpy()[edge] == -77).all()
    assert out[edge].tobytes() == (poses[edge] if alias else
                                   np.full(2 * PAD * ps, SENT, np.uint8)).tobytes()
    assert (flag_o[:PAD] == SENT).all() and (flag_o[fo[-1]:] == SENT).all()
    if alias:
        assert d_poses.data_ptr() == d_out.data_ptr()
    return [(out[PAD + j], flag_o[fo[j]:fo[j + 1]], int(ng[PAD + j]), int(info[PAD + j]))
            for j in range(nf)]


def _check(cases, got, max_feat):
    for c, (pose, flag, ngood, info) in zip(cases, got):
        r = _expect(c, max_feat)
        what = (c["name"], pc.info_fields(info), pc.info_fields(r["info"]))
        assert (ngood, info) == (r["ngood"], r["info"]), what
        assert pose.tobytes() == r["pose"].tobytes(), what
        assert flag.tobytes() == r["outlier"].tobytes(), what
        has = c["mp_of_feat"] >= 0
        if not (info & (0xf << 24)):
            assert (flag[~has] == pc.UNTOUCHED).all() and (flag[has] <= 1).all(), what


def test_every_case_host_form(orbx_lib, gpu):
    for c in pc.all_cases():
        if len(c["keys"]) > c["max_feat"]:
            continue                      # the host form's max_feat is the frame's own count
        r = pc.reference(c)
        pose, flag, ngood, info = pose_optimization(c["pose"], c["keys"], c["mp_of_feat"], c["mps"],
                                                    c["ur"], c["outlier_in"])
        what = (c["name"], pc.info_fields(info), pc.info_fields(r["info"]))
        assert (ngood, info) == (r["ngood"], r["info"]), what
        assert pose.tobytes() == r["pose"].tobytes(), what
        assert flag.tobytes() == r["outlier"].tobytes(), what
    # mono frames pass no u_right at all; no outlier array means zeros
    c = pc.case_named("count_65_mono")
    assert c["ur"] is None
    r = pc.reference(c)
    pose, flag, ngood, _ = pose_optimization(c["pose"], c["keys"], c["mp_of_feat"], c["mps"])
    assert pose.tobytes() == r["pose"].tobytes() and ngood == r["ngood"]
    assert np.array_equal(flag, np.where(c["mp_of_feat"] >= 0, r["outlier"], 0))


def test_every_case_in_one_launch(orbx_lib, gpu):
    cases = pc.all_cases()
    mf = max(len(c["keys"]) for c in cases)
    _check(cases, run_batch(cases, gpu), mf)
    flags = set()
    for c in cases:
        flags |= pc.info_fields(_expect(c, mf)["info"])["flags"]
    assert {"REFUSED_MP_INDEX", "REFUSED_OCTAVE", "REFUSED_NLEVELS", "THETA_LIMIT",
            "NONPOSITIVE_SOLVE", "FEW_EDGES"} <= flags


SMALL = ("count_10_mixed", "count_3_mono", "count_9_stereo", "exact_mixed", "count_2_mixed",
         "rho0_stale_one_round", "count_63_mixed", "refuse_octave_high", "count_65_stereo",
         "count_0_mono", "far_3_mixed", "count_129_mixed", "z_zero", "nonpositive_mixed_11",
         "nonpositive_stereo_4_qmax")


@pytest.mark.parametrize("nframes", [1, 2, 5, 257])
def test_launch_shapes(orbx_lib, gpu, nframes):
    cases = [pc.case_named(SMALL[j % len(SMALL)]) for j in range(nframes)]
    mf = max(len(c["keys"]) for c in cases)
    _check(cases, run_batch(cases, gpu), mf)
    _check(cases, run_batch(cases, gpu, alias=True), mf)


def test_unequal_frames_with_an_empty_one_in_the_middle(orbx_lib, gpu):
    empty = dict(pc.case_named("count_0_mono"), name="empty")
    for k in ("keys", "mp_of_feat", "outlier_in"):
        empty[k] = empty[k][:0]
    empty["mps"] = empty["mps"][:0]
    got = run_batch([empty], gpu)
    assert got[0][2:] == (0, pc.FEW_EDGES) and got[0][0].tobytes() == empty["pose"].tobytes()
    cases = [pc.case_named("count_129_mono"), pc.case_named("count_3_stereo"), empty,
             pc.case_named("count_64_mixed"), pc.case_named("count_2_stereo")]
    got = run_batch(cases, gpu, alias=True)
    for c, g in zip(cases, got):
        r = pc.pose_optimization_np(c) if c is empty else pc.reference(c)
        assert g[0].tobytes() == r["pose"].tobytes() and g[2:] == (r["ngood"], r["info"]), c["name"]
        assert g[1].tobytes() == r["outlier"].tobytes()
    # mono frames through a NULL d_u_right
    cases = [pc.case_named("count_65_mono"), pc.case_named("count_9_mono")]
    _check(cases, run_batch(cases, gpu, mono_null=True), 70)


def test_feature_count_above_max_feat_is_refused(orbx_lib, gpu):
    cases = [pc.case_named("count_10_mono"), pc.case_named("refuse_count"),
             pc.case_named("count_9_mixed")]
    mf = pc.case_named("refuse_count")["max_feat"]
    assert len(cases[1]["keys"]) == mf + 1 and len(cases[0]["keys"]) <= mf
    got = run_batch(cases, gpu, max_feat=mf)
    _check(cases, got, mf)
    assert got[1][3] == pc.REFUSED_COUNT and got[1][2] == 0
    assert (got[1][1] == pc.UNTOUCHED).all() and got[1][0].tobytes() == cases[1]["pose"].tobytes()


def test_no_frames_touches_nothing(orbx_lib, gpu):
    import torch
    z = torch.full((64,), SENT, dtype=torch.uint8, device=gpu)
    pose_optimization_batch_device(z, 0, z, z, z, 8, z, z, z, z, z, z, z)
    pose_optimization_batch_device(None, 0, None, None, None, 0, None, None, None, None, None,
                                   None, None)
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == SENT).all()


# ---- k_match_scatter -----------------------------------------------------------------------------

def _scatter_np(match, q_off, feat_off, prior):
    out = np.full(feat_off[-1], -1, np.int32)
    flagged = 0
    for j in range(len(q_off) - 1):
        n = feat_off[j + 1] - feat_off[j]
        for q, i in enumerate(match[q_off[j]:q_off[j + 1]]):     # in query order: later overwrites
            if i == -1:
                continue
            if i < 0 or i >= n:
                flagged = 1
            else:
                out[feat_off[j] + i] = q
    if prior is not None:
        # the scatter overwrites the copied-in prior
        seen = out >= 0
        out = np.where(seen, out, prior)
    return out, flagged


@pytest.mark.parametrize("with_prior", [False, True])
def test_match_scatter(orbx_lib, gpu, with_prior):
    import torch
    rng = np.random.default_rng(17)
    nq, nf = [300, 0, 1000, 5], [256, 40, 700, 9]
    q_off = np.concatenate([[0], np.cumsum(nq)]).astype(np.int32)
    feat_off = np.concatenate([[0], np.cumsum(nf)]).astype(np.int32)
    match = np.full(q_off[-1], -1, np.int32)
    for j in range(4):
        m = match[q_off[j]:q_off[j + 1]]
        pick = rng.random(nq[j]) < 0.6
        m[pick] = rng.integers(0, nf[j], int(pick.sum()))         # duplicates abound
    m = match[q_off[2]:q_off[3]]
    m[m == 11] = -1
    m[3] = m[900] = 11                                            # a planted duplicate: 900 wins
    prior = None
    if with_prior:
        prior = np.where(rng.random(feat_off[-1]) < 0.3, rng.integers(0, 2000, feat_off[-1]),
                         -1).astype(np.int32)
    want, flagged = _scatter_np(match, q_off, feat_off, prior)
    assert want[feat_off[2] + 11] == 900 and flagged == 0
    d_out = torch.full((feat_off[-1] + 2 * PAD,), -77, dtype=torch.int32, device=gpu)
    d_flag = torch.full((3,), -77, dtype=torch.int32, device=gpu)

    def run(m):
        matches_to_features_batch_device(_dev(m, gpu), _dev(q_off, gpu), _dev(feat_off + PAD, gpu),
                                         4, max(nq), max(nf), d_out, d_flag[1:],
                                         None if prior is None else
                                         _dev(np.concatenate([np.zeros(PAD, np.int32), prior]), gpu))
        torch.cuda.synchronize()
        o, f = d_out.cpu().numpy(), d_flag.cpu().numpy()
        assert (o[:PAD] == -77).all() and (o[-PAD:] == -77).all() and f[0] == f[2] == -77
        return o[PAD:-PAD], int(f[1])

    got, f = run(match)
    np.testing.assert_array_equal(got, want)
    assert f == 0
    # an out-of-range feature index is skipped and flagged
    bad = match.copy()
    bad[q_off[0] + 7], bad[q_off[3] + 1], bad[q_off[2] + 5] = nf[0], -2, 1 << 30
    want, flagged = _scatter_np(bad, q_off, feat_off, prior)
    got, f = run(bad)
    np.testing.assert_array_equal(got, want)
    assert f == flagged == 1


# ---- TrackWithMotionModel up to its PoseOptimization on the batched front-ends ---------------------

TW, TH_, TB = 320, 240, 3
TK4, TDIST = (230.0, 231.0, 161.5, 118.5), (-0.12, 0.03, 0.0005, -0.0003)


def _chain(mt, gpu, mono, depth=None, u_right=None):
    import torch
    from oracle import matcher as om
    nkp, ku, desc = mt.fetch_undistorted()
    assert (nkp > 200).all()
    kc = mt.kp_cap
    per = []
    for j in range(TB):
        n = int(nkp[j])
        rng = np.random.default_rng(190 + j)
        cam = prj.random_pose(190 + j, TK4, mt.bounds, mbf=getattr(mt, "mbf", 0.0))
        target = np.where(rng.random(n) < 0.75, rng.permutation(n), -1)
        mps = prj.mappoints_onto(j, cam, ku[j, :n], target,
                                 depth=None if depth is None else depth[j, :n])
        skip = (target < 0).astype(np.uint8)
        src = ku[j, :n].copy()
        ti = np.maximum(target, 0)
        src["octave"] = np.clip(src["octave"][ti] + rng.integers(-1, 2, n), 0, 7)
        src["angle"] = src["angle"][ti]
        Rlw, tlw = synth._rot(rng, 5.0), rng.normal(0, 0.3, 3)
        job = prj.proj_job(cam, 7.0 if mono else 15.0, Rlw, tlw, mb=0.08, mono=mono)
        qd = synth._flip(rng, desc[j, :n][ti], rng.integers(0, 16, n))
        q_np, _, _ = prj.project_np(PROJ_LAST_FRAME, job, mps, src, skip)
        per.append(dict(n=n, cam=cam, mps=mps, skip=skip, src=src, job=job, qdesc=qd, q_np=q_np))
    off = np.concatenate([[0], np.cumsum([p["n"] for p in per])]).astype(np.int32)
    total, max_mps = int(off[-1]), max(p["n"] for p in per)
    cat = lambda k: np.concatenate([p[k] for p in per])
    i32 = dict(dtype=torch.int32, device=gpu)
    d_q = torch.zeros((total * 32,), dtype=torch.uint8, device=gpu)
    d_match, d_cnt = torch.full((total,), -7, **i32), torch.full((TB,), -7, **i32)
    d_mpf, d_flagged = torch.full((TB * kc,), -7, **i32), torch.full((1,), -7, **i32)
    d_poses = _dev(np.stack([p["cam"] for p in per]), gpu)
    d_out = torch.zeros_like(d_poses)
    d_outl = torch.full((TB * kc,), pc.UNTOUCHED, dtype=torch.uint8, device=gpu)
    d_ng, d_info = torch.full((TB,), -7, **i32), torch.full((TB,), -7, **i32)
    d_off, d_mps = torch.from_numpy(off).to(gpu), _dev(cat("mps"), gpu)
    mt.track_with_motion_model_and_optimize(
        _dev(np.stack([p["job"] for p in per]), gpu), d_poses, d_mps, d_off, max_mps,
        _dev(cat("src"), gpu), _dev(cat("skip"), gpu), d_q, _dev(cat("qdesc"), gpu), d_match,
        d_cnt, d_mpf, d_flagged, d_out, d_outl, d_ng, d_info)
    mt.matcher.sync()
    torch.cuda.synchronize()
    match, mpf = d_match.cpu().numpy(), d_mpf.cpu().numpy().reshape(TB, kc)
    out = d_out.cpu().numpy().view(FRAME_POSE_DTYPE)
    outl, ng = d_outl.cpu().numpy().reshape(TB, kc), d_ng.cpu().numpy()
    info = d_info.cpu().numpy().view(np.uint32)
    assert int(d_flagged.cpu()[0]) == 0
    refs = []
    for j, p in enumerate(per):
        n, sl = p["n"], slice(off[j], off[j + 1])
        fs = FeatureSet(ku[j, :n].copy(), desc[j, :n].copy(),
                        None if u_right is None else u_right[j, :n].copy(), None,
                        assign_features_to_grid(ku[j, :n], *mt.bounds))
        n_o, m_o = om.search_by_projection(PROJ_LAST_FRAME, fs, p["q_np"], p["qdesc"], None, None,
                                           nnratio=0.8)
        np.testing.assert_array_equal(match[sl], m_o)
        want = np.full(kc, -1, np.int32)
        for q, i in enumerate(m_o):
            if i >= 0:
                want[i] = q
        np.testing.assert_array_equal(mpf[j], want)
        case = dict(name=f"chain{j}", pose=p["cam"], keys=ku[j], mp_of_feat=want, mps=p["mps"],
                    ur=None if u_right is None else u_right[j],
                    outlier_in=np.full(kc, pc.UNTOUCHED, np.uint8), max_feat=kc)
        r = pc.pose_optimization_np(case)
        f = pc.info_fields(r["info"])
        assert f["rounds"] == 4 and not f["flags"] and r["ngood"] >= 10, (j, f, r["ngood"])
        if u_right is not None:       # the frame's edges are stereo where the depth map has depth
            assert (u_right[j][want >= 0] >= 0).any()
        assert (int(ng[j]), int(info[j])) == (r["ngood"], r["info"]), (j, f, pc.info_fields(info[j]))
        assert out[j].tobytes() == r["pose"].tobytes(), j
        assert outl[j].tobytes() == r["outlier"].tobytes(), j
        refs.append(r)
    # the refined poses go on into SearchLocalPoints' projection: against the oracle from the
    # restatement's poses
    nl = 400
    lm = [synth.local_map_points(300 + j, ku[j, :per[j]["n"]], desc[j, :per[j]["n"]], nl, TK4,
                                 mt.bounds, mbf=getattr(mt, "mbf", 0.0)) for j in range(TB)]
    l_off = (nl * np.arange(TB + 1)).astype(np.int32)
    d_lq = torch.zeros((nl * TB * 32,), dtype=torch.uint8, device=gpu)
    d_nv = torch.full((TB,), -7, **i32)
    mt.project_local_map(d_out, _dev(np.concatenate([m[1] for m in lm]), gpu),
                         torch.from_numpy(l_off).to(gpu), nl,
                         _dev(np.concatenate([m[3] for m in lm]), gpu), d_lq, d_nv)
    torch.cuda.synchronize()
    lq, nv = d_lq.cpu().numpy().reshape(TB, nl * 32), d_nv.cpu().numpy()
    for j in range(TB):
        qo, no = om.is_in_frustum(refs[j]["pose"], lm[j][1], lm[j][3])
        assert nv[j] == no
        assert lq[j].tobytes() == np.asarray(qo).tobytes(), j


def test_mono_track_with_motion_model_and_optimize(oracle_mod, orbx_lib, gpu):
    import torch
    from my_orb_slam2_amd.tracking import MonoTrackBatch
    imgs = np.stack([synth.frame(800 + i, TW, TH_) for i in range(TB)])
    mt = MonoTrackBatch(TB, TW, TH_, TK4, TDIST, nfeatures=500, device=gpu.index or 0)
    mt.frames(torch.from_numpy(imgs).to(gpu))
    _chain(mt, gpu, mono=True)


def test_rgbd_track_with_motion_model_and_optimize(oracle_mod, orbx_lib, gpu):
    import torch
    from my_orb_slam2_amd.tracking import RGBDTrackBatch
    imgs = np.stack([synth.frame(820 + i, TW, TH_) for i in range(TB)])
    yy, xx = np.mgrid[0:TH_, 0:TW]
    depth = np.stack([(5000.0 * (3.0 + np.sin(xx / 60.0 + i) + 0.8 * np.cos(yy / 45.0))).astype(np.uint16)
                      for i in range(TB)])
    mt = RGBDTrackBatch(TB, TW, TH_, TK4, TDIST, 40.0, depth_factor=float(f32(1.0) / f32(5000.0)),
                        nfeatures=500, device=gpu.index or 0)
    mt.frames(torch.from_numpy(imgs).to(gpu), torch.from_numpy(depth.view(np.int16)).to(gpu))
    ur, de = mt.fetch_stereo()
    _chain(mt, gpu, mono=False, depth=de, u_right=ur)
