"""GPU: the RGB-D front-end (k_rgbd_depth, k_unproject, k_close_points and RGBDTrackBatch)
against the numpy restatements of tests/rgbd_cases.py, bit for bit: Frame::ComputeStereoFromRGBD
with the depth scaling (Frame.cc:689-710, Tracking.cc:244-245), Frame::UnprojectStereo
(Frame.cc:713-727) and the close-point pass (Tracking.cc:862-912, 1080-1089, 1164-1217)."""
import numpy as np
import pytest

import rgbd_cases as rc
from my_orb_slam2_amd import synth
from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
from my_orb_slam2_amd.features import (DEPTH_F32, DEPTH_U16, FRAME_POSE_DTYPE, PROJ_LAST_FRAME,
                                       FeatureSet, assign_features_to_grid)

pytestmark = pytest.mark.gpu
f32 = np.float32
SENT = f32(77.25)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _dev(a, gpu):
    """A numpy array's bytes on the device."""
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(gpu)


def _host(t, dtype, shape=(-1,)):
    return t.cpu().numpy().view(dtype).reshape(shape)


@pytest.fixture(scope="module")
def depth_refs():
    """Every directed depth case with the restatement's answer, computed once."""
    out = []
    for c in rc.depth_cases():
        ur, de = rc.compute_stereo_from_rgbd(c["img"], c["depth_type"], c["factor"], c["mbf"],
                                             c["kps"], c["kps_un"])
        out.append((c, ur, de))
    return out


def test_depth_host_form_directed(orbx_lib, gpu, depth_refs):
    from my_orb_slam2_amd.features import compute_stereo_from_rgbd
    for c, ur_o, de_o in depth_refs:
        # the strided H x W view of the padded allocation
        ur, de = compute_stereo_from_rgbd(c["img"], c["factor"], c["mbf"], c["kps"], c["kps_un"])
        tag = (c["depth_type"], c["factor_name"], len(c["kps"]))
        bad = np.nonzero((_bits(de) != _bits(de_o)) | (_bits(ur) != _bits(ur_o)))[0]
        assert bad.size == 0, (tag, bad[:8], [c["style"][i] for i in bad[:8]])


def _batch_depth(gpu, group, kp_stride, run):
    """The frames of `group` ((case, ur, de) with one depth type and factor) as one batch:
    run(d_img, d_kps, d_kps_un, d_n, d_ur, d_de) fills the outputs; slots past d_n keep SENT."""
    import torch
    B = len(group)
    kps = np.zeros((B, kp_stride), KEYPOINT_DTYPE)
    kun = np.zeros((B, kp_stride), KEYPOINT_DTYPE)
    n = np.zeros(B, np.int32)
    for f, (c, _, _) in enumerate(group):
        n[f] = len(c["kps"])
        kps[f, :n[f]], kun[f, :n[f]] = c["kps"], c["kps_un"]
        # past d_n: keypoints that would sample a valid pixel if they were visited
        kps[f, n[f]:]["x"], kps[f, n[f]:]["y"] = 5.0, 5.0
    d_img = _dev(np.stack([c["alloc"] for c, _, _ in group]), gpu)
    d_ur = torch.full((B, kp_stride), float(SENT), dtype=torch.float32, device=gpu)
    d_de = torch.full((B, kp_stride), float(SENT), dtype=torch.float32, device=gpu)
    d_kun = _dev(kun, gpu)
    run(d_img, _dev(kps, gpu), d_kun, _dev(n, gpu), d_ur, d_de)
    torch.cuda.synchronize()
    ur, de = d_ur.cpu().numpy(), d_de.cpu().numpy()
    for f, (c, ur_o, de_o) in enumerate(group):
        tag = (c["depth_type"], c["factor_name"], int(n[f]), f)
        assert np.array_equal(_bits(de[f, :n[f]]), _bits(de_o)), tag
        assert np.array_equal(_bits(ur[f, :n[f]]), _bits(ur_o)), tag
        assert (ur[f, n[f]:] == SENT).all() and (de[f, n[f]:] == SENT).all(), tag
    return _host(d_kun, KEYPOINT_DTYPE, (B, kp_stride)), ur, de


def test_depth_batch_form_directed(orbx_lib, gpu, depth_refs):
    from my_orb_slam2_amd.features import compute_stereo_from_rgbd_batch_device
    by = {}
    for c, ur, de in depth_refs:
        by[(c["depth_type"], c["factor_name"], len(c["kps"]))] = (c, ur, de)
    for t, fname in rc.DEPTH_COMBOS:
        c0 = by[(t, fname, 0)][0]
        es = c0["alloc"].itemsize

        def run(d_img, d_kps, d_kun, d_n, d_ur, d_de, B=0, stride=0):
            compute_stereo_from_rgbd_batch_device(
                d_img, t, c0["row_stride"], c0["alloc"].size * es, rc.W, rc.H, c0["factor"],
                c0["mbf"], d_kps, d_kun, stride, d_n, B, d_ur, d_de)

        # three frames with an empty one in the middle, several blocks per frame
        grp = [by[(t, fname, 257)], by[(t, fname, 0)], by[(t, fname, 65)]]
        _batch_depth(gpu, grp, 300, lambda *a: run(*a, B=3, stride=300))
        # batches of one at every size, the slot count equal to and above the frame's
        for n in rc.DEPTH_SIZES:
            cap = max(n, 1) if n in (64, 256) else n + 3
            _batch_depth(gpu, [by[(t, fname, n)]], cap, lambda *a: run(*a, B=1, stride=cap))


@pytest.mark.parametrize("distorted", [True, False])
def test_fused_geometry_equals_undistort_then_unfused(oracle_mod, orbx_lib, gpu, distorted):
    import torch
    from oracle import matcher as om
    from my_orb_slam2_amd.features import (compute_stereo_from_rgbd_batch_device,
                                           rgbd_frame_geometry_batch_device,
                                           undistort_keypoints_batch_device)
    K4, dist = synth.EUROC_CAM
    dist = np.asarray(dist, f32).copy()
    if not distorted:
        dist[0] = 0.0               # Frame.cc:431: mvKeysUn = mvKeys, whatever else is set
    for t, fname in ((DEPTH_U16, "tum"), (DEPTH_F32, "one+2e-5")):
        cases = [rc.depth_case(9, t, fname, n) for n in (257, 0, 64)]
        B, cap = 3, 260
        kps = np.zeros((B, cap), KEYPOINT_DTYPE)
        n = np.array([len(c["kps"]) for c in cases], np.int32)
        for f, c in enumerate(cases):
            kps[f, :n[f]] = c["kps"]
        c0 = cases[0]
        img = (_dev(np.stack([c["alloc"] for c in cases]), gpu), t, c0["row_stride"],
               c0["alloc"].nbytes, rc.W, rc.H, c0["factor"], c0["mbf"])
        d_n = _dev(n, gpu)
        outs = []
        for mode in ("unfused", "fused", "fused-in-place"):
            d_kps = _dev(kps, gpu)
            d_kun = d_kps if mode == "fused-in-place" else _dev(np.full(kps.shape, 0, KEYPOINT_DTYPE), gpu)
            d_ur = torch.full((B, cap), float(SENT), dtype=torch.float32, device=gpu)
            d_de = torch.full((B, cap), float(SENT), dtype=torch.float32, device=gpu)
            if mode == "unfused":
                undistort_keypoints_batch_device(K4, dist, d_kps, cap, d_n, B, d_kun)
                compute_stereo_from_rgbd_batch_device(*img, d_kps, d_kun, cap, d_n, B, d_ur, d_de)
            else:
                rgbd_frame_geometry_batch_device(K4, dist, *img, d_kps, cap, d_n, B, d_kun, d_ur,
                                                 d_de)
            torch.cuda.synchronize()
            outs.append((_host(d_kun, KEYPOINT_DTYPE, (B, cap)), d_ur.cpu().numpy(), d_de.cpu().numpy()))
        for f in range(B):
            for kun, ur, de in outs[1:]:
                assert kun[f, :n[f]].tobytes() == outs[0][0][f, :n[f]].tobytes()
                assert ur[f].tobytes() == outs[0][1][f].tobytes()
                assert de[f].tobytes() == outs[0][2][f].tobytes()
            # against the restatement, mvKeysUn from the oracle's UndistortKeyPoints
            c = cases[f]
            if n[f] == 0:
                continue
            un = c["kps"].copy()
            if distorted:
                xy = om.undistort_keypoints(c["kps"], K4, dist)
                un["x"], un["y"] = xy[:, 0], xy[:, 1]
            inside = np.array([s != "oob" for s in c["cls"]])
            kun = outs[1][0][f, :n[f]]
            assert np.array_equal(_bits(kun["x"][inside]), _bits(un["x"][inside]))
            assert np.array_equal(_bits(kun["y"][inside]), _bits(un["y"][inside]))
            assert distorted == bool((kun["x"][inside] != c["kps"]["x"][inside]).any())
            ur_o, de_o = rc.compute_stereo_from_rgbd(c["img"], t, c["factor"], c["mbf"], c["kps"], un)
            assert np.array_equal(_bits(outs[1][1][f, :n[f]]), _bits(ur_o))
            assert np.array_equal(_bits(outs[1][2][f, :n[f]]), _bits(de_o))
            assert (outs[1][1][f, n[f]:] == SENT).all()


def test_unsupported_depth_type_and_size(orbx_lib, gpu):
    import torch
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd import features as ft
    z = torch.zeros(64, dtype=torch.uint8, device=gpu)
    with pytest.raises(m.OrbxError) as e:
        ft.compute_stereo_from_rgbd_batch_device(z, 2, 16, 64, 4, 4, 1.0, 40.0, z, z, 1, z, 1, z, z)
    assert e.value.code == -4
    with pytest.raises(m.OrbxError) as e:
        ft.close_points_batch_device(z, z, 8193, z, None, None, z, 1, 3.0, z, z, z, z)
    assert e.value.code == -4
    n = 8193
    with pytest.raises(m.OrbxError) as e:
        ft.close_points(rc.pose(None), np.zeros(n, KEYPOINT_DTYPE), np.ones(n, f32), 3.0)
    assert e.value.code == -4


@pytest.mark.parametrize("seed", [None, 5, 6])
def test_unprojection(orbx_lib, gpu, seed):
    import torch
    from my_orb_slam2_amd.features import unproject_stereo, unproject_stereo_batch_device
    F = rc.pose(seed)
    cases = [c for c in rc.close_cases() if c["name"] in ("M=1", "L<100<M", "inf-denormal")]
    cases.append(rc.close_size_case(257))
    for c in cases:
        sent = np.full((c["n"], 3), SENT, f32)
        want, valid_o = rc.unproject_all(F, c["keys"], c["depth"], sent)
        got, valid = unproject_stereo(F, c["keys"], c["depth"], sent)
        assert np.array_equal(valid, valid_o) and 0 < valid.sum() <= c["n"]
        assert rc.same_floats(got, want), c["name"]
        assert (got[valid == 0] == SENT).all()
        finite = np.isfinite(want).all(1)
        assert np.array_equal(_bits(got[finite]), _bits(want[finite]))
    # batch form: two poses, an empty frame in the middle, slots past d_n untouched
    cap = 300
    grp = [(cases[1], rc.pose(8)), (None, rc.pose(None)), (cases[3], rc.pose(9))]
    keys = np.zeros((3, cap), KEYPOINT_DTYPE)
    depth = np.full((3, cap), 2.0, f32)
    n = np.zeros(3, np.int32)
    for f, (c, _) in enumerate(grp):
        if c is not None:
            n[f] = c["n"]
            keys[f, :n[f]], depth[f, :n[f]] = c["keys"], c["depth"]
    d_x = torch.full((3, cap, 3), float(SENT), dtype=torch.float32, device=gpu)
    d_v = torch.full((3, cap), 9, dtype=torch.uint8, device=gpu)
    poses = np.stack([p for _, p in grp]).astype(FRAME_POSE_DTYPE)
    unproject_stereo_batch_device(_dev(poses, gpu), _dev(keys, gpu), cap, _dev(depth, gpu),
                                  _dev(n, gpu), 3, d_x, d_v)
    torch.cuda.synchronize()
    x, v = d_x.cpu().numpy(), d_v.cpu().numpy()
    for f, (c, p) in enumerate(grp):
        assert (x[f, n[f]:] == SENT).all() and (v[f, n[f]:] == 9).all()
        if c is not None:
            want, valid_o = rc.unproject_all(p, c["keys"], c["depth"], np.full((c["n"], 3), SENT, f32))
            assert np.array_equal(v[f, :n[f]], valid_o) and rc.same_floats(x[f, :n[f]], want)


def _check_close(tag, c, ref, order, counts, create, x3d):
    """order / create / x3d are full-length arrays that held sentinels (-5 / 9 / SENT)."""
    order_o, counts_o, create_o, x3d_o = ref
    M, V = int(counts_o[0]), int(counts_o[1])
    assert np.array_equal(np.asarray(counts).reshape(4), counts_o), (tag, counts, counts_o)
    assert np.array_equal(order[:M], order_o), tag
    assert np.array_equal(create[:V], create_o), tag
    assert rc.same_floats(x3d[:V], x3d_o), tag
    finite = np.isfinite(x3d_o).all(1)
    assert np.array_equal(_bits(x3d[:V][finite]), _bits(x3d_o[finite])), tag
    assert (order[M:] == -5).all() and (create[V:] == 9).all() and (x3d[V:] == SENT).all(), tag


@pytest.fixture(scope="module")
def close_refs():
    cases = rc.close_cases() + [rc.close_size_case(n) for n in rc.CLOSE_SIZES]
    return [(c, rc.close_points_ref(c["F"], c["keys"], c["depth"], c["th"], c["has_point"],
                                    c["tracked"])) for c in cases]


def test_close_points_host_form(orbx_lib, gpu, close_refs):
    from my_orb_slam2_amd.features import close_points
    assert {c["n"] for c, _ in close_refs} >= set(rc.CLOSE_SIZES)
    for c, ref in close_refs:
        n = c["n"]
        out = (np.full(n, -5, np.int32), np.full(n, 9, np.uint8), np.full((n, 3), SENT, f32))
        order, counts, create, x3d = close_points(c["F"], c["keys"], c["depth"], c["th"],
                                                  c["has_point"], c["tracked"], out=out)
        _check_close(c["name"], c, ref, order, counts, create, x3d)


@pytest.mark.parametrize("masks", [True, False])
def test_close_points_batch_form(orbx_lib, gpu, close_refs, masks):
    import torch
    from my_orb_slam2_amd.features import close_points_batch_device
    # one threshold per call: the TH cases of at most 1025 slots, an empty frame among them
    grp = [(c, r) for c, r in close_refs
           if c["th"] == rc.TH and c["n"] <= 1025 and (c["has_point"] is not None) == masks]
    if not masks:
        grp += [(c, rc.close_points_ref(c["F"], c["keys"], c["depth"], c["th"]))
                for c, _ in close_refs if c["name"] in ("n=1", "n=1024", "n=1025", "tie-across-100")]
    assert len(grp) >= 5
    grp.insert(1, (None, None))
    B, cap = len(grp), 1100
    keys = np.zeros((B, cap), KEYPOINT_DTYPE)
    depth = np.full((B, cap), 1.0, f32)          # past d_n: would count if visited
    hp = np.zeros((B, cap), np.uint8)
    tr = np.zeros((B, cap), np.uint8)
    n = np.zeros(B, np.int32)
    poses = np.zeros(B, FRAME_POSE_DTYPE)
    for f, (c, _) in enumerate(grp):
        poses[f] = rc.pose(None) if c is None else c["F"]
        if c is None:
            continue
        n[f] = c["n"]
        keys[f, :n[f]], depth[f, :n[f]] = c["keys"], c["depth"]
        if masks:
            hp[f, :n[f]], tr[f, :n[f]] = c["has_point"], c["tracked"]
    d_order = torch.full((B, cap), -5, dtype=torch.int32, device=gpu)
    d_counts = torch.full((B, 4), -5, dtype=torch.int32, device=gpu)
    d_create = torch.full((B, cap), 9, dtype=torch.uint8, device=gpu)
    d_x3d = torch.full((B, cap, 3), float(SENT), dtype=torch.float32, device=gpu)
    close_points_batch_device(_dev(poses, gpu), _dev(keys, gpu), cap, _dev(depth, gpu),
                              _dev(hp, gpu) if masks else None, _dev(tr, gpu) if masks else None,
                              _dev(n, gpu), B, rc.TH, d_order, d_counts, d_create, d_x3d)
    torch.cuda.synchronize()
    order, counts = d_order.cpu().numpy(), d_counts.cpu().numpy()
    create, x3d = d_create.cpu().numpy(), d_x3d.cpu().numpy()
    for f, (c, ref) in enumerate(grp):
        if c is None:
            assert (counts[f] == 0).all() and (order[f] == -5).all() and (create[f] == 9).all()
            continue
        _check_close((c["name"], f), c, ref, order[f], counts[f], create[f], x3d[f])


def _depth_map(seed, w, h):
    """A u16 depth map: smooth ramps between 0.4 m and 8 m (x 5000) with rectangular holes."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    z = 2.5 + 1.8 * np.sin(xx / 97.0 + seed) + 1.5 * np.cos(yy / 61.0) + rng.uniform(0, 0.02, (h, w))
    d = np.clip(z * 5000.0, 2000, 40000).astype(np.uint16)
    for _ in range(12):
        x0, y0 = int(rng.integers(0, w - 80)), int(rng.integers(0, h - 60))
        d[y0:y0 + int(rng.integers(10, 60)), x0:x0 + int(rng.integers(10, 80))] = 0
    return d


def test_rgbd_track_batch(oracle_mod, orbx_lib, gpu):
    import torch
    import oracle
    from oracle import matcher as om
    import my_orb_slam2_amd as m
    W, H, B = 640, 480, 3
    K4, dist = synth.EUROC_CAM            # a distorted camera, so mvKeysUn differs from mvKeys
    mbf, th = 40.0, f32(3.2)
    imgs = np.stack([synth.frame(700 + i, W, H) for i in range(B)])
    imgs[1] = 0                           # a frame without features
    depth = np.stack([_depth_map(i, W, H) for i in range(B)])
    rt = m.RGBDTrackBatch(B, W, H, K4, dist, mbf, depth_factor=rc.TUM_FACTOR, th_depth=th,
                          device=gpu.index or 0)
    d_imgs = torch.from_numpy(imgs).to(gpu)
    d_depth = torch.from_numpy(depth.view(np.int16)).to(gpu)     # the u16 bits
    rt.frames(d_imgs, d_depth)
    nkp, ku, desc = rt.fetch_undistorted()
    ur, de = rt.fetch_stereo()
    assert nkp[1] == 0 and (nkp[[0, 2]] > 800).all()
    # poses and masks for the close-point pass
    poses = np.stack([rc.pose(50 + j) for j in range(B)]).astype(FRAME_POSE_DTYPE)
    rng = np.random.default_rng(3)
    hp = (rng.random((B, rt.kp_cap)) < 0.5).astype(np.uint8)
    tr = (hp & (rng.random((B, rt.kp_cap)) < 0.8)).astype(np.uint8)
    rt.order.fill_(-5), rt.create.fill_(9), rt.x3d.fill_(float(SENT))
    rt.close_points(_dev(poses, gpu), _dev(hp, gpu), _dev(tr, gpu))
    torch.cuda.synchronize()
    order, counts = rt.order.cpu().numpy(), rt.counts.cpu().numpy()
    create, x3d = rt.create.cpu().numpy(), rt.x3d.cpu().numpy()
    ox = oracle.OracleExtractor(1000, 1.2, 8, 20, 7)
    fsets = []
    for j in range(B):
        n = int(nkp[j])
        _, kraw, _ = rt.ext.batch_fetch(j, 1)
        kraw = kraw[0, :n]
        if j == 0:                        # extraction against the oracle
            k_o, d_o = ox(imgs[0])
            np.testing.assert_array_equal(kraw.view(np.uint8), k_o.view(np.uint8))
            np.testing.assert_array_equal(desc[0, :n], d_o)
        un = kraw.copy()
        if n:
            xy = om.undistort_keypoints(kraw, K4, dist)
            un["x"], un["y"] = xy[:, 0], xy[:, 1]
        assert ku[j, :n].tobytes() == un.tobytes()
        ur_o, de_o = rc.compute_stereo_from_rgbd(depth[j], DEPTH_U16, rc.TUM_FACTOR, mbf, kraw, un)
        assert np.array_equal(_bits(ur[j, :n]), _bits(ur_o)) and np.array_equal(_bits(de[j, :n]), _bits(de_o))
        assert (ur[j, n:] == -1).all() and (de[j, n:] == -1).all()      # as constructed
        if n:
            holes = int((de_o < 0).sum())
            assert 0 < holes < n // 2, holes
        g = assign_features_to_grid(ku[j, :n], *rt.bounds)
        np.testing.assert_array_equal(rt.grid_off[j].cpu().numpy(), g.off)
        np.testing.assert_array_equal(rt.grid_feat[j, :len(g.feat)].cpu().numpy(), g.feat)
        ref = rc.close_points_ref(poses[j], un, de_o, th, hp[j, :n], tr[j, :n])
        _check_close(("track", j), None, ref, order[j], counts[j], create[j], x3d[j])
        if n:
            assert 0 < ref[1][1] < ref[1][0] and ref[1][2] > 0 and ref[1][3] > 0
        fsets.append(FeatureSet(un, desc[j, :n].copy(), ur_o, None, g))
    # one LAST_FRAME projection search per frame: the stereo check reads the frames' u_right
    qs, ds, refs, blind = [], [], [], []
    for j in range(B):
        fs = fsets[j]
        q, d = synth.local_map_queries(j, fs.keys, fs.desc, 900, W, H)
        if fs.n:
            near = np.argmin(np.hypot(q["u"][:, None] - fs.keys["x"][None, :],
                                      q["v"][:, None] - fs.keys["y"][None, :]), 1)
            u = fs.u_right[near]
            jitter = np.random.default_rng(j).normal(0, 0.7, len(q)).astype(f32) * q["radius"]
            q["ur"] = np.where(u > 0, u + jitter, f32(-1)).astype(f32)
        refs.append(om.search_by_projection(PROJ_LAST_FRAME, fs, q, d, None, None, nnratio=0.8))
        blind.append(om.search_by_projection(
            PROJ_LAST_FRAME, FeatureSet(fs.keys, fs.desc, None, None, fs.grid), q, d, None, None,
            nnratio=0.8))
        qs.append(q)
        ds.append(d)
    q_off = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int32)
    out = torch.full((int(q_off[-1]),), -7, dtype=torch.int32, device=gpu)
    cnt = torch.full((B,), -7, dtype=torch.int32, device=gpu)
    rt.matcher.search_by_projection_batch_device(
        PROJ_LAST_FRAME, rt, _dev(np.concatenate(ds), gpu), _dev(np.concatenate(qs), gpu),
        torch.from_numpy(q_off).to(gpu), out, cnt)
    rt.matcher.sync()
    out, cnt = out.cpu().numpy(), cnt.cpu().numpy()
    for j, (n_o, m_o) in enumerate(refs):
        assert cnt[j] == n_o, j
        np.testing.assert_array_equal(out[q_off[j]:q_off[j + 1]], m_o)
    assert cnt[0] > 100 and cnt[1] == 0
    assert not np.array_equal(blind[0][1], refs[0][1])       # u_right changed the outcome


@pytest.mark.parametrize("name", ["rgbd_u16", "rgbd_f32"])
def test_depth_host_form_sentinels(orbx_lib, gpu, name):
    """orbx_compute_stereo_from_rgbd on three keypoints of the padded image, the outputs inside
    sentinel-filled allocations: three values each, the restatement's; nothing else is written."""
    import host_array_cases as hc
    c = hc.case(name)
    r = c.call()
    assert r["u_right"].guards_intact() and r["depth"].guards_intact()
    d = c.d
    ur, de = rc.compute_stereo_from_rgbd(d["img"], d["depth_type"], d["factor"], d["mbf"], d["kps"],
                                         d["kps_un"])
    assert np.array_equal(_bits(r["u_right"].a), _bits(ur))
    assert np.array_equal(_bits(r["depth"].a), _bits(de))


def test_unprojection_host_form_sentinels(orbx_lib, gpu):
    """orbx_unproject_stereo on three keypoints, the middle one without depth: its x3d row keeps the
    sentinel bytes it held, the other rows and `valid` are the restatement's, the guards intact."""
    import host_array_cases as hc
    c = hc.case("unproject")
    r = c.call()
    assert r["x3d"].guards_intact() and r["valid"].guards_intact()
    want, valid = rc.unproject_all(c.F, c.keys, c.depth, hc.sentinel(f32, 9).reshape(3, 3).copy())
    assert valid.tolist() == [1, 0, 1] and r["valid"].a.tolist() == [1, 0, 1]
    assert r["x3d"].a.tobytes() == want.tobytes()
    assert r["x3d"].a[1].tobytes() == bytes([hc.SENT]) * 12


def test_close_points_host_form_guards(orbx_lib, gpu):
    """orbx_close_points with has_point given and tracked null on five keypoints: order[:M],
    create[:V], x3d[:V] and the counts are the restatement's; the slots past the counts and the
    guards keep the sentinel."""
    import host_array_cases as hc
    c = hc.case("close")
    r = c.call()
    assert all(g.guards_intact() for g in r.values())
    order_o, counts_o, create_o, x3d_o = rc.close_points_ref(c.F, c.keys, c.depth, c.th,
                                                             c.has_point, None)
    M, V = int(counts_o[0]), int(counts_o[1])
    assert 0 < V <= M < 5
    assert np.array_equal(r["counts"].a, counts_o)
    assert np.array_equal(r["order"].a[:M], order_o) and np.array_equal(r["create"].a[:V], create_o)
    assert np.array_equal(_bits(r["x3d"].a[:V]), _bits(x3d_o))
    assert r["order"].a[M:].tobytes() == bytes([hc.SENT]) * (4 * (5 - M))
    assert (r["create"].a[V:] == hc.SENT).all()
    assert r["x3d"].a[V:].tobytes() == bytes([hc.SENT]) * (12 * (5 - V))
