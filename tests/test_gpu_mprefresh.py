"""GPU: orbx_refresh_map_points* (k_refresh_map_points) against the restatement of
tests/mprefresh_cases.py, bit for bit (NaN components as NaN) with guard values around every output:
every directed case through both entry points, the max_obs classes, 1 / 7 / 300 points per call, the
corrupt snapshots carved out of one larger zero-filled tensor, the random batches, one eager run and
one replay from a captured graph, and SearchForTriangulation + triangulation -> bookkeeping ->
refresh -> isInFrustum against the same chain with the restatement in the middle."""
import numpy as np
import pytest

import mprefresh_cases as mc

pytestmark = pytest.mark.gpu

GUARD = 16          # elements on either side of every output block
f32 = np.float32


def guarded(a, torch, dev):
    """A device copy of `a` with GUARD sentinel elements on both sides; the interior view."""
    flat = np.ascontiguousarray(a).reshape(-1)
    raw = flat.view(np.uint8)
    g = GUARD * flat.dtype.itemsize
    host = np.full(len(raw) + 2 * g, 0xc3, np.uint8)
    host[g:g + len(raw)] = raw
    t = torch.from_numpy(host).to(dev)
    return t, t[g:g + len(raw)], g


def view_of(S, gpu):
    from my_orb_slam2_amd.localmap import LocalMapView
    v = LocalMapView({k: S[k] for k in mc.ARRAYS}, gpu.index or 0)
    return v.set_refresh_inputs({k: S[k] for k in mc.EXTRA})


def outputs(S, n, torch, gpu):
    return dict(rec=guarded(S["mp_rec"], torch, gpu), desc=guarded(S["mp_desc"], torch, gpu),
                info=guarded(np.full(max(n, 1), 0x77777777, np.uint32), torch, gpu))


def compare(out, want, S, n, name):
    """The device blocks against the restatement's result; the guards are as they were."""
    for k, (full, inner, g) in out.items():
        host = full.cpu().numpy()
        assert (host[:g] == 0xc3).all() and (host[len(host) - g:] == 0xc3).all(), (name, k)
    rec = out["rec"][1].cpu().numpy().view(mc.MAP_POINT_DTYPE)
    desc = out["desc"][1].cpu().numpy().reshape(-1, 32)
    info = out["info"][1].cpu().numpy().view(np.uint32)
    assert info[:n].tolist() == want["info"], name
    assert (info[n:] == 0x77777777).all(), name
    assert rec["pos"].tobytes() == S["mp_rec"]["pos"].tobytes(), name
    if not mc.same_records(rec, want["rec"]):
        bad = [p for p in range(len(rec)) if not mc.same_records(rec[p:p + 1], want["rec"][p:p + 1])]
        pytest.fail(f"{name}: records {bad[:8]} differ: {rec[bad[0]]} != {want['rec'][bad[0]]}")
    bad = np.flatnonzero((desc != want["desc"]).any(axis=1))
    assert bad.size == 0, (name, bad[:8])


def run_device(S, ids, what, max_obs, gpu, name, view=None):
    import torch
    from my_orb_slam2_amd.localmap import refresh_map_points
    view = view or view_of(S, gpu)
    out = outputs(S, len(ids), torch, gpu)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(gpu)
    refresh_map_points(view, d_ids, what, max_obs, out["desc"][1], out["info"][1],
                       d_mp_rec=out["rec"][1], n=len(ids))
    torch.cuda.synchronize()
    want = mc.refresh_np(S, ids, what, max_obs)
    compare(out, want, S, len(ids), name)
    return want


def run_host(S, ids, what, max_obs, name):
    from my_orb_slam2_amd.localmap import refresh_map_points_host
    h = refresh_map_points_host({k: S[k] for k in mc.ARRAYS}, {k: S[k] for k in mc.EXTRA}, ids, what,
                                max_obs, S["mp_desc"])
    want = mc.refresh_np(S, ids, what, max_obs)
    assert h["info"].tolist() == want["info"], name
    assert mc.same_records(h["mp_rec"], want["rec"]), name
    assert h["mp_desc"].tobytes() == want["desc"].tobytes(), name


@pytest.mark.parametrize("case", mc.directed_cases(), ids=lambda c: c["name"])
def test_directed_both_entry_points(case, orbx_lib, gpu):
    run_device(case["S"], case["ids"], case["what"], case["max_obs"], gpu, case["name"])
    run_host(case["S"], case["ids"], case["what"], case["max_obs"], case["name"])


@pytest.mark.parametrize("max_obs", mc.MAX_OBS_CLASSES)
def test_every_directed_case_under_each_max_obs(max_obs, orbx_lib, gpu):
    """Equal results wherever the row is not refused: the restatement of the unrefused points does
    not depend on max_obs, and the kernel equals it under every class."""
    refused = 0
    for c in mc.directed_cases():
        want = run_device(c["S"], c["ids"], c["what"], max_obs, gpu, f"{c['name']} @ {max_obs}")
        full = mc.reference(c) if c["max_obs"] == mc.MAX_OBS else None
        for k, (p, w) in enumerate(zip(c["ids"], want["info"])):
            if w == mc.CAP_OBS:
                refused += 1
            elif full is not None and full["info"][k] != mc.CAP_OBS:
                assert w == full["info"][k]
                assert mc.same_records(want["rec"][p:p + 1], full["rec"][p:p + 1])
                assert want["desc"][p].tobytes() == full["desc"][p].tobytes()
    assert refused > 0 or max_obs == mc.MAX_OBS


@pytest.mark.parametrize("n", [1, 7, 300])
def test_points_per_call(n, orbx_lib, gpu):
    rng = np.random.RandomState(50)
    rows = [list(rng.permutation(30)[:rng.randint(1, 12)]) for _ in range(300)]
    S = mc.snapshot(30, rows, seed=50, bad_kf=[3, 17], bad_mp=[5, 250])
    ids = rng.permutation(300)[:n]
    run_device(S, ids, mc.BOTH, 32, gpu, f"{n} points")


def test_no_points_launches_nothing(orbx_lib, gpu):
    import torch
    from my_orb_slam2_amd.localmap import refresh_map_points
    S = mc.case_named("bad_point")["S"]
    z = torch.full((64,), 5, dtype=torch.int32, device=gpu)
    refresh_map_points(view_of(S, gpu), z, mc.BOTH, 8, z, z, d_mp_rec=z, n=0)
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == 5).all()


def carved_view(S, gpu):
    """The snapshot's arrays inside one zero-filled tensor, 8 KiB apart and 64 KiB from its ends:
    the address a small out-of-range index gives still lies inside it."""
    import torch
    from my_orb_slam2_amd.localmap import LocalMapView
    names = mc.ARRAYS + mc.EXTRA
    big = torch.zeros(128 * 1024 + 8192 * len(names), dtype=torch.uint8, device=gpu)
    arrays, at = {}, 64 * 1024
    for k in names:
        a = np.ascontiguousarray(S[k])
        raw = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(gpu)
        assert len(raw) <= 8192
        big[at:at + len(raw)] = raw
        piece = big[at:at + len(raw)]
        byte_arrays = ("kf_bad", "mp_bad", "mp_rec", "kf_pose", "kf_keys", "kf_desc")
        arrays[k] = piece if k in byte_arrays else piece.view(torch.int32)
        at += 8192
    v = LocalMapView({k: arrays[k] for k in mc.ARRAYS}, gpu.index or 0)
    v.set_refresh_inputs({k: arrays[k] for k in mc.EXTRA})
    v._big = big
    return v


@pytest.mark.parametrize("case", mc.bad_index_cases(), ids=lambda c: c["name"])
def test_bad_index_is_refused_beside_healthy_points(case, orbx_lib, gpu):
    want = run_device(case["S"], case["ids"], case["what"], case["max_obs"], gpu, case["name"],
                      view=carved_view(case["S"], gpu))
    assert mc.BAD_INDEX in want["info"] and 0 in want["info"]


@pytest.mark.parametrize("seed", range(1, 9))
def test_random_batches(seed, orbx_lib, gpu):
    c = mc.random_batch(seed)
    run_device(c["S"], c["ids"], c["what"], c["max_obs"], gpu, c["name"])
    if seed <= 2:
        run_host(c["S"], c["ids"], c["what"], c["max_obs"], c["name"])


def test_view_mp_rec_in_place(orbx_lib, gpu):
    """d_mp_rec defaults to the view's own mp_rec: refreshed in place."""
    import torch
    from my_orb_slam2_amd.localmap import refresh_map_points
    c = mc.case_named("some_keyframes_bad")
    S = c["S"]
    view = view_of(S, gpu)
    d_desc = torch.from_numpy(S["mp_desc"].copy()).to(gpu)
    d_info = torch.zeros(len(c["ids"]), dtype=torch.int32, device=gpu)
    refresh_map_points(view, torch.from_numpy(c["ids"]).to(gpu), mc.BOTH, 8, d_desc, d_info)
    torch.cuda.synchronize()
    want = mc.reference(c)
    got = view.t["mp_rec"].cpu().numpy().reshape(-1).view(mc.MAP_POINT_DTYPE)
    assert mc.same_records(got, want["rec"]) and d_desc.cpu().numpy().tobytes() == want["desc"].tobytes()


def test_eager_and_graph_replay(orbx_lib, gpu):
    import torch
    from my_orb_slam2_amd.localmap import refresh_map_points
    c = mc.random_batch(3)
    S, ids = c["S"], c["ids"]
    want = mc.refresh_np(S, ids, mc.BOTH, 64)
    view = view_of(S, gpu)
    d_ids = torch.from_numpy(np.ascontiguousarray(ids, np.int32)).to(gpu)
    eager = outputs(S, len(ids), torch, gpu)
    refresh_map_points(view, d_ids, mc.BOTH, 64, eager["desc"][1], eager["info"][1],
                       d_mp_rec=eager["rec"][1])
    torch.cuda.synchronize()
    compare(eager, want, S, len(ids), "eager")
    out = outputs(S, len(ids), torch, gpu)
    st = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            refresh_map_points(view, d_ids, mc.BOTH, 64, out["desc"][1], out["info"][1],
                               d_mp_rec=out["rec"][1], stream=st.cuda_stream)
    torch.cuda.synchronize()
    # the capture ran nothing
    assert (out["info"][1].cpu().numpy().view(np.uint32) == 0x77777777).all()
    graph.replay()
    torch.cuda.synchronize()
    compare(out, want, S, len(ids), "replay")
    graph.replay()                                   # and again: it reads nothing it wrote
    torch.cuda.synchronize()
    compare(out, want, S, len(ids), "second replay")


# ---- the chain: triangulate, bookkeeping, refresh, isInFrustum -----------------------------------------

FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375
MBF = f32(47.9)


def test_triangulate_refresh_frustum_chain(orbx_lib, gpu):
    import torch
    from my_orb_slam2_amd import ORBmatcher, synth
    from my_orb_slam2_amd.features import (FRAME_POSE_DTYPE, PROJ_QUERY_DTYPE, frame_pose,
                                           is_in_frustum_batch_device)
    from my_orb_slam2_amd.localmap import LocalMapView, refresh_map_points
    from my_orb_slam2_amd.matcher import DeviceKfDb, parallax_stereo_cos
    import triangulate_cases as tc
    matcher = ORBmatcher(0.6, False)
    s, s2, _ = synth.scale_tables()
    mb = f32(MBF / f32(FX))
    A, B, F_ab, epi_ab, _ = synth.keyframe_pair(23, n1=200, n2=200)
    rng = np.random.default_rng(23 + 7919)      # the pose keyframe_pair(23) gave B
    R_b = synth._rot(rng, 5.0)
    C_b = 0.5 * np.array([rng.uniform(-1, 1), rng.uniform(-0.2, 0.2), rng.uniform(-1.2, 1.2)])
    bounds, K4 = (0.0, 752.0, 0.0, 480.0), (FX, FY, CX, CY)
    poses = np.concatenate([frame_pose(np.eye(3), np.zeros(3), K4, bounds, s, MBF).reshape(1),
                            frame_pose(R_b, -R_b @ C_b, K4, bounds, s, MBF).reshape(1)])
    kfs = [A, B]
    db = DeviceKfDb(kfs, [np.zeros(k.n, np.uint8) for k in kfs], gpu)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)

    def tables(fs):
        ur = np.full(fs.n, -1, f32) if fs.u_right is None else np.asarray(fs.u_right, f32)
        with np.errstate(all="ignore"):
            depth = np.where(ur >= 0, MBF / (fs.keys["x"] - ur), f32(-1)).astype(f32)
        return depth, parallax_stereo_cos(mb, depth)

    tabs = [tables(k) for k in kfs]
    d_match = torch.full((A.n,), -7, dtype=torch.int32, device=gpu)
    d_cnt = torch.zeros(1, dtype=torch.int32, device=gpu)
    d_status = torch.full((A.n,), -77, dtype=torch.int32, device=gpu)
    d_x3d = torch.zeros((A.n, 3), dtype=torch.float32, device=gpu)
    d_nnew = torch.zeros(1, dtype=torch.int32, device=gpu)
    d_poses = T(poses.view(np.uint8).reshape(-1))
    matcher.search_and_triangulate_batch_device(
        db.c, T(np.array([0], np.int32)), T(np.array([1], np.int32)), T(F_ab.reshape(1, 9).astype(f32)),
        T(np.array([epi_ab], f32)), s2, s, T(np.array([0, A.n], np.int32)), d_match, d_cnt, d_poses,
        T(np.concatenate([t[0] for t in tabs])), T(np.concatenate([t[1] for t in tabs])),
        tc.RATIO_FACTOR, d_status, d_x3d, d_nnew, mb=mb)
    matcher.sync()
    status, match, x3d = d_status.cpu().numpy(), d_match.cpu().numpy(), d_x3d.cpu().numpy()
    new = np.flatnonzero(status <= tc.OK_STEREO2)
    assert len(new) >= 10 and len(new) == int(d_nnew.cpu().numpy()[0])

    # the bookkeeping of CreateNewMapPoints: a new id per point, two observations each, the
    # current keyframe (slot 0) the reference keyframe
    n_mp = len(new)
    kf_mp = np.full(A.n + B.n, -1, np.int32)
    kf_mp[new] = np.arange(n_mp)
    kf_mp[A.n + match[new]] = np.arange(n_mp)
    rec = np.zeros(n_mp, mc.MAP_POINT_DTYPE)
    rec["pos"] = x3d[new]
    arrays = dict(kf_order=np.array([1, 0], np.int32), kf_bad=np.zeros(2, np.uint8),
                  kf_parent=np.array([-1, 0], np.int32), kf_cov_off=np.zeros(3, np.int32),
                  kf_cov=np.zeros(0, np.int32), kf_child_off=np.zeros(3, np.int32),
                  kf_child=np.zeros(0, np.int32), kf_mp_off=db.feat_off.astype(np.int32), kf_mp=kf_mp,
                  mp_bad=np.zeros(n_mp, np.uint8), mp_obs_off=np.arange(0, 2 * n_mp + 1, 2, dtype=np.int32),
                  mp_obs=np.tile(np.array([0, 1], np.int32), n_mp), mp_rec=rec)
    extra = dict(mp_obs_feat=np.stack([new, match[new]], axis=1).reshape(-1).astype(np.int32),
                 mp_ref_kf=np.zeros(n_mp, np.int32), kf_pose=poses,
                 kf_keys=np.concatenate([A.keys, B.keys]), kf_desc=np.concatenate([A.desc, B.desc]))
    view = LocalMapView(arrays, gpu.index or 0)
    # the database's keys and descriptors as they are
    view.set_refresh_inputs(dict(extra, kf_keys=db.tensors[1], kf_desc=db.tensors[2]))
    d_desc = torch.zeros((n_mp, 32), dtype=torch.uint8, device=gpu)
    d_info = torch.full((n_mp,), 0x77, dtype=torch.int32, device=gpu)
    d_ids = torch.arange(n_mp, dtype=torch.int32, device=gpu)
    refresh_map_points(view, d_ids, mc.BOTH, 2, d_desc, d_info)
    d_q = torch.zeros(n_mp * PROJ_QUERY_DTYPE.itemsize, dtype=torch.uint8, device=gpu)
    d_nv = torch.zeros(1, dtype=torch.int32, device=gpu)
    d_off = T(np.array([0, n_mp], np.int32))
    d_skip = torch.zeros(n_mp, dtype=torch.uint8, device=gpu)
    frame = d_poses[FRAME_POSE_DTYPE.itemsize:]                  # seen from B
    is_in_frustum_batch_device(frame, 1, view.t["mp_rec"], d_off, n_mp, d_skip, d_q, d_nv)
    torch.cuda.synchronize()
    assert (d_info.cpu().numpy() == 0).all()

    # the same chain with the restatement in the middle
    S = dict(arrays, **extra, n_kf=2, n_mp=n_mp, n_cov=0, n_child=0, n_kfmp=A.n + B.n, n_obs=2 * n_mp,
             mp_desc=np.zeros((n_mp, 32), np.uint8))
    want = mc.refresh_np(S, np.arange(n_mp), mc.BOTH, 2)
    got = view.t["mp_rec"].cpu().numpy().reshape(-1).view(mc.MAP_POINT_DTYPE)
    assert mc.same_records(got, want["rec"])
    assert d_desc.cpu().numpy().tobytes() == want["desc"].tobytes()
    assert (want["rec"]["max_dist"] > want["rec"]["min_dist"]).all()
    d_q2 = torch.zeros_like(d_q)
    d_nv2 = torch.zeros_like(d_nv)
    is_in_frustum_batch_device(frame, 1, T(want["rec"].view(np.uint8).reshape(-1)), d_off, n_mp, d_skip,
                               d_q2, d_nv2)
    torch.cuda.synchronize()
    assert d_q.cpu().numpy().tobytes() == d_q2.cpu().numpy().tobytes()
    assert int(d_nv.cpu()[0]) == int(d_nv2.cpu()[0]) > 0
