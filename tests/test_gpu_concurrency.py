"""The host-image path under the reference's threading (src/System.cc:91-101, Frame.cc:89-92):
per stereo frame two threads extract the left and right images on their own ORBextractor
handles while a third thread (LocalMapping / LoopClosing) runs matcher calls on its own
ORBmatcher, and a fourth runs batched device extractions on a torch stream.  Every result
must be bit-identical to the same calls made one at a time."""
import threading

import numpy as np
import pytest

from helpers import assert_bytes_equal, assert_f32_bits_equal, assert_kps_equal
from my_orb_slam2_amd import synth

pytestmark = pytest.mark.gpu

MBF, FX = 386.1448, 718.856


def test_concurrent_dropin_threads(orbx_lib, gpu):
    import torch
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd import ORBmatcher
    mb = float(np.float32(MBF) / np.float32(FX))
    frames = [synth.stereo_pair(700 + i, 1241, 376) for i in range(6)]
    cases = [synth.feature_pair(710 + i, n1=1200, n2=1200) for i in range(4)]
    tri = [synth.keyframe_pair(720 + i, n1=1500, n2=1500) for i in range(3)]
    s, s2, _ = synth.scale_tables()
    batch = torch.from_numpy(np.stack([synth.frame(730 + i, 640, 480) for i in range(8)])).to(gpu)

    def frame_serial(gl, gr, L, R):
        kl, dl = gl(L)
        kr, dr = gr(R)
        u, z, nv = m.compute_stereo_matches(gl, gr, MBF, mb)
        return kl, dl, kr, dr, u, z, nv

    def match_serial(mt, mt2):
        out = []
        for f1, f2, _ in cases:
            out.append(mt.SearchByBoW(f1, np.ones(f1.n, bool), f2))
        for k1, k2, F, epi, _ in tri:
            out.append(mt2.SearchForTriangulation(k1, np.zeros(k1.n, bool), k2, np.zeros(k2.n, bool),
                                                  F, epi, s2, s, False))
        return out

    def batch_serial(ext, st):
        ext.extract_batch_device(batch, st)
        return ext.batch_fetch()

    gl, gr = m.ORBextractor(2000, 1.2, 8, 20, 7), m.ORBextractor(2000, 1.2, 8, 20, 7)
    mt, mt2 = ORBmatcher(0.75, True), ORBmatcher(0.6, False)
    bext = m.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=8)
    stream = torch.cuda.Stream(gpu)
    ref_frames = [frame_serial(gl, gr, L, R) for L, R in frames]
    ref_match = match_serial(mt, mt2)
    ref_batch = batch_serial(bext, stream.cuda_stream)
    torch.cuda.synchronize()

    errors, got_match, got_batch = [], [], []
    stop = threading.Event()

    def mapping_thread():
        try:
            while not stop.is_set():
                got_match.append(match_serial(mt, mt2))
        except Exception as e:   # pragma: no cover - reported below
            errors.append(e)

    def batch_thread():
        try:
            while not stop.is_set():
                got_batch.append(batch_serial(bext, stream.cuda_stream))
        except Exception as e:   # pragma: no cover
            errors.append(e)

    side = [threading.Thread(target=mapping_thread), threading.Thread(target=batch_thread)]
    for t in side:
        t.start()
    got_frames = []
    try:
        for rnd in range(3):
            for L, R in frames:
                res = {}

                def ext(h, img, key):
                    try:
                        res[key] = h(img)
                    except Exception as e:   # pragma: no cover
                        errors.append(e)
                tl = threading.Thread(target=ext, args=(gl, L, "l"))
                tr = threading.Thread(target=ext, args=(gr, R, "r"))
                tl.start()
                tr.start()
                tl.join()
                tr.join()
                u, z, nv = m.compute_stereo_matches(gl, gr, MBF, mb)
                got_frames.append((*res["l"], *res["r"], u, z, nv))
    finally:
        stop.set()
        for t in side:
            t.join()
    assert not errors, errors
    assert len(got_match) >= 1 and len(got_batch) >= 1
    for i, g in enumerate(got_frames):
        r = ref_frames[i % len(frames)]
        assert_kps_equal(g[0], r[0], f"frame {i} left")
        assert_bytes_equal(g[1], r[1], f"frame {i} left desc")
        assert_kps_equal(g[2], r[2], f"frame {i} right")
        assert_bytes_equal(g[3], r[3], f"frame {i} right desc")
        assert_f32_bits_equal(g[4], r[4], f"frame {i} uRight")
        assert_f32_bits_equal(g[5], r[5], f"frame {i} depth")
        assert g[6] == r[6]
    for rnd in got_match:
        for (n_g, m_g), (n_r, m_r) in zip(rnd, ref_match):
            assert n_g == n_r
            np.testing.assert_array_equal(m_g, m_r)
    for nkp, kps, desc in got_batch:
        assert np.array_equal(nkp, ref_batch[0])
        for j in range(len(nkp)):
            assert_kps_equal(kps[j, :nkp[j]], ref_batch[1][j, :nkp[j]], f"batch image {j}")
            assert_bytes_equal(desc[j, :nkp[j]], ref_batch[2][j, :nkp[j]], f"batch image {j}")


def test_batch_fetch_races_extract(orbx_lib, gpu):
    """orbx_batch_fetch / orbx_batch_view_get on one thread while another thread keeps
    extracting batches on the same handle (on a torch stream): the handle's lock and done event
    order them, so every fetch returns one whole extraction, batch A's or batch B's, never a mix
    (include/orbx.h: calls on one handle may come from any thread)."""
    import torch
    import my_orb_slam2_amd as m
    imgs = [torch.from_numpy(np.stack([synth.frame(760 + 10 * k + i, 640, 480) for i in range(6)]))
            .to(gpu) for k in range(2)]
    ext = m.ORBextractor(1000, 1.2, 8, 20, 7, max_batch=6)
    stream = torch.cuda.Stream(gpu)
    refs = []
    for b in imgs:
        ext.extract_batch_device(b, stream.cuda_stream)
        refs.append(ext.batch_fetch())
    assert not np.array_equal(refs[0][2], refs[1][2])
    errors, fetched = [], []
    stop = threading.Event()

    def extractor_thread():
        try:
            i = 0
            while not stop.is_set():
                ext.extract_batch_device(imgs[i % 2], stream.cuda_stream)
                i += 1
        except Exception as e:   # pragma: no cover
            errors.append(e)

    t = threading.Thread(target=extractor_thread)
    t.start()
    try:
        for _ in range(40):
            v = ext.batch_view()
            assert v.batch == 6 and v.kp_cap == refs[0][1].shape[1]
            fetched.append(ext.batch_fetch())
    finally:
        stop.set()
        t.join()
    assert not errors, errors
    torch.cuda.synchronize()
    seen = set()
    for nkp, kps, desc in fetched:
        which = [k for k, r in enumerate(refs) if np.array_equal(nkp, r[0]) and
                 all(np.array_equal(desc[j, :nkp[j]], r[2][j, :nkp[j]]) and
                     np.array_equal(kps[j, :nkp[j]].view(np.uint8), r[1][j, :nkp[j]].view(np.uint8))
                     for j in range(len(nkp)))]
        assert which, "a fetch mixed two extractions"
        seen.add(which[0])


def test_k_tracker_sessions(orbx_lib, gpu):
    """K = 4 tracking sessions sharing the GPU (bench.py --workload dropin --trackers 4): each
    session has its own left / right handles and runs Frame.cc:89-102 (two extraction threads,
    then the stereo match) over the same frames at the same time as the others.  Every
    session's results equal the serial single-session run, bit for bit."""
    import my_orb_slam2_amd as m
    mb = float(np.float32(MBF) / np.float32(FX))
    frames = [synth.stereo_pair(740 + i, 1241, 376) for i in range(4)]
    K = 4
    sess = [(m.ORBextractor(2000, 1.2, 8, 20, 7), m.ORBextractor(2000, 1.2, 8, 20, 7))
            for _ in range(K)]
    ref = []
    for L, R in frames:
        kl, dl = sess[0][0](L)
        kr, dr = sess[0][1](R)
        ref.append((kl, dl, kr, dr, *m.compute_stereo_matches(sess[0][0], sess[0][1], MBF, mb)))
    got = [[] for _ in range(K)]
    errors = []

    def session(k):
        gl, gr = sess[k]
        try:
            for rnd in range(2):
                for L, R in frames:
                    res = {}
                    tl = threading.Thread(target=lambda: res.__setitem__("l", gl(L)))
                    tr = threading.Thread(target=lambda: res.__setitem__("r", gr(R)))
                    tl.start()
                    tr.start()
                    tl.join()
                    tr.join()
                    got[k].append((*res["l"], *res["r"], *m.compute_stereo_matches(gl, gr, MBF, mb)))
        except Exception as e:   # pragma: no cover
            errors.append(e)
    ths = [threading.Thread(target=session, args=(k,)) for k in range(K)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors
    for k in range(K):
        assert len(got[k]) == 2 * len(frames)
        for i, g in enumerate(got[k]):
            r = ref[i % len(frames)]
            assert_kps_equal(g[0], r[0], f"session {k} frame {i} left")
            assert_bytes_equal(g[1], r[1], f"session {k} frame {i} left desc")
            assert_kps_equal(g[2], r[2], f"session {k} frame {i} right")
            assert_bytes_equal(g[3], r[3], f"session {k} frame {i} right desc")
            assert_f32_bits_equal(g[4], r[4], f"session {k} frame {i} uRight")
            assert_f32_bits_equal(g[5], r[5], f"session {k} frame {i} depth")
            assert g[6] == r[6]


def test_cpp_tracker_sessions_agree(orbx_lib, gpu, tmp_path):
    """The C++ K-tracker loop bench.py times (boundary_test `bench DIR N W K`): 4 sessions over
    the same pairs report the same output digest."""
    import json
    import subprocess
    from my_orb_slam2_amd import build as b
    binp = b.build_boundary_test()
    mb = float(np.float32(MBF) / np.float32(FX))
    for i in range(2):
        L, R = synth.stereo_pair(750 + i, 1241, 376)
        L.tofile(tmp_path / f"pair_{i}_left.raw")
        R.tofile(tmp_path / f"pair_{i}_right.raw")
    (tmp_path / "params.txt").write_text(f"1241 376 2000 {MBF!r} {mb!r} 2\n")
    r = subprocess.run([str(binp), "bench", str(tmp_path), "6", "2", "4"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert res["trackers"] == 4 and len(res["latency_ms"]) == 24
    assert len(set(res["digests"])) == 1, res["digests"]


def test_capture_beside_cross_stream_wait(orbx_lib, gpu):
    """The right handle's done event sits on the left handle's stream after
    ComputeStereoMatches (orbx_stereo_match records it there); the right handle's next
    extraction waits on it from its own stream while the left handle's thread re-captures its
    graph (a new image size: new graph key).  The runtime refuses such a wait while the
    event's stream is capturing, so the library orders the two (orbx_capi.hip
    order_after_last / graph_current); every call must succeed and equal the serial result.
    (The refusal was seen in test_facade_cpp's three-session facade bench, once in four runs;
    this sweep of the right thread's start over the left thread's re-capture did not reproduce
    it on the library without the ordering either, so it guards the scenario, not the timing.)"""
    import my_orb_slam2_amd as m
    mb = float(np.float32(MBF) / np.float32(FX))
    sizes = [(1241, 376), (1226, 370)]
    pairs = [synth.stereo_pair(760 + i, *sizes[i % 2]) for i in range(4)]
    gl, gr = m.ORBextractor(2000, 1.2, 8, 20, 7), m.ORBextractor(2000, 1.2, 8, 20, 7)
    ref = [(gl(L), gr(R)) for L, R in pairs]
    errors = []
    import time
    for it in range(80):
        L, R = pairs[it % 4]
        gl(L)
        gr(R)
        m.compute_stereo_matches(gl, gr, MBF, mb)
        nxt = (it + 1) % 4   # the other size: the left handle re-captures
        out = {}

        def left():
            try:
                out["l"] = gl(pairs[nxt][0])
            except Exception as e:   # noqa: BLE001 -- reported below
                errors.append(("left", it, repr(e)))

        def right():
            # the right thread's wait lands at a different point of the left thread's
            # re-capture each iteration (0-9.75 ms after it starts: its workspace is rebuilt
            # for the new size first)
            time.sleep(2.5e-4 * (it % 40))
            try:
                out["r"] = gr(pairs[it % 4][1])
            except Exception as e:   # noqa: BLE001
                errors.append(("right", it, repr(e)))

        ts = [threading.Thread(target=left), threading.Thread(target=right)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert_kps_equal(out["l"][0], ref[nxt][0][0], f"left it {it}")
        assert_bytes_equal(out["l"][1], ref[nxt][0][1], f"left desc it {it}")
        assert_kps_equal(out["r"][0], ref[it % 4][1][0], f"right it {it}")
        assert_bytes_equal(out["r"][1], ref[it % 4][1][1], f"right desc it {it}")


def _host_array_calls():
    """The fourteen handle-free host-array entry points and the nine of a matcher handle.  The five
    solvers, each on its smallest committed
    directed case that runs at least one full iteration: name -> a function that makes the case's
    call(s) from fresh inputs and returns every array and record that comes back, as bytes, ahead of
    a count of the iterations the call ran.  The nine per-frame ones on the tiny cases of
    tests/host_array_cases.py (the count is 1): the returned bytes are the callers' whole output
    allocations, sentinel guards and row padding included.  The matcher forms on the cases of
    host_array_cases.MATCHER_NAMES in the same way, every calling thread with matcher handles of
    its own (a handle is not re-entrant)."""
    import host_array_cases
    import pnp_cases
    import poseopt_cases
    import sim3_cases
    import sim3opt_cases
    import triangulate_cases
    from my_orb_slam2_amd import triangulate_matches
    from my_orb_slam2_amd.features import pose_optimization
    from my_orb_slam2_amd.pnp import (PNP_RESULT_DTYPE, PNP_STATE_DTYPE, pnp_iterate,
                                      pnp_ransac_parameters, pnp_sample_quads)
    from my_orb_slam2_amd.sim3 import (SIM3_RESULT_DTYPE, SIM3_STATE_DTYPE, sim3_iterate,
                                       sim3_optimize, sim3_ransac_iterations, sim3_sample_triples)

    def poseopt():      # three edges: the fewest PoseOptimization takes
        c = poseopt_cases.case_named("count_3_mono")
        pose, flag, ngood, info = pose_optimization(c["pose"], c["keys"], c["mp_of_feat"], c["mps"],
                                                    c["ur"], c["outlier_in"])
        return (poseopt_cases.info_fields(info)["iters"], pose.tobytes(), flag.tobytes(), ngood,
                info)

    def sim3opt():      # one correspondence: two edges
        c = sim3opt_cases.case_named("count_1_free")
        res, keep = sim3_optimize(c["pose1"], c["pose2"], sim3opt_cases.job_record(c), c["corr"],
                                  c["sim3_in"], c["keep_in"])
        return (sim3opt_cases.info_fields(res["info"])["iters"], res.tobytes(), keep.tobytes())

    def sim3():         # three correspondences: the one triple
        c = sim3_cases.case_named("random_3")
        N = len(c["corr"])
        max_its = sim3_ransac_iterations(c["prob"], c["min_inliers"], c["max_iterations"], N)
        tri = sim3_sample_triples(N, c["rand"][:3 * max_its])
        state = np.zeros(1, SIM3_STATE_DTYPE)
        state["iterations"], state["best_inliers"] = c["state0"]
        out = []
        for n_it in c["calls"]:
            res = np.zeros(1, SIM3_RESULT_DTYPE)
            inl = np.zeros(c["mN1"], np.uint8)
            sim3_iterate(c["pose1"], c["pose2"], sim3_cases.job_of(c, max_its, n_it), c["corr"],
                         tri, state, res, inl)
            out += [res.tobytes(), inl.tobytes(), state.tobytes()]
        return (int(state["iterations"][0]), *out)

    def pnp():          # four correspondences: the one minimal set
        c = pnp_cases.case_named("n_is_4")
        N = len(c["corr"])
        mi, mx = pnp_ransac_parameters(c["prob"], c["min_inliers"], c["max_iterations"], 4,
                                       c["epsilon"], N)
        q = pnp_sample_quads(N, c["rand"])
        for k, v in c["quad_edits"].items():
            q[k] = v
        state = np.zeros(1, PNP_STATE_DTYPE)
        state["iterations"], state["best_inliers"] = c["state0"]
        state["best_Tcw"] = c["best_Tcw0"]
        best = c["best0"].copy()
        out = []
        for n_it in c["calls"]:
            res = np.zeros(1, PNP_RESULT_DTYPE)
            inl = np.zeros(c["n_matches"], np.uint8)
            pnp_iterate(pnp_cases.job_of(c, mi, mx, n_it), c["corr"], q, state, best, res, inl)
            out += [res.tobytes(), inl.tobytes(), state.tobytes(), best.tobytes()]
        return (int(state["iterations"][0]), *out)

    def triangulate():  # two pairs, both triangulated
        c = triangulate_cases.case_named("far_st01")
        st, x, nnew = triangulate_matches(
            c["pose1"], c["pose2"], c["keys1"], c["keys2"], c["pairs"], c["ratio_factor"],
            mb=c["mb"], u_right1=c["ur1"], u_right2=c["ur2"], depth1=c["depth1"],
            depth2=c["depth2"], keys_raw1=c["raw1"], keys_raw2=c["raw2"], cos_stereo1=c["cos1"],
            cos_stereo2=c["cos2"])
        return (nnew, st.tobytes(), x.tobytes())

    calls = dict(poseopt=poseopt, sim3opt=sim3opt, sim3=sim3, pnp=pnp, triangulate=triangulate)
    for name in host_array_cases.NAMES + host_array_cases.MATCHER_NAMES:
        assert name not in calls, name          # a solver and a case of one name would share an id
        calls[name] = host_array_cases.case(name).call_bytes
    return calls


HOST_ARRAY_ENTRY_POINTS = ("poseopt", "sim3opt", "sim3", "pnp", "triangulate", "undistort",
                           "frustum", "project", "unproject", "close", "rgbd_u16", "rgbd_f32",
                           "cvt_color3", "cvt_color4", "remap", "bow_db_score",
                           "bow_kf_frame", "bow_kf_kf", "tri_exact", "tri_short", "proj_greedy",
                           "proj_fuse", "proj_ex", "proj_nq0", "by_sim3", "init", "distinctive", "bf",
                           "bf_ndb0")


@pytest.fixture(scope="module")
def host_array_serial(orbx_lib, gpu):
    """Every entry point's call made alone, first: what the threads' results must equal."""
    calls = _host_array_calls()
    serial = {name: calls[name]() for name in HOST_ARRAY_ENTRY_POINTS}
    for name, r in serial.items():
        assert r[0] >= 1, (name, "the case runs no iteration")
    return calls, serial


@pytest.mark.parametrize("name", HOST_ARRAY_ENTRY_POINTS)
def test_host_array_solver_threads_equal_serial(host_array_serial, name):
    """Every host-array entry point stages through a leased (stream, buffer, plan) slot
    (orbx_host.h, HostCall), so calls of one entry point from several threads run beside each
    other: four threads leave a barrier together and call it three times each on the same case
    while a fifth calls another entry point.  Every array and record equals the serial call's,
    byte for byte."""
    calls, serial = host_array_serial
    names = HOST_ARRAY_ENTRY_POINTS
    other = names[(names.index(name) + 1) % len(names)]
    barrier = threading.Barrier(5)
    got, errors = [], []

    def worker(which):
        try:
            barrier.wait()
            for _ in range(3):
                got.append((which, calls[which]()))
        except Exception as e:   # pragma: no cover - reported below
            errors.append((which, repr(e)))
            barrier.abort()

    ths = [threading.Thread(target=worker, args=(n,)) for n in (name,) * 4 + (other,)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    assert not errors, errors
    assert sorted(w for w, _ in got) == sorted([name] * 12 + [other] * 3)
    for which, r in got:
        assert r == serial[which], which
