"""GPU: orbx_update_local_map* against the restatement of tests/localmap_cases.py, integer for integer
and record byte for byte, with guard values around every output block: every directed case, the
corrupt snapshots (carved out of one larger zero-filled tensor), a batch that mixes the regimes, the
same frames one per call, the random batches, the host-array form, the search's inputs
(descriptors and claimed features) next to the block, and MonoTrackBatch.track_local_map against
its stages called one by one with the restated update in the middle, eagerly and replayed from a
captured graph."""
import numpy as np
import pytest

import localmap_cases as lc

pytestmark = pytest.mark.gpu

GUARD = 16          # elements on either side of every output block
ARRAYS = ("kf_order", "kf_bad", "kf_parent", "kf_cov_off", "kf_cov", "kf_child_off", "kf_child",
          "kf_mp_off", "kf_mp", "mp_bad", "mp_obs_off", "mp_obs", "mp_rec")


def make_outputs(frames):
    """The output blocks of one call as they are before it (numpy, with guards), and the call's
    shape.  Every frame of a call shares stride, cap_kf and cap_mp."""
    B = len(frames)
    F0 = frames[0]
    stride, ck, cm = len(F0["feat_mp"]), F0["cap_kf"], F0["cap_mp"]
    assert all((len(F["feat_mp"]), F["cap_kf"], F["cap_mp"]) == (stride, ck, cm) for F in frames)
    out = dict(local_kf=np.full((B, ck), -7, np.int32), n_local_kf=np.zeros(B, np.int32),
               ref_kf=np.zeros(B, np.int32), local_mp=np.full((B, cm), -7, np.int32),
               n_local_mp=np.full((B, 2), -7, np.int32),
               mps=np.frombuffer(b"\x5a" * (32 * B * cm), lc.MAP_POINT_DTYPE).reshape(B, cm).copy(),
               skip=np.full((B, cm), 9, np.uint8), mp_of_feat=np.full((B, stride), -7, np.int32),
               info=np.full(B, 0x77777777, np.uint32))
    for f, F in enumerate(frames):
        out["local_kf"][f] = F["local_kf"][:ck]
        out["n_local_kf"][f] = F["n_local_kf"]
        out["ref_kf"][f] = F["ref_kf"]
    return out, (B, stride, ck, cm)


def guarded(a, torch, dev):
    """A device copy of `a` with GUARD sentinel elements on both sides; the interior view."""
    flat = np.ascontiguousarray(a).reshape(-1)
    raw = flat.view(np.uint8)
    g = GUARD * flat.dtype.itemsize
    host = np.full(len(raw) + 2 * g, 0xc3, np.uint8)
    host[g:g + len(raw)] = raw
    t = torch.from_numpy(host).to(dev)
    return t, t[g:g + len(raw)], host


def run(view, frames, gpu, arrays_for_rec):
    """One call.  Returns (got, want): every output block with its guards, as bytes."""
    import torch
    from my_orb_slam2_amd.localmap import update_local_map
    out, (B, stride, ck, cm) = make_outputs(frames)
    feat = np.stack([F["feat_mp"] for F in frames])
    nfeat = np.array([F["nfeat"] for F in frames], np.int32)
    has_ol = any(F["outlier"] is not None for F in frames)
    ol = np.stack([F["outlier"] if F["outlier"] is not None else np.zeros(stride, np.uint8)
                   for F in frames]) if has_ol else None
    d_feat, d_nfeat = torch.from_numpy(feat).to(gpu), torch.from_numpy(nfeat).to(gpu)
    d_ol = torch.from_numpy(ol).to(gpu) if has_ol else None
    dev = {k: guarded(v, torch, gpu) for k, v in out.items()}
    update_local_map(view, B, d_feat, stride, d_nfeat, d_ol, ck, cm, dev["local_kf"][1],
                     dev["n_local_kf"][1], dev["ref_kf"][1], dev["local_mp"][1],
                     dev["n_local_mp"][1], dev["mps"][1], dev["skip"][1], dev["mp_of_feat"][1],
                     dev["info"][1])
    torch.cuda.synchronize()
    want = {k: v.copy() for k, v in out.items()}
    results = []
    for f, F in enumerate(frames):
        r = lc.update_local_map_np(arrays_for_rec, F)
        lc.apply_result(r, arrays_for_rec, F, want, f)
        results.append(r)
    got_b, want_b = {}, {}
    for k in out:
        got_b[k] = dev[k][0].cpu().numpy().tobytes()
        host = dev[k][2].copy()
        g = GUARD * out[k].dtype.itemsize
        host[g:len(host) - g] = np.ascontiguousarray(want[k]).reshape(-1).view(np.uint8)
        want_b[k] = host.tobytes()
    return got_b, want_b, results, dev


def check(got, want, name):
    for k in want:
        if got[k] != want[k]:
            g, w = np.frombuffer(got[k], np.uint8), np.frombuffer(want[k], np.uint8)
            at = int(np.flatnonzero(g != w)[0])
            pytest.fail(f"{name}: {k} differs from byte {at} ({g[at:at + 16]} != {w[at:at + 16]})")


def view_of(S, gpu):
    from my_orb_slam2_amd.localmap import LocalMapView
    return LocalMapView({k: S[k] for k in ARRAYS}, gpu.index or 0)


@pytest.mark.parametrize("case", lc.directed_cases(), ids=lambda c: c["name"])
def test_directed(case, orbx_lib, gpu):
    got, want, results, _ = run(view_of(case["S"], gpu), [case["F"]], gpu, case["S"])
    check(got, want, case["name"])
    if case["name"].startswith("cap_") and "over" in case["name"]:
        assert results[0]["refused"]


def carved_view(S, gpu):
    """The snapshot's arrays inside one zero-filled tensor, 4 KiB apart and 64 KiB from its ends:
    the address a small out-of-range index gives still lies inside it."""
    import torch
    from my_orb_slam2_amd.localmap import LocalMapView
    big = torch.zeros(128 * 1024 + 4096 * len(ARRAYS), dtype=torch.uint8, device=gpu)
    arrays, at = {}, 64 * 1024
    for k in ARRAYS:
        a = np.ascontiguousarray(S[k])
        raw = torch.from_numpy(a.reshape(-1).view(np.uint8).copy()).to(gpu)
        assert len(raw) <= 4096
        big[at:at + len(raw)] = raw
        piece = big[at:at + len(raw)]
        arrays[k] = piece if k in ("kf_bad", "mp_bad", "mp_rec") else piece.view(torch.int32)
        at += 4096
    v = LocalMapView(arrays, gpu.index or 0)
    v._big = big
    return v


@pytest.mark.parametrize("case", lc.bad_index_cases(), ids=lambda c: c["name"])
def test_bad_index_is_refused_without_a_stray_access(case, orbx_lib, gpu):
    got, want, results, _ = run(carved_view(case["S"], gpu), [case["F"]], gpu, case["S"])
    assert results[0]["refused"] and results[0]["info"] == lc.BAD_INDEX
    check(got, want, case["name"])


def test_healthy_twin_of_the_corrupt_snapshots_in_the_carved_tensor(orbx_lib, gpu):
    c = lc.bad_index_cases()[0]
    S = dict(c["S"], kf_order=np.array([1, 0, 2, 3, 5, 4], np.int32))
    got, want, results, _ = run(carved_view(S, gpu), [c["F"]], gpu, S)
    assert not results[0]["refused"] and results[0]["n_local"] > 0
    check(got, want, "healthy")


def test_mixed_batch_and_the_same_frames_one_per_call(orbx_lib, gpu):
    S, frames = lc.mixed_batch()
    view = view_of(S, gpu)
    got, want, results, _ = run(view, frames, gpu, S)
    infos = [r["info"] for r in results]
    assert infos == [0, lc.KEPT, lc.KEPT, lc.CAP_MP, lc.BAD_INDEX, 0]
    check(got, want, "mixed")
    # one frame per call: the same bytes as the frame's part of the batch
    for f, F in enumerate(frames):
        got1, want1, _, _ = run(view, [F], gpu, S)
        check(got1, want1, f"mixed[{f}] alone")
        for k, a in make_outputs(frames)[0].items():
            per = a[0].nbytes if a.ndim > 1 else a.itemsize
            lo = GUARD * a.itemsize
            assert got1[k][lo:lo + per] == got[k][lo + f * per:lo + (f + 1) * per], (f, k)


def test_no_frames_launches_nothing(orbx_lib, gpu):
    import torch
    from my_orb_slam2_amd.localmap import update_local_map
    S, frames = lc.mixed_batch()
    z = torch.full((64,), 5, dtype=torch.int32, device=gpu)
    update_local_map(view_of(S, gpu), 0, z, 8, z, None, 4, 4, z, z, z, z, z, z, z, z, z)
    torch.cuda.synchronize()
    assert (z.cpu().numpy() == 5).all()


@pytest.mark.parametrize("seed", range(1, 9))
def test_random_batches(seed, orbx_lib, gpu):
    S, frames = lc.random_batch(seed)
    got, want, results, _ = run(view_of(S, gpu), frames, gpu, S)
    assert not any(r["refused"] for r in results)
    check(got, want, f"random {seed}")


@pytest.mark.parametrize("name", ["extras_with_outliers", "parent_new_middle", "kept_temporal_only",
                                  "cap_mp_over"])
def test_host_array_form_equals_the_batched_form(name, orbx_lib, gpu):
    from my_orb_slam2_amd.localmap import update_local_map_host
    c = lc.case_named(name)
    S, F = c["S"], c["F"]
    r = lc.reference(c)
    n = F["nfeat"]
    h = update_local_map_host({k: S[k] for k in ARRAYS}, F["feat_mp"][:n], F["cap_kf"], F["cap_mp"],
                              local_kf=F["local_kf"][:F["n_local_kf"]], ref_kf=F["ref_kf"],
                              outlier=None if F["outlier"] is None else F["outlier"][:n])
    assert h["info"] == r["info"]
    if r["refused"]:
        # untouched: what update_local_map_host put in
        assert (h["local_mp"] == -1).all() and not h["skip"].any() and (h["mp_of_feat"] == -1).all()
        assert list(h["local_kf"]) == list(F["local_kf"][:F["n_local_kf"]])
        return
    want_kf = r["local_kf"]
    assert list(h["local_kf"]) == want_kf and h["ref_kf"] == r["ref_kf"]
    nb = len(r["block"])
    assert (h["n_local"], h["n_block"]) == (r["n_local"], nb)
    assert list(h["local_mp"][:nb]) == r["block"] and (h["local_mp"][nb:] == -1).all()
    assert h["mps"][:nb].tobytes() == S["mp_rec"][r["block"]].tobytes()
    assert h["mps"][nb:].tobytes() == bytes(32 * (F["cap_mp"] - nb))
    assert list(h["skip"][:nb]) == r["skip"] and (h["skip"][nb:] == 1).all()
    assert list(h["mp_of_feat"]) == r["mp_of_feat"]


def test_search_inputs_next_to_the_block(orbx_lib, gpu):
    import torch
    from my_orb_slam2_amd.localmap import local_map_search_inputs
    S, frames = lc.mixed_batch()
    view = view_of(S, gpu)
    got, want, results, dev = run(view, frames, gpu, S)
    check(got, want, "mixed")
    B, stride, cm = len(frames), len(frames[0]["feat_mp"]), frames[0]["cap_mp"]
    rng = np.random.default_rng(3)
    desc = rng.integers(0, 256, (S["n_mp"], 32), dtype=np.uint8)
    d_desc = torch.from_numpy(desc).to(gpu)
    d_nfeat = torch.tensor([F["nfeat"] for F in frames], dtype=torch.int32, device=gpu)
    d_qdesc = torch.full((B, cm, 32), 7, dtype=torch.uint8, device=gpu)
    d_claimed = torch.full((B, stride), 7, dtype=torch.uint8, device=gpu)
    i32 = lambda k: dev[k][1].view(torch.int32)
    local_map_search_inputs(view, d_desc, B, i32("local_mp"), i32("n_local_mp"), cm,
                            i32("mp_of_feat"), stride, d_nfeat, d_qdesc, d_claimed)
    torch.cuda.synchronize()
    qd, cl = d_qdesc.cpu().numpy(), d_claimed.cpu().numpy()
    for f, (F, r) in enumerate(zip(frames, results)):
        if r["refused"]:
            continue        # the block is what it was: guard values
        nb = len(r["block"])
        assert np.array_equal(qd[f, :nb], desc[r["block"]]) and not qd[f, nb:].any()
        has_obs = lambda m: S["mp_obs_off"][m + 1] > S["mp_obs_off"][m]
        want_cl = [int(k >= 0 and has_obs(r["block"][k])) for k in r["mp_of_feat"]]
        assert list(cl[f, :F["nfeat"]]) == want_cl and not cl[f, F["nfeat"]:].any()
    # a temporal point claims nothing, a point only bad keyframes observe does
    assert 0 in cl[0, :frames[0]["nfeat"]] and 1 in cl[5, :frames[5]["nfeat"]]


# ---- the chain: MonoTrackBatch.track_local_map against its stages one by one -------------------------

CW, CH, CB = 320, 240, 4
CK4, CDIST = (230.0, 231.0, 161.5, 118.5), (-0.12, 0.03, 0.0005, -0.0003)
N_PER, N_KF, CAP_KF, CAP_MP = 400, 150, 160, 1700


def _bytes(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(gpu)


def _chain_scene(mt, gpu):
    """A map of CB * N_PER MapPoints (N_PER around every frame's own features,
    synth.local_map_points) and 8 temporal ones, N_KF keyframes that each hold points of one
    frame's group and a few of the next, and per frame the features a first search already
    matched (every second match), one temporal point, one bad point and a few outliers."""
    import torch
    from my_orb_slam2_amd import synth
    from my_orb_slam2_amd.features import FRAME_POSE_DTYPE
    nkp, ku, desc = mt.fetch_undistorted()
    assert (nkp > 150).all()
    kc = mt.kp_cap
    lm = [synth.local_map_points(500 + j, ku[j, :nkp[j]], desc[j, :nkp[j]], N_PER, CK4, mt.bounds,
                                 width=CW, height=CH) for j in range(CB)]
    poses = np.stack([np.asarray(m[0], FRAME_POSE_DTYPE).reshape(()) for m in lm])
    n_mp = CB * N_PER + 8
    rec = np.concatenate([m[1] for m in lm] + [lm[0][1][:8]])
    mp_desc = np.concatenate([m[2] for m in lm] + [lm[1][2][:8]])
    # the first search: every frame against its own group, stage by stage on the device
    off = torch.arange(CB + 1, dtype=torch.int32, device=gpu) * N_PER
    d_q = torch.zeros(CB * N_PER * 32, dtype=torch.uint8, device=gpu)
    d_match = torch.full((CB * N_PER,), -7, dtype=torch.int32, device=gpu)
    d_cnt = torch.zeros(CB, dtype=torch.int32, device=gpu)
    mt.project_local_map(_bytes(poses, gpu), _bytes(rec[:CB * N_PER], gpu), off, N_PER,
                         torch.zeros(CB * N_PER, dtype=torch.uint8, device=gpu), d_q)
    mt.search_local_points(_bytes(mp_desc[:CB * N_PER], gpu), d_q, off, d_match, d_cnt)
    mt.matcher.sync()
    torch.cuda.synchronize()
    match = d_match.cpu().numpy().reshape(CB, N_PER)
    rng = np.random.default_rng(42)
    bad_mp = [int(m) for m in rng.choice(CB * N_PER, 40, replace=False)]
    feat_mp = np.full((CB, kc), -1, np.int32)
    outlier = np.zeros((CB, kc), np.uint8)
    for j in range(CB):
        held = [(int(match[j, q]), j * N_PER + q) for q in range(0, N_PER, 2) if match[j, q] >= 0]
        assert len(held) > 40
        for i, m in held:
            feat_mp[j, i] = m
        free = np.flatnonzero(feat_mp[j, :nkp[j]] < 0)
        feat_mp[j, free[0]] = CB * N_PER + j            # a temporal point
        feat_mp[j, free[1]] = bad_mp[j]                 # a bad one: nulled
        outlier[j, [i for i, _ in held[::9]]] = 1
    kf_mp, cov = [], []
    for k in range(N_KF):
        g = k % CB
        ids = np.concatenate([g * N_PER + rng.choice(N_PER, 40, replace=False),
                              ((g + 1) % CB) * N_PER + rng.choice(N_PER, 5, replace=False)])
        ids = rng.permutation(ids)
        ids[rng.random(len(ids)) < 0.2] = -1
        kf_mp.append([int(x) for x in ids])
        cov.append([int(x) for x in rng.choice(N_KF, int(rng.integers(0, 13)), replace=False)])
    lists = dict(order=[int(x) for x in rng.permutation(N_KF)],
                 bad_kf=[int(x) for x in rng.choice(N_KF, 12, replace=False)],
                 parent=[-1] + [int(rng.integers(0, k)) for k in range(1, N_KF)], cov=cov)
    S = lc.snapshot(N_KF, kf_mp, n_mp=n_mp, bad_mp=bad_mp, temporal=range(CB * N_PER, n_mp), rec=rec,
                    **lists)
    frames = [lc.frame(S, feat_mp[j, :nkp[j]], outlier=outlier[j, :nkp[j]], stride=kc,
                       cap_kf=CAP_KF, cap_mp=CAP_MP) for j in range(CB)]
    return S, lists, kf_mp, frames, poses, mp_desc, feat_mp, outlier, nkp


def test_track_local_map_equals_its_stages_and_replays_from_a_graph(orbx_lib, gpu):
    import torch
    from my_orb_slam2_amd import synth
    from my_orb_slam2_amd.localmap import LocalMapView
    from my_orb_slam2_amd.tracking import MonoTrackBatch
    imgs = np.stack([synth.frame(840 + i, CW, CH) for i in range(CB)])
    mt = MonoTrackBatch(CB, CW, CH, CK4, CDIST, nfeatures=500, device=gpu.index or 0)
    mt.frames(torch.from_numpy(imgs).to(gpu))
    S, lists, kf_mp, frames, poses, mp_desc, feat_mp, outlier, nkp = _chain_scene(mt, gpu)
    kc = mt.kp_cap
    # the view from plain lists (the children unsorted, as a caller has them)
    children = [[c for c in range(N_KF - 1, -1, -1) if lists["parent"][c] == k] for k in range(N_KF)]
    obs = [list(S["mp_obs"][S["mp_obs_off"][m]:S["mp_obs_off"][m + 1]]) for m in range(S["n_mp"])]
    view = LocalMapView.from_lists(lists["order"], S["kf_bad"], lists["parent"], lists["cov"],
                                   children, kf_mp, S["mp_bad"], obs, S["mp_rec"], gpu.index or 0)
    for k in ARRAYS:
        got = view.t[k].cpu().numpy()
        want = S[k].view(np.float32).reshape(-1, 8) if k == "mp_rec" else S[k]
        assert np.array_equal(got, want), k

    # -- the stages one by one, the restated update in the middle, host copies between them
    results = [lc.update_local_map_np(S, F) for F in frames]
    assert not any(r["refused"] or r["info"] for r in results)
    assert all(len(r["local_kf"]) > 30 and r["n_local"] > 300 and len(r["block"]) > r["n_local"]
               for r in results)
    out, _ = make_outputs(frames)
    for f, (F, r) in enumerate(zip(frames, results)):
        lc.apply_result(r, S, F, out, f)
    off = mt.local_map_offsets(CAP_MP)
    qdesc = np.zeros((CB, CAP_MP, 32), np.uint8)
    claimed = np.zeros((CB, kc), np.uint8)
    for f, r in enumerate(results):
        qdesc[f, :len(r["block"])] = mp_desc[r["block"]]
        for i, k in enumerate(r["mp_of_feat"]):
            m = r["block"][k] if k >= 0 else -1
            claimed[f, i] = m >= 0 and S["mp_obs_off"][m + 1] > S["mp_obs_off"][m]
    i32 = dict(dtype=torch.int32, device=gpu)
    host = lambda t: t.cpu().numpy().copy()
    d_q = torch.zeros(CB * CAP_MP * 32, dtype=torch.uint8, device=gpu)
    mt.project_local_map(_bytes(poses, gpu), _bytes(out["mps"], gpu), off, CAP_MP,
                         _bytes(out["skip"], gpu), d_q)
    torch.cuda.synchronize()
    want_q = host(d_q)
    d_match, d_cnt = torch.full((CB * CAP_MP,), -7, **i32), torch.full((CB,), -7, **i32)
    mt.search_local_points(_bytes(qdesc, gpu), _bytes(want_q, gpu), off, d_match, d_cnt,
                           _bytes(claimed, gpu))
    mt.matcher.sync()
    torch.cuda.synchronize()
    want_match, want_cnt = host(d_match), host(d_cnt)
    assert (want_cnt > 20).all()
    d_mpf, d_flag = torch.full((CB * kc,), -7, **i32), torch.full((1,), -7, **i32)
    mt.matches_to_features(torch.from_numpy(want_match).to(gpu), off, CAP_MP, d_mpf, d_flag,
                           torch.from_numpy(out["mp_of_feat"].reshape(-1)).to(gpu))
    torch.cuda.synchronize()
    want_mpf = host(d_mpf)
    assert int(d_flag.cpu()[0]) == 0
    new = (want_mpf.reshape(CB, kc) != out["mp_of_feat"]).sum(1)
    assert (new > 20).all()                              # the search added MapPoints to the held ones
    d_po, d_outl = torch.zeros(poses.nbytes, dtype=torch.uint8, device=gpu), \
        torch.full((CB * kc,), 0xA5, dtype=torch.uint8, device=gpu)
    d_ng, d_pinfo = torch.full((CB,), -7, **i32), torch.full((CB,), -7, **i32)
    mt.pose_optimization(_bytes(poses, gpu), torch.from_numpy(want_mpf).to(gpu),
                         _bytes(out["mps"], gpu), off, d_po, d_outl, d_ng, d_pinfo)
    torch.cuda.synchronize()
    want = dict(q=want_q, match=want_match, cnt=want_cnt, mpf=want_mpf, po=host(d_po),
                outl=host(d_outl), ng=host(d_ng), pinfo=host(d_pinfo))
    assert (want["ng"] >= 10).all()

    # -- the chain, on one stream
    def buffers():
        b = dict(local_kf=torch.full((CB, CAP_KF), -7, **i32), n_local_kf=torch.zeros(CB, **i32),
                 ref_kf=torch.full((CB,), -1, **i32), local_mp=torch.full((CB, CAP_MP), -7, **i32),
                 n_local_mp=torch.full((CB, 2), -7, **i32),
                 mps=torch.full((CB * CAP_MP * 32,), 0x5a, dtype=torch.uint8, device=gpu),
                 skip=torch.full((CB, CAP_MP), 9, dtype=torch.uint8, device=gpu),
                 prior=torch.full((CB, kc), -7, **i32), lm_info=torch.full((CB,), -7, **i32),
                 q=torch.zeros(CB * CAP_MP * 32, dtype=torch.uint8, device=gpu),
                 qdesc=torch.full((CB, CAP_MP, 32), 7, dtype=torch.uint8, device=gpu),
                 claimed=torch.full((CB, kc), 7, dtype=torch.uint8, device=gpu),
                 match=torch.full((CB * CAP_MP,), -7, **i32), cnt=torch.full((CB,), -7, **i32),
                 mpf=torch.full((CB * kc,), -7, **i32), flag=torch.full((1,), -7, **i32),
                 po=torch.zeros(poses.nbytes, dtype=torch.uint8, device=gpu),
                 outl=torch.full((CB * kc,), 0xA5, dtype=torch.uint8, device=gpu),
                 ng=torch.full((CB,), -7, **i32), pinfo=torch.full((CB,), -7, **i32))
        return b

    d_desc, d_feat = torch.from_numpy(mp_desc).to(gpu), torch.from_numpy(feat_mp).to(gpu)
    d_ol, d_poses = torch.from_numpy(outlier).to(gpu), _bytes(poses, gpu)

    def chain(b, stream=0):
        mt.track_local_map(view, d_desc, d_feat, d_ol, CAP_KF, CAP_MP, b["local_kf"],
                           b["n_local_kf"], b["ref_kf"], b["local_mp"], b["n_local_mp"], b["mps"],
                           b["skip"], b["prior"], b["lm_info"], d_poses, b["q"], b["qdesc"],
                           b["claimed"], b["match"], b["cnt"], b["mpf"], b["flag"], b["po"],
                           b["outl"], b["ng"], b["pinfo"], stream=stream)

    def compare(b, what):
        assert not host(b["lm_info"]).any(), what
        for k, t in (("local_kf", "local_kf"), ("n_local_kf", "n_local_kf"), ("ref_kf", "ref_kf"),
                     ("local_mp", "local_mp"), ("n_local_mp", "n_local_mp"), ("skip", "skip"),
                     ("mp_of_feat", "prior")):
            assert np.array_equal(host(b[t]).reshape(out[k].shape), out[k]), (what, k)
        assert host(b["mps"]).tobytes() == out["mps"].tobytes(), what
        assert np.array_equal(host(b["qdesc"]), qdesc) and np.array_equal(host(b["claimed"]), claimed)
        for k in ("q", "match", "cnt", "mpf", "po", "outl", "ng", "pinfo"):
            assert host(b[k]).tobytes() == want[k].tobytes(), (what, k)
        assert int(b["flag"].cpu()[0]) == 0

    b = buffers()
    chain(b)
    mt.matcher.sync()
    torch.cuda.synchronize()
    compare(b, "eager")

    # -- captured once, replayed into fresh buffers: nothing in the chain reads the host
    b = buffers()
    s = torch.cuda.Stream(gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        chain(b, s.cuda_stream)
    for k, t in buffers().items():       # the capture ran nothing: the buffers as they were before
        b[k].copy_(t)
    torch.cuda.synchronize()
    assert (host(b["lm_info"]) == -7).all() and (host(b["ng"]) == -7).all()
    with torch.cuda.stream(s):
        g.replay()
    s.synchronize()
    compare(b, "graph replay")
