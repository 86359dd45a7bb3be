#!/usr/bin/env python3
"""Cost of the per-match loop of CreateNewMapPoints on the device (k_triangulate_points) next to
the SearchForTriangulation it follows.

    python tools/triangulate_step.py [--jobs 512] [--out profiles/triangulate_step.json]

The local-mapping job list of bench.py's triangulation workload: `--jobs` keyframe pairs of 2000
features each (`--distinct` different pairs, tiled), resident as one orbx_kf_db with node order,
30 % of the features with a MapPoint, 30 % stereo.  One process alternates

  search        search_for_triangulation_batch_device          the search alone
  search_tri    search_and_triangulate_batch_device            + k_triangulate_points, no host step
  search_d2h    the search, then its matches copied to the host (what a host loop needs first)

each timed over a window of `steps` calls (sized from a calibration step so that a window lasts
about --window seconds), `--repeats` windows each, alternating: device events for the first two,
the wall clock around search + copy + synchronise for the third.  The host loop itself is the
cv::Mat restatement tests/native/triangulate_ref (one thread, the cv stand-in) run once on the
distinct jobs' matches; its seconds per pair times the pairs of all jobs is added to search_d2h as
`search_host_loop`.  The kernel's share of the step is (search_tri - search) / search_tri.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import pathlib
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375     # synth.keyframe_pair's camera
W, H, NFEAT, MBF = 752, 480, 2000, 47.9


def second_pose(seed, baseline=0.5):
    """The pose synth.keyframe_pair(seed) gives its second keyframe (the first is the identity)."""
    from my_orb_slam2_amd import synth
    rng = np.random.default_rng(seed + 7919)
    R2w = synth._rot(rng, 5.0)
    C2w = baseline * np.array([rng.uniform(-1, 1), rng.uniform(-0.2, 0.2), rng.uniform(-1.2, 1.2)])
    return R2w, -R2w @ C2w


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=512)
    ap.add_argument("--distinct", type=int, default=32, help="distinct keyframe pairs, tiled")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.5, help="seconds per timed window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "triangulate_step.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("triangulate_step: no GPU visible; nothing measured", file=sys.stderr)
        return 2
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd import build as b
    from my_orb_slam2_amd import synth
    from my_orb_slam2_amd.features import FRAME_POSE_DTYPE, frame_pose
    from my_orb_slam2_amd.matcher import DeviceKfDb, parallax_stereo_cos

    dev = torch.device("cuda", 0)
    f32 = np.float32
    k = min(a.distinct, a.jobs)
    s, s2, _ = synth.scale_tables()
    mb = f32(f32(MBF) / f32(FX))
    ratio_factor = f32(f32(1.5) * f32(1.2))
    K4, bounds = (FX, FY, CX, CY), (0.0, float(W), 0.0, float(H))
    kfs, flags, poses, F12, epi, depth, cos, ur = [], [], [], [], [], [], [], []
    for j in range(k):
        k1, k2, F, e, _ = synth.keyframe_pair(10000 + j, n1=NFEAT, n2=NFEAT, nodes=100)
        rng = np.random.default_rng(j)
        R2, t2 = second_pose(10000 + j)
        kfs += [k1, k2]
        flags += [rng.random(k1.n) < 0.3, rng.random(k2.n) < 0.3]
        poses += [frame_pose(np.eye(3), np.zeros(3), K4, bounds, s, MBF),
                  frame_pose(R2, t2, K4, bounds, s, MBF)]
        F12.append(F.reshape(9))
        epi.append(e)
        for fs in (k1, k2):
            u = np.full(fs.n, -1, f32) if fs.u_right is None else np.asarray(fs.u_right, f32)
            with np.errstate(all="ignore"):
                d = np.where(u >= 0, f32(MBF) / (fs.keys["x"] - u), f32(-1)).astype(f32)
            ur.append(u)
            depth.append(d)
            cos.append(parallax_stereo_cos(mb, d))
    matcher = m.ORBmatcher(0.6, False)
    db = DeviceKfDb(kfs, flags, dev).node_order(matcher)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    idx = np.arange(a.jobs) % k
    kf1, kf2 = T((2 * idx).astype(np.int32)), T((2 * idx + 1).astype(np.int32))
    n1 = np.array([kfs[2 * i].n for i in idx], np.int32)
    job_off_h = np.concatenate([[0], np.cumsum(n1)]).astype(np.int32)
    slots = int(job_off_h[-1])
    job_off = T(job_off_h)
    d_F, d_epi = T(np.array(F12, f32)[idx]), T(np.array(epi, f32)[idx])
    d_poses = T(np.concatenate([p.reshape(1) for p in poses]).astype(FRAME_POSE_DTYPE)
                .view(np.uint8).reshape(-1))
    d_depth, d_cos = T(np.concatenate(depth)), T(np.concatenate(cos))
    d_match = torch.full((slots,), -1, dtype=torch.int32, device=dev)
    d_cnt = torch.zeros(a.jobs, dtype=torch.int32, device=dev)
    d_status = torch.zeros(slots, dtype=torch.int32, device=dev)
    d_x3d = torch.zeros(slots, 3, dtype=torch.float32, device=dev)
    d_nnew = torch.zeros(a.jobs, dtype=torch.int32, device=dev)
    h_match = torch.empty(slots, dtype=torch.int32).pin_memory()

    def search():
        matcher.search_for_triangulation_batch_device(db.c, kf1, kf2, d_F, d_epi, s2, s, job_off,
                                                      d_match, d_cnt)

    def search_tri():
        matcher.search_and_triangulate_batch_device(db.c, kf1, kf2, d_F, d_epi, s2, s, job_off,
                                                    d_match, d_cnt, d_poses, d_depth, d_cos,
                                                    ratio_factor, d_status, d_x3d, d_nnew, mb=mb)

    def search_d2h():
        search()
        h_match.copy_(d_match, non_blocking=True)
        torch.cuda.synchronize()

    def window_events(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    def window_wall(fn, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / steps

    work = {"search": (search, window_events), "search_tri": (search_tri, window_events),
            "search_d2h": (search_d2h, window_wall)}
    steps = {}
    for name, (fn, win) in work.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        steps[name] = max(3, math.ceil(a.window * 1e3 / max(win(fn, 5), 1e-3)))
    times = {name: [] for name in work}
    for _ in range(a.repeats):
        for name, (fn, win) in work.items():       # alternate within every repeat
            times[name].append(win(fn, steps[name]))
    matcher.sync()
    med = {n: float(np.median(t)) for n, t in times.items()}

    # the host loop: the cv::Mat restatement on the distinct jobs' matches
    import triangulate_cases as tc
    from test_triangulate_cases import run_ref
    search_tri()
    torch.cuda.synchronize()
    match, status = d_match.cpu().numpy(), d_status.cpu().numpy()
    cases = []
    for j in range(k):
        seg = match[job_off_h[j]:job_off_h[j + 1]]
        i1 = np.nonzero(seg >= 0)[0]
        cases.append(tc.make(f"job{j}", poses[2 * j], poses[2 * j + 1], kfs[2 * j].keys,
                             kfs[2 * j + 1].keys, np.stack([i1, seg[i1]], 1), ur1=ur[2 * j],
                             ur2=ur[2 * j + 1], depth1=depth[2 * j], depth2=depth[2 * j + 1],
                             cos1=cos[2 * j], cos2=cos[2 * j + 1], mb=mb, ratio_factor=ratio_factor))
    ref_bin = b.build_triangulate_ref()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        ref = run_ref(ref_bin, cases, tmp)
        r = subprocess.run([str(ref_bin), str(tmp / "cases.bin"), str(tmp / "out.bin")],
                           capture_output=True, text=True, check=True)
    words = r.stdout.split()
    loop_s, loop_pairs = float(words[1]), int(words[3])
    agree = all(np.array_equal(status[job_off_h[j]:job_off_h[j + 1]][c["pairs"][:, 0]], st)
                for j, (c, (st, _)) in enumerate(zip(cases, ref)))
    pairs_all = int((match >= 0).sum())
    host_loop_ms = loop_s / max(loop_pairs, 1) * pairs_all * 1e3
    share = [(t - s_) / t for t, s_ in zip(times["search_tri"], times["search"])]
    res = {
        "tool": "tools/triangulate_step.py", "device": torch.cuda.get_device_name(0),
        "settings": {"jobs": a.jobs, "distinct_pairs": k, "features_per_keyframe": NFEAT,
                     "steps": steps, "repeats": a.repeats,
                     "timing": "device events around `steps` calls (search, search_tri); wall "
                               "clock around search + D2H copy + synchronise (search_d2h)"},
        "ms_per_step": {n: {"median": med[n], "min": float(min(t)), "max": float(max(t)),
                            "repeats": [float(v) for v in t]} for n, t in times.items()},
        "kernel_ms": med["search_tri"] - med["search"],
        "kernel_share_of_step": float(np.median(share)),
        "kernel_share_spread": [float(min(share)), float(max(share))],
        "jobs_per_second": {"search": a.jobs / (med["search"] * 1e-3),
                            "search_tri": a.jobs / (med["search_tri"] * 1e-3)},
        "matches_per_call": pairs_all, "new_points_per_call": int(d_nnew.sum().item()),
        "host_loop": {"program": "tests/native/triangulate_ref (one thread, cv stand-in)",
                      "pairs_timed": loop_pairs, "seconds": loop_s,
                      "us_per_pair": loop_s / max(loop_pairs, 1) * 1e6,
                      "ms_for_all_jobs": host_loop_ms,
                      "statuses_equal_the_device": bool(agree)},
        "search_host_loop_ms": med["search_d2h"] + host_loop_ms,
    }
    out = pathlib.Path(a.out)
    os.makedirs(out.parent, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k2: res[k2] for k2 in ("kernel_ms", "kernel_share_of_step",
                                            "search_host_loop_ms", "matches_per_call")}))
    print(json.dumps(med))
    return 0


if __name__ == "__main__":
    sys.exit(main())
