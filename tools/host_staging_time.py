#!/usr/bin/env python3
"""Host wall-clock per call of eight host-array entry points: one of each staging style of the
handle-free ones, and four of a matcher handle.

    python tools/host_staging_time.py [--lib PATH/liborbx.so] [--calls 300] [--warmup 30]
                                         [--cases bow,proj,tri,bf]

  remap      orbx_remap at 752 x 480 (the glue's Rectifier, once per image)
  rgbd       orbx_compute_stereo_from_rgbd at 640 x 480 uint16 with 1000 keypoints
  poseopt    orbx_pose_optimization on the directed case count_3_mono
  frustum    orbx_is_in_frustum with 1000 MapPoints
  bow        orbx_search_by_bow_kf_frame, 1000 features each
  proj       orbx_search_by_projection (FRAME_MAPPOINTS), 1000 queries on a 1000-feature target
  tri        orbx_search_for_triangulation, 1000 features against 1000
  bf         orbx_hamming_bf_top2, 1000 queries against 20000 rows

Each matcher case has an ORBmatcher of its own, created once.

One process makes `warmup` calls of an entry point, then times `calls` single calls with
time.perf_counter_ns and prints the median, the quartiles and the minimum in microseconds, one
line per entry point.  It writes no file.  To compare two builds, run it in turns with --lib
pointing at each library, at least three times each, and compare the medians of the medians with
the spread of one build's own repeats.
"""
from __future__ import annotations

import argparse
import os
import pathlib
import sys
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))


def cases():
    import poseopt_cases
    from my_orb_slam2_amd import ORBmatcher, Rectifier, synth
    from my_orb_slam2_amd._lib import KEYPOINT_DTYPE
    from my_orb_slam2_amd.features import (compute_stereo_from_rgbd, is_in_frustum,
                                           PROJ_FRAME_MAPPOINTS, pose_optimization)
    rng = np.random.default_rng(1)

    w, h = 752, 480
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    rect = Rectifier(xx * np.float32(0.98) + np.float32(3.25), yy * np.float32(0.99) + xx * np.float32(0.004))
    src = rng.integers(0, 256, (h, w), dtype=np.uint8)
    dst = np.zeros((h, w), np.uint8)

    depth = rng.integers(0, 40000, (480, 640)).astype(np.uint16)
    kps = np.zeros(1000, KEYPOINT_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 639, 1000), rng.uniform(0, 479, 1000)

    c = poseopt_cases.case_named("count_3_mono")

    keys = np.zeros(800, KEYPOINT_DTYPE)
    keys["x"], keys["y"] = rng.uniform(20, 732, 800), rng.uniform(20, 460, 800)
    keys["octave"] = rng.integers(0, 8, 800)
    F, mps, _, skip = synth.local_map_points(3, keys, rng.integers(0, 256, (800, 32), dtype=np.uint8),
                                             1000, synth.EUROC_CAM[0], (0.0, 752.0, 0.0, 480.0),
                                             mbf=40.0)

    b1, b2, bt = synth.feature_pair(2, n1=1000, n2=1000)
    valid = rng.random(1000) < 0.85
    pq, pd = synth.projection_queries(2, b1, b2, bt, th=7.0)
    k1, k2, F12, epi, _ = synth.keyframe_pair(2, n1=1000, n2=1000)
    has1, has2 = rng.random(1000) < 0.3, rng.random(1000) < 0.3
    scale, sigma2, _ = synth.scale_tables()
    bq = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    bdb = rng.integers(0, 256, (20000, 32), dtype=np.uint8)
    m_bow, m_proj, m_tri, m_bf = (ORBmatcher(0.75, True), ORBmatcher(0.8, True),
                                  ORBmatcher(0.6, False), ORBmatcher())
    return [
        ("remap", lambda: rect.remap(src, dst)),
        ("rgbd", lambda: compute_stereo_from_rgbd(depth, 1.0 / 5000.0, 40.0, kps)),
        ("poseopt", lambda: pose_optimization(c["pose"], c["keys"], c["mp_of_feat"], c["mps"],
                                              c["ur"], c["outlier_in"])),
        ("frustum", lambda: is_in_frustum(F, mps, skip)),
        ("bow", lambda: m_bow.search_by_bow_kf_frame(b1, valid, b2)),
        ("proj", lambda: m_proj.search_by_projection(PROJ_FRAME_MAPPOINTS, b2, pq, pd, orb_dist=64)),
        ("tri", lambda: m_tri.SearchForTriangulation(k1, has1, k2, has2, F12, epi, sigma2, scale)),
        ("bf", lambda: m_bf.hamming_bf_top2(bq, bdb)),
    ]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="the liborbx.so to time (default: the tree's)")
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--cases", help="comma-separated entry points to time (default: all)")
    a = ap.parse_args()
    if a.lib:
        os.environ["ORBX_LIB"] = str(pathlib.Path(a.lib).resolve())
    from my_orb_slam2_amd._lib import load
    print("library", load().orbx_version().decode(), flush=True)
    for name, fn in cases():
        if a.cases and name not in a.cases.split(","):
            continue
        for _ in range(a.warmup):
            fn()
        t = np.empty(a.calls)
        for i in range(a.calls):
            t0 = time.perf_counter_ns()
            fn()
            t[i] = (time.perf_counter_ns() - t0) / 1e3
        q1, med, q3 = np.percentile(t, [25, 50, 75])
        print(f"{name:8s} median_us {med:9.1f}  q1 {q1:9.1f}  q3 {q3:9.1f}  min {t.min():9.1f}  "
              f"calls {a.calls}", flush=True)


if __name__ == "__main__":
    main()
