#!/usr/bin/env python3
"""Cost of Sim3Solver::iterate on the device (k_sim3_prepare, k_sim3_hypotheses, k_sim3_select)
for the candidates of a loop detection.

    python tools/sim3_step.py [--out profiles/sim3_step.json]

EuRoC intrinsics, 8 distinct candidate jobs of about 100 correspondences each (a third of them
displaced), tiled to 8 and to 256 jobs per call; minInliers 20, 300 iterations at most, as
LoopClosing::ComputeSim3 sets them.  One process alternates

  find       iterate(mRansacMaxIts): every iteration of every job in one call
  iterate5   iterate(5), LoopClosing's round-robin step

for both job counts, each timed with device events over a window of `steps` calls (sized from a
calibration step so that a window lasts about --window seconds), `--repeats` windows each,
alternating.  Every call starts from a zeroed state (a 2 KiB memset inside the window), so the
same iterations are timed every time.  The device scores every iteration of the call; the
reference, and tests/native/sim3_ref (one thread) beside it for the same distinct jobs, stop at
the first returned model, so its time depends on where that is (recorded as
`iterations_until_return`).
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

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

DISTINCT, N, MIN_INLIERS, MAX_ITERATIONS = 8, 100, 20, 300


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sim3_step.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        print("sim3_step: no GPU visible; nothing measured", file=sys.stderr)
        return 2
    import sim3_cases as sc
    from my_orb_slam2_amd import ORBmatcher
    from my_orb_slam2_amd import build as b
    from my_orb_slam2_amd.features import FRAME_POSE_DTYPE
    from my_orb_slam2_amd.sim3 import (SIM3_JOB_DTYPE, SIM3_RESULT_DTYPE, SIM3_STATE_DTYPE,
                                       sim3_ransac_iterations, sim3_sample_triples)
    dev = torch.device("cuda", 0)
    T = lambda x: torch.from_numpy(np.frombuffer(np.ascontiguousarray(x).tobytes(), np.uint8).copy()).to(dev)
    cases = [sc.make_case(f"cand{j}", 500 + j, N - 4 + j, n_outliers=N // 3, noise=0.5,
                          min_inliers=MIN_INLIERS, max_iterations=MAX_ITERATIONS, sparse_i1=True,
                          rot=(0.05 * j, -0.1, 0.02 * j), calls=(MAX_ITERATIONS,))
             for j in range(DISTINCT)]
    max_its = [sim3_ransac_iterations(c["prob"], MIN_INLIERS, MAX_ITERATIONS, len(c["corr"]))
               for c in cases]
    tri = [sim3_sample_triples(len(c["corr"]), c["rand"][:3 * m]) for c, m in zip(cases, max_its)]
    matcher = ORBmatcher(0.75, True)

    def setup(njobs, n_iterations):
        idx = np.arange(njobs) % DISTINCT
        corr_off = np.cumsum([0] + [len(cases[i]["corr"]) for i in idx])
        tri_off = np.cumsum([0] + [len(tri[i]) for i in idx])
        inl_off = np.cumsum([0] + [cases[i]["mN1"] for i in idx])
        jobs = np.zeros(njobs, SIM3_JOB_DTYPE)
        for j, i in enumerate(idx):
            jobs[j] = sc.job_of(cases[i], max_its[i], n_iterations, kf1=2 * j, kf2=2 * j + 1,
                                corr_off=corr_off[j], inlier_off=inl_off[j], triple_off=tri_off[j])
        poses = np.concatenate([np.stack([np.asarray(cases[i][k], FRAME_POSE_DTYPE).reshape(())
                                          for k in ("pose1", "pose2")]) for i in idx])
        d = dict(jobs=T(jobs), poses=T(poses), corr=T(np.concatenate([cases[i]["corr"] for i in idx])),
                 tri=T(np.concatenate([tri[i] for i in idx]).astype(np.int32)),
                 state=T(np.zeros(njobs, SIM3_STATE_DTYPE)),
                 res=T(np.zeros(njobs, SIM3_RESULT_DTYPE)),
                 inl=torch.zeros(int(inl_off[-1]), dtype=torch.uint8, device=dev))
        max_n = max(len(c["corr"]) for c in cases)
        max_call = min(max(max_its), n_iterations)

        def step():
            d["state"].zero_()
            matcher.sim3_iterate_batch_device(d["jobs"], njobs, max_n, max_call, d["poses"], d["corr"],
                                              d["tri"], d["state"], d["res"], d["inl"])
        return step, d, inl_off

    def window(fn, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    work = {f"{name}_{njobs}": setup(njobs, n_it)
            for njobs in (8, 256) for name, n_it in (("find", MAX_ITERATIONS), ("iterate5", 5))}
    steps = {}
    for name, (fn, _, _) in work.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        steps[name] = max(3, math.ceil(a.window * 1e3 / max(window(fn, 5), 1e-3)))
    times = {name: [] for name in work}
    for _ in range(a.repeats):
        for name, (fn, _, _) in work.items():          # alternate within every repeat
            times[name].append(window(fn, steps[name]))
    matcher.sync()

    # the restatement on the distinct jobs, one thread, and its results against the device's
    ref_bin = b.build_sim3_ref()
    report = {}
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        for name, n_it in (("find", MAX_ITERATIONS), ("iterate5", 5)):
            cs = [dict(c, calls=(n_it,)) for c in cases]
            sc.write_cases(tmp / "cases.bin", cs)
            subprocess.run([str(ref_bin), str(tmp / "cases.bin"), str(tmp / "out.bin")], check=True)
            ref = sc.read_results(tmp / "out.bin", cs)
            ms = [float(subprocess.run([str(ref_bin), "--time", str(tmp / "cases.bin"), "20"],
                                       check=True, capture_output=True, text=True).stdout)
                  for _ in range(3)]
            _, d, inl_off = work[f"{name}_8"]
            res = np.frombuffer(d["res"].cpu().numpy().tobytes(), SIM3_RESULT_DTYPE)
            inl = d["inl"].cpu().numpy()
            agree = all(sc.canon(res[j:j + 1].tobytes()) == sc.canon(ref[j][0][0]) and
                        inl[inl_off[j]:inl_off[j + 1]].tobytes() == ref[j][0][1]
                        for j in range(DISTINCT))
            report[name] = {"program": "tests/native/sim3_ref --time (one thread)",
                            "ms_per_8_jobs": float(np.median(ms)), "runs": ms,
                            "equals_the_device": bool(agree),
                            "iterations_until_return": [int(r[0][2][0]) for r in ref]}
    med = {n: float(np.median(t)) for n, t in times.items()}
    out = {"tool": "tools/sim3_step.py", "device": torch.cuda.get_device_name(0),
           "timing": "device events around `steps` calls, each a state memset and the three kernels",
           "settings": {"distinct_jobs": DISTINCT, "correspondences": [len(c["corr"]) for c in cases],
                        "max_its": max_its, "min_inliers": MIN_INLIERS, "steps": steps,
                        "repeats": a.repeats},
           "ms_per_call": {n: {"median": med[n], "min": float(min(t)), "max": float(max(t)),
                               "repeats": [float(v) for v in t]} for n, t in times.items()},
           "us_per_job": {n: 1e3 * med[n] / int(n.rsplit("_", 1)[1]) for n in med},
           "restatement": report,
           "device_slower_than_one_thread_at_8_jobs": {
               k: bool(med[f"{k}_8"] > report[k]["ms_per_8_jobs"]) for k in report}}
    p = pathlib.Path(a.out)
    os.makedirs(p.parent, exist_ok=True)
    p.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({"ms_per_call": med, "restatement_ms_per_8_jobs":
                      {k: v["ms_per_8_jobs"] for k, v in report.items()},
                      "equal": {k: v["equals_the_device"] for k, v in report.items()},
                      "iterations_until_return": report["find"]["iterations_until_return"]}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
