#!/usr/bin/env python3
"""Cost of Tracking::UpdateLocalMap on the device (k_update_local_map) against the host round trip
it removes.

    python tools/localmap_step.py [--batch 256] [--out profiles/localmap_step.json]

A synthetic map along a trajectory: --keyframes keyframes of 1000 features each, a quarter of them
holding MapPoints out of the keyframe's window of 600 ids (windows 60 ids apart, so about ten
keyframes on either side share points), up to 15 ordered covisibles, the predecessor as parent.
B frames, each somewhere on the trajectory with 1000 features, 400 of them on MapPoints of the
window there and 5 % of those flagged as outliers: about 20 voted keyframes and about 2000 local
MapPoints per frame (the C3 shape of tests/test_gpu_bench_geometry.py).  One process alternates

  device      orbx_update_local_map_batch_device, device events around a window of calls
  round_trip  what the parent commit's caller does instead, wall clock: mp_of_feat and the outlier
              flags to pinned host memory and a synchronise; (the walk, below); the records gathered
              on the host into the pinned block; the block, the skip flags and mp_of_feat back to the
              device and a synchronise.  The copies and the gather are timed here; the walk is
              tests/native/localmap_ref --time on one core, on --distinct of the frames, scaled to B.

The device's lists, reference keyframes and local points of those frames are checked against
localmap_ref's before anything is timed.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import pathlib
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

FEATS, HELD, WINDOW, STEP, FILL, KP_CAP = 1000, 400, 600, 60, 0.25, 1024
CAP_KF, CAP_MP = 128, 4096


def scene(n_kf: int, seed: int = 0):
    import localmap_cases as lc
    rng = np.random.default_rng(seed)
    n_mp = (n_kf - 1) * STEP + WINDOW
    per = int(FILL * FEATS)
    kf_mp = np.full((n_kf, FEATS), -1, np.int32)
    for k in range(n_kf):
        kf_mp[k, rng.choice(FEATS, per, replace=False)] = k * STEP + rng.choice(WINDOW, per, replace=False)
    kf_of = np.repeat(np.arange(n_kf, dtype=np.int32), FEATS)
    flat = kf_mp.reshape(-1)
    has = flat >= 0
    by_id = np.argsort(flat[has], kind="stable")
    obs = kf_of[has][by_id]
    obs_off = np.zeros(n_mp + 1, np.int32)
    obs_off[1:] = np.cumsum(np.bincount(flat[has], minlength=n_mp))
    cov = [[c for d in range(1, 9) for c in (k - d, k + d) if 0 <= c < n_kf][:15] for k in range(n_kf)]
    cov_off = np.zeros(n_kf + 1, np.int32)
    cov_off[1:] = np.cumsum([len(r) for r in cov])
    child = [[k + 1] if k + 1 < n_kf else [] for k in range(n_kf)]
    child_off = np.zeros(n_kf + 1, np.int32)
    child_off[1:] = np.cumsum([len(r) for r in child])
    S = dict(n_kf=n_kf, n_mp=n_mp, kf_order=rng.permutation(n_kf).astype(np.int32),
             kf_bad=(rng.random(n_kf) < 0.02).astype(np.uint8),
             kf_parent=np.arange(-1, n_kf - 1, dtype=np.int32),
             kf_cov_off=cov_off, kf_cov=np.array([c for r in cov for c in r], np.int32),
             kf_child_off=child_off, kf_child=np.array([c for r in child for c in r], np.int32),
             kf_mp_off=(np.arange(n_kf + 1) * FEATS).astype(np.int32), kf_mp=flat.copy(),
             mp_bad=(rng.random(n_mp) < 0.02).astype(np.uint8), mp_obs_off=obs_off, mp_obs=obs,
             mp_rec=lc.records(n_mp))
    for n, a in (("n_cov", "kf_cov"), ("n_child", "kf_child"), ("n_kfmp", "kf_mp"), ("n_obs", "mp_obs")):
        S[n] = len(S[a])
    return S


def frames_of(S, B: int, seed: int = 1):
    rng = np.random.default_rng(seed)
    feat = np.full((B, KP_CAP), -1, np.int32)
    outlier = np.zeros((B, KP_CAP), np.uint8)
    for f in range(B):
        c = int(rng.integers(0, S["n_kf"]))
        at = rng.choice(FEATS, HELD, replace=False)
        feat[f, at] = c * STEP + rng.integers(0, WINDOW, HELD)
        outlier[f, at[rng.random(HELD) < 0.05]] = 1
    return feat, outlier, np.full(B, FEATS, np.int32)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--keyframes", type=int, default=1000)
    ap.add_argument("--distinct", type=int, default=4, help="frames the one-core walk is timed on")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.3, help="seconds per timed window")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "localmap_step.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("localmap_step: no GPU visible; nothing measured", file=sys.stderr)
        return 2
    import localmap_cases as lc
    from my_orb_slam2_amd import build as b
    from my_orb_slam2_amd.localmap import LocalMapView, update_local_map
    dev = torch.device("cuda", 0)
    B = a.batch
    S = scene(a.keyframes)
    feat, outlier, nfeat = frames_of(S, B)
    names = ("kf_order", "kf_bad", "kf_parent", "kf_cov_off", "kf_cov", "kf_child_off", "kf_child",
             "kf_mp_off", "kf_mp", "mp_bad", "mp_obs_off", "mp_obs", "mp_rec")
    view = LocalMapView({k: S[k] for k in names})
    i32 = dict(dtype=torch.int32, device=dev)
    d_feat, d_ol, d_nfeat = (torch.from_numpy(x).to(dev) for x in (feat, outlier, nfeat))
    d_lkf, d_nlkf, d_ref = torch.zeros((B, CAP_KF), **i32), torch.zeros(B, **i32), torch.full((B,), -1, **i32)
    d_lmp, d_nlmp = torch.zeros((B, CAP_MP), **i32), torch.zeros((B, 2), **i32)
    d_mps = torch.zeros((B, CAP_MP, 8), dtype=torch.float32, device=dev)
    d_skip = torch.zeros((B, CAP_MP), dtype=torch.uint8, device=dev)
    d_mpf, d_info = torch.zeros((B, KP_CAP), **i32), torch.zeros(B, **i32)

    def device():
        update_local_map(view, B, d_feat, KP_CAP, d_nfeat, d_ol, CAP_KF, CAP_MP, d_lkf, d_nlkf, d_ref,
                         d_lmp, d_nlmp, d_mps, d_skip, d_mpf, d_info)

    device()
    torch.cuda.synchronize()
    info, nlkf, nlmp = d_info.cpu().numpy(), d_nlkf.cpu().numpy(), d_nlmp.cpu().numpy()
    assert not info.any(), sorted(set(int(v) for v in info))
    lkf, lmp, ref = d_lkf.cpu().numpy(), d_lmp.cpu().numpy(), d_ref.cpu().numpy()

    # the one-core walk on the first --distinct frames, and its results against the device's
    k = min(a.distinct, B)
    cases = [dict(name=f"f{f}", S=S, F=lc.frame(S, feat[f, :FEATS], outlier=outlier[f, :FEATS],
                                                 stride=KP_CAP, cap_kf=CAP_KF, cap_mp=CAP_MP))
             for f in range(k)]
    exe = b.build_localmap_ref()
    with tempfile.TemporaryDirectory() as tmp:
        tmp = pathlib.Path(tmp)
        lc.write_cases(tmp / "cases.bin", cases)
        us = []
        for _ in range(3):
            out = subprocess.run([str(exe), str(tmp / "cases.bin"), str(tmp / "out.bin"), "--time", "20"],
                                 check=True, capture_output=True, text=True).stdout
            us.append(float(re.search(r"([0-9.]+) us per call", out).group(1)))
        res = lc.read_results(tmp / "out.bin", cases)
    agree = all(list(lkf[f, :nlkf[f]]) == r["local_kf"] and int(ref[f]) == r["ref_kf"] and
                list(lmp[f, :nlmp[f, 0]]) == r["local_mp"] for f, r in enumerate(res))
    assert agree, "the device differs from tests/native/localmap_ref"

    # the parent's round trip around that walk
    h_mpf = torch.empty((B, KP_CAP), dtype=torch.int32).pin_memory()
    h_ol = torch.empty((B, KP_CAP), dtype=torch.uint8).pin_memory()
    h_mps = torch.zeros((B, CAP_MP, 8), dtype=torch.float32).pin_memory()
    h_skip = torch.ones((B, CAP_MP), dtype=torch.uint8).pin_memory()
    rec = S["mp_rec"].view(np.float32).reshape(-1, 8)
    parts = {"d2h": [], "gather": [], "h2d": []}

    def round_trip():
        t0 = time.perf_counter()
        h_mpf.copy_(d_mpf, non_blocking=True)
        h_ol.copy_(d_ol, non_blocking=True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        m = h_mps.numpy()
        for f in range(B):                                   # the records of the walk's result
            n = nlmp[f, 1]
            np.take(rec, lmp[f, :n], axis=0, out=m[f, :n])
        t2 = time.perf_counter()
        d_mps.copy_(h_mps, non_blocking=True)
        d_skip.copy_(h_skip, non_blocking=True)
        d_mpf.copy_(h_mpf, non_blocking=True)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        parts["d2h"].append((t1 - t0) * 1e3)
        parts["gather"].append((t2 - t1) * 1e3)
        parts["h2d"].append((t3 - t2) * 1e3)

    def window_events(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            device()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / steps

    for _ in range(a.warmup):
        device()
        round_trip()
    torch.cuda.synchronize()
    steps = max(3, math.ceil(a.window * 1e3 / max(window_events(5), 1e-3)))
    for v in parts.values():
        v.clear()
    dev_ms = []
    for _ in range(a.repeats):                               # alternate within every repeat
        dev_ms.append(window_events(steps))
        for _ in range(5):
            round_trip()
    med = lambda v: float(np.median(v))
    walk_ms = med(us) * 1e-3 * B
    copies = {n: {"median": med(v), "min": float(min(v)), "max": float(max(v))} for n, v in parts.items()}
    trip = copies["d2h"]["median"] + walk_ms + copies["gather"]["median"] + copies["h2d"]["median"]
    out = {
        "tool": "tools/localmap_step.py", "device": torch.cuda.get_device_name(0),
        "timing": "device events around `steps` calls (device); wall clock per part (round trip); "
                  "tests/native/localmap_ref --time 20 on one core, median of 3 runs (walk)",
        "settings": {"batch": B, "keyframes": a.keyframes, "map_points": S["n_mp"], "features": FEATS,
                     "held": HELD, "cap_kf": CAP_KF, "cap_mp": CAP_MP, "steps": steps,
                     "repeats": a.repeats, "scratch_bytes": view.scratch_bytes(B, CAP_KF, CAP_MP)},
        "per_frame": {"local_keyframes": {"mean": float(nlkf.mean()), "min": int(nlkf.min()),
                                          "max": int(nlkf.max())},
                      "local_points": {"mean": float(nlmp[:, 0].mean()), "min": int(nlmp[:, 0].min()),
                                       "max": int(nlmp[:, 0].max())},
                      "extras": float((nlmp[:, 1] - nlmp[:, 0]).mean())},
        "device_ms_per_call": {"median": med(dev_ms), "min": float(min(dev_ms)),
                               "max": float(max(dev_ms)), "repeats": [float(v) for v in dev_ms]},
        "round_trip_ms_per_call": {"total": trip, "walk_one_core": walk_ms,
                                   "walk_us_per_frame": med(us), "walk_runs_us": us, **copies},
        "equals_localmap_ref": bool(agree),
        "device_beats_round_trip": bool(med(dev_ms) < trip),
        "device_beats_the_copies_alone": bool(med(dev_ms) < trip - walk_ms),
    }
    p = pathlib.Path(a.out)
    os.makedirs(p.parent, exist_ok=True)
    p.write_text(json.dumps(out, indent=1) + "\n")
    print(json.dumps({k: out[k] for k in ("per_frame", "device_ms_per_call", "round_trip_ms_per_call",
                                          "device_beats_round_trip", "device_beats_the_copies_alone")}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
