"""k_stereo against the oracle in every launch regime, on directed cases.

stereo_split() / stereo_lpk() (orbx_stereo.hip) choose the template instance and the number of
workgroups per pair from the number of pairs: k_stereo<8> x 16 (1 - 16 pairs), k_stereo<8> x 8
(17 - 32), k_stereo<1> x 4 (33 - 64), k_stereo<1> x 2 (65 - 128), k_stereo<1> x 1 (129 and up).
The tests here run every one of them against oracle_stereo_match, bit for bit:

3. the matcher alone over injected features (tests/stereo_cases.py: Hamming distances 74 / 75 /
   99 / 100, ties, uR at and one step beyond minU / maxU, the band's first and last row, octaves
   +-1 / +-2, the disparity <= 0 clamp, empty views, a full kp_cap), the pair counts ordered so
   that the split scratch grows and shrinks and a counter one regime left non-zero would
   corrupt the next;
4. orbx_stereo_match after a one-image batched extraction (the left count read back from the
   device), and its capacity error;
5. StereoBatch end to end, extraction included, in the three regimes no other test reaches.

tests/test_oracle_stereo.py checks the oracle's matcher against an independent reading and
asserts how often every exit and every construct occurs in exactly the cases of test 3.
"""
import ctypes
import dataclasses

import numpy as np
import pytest

import stereo_cases as sc
from helpers import assert_bytes_equal, assert_f32_bits_equal, assert_kps_equal
from my_orb_slam2_amd import synth

pytestmark = pytest.mark.gpu

W, H = sc.SIZE
FILL = -7


@pytest.fixture(scope="module")
def bases(oracle_mod):
    return sc.base_pairs(oracle_mod)


def _expected(oracle_mod, bases, c):
    """The oracle's (uRight, depth, nvalid) of one case."""
    b = bases[c.base]
    b["ol"].set_features(c.kL, c.dL)
    b["orr"].set_features(c.kR, c.dR)
    return oracle_mod.stereo_match(b["ol"], b["orr"], len(c.kL), sc.MBF, sc.MB)


def _inject(g, views, gpu):
    """Overwrite the keypoints, descriptors and counts of g's last batched extraction with
    `views` = [(keypoints, descriptors)] (one per image); the pyramids stay."""
    import torch
    kps_t, desc_t, nkp_t = g.batch_tensors()
    B, KC = kps_t.shape[0], kps_t.shape[1]
    assert B == len(views) and KC == sc.KP_CAP and kps_t.shape[2] == sc.KEYPOINT_DTYPE.itemsize
    hk = np.zeros((B, KC), sc.KEYPOINT_DTYPE)
    hd = np.zeros((B, KC, 32), np.uint8)
    hn = np.zeros(B, np.int32)
    for p, (k, d) in enumerate(views):
        hk[p, :len(k)], hd[p, :len(k)], hn[p] = k, d, len(k)
    kps_t.copy_(torch.from_numpy(hk.view(np.uint8).reshape(B, KC, 28)).to(gpu))
    desc_t.copy_(torch.from_numpy(hd).to(gpu))
    nkp_t.copy_(torch.from_numpy(hn).to(gpu))


# ---- 3. every regime against the oracle ------------------------------------------------------
def test_every_regime_against_oracle(oracle_mod, orbx_lib, gpu, bases):
    """One pair of handles (left views, right views) through 16, 129, 33, 1, 128, 17, 65, 32, 64
    pairs, twice: extraction of the tiled base images, injection of pair p's case (base pair
    p % 4, seed pair_seed(B, p); the last five pairs of a batch are the special ones),
    orbx_stereo_match_batch_device into -7-filled outputs.  Per pair uRight[:n] and depth[:n]
    equal the oracle's bit for bit, nvalid equals, and the slots from n on still hold the fill.
    (Time: the 485 cases take about 4 s to generate, the oracle 0.4 s; the GPU part is small.)"""
    import torch
    import my_orb_slam2_amd as m
    gl, gr = m.ORBextractor(*sc.PARAMS, max_batch=129), m.ORBextractor(*sc.PARAMS, max_batch=129)
    assert gl.prepare(W, H, 129) == sc.KP_CAP and gr.prepare(W, H, 129) == sc.KP_CAP
    imgL = torch.from_numpy(np.stack([bases[p % 4]["imgL"] for p in range(129)])).to(gpu)
    imgR = torch.from_numpy(np.stack([bases[p % 4]["imgR"] for p in range(129)])).to(gpu)
    cases, expected, first = {}, {}, {}
    for rnd in range(2):
        for B in sc.REGIMES:
            what = f"round {rnd} B={B}"
            assert gl.launch_info(2 * B)[1] == sc.SPLIT[B], what
            if B not in cases:
                cases[B] = sc.batch_cases(bases, B)
                expected[B] = [_expected(oracle_mod, bases, c) for c in cases[B]]
            gl.extract_batch_device(imgL[:B])
            gr.extract_batch_device(imgR[:B])
            torch.cuda.synchronize()
            _inject(gl, [(c.kL, c.dL) for c in cases[B]], gpu)
            _inject(gr, [(c.kR, c.dR) for c in cases[B]], gpu)
            torch.cuda.synchronize()
            uR = torch.full((B, sc.KP_CAP), FILL, dtype=torch.float32, device=gpu)
            dep = torch.full((B, sc.KP_CAP), FILL, dtype=torch.float32, device=gpu)
            nv = torch.full((B,), FILL, dtype=torch.int32, device=gpu)
            m.compute_stereo_matches_batch_device(gl, gr, sc.MBF, sc.MB, uR, dep, nv)
            torch.cuda.synchronize()
            uRh, deph, nvh = uR.cpu().numpy(), dep.cpu().numpy(), nv.cpu().numpy()
            for p, (c, (u_o, d_o, n_o)) in enumerate(zip(cases[B], expected[B])):
                n = len(c.kL)
                w = f"{what} pair {p} ({c.kind}, base {c.base})"
                assert_f32_bits_equal(uRh[p, :n], u_o, w + " uRight")
                assert_f32_bits_equal(deph[p, :n], d_o, w + " depth")
                assert nvh[p] == n_o, (w, nvh[p], n_o)
                assert (uRh[p, n:] == FILL).all() and (deph[p, n:] == FILL).all(), w + " past n"
            if rnd == 0:
                first[B] = (uRh, deph, nvh)
            else:
                for a, b in zip(first[B], (uRh, deph, nvh)):
                    assert a.tobytes() == b.tobytes(), what + " differs from round 0"


# ---- 4. orbx_stereo_match after a one-image batched extraction -------------------------------
def test_stereo_match_after_one_image_batch(oracle_mod, orbx_lib, gpu, bases):
    """A one-image extract_batch_device leaves the left keypoint count on the device only, so
    orbx_stereo_match reads it back with its results: the injected count, not the extracted
    one.  With room for fewer values than that it returns ORBX_ERR_CAPACITY and the first
    n_left values."""
    import torch
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd._lib import ptr
    gl, gr = m.ORBextractor(*sc.PARAMS), m.ORBextractor(*sc.PARAMS)
    for base, seed in ((1, 11), (0, 12)):
        b = bases[base]
        c = sc.generate(b, seed)
        # seven left keypoints fewer than were extracted: the count is the injected one
        c = dataclasses.replace(c, kL=c.kL[:-7], dL=c.dL[:-7])
        u_o, d_o, n_o = _expected(oracle_mod, bases, c)
        n = len(c.kL)
        assert n_o >= 50 and n == len(b["kL"]) - 7
        gl.extract_batch_device(torch.from_numpy(b["imgL"][None]).to(gpu))
        gr.extract_batch_device(torch.from_numpy(b["imgR"][None]).to(gpu))
        torch.cuda.synchronize()
        _inject(gl, [(c.kL, c.dL)], gpu)
        _inject(gr, [(c.kR, c.dR)], gpu)
        torch.cuda.synchronize()
        for room in (n, n + 9, n - 1, n // 2, 1):
            u = np.full(room + 4, FILL, np.float32)
            d = np.full(room + 4, FILL, np.float32)
            nv = ctypes.c_int(FILL)
            code = orbx_lib.orbx_stereo_match(gl._h, gr._h, sc.MBF, sc.MB, ptr(u), ptr(d), room,
                                              ctypes.byref(nv))
            what = f"base {base} room {room} of {n}"
            assert code == (0 if room >= n else -3), what     # ORBX_OK / ORBX_ERR_CAPACITY
            k = min(room, n)
            assert_f32_bits_equal(u[:k], u_o[:k], what + " uRight")
            assert_f32_bits_equal(d[:k], d_o[:k], what + " depth")
            assert (u[k:] == FILL).all() and (d[k:] == FILL).all(), what + " past the count"
            assert nv.value == n_o, what


# ---- 5. the one-handle path in the regimes between 16 and 129 pairs ----------------------------
def _rolled(base, B, step):
    """B distinct images: base image i % k rolled down by step * (i // k) rows (a rolled
    rectified pair stays rectified)."""
    k = len(base)
    return np.stack([np.roll(base[i % k], step * (i // k), axis=0) for i in range(B)])


DATASET_MBF = 386.1448
DATASET_MB = float(np.float32(DATASET_MBF) / np.float32(718.856))


@pytest.mark.parametrize("B,split", [(24, 8), (40, 4), (96, 2)])
def test_stereo_batch_between_regimes(oracle_mod, orbx_lib, gpu, B, split):
    """StereoBatch, extraction and match in one call, at 24 pairs (k_stereo<8> x 8 workgroups),
    40 (k_stereo<1> x 4) and 96 (k_stereo<1> x 2): keypoints and descriptors of both views,
    uRight, depth and the valid count of every pair against the oracle.  No injection."""
    import torch
    import my_orb_slam2_amd as m
    base = [synth.stereo_pair(60 + i, W, H) for i in range(3)]
    Lh = _rolled([p[0] for p in base], B, 3)
    Rh = _rolled([p[1] for p in base], B, 3)
    sb = m.StereoBatch(B, *sc.PARAMS)
    uR, dep, nv = sb(torch.from_numpy(Lh).to(gpu), torch.from_numpy(Rh).to(gpu), DATASET_MBF, DATASET_MB)
    torch.cuda.synchronize()
    assert sb.ext.launch_info(2 * B)[1] == split
    nkp, kps, desc = sb.fetch("left")
    nkpr, kpsr, descr = sb.fetch("right")
    uRh, deph, nvh = uR.cpu().numpy(), dep.cpu().numpy(), nv.cpu().numpy()
    ol, orr = oracle_mod.OracleExtractor(*sc.PARAMS), oracle_mod.OracleExtractor(*sc.PARAMS)
    for i in range(B):
        k_o, d_o = ol(Lh[i])
        kr_o, dr_o = orr(Rh[i])
        u_o, z_o, n_o = oracle_mod.stereo_match(ol, orr, len(k_o), DATASET_MBF, DATASET_MB)
        assert len(k_o) >= 200 and len(kr_o) >= 200 and n_o >= 70, (i, len(k_o), len(kr_o), n_o)
        assert_kps_equal(kps[i, :nkp[i]], k_o, f"pair {i} left")
        assert_bytes_equal(desc[i, :nkp[i]], d_o, f"pair {i} left desc")
        assert_kps_equal(kpsr[i, :nkpr[i]], kr_o, f"pair {i} right")
        assert_bytes_equal(descr[i, :nkpr[i]], dr_o, f"pair {i} right desc")
        assert_f32_bits_equal(uRh[i, :nkp[i]], u_o, f"pair {i} uRight")
        assert_f32_bits_equal(deph[i, :nkp[i]], z_o, f"pair {i} depth")
        assert nvh[i] == n_o, f"pair {i}"
