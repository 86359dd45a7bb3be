"""The directed extractor cases (tests/extract_cases.py) through every regime of k_fast,
k_octree and k_orient_desc that image content can tell apart, library = oracle bit for bit:
keypoints (every field), descriptors, pyramid and blurred levels.

tests/test_extract_cases.py proves on the CPU what each case contains (closed-form FAST
prediction, octree events, moments) and that a flipped decision would change its result;
here each one runs through

* the single-frame path (256 octree threads, wide counts, list order, one cell per wave),
* a batch of 2, of 16 (spatial orientation order, wide counts) and of 17 (packed counts while
  the level's candidates fit kcap, the global scratch beyond), the directed image at the
  first, a middle and the last index among noise images, from a strided, unaligned view,
* for chosen cases: nfeatures = 1500 at 17 images (kcap falls below the candidate count), the
  batches that give 2 and 4 FAST cells per wave, and the 128-thread octree (batch x levels >
  256).

Every regime is asserted from orbx_extractor_regime_info before it is relied on, and the
oracle's keypoint count is asserted against the table (extract_cases.FLOORS) before anything
is compared, so neither a stale regime nor an empty result can pass.
"""
import numpy as np
import pytest

import extract_cases as ec
from helpers import assert_bytes_equal, assert_kps_equal

pytestmark = pytest.mark.gpu

CASE = {c.name: c for c in ec.cases()}
NAMES = list(CASE)
_ORACLE = {}
RUN = []     # (case, regime) pairs compared, for the count test_pairs_run prints


def _oracle(oracle_mod, name, params=None):
    """(extractor, keypoints, descriptors) of a case on the CPU (once per case and params)."""
    c = CASE[name]
    params = params or c.params
    key = (name, params)
    if key not in _ORACLE:
        o = oracle_mod.OracleExtractor(*params)
        k, d = o(c.img)
        if params == c.params:
            assert len(k) == ec.FLOORS[name], (name, len(k))
        _ORACLE[key] = (o, k, d)
    return _ORACLE[key]


def _noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _strided(imgs, gpu):
    """[B, H, W] host images as a device view with rows W + 5 bytes apart from a base 3 bytes
    past an aligned address."""
    import torch
    B, H, W = imgs.shape
    big = torch.zeros((B, H, W + 5), dtype=torch.uint8)
    big[:, :, 3:3 + W] = torch.from_numpy(imgs)
    v = big.to(gpu)[:, :, 3:3 + W]
    assert v.stride(1) == W + 5 and v.storage_offset() == 3
    return v


def _check_levels(g, o, index, what):
    import oracle
    for l in range(o.nlevels):
        lvl = o.level(l)
        assert_bytes_equal(g.pyramid_level(l, index), lvl, f"{what} pyramid L{l}")
        assert_bytes_equal(g.blur_level(l, index), oracle.gaussian7(lvl, 1), f"{what} blur L{l}")


def _single(g, ref, img, what):
    o, k_o, d_o = ref
    k_g, d_g = g(img)
    assert_kps_equal(k_g, k_o, what)
    assert_bytes_equal(d_g, d_o, what + " descriptors")
    _check_levels(g, o, 0, what)


def _batch(g, ref, img, B, where, gpu, what, seed=0):
    """The directed image at the indices `where` of a batch of B, noise elsewhere."""
    import torch
    o, k_o, d_o = ref
    h, w = img.shape
    noise = [_noise(1000 + seed + i, w, h) for i in range(min(B, 3))]
    imgs = np.stack([img if i in where else np.roll(noise[i % len(noise)], 5 * (i // 3), axis=0)
                     for i in range(B)])
    g.extract_batch_device(_strided(imgs, gpu))
    torch.cuda.synchronize()
    for i in where:
        wh = f"{what} image {i} of {B}"
        nkp, kps, desc = g.batch_fetch(i, 1)
        n = nkp[0]
        assert_kps_equal(kps[0, :n], k_o, wh)
        assert_bytes_equal(desc[0, :n] if n > 0 else None, d_o, wh + " descriptors")
        _check_levels(g, o, i, wh)
    others = [i for i in range(B) if i not in where]
    if others and g.params.ini_th_fast <= 100:
        # the neighbours are not empty (their content is not compared)
        assert g.batch_fetch(others[0], 1)[0][0] > 0


def _ncand(ref):
    return [len(ref[0].candidates(l)) for l in range(ref[0].nlevels)]


def _where(B):
    return sorted({0, B // 2, B - 1})


# ---- every case through the four batch regimes -----------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_case_in_every_batch_regime(oracle_mod, orbx_lib, gpu, name):
    import my_orb_slam2_amd as m
    c = CASE[name]
    ref = _oracle(oracle_mod, name)
    h, w = c.img.shape
    g = m.ORBextractor(*c.params)
    _single(g, ref, c.img, f"{name} single")
    r = g.regime_info(1, in_place=True)
    assert (r["octree_threads"], r["packed"], r["spatial"], r["fast_cells_per_wave"]) == \
        (256, 0, 0, 1), r
    RUN.append((name, "single"))
    for B in (2, 16, 17):
        g.prepare(w, h, B)
        r = g.regime_info(B)
        assert r["octree_threads"] == 256 and r["fast_cells_per_wave"] == 1, r
        assert (r["spatial"], r["packed"]) == {2: (0, 0), 16: (1, 0), 17: (1, 1)}[B], r
        assert r["nfeat"] == [int(v) for v in ref[0].tables()["features_per_level"]]
        _batch(g, ref, c.img, B, _where(B), gpu, f"{name} B={B}")
        RUN.append((name, f"B={B}"))
    # and the single-frame path again on the handle that has run batches
    _single(g, ref, c.img, f"{name} single after batches")


# ---- in LDS / global scratch at 17 images ----------------------------------------------------
SCRATCH = ["roots2_field", "margin_0", "margin_1", "big_nodes"]


def test_candidate_storage_at_17(oracle_mod, orbx_lib, gpu):
    """Packed counts need the level's candidates in LDS (ncand <= kcap).  The table's cases
    fall on both sides at their own parameters; the SCRATCH cases, in LDS at theirs, run again
    with nfeatures = 1500 (kcap falls to 64, below their candidate counts)."""
    import my_orb_slam2_amd as m
    side = {}
    for name, c in CASE.items():
        if not c.single_level:
            continue
        g = m.ORBextractor(*c.params)
        g.prepare(c.img.shape[1], c.img.shape[0], 17)
        r = g.regime_info(17)
        n = _ncand(_oracle(oracle_mod, name))[0]
        assert n <= r["cand_cap"][0], (name, n, r)
        side[name] = n <= r["kcap"]
        print(f"{name}: ncand {n} kcap {r['kcap']} ncap {r['ncap']} "
              f"{'LDS, packed' if side[name] else 'global scratch, wide'}")
    for name in ("cut_128_end_eq_n", "cut_129", "cut_256", "cut_257"):
        assert not side[name], name
    for name in SCRATCH + ["pairs", "crowded_cells"]:
        assert side[name], name
    for name in SCRATCH:
        c = CASE[name]
        params = (1500,) + c.params[1:]
        ref = _oracle(oracle_mod, name, params)
        assert len(ref[1]) > 0
        g = m.ORBextractor(*params)
        g.prepare(c.img.shape[1], c.img.shape[0], 17)
        r = g.regime_info(17)
        assert r["packed"] == 1 and r["kcap"] < _ncand(ref)[0], (name, r, _ncand(ref))
        _batch(g, ref, c.img, 17, _where(17), gpu, f"{name} nfeatures=1500 B=17")
        RUN.append((name, "B=17 scratch"))


# ---- FAST cells per wave ---------------------------------------------------------------------
def _batch_for_cells_per_wave(g, nc):
    B = 1
    while g.regime_info(B)["fast_cells_per_wave"] != nc:
        B *= 2
        assert B <= 8192, "no batch gives this many cells per wave"
    return B


@pytest.mark.parametrize("name", ["crowded_cells", "pairs_across_cells", "thresholds_20_7_dark"])
def test_fast_cells_per_wave(oracle_mod, orbx_lib, gpu, name):
    """2 and 4 cells per wave (the next cell's ROI is prefetched while the current one runs):
    the batch that gives each is read from regime_info."""
    import my_orb_slam2_amd as m
    c = CASE[name]
    ref = _oracle(oracle_mod, name)
    h, w = c.img.shape
    g = m.ORBextractor(*c.params)
    g.prepare(w, h, 1)
    for nc in (2, 4):
        B = _batch_for_cells_per_wave(g, nc)
        g.prepare(w, h, B)
        assert g.regime_info(B)["fast_cells_per_wave"] == nc
        print(f"{name}: {nc} cells per wave at {B} images")
        _batch(g, ref, c.img, B, _where(B), gpu, f"{name} nc={nc}")
        RUN.append((name, f"nc={nc}"))


# ---- the 128-thread octree -------------------------------------------------------------------
@pytest.mark.parametrize("name,B,rank", [("pairs_L8", 33, 1), ("crowded_cells_L8", 33, 1),
                                         ("moments_exact_L8", 33, 1), ("textured_L8", 33, 1),
                                         ("cut_128_end_eq_n", 257, 0), ("cut_129", 257, 0),
                                         ("roots2_field", 257, 1), ("big_nodes", 257, 1)])
def test_octree_128_threads(oracle_mod, orbx_lib, gpu, name, B, rank):
    """batch x levels > 256: 33 images at 8 levels, 257 at one.  cut_128_end_eq_n / cut_129
    put phase 2's cut at the end of the first chunk of 128 sorted nodes and one past it (the
    bucket sort: ncap >= 128); the others' node capacity is below 128, the rank sort."""
    import my_orb_slam2_amd as m
    c = CASE[name]
    ref = _oracle(oracle_mod, name)
    h, w = c.img.shape
    g = m.ORBextractor(*c.params)
    g.prepare(w, h, B)
    r = g.regime_info(B)
    assert r["octree_threads"] == 128 and B * c.params[2] > 256, r
    assert (r["ncap"] < 128) == bool(rank), r
    _batch(g, ref, c.img, B, _where(B), gpu, f"{name} B={B}")
    RUN.append((name, "octree 128 threads"))


def test_regime_info_contract(orbx_lib, gpu):
    """regime_info before a geometry is ORBX_ERR_STATE; a batch of 0 is invalid; the chain
    flag follows in_place."""
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd._lib import OrbxError
    g = m.ORBextractor(500, 1.2, 8, 20, 7)
    with pytest.raises(OrbxError) as e:
        g.regime_info(1)
    assert e.value.code == -5
    g.prepare(241, 133, 1)
    with pytest.raises(OrbxError) as e:
        g.regime_info(0)
    assert e.value.code == -1
    # (8 resident images of this size are the largest batch that takes one chain launch:
    # test_gpu_geometry_sweep.py test_resident_batches)
    assert g.regime_info(1, in_place=False)["chain"] == 0
    assert g.regime_info(8, in_place=True)["chain"] == 1
    assert g.regime_info(9, in_place=True)["chain"] == 0
    # the regime table of DESIGN.md ("Directed extractor cases") is this output
    for params, (w, h) in (((500, 1.2, 1, 20, 7), (164, 96)), ((1500, 1.2, 1, 20, 7), (320, 240)),
                           ((1000, 1.2, 8, 20, 7), (320, 240))):
        t = m.ORBextractor(*params)
        t.prepare(w, h, 1)
        for B in (1, 2, 8, 9, 16, 17, 33, 257):
            r = t.regime_info(B, in_place=True)
            print(f"regime {w}x{h} nfeatures={params[0]} nlevels={params[2]} B={B}: "
                  + " ".join(f"{k}={r[k]}" for k in ("octree_threads", "packed", "ncap", "kcap",
                                                     "spatial", "fast_cells_per_wave", "chain")))
            assert r["octree_threads"] == (128 if B * params[2] > 256 else 256)
            assert r["spatial"] == (B >= 16) and r["packed"] == (B > 16)
    r = g.regime_info(1)
    assert len(r["cand_cap"]) == len(r["nfeat"]) == 8
    assert r["nfeat"] == g.features_per_level.tolist()
    assert r["ncap"] % 16 == 0 and r["ncap"] >= max(r["nfeat"]) + 3


def test_pairs_run():
    """The number of (case, regime) pairs the module compared (it runs last)."""
    print(f"{len(RUN)} (case, regime) pairs over {len({n for n, _ in RUN})} cases")
    assert len(RUN) >= 4 * len(NAMES) or len(RUN) == 0   # 0: run alone
