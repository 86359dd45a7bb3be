"""Image geometry and batch regimes against the CPU restatement, bit for bit.

Everything the pyramid / FAST / octree / stereo kernels index with is built from the image's
width and height (build_geometry, build_strip_tables, build_chain in orbx_plan.hip) and the
launch policy switches on the batch size (extract_launch).  The other parity tests run a
handful of dataset sizes; here the sizes are picked from the table code:

1. the single-frame path (k_pyr_chain, small-octree budget, lone-frame stereo) over sizes
   around every table boundary, forwards and backwards on the same handles;
2. degenerate shapes (no FAST cell, no octree root, `copy` and `area2` levels, the octree's
   root limit);
3. batches just past each policy switch (8 / 9 / 16 / 17 images) from strided, unaligned views;
4. every strip height (64 / 32 / 16 / 8 rows) at sizes that are no multiple of it;
5. what a handle holds across a geometry change: its last results and the host pyramid view.

Per image: every pyramid level, every blurred level (GaussianBlur 7x7 restated on the oracle's
level), keypoints (every field, bitwise) and descriptors; for pairs uRight / depth (bitwise)
and the valid-match count.  The oracle's own counts are asserted first (floors measured on the
CPU with the seeds below), so an all-empty result cannot pass.
"""
import numpy as np
import pytest

from helpers import assert_bytes_equal, assert_f32_bits_equal, assert_kps_equal
from my_orb_slam2_amd import synth

pytestmark = pytest.mark.gpu

PARAMS = (500, 1.2, 8, 20, 7)
MBF, FX = 386.1448, 718.856
MB = float(np.float32(MBF) / np.float32(FX))


def _pair(oracle_mod, params=PARAMS, simd=1):
    import my_orb_slam2_amd as m
    return (m.ORBextractor(*params, cv_simd=simd), oracle_mod.OracleExtractor(*params, simd=simd))


def _noise(seed, w, h):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


def _check_levels(g, o, index, what):
    """Pyramid and blurred levels of image `index` of g's last call vs the oracle's last frame."""
    import oracle
    simd = int(g.params.cv_simd)
    for l in range(o.nlevels):
        lvl = o.level(l)
        assert_bytes_equal(g.pyramid_level(l, index), lvl, f"{what} pyramid L{l}")
        assert_bytes_equal(g.blur_level(l, index), oracle.gaussian7(lvl, simd), f"{what} blur L{l}")


def _check_frame(g, o, img, what=""):
    """One image through the single-frame path: levels, blurred levels, keypoints, descriptors.
    Returns the oracle's keypoints."""
    k_g, d_g = g(img)
    k_o, d_o = o(img)
    _check_levels(g, o, 0, what)
    assert_kps_equal(k_g, k_o, what)
    assert_bytes_equal(d_g, d_o, what + " descriptors")
    return k_o


def _check_batch(g, o, imgs, indices, what=""):
    """Images `indices` of g's last batched call (inputs `imgs`) vs the oracle, as _check_frame.
    Returns the oracle's keypoint counts of those images."""
    nkp, kps, desc = g.batch_fetch()
    counts = []
    for i in indices:
        k_o, d_o = o(imgs[i])
        w = f"{what} image {i}"
        _check_levels(g, o, i, w)
        assert_kps_equal(kps[i, :nkp[i]], k_o, w)
        assert_bytes_equal(desc[i, :nkp[i]] if nkp[i] > 0 else None, d_o, w + " descriptors")
        counts.append(len(k_o))
    return counts


def _strided(imgs, gpu):
    """[B, H, W] host images as a device view with rows W + 5 bytes apart from a base 3 bytes
    past an aligned address: every row starts at another alignment."""
    import torch
    B, H, W = imgs.shape
    big = torch.zeros((B, H, W + 5), dtype=torch.uint8)
    big[:, :, 3:3 + W] = torch.from_numpy(imgs)
    v = big.to(gpu)[:, :, 3:3 + W]
    assert v.stride(1) == W + 5 and v.storage_offset() == 3
    return v


def _rolled(base, B, step):
    """B distinct images: base image i % k rolled down by step * (i // k) rows (a rolled
    rectified pair stays rectified)."""
    k = len(base)
    return np.stack([np.roll(base[i % k], step * (i // k), axis=0) for i in range(B)])


# ---- 1. single-frame path, size sweep --------------------------------------------------------
# (w, h, oracle keypoint floor, stereo match floor); stereo_pair(7, w, h).  Measured on the CPU
# (left keypoints / matches): 22/9, 20/9, 23/10, 21/7; 207/48, 228/50, 224/99, 92/27; 469/145,
# 337/132, 216/77, 504/140, 274/117, 275/136.
SWEEP = [
    # one half-strip against two (odd / even snh); level-0 pitch 128 -> 192 at w = 125
    (119, 101, 20, 7), (120, 100, 20, 7), (121, 99, 20, 7), (125, 98, 20, 7),
    # snh 2 -> 3; w mod 16 and h mod 4 in all residues over the levels
    (239, 131, 90, 25), (240, 132, 90, 25), (241, 133, 90, 25),
    # w a multiple of 64 and 16, h of 32
    (256, 96, 90, 25),
    # odd everything; levels of width 121 and 120 deep in the pyramid
    (301, 203, 200, 70), (361, 150, 200, 70), (359, 118, 200, 70),
    # 7 chain tiles across, n_ini 2
    (481, 242, 200, 70),
    # wide (n_ini 8 and 18), 10 half-strips, stereo with very few rows
    (600, 100, 200, 70), (1200, 100, 200, 70),
]
SWEEP_SCALAR = [s for s in SWEEP if s[:2] in ((241, 133), (361, 150), (600, 100))]


@pytest.mark.parametrize("simd", [1, 0])
def test_single_frame_size_sweep(oracle_mod, orbx_lib, gpu, simd):
    """One extractor pair over the whole size list, forwards then backwards: every size is
    reached from a smaller and from a larger geometry (tables rebuilt, cap_batch reset, the
    single-frame graph re-captured).  cv_simd = 0 runs three of the sizes."""
    import my_orb_slam2_amd as m
    gl, ol = _pair(oracle_mod, simd=simd)
    gr, orr = _pair(oracle_mod, simd=simd)
    sizes = SWEEP if simd else SWEEP_SCALAR
    for w, h, kp_floor, match_floor in sizes + sizes[::-1]:
        what = f"{w}x{h} simd={simd}"
        L, R = synth.stereo_pair(7, w, h)
        kl = _check_frame(gl, ol, L, what + " left")
        _check_frame(gr, orr, R, what + " right")
        u_o, d_o, n_o = oracle_mod.stereo_match(ol, orr, len(kl), MBF, MB)
        assert len(kl) >= kp_floor and n_o >= match_floor, (what, len(kl), n_o)
        u_g, d_g, n_g = m.compute_stereo_matches(gl, gr, MBF, MB)
        assert_f32_bits_equal(u_g, u_o, what + " uRight")
        assert_f32_bits_equal(d_g, d_o, what + " depth")
        assert n_g == n_o, what
        if (w, h) == (361, 150) and simd:
            # portrait with n_ini 1 between two landscape sizes (211 oracle keypoints)
            k = _check_frame(gl, ol, synth.frame(3, 150, 200), "150x200")
            assert len(k) >= 200, len(k)


# ---- 2. degenerate shapes --------------------------------------------------------------------
# (params, (w, h), image kind, oracle keypoint range); the oracle runs all of them, and the
# pyramid and blurred levels are compared at every one.  No level is below 6 pixels.
DEGENERATE = [
    # no FAST cell on any level (or levels too short for one): 0 keypoints
    (PARAMS, (53, 38), "synth", (0, 0)), (PARAMS, (52, 52), "noise", (0, 0)),
    (PARAMS, (36, 36), "synth", (0, 0)), (PARAMS, (1000, 60), "synth", (0, 0)),
    ((500, 1.2, 4, 20, 7), (640, 37), "noise", (0, 0)),
    # a portrait narrower than half its height: n_ini = round(w / h) = 0 octree roots, so
    # DistributeOctTree keeps nothing although FAST finds corners, as in the reference
    (PARAMS, (150, 300), "synth", (0, 0)),
    # lower levels without cells (53 oracle keypoints)
    (PARAMS, (200, 90), "synth", (50, 500)),
    # copy levels: 12 x 12 at 1.1 has levels 5 and 6 both 7 x 7; 20 x 16 with 12 levels ends in
    # 9 x 7, 8 x 7, 8 x 6, 7 x 6: neighbours that share one dimension only (no copy level)
    ((500, 1.1, 8, 20, 7), (12, 12), "noise", (0, 0)),
    ((500, 1.1, 12, 20, 7), (20, 16), "noise", (0, 0)),
    # exact 2:1 (area) levels and their neighbours: 201 x 151 area then 100 x 76 linear;
    # 200 x 150 linear then 100 x 75 area; both area (493 / 487 / 487 oracle keypoints)
    ((500, 2.0, 3, 20, 7), (402, 302), "synth", (450, 510)),
    ((500, 2.0, 3, 20, 7), (401, 301), "synth", (450, 510)),
    ((500, 2.0, 3, 20, 7), (400, 300), "synth", (450, 510)),
]


@pytest.mark.parametrize("params,size,kind,kp_range", DEGENERATE,
                         ids=[f"{s[0]}x{s[1]}-{p[1]}-{p[2]}" for p, s, _, _ in DEGENERATE])
def test_degenerate_shapes(oracle_mod, orbx_lib, gpu, params, size, kind, kp_range):
    g, o = _pair(oracle_mod, params)
    w, h = size
    o(np.zeros((h, w), np.uint8))
    # smaller levels would reflect more than once in the blur's halo
    assert all(min(o.level_size(l)) >= 6 for l in range(params[2]))
    img = synth.frame(7, w, h) if kind == "synth" else _noise(7, w, h)
    k = _check_frame(g, o, img, f"{w}x{h} {params}")
    assert kp_range[0] <= len(k) <= kp_range[1], len(k)
    # and once more on the handle that now holds this geometry (graph replay, no rebuild),
    # with the other kind of image
    img2 = _noise(8, w, h) if kind == "synth" else synth.frame(8, w, h)
    _check_frame(g, o, img2, f"{w}x{h} {params} second image")


def test_octree_root_limit(oracle_mod, orbx_lib, gpu):
    """A level of w x h pixels has round((w - 32) / (h - 32)) octree roots (ORBextractor.cc:543);
    k_octree keeps 4 nodes per root in LDS, which fits up to 512 roots (include/orbx.h).  A strip
    one usable row tall reaches that: 544 x 33 (512 roots) runs and equals the oracle, 545 x 33
    (513) is refused with ORBX_ERR_UNSUPPORTED, as is 891 x 40 (level 1 is 742 x 33), and the
    refusal leaves the handle usable and without a stale host pyramid."""
    from my_orb_slam2_amd._lib import OrbxError
    g, o = _pair(oracle_mod)
    g.host_pyramid(True)
    k = _check_frame(g, o, synth.frame(7, 544, 33), "544x33")
    assert len(k) == 0 and len(g.host_pyramid_view()) == 8
    for w, h in ((545, 33), (891, 40)):
        with pytest.raises(OrbxError) as e:
            g(synth.frame(7, w, h))
        assert e.value.code == -4, (w, h)   # ORBX_ERR_UNSUPPORTED
        with pytest.raises(OrbxError) as e:
            g.host_pyramid_view()
        assert e.value.code == -5
        k = _check_frame(g, o, synth.frame(7, 241, 133), f"241x133 after {w}x{h}")
        assert len(k) >= 90


def test_copy_levels_exist(oracle_mod):
    """The copy-level cases of test_degenerate_shapes have the levels they are there for."""
    o = oracle_mod.OracleExtractor(500, 1.1, 8, 20, 7)
    o(_noise(7, 12, 12))
    assert o.level_size(5) == o.level_size(6) == (7, 7)
    o = oracle_mod.OracleExtractor(500, 1.1, 12, 20, 7)
    o(_noise(7, 20, 16))
    assert [o.level_size(l) for l in range(8, 12)] == [(9, 7), (8, 7), (8, 6), (7, 6)]


# ---- 3. batches just past each policy switch -------------------------------------------------
@pytest.mark.parametrize("size", [(241, 133), (361, 150), (600, 100)])
def test_batches_at_policy_switches(oracle_mod, orbx_lib, gpu, size):
    """8 / 9 images: either side of the k_pyr_chain limit (images copied from the caller's
    tensor take per-level strips on both sides; test_resident_batches runs the chain); 16: the
    last small-octree batch and the first with the side branch; 17: the large octree.  One
    handle grows through all four, from strided views."""
    import torch
    w, h = size
    g, o = _pair(oracle_mod)
    base = [synth.frame(50 + i, w, h) for i in range(4)]
    for B in (8, 9, 16, 17):
        imgs = _rolled(base, B, 7)
        g.extract_batch_device(_strided(imgs, gpu))
        torch.cuda.synchronize()
        counts = _check_batch(g, o, imgs, range(B), f"{w}x{h} B={B}")
        assert min(counts) >= 90, counts   # 165 .. 385 on the CPU


def test_stereo_batch_past_chain_switch(oracle_mod, orbx_lib, gpu):
    """9 pairs (18 images) of 361 x 150 through StereoBatch from strided views."""
    import torch
    import my_orb_slam2_amd as m
    B, (w, h) = 9, (361, 150)
    base = [synth.stereo_pair(60 + i, w, h) for i in range(3)]
    Lh = _rolled([p[0] for p in base], B, 11)
    Rh = _rolled([p[1] for p in base], B, 11)
    sb = m.StereoBatch(B, *PARAMS)
    uR, dep, nv = sb(_strided(Lh, gpu), _strided(Rh, gpu), MBF, MB)
    torch.cuda.synchronize()
    nkp, kps, desc = sb.fetch("left")
    nkpr, kpsr, descr = sb.fetch("right")
    uRh, deph, nvh = uR.cpu().numpy(), dep.cpu().numpy(), nv.cpu().numpy()
    ol, orr = oracle_mod.OracleExtractor(*PARAMS), oracle_mod.OracleExtractor(*PARAMS)
    for i in range(B):
        k_o, d_o = ol(Lh[i])
        kr_o, dr_o = orr(Rh[i])
        _check_levels(sb.ext, ol, i, f"pair {i} left")
        _check_levels(sb.ext, orr, B + i, f"pair {i} right")
        assert_kps_equal(kps[i, :nkp[i]], k_o, f"pair {i} left")
        assert_bytes_equal(desc[i, :nkp[i]], d_o, f"pair {i} left desc")
        assert_kps_equal(kpsr[i, :nkpr[i]], kr_o, f"pair {i} right")
        assert_bytes_equal(descr[i, :nkpr[i]], dr_o, f"pair {i} right desc")
        u_o, z_o, n_o = oracle_mod.stereo_match(ol, orr, len(k_o), MBF, MB)
        assert len(k_o) >= 200 and n_o >= 70, (i, len(k_o), n_o)
        assert_f32_bits_equal(uRh[i, :nkp[i]], u_o, f"pair {i} uRight")
        assert_f32_bits_equal(deph[i, :nkp[i]], z_o, f"pair {i} depth")
        assert nvh[i] == n_o, f"pair {i}"


@pytest.mark.parametrize("B", [8, 17])
def test_resident_batches(oracle_mod, orbx_lib, gpu, B):
    """Images of 241 x 133 written into the level-0 slots (input_views) and extracted in
    place: 8 images are the largest batch that takes one k_pyr_chain launch (only images in
    place do), 17 take k_level_strip's blur-only level 0, the side branch and the large octree."""
    import torch
    w, h = 241, 133
    g, o = _pair(oracle_mod)
    imgs = _rolled([synth.frame(70 + i, w, h) for i in range(4)], B, 9)
    v = g.input_views(w, h, B)
    assert tuple(v.shape) == (B, h, w)
    v.copy_(torch.from_numpy(imgs).to(gpu))
    g.extract_batch_resident(B)
    torch.cuda.synchronize()
    counts = _check_batch(g, o, imgs, range(B), "resident 241x133")
    assert min(counts) >= 90, counts   # 129 .. 290 on the CPU
    assert torch.equal(v.cpu(), torch.from_numpy(imgs))   # the inputs stay as written


# ---- 4. every strip height at odd geometry ---------------------------------------------------
STRIP_CASES = [((600, 100), 384), ((301, 203), 256)]


def _strip_rows(size, B):
    import my_orb_slam2_amd as m
    g = m.ORBextractor(*PARAMS)
    g.prepare(size[0], size[1], B)
    return g, g.launch_info(B)[0]


def test_strip_heights_all_present(oracle_mod, orbx_lib, gpu):
    """The two large-batch cases below walk strips of every height between them, each height
    on at least one level whose height is no multiple of it (with 256 CUs: 600 x 100 at 384
    images 64, 64, 32, 16, 16, 16, 8, 8 and 301 x 203 at 256 images 64, 32, 16, 16, 8, 8, 8, 8).
    On a device with another CU count the heuristic may choose otherwise: then raise B."""
    o = oracle_mod.OracleExtractor(*PARAMS)
    seen, ragged = set(), set()
    for size, B in STRIP_CASES:
        _, rows = _strip_rows(size, B)
        o(np.zeros((size[1], size[0]), np.uint8))
        print(f"{size[0]}x{size[1]} B={B} strip rows {rows.tolist()}")
        for l, r in enumerate(rows.tolist()):
            seen.add(r)
            if r and o.level_size(l)[1] % r:
                ragged.add(r)
    assert seen == {8, 16, 32, 64}, seen
    assert ragged == {8, 16, 32, 64}, ragged


def test_strip_heights_600x100_b384(oracle_mod, orbx_lib, gpu):
    """384 distinct images, every one against the oracle."""
    import torch
    (w, h), B = STRIP_CASES[0]
    g, rows = _strip_rows((w, h), B)
    o = oracle_mod.OracleExtractor(*PARAMS)
    imgs = _rolled([synth.frame(80 + i, w, h) for i in range(8)], B, 2)
    g.extract_batch_device(torch.from_numpy(imgs).to(gpu))
    torch.cuda.synchronize()
    assert np.array_equal(g.launch_info(B)[0], rows)
    counts = _check_batch(g, o, imgs, range(B), f"600x100 B={B}")
    assert min(counts) >= 150, min(counts)   # 173 .. 275 on the CPU


def test_strip_heights_301x203_b256(oracle_mod, orbx_lib, gpu):
    """256 images, image i = base image i mod 7: the first, the last and every fourth (all
    seven base images among them) against the oracle, the others against the same base image
    run singly (8-row strips on every level, k_pyr_chain)."""
    import torch
    ((w, h), B), K = STRIP_CASES[1], 7
    g, rows = _strip_rows((w, h), B)
    o = oracle_mod.OracleExtractor(*PARAMS)
    base = [synth.frame(90 + i, w, h) for i in range(K)]
    imgs = np.stack([base[i % K] for i in range(B)])
    g.extract_batch_device(torch.from_numpy(imgs).to(gpu))
    torch.cuda.synchronize()
    assert np.array_equal(g.launch_info(B)[0], rows)
    picked = sorted(set(range(0, B, 4)) | {B - 1})
    assert len(picked) >= 64 and {i % K for i in picked} == set(range(K))
    counts = _check_batch(g, o, imgs, picked, f"301x203 B={B}")
    assert min(counts) >= 200, min(counts)   # 436 .. 471 on the CPU
    import my_orb_slam2_amd as m
    one = m.ORBextractor(*PARAMS)
    single = []
    for img in base:
        k1, d1 = one(img)
        single.append((k1, d1, [one.pyramid_level(l) for l in range(8)],
                       [one.blur_level(l) for l in range(8)]))
    nkp, kps, desc = g.batch_fetch()
    for i in sorted(set(range(B)) - set(picked)):
        k1, d1, pyr, blr = single[i % K]
        assert_kps_equal(kps[i, :nkp[i]], k1, f"image {i} vs single")
        assert_bytes_equal(desc[i, :nkp[i]], d1, f"image {i} desc vs single")
        for l in range(8):
            assert_bytes_equal(g.pyramid_level(l, i), pyr[l], f"image {i} pyramid L{l} vs single")
            assert_bytes_equal(g.blur_level(l, i), blr[l], f"image {i} blur L{l} vs single")


# ---- 5. what a handle holds across a geometry change -----------------------------------------
@pytest.mark.parametrize("change", ["size", "growth", "unsupported"])
def test_last_results_dropped_by_workspace_change(oracle_mod, orbx_lib, gpu, change):
    """A call that rebuilds the geometry for another size (supported or refused) or regrows the
    workspace leaves no pyramids and no outputs behind: the buffers were reallocated and the
    tables describe another size, so every query of the last extraction, and a stereo match
    over it, return ORBX_ERR_STATE instead of reading them.  The next extraction restores all
    of it; the other handle of the pair is untouched."""
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd._lib import OrbxError
    gl, ol = _pair(oracle_mod)
    gr, orr = _pair(oracle_mod)
    L, R = synth.stereo_pair(7, 241, 133)
    _check_frame(gl, ol, L, "left")
    _check_frame(gr, orr, R, "right")
    if change == "size":
        gl.prepare(481, 242, 1)
    elif change == "growth":
        gl.prepare(241, 133, 3)
    else:
        with pytest.raises(OrbxError) as e:
            gl.prepare(545, 33, 1)
        assert e.value.code == -4
    for name, call in (("pyramid_level", lambda: gl.pyramid_level(0)),
                       ("blur_level", lambda: gl.blur_level(0)),
                       ("batch_view", gl.batch_view), ("batch_fetch", gl.batch_fetch),
                       ("stereo", lambda: m.compute_stereo_matches(gl, gr, MBF, MB))):
        with pytest.raises(OrbxError) as e:
            call()
        assert e.value.code == -5, name   # ORBX_ERR_STATE
    kl = _check_frame(gl, ol, L, "left again")
    u_o, d_o, n_o = oracle_mod.stereo_match(ol, orr, len(kl), MBF, MB)
    u_g, d_g, n_g = m.compute_stereo_matches(gl, gr, MBF, MB)
    assert_f32_bits_equal(u_g, u_o, "uRight")
    assert_f32_bits_equal(d_g, d_o, "depth")
    assert n_g == n_o and n_o >= 25


@pytest.mark.parametrize("change", ["batch", "prepare"])
def test_host_pyramid_view_after_geometry_change(oracle_mod, orbx_lib, gpu, change):
    """orbx_host_pyramid_view describes the handle's pinned pyramid copy with the handle's
    current geometry, so after a call that rebuilds the geometry for another size (a batched
    extraction, orbx_extractor_prepare) it must return ORBX_ERR_STATE until the next
    orbx_extract refills the copy; the stale block (here the smaller one) is never read."""
    import torch
    from my_orb_slam2_amd._lib import OrbxError
    g, o = _pair(oracle_mod)
    g.host_pyramid(True)
    with pytest.raises(OrbxError) as e:   # nothing extracted yet
        g.host_pyramid_view()
    assert e.value.code == -5

    def extract_and_compare(img, what):
        _check_frame(g, o, img, what)
        levels = g.host_pyramid_view()
        assert len(levels) == o.nlevels
        for l, lvl in enumerate(levels):
            assert_bytes_equal(lvl, o.level(l), f"{what} host pyramid L{l}")

    small, big = synth.frame(7, 241, 133), synth.frame(7, 481, 242)
    extract_and_compare(small, "241x133")
    if change == "batch":
        g.extract_batch_device(torch.from_numpy(big[None]).to(gpu))
        torch.cuda.synchronize()
    else:
        g.prepare(481, 242, 1)
    with pytest.raises(OrbxError) as e:
        g.host_pyramid_view()
    assert e.value.code == -5   # ORBX_ERR_STATE
    extract_and_compare(big, "481x242")
    # a batched call at the same size leaves the copy (and the view) valid
    g.extract_batch_device(torch.from_numpy(big[None]).to(gpu))
    torch.cuda.synchronize()
    for l, lvl in enumerate(g.host_pyramid_view()):
        assert_bytes_equal(lvl, o.level(l), f"481x242 host pyramid L{l} after a same-size batch")
    g.host_pyramid(False)
    with pytest.raises(OrbxError):
        g.host_pyramid_view()
