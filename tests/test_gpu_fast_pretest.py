"""k_fast's 4-pixel pre-test, realigned ROI and tail blocks against the oracle, bit for bit
(keypoints, descriptors), on one-level images around 100-170 pixels a side.

What the kernel can get wrong here depends on where a pixel sits and on its value's low bits:
the ROI is shifted by ini_x & 3 at staging, a lane tests 16, 8 or 4 pixels (the cell's last
rows take the narrow forms), rows of more than 32 columns take four lanes, and the pre-test
runs on pixels >> 1 with thresholds (t + 1) >> 1.  So the images are chosen by their cell
grid (extract_cases.cell_grid; the coverage is asserted below) and filled with StampImage
dots and pairs of amplitudes t - 1 .. t + 2 for t = 20 and 7, in both polarities, on
backgrounds of both parities and next to 0 and 255, at every x mod 4, on the first and last
detection column and row of the cells and in their tail rows; and one noise image per grid
whose cells hold more than 64 survivors.  Each image runs as a single frame and in the batches
that give 2 and 4 cells per wave (regime_info) and in one of 17.
"""
import numpy as np
import pytest

import extract_cases as ec
from helpers import assert_bytes_equal, assert_kps_equal

pytestmark = pytest.mark.gpu

PARAMS = (500, 1.2, 1, 20, 7)
AMPS_HI = (19, 20, 21, 22)          # t - 1 .. t + 2 at iniThFAST
AMPS_LO = (6, 7, 8, 9)              # ... at minThFAST
BGS = (0, 5, 100, 101, 250, 255)    # both parities; v - t < 0 at 0 / 5, v + t > 255 at 250 / 255

# (w, h): what its grid must give.  tails: detection rows of a cell beyond its last full block
# of 32 (16 with more than 32 columns).  ROIs of more than 40 rows (hcell > 34) are not
# prefetched.  The last cell row and column lose the 6 ROI border pixels that would cross the
# image border, and more where the grid overshoots (trim_*).  90 x 129 is one column of wide cells.
GEOMS = {
    (153, 129): dict(xo={0, 1, 2, 3}, wide={False}, hcell=33, tails={1, 25}, trim_col=True, trim_row=True),
    (153, 142): dict(xo={0, 1, 2, 3}, wide={False}, hcell=37, tails={5, 30}, trim_col=True, trim_row=True),
    (153, 111): dict(xo={0, 1, 2, 3}, wide={False}, hcell=40, tails={8, 1}, trim_col=True, trim_row=True),
    (164, 96): dict(xo={0, 1, 2, 3}, wide={True, False}, hcell=32, tails={10, 26}, trim_col=False, trim_row=False),
    (164, 112): dict(xo={0, 1, 2, 3}, wide={True, False}, hcell=40, tails={8, 2}, trim_col=False, trim_row=False),
    (90, 129): dict(xo={0}, wide={True}, hcell=33, tails={1, 9}, trim_col=False, trim_row=True),
}


def _cells(w, h):
    """(ini_x, det x0, y0, x1, y1 (inclusive), rows per block) of every cell."""
    out = []
    for (_, _, c0, r0, c1, r1) in ec.cell_grid(w, h)["cells"]:
        dw = c1 - c0 - 6
        out.append((c0, c0 + 3, r0 + 3, c1 - 4, r1 - 4, 16 if dw > 32 else 32))
    return out


def _check_grid(w, h):
    want, grid, cells = GEOMS[(w, h)], ec.cell_grid(w, h), _cells(w, h)
    assert grid["hcell"] == want["hcell"], grid
    assert {c[0] & 3 for c in cells} == want["xo"]
    assert {(c[3] - c[1] + 1) > 32 for c in cells} == want["wide"]
    assert {(c[4] - c[2] + 1) % c[5] for c in cells} - {0} == want["tails"]
    assert (grid["ncols"] * grid["wcell"] > w - 32) == want["trim_col"]
    assert (grid["nrows"] * grid["hcell"] > h - 32) == want["trim_row"]


def test_grids_cover():
    for (w, h) in GEOMS:
        _check_grid(w, h)
    cells = [c for g in GEOMS for c in _cells(*g)]
    assert {c[0] & 3 for c in cells} == {0, 1, 2, 3}
    assert {(c[3] - c[1] + 1) > 32 for c in cells} == {False, True}
    tails = {(c[4] - c[2] + 1) % c[5] for c in cells}
    assert 1 in tails and tails & {5, 6} and 8 in tails
    assert {c[4] - c[2] + 1 + 6 > 40 for c in cells} == {False, True}   # prefetched and not


def _stamps(w, h, bg):
    """Dots and pairs placed greedily (>= 4 apart): the corners of every cell's detection
    region first, then its tail rows, then a lattice.  Cells alternate between the amplitudes
    around iniThFAST and those below it (the latter take the second pass at minThFAST)."""
    s = ec.StampImage(w, h, bg)
    blocked = np.zeros((h, w), bool)
    stat = dict(first_col=0, last_col=0, first_row=0, last_row=0, xmod=set(), tail_amps=set(), pairs=0)
    n = [0]

    def put(cell, ci, x, y, pair=None):
        _, x0, y0, x1, y1, blk = cell
        px = [(x, y)] + ([(x + ec.PAIR_DIRS[pair][0], y + ec.PAIR_DIRS[pair][1])] if pair else [])
        if any(not (x0 <= u <= x1 and y0 <= v <= y1) or blocked[v, u] for u, v in px):
            return
        amps = (AMPS_HI + AMPS_LO) if ci % 2 == 0 else (AMPS_LO + (19, 20))
        a = amps[n[0] % len(amps)]
        n[0] += 1
        if pair:
            s.pair(x, y, a, amps[(n[0] * 3) % len(amps)], pair)
            stat["pairs"] += 1
        else:
            s.dot(x, y, a)
        for u, v in px:
            blocked[max(v - 3, 0):v + 4, max(u - 3, 0):u + 4] = True
            stat["first_col"] += u == x0
            stat["last_col"] += u == x1
            stat["first_row"] += v == y0
            stat["last_row"] += v == y1
            stat["xmod"].add((u - x0) & 3)
            if (v - y0) >= (y1 - y0 + 1) // blk * blk:
                stat["tail_amps"].add(a)

    for ci, cell in enumerate(_cells(w, h)):
        _, x0, y0, x1, y1, blk = cell
        for (x, y) in ((x0, y0), (x1, y1), (x0, y1), (x1, y0)):
            put(cell, ci, x, y)
        for y in range(y0 + (y1 - y0 + 1) // blk * blk, y1 + 1, 4):
            for k, x in enumerate(range(x0 + (y & 3), x1 + 1, 5)):
                put(cell, ci, x, y)
        for j, y in enumerate(range(y0 + 1 + ci % 3, y1 + 1, 4)):
            for k, x in enumerate(range(x0 + (j + ci) % 5, x1 + 1, 5)):
                put(cell, ci, x, y, pair=("h", "v", "d", "a")[(j + k) % 4] if (j + k) % 3 == 0 else None)
    s.check()
    return s, stat


def _check_stamps(w, h, stat):
    assert min(stat["first_col"], stat["last_col"], stat["first_row"], stat["last_row"]) > 0, stat
    assert stat["xmod"] == {0, 1, 2, 3} and stat["pairs"] > 0, stat
    if GEOMS[(w, h)]["tails"]:
        assert stat["tail_amps"] >= set(AMPS_HI + AMPS_LO), stat


def _exact_compass(img, t):
    """The exact compass test of every pixel (borders excluded: False there)."""
    v = img.astype(np.int32)
    out = np.zeros(img.shape, bool)
    c = v[3:-3, 3:-3]
    n0, n8, n4, n12 = v[6:, 3:-3], v[:-6, 3:-3], v[3:-3, 6:], v[3:-3, :-6]
    br = ((n0 > c + t) | (n8 > c + t)) & ((n4 > c + t) | (n12 > c + t))
    dk = ((n0 < c - t) | (n8 < c - t)) & ((n4 < c - t) | (n12 < c - t))
    out[3:-3, 3:-3] = br | dk
    return out


def _noise(w, h, seed=7):
    """Noise whose every cell holds more than 64 survivors of the compass test at iniThFAST."""
    img = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    m = _exact_compass(img, PARAMS[3])
    for (_, x0, y0, x1, y1, _) in _cells(w, h):
        assert m[y0:y1 + 1, x0:x1 + 1].sum() > 64
    return img


_IMAGES = {}


def _images(oracle_mod, w, h):
    """[(name, image, oracle keypoints, oracle descriptors)] of a grid, computed once."""
    if (w, h) not in _IMAGES:
        _check_grid(w, h)
        out = []
        for bg in BGS:
            s, stat = _stamps(w, h, bg)
            _check_stamps(w, h, stat)
            out.append((f"stamps bg={bg}", s.img))
        out.append(("noise", _noise(w, h)))
        res = []
        for name, img in out:
            k, d = oracle_mod.OracleExtractor(*PARAMS)(img)
            assert len(k) > 0, name
            res.append((name, img, k, d))
        # both passes ran: a stamp image has keypoints of response below iniThFAST
        assert any((k["response"] < PARAMS[3]).any() for name, _, k, _ in res if name != "noise")
        _IMAGES[(w, h)] = res
    return _IMAGES[(w, h)]


def _smallest_batch(g, nc):
    """The smallest batch at which k_fast takes nc cells per wave."""
    lo, hi = 1, 1
    while g.regime_info(hi)["fast_cells_per_wave"] < nc:
        lo, hi = hi, hi * 2
        assert hi <= 16384, "no batch gives this many cells per wave"
    while lo < hi:
        mid = (lo + hi) // 2
        if g.regime_info(mid)["fast_cells_per_wave"] < nc:
            lo = mid + 1
        else:
            hi = mid
    return hi


def _run_batch(g, images, w, h, B, gpu, what):
    import torch
    filler = images[-1][1]
    imgs = np.broadcast_to(filler, (B, h, w)).copy()
    where = {}
    for i, im in enumerate(images):   # spread over the batch, first and last index included
        where[(i * (B - 1)) // (len(images) - 1)] = im
    for i, im in where.items():
        imgs[i] = im[1]
    g.extract_batch_device(torch.from_numpy(imgs).to(gpu))
    torch.cuda.synchronize()
    for i, (name, _, k_o, d_o) in where.items():
        nkp, kps, desc = g.batch_fetch(i, 1)
        n = nkp[0]
        assert_kps_equal(kps[0, :n], k_o, f"{what} {name} image {i} of {B}")
        assert_bytes_equal(desc[0, :n] if n > 0 else None, d_o, f"{what} {name} image {i} of {B} descriptors")


@pytest.mark.parametrize("w,h", list(GEOMS))
def test_single_frame(oracle_mod, orbx_lib, gpu, w, h):
    import my_orb_slam2_amd as m
    g = m.ORBextractor(*PARAMS)
    for name, img, k_o, d_o in _images(oracle_mod, w, h):
        k_g, d_g = g(img)
        assert_kps_equal(k_g, k_o, f"{w}x{h} {name}")
        assert_bytes_equal(d_g, d_o, f"{w}x{h} {name} descriptors")
    assert g.regime_info(1, in_place=True)["fast_cells_per_wave"] == 1


@pytest.mark.parametrize("w,h", list(GEOMS))
def test_batches(oracle_mod, orbx_lib, gpu, w, h):
    """2 and 4 cells per wave (the next cell's ROI is prefetched and realigned while the current
    one runs) and a batch of 17."""
    import my_orb_slam2_amd as m
    images = _images(oracle_mod, w, h)
    g = m.ORBextractor(*PARAMS)
    g.prepare(w, h, 1)
    for nc in (1, 2, 4):
        B = 17 if nc == 1 else _smallest_batch(g, nc)
        g.prepare(w, h, B)
        assert g.regime_info(B)["fast_cells_per_wave"] == nc and B >= len(images)
        print(f"{w}x{h}: {nc} cells per wave at {B} images")
        _run_batch(g, images, w, h, B, gpu, f"{w}x{h} nc={nc}")
