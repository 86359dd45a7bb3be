"""The pyramid levels that do not run the strip walk (k_level_plain + k_blur_plain), bit for bit.

build_strip_tables (orbx_plan.hip) leaves a level to the plain kernels when it is a copy of the
level above (equal sizes), an exact 2:1 area level, or an INTER_LINEAR level whose 4-pixel
groups span more than the strip walk's 8-byte window (scale factors from about 2.3).  No
benchmarked configuration has such a level, so the cases here are chosen to have them, and each
first asserts from launch_info() that exactly the expected levels report no strip rows: a case
that stops exercising the fallback fails instead of passing on the strip walk.

Per case and cv_simd setting, on four paths (one host image, device batches of 2 and of 9, a
resident batch extracted in place): every pyramid level against the oracle's level, every
blurred level against the oracle's GaussianBlur 7x7 of that level, bytewise.
"""
import numpy as np
import pytest

from helpers import assert_bytes_equal

pytestmark = pytest.mark.gpu

# (width, height, scale factor, levels, the levels that take the plain kernels)
CASES = [
    (64, 48, 2.0, 3, {1, 2}),     # area2, area2
    (66, 50, 2.0, 4, {1, 3}),     # 33x25 area2 (odd width, partial last group), 16x12 strip, 8x6 area2
    (70, 50, 2.5, 3, {1, 2}),     # wide-tap INTER_LINEAR, widths 28 and 11
    (96, 64, 3.0, 3, {1, 2}),     # wide-tap INTER_LINEAR, widths 32 and 11
    (64, 48, 1.0, 3, {1, 2}),     # copy, copy
    (12, 12, 1.1, 8, {6}),        # a 7x7 copy: the blur reflects further than half the level
    (3, 3, 1.2, 3, {2}),          # a 2x2 copy
]
NIMG = 9   # distinct noise images per case: the batch of 9 takes all, the others the first ones

_reference = {}


def _ref(oracle_mod, case, simd):
    """[(image, [level], [blurred level])] for the case's NIMG images, computed once."""
    key = (case[:4], simd)
    if key not in _reference:
        w, h, scale, nlevels, _ = case
        o = oracle_mod.OracleExtractor(500, scale, nlevels, 20, 7, simd=simd)
        out = []
        for i in range(NIMG):
            img = np.random.default_rng(1000 * w + 10 * i + simd).integers(0, 256, (h, w), dtype=np.uint8)
            o(img)
            levels = [o.level(l) for l in range(nlevels)]
            out.append((img, levels, [oracle_mod.gaussian7(lv, simd) for lv in levels]))
        _reference[key] = out
    return _reference[key]


def _check(g, ref, count, what):
    for i in range(count):
        _, levels, blurs = ref[i]
        for l, (lv, bl) in enumerate(zip(levels, blurs)):
            assert_bytes_equal(g.pyramid_level(l, i), lv, f"{what} image {i} pyramid L{l}")
            assert_bytes_equal(g.blur_level(l, i), bl, f"{what} image {i} blur L{l}")


@pytest.mark.parametrize("simd", [1, 0])
@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}-{c[3]}" for c in CASES])
def test_fallback_levels(oracle_mod, orbx_lib, gpu, case, simd):
    import torch
    import my_orb_slam2_amd as m
    w, h, scale, nlevels, plain = case
    ref = _ref(oracle_mod, case, simd)
    imgs = np.stack([r[0] for r in ref])
    g = m.ORBextractor(500, scale, nlevels, 20, 7, cv_simd=simd)
    what = f"{w}x{h} @{scale}/{nlevels} simd={simd}"

    g(imgs[0])
    for B in (1, 2, NIMG):
        rows = g.launch_info(B)[0]
        assert {l for l in range(nlevels) if rows[l] == 0} == plain, (what, B, rows.tolist())
    _check(g, ref, 1, what + " host image")

    for B in (2, NIMG):
        g.extract_batch_device(torch.from_numpy(imgs[:B]).to(gpu))
        torch.cuda.synchronize()
        _check(g, ref, B, what + f" device batch of {B}")

    B = 2
    v = g.input_views(w, h, B)
    v.copy_(torch.from_numpy(imgs[NIMG - B:]).to(gpu))
    g.extract_batch_resident(B)
    torch.cuda.synchronize()
    _check(g, ref[NIMG - B:], B, what + " resident batch")
