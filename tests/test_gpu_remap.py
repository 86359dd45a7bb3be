"""GPU: k_remap against the numpy restatement ``remap_closed`` (tests/remap_cases.py), bit for bit,
on every directed case through the three entry points (orbx_remap_batch_device, orbx_remap, the
stereo form), with every destination byte outside the images intact; raw EuRoC-size pairs through
``RectifiedStereoBatch`` against ``StereoBatch`` on host-rectified images; the error statuses."""
import ctypes
import pathlib

import numpy as np
import pytest

import remap_cases as rc

pytestmark = pytest.mark.gpu
ROOT = pathlib.Path(__file__).resolve().parents[1]
EUROC_YAML = str(ROOT / "tests" / "golden" / "euroc_stereo.yaml")


@pytest.fixture(scope="module")
def chunk(orbx_lib):
    from my_orb_slam2_amd import rectify
    return rectify.images_per_chunk()


@pytest.fixture(scope="module")
def cases(chunk):
    return rc.build_cases(chunk)


def _vp(t, off=0):
    return ctypes.c_void_p(t.data_ptr() + off)


def _rectifier(c):
    import my_orb_slam2_amd as m
    _, sh, sw = c["src"].shape
    return m.Rectifier(c["map1"], c["map2"], src_size=(sw, sh))


def test_batch_device_every_case(orbx_lib, gpu, cases):
    import torch
    for c in cases:
        lay = rc.layout(c)
        r = _rectifier(c)
        src = torch.from_numpy(lay["src"]).to(gpu)
        dst = torch.from_numpy(lay["dst"]).to(gpu)
        st = orbx_lib.orbx_remap_batch_device(
            r._h, _vp(src, lay["src_off"]), lay["src_rs"], lay["src_is"], _vp(dst, lay["dst_off"]),
            lay["dst_rs"], lay["dst_is"], c["src"].shape[0], None)
        assert st == 0, (c["name"], st)
        torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), rc.expected_dst(c, lay)), c["name"]


def test_tensor_form_equals_closed(gpu, cases):
    import torch
    c = next(c for c in cases if c["name"] == "src13x7_dst9x11")
    r = _rectifier(c)
    src = torch.from_numpy(c["src"]).to(gpu)
    dst = torch.full((c["src"].shape[0],) + c["map1"].shape, rc.SENTINEL, dtype=torch.uint8,
                     device=gpu)
    r.remap_batch_device(src, dst)
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), rc.remap_closed(c["src"], c["map1"], c["map2"]))


def test_host_form_every_case(gpu, cases):
    for c in cases:
        lay = rc.layout(c)
        r = _rectifier(c)
        _, sh, sw = c["src"].shape
        dh, dw = c["map1"].shape
        want = rc.expected_dst(c, lay)
        got = lay["dst"].copy()
        for i in range(min(c["src"].shape[0], 2)):
            s = np.lib.stride_tricks.as_strided(lay["src"][lay["src_off"] + i * lay["src_is"]:],
                                                (sh, sw), (lay["src_rs"], 1))
            d = np.lib.stride_tricks.as_strided(got[lay["dst_off"] + i * lay["dst_is"]:],
                                                (dh, dw), (lay["dst_rs"], 1))
            r.remap(s, d)
            wi = np.lib.stride_tricks.as_strided(want[lay["dst_off"] + i * lay["dst_is"]:],
                                                 (dh, dw), (lay["dst_rs"], 1))
            assert np.array_equal(d, wi), (c["name"], i)
        # nothing outside the images was written
        B = min(c["src"].shape[0], 2)
        end = lay["dst_off"] + B * lay["dst_is"]
        assert np.array_equal(got[:end], want[:end]), c["name"]
        assert (got[end:] == rc.SENTINEL).all(), c["name"]


def test_stereo_form(orbx_lib, gpu, chunk):
    import torch
    for cl, cr in rc.build_stereo_cases(chunk):
        ll, lr = rc.layout(cl), rc.layout(cr)
        rl, rr = _rectifier(cl), _rectifier(cr)
        assert (ll["src_rs"], ll["src_is"], ll["dst_rs"], ll["dst_is"]) == \
            (lr["src_rs"], lr["src_is"], lr["dst_rs"], lr["dst_is"])
        sl, sr = torch.from_numpy(ll["src"]).to(gpu), torch.from_numpy(lr["src"]).to(gpu)
        dl, dr = torch.from_numpy(ll["dst"]).to(gpu), torch.from_numpy(lr["dst"]).to(gpu)
        st = orbx_lib.orbx_remap_stereo_batch_device(
            rl._h, rr._h, _vp(sl, ll["src_off"]), _vp(sr, lr["src_off"]), ll["src_rs"],
            ll["src_is"], _vp(dl, ll["dst_off"]), _vp(dr, lr["dst_off"]), ll["dst_rs"],
            ll["dst_is"], cl["src"].shape[0], None)
        assert st == 0, (cl["name"], st)
        torch.cuda.synchronize()
        assert np.array_equal(dl.cpu().numpy(), rc.expected_dst(cl, ll)), cl["name"]
        assert np.array_equal(dr.cpu().numpy(), rc.expected_dst(cr, lr)), cr["name"]
        # the maps differ: a side remapped with the other side's map would not pass
        assert not np.array_equal(rc.remap_closed(cl["src"], cr["map1"], cr["map2"]),
                                  rc.remap_closed(cl["src"], cl["map1"], cl["map2"]))


def test_rectified_stereo_batch_equals_host_rectified(gpu):
    import torch
    import my_orb_slam2_amd as m
    from my_orb_slam2_amd import synth
    ml, mr, s = rc.euroc_maps(EUROC_YAML)
    W, H, B = rc.EUROC_W, rc.EUROC_H, 2
    pairs = [synth.stereo_pair(300 + i, W, H) for i in range(B)]
    rawL = np.stack([p[0] for p in pairs])
    rawR = np.stack([p[1] for p in pairs])
    rectL, rectR = rc.remap_closed(rawL, *ml), rc.remap_closed(rawR, *mr)
    mbf = float(s["bf"])
    mb = float(np.float32(s["bf"]) / np.float32(s["fx"]))
    kw = dict(nfeatures=1200)
    # the reference run takes the host-rectified images in the level-0 slots too (input_views +
    # run_resident), the path RectifiedStereoBatch extends
    ref = m.StereoBatch(B, **kw)
    Lv, Rv = ref.input_views(W, H)
    Lv.copy_(torch.from_numpy(rectL).to(gpu))
    Rv.copy_(torch.from_numpy(rectR).to(gpu))
    uR0, de0, nv0 = [t.cpu().numpy() for t in ref.run_resident(mbf, mb)]
    torch.cuda.synchronize()
    rb = m.RectifiedStereoBatch(B, m.Rectifier(*ml), m.Rectifier(*mr), **kw)
    uR1, de1, nv1 = [t.cpu().numpy() for t in rb(torch.from_numpy(rawL).to(gpu),
                                                  torch.from_numpy(rawR).to(gpu), mbf, mb)]
    torch.cuda.synchronize()
    vl, vr = rb.input_views(W, H)
    assert np.array_equal(vl.cpu().numpy(), rectL) and np.array_equal(vr.cpu().numpy(), rectR)
    assert np.array_equal(nv0, nv1) and nv0.min() > 0
    for side in ("left", "right"):
        n0, k0, d0 = ref.fetch(side)
        n1, k1, d1 = rb.fetch(side)
        assert np.array_equal(n0, n1) and n0.min() > 100, n0
        for i in range(B):
            assert k0[i][:n0[i]].tobytes() == k1[i][:n1[i]].tobytes(), (side, i)
            assert np.array_equal(d0[i][:n0[i]], d1[i][:n1[i]]), (side, i)
        if side == "left":
            for i in range(B):
                assert uR0[i, :n0[i]].tobytes() == uR1[i, :n0[i]].tobytes()
                assert de0[i, :n0[i]].tobytes() == de1[i, :n0[i]].tobytes()


def test_statuses(orbx_lib, gpu):
    import torch
    import my_orb_slam2_amd as m
    ident = np.zeros((4, 8), np.float32)
    with pytest.raises(m.OrbxError) as e:
        m.Rectifier(ident, ident, src_size=(32768, 4))
    assert e.value.code == -4
    with pytest.raises(m.OrbxError) as e:
        m.Rectifier(ident, ident, src_size=(0, 4))
    assert e.value.code == -1
    r = m.Rectifier(ident, ident)                       # 8 x 4 -> 8 x 4
    r2 = m.Rectifier(np.zeros((4, 12), np.float32), np.zeros((4, 12), np.float32), src_size=(8, 4))
    buf = torch.zeros(4096, dtype=torch.uint8, device=gpu)
    a, b = _vp(buf), _vp(buf, 2048)
    L = orbx_lib
    assert L.orbx_remap_batch_device(r._h, None, 8, 32, b, 8, 32, 1, None) == -1
    assert L.orbx_remap_batch_device(r._h, a, 8, 32, None, 8, 32, 1, None) == -1
    assert L.orbx_remap_batch_device(r._h, a, 8, 32, b, 8, 32, 0, None) == -1
    assert L.orbx_remap_batch_device(r._h, a, 7, 32, b, 8, 32, 1, None) == -1
    assert L.orbx_remap_batch_device(r._h, a, 8, 32, b, 7, 32, 1, None) == -1
    assert L.orbx_remap_batch_device(r._h, a, 8, 32, b, 8, 32, 2, None) == 0
    assert L.orbx_remap_stereo_batch_device(r._h, r2._h, a, a, 8, 32, b, b, 12, 48, 1, None) == -1
    assert L.orbx_remap_stereo_batch_device(r._h, None, a, a, 8, 32, b, b, 8, 32, 1, None) == -1
    assert L.orbx_remap_stereo_batch_device(r._h, r._h, a, a, 8, 32, b, _vp(buf, 3072), 8, 32, 1,
                                            None) == 0
    torch.cuda.synchronize()


def test_host_form_guards(gpu):
    """orbx_remap through the smallest rectifier with dst_stride > dst_w, the destination inside a
    sentinel-filled allocation: the dst_w bytes of each row are the restatement's, the row padding
    and the guards keep the sentinel."""
    import host_array_cases as hc
    c = hc.case("remap")
    dst = c.call()["dst"]
    assert dst.guards_intact()
    dw = c.c0["map1"].shape[1]
    want = rc.remap_closed(c.c0["src"][:1], c.c0["map1"], c.c0["map2"])[0]
    assert np.array_equal(dst.a[:, :dw], want)
    assert (dst.a[:, dw:] == hc.SENT).all() and dst.a.shape[1] > dw
