"""The graphs of the host-image calls across workspace regrowth, on ONE handle: orbx_extract and
orbx_stereo_frame_view each replay a captured graph whose key names the output block's layout and
every buffer, and each call that regrows the workspace must make the other's graph stale.

    1. orbx_extract                      (workspace of 1 image, the single-image graph is new)
    2. orbx_stereo_frame_view            (grows to 2 images, the frame graph is new, one DMA back)
    3. orbx_extract                      (the single-image graph rebuilt against the regrown buffers)
    4. orbx_extractor_prepare(batch 4),
       orbx_stereo_frame_view            (stale key, the stereo block no longer follows image 1:
                                          two DMAs back)
       orbx_extract                      (rebuilt once more, in the four-image layout)

once without and once with orbx_extractor_host_pyramid (the pinned pyramid block is part of the
single-image graph and of its key).  Every result equals the CPU oracle bit for bit, and every
stereo result equals orbx_stereo_frames_device on the same pair.
"""
import numpy as np
import pytest

from helpers import assert_bytes_equal, assert_f32_bits_equal, assert_kps_equal
from my_orb_slam2_amd import synth

pytestmark = pytest.mark.gpu

PARAMS = (600, 1.2, 8, 20, 7)
SIZE = (320, 240)
MBF, FX = 386.1448, 718.856
MB = float(np.float32(MBF) / np.float32(FX))


@pytest.fixture(scope="module")
def reference(oracle_mod, orbx_lib, gpu):
    """The pair, the oracle's results for it and orbx_stereo_frames_device's (read-only)."""
    import torch
    import my_orb_slam2_amd as m
    L, R = synth.stereo_pair(77, *SIZE)
    ol, orr = oracle_mod.OracleExtractor(*PARAMS), oracle_mod.OracleExtractor(*PARAMS)
    kl, dl = ol(L)
    kr, dr = orr(R)
    u, d, nv = oracle_mod.stereo_match(ol, orr, len(kl), MBF, MB)
    levels = [ol.level(l) for l in range(ol.nlevels)]
    sb = m.StereoBatch(1, *PARAMS)
    uR, dep, nvalid = sb(torch.from_numpy(L[None]).to(gpu), torch.from_numpy(R[None]).to(gpu),
                         MBF, MB)
    torch.cuda.synchronize()
    nl, kps_l, desc_l = sb.fetch("left")
    nr, kps_r, desc_r = sb.fetch("right")
    dev = dict(kl=kps_l[0, :nl[0]], dl=desc_l[0, :nl[0]], kr=kps_r[0, :nr[0]],
               dr=desc_r[0, :nr[0]], u=uR.cpu().numpy()[0, :nl[0]],
               d=dep.cpu().numpy()[0, :nl[0]], nv=int(nvalid.cpu().numpy()[0]))
    assert len(kl) > 50 and nv > 0, "the pair exercises nothing"
    return dict(L=L, R=R, kl=kl, dl=dl, kr=kr, dr=dr, u=u, d=d, nv=nv, levels=levels, dev=dev)


def _check_single(ext, ref, host_pyr, what):
    k, d = ext(ref["L"])
    assert_kps_equal(k, ref["kl"], what)
    assert_bytes_equal(d, ref["dl"], what + " descriptors")
    if host_pyr:
        got = ext.host_pyramid_view()
        assert len(got) == len(ref["levels"])
        for l, (a, b) in enumerate(zip(got, ref["levels"])):
            assert_bytes_equal(a, b, f"{what} host pyramid L{l}")


def _check_frame(ext, ref, what):
    import my_orb_slam2_amd as m
    kl, dl, kr, dr, u, d, nv = m.extract_stereo(ext, ref["L"], ref["R"], MBF, MB)
    for other, name in ((ref, "oracle"), (ref["dev"], "orbx_stereo_frames_device")):
        assert_kps_equal(kl, other["kl"], f"{what} left vs {name}")
        assert_bytes_equal(dl, other["dl"], f"{what} left descriptors vs {name}")
        assert_kps_equal(kr, other["kr"], f"{what} right vs {name}")
        assert_bytes_equal(dr, other["dr"], f"{what} right descriptors vs {name}")
        assert_f32_bits_equal(u, other["u"], f"{what} uRight vs {name}")
        assert_f32_bits_equal(d, other["d"], f"{what} depth vs {name}")
        assert nv == other["nv"], f"{what} n_valid vs {name}"


@pytest.mark.parametrize("host_pyr", [False, True])
def test_graphs_follow_workspace_regrowth(reference, host_pyr):
    import my_orb_slam2_amd as m
    ext = m.ORBextractor(*PARAMS)
    if host_pyr:
        ext.host_pyramid(True)
    _check_single(ext, reference, host_pyr, "1 extract")
    _check_frame(ext, reference, "2 frame, workspace of 2")
    _check_single(ext, reference, host_pyr, "3 extract after regrowth")
    ext.prepare(*SIZE, 4)
    _check_frame(ext, reference, "4 frame, workspace of 4")
    _check_single(ext, reference, host_pyr, "4 extract, workspace of 4")
    # and replays of both graphs, nothing stale
    _check_frame(ext, reference, "frame replay")
    _check_single(ext, reference, host_pyr, "extract replay")
    ext.close()
