"""GPU: the directed brute-force top-2 cases (tests/bf_cases.py) on k_bf_top2, k_bf_mfma and
k_bf_merge.

Every case runs with both distance kernels, through orbx_hamming_bf_top2 (host arrays) and
orbx_hamming_bf_top2_device (the row-limit case through the device entry only), exact against
the oracle and against the outcome the case states (tests/test_bf_cases.py has checked the
oracle and a plain reference on the same cases).  Before a case is relied on, its regime is
asserted from orbx_matcher_bf_launch_info: chunk, nchunks, query_blocks, nqpad, merge_slice.
One ORBmatcher serves the whole module, and the table runs forwards, backwards and with the
kernel alternating case by case: the partials scratch only grows and its query stride changes
from call to call, so a large call must not leak into a small one.  Outputs are filled with -7
before every call.
"""
import ctypes

import numpy as np
import pytest

import bf_cases as bc
from bf_cases import MFMA, VALU

pytestmark = pytest.mark.gpu

INVALID = -1
FILL = -7
_state = {}


def matcher():
    """The one ORBmatcher of this module."""
    from my_orb_slam2_amd import ORBmatcher
    if "m" not in _state:
        _state["m"] = ORBmatcher(0.75, True)
    return _state["m"]


def oracle_of(c):
    """The oracle's result per case, computed once, never modified."""
    import oracle.matcher as om
    key = ("oracle", c.name)
    if key not in _state:
        r = om.bf_top2(c.q, c.db)
        for a in r:
            a.setflags(write=False)
        _state[key] = r
    return _state[key]


def device_arrays(c, gpu):
    """The case's q and db on the device, uploaded once."""
    import torch
    key = ("dev", c.name)
    if key not in _state:
        # (the cases' arrays are read-only: torch wants writable memory, hence the copies)
        dq = torch.from_numpy(c.q.copy()).to(gpu)
        ddb = torch.from_numpy(c.db.copy() if c.ndb else np.zeros((1, 32), np.uint8)).to(gpu)
        _state[key] = (dq, ddb)
    return _state[key]


def set_regime(m, c, kernel):
    """Select the case's kernel and chunk and assert the launch geometry it means to run."""
    m.set_bf_kernel(kernel)
    m.set_bf_chunk(c.chunk or 0)
    info = m.bf_launch_info(c.nq, c.ndb)
    assert info == c.regime(kernel), f"{c.name} / {bc.KERNEL_NAMES[kernel]}: regime {info}"


def run_host(m, c):
    """orbx_hamming_bf_top2 with outputs filled beforehand (ORBmatcher.hamming_bf_top2
    allocates its own)."""
    from my_orb_slam2_amd._lib import check, ptr
    out = [np.full(c.nq, FILL, np.int32) for _ in range(3)]
    check("orbx_hamming_bf_top2", m._lib.orbx_hamming_bf_top2(
        m._h, ptr(c.q), c.nq, ptr(c.db), c.ndb, *[ptr(o) for o in out]))
    return out


def run_device(m, c, gpu):
    import torch
    dq, ddb = device_arrays(c, gpu)
    out = [torch.full((c.nq,), FILL, dtype=torch.int32, device=gpu) for _ in range(3)]
    m.hamming_bf_top2_device(dq, c.nq, ddb, c.ndb, *out, idx_base=c.idx_base)
    torch.cuda.synchronize(gpu)
    return [o.cpu().numpy() for o in out]


def mismatches(c, got, want, what):
    """Failure lines: the result arrays against the oracle's, then the stated outcomes."""
    bad = []
    for g, w, name in zip(got, want, ("best_idx", "best_dist", "second_dist")):
        if not np.array_equal(g, w):
            i = int(np.nonzero(g != w)[0][0])
            bad.append(f"{what}: {name}[{i}] = {int(g[i])}, oracle {int(w[i])} "
                       f"({int((g != w).sum())} of {len(w)} differ)")
    for i, e in c.expect.items():
        e = (e[0] + c.idx_base if e[0] >= 0 and what.endswith("device") else e[0], e[1], e[2])
        gi = (int(got[0][i]), int(got[1][i]), int(got[2][i]))
        if gi != e and not bad:
            bad.append(f"{what}: query {i} = {gi}, the case states {e}")
    return bad


def run_case(c, kernel, gpu):
    m = matcher()
    set_regime(m, c, kernel)
    ora = oracle_of(c)
    tag = f"{c.name} / {bc.KERNEL_NAMES[kernel]}"
    bad = []
    if not c.device_only:
        bad += mismatches(c, run_host(m, c), ora, f"{tag} / host")
    bad += mismatches(c, run_device(m, c, gpu), c.with_base(ora), f"{tag} / device")
    return bad


def table(order):
    cs = list(bc.cases())
    return cs[::-1] if order == "reverse" else cs


@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_cases_both_kernels(oracle_mod, orbx_lib, gpu, order):
    bad = []
    for c in table(order):
        for k in (c.kernels if order == "forward" else c.kernels[::-1]):
            bad += run_case(c, k, gpu)
    matcher().set_bf_chunk(0)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("first", [MFMA, VALU], ids=["mfma_first", "valu_first"])
def test_cases_kernel_alternating(oracle_mod, orbx_lib, gpu, first):
    """The kernel changes from case to case (and with it the partials' layout in the shared
    scratch); the row-limit case has run in both orders above."""
    bad = []
    for i, c in enumerate(x for x in bc.cases() if not x.device_only):
        k = (first + i) % 2
        if k in c.kernels:
            bad += run_case(c, k, gpu)
    matcher().set_bf_chunk(0)
    assert not bad, "\n".join(bad)


# ---- the contract of the two host-side entry points ---------------------------------------------

def test_set_bf_chunk_validation(orbx_lib):
    m = matcher()
    L, h = m._lib, m._h
    m.set_bf_kernel(MFMA)
    m.set_bf_chunk(0)
    auto = [m.bf_launch_info(nq, ndb) for nq, ndb in ((1000, 10**7), (1, 5), (2049, 70000))]
    m.set_bf_chunk(320)
    for rows in (1, 64, 192, 255, 257, 300, 352 + 16, (1 << 23) - 63, (1 << 23) - 32, 1 << 23,
                 (1 << 23) + 64, 1 << 31, -256, -64, -1):
        assert L.orbx_matcher_set_bf_chunk(h, rows) == INVALID, rows
        assert m.bf_launch_info(5, 1000)["chunk"] == 320, f"refused {rows} changed the setting"
    with pytest.raises(Exception, match="ORBX_ERR_INVALID"):
        m.set_bf_chunk(100)
    for rows in (256, 320, 576, 1 << 22, (1 << 23) - 64):
        m.set_bf_chunk(rows)
        assert m.bf_launch_info(5, 1000)["chunk"] == rows
    # 0 restores the automatic choice, which does not depend on what was set in between
    m.set_bf_chunk(0)
    assert [m.bf_launch_info(nq, ndb) for nq, ndb in ((1000, 10**7), (1, 5), (2049, 70000))] == auto
    assert auto[1]["chunk"] == 256 and auto[0]["chunk"] % 64 == 0 and auto[0]["chunk"] > 256
    assert auto[0]["nchunks"] * auto[0]["chunk"] >= 10**7 > (auto[0]["nchunks"] - 1) * auto[0]["chunk"]


def test_bf_launch_info_under_the_override(orbx_lib):
    m = matcher()
    L, h = m._lib, m._h
    m.set_bf_chunk(320)
    for kernel, qpb in ((MFMA, 1024), (VALU, 256)):
        m.set_bf_kernel(kernel)
        for nq, ndb in ((1, 0), (5, 1), (5, 320), (5, 321), (1024, 420), (1025, 3201), (2049, 25 * 320)):
            nchunks = -(-ndb // 320)
            nqpad = -(-nq // 1024) * 1024
            assert m.bf_launch_info(nq, ndb) == dict(
                chunk=320, nchunks=nchunks, query_blocks=nqpad // qpb, nqpad=nqpad,
                merge_slice=-(-nchunks // 8), partial_bytes=8 * nchunks * nqpad), (kernel, nq, ndb)
    from my_orb_slam2_amd._lib import BfLaunchInfo
    r = BfLaunchInfo()
    for nq, ndb in ((-1, 10), (5, -1), (5, 2**31 - 1), (5, 2**40)):
        assert L.orbx_matcher_bf_launch_info(h, nq, ndb, ctypes.byref(r)) == INVALID, (nq, ndb)
    assert L.orbx_matcher_bf_launch_info(h, 5, 10, None) == INVALID
    m.set_bf_chunk(0)
    m.set_bf_kernel(MFMA)


def test_device_entry_refusals(oracle_mod, orbx_lib, gpu):
    """ndb + idx_base >= 2^31 - 1, a negative idx_base and a d_q or d_db that is not 4-byte
    aligned (any byte slice of a uint8 tensor) are refused before anything is launched: the
    outputs keep their fill.  An offset of 4 bytes is within the contract and gives the rows
    from there on."""
    import torch
    from my_orb_slam2_amd._lib import ptr
    c = next(x for x in bc.cases() if x.name == "ties_c256")
    m = matcher()
    L, h = m._lib, m._h
    nq, ndb = c.nq, c.ndb - 1
    qbuf = torch.zeros(32 * nq + 8, dtype=torch.uint8, device=gpu)
    dbuf = torch.zeros(32 * c.ndb + 8, dtype=torch.uint8, device=gpu)
    qbuf[:32 * nq] = torch.from_numpy(c.q.reshape(-1).copy()).to(gpu)
    dbuf[:32 * c.ndb] = torch.from_numpy(c.db.reshape(-1).copy()).to(gpu)
    out = [torch.full((nq,), FILL, dtype=torch.int32, device=gpu) for _ in range(3)]

    def call(dq, ddb, n, base):
        return L.orbx_hamming_bf_top2_device(h, ptr(dq), nq, ptr(ddb), n, base,
                                             *[ptr(o) for o in out], None)

    for kernel in (MFMA, VALU):
        m.set_bf_kernel(kernel)
        for chunk in (0, 256):
            m.set_bf_chunk(chunk)
            for off in (1, 2, 3, 5, 31):
                assert call(qbuf, dbuf[off:], ndb, 0) == INVALID, ("d_db", off)
                assert call(qbuf[off:], dbuf, ndb, 0) == INVALID, ("d_q", off)
            assert call(qbuf, dbuf, ndb, -1) == INVALID
            assert call(qbuf, dbuf, ndb, bc.INT_MAX - ndb) == INVALID
            assert call(qbuf, dbuf, ndb, 2**40) == INVALID
            assert call(qbuf, dbuf, -1, 0) == INVALID
            torch.cuda.synchronize(gpu)
            for o in out:
                assert (o.cpu().numpy() == FILL).all(), "a refused call wrote its outputs"
    # 4-byte aligned but not row aligned: rows 0 .. ndb - 1 of the view are bytes 4 .. of the
    # buffer.  Built as such: a database whose row k is bytes [32 k + 4, 32 k + 36).
    import oracle.matcher as om
    shifted = np.concatenate([c.db.reshape(-1)[4:], np.zeros(4, np.uint8)]).reshape(-1, 32)[:ndb]
    want = om.bf_top2(c.q, shifted)
    m.set_bf_chunk(256)
    for kernel in (MFMA, VALU):
        m.set_bf_kernel(kernel)
        assert call(qbuf, dbuf[4:], ndb, 0) == 0
        torch.cuda.synchronize(gpu)
        for o, w in zip(out, want):
            np.testing.assert_array_equal(o.cpu().numpy(), w)
        for o in out:
            o.fill_(FILL)
    m.set_bf_chunk(0)
    m.set_bf_kernel(MFMA)
