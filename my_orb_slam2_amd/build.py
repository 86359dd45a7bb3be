"""Build liborbx.so (the HIP kernels + C ABI) in-tree for gfx950.

    python -m my_orb_slam2_amd.build        # or __graft_entry__.build()

hipcc cross-compiles for gfx950 without a GPU.  The .so lands next to this file so it
travels with the repo snapshot to the GPU box (it is git-ignored, not gpurun-ignored).

Staleness is decided by content, not by file times: the build embeds a hash of every source
and header (``orbx-src:<hash>`` in the binary, also reported by ``orbx_version()``), and a
library whose embedded hash differs from the tree's is rebuilt.  A snapshot copied to another
machine keeps a fresh library fresh whatever the copy does to modification times.
"""
from __future__ import annotations

import hashlib
import os
import pathlib
import subprocess
import sys

PKG = pathlib.Path(__file__).resolve().parent
CSRC = PKG / "csrc"
LIB = PKG / "liborbx.so"
SOURCES = ["orbx_pyramid.hip", "orbx_extract.hip", "orbx_stereo.hip", "orbx_match.hip",
           "orbx_plan.hip", "orbx_capi.hip", "orbx_stereo_frame.hip", "orbx_match_capi.hip",
           "orbx_vocab.hip", "orbx_frame.hip", "orbx_kfdb.hip", "orbx_bf.hip", "orbx_rectify.hip", "orbx_triangulate.hip",
           "orbx_poseopt.hip", "orbx_sim3.hip", "orbx_sim3opt.hip", "orbx_pnp.hip",
           "orbx_localmap.hip", "orbx_host.hip"]
HEADERS = ["orbx_internal.h", "orbx_device.h", "orbx_math.h", "orbx_hypot.h", "orbx_kernels.h",
           "orbx_host.h", "orbx_stage.h", "orbx_layout.h", "orbx_extractor.h", "orbx_lm.h",
           "orbx_match_kernels.h", "orbx_matcher.h", "orbx_ransac.h", "orbx_fast_pretest.h",
           "orbx_pattern.inc", "orbx_cv.h", "orbx_distinctive.h",
           "../../include/orbx.h", "../../include/orbx_match.h", "../../include/orbx_vocab.h",
           "../../include/orbx_frame.h", "../../include/orbx_kfdb.h",
           "../../include/orbx_localmap.h"]
HASH_TAG = b"orbx-src:"

# -ffp-contract=off: every float a*b+c in the path is two roundings, as in the x86 reference
# (hipcc defaults to fast contraction).  No -ffast-math: IEEE division/rounding throughout.
# -amdgpu-mfma-vgpr-form: MFMA accumulators in VGPRs (k_bf_mfma's 16-bit keys are read by
# VALU min / max straight from them; in AGPRs each read costs a v_accvgpr_read).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
         "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wno-unused-function",
         "-mllvm", "-amdgpu-mfma-vgpr-form",
         "-I" + str(PKG.parent / "include")]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if cand and pathlib.Path(cand).exists():
            return cand
    return "hipcc"


def source_hash(extra_flags=()) -> str:
    """16 hex digits over the sources, headers and compile flags of the library."""
    h = hashlib.sha256()
    for name in SOURCES + HEADERS:
        p = CSRC / name
        h.update(name.encode() + b"\0")
        h.update(p.read_bytes() if p.exists() else b"<missing>")
    h.update(" ".join(FLAGS[:-1] + list(extra_flags)).encode())
    return h.hexdigest()[:16]


def embedded_hash(path: pathlib.Path = LIB) -> str | None:
    """The source hash a built library carries, or None."""
    try:
        data = path.read_bytes()
    except OSError:
        return None
    i = data.find(HASH_TAG)
    if i < 0:
        return None
    return data[i + len(HASH_TAG):i + len(HASH_TAG) + 16].decode("ascii", "replace")


def stale() -> bool:
    return embedded_hash() != source_hash()


def build(force: bool = False, verbose: bool = False, extra_flags=(),
          out: pathlib.Path | None = None) -> pathlib.Path:
    """Compile the library (if stale, or always with force).  `extra_flags` / `out` build a
    tuning variant (tools/variants.py) next to the product library."""
    target = pathlib.Path(out) if out else LIB
    if extra_flags and target.resolve() == LIB.resolve():
        # the product library is the sources as they are: no variant or diagnostic switches
        raise ValueError(f"refusing to build {LIB.name} with extra flags {list(extra_flags)}")
    digest = source_hash(extra_flags)
    if not force and embedded_hash(target) == digest:
        return target
    srcs = [str(CSRC / s) for s in SOURCES if (CSRC / s).exists()]
    cmd = ([hipcc()] + FLAGS + list(extra_flags) + [f'-DORBX_SRC_HASH="{digest}"'] + srcs +
           ["-o", str(target) + ".tmp"])
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(target) + ".tmp", target)
    return target


if __name__ == "__main__":
    build(force="--force" in sys.argv, verbose=True)
    print(LIB, source_hash())


# ---- the native test programs (tests/native/*.cpp) ----------------------------------------------
ROOT = PKG.parent
NATIVE = ROOT / "tests" / "native"
INCLUDE, INTEGRATION, CV_STANDIN = ROOT / "include", ROOT / "integration", NATIVE / "cv_standin"
# found at run time through the binary's RUNPATH, $ORIGIN-relative, so the tree can move
LINK_LIB = ["-L" + str(PKG), "-lorbx", "-L/opt/rocm/lib", "-Wl,-rpath-link,/opt/rocm/lib",
            "-Wl,-rpath,$ORIGIN/../../my_orb_slam2_amd"]
# -ffp-contract=off: the float statements restated in a program as written, every operation
# rounded on its own as in the kernels
REF_FLAGS = ("-Wextra", "-ffp-contract=off")
SANITIZE = ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _headers(*dirs) -> list:
    """The *.h of each directory; the *.hpp below the cv stand-in."""
    return [h for d in dirs for h in sorted(d.rglob("*.hpp") if d == CV_STANDIN else d.glob("*.h"))]


def _build_native(src, target, deps, includes, *, flags=REF_FLAGS, link_lib=False, extra=(),
                  force, verbose) -> pathlib.Path:
    """g++ `src` into `target` when the target is older than the source or its newest dependency
    (or always with force).  link_lib: against the in-tree liborbx.so, built first.  `extra`
    follows the source on the command line."""
    newest = max(p.stat().st_mtime for p in [src, *deps])
    if not force and target.exists() and target.stat().st_mtime >= newest:
        return target
    if link_lib:
        build(verbose=verbose)
    cmd = (["g++", "-std=c++17", "-O2", "-Wall", *flags] + ["-I" + str(d) for d in includes] +
           [str(src)] + (LINK_LIB if link_lib else []) + list(extra) +
           ["-o", str(target) + ".tmp"])
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(str(target) + ".tmp", target)
    return target


def _sanitized(sanitize, out, plain) -> pathlib.Path:
    """Where a reference program goes: `out` or `plain`; never a sanitised build over `plain`."""
    target = pathlib.Path(out) if out else plain
    if sanitize and target.resolve() == plain.resolve():
        raise ValueError("the sanitized program goes to a path of its own")
    return target


# the C++ boundary consumer
BOUNDARY_SRC = NATIVE / "boundary_test.cpp"
BOUNDARY_BIN = NATIVE / "boundary_test"


def build_boundary_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ against include/orbx*.h only, linked to the in-tree liborbx.so (found at run time
    through the binary's RUNPATH, $ORIGIN-relative, so the tree can move)."""
    return _build_native(BOUNDARY_SRC, BOUNDARY_BIN, _headers(INCLUDE), [INCLUDE], flags=(),
                         link_lib=True, extra=("-pthread",), force=force, verbose=verbose)


# the drop-in facade compiled as ORB-SLAM2 would include it
FACADE_SRC = NATIVE / "facade_test.cpp"
FACADE_BIN = NATIVE / "facade_test"


def build_facade_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on integration/ORBextractor.h + integration/orbx_slam2_glue.h with the cv stand-in
    headers of tests/native/cv_standin, linked to the in-tree liborbx.so."""
    return _build_native(FACADE_SRC, FACADE_BIN, _headers(INCLUDE, INTEGRATION, CV_STANDIN),
                         [INCLUDE, INTEGRATION, CV_STANDIN], flags=("-Wextra",), link_lib=True,
                         extra=("-pthread",), force=force, verbose=verbose)


# the ORBmatcher drop-in compiled as ORB-SLAM2 would include it
MATCHER_SRC = NATIVE / "matcher_test.cpp"
MATCHER_BIN = NATIVE / "matcher_test"
MATCHER_CPU_BIN = NATIVE / "matcher_test_cpu"


def build_matcher_test(force: bool = False, verbose: bool = False,
                       cpu: bool = False) -> pathlib.Path:
    """g++ on integration/ORBmatcher.h with the ORB-SLAM2 stand-in classes
    (tests/native/slam2_standin) and the cv stand-in, plus the CPU restatement it is checked
    against (oracle/orb_matcher_objects.h).  cpu=False: linked to the in-tree liborbx.so (the
    searches run on the GPU).  cpu=True: matcher_test_cpu, linked instead to the C-ABI test
    double tests/native/oracle_abi.cpp over oracle/orb_matcher_oracle.cpp (no GPU, no liborbx),
    for the CPU test suite."""
    double = [NATIVE / "oracle_abi.cpp", ROOT / "oracle" / "orb_matcher_oracle.cpp"]
    deps = (double + [ROOT / "oracle" / "orb_matcher_objects.h"] +
            _headers(INCLUDE, INTEGRATION, CV_STANDIN, NATIVE / "slam2_standin"))
    return _build_native(MATCHER_SRC, MATCHER_CPU_BIN if cpu else MATCHER_BIN, deps,
                         [INCLUDE, INTEGRATION, ROOT / "oracle", CV_STANDIN,
                          NATIVE / "slam2_standin"], link_lib=not cpu,
                         extra=([str(p) for p in double] if cpu else []) + ["-pthread"],
                         force=force, verbose=verbose)


# the RGB-D glue compiled as ORB-SLAM2 would include it
RGBD_SRC = NATIVE / "rgbd_test.cpp"
RGBD_BIN = NATIVE / "rgbd_test"


def build_rgbd_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on integration/orbx_slam2_glue.h (ComputeStereoFromRGBD) with the cv stand-in and
    tests/native/rgbd_standin.h, linked to the in-tree liborbx.so."""
    deps = [NATIVE / "rgbd_standin.h"] + _headers(INCLUDE, INTEGRATION, CV_STANDIN)
    return _build_native(RGBD_SRC, RGBD_BIN, deps, [INCLUDE, INTEGRATION, CV_STANDIN, NATIVE],
                         link_lib=True, extra=("-pthread",), force=force, verbose=verbose)


# the rectifier glue compiled as ORB-SLAM2 would include it
REMAP_SRC = NATIVE / "remap_test.cpp"
REMAP_BIN = NATIVE / "remap_test"


def build_remap_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on integration/orbx_slam2_glue.h (orbx_glue::Rectifier) with the cv stand-in, linked to
    the in-tree liborbx.so."""
    return _build_native(REMAP_SRC, REMAP_BIN, _headers(INCLUDE, INTEGRATION, CV_STANDIN),
                         [INCLUDE, INTEGRATION, CV_STANDIN], link_lib=True, extra=("-pthread",),
                         force=force, verbose=verbose)


# the projection loops restated over the cv stand-in
PROJECT_REF_SRC = NATIVE / "project_ref.cpp"
PROJECT_REF_BIN = NATIVE / "project_ref"


def build_project_ref(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on the cv stand-in and the record layouts of include/orbx_frame.h only: no liborbx and
    no GPU (the CPU reference of orbx_project_map_points*)."""
    return _build_native(PROJECT_REF_SRC, PROJECT_REF_BIN, _headers(INCLUDE, CV_STANDIN),
                         [INCLUDE, CV_STANDIN], force=force, verbose=verbose)


# CreateNewMapPoints' loop restated over the cv stand-in
TRIANGULATE_REF_SRC = NATIVE / "triangulate_ref.cpp"
TRIANGULATE_REF_BIN = NATIVE / "triangulate_ref"


def build_triangulate_ref(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on the cv stand-in and the record layouts of include/ only: no liborbx and no GPU (the
    CPU reference of orbx_triangulate_matches*)."""
    return _build_native(TRIANGULATE_REF_SRC, TRIANGULATE_REF_BIN, _headers(INCLUDE, CV_STANDIN),
                         [INCLUDE, CV_STANDIN], force=force, verbose=verbose)


# PoseOptimization restated in plain C++ doubles
POSEOPT_REF_SRC = NATIVE / "poseopt_ref.cpp"
POSEOPT_REF_BIN = NATIVE / "poseopt_ref"


def build_poseopt_ref(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on the record layouts of include/ and csrc/orbx_math.h (orbx_sincos_f64) only: no
    liborbx and no GPU (the CPU reference of orbx_pose_optimization*)."""
    return _build_native(POSEOPT_REF_SRC, POSEOPT_REF_BIN,
                         [CSRC / "orbx_math.h"] + _headers(INCLUDE), [INCLUDE, CSRC],
                         force=force, verbose=verbose)


# Sim3Solver restated over the cv stand-in
SIM3_REF_SRC = NATIVE / "sim3_ref.cpp"
SIM3_REF_BIN = NATIVE / "sim3_ref"


def build_sim3_ref(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on the cv stand-in, tests/native/cv_sim3_standin.hpp, the record layouts of include/ and
    csrc/orbx_math.h (orbx_atan2_f64, orbx_sincos_f64) only: no liborbx and no GPU (the CPU
    reference of orbx_sim3_iterate*)."""
    deps = [NATIVE / "cv_sim3_standin.hpp", CSRC / "orbx_math.h"] + _headers(INCLUDE, CV_STANDIN)
    return _build_native(SIM3_REF_SRC, SIM3_REF_BIN, deps, [INCLUDE, CSRC, CV_STANDIN, NATIVE],
                         force=force, verbose=verbose)


# OptimizeSim3 restated in plain C++ doubles
SIM3OPT_REF_SRC = NATIVE / "sim3opt_ref.cpp"
SIM3OPT_REF_BIN = NATIVE / "sim3opt_ref"


def build_sim3opt_ref(force: bool = False, verbose: bool = False, sanitize: bool = False,
                      out: pathlib.Path | None = None) -> pathlib.Path:
    """g++ on the record layouts of include/ and csrc/orbx_math.h (orbx_sincos_f64, orbx_exp_f64)
    only: no liborbx and no GPU (the CPU reference of orbx_sim3_optimize*).  sanitize: the
    stand-alone program with -fsanitize=address,undefined, to `out`."""
    return _build_native(SIM3OPT_REF_SRC, _sanitized(sanitize, out, SIM3OPT_REF_BIN),
                         [CSRC / "orbx_math.h"] + _headers(INCLUDE), [INCLUDE, CSRC],
                         extra=SANITIZE if sanitize else (), force=force, verbose=verbose)


# PnPsolver restated in plain C++
PNP_REF_SRC = NATIVE / "pnp_ref.cpp"
PNP_REF_BIN = NATIVE / "pnp_ref"


def build_pnp_ref(force: bool = False, verbose: bool = False, sanitize: bool = False,
                  out: pathlib.Path | None = None) -> pathlib.Path:
    """g++ on the record layouts of include/ only: no liborbx and no GPU (the CPU reference of
    orbx_pnp_iterate*).  sanitize: the stand-alone program with -fsanitize=address,undefined, to
    `out`."""
    return _build_native(PNP_REF_SRC, _sanitized(sanitize, out, PNP_REF_BIN), _headers(INCLUDE),
                         [INCLUDE], extra=SANITIZE if sanitize else (), force=force,
                         verbose=verbose)


# Tracking::UpdateLocalMap restated over stand-in KeyFrame / MapPoint objects
LOCALMAP_REF_SRC = NATIVE / "localmap_ref.cpp"
LOCALMAP_REF_BIN = NATIVE / "localmap_ref"


def build_localmap_ref(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on the standard library only: no liborbx and no GPU (the CPU reference of
    orbx_update_local_map*)."""
    return _build_native(LOCALMAP_REF_SRC, LOCALMAP_REF_BIN, [], [], flags=("-Wextra",),
                         force=force, verbose=verbose)


# UpdateNormalAndDepth / ComputeDistinctiveDescriptors restated over stand-in objects and the cv
# stand-in
MPREFRESH_REF_SRC = NATIVE / "mprefresh_ref.cpp"
MPREFRESH_REF_BIN = NATIVE / "mprefresh_ref"


def build_mprefresh_ref(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on the cv stand-in and the standard library only: no liborbx and no GPU (the CPU
    reference of orbx_refresh_map_points*)."""
    return _build_native(MPREFRESH_REF_SRC, MPREFRESH_REF_BIN, _headers(CV_STANDIN), [CV_STANDIN],
                         force=force, verbose=verbose)


# the staging plan of the host-array entry points, on its own
STAGING_SRC = NATIVE / "staging_test.cpp"
STAGING_BIN = NATIVE / "staging_test"


def build_staging_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on csrc/orbx_stage.h only, with -fsanitize=address,undefined: no HIP, no liborbx and no
    GPU."""
    return _build_native(STAGING_SRC, STAGING_BIN, [CSRC / "orbx_stage.h"], [CSRC], extra=SANITIZE,
                         force=force, verbose=verbose)


# the extractor's output-block layouts, on their own
LAYOUT_SRC = NATIVE / "layout_test.cpp"
LAYOUT_BIN = NATIVE / "layout_test"


def build_layout_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on csrc/orbx_layout.h (and the record layouts of include/orbx.h) only, with
    -fsanitize=address,undefined: no HIP, no liborbx and no GPU."""
    return _build_native(LAYOUT_SRC, LAYOUT_BIN, [CSRC / "orbx_layout.h", INCLUDE / "orbx.h"],
                         [CSRC], extra=SANITIZE, force=force, verbose=verbose)


# k_fast's 4-pixel compass pre-test, on its own
FAST_PRETEST_SRC = NATIVE / "fast_pretest_test.cpp"
FAST_PRETEST_BIN = NATIVE / "fast_pretest_test"


def build_fast_pretest_test(force: bool = False, verbose: bool = False) -> pathlib.Path:
    """g++ on csrc/orbx_fast_pretest.h (and csrc/orbx_math.h for ORBX_HD) only, with -fsanitize=address,undefined: no HIP, no liborbx
    and no GPU."""
    return _build_native(FAST_PRETEST_SRC, FAST_PRETEST_BIN,
                         [CSRC / "orbx_fast_pretest.h", CSRC / "orbx_math.h"], [CSRC],
                         extra=SANITIZE, force=force, verbose=verbose)
