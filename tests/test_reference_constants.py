"""Every constant the reference holds as SOURCE TEXT on the hot path, compared with what the oracle AND the product compile in
(VERDICT r5, next-round item 4).  The values were parsed out of the reference's own files (one parser per section below) and are
recorded in tests/golden/reference_constants.json -- scalars as they are, the two tables (BRIEF pattern, GMS rotation patterns) as
length, range and SHA-256 only.  The checks of this project's code run against that record everywhere; where the reference tree is
present, every section is parsed again and must equal the record.  `python tests/test_reference_constants.py` rewrites the record.

It does not make the oracle a reference OUTPUT (no OpenCV / Eigen build exists in this image: DESIGN.md section 2); it removes the
indirection for everything that is a literal."""
import ctypes as C
import hashlib
import json
import math
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_constants.json")


def _have_ref():
    return os.path.isdir(os.path.join(REF, "src"))


def _ref(path):
    return open(os.path.join(REF, path), errors="replace").read()


def _ours(path):
    return open(os.path.join(ROOT, path)).read()


def _lines(text, a, b):
    return "\n".join(text.splitlines()[a - 1:b])


def _ints(text):
    return [int(v) for v in re.findall(r"-?\d+", text)]


def _one(pattern, text, cast=float):
    m = re.findall(pattern, text)
    assert len(m) >= 1, pattern
    assert len(set(m)) == 1, (pattern, m)
    return cast(m[0])


def _digest(values):
    return hashlib.sha256(",".join(str(int(v)) for v in values).encode()).hexdigest()


def _recorded(section):
    """The recorded values of one section; parsed again from the reference tree and compared where that tree exists."""
    rec = json.load(open(GOLDEN))[section]
    if _have_ref():
        assert json.loads(json.dumps(PARSERS[section]())) == rec, f"tests/golden/reference_constants.json [{section}] differs from the reference tree"
    return rec


# ---------------------------------------------------------------------------------------------- ORBextractor
def _parse_brief_pattern():
    """bit_pattern_31_[256 * 4], src/ORBextractor.cc:162-419: length, range and digest."""
    src = _ref("src/ORBextractor.cc")
    m = re.search(r"static int bit_pattern_31_\[256 \* 4\]\s*=\s*\{(.*?)\};", src, re.S)
    assert m, "bit_pattern_31_ not found"
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)  # the /*mean (0), correlation (0)*/ annotations
    body = re.sub(r"//[^\n]*", "", body)
    vals = _ints(body)
    return dict(count=len(vals), min=min(vals), max=max(vals), sha256=_digest(vals))


def test_brief_pattern_is_the_references_table():
    """bit_pattern_31_[256 * 4], src/ORBextractor.cc:162-419 -> oracle/brief_pattern.inc and csrc/brief_pattern.inc."""
    ref = _recorded("brief_pattern")
    assert ref["count"] == 1024 and ref["min"] == -13 and ref["max"] <= 13
    for path in ("oracle/brief_pattern.inc", "geoflowslam_amd/csrc/brief_pattern.inc"):
        txt = "\n".join(l for l in _ours(path).splitlines() if not l.lstrip().startswith("//"))
        vals = _ints(txt)
        assert len(vals) == ref["count"] and _digest(vals) == ref["sha256"], path


def _parse_patch():
    hdr = _ref("include/ORBextractor.h")
    ref = {k: _one(rf"static const int {k}\s*=\s*(\d+)\s*;", hdr, int) for k in ("PATCH_SIZE", "HALF_PATCH_SIZE", "EDGE_THRESHOLD")}
    ref["W"] = _one(r"const float W\s*=\s*(\d+)\s*;", _lines(_ref("src/ORBextractor.cc"), 770, 810))
    return ref


def test_patch_and_border_constants():
    """PATCH_SIZE / HALF_PATCH_SIZE / EDGE_THRESHOLD, include/ORBextractor.h:29-31; the FAST cell size W = 35 and the +6 / -3 cell
    arithmetic of ComputeKeyPointsOctTree (src/ORBextractor.cc:778-806)."""
    rec = _recorded("patch")
    ref = {k: rec[k] for k in ("PATCH_SIZE", "HALF_PATCH_SIZE", "EDGE_THRESHOLD")}
    assert ref == dict(PATCH_SIZE=31, HALF_PATCH_SIZE=15, EDGE_THRESHOLD=19) or ref  # (whatever the reference says is the bar)
    orc = _ours("oracle/orb_oracle.cpp")
    for k, v in ref.items():
        assert _one(rf"constexpr int {k}\s*=\s*(\d+)\s*;", orc, int) == v, k
    host = _ours("geoflowslam_amd/csrc/orb_host.hpp")
    for ours, k in (("kPatchSize", "PATCH_SIZE"), ("kHalfPatch", "HALF_PATCH_SIZE"), ("kEdgeThreshold", "EDGE_THRESHOLD")):
        assert _one(rf"constexpr int {ours}\s*=\s*(\d+)\s*;", host, int) == ref[k], ours
    w_ref = rec["W"]
    assert _one(r"const float W\s*=\s*(\d+)\s*;", orc) == w_ref
    assert re.search(rf"\b{int(w_ref)}\b", _ours("geoflowslam_amd/csrc/orb_host.cpp")), "cell size W"


def _parse_orb_settings():
    """(scaleFactor, nLevels, minThFAST) of every example settings file with ORBextractor keys (Examples/**/*.yaml), sorted."""
    import glob
    seen = set()
    for y in glob.glob(os.path.join(REF, "Examples", "**", "*.yaml"), recursive=True):
        t = open(y, errors="replace").read()
        g = {k: re.search(rf"ORBextractor\.{k}:\s*([0-9.]+)", t) for k in ("scaleFactor", "nLevels", "minThFAST")}
        if all(g.values()):
            seen.add((float(g["scaleFactor"].group(1)), int(g["nLevels"].group(1)), int(g["minThFAST"].group(1))))
    return sorted(list(v) for v in seen)


def test_orb_default_parameters_of_the_settings_files():
    """nFeatures / scaleFactor / nLevels / iniThFAST / minThFAST as the RGB-D example settings hold them are what gfs_orb_default_config
    and the oracle's defaults say (reference Examples/**/*.yaml: ORBextractor.* keys)."""
    seen = {tuple(v) for v in _recorded("orb_settings")}
    assert seen, "no settings file with ORBextractor keys in the record"
    assert (1.2, 8, 7) in seen, seen  # the defaults the ABI documents (include/gfs_abi.h gfs_orb_default_config)
    orb = _ours("geoflowslam_amd/csrc/orb.hip")
    assert re.search(r"c->min_th_fast = 7;", orb) and re.search(r"c->nlevels = 8;", orb) and re.search(r"c->scale_factor = 1\.2f;", orb)


# ---------------------------------------------------------------------------------------------- ORBmatcher
def _parse_matcher():
    src = _ref("src/ORBmatcher.cc")
    ref = {k: _one(rf"const int ORBmatcher::{k}\s*=\s*(\d+)\s*;", src, int) for k in ("TH_HIGH", "TH_LOW", "HISTO_LENGTH")}
    fh = _ref("include/Frame.h")
    ref["FRAME_GRID_ROWS"] = _one(r"#define FRAME_GRID_ROWS\s+(\d+)", fh, int)
    ref["FRAME_GRID_COLS"] = _one(r"#define FRAME_GRID_COLS\s+(\d+)", fh, int)
    return ref


def test_matcher_thresholds():
    """ORBmatcher::TH_HIGH / TH_LOW / HISTO_LENGTH, src/ORBmatcher.cc:36-38 -> oracle/sbp_oracle.cpp, csrc/sbp.hip; the frame grid -> csrc/sbp_dev.hpp."""
    ref = _recorded("matcher")
    for path in ("oracle/sbp_oracle.cpp", "geoflowslam_amd/csrc/sbp.hip"):
        t = _ours(path)
        assert _one(r"kHisto\s*=\s*(\d+)", t, int) == ref["HISTO_LENGTH"], path
        assert _one(r"kThHigh\s*=\s*(\d+)", t, int) == ref["TH_HIGH"], path
    # the frame grid the windowed matcher walks (include/Frame.h FRAME_GRID_ROWS / COLS)
    rows, cols = ref["FRAME_GRID_ROWS"], ref["FRAME_GRID_COLS"]
    t = _ours("oracle/sbp_oracle.cpp")
    assert _one(r"kGridCols\s*=\s*(\d+)", t, int) == cols and _one(r"kGridRows\s*=\s*(\d+)", t, int) == rows
    assert re.search(rf"\b{cols}\b", _ours("geoflowslam_amd/csrc/sbp_dev.hpp")) and re.search(rf"\b{rows}\b", _ours("geoflowslam_amd/csrc/sbp_dev.hpp"))


# ---------------------------------------------------------------------------------------------- Optimizer
def _parse_chi2():
    src = _ref("src/Optimizer.cc")
    po = _lines(src, 763, 1100)  # PoseOptimization
    m = re.search(r"const float chi2Mono\[4\]\s*=\s*\{([^}]*)\}", po)
    s = re.search(r"const float chi2Stereo\[4\]\s*=\s*\{([^}]*)\}", po)
    its = re.search(r"const int its\[4\]\s*=\s*\{([^}]*)\}", po)
    lba = _lines(src, 1588, 2040)  # LocalBundleAdjustment
    return dict(deltaMono=_one(r"const float deltaMono\s*=\s*sqrt\(([0-9.]+)\)", po),
                deltaStereo=_one(r"const float deltaStereo\s*=\s*sqrt\(([0-9.]+)\)", po),
                chi2Mono=[float(v) for v in m.group(1).split(",")], chi2Stereo=[float(v) for v in s.group(1).split(",")],
                its=[int(v) for v in its.group(1).split(",")],
                thHuberMono=_one(r"const float thHuberMono\s*=\s*sqrt\(([0-9.]+)\)", lba),
                thHuberStereo=_one(r"const float thHuberStereo\s*=\s*sqrt\(([0-9.]+)\)", lba),
                lba_chi2_gates=sorted({float(v) for v in re.findall(r"e->chi2\(\)\s*>\s*([0-9.]+)", lba)}))


def test_chi2_and_huber_thresholds():
    """deltaMono / deltaStereo (src/Optimizer.cc:807-808), chi2Mono / chi2Stereo / its (:967-970), thHuberMono / thHuberStereo of
    LocalBundleAdjustment (:1753-1754) and its outlier gates (:1972 ff.) -> oracle/pose_oracle.cpp, csrc/pose_lm_dev.hpp, the LBA adaptor."""
    ref = _recorded("chi2")
    d_mono, d_stereo = ref["deltaMono"], ref["deltaStereo"]
    chi_m, chi_s = set(ref["chi2Mono"]), set(ref["chi2Stereo"])
    assert chi_m == {d_mono} and chi_s == {d_stereo} and set(ref["its"]) == {10}
    h_mono, h_stereo = ref["thHuberMono"], ref["thHuberStereo"]
    gates = ref["lba_chi2_gates"]
    assert (h_mono, h_stereo) == (d_mono, d_stereo) and gates == sorted({d_mono, d_stereo})
    # ours
    orc = _ours("oracle/pose_oracle.cpp")
    assert {float(v) for v in re.findall(r"std::sqrt\(([0-9.]+)\)", orc)} >= {d_mono, d_stereo}
    assert _one(r"chi2Mono\s*=\s*([0-9.]+)f", orc) == d_mono and _one(r"chi2Stereo\s*=\s*([0-9.]+)f", orc) == d_stereo
    dev = _ours("geoflowslam_amd/csrc/pose_lm_dev.hpp")  # the one definition both pose kernels use
    assert re.search(rf"\(float\)sqrt\({d_mono}\)", dev) and re.search(rf"\(float\)sqrt\({d_stereo}\)", dev)
    assert re.search(rf"pass \? {d_stereo}f : {d_mono}f", dev)
    for path in ("geoflowslam_amd/csrc/pose.hip", "geoflowslam_amd/csrc/pose_lidar.hip"):
        assert str(d_mono) not in _ours(path) and str(d_stereo) not in _ours(path), path
    ad = _ours("geoflowslam_amd/host/gfs_adaptors.hpp")
    assert re.search(rf"thHuberMono = \(float\)std::sqrt\({d_mono}\)", ad) and re.search(rf"thHuberStereo = \(float\)std::sqrt\({d_stereo}\)", ad)
    assert re.search(rf"chi2\[e\] > {d_mono} ", ad) and re.search(rf"chi2\[e\] > {d_stereo} ", ad)
    # the ABI documents rounds / iterations of PoseOptimization
    assert re.search(r"n_rounds;\s*/\* 4 \*/", _ours("include/gfs_abi.h")) and re.search(r"its;\s*/\* 10 ", _ours("include/gfs_abi.h"))


# ---------------------------------------------------------------------------------------------- RegistrationGICP / small_gicp
def _default_cfg(libpath, fn, fields):
    class Cfg(C.Structure):
        _fields_ = fields
    L = C.CDLL(libpath)
    c = Cfg()
    getattr(L, fn)(C.byref(c))
    return c


GICP_FIELDS = [("num_threads", C.c_int32), ("downsampling_resolution", C.c_double), ("max_correspondence_distance", C.c_double),
               ("rotation_eps", C.c_double), ("translation_eps", C.c_double), ("max_iterations", C.c_int32), ("num_neighbors", C.c_int32)]


def _parse_gicp():
    reg = _ref("src/RegistrationGICP.cc")
    ref = dict(num_threads=_one(r"setting\.num_threads\s*=\s*(\d+)", reg, int),
               downsampling_resolution=_one(r"setting\.downsampling_resolution\s*=\s*([0-9.]+)", reg),
               max_correspondence_distance=_one(r"setting\.max_correspondence_distance\s*=\s*([0-9.]+)", reg))
    sg = "Thirdparty/small_gicp/include/small_gicp/registration/"
    tc = _ref(sg + "termination_criteria.hpp")
    m = re.search(r"TerminationCriteria\(\)\s*:\s*translation_eps\(([0-9.e+-]+)\),\s*rotation_eps\(([0-9.]+) \* M_PI / ([0-9.]+)\)", tc)
    assert m
    ref["translation_eps"], ref["rotation_eps"] = float(m.group(1)), float(m.group(2)) * math.pi / float(m.group(3))
    rh = _ref(sg + "registration_helper.hpp")
    assert _one(r"double rotation_eps\s*=\s*([0-9.]+) \* M_PI / 180\.0", rh) * math.pi / 180.0 == ref["rotation_eps"]
    assert _one(r"double translation_eps\s*=\s*([0-9.e+-]+);", rh) == ref["translation_eps"]
    ref["max_iterations"] = _one(r"int max_iterations\s*=\s*(\d+);", rh, int)
    ref["num_neighbors"] = _one(r"double downsampling_resolution, int num_neighbors = (\d+)", rh, int)
    op = _ref(sg + "optimizer.hpp")
    lm = re.search(r"LevenbergMarquardtOptimizer\(\)\s*:\s*verbose\(false\),\s*max_iterations\((\d+)\),\s*max_inner_iterations\((\d+)\),\s*init_lambda\(([0-9.e+-]+)\),\s*lambda_factor\(([0-9.]+)\)", op)
    assert lm and int(lm.group(1)) == ref["max_iterations"]
    # CovarianceSetter's regularisation (util/normal_estimation.hpp: values 1e-3, 1, 1)
    ne = _ref("Thirdparty/small_gicp/include/small_gicp/util/normal_estimation.hpp")
    assert re.search(r"values\s*=\s*Eigen::Vector3d\(1e-3, 1, 1\)|1e-3, 1\.?0?, 1\.?0?", ne)
    return dict(setting=ref, max_inner_iterations=int(lm.group(2)), init_lambda=float(lm.group(3)), lambda_factor=float(lm.group(4)),
                covariance_regularisation=[1e-3, 1.0, 1.0])


def test_registration_settings_and_termination_criteria():
    """RegistrationGICP::RegisterPointClouds' settings (src/RegistrationGICP.cc:9-15), RegistrationSetting's defaults
    (registration_helper.hpp:42-47), TerminationCriteria (termination_criteria.hpp:12), the LM constants (optimizer.hpp:72) and
    preprocess_points' num_neighbors default (registration_helper.hpp:20) against gfs_gicp_default_config and gfso_gicp_default_cfg, CALLED."""
    rec = _recorded("gicp")
    ref = rec["setting"]
    max_inner, init_lambda, lambda_factor = rec["max_inner_iterations"], rec["init_lambda"], rec["lambda_factor"]
    for libpath, fn in ((os.path.join(ROOT, "geoflowslam_amd", "libgfs_hip.so"), "gfs_gicp_default_config"),
                        (os.path.join(ROOT, "oracle", "libgfs_oracle.so"), "gfso_gicp_default_cfg")):
        if not os.path.exists(libpath):
            pytest.skip(f"{libpath} not built")
        c = _default_cfg(libpath, fn, GICP_FIELDS)
        got = {k: getattr(c, k) for k, _ in GICP_FIELDS}
        assert got == ref, (fn, got, ref)
    # the LM constants are literals of the state machine (csrc/gicp.hip) and of the oracle's loop
    dev, orc = _ours("geoflowslam_amd/csrc/gicp.hip"), _ours("oracle/gicp_oracle.cpp")
    assert _one(r"S\.lambda = ([0-9.e+-]+);\s*// init_lambda", dev) == init_lambda
    assert {float(v) for v in re.findall(r"S\.lambda /= ([0-9.]+);", dev)} == {lambda_factor}
    assert {float(v) for v in re.findall(r"S\.lambda \*= ([0-9.]+);", dev)} == {lambda_factor}
    assert {int(v) for v in re.findall(r"S\.inner >= (\d+)\)", dev)} == {max_inner}
    m = re.search(r"const double init_lambda = ([0-9.e+-]+), lambda_factor = ([0-9.]+);", orc)
    assert m and float(m.group(1)) == init_lambda and float(m.group(2)) == lambda_factor
    assert re.search(rf"j < {max_inner}\b|max_inner_iterations = {max_inner}\b|< {max_inner}; j\+\+", orc), "max_inner_iterations in the oracle"
    # CovarianceSetter's regularisation (util/normal_estimation.hpp: values 1e-3, 1, 1)
    assert rec["covariance_regularisation"] == [1e-3, 1.0, 1.0]
    assert re.search(r"values\[3\] = \{1e-3, 1\.0, 1\.0\}", orc)


def _parse_voxel():
    so = _ref("Thirdparty/small_gicp/include/small_gicp/util/sort_omp.hpp")
    ds = _ref("Thirdparty/small_gicp/include/small_gicp/util/downsampling_omp.hpp")
    bits = _one(r"constexpr int coord_bit_size = (\d+);", ds, int)
    mask_bits = _one(r"constexpr size_t coord_bit_mask = \(1 << (\d+)\) - 1;", ds, int)
    assert re.search(r"constexpr int coord_offset = 1 << \(coord_bit_size - 1\);", ds) and mask_bits == bits
    return dict(sort_serial_cutoff=_one(r"if \(n < (\d+)\)", so, int), block_size=_one(r"const int block_size = (\d+);", ds, int),
                coord_bit_size=bits)


def test_voxel_sort_block_and_key_layout():
    """util/sort_omp.hpp's 1024-element serial cutoff, downsampling_omp.hpp's 1024-point blocks, the 21-bit coordinate fields and the
    coordinate offset of the voxel key -> csrc/voxel_qsort.hpp / gicp.hip and the oracle."""
    rec = _recorded("voxel")
    cutoff, block, bits = rec["sort_serial_cutoff"], rec["block_size"], rec["coord_bit_size"]
    dev = _ours("geoflowslam_amd/csrc/gicp.hip")
    assert _one(r"constexpr int kCoordBits\s*=\s*(\d+);", dev, int) == bits
    assert re.search(r"constexpr int kCoordOffset = 1 << \(kCoordBits - 1\);", dev) and re.search(r"constexpr int kCoordMask = \(1 << kCoordBits\) - 1;", dev)
    orc = _ours("oracle/gicp_oracle.cpp")
    assert _one(r"constexpr int coord_bit_size = (\d+);", orc, int) == bits
    assert str(cutoff) in re.findall(r"if \(n < (\d+)\)", orc)  # (the restatement of quick_sort_omp; the other `n <` is the neighbour count)
    assert re.search(rf"block_size = {block}\b|\b{block}\b", orc)
    assert re.search(rf"\b{cutoff}\b", _ours("geoflowslam_amd/csrc/voxel_qsort.hpp"))


# ---------------------------------------------------------------------------------------------- GMS
def _parse_gms():
    g = _ref("Thirdparty/GMS/include/gms_matcher.h")
    pat = _ints(re.search(r"const int mRotationPatterns\[8\]\[9\]\s*=\s*\{(.*?)\};", g, re.S).group(1))
    gw, gh = re.search(r"mGridSizeLeft = Size\((\d+), (\d+)\);", g).groups()
    assert re.search(r"NB9\[xi \+ 4 \+ yi \* 3\] = idx_xx \+ idx_yy \* GridSize\.width;", g)
    return dict(THRESH_FACTOR=_one(r"#define THRESH_FACTOR (\d+)", g, int), rotation_patterns_count=len(pat),
                rotation_pattern_1=pat[:9], grid=[int(gw), int(gh)])


def test_gms_tables():
    """THRESH_FACTOR, the rotation patterns (only pattern 1, the identity, is used by GetInlierMask(mask, false, false)), the 20 x 20
    grid and GetNB9's index arithmetic, Thirdparty/GMS/include/gms_matcher.h:4-48, 187-206."""
    rec = _recorded("gms")
    tf, (gw, gh) = rec["THRESH_FACTOR"], rec["grid"]
    # pattern 1 = identity: neighbour j of the left cell <-> neighbour j of the right
    assert rec["rotation_patterns_count"] == 72 and rec["rotation_pattern_1"] == [1, 2, 3, 4, 5, 6, 7, 8, 9]
    orc = _ours("oracle/gms_oracle.cpp")
    assert _one(r"kThreshFactor\s*=\s*(\d+)", orc, int) == tf
    assert _one(r"kGridW\s*=\s*(\d+)", orc, int) == int(gw) and _one(r"kGridH\s*=\s*(\d+)", orc, int) == int(gh)
    assert re.search(r"out\[xi \+ 4 \+ yi \* 3\] = xx \+ yy \* kGridW;", orc)
    dev = _ours("geoflowslam_amd/csrc/gms.hip")
    assert re.search(rf"thresh = {tf} \* sqrt\(thresh / numpair\);", dev)
    assert re.search(rf"\b{int(gw)}\b", dev)


PARSERS = dict(brief_pattern=_parse_brief_pattern, patch=_parse_patch, orb_settings=_parse_orb_settings, matcher=_parse_matcher,
               chi2=_parse_chi2, gicp=_parse_gicp, voxel=_parse_voxel, gms=_parse_gms)


if __name__ == "__main__":
    assert _have_ref(), f"no reference tree at {REF}"
    with open(GOLDEN, "w") as f:
        json.dump({k: p() for k, p in PARSERS.items()}, f, indent=1)
        f.write("\n")
    print(f"wrote {GOLDEN}")
