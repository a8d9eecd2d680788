"""The constants and comparison operators of Sim3Solver and of its call site (9.210 and the type it is stored in, the defaults of
SetRansacParameters, 0.99 / nBoWInliers / 300 and the iterate(20, ...) step, the >= update and > return tests, the strict inlier
test, RandomInt's formula): tests/golden/sim3_ransac_constants.json holds the reference's values, parsed from the reference itself
when it is on the machine, and is compared with what the rule, the restatement and the adaptor state.  Also: the new entry points are
declared and listed.  No GPU."""
import json
import os
import re

import pytest

import sim3_ransac_support as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "sim3_ransac_constants.json")))


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "src")), reason="the reference sources are not on this machine")
def test_fixture_is_the_reference():
    src = open(os.path.join(REF, "src", "Sim3Solver.cc")).read()
    head = open(os.path.join(REF, "include", "Sim3Solver.h")).read()
    loop = open(os.path.join(REF, "src", "LoopClosing.cc")).read()
    rnd = open(os.path.join(REF, "Thirdparty", "DBoW2", "DUtils", "Random.cpp")).read()
    chi = set(re.findall(r"mvnMaxError[12]\.push_back\(([0-9.]+) \* sigmaSquare[12]\);", src))
    assert len(chi) == 1
    dflt = re.search(r"void SetRansacParameters\(double probability = ([0-9.]+), int minInliers = (\d+),\s+int maxIterations = (\d+)\);", head)
    a = loop.index("bool LoopClosing::DetectCommonRegionsFromBoW(")
    fn = loop[a:loop.index("\n}\n", a)]
    site = re.search(r"solver\.SetRansacParameters\(([0-9.]+), (\w+),\s+(\d+)\);", fn)
    five = src[src.index("bool &bConverge) {"):src.index("Eigen::Matrix4f Sim3Solver::find(")]
    parsed = dict(
        chi2=float(chi.pop()), max_error_type=re.search(r"(std::vector<\w+>) mvnMaxError1;", head).group(1),
        default_probability=float(dflt.group(1)), default_min_inliers=int(dflt.group(2)), default_max_iterations=int(dflt.group(3)),
        call_site_probability=float(site.group(1)), call_site_min_inliers=site.group(2), call_site_max_iterations=int(site.group(3)),
        call_site_step=int(re.search(r"mTcm = solver\.iterate\((\d+), bNoMore, vbInliers, nInliers, bConverge\);", fn).group(1)),
        bow_inliers=int(re.search(r"int nBoWInliers = (\d+);", fn).group(1)),
        update_test=re.search(r"if \((mnInliersi \S+ mnBestInliers)\) \{", five).group(1),
        converge_test=re.search(r"if \((mnInliersi \S+ mRansacMinInliers)\) \{", five).group(1),
        too_few_test=re.search(r"if \((N \S+ mRansacMinInliers)\) \{\s+bNoMore = true;", five).group(1),
        inlier_test=re.search(r"if \((err1 \S+ mvnMaxError1\[i\] && err2 \S+ mvnMaxError2\[i\])\) \{", src).group(1),
        no_more_test=re.search(r"if \((mnIterations \S+ mRansacMaxIts)\) bNoMore = true;", five).group(1),
        random_int=re.search(r"int DUtils::Random::RandomInt\(int min, int max\)\{\s+int d = max - min \+ 1;\s+return (.*?);", rnd).group(1),
        epsilon_type=re.search(r"(\w+) epsilon = \(float\)mRansacMinInliers / N;", src).group(1))
    assert parsed == {k: v for k, v in GOLDEN.items() if k != "source"}
    # the one live call site: the other `iterate` in the tree belongs to the MLPnP solver
    assert len(re.findall(r"Sim3Solver\(", loop)) == 1


def test_constants_in_rule_restatement_and_adaptor():
    g = GOLDEN
    c = S.constants()
    assert c["chi2"] == g["chi2"] and c["default_probability"] == g["default_probability"]
    assert c["default_min_inliers"] == g["default_min_inliers"] and c["default_max_iterations"] == g["default_max_iterations"]
    rule = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "sim3_ransac_rule.hpp")).read()
    assert "return *err1 < max1 && *err2 < max2;" in rule and g["inlier_test"].count("<") == 2 and "<=" not in g["inlier_test"]
    assert "if (c[i] > min_inliers) return Pick{i, i + 1, kConverged};" in rule and g["converge_test"].split()[1] == ">"
    assert "if (c[i] >= best_c) {" in rule and g["update_test"].split()[1] == ">="
    assert "const float epsilon = (float)min_inliers / N;" in rule and g["epsilon_type"] == "float"
    rst = open(os.path.join(ROOT, "tests", "host", "sim3_ransac_restatement.cpp")).read()
    assert "if (sc.count >= mnBestInliers) {" in rst and "if (sc.count > p.min_inliers) {" in rst and "gfs_s3r::pick(" not in rst.split('extern "C"')[1].split("s3rr_pick")[0]
    assert "if (N < p.min_inliers || N < 3) {" in rst and g["too_few_test"] == "N < mRansacMinInliers"
    hip = open(os.path.join(ROOT, "geoflowslam_amd", "csrc", "sim3_ransac.hip")).read()
    assert "if (c > F.min_inliers) first = min(first, h);" in hip and "(p.n_pairs < p.min_inliers || p.n_pairs < 3) ? 0 : p.n_iterations" in hip
    # ---- the adaptor and the call site's numbers
    a = S.adaptor_constants()
    assert a == dict(probability=g["call_site_probability"], max_iterations=g["call_site_max_iterations"], step=g["call_site_step"],
                     bow_inliers=g["bow_inliers"]) and g["call_site_min_inliers"] == "nBoWInliers"
    ada = open(os.path.join(ROOT, "geoflowslam_amd", "host", "gfs_adaptors.hpp")).read()
    cls = ada[ada.index("class Sim3RansacSolver {"):ada.index("class Sim3RansacDevice {")]
    assert g["max_error_type"] == "std::vector<size_t>" and cls.count("(float)(size_t)(gfs_s3r::kChi2 * sigmaSquare") == 2
    assert "if (N < mRansacMinInliers || N < 3 || finished_) {" in cls and "if (mnIterations >= mRansacMaxIts) {" in cls
    assert g["no_more_test"] == "mnIterations >= mRansacMaxIts"
    assert "Access::random_int(0, N - k - 1)" in cls
    harness = open(os.path.join(ROOT, "tests", "host", "sim3_ransac_adaptor_test.cpp")).read()
    assert "return int(((double)stream[stream_at++] / (2147483647.0 + 1.0)) * d) + min;" in harness
    assert g["random_int"] == "int(((double)rand()/((double)RAND_MAX + 1.0)) * d) + min"


def test_entry_points_are_declared_and_listed():
    from geoflowslam_amd import api
    head = open(os.path.join(ROOT, "include", "gfs_abi.h")).read()
    for name in ("gfs_sim3_ransac_iterations", "gfs_sim3_ransac_create", "gfs_sim3_ransac_solve", "gfs_sim3_ransac_destroy"):
        assert name + "(" in head and name in api.ABI_SYMBOLS
    assert [int(v) for v in re.findall(r"#define GFS_SIM3_RANSAC_\w+ (\d)", head)] == [api.SIM3_RANSAC_CONVERGED, api.SIM3_RANSAC_NO_MORE, api.SIM3_RANSAC_TOO_FEW]
