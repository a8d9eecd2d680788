"""Case table and helpers of the ORB edge-geometry tests (tests/test_orb_geometry_reference.py on the CPU, tests/test_gpu_orb_geometry.py
on the GPU): image sizes, feature counts and level counts at which csrc/orb.hip and csrc/orb_host.cpp take a path that 640 x 480 with
1000 features never takes.  Every row says what it is there for; the CPU file asserts that property on the oracle and on the host
hook gfs_test_orb_geometry, the GPU file compares the extraction with the oracle bit for bit and asserts the path.

Images are synth.noise_image(SEED + i, W, H); with SEED = 1 every row has key points on all its levels (asserted on the CPU).  One row
of a group is also run on synth.frame_pair(SEED, W, H, 4)["gray0"], a rendered scene."""
import numpy as np

from geoflowslam_amd import synth

SEED = 1
SCALE = 1.2
INI_TH, MIN_TH = 20, 7
OCT_MAX_NODES = 768  # kOctMaxNodes (csrc/orb_host.hpp)
ERR_CAPACITY, ERR_UNSUPPORTED = -4, -5  # GFS_ERR_* (include/gfs_abi.h)


def _case(key, group, w, h, nf, nl, what, **kw):
    return dict(dict(key=key, group=group, w=w, h=h, nf=nf, nl=nl, what=what, rendered=False, octree="device"), **kw)


# rendered: also run on the rendered scene.  octree: the quadtree the call must end on.  The remaining keys are the row's property.
CASES = [
    _case("a241", "a", 241, 241, 300, 8, "levels 5..7 are one cell each; level 7 is 67 x 67 with one 35 x 35 cell, the smallest build takes",
          one_cell_levels=(5, 6, 7), top_level=(67, 67, 35, 35), rendered=True),
    _case("a240", "a", 240, 240, 300, 8, "level 7 rounds up to the same 67", one_cell_levels=(5, 6, 7), top_level=(67, 67, 35, 35)),
    _case("b68", "b", 68, 68, 50, 1, "nlevels = 1: one cell in the frame, two blur-tile columns, the second 4 pixels wide",
          one_cell_levels=(0,), blur_tile_cols=2, last_tile_w=4, rendered=True),
    _case("b67", "b", 67, 67, 50, 1, "nlevels = 1: the second blur-tile column 3 pixels wide", one_cell_levels=(0,), blur_tile_cols=2,
          last_tile_w=3),
    _case("b640", "b", 640, 480, 1000, 1, "nlevels = 1 with quota 1000 > 768: the host quadtree", octree="host", quotas=(1000,),
          device_levels=(False,)),
    _case("c82", "c", 82, 81, 60, 2, "two one-cell levels", one_cell_levels=(0, 1), rendered=True),
    _case("c100", "c", 100, 90, 100, 2, "one 68 x 58 cell: the widest cell and the largest fast_lds_wave of this table", one_cell_levels=(0, 1),
          widest_cell=(68, 58)),
    _case("d150", "d", 640, 150, 500, 4, "nIni 5, 5, 6, 6: every level outside k_octree, the fallback is automatic", octree="host",
          n_ini=(5, 5, 6, 6), device_levels=(False,) * 4, rendered=True),
    _case("d4000", "d", 640, 480, 4000, 8, "only level 0 (quota 869) is outside; the whole call goes to the host", octree="host",
          quota0=869, device_levels=(False,) + (True,) * 7),
    _case("d3400", "d", 640, 480, 3400, 8, "level-0 quota 738: 738 + 4 + 8 = 750 <= 768, the largest count on the device", quota0=738,
          device_levels=(True,) * 8),
    _case("e150", "e", 150, 640, 500, 4, "portrait: nIni rounds to 0, is set to 1, and runs on the device", n_ini=(1, 1, 1, 1),
          raw_aspect_rounds_to_zero=True, device_levels=(True,) * 4, rendered=True),
    _case("f1241", "f", 1241, 376, 2000, 8, "nIni = 4 on every level: the widest image the device quadtree takes; x tables of the coarse cut in memory",
          n_ini=(4,) * 8, device_levels=(True,) * 8, xtab_in_lds=0, rendered=True),
    _case("g8", "g", 640, 480, 8, 8, "quotas 2,1,1,1,1,1,1,0; the oracle keeps 4 key points a level (the first sweep runs before the stop test)",
          quotas=(2, 1, 1, 1, 1, 1, 1, 0), kept_per_level=4, device_levels=(True,) * 8, rendered=True),
    _case("g1", "g", 640, 480, 1, 8, "quotas 0 on levels 0..6 and 1 on level 7", quotas=(0,) * 7 + (1,), kept_per_level=4,
          device_levels=(True,) * 8),
]
CASE = {c["key"]: c for c in CASES}

# case h, the lapping area: 320 x 240, 6 levels, 500 features
LAP = dict(w=320, h=240, nf=500, nl=6)
# kp_cap (OrbGeometry::build: the sum over levels of quota + 3 + 4 nIni) of 1000 features, 8 levels: what the capacity rule compares
KP_CAP = {(640, 480): 1056, (320, 240): 1068, (640, 300): 1100}


def image(c, i=0, rendered=False):
    """Frame i of a row: the noise image of seed SEED + i, or the rendered scene."""
    if rendered:
        return np.ascontiguousarray(synth.frame_pair(SEED + i, c["w"], c["h"], 4)["gray0"])
    return synth.noise_image(SEED + i, c["w"], c["h"])


def make_oracle(O, c):
    return O.OrbOracle(c["nf"], SCALE, c["nl"], INI_TH, MIN_TH)


def make_extractor(api, c, max_batch=1):
    return api.ORBextractor(c["nf"], SCALE, c["nl"], INI_TH, MIN_TH, max_rows=c["h"], max_cols=c["w"], max_batch=max_batch)


def level_counts(orc, nl):
    return [len(orc.level_keypoints(l)) for l in range(nl)]


def n_ini_raw(width, height):
    """round(width / height) of a level's border box as DistributeOctTree computes it (float division, half away from zero) -- BEFORE
    the reference sets a 0 to 1."""
    q = np.float32(width) / np.float32(height)
    return int(np.floor(q + np.float32(0.5)))


def lap_probes(orc, img, nl):
    """The lapping areas of case h for one image: a list of (name, lap, others) -- `lap` holds a key point exactly on an inclusive bound,
    every lap of `others` is one integer off at that bound and must sort at least one key point into the other block.
    Level 0 compares x itself, a level >= 1 compares the float32 product x * mvScaleFactor[level] (src/ORBextractor.cc:1198-1215)."""
    scale = orc.tables()["scale"]
    orc.extract(img)
    lv = [orc.level_keypoints(l) for l in range(nl)]
    probes = [("all stereo", (-10, 1000), []), ("empty interval", (300, 100), [])]
    x0 = int(lv[0]["x"][len(lv[0]) // 2])  # a level-0 key point (level coordinates = image coordinates)
    probes.append(("lap0 = lap1 = x of a level-0 key point", (x0, x0), [(x0 + 1, x0), (x0, x0 - 1)]))
    exact = None
    for l in range(1, nl):
        prod = lv[l]["x"].astype(np.float32) * np.float32(scale[l])  # level_keypoints are in level coordinates
        hit = np.nonzero(prod == np.floor(prod))[0]
        if len(hit):
            exact = int(prod[hit[len(hit) // 2]])
            break
    if exact is not None:
        probes.append(("lap1 = x * scale of a level >= 1 key point, an exact integer", (-10, exact), [(-10, exact - 1)]))
        probes.append(("lap0 = x * scale of a level >= 1 key point, an exact integer", (exact, 1000), [(exact + 1, 1000)]))
    else:
        prod = float(np.float32(lv[1]["x"][0]) * np.float32(scale[1]))
        lo, hi = int(np.floor(prod)), int(np.ceil(prod))
        probes.append(("lap1 on either side of x * scale of a level-1 key point", (-10, hi), [(-10, lo)]))
        probes.append(("lap0 on either side of x * scale of a level-1 key point", (lo, 1000), [(hi, 1000)]))
    return probes, exact is not None


class BatchFrame:
    """What _compare_full (tests/test_gpu_orb_match.py) asks of an extractor, bound to frame b of the batch the handle ran last: the
    call returns that frame's result, level() and candidates() read that frame."""

    def __init__(self, ext, b, result=None):
        self.ext, self.b, self.nlevels, self.result = ext, b, ext.nlevels, result

    def __call__(self, img, lap=(0, 0)):
        return self.result if self.result is not None else self.ext.fetch(self.b)

    def level(self, l, blurred=False):
        return self.ext.level(l, b=self.b, blurred=blurred)

    def candidates(self, l):
        return self.ext.candidates(l, b=self.b)
