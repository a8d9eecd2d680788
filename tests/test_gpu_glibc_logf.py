"""The device side of gfs_glibc::logf (csrc/glibc_math.hpp) against the host's libm, bit for bit: 2^24 arguments strided over all
positive floats, and the arguments MapPoint::PredictScale's level boundaries sit on (tests/test_glibc_logf.py checks the same header
compiled for the host on every positive float)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _device(gpu_api, x):
    L = gpu_api.lib()
    x = np.ascontiguousarray(x, np.float32)
    out = np.empty_like(x)
    rc = L.gfs_test_glibc_logf(0, x.ctypes.data, len(x), out.ctypes.data)
    assert rc == 0, L.gfs_last_error()
    return out


def _host(x):
    """libm's logf, element by element through ctypes (small sets)."""
    libm = C.CDLL("libm.so.6")
    libm.logf.restype = C.c_float
    libm.logf.argtypes = [C.c_float]
    return np.fromiter((libm.logf(float(v)) for v in x), np.float32, len(x))


def test_device_logf_strided_over_all_positive_floats(gpu_api, tmp_path):
    # 2^24 bit patterns spread evenly from 1 (the smallest subnormal) to 0x7f7fffff (FLT_MAX), both included
    n = 1 << 24
    bits = (1 + np.arange(n, dtype=np.uint64) * 0x7f7ffffe // (n - 1)).astype(np.uint32)
    assert bits[0] == 1 and bits[-1] == 0x7f7fffff and len(np.unique(bits)) == n
    x = bits.view(np.float32)
    got = _device(gpu_api, x)
    # the host side in C (2^24 ctypes calls would take a minute): a five-line program calling logf, built on demand
    import subprocess
    src = tmp_path / "host_logf.c"
    src.write_text("#include <math.h>\n#include <stdio.h>\n#include <stdlib.h>\nint main(int c, char** v) { FILE* f = fopen(v[1], \"rb\"); "
                   "long n = atol(v[3]); float* x = malloc(4 * n); if (fread(x, 4, n, f) != (size_t)n) return 2; fclose(f); "
                   "for (long i = 0; i < n; i++) { volatile float a = x[i]; x[i] = logf(a); } f = fopen(v[2], \"wb\"); fwrite(x, 4, n, f); "
                   "fclose(f); return 0; }\n")
    exe = tmp_path / "host_logf"
    subprocess.check_call(["gcc", "-O1", "-fno-builtin", str(src), "-o", str(exe), "-lm"])
    x.tofile(tmp_path / "x.bin")
    subprocess.check_call([str(exe), str(tmp_path / "x.bin"), str(tmp_path / "y.bin"), str(n)])
    want = np.fromfile(tmp_path / "y.bin", np.float32)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert len(bad) == 0, [(float(x[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:8]]


def test_device_logf_on_the_level_boundaries(gpu_api):
    f = np.float32
    xs = []
    up, down = f(1), f(1)
    for k in range(21):  # 1.2f^k and 1.2f^-k as float products, each +- 4 ulps
        for c in (up, down):
            b = int(np.array(c, f).view(np.uint32))
            xs += [np.array(b + d, np.uint32).view(f) for d in range(-4, 5)]
        up, down = f(up * f(1.2)), f(down / f(1.2))
    xs += [np.array(b, np.uint32).view(f) for b in (1, 2, 3, 0x7fffff, 0x800000, 0x800001, 0x12345, 0x400000)]  # subnormals and the first normals
    xs += [f(3.4028234663852886e38), f(1.0), f(1.2), f(0.5), f(2.0)]
    x = np.array(xs, f)
    got = _device(gpu_api, x)
    want = _host(x)
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))[0]
    assert len(bad) == 0, [(float(x[i]).hex(), float(got[i]).hex(), float(want[i]).hex()) for i in bad[:8]]
    special = np.array([0.0, np.inf, -1.0, np.nan], f)
    g = _device(gpu_api, special)
    assert g[0] == -np.inf and g[1] == np.inf and np.isnan(g[2]) and np.isnan(g[3])
