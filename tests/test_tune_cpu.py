"""CPU: dvt_tune_set(key, value) (csrc/dvt_tune.hip) accepts exactly the (key, value) pairs written out below and answers
DVT_E_BADARG (-1) to every other pair of the sweep: keys -2 .. 24 except 1 (tests/test_vit_tune_cpu.py sweeps that one), values
-70 .. 70 and 4095, 4096, 40960, 65536, INT_MAX, INT_MIN.

The sets are the if-chain of the one-file decoder (dvt_tune_set at the end of csrc/dvt_gemm_f32.hip before the decoders moved
into the units that own the knobs), key by key; the test passes unedited against a library built from that source.  Now
gemm_f32_tune (csrc/dvt_gemm_f32.hip), gemm_f32_big_tune (csrc/dvt_gemm_f32_big.hip), gemm_f32_glds_tune
(csrc/dvt_gemm_f32_glds.hip), fit_tune (csrc/dvt_fit.hip) and fit_fused_tune (csrc/dvt_fit_fused.hip) answer for their own
keys, and keys 2, 3 and 18 go to dvt_grid_tune, dvt_adam_tune and dvt_s2_tune as before.

dvt_tune_set leaves process-global state behind, so the sweep runs in a fresh child process, which loads the library with
ctypes, never touches the GPU, puts every key it touched back to its default and exits."""
import json
import subprocess
import sys

import pytest

INT_MAX, INT_MIN = 2**31 - 1, -2**31
KEYS = [k for k in range(-2, 25) if k != 1]
VALUES = list(range(-70, 71)) + [4095, 4096, 40960, 65536, INT_MAX, INT_MIN]
ANY = VALUES

# every value that returns 0, key by key; a key that is not listed accepts nothing
PRODUCT = {
    0: ANY,           # fp32 GEMM tile override (out-of-range values: no override)
    2: ANY,           # grid backward: -256 / -1024 chunk, other negatives LDS atomics per block, else the level bound
    3: ANY,           # Adam: 10 / 11 the non-temporal hint, else zero-all
    4: ANY,           # fp32 GEMM: 2 / 3 ring depth, 10 / 11 the 128 x 128 tile, every other value the ring off / on
    5: [16, 32, 64],  # k-depth of the register-staged kernel
    6: ANY,           # fused fit step: 2 / 3 its fp32-operand mode, else off / on
    7: ANY,           # sorted grid-corner lists
    8: ANY,           # Adam ping-pong
    9: ANY,           # lazy Adam (n >= 2: refresh interval)
    10: ANY,          # lazy replay arithmetic
    11: ANY,          # merged catch-up
    12: ANY,          # shadow stored by the Adam launch
    13: [0, 1, 2],    # rows per workgroup of the fused row kernel
    14: ANY,          # small workgroups
    16: ANY,          # fit -> XCD map
    18: list(range(0, 64)),  # stage-2 switches
}
LAB = dict(PRODUCT)
LAB[15] = ANY         # developer library only: timing-only ablation mask of the fused fit step

# (key, value) pairs that put every knob back to its default, in this order
DEFAULTS = [(0, -1), (2, 40960), (2, -256), (2, -4096), (3, 0), (3, 10), (4, 1), (4, 2), (4, 11), (5, 32), (6, 1), (6, 3),
            (7, 1), (8, 1), (9, 1), (9, 32), (10, 0), (11, 1), (12, 1), (13, 1), (14, 0), (16, 1), (18, 63)]

CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
f = lib.dvt_tune_set
f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
job = json.loads(sys.stdin.read())
accepted, other = {}, []
for k in job["keys"]:
    for v in job["values"]:
        rc = f(k, v)
        if rc == 0:
            accepted.setdefault(str(k), []).append(v)
        elif rc != -1:
            other.append([k, v, rc])
restored = [f(k, v) for k, v in job["defaults"]]
print(json.dumps({"accepted": accepted, "other": other, "restored": restored}))
"""


def sweep(path, defaults):
    job = json.dumps({"keys": KEYS, "values": VALUES, "defaults": defaults})
    r = subprocess.run([sys.executable, "-c", CHILD, str(path)], input=job, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def check(got, want, defaults):
    assert got["other"] == [], "a pair answered neither 0 nor DVT_E_BADARG"
    for k in KEYS:
        assert got["accepted"].get(str(k), []) == list(want.get(k, [])), f"key {k}"
    assert got["restored"] == [0] * len(defaults)


def test_product_tune_table(built_lib):
    from dvt_amd import _lib
    check(sweep(_lib.LIB_PATH, DEFAULTS), PRODUCT, DEFAULTS)  # key 15 is not in PRODUCT: refused


def test_lab_tune_table():
    from dvt_amd import _lib
    if not _lib.LAB_LIB_PATH.exists():
        pytest.skip("developer library not built (python tools/build_lab.py)")
    defaults = DEFAULTS + [(15, 0)]
    check(sweep(_lib.LAB_LIB_PATH, defaults), LAB, defaults)
