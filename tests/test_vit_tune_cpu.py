"""CPU: the decoder of dvt_tune_set(1, v) -- dvt_vit_tune (csrc/dvt_vit.hip) over vit_forward_tune, vit_f32_tune
(csrc/dvt_vit_f32.hip), vit_attn_tune (csrc/dvt_vit_attn.hip) and vit_gemm_tune (csrc/dvt_vit_gemm.hip) -- accepts exactly
the keys written out below and answers DVT_E_BADARG (-1) to every other integer of [-270000, 70000].

The lists are the if-chain of the one-file decoder (dvt_vit_tune before the source was split into units), key by key; the
test passes unedited against a library built from that source.  dvt_tune_set leaves process-global state behind, so the
sweep runs in a fresh child process, which loads the library with ctypes and never touches the GPU.

The developer library (csrc/libdvt_hip_lab.so, -DDVT_LAB) is swept with its own list when it has been built
(`__graft_entry__.build()` builds it); its sweep is ASCENDING from the defaults, because -300 - n answers by the currently
selected GEMM schedule (4 while the sweep passes -398 .. -301: only -300 is accepted there); three schedules are then
selected to see the rest of that key."""
import json
import subprocess
import sys

import pytest

LO, HI = -270000, 70000
BADARG = -1

CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
f = lib.dvt_tune_set
f.restype, f.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
lo, hi = int(sys.argv[2]), int(sys.argv[3])
accepted, other = [], {}
for v in range(lo, hi + 1):
    rc = f(1, v)
    if rc == 0:
        accepted.append(v)
    elif rc != -1:
        other[v] = rc
runs = []  # the accepted set as inclusive runs
for v in accepted:
    if runs and runs[-1][1] == v - 1:
        runs[-1][1] = v
    else:
        runs.append([v, v])
probe = {}
for sched in (6, 5, 4):  # -300 - n under a 4w schedule, under schedule 5, under the default
    rc_s = f(1, sched)
    probe[str(sched)] = [rc_s] + [f(1, -300 - n) for n in range(0, 100)]
print(json.dumps({"runs": runs, "other": other, "probe": probe}))
"""


def runs_of(values):
    out = []
    for v in sorted(set(values)):
        if out and out[-1][1] == v - 1:
            out[-1][1] = v
        else:
            out.append([v, v])
    return out


def span(a, b):
    return list(range(a, b + 1))


# dvt_vit_tune, product build: every key that returns 0
PRODUCT = (
    [-60, -61]                                   # LayerNorm kernels / folded into the GEMMs
    + [-50, -51]                                 # non-temporal bf16 output stores off / on
    + [-70, -71, -72, -74]                       # XCD column sets of the tile order
    + span(-100000 - 65536, -100000)             # ... auto: W bytes per XCD in KiB
    + [-200000 - 128]                            # epilogue cache policy: auto
    + [-200000 - m for m in range(128) if (m & 7) not in (3, 5, 6)]  # ... EPOL_* mask; residual bits: one of them or all
    + span(-572, -570)                           # L2 prefetch of the next workgroup's k-tiles
    + [-530, -531]                               # attention on q as it is / pre-scaled
    + [-520, -521, -522, -523]                   # fp32 extractor, bf16x3 mode
    + [-502, -510 - 15]                          # the one attention kernel / schedule mask the product contains
    + span(-1100, -700)                          # de-synchronised start of the 8p workgroups
    + span(-199, -100)                           # M panels per block of the tile order
    + span(16, HI)                               # L2 group budget in KiB
    + [1, 3, 4]                                  # GEMM schedule
)

# ... developer build: the product's keys (its -502 / -525 as members of the lab's own ranges) and
LAB = PRODUCT + (
    span(-699, -600) + span(-1100 - 65536, -1101)  # the 4w GEMM's grid
    + span(-563, -560)                           # timing-only ablation of the GEMM epilogues
    # schedule mask of the log2-domain attention kernel, -540 - x; x = 128, 1024 ... 32768 fall into the 4w grid's keys
    # above, 256 / 384 / 512 / 514 into -700 - pct: accepted either way
    + [-540 - x for x in (0, 2, 128, 256, 384, 512, 514, 1024, 2048, 4096, 8192, 16384, 32768, 32768 + 65536)]
    + span(-529, -510) + [-510 - 31, -510 - 64, -510 - 79]  # schedule mask of attention_kernel_v2
    + [-501, -502]                               # attention kernel
    + [-300]                                     # ablation / timing build off (others: by schedule, see the probes)
    + span(-299, -200)                           # tiles per workgroup of the 4w kernel
    + span(0, 15)                                # every GEMM schedule
)


def sweep(path):
    r = subprocess.run([sys.executable, "-c", CHILD, str(path), str(LO), str(HI)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_product_tune_keys(built_lib):
    from dvt_amd import _lib
    got = sweep(_lib.LIB_PATH)
    assert got["other"] == {}, "a key answered neither 0 nor DVT_E_BADARG"
    assert got["runs"] == runs_of(PRODUCT)
    # the product library knows no ablation / timing build: -300 - n is DVT_E_BADARG under every schedule it accepts
    assert got["probe"]["6"] == [BADARG] * 101 and got["probe"]["5"] == [BADARG] * 101
    assert got["probe"]["4"] == [0] + [BADARG] * 100


def test_lab_tune_keys():
    from dvt_amd import _lib
    if not _lib.LAB_LIB_PATH.exists():
        pytest.skip("developer library not built (python tools/build_lab.py)")
    got = sweep(_lib.LAB_LIB_PATH)
    assert got["other"] == {}
    assert got["runs"] == runs_of(LAB)
    ok = lambda ns: [0 if n in ns else BADARG for n in range(100)]  # noqa: E731
    assert got["probe"]["6"] == [0] + ok(set(range(0, 99)))       # a 4w schedule: every mask -300 .. -398
    assert got["probe"]["5"] == [0] + ok({0, 3, 6, 7, 8, 9})      # schedule 5: its timing builds
    assert got["probe"]["4"] == [0] + ok({0})                     # any other schedule: off only
