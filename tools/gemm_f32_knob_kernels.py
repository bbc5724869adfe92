"""Which fp32 GEMM kernel each setting of dvt_tune_set keys 0, 4 and 5 selects: one tiny call per tile family and setting.

For every k-depth (key 5 = 16, 32, 64) and, at that depth, every value of key 0 (-1 .. 3) and of key 4 (0, 1, 2, 3, 10, 11),
three calls that launch ONE kernel each, in this order:
  fit     dvt_linear_fwd            64 x 64 x 64     (csrc/dvt_gemm_f32.hip; the ring when key 5 = 64, key 4 != 0, key 0 <= 0)
  big     dvt_parts_linear_big_epi  128 x 128 x 64   (csrc/dvt_gemm_f32_big.hip; the ring of key 4's depth when key 4 = 10)
  ring    dvt_parts_gemm_ex         64 x 64 x 64     (csrc/dvt_gemm_f32_glds.hip)
and the knobs back at their defaults after each setting.  Prints the settings in launch order; run it under
`rocprofv3 --kernel-trace -- python tools/gemm_f32_knob_kernels.py` and read the trace three kernels per printed line
(tools/gemm_f32_knob_kernels.py --table TRACE.csv does that)."""
import csv
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "denoising-vit_amd"))

DEFAULTS = {0: -1, 4: (1, 2, 11), 5: 32}
SETTINGS = [(bk, key, v) for bk in (16, 32, 64) for key, vals in ((0, (-1, 0, 1, 2, 3)), (4, (0, 1, 2, 3, 10, 11))) for v in vals]


def label(bk, key, v):
    return f"5={bk} {key}={v}"


def run():
    import torch
    from dvt_amd import _lib
    L = _lib.lib()
    s = torch.cuda.current_stream().cuda_stream
    x, w, y = torch.randn(128, 64, device="cuda"), torch.randn(128, 64, device="cuda"), torch.empty(128, 128, device="cuda")
    for bk, key, v in SETTINGS:
        try:
            assert L.dvt_tune_set(5, bk) == 0 and L.dvt_tune_set(key, v) == 0
            assert L.dvt_linear_fwd(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), 64, 64, 64, 0, s) == 0
            assert L.dvt_parts_linear_big_epi(x.data_ptr(), w.data_ptr(), None, y.data_ptr(), 128, 128, 64, 0, None, s) == 0
            g = _lib.PartsGemmEx(layout=0, A=x.data_ptr(), B=w.data_ptr(), C=y.data_ptr(), M=64, N=64, K=64, lda=64, ldb=64, ldc=64)
            assert L.dvt_parts_gemm_ex(C.byref(g), s) == 0
            torch.cuda.synchronize()
        finally:
            L.dvt_tune_set(0, DEFAULTS[0])
            L.dvt_tune_set(5, DEFAULTS[5])
            for d in DEFAULTS[4]:
                L.dvt_tune_set(4, d)
        print(label(bk, key, v), flush=True)


def table(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows if "gemm_f32" in r["Kernel_Name"]]
    assert len(names) == 3 * len(SETTINGS), (len(names), len(SETTINGS))
    for i, (bk, key, v) in enumerate(SETTINGS):
        fit, big, ring = (n.replace("void ", "").replace("(anonymous namespace)::", "").split("(")[0] for n in names[3 * i:3 * i + 3])
        print(f"{label(bk, key, v):12s} fit {fit:52s} big {big:44s} ring {ring}")


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--table":
        table(sys.argv[2])
    else:
        run()
