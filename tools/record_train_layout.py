"""Record what the stage-2 and stage-3 trainers answer about their memory layout -- workspace bytes and parameter offsets --
over the table of configurations below: tests/golden/train_layout_parent.json, which tests/test_train_layout_cpu.py holds
every later build to.  A change to how the steps carve their workspace or lay out `params` shows here, without a GPU.

    python tools/record_train_layout.py [--tree PATH_OF_ANOTHER_CHECKOUT] [--out FILE]

`--tree`: ask the library of another checkout of the project (built): the parent commit of a change that must not alter
the layout.  The entry points only compute sizes: the child process loads the library with plain ctypes and never touches
a GPU.

Stage 2: dim 384 / 768 / 1024; tokens 49 / 121 / 1369 (padded to 64 / 128 / 1408); 1 and 2 blocks; enable_pe 0 / 1;
training 0 / 1; batch 1 and 3.  Stage 3: ViT-S / B / L geometry (patch 14) at 98 and 518 pixels; 0 and 4 registers; g0 in
{0, 16, 37}; gemm_mode 0 / 1; batch 1 and 2.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = r"""
import ctypes as C, json, sys
lib = C.CDLL(sys.argv[1])
I, L = C.c_int, C.c_int64


class S2(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dim", "heads", "mlp_dim", "tokens", "tokens_pad", "n_blocks", "enable_pe")] + [
        ("ln_eps", C.c_float)]


class Vit(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("dim", "depth", "heads", "mlp_dim", "patch", "stride", "img_h", "img_w", "grid_h",
                                         "grid_w", "n_tokens", "s_pad", "k_patch", "n_prefix")] + [
        ("ln_eps", C.c_float), ("pos_has_cls", C.c_int32), ("mlp_kind", C.c_int32)]


for name, res, args in (("dvt_s2_workspace_bytes", L, [C.POINTER(S2), I, I]),
                        ("dvt_s2_param_offsets", I, [C.POINTER(S2), C.POINTER(L)]),
                        ("dvt_vit_config_reg", I, [I, I, I, I, I, I, I, C.POINTER(Vit)]),
                        ("dvt_s3_workspace_bytes", L, [C.POINTER(Vit), I]),
                        ("dvt_s3_workspace_bytes_pos", L, [C.POINTER(Vit), I, I]),
                        ("dvt_s3_workspace_bytes_mp", L, [C.POINTER(Vit), I, I, I]),
                        ("dvt_s3_param_offsets", I, [C.POINTER(Vit), C.POINTER(L)]),
                        ("dvt_s3_param_offsets_pos", I, [C.POINTER(Vit), I, C.POINTER(L)])):
    f = getattr(lib, name)
    f.restype, f.argtypes = res, args
out = {}
for dim in (384, 768, 1024):
    for tokens, pad in ((49, 64), (121, 128), (1369, 1408)):
        for blocks in (1, 2):
            for pe in (0, 1):
                c = S2(dim, dim // 64, 4 * dim, tokens, pad, blocks, pe, 1e-6)
                key = f"s2 dim{dim} t{tokens} nb{blocks} pe{pe}"
                o = (L * (2 + 12 * blocks))()
                assert lib.dvt_s2_param_offsets(C.byref(c), o) == 0, key
                out[key + " offsets"] = list(o)
                for training in (0, 1):
                    for batch in (1, 3):
                        out[f"{key} train{training} b{batch} bytes"] = lib.dvt_s2_workspace_bytes(C.byref(c), batch, training)
for tag, dim, depth in (("S", 384, 12), ("B", 768, 12), ("L", 1024, 24)):
    for px in (98, 518):
        for reg in (0, 4):
            c = Vit()
            key = f"s3 vit{tag} px{px} reg{reg}"
            assert lib.dvt_vit_config_reg(dim, depth, 14, 14, px, px, reg, C.byref(c)) == 0, key
            for g0 in (0, 16, 37):
                o = (L * (9 + 14 * depth))()
                rc = lib.dvt_s3_param_offsets_pos(C.byref(c), g0, o) if g0 else lib.dvt_s3_param_offsets(C.byref(c), o)
                assert rc == 0, key
                out[f"{key} g{g0} offsets"] = list(o)
                for batch in (1, 2):
                    if g0:
                        out[f"{key} g{g0} b{batch} bytes_pos"] = lib.dvt_s3_workspace_bytes_pos(C.byref(c), batch, g0)
                    else:
                        out[f"{key} b{batch} bytes"] = lib.dvt_s3_workspace_bytes(C.byref(c), batch)
                    for mode in (0, 1):
                        out[f"{key} g{g0} mode{mode} b{batch} bytes_mp"] = lib.dvt_s3_workspace_bytes_mp(C.byref(c), batch, g0, mode)
print(json.dumps(out))
"""


def layout(lib_path) -> dict:
    """{"<configuration> <what>": bytes or [offsets]} as the library at lib_path answers, asked in a child process."""
    r = subprocess.run([sys.executable, "-c", CHILD, str(lib_path)], capture_output=True, text=True, timeout=120)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "train_layout_parent.json"))
    a = ap.parse_args()
    values = layout(os.path.join(os.path.abspath(a.tree), "denoising-vit_amd", "csrc", "libdvt_hip.so"))
    with open(a.out, "w") as f:
        json.dump({"what": "workspace bytes and parameter offsets of the stage-2 and stage-3 trainers per configuration of "
                           "tools/record_train_layout.py", "values": values}, f, indent=0)
        f.write("\n")
    print(json.dumps({"entries": len(values), "negative": [k for k, v in values.items() if isinstance(v, int) and v < 0]}))


if __name__ == "__main__":
    main()
