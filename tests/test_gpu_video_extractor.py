"""GPU: the extractor at the video demo's shape -- ViT/14 at stride 4 on 490 x 854: a 120 x 211 token grid, 25 321 tokens
(s_pad 25 344), batch 1 -- against the query-chunked fp32 reference of tests/video_reference.py (pinned to oracle.vit on the
CPU by tests/test_video_cpu.py), with the bars tests/test_gpu_vit.py uses for whole forwards.  Every GPU step runs in a child
process under its own time limit (tests/video_gpu_child.py)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import video_gpu_child as CH
from tests import video_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ((128, 2, 4), (768, 1, 0))  # dim, depth, register tokens


def run_child(args, limit):
    t0 = time.time()
    r = subprocess.run([sys.executable, "-m", "tests.video_gpu_child", *[str(a) for a in args]], cwd=ROOT, timeout=limit,
                       capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-2000:], f"[{time.time() - t0:.1f}s]")
    assert r.returncode == 0, f"child {args} ended with {r.returncode}"


@pytest.fixture(scope="module")
def references(built_lib):
    cache = {}

    def get(case):
        if case not in cache:
            dim, depth, n_reg = case
            sd, img = CH.demo_case(dim, depth, n_reg)
            t0 = time.time()
            chunk = R.q_chunk_for(dim // 64, 1 + n_reg + 120 * 211)
            cache[case] = R.chunked_vit_forward(sd, img, CH.PATCH, CH.STRIDE, q_chunk=chunk)
            print(f"chunked reference {case}: {chunk} queries per chunk, {time.time() - t0:.1f}s on the CPU")
        return cache[case]
    return get


@pytest.mark.parametrize("dtype", ("bfloat16", "float32"))
@pytest.mark.parametrize("case", CASES)
def test_extractor_at_the_demo_shape(references, tmp_path, case, dtype):
    dim, depth, n_reg = case
    out = str(tmp_path / "tokens.npy")
    run_child(("forward", dim, depth, n_reg, dtype, out), 300)
    got, want = torch.from_numpy(np.load(out)), references(case)
    assert tuple(got.shape) == tuple(want.shape) == (1, 120, 211, dim)
    assert bool(torch.isfinite(got).all())
    cos = F.cosine_similarity(got.reshape(-1, dim), want.reshape(-1, dim), dim=-1)
    err = float((got - want).norm() / want.norm())
    print(f"demo shape dim={dim} depth={depth} reg={n_reg} {dtype}: cos mean {cos.mean():.8f} min {cos.min():.8f} rel-L2 {err:.3e}")
    if dtype == "bfloat16":
        assert cos.min() > 0.999 and err < 2e-2
    else:
        assert err < 2e-5 and cos.min() > 0.999999


@pytest.mark.parametrize("dtype", ("bfloat16", "float32"))
def test_wrapper_at_full_depth(built_lib, dtype):
    """PretrainedViTWrapper(stride=4) on 490 x 854, ViT-B/14 at its full depth: [1, 120, 211, 768], finite (no reference)."""
    run_child(("wrapper", dtype), 300)
