"""CPU: the host side of stage 3 at another position grid (dvt_amd.s3 `pos_grid`) -- the two interpolation tables against
the product's own resample, the arena layout with the checkpoint's table, and the refusals of the new C entry points."""
import ctypes as C
import math

import pytest
import torch

# (g0, gh, gw): enlarging, shrinking (10 taps), non-square, a 4-row table, and the two DINOv2 geometries (224 px; stride 7)
SHAPES = [(5, 7, 7), (16, 7, 7), (5, 7, 9), (4, 7, 7), (37, 16, 16), (37, 73, 73)]
U = 2.0 ** -24  # unit roundoff of fp32


def dense(t, g0):
    return torch.eye(g0) if t is None else t


def row_taps(t):
    return 1 if t is None else int((t != 0).sum(1).max())


@pytest.mark.parametrize("g0,gh,gw", SHAPES)
@pytest.mark.parametrize("has_cls", [0, 1])
def test_tables_equal_the_product_resample(g0, gh, gw, has_cls):
    """einsum(Wy, P, Wx) in fp32 against dvt_amd.vit.resample_pos_embed.  Both are fp32 evaluations of the same sum, each
    within (tx + ty + 2) 2^-24 (|Wy| |P| |Wx|^T) of it to first order (tx, ty: the largest tap counts per row), so they
    differ by at most twice that."""
    from dvt_amd import s3
    from dvt_amd.vit import resample_pos_embed
    dim = 48
    wy, wx = s3.pos_tables(g0, gh, gw)
    assert (wy is None) == (gh == g0) and (wx is None) == (gw == g0)
    assert wy is None or tuple(wy.shape) == (gh, g0)
    assert wx is None or tuple(wx.shape) == (gw, g0)
    g = torch.Generator().manual_seed(g0 * 100 + gh + gw)
    pos = torch.randn(1, has_cls + g0 * g0, dim, generator=g) * torch.logspace(-2, 2, dim)
    want = resample_pos_embed(pos, (gh, gw), has_cls)
    P = pos[0, has_cls:].reshape(g0, g0, dim)
    Wy, Wx = dense(wy, g0), dense(wx, g0)
    got = torch.einsum("ip,pjc->ijc", Wy, torch.einsum("jq,pqc->pjc", Wx, P)).reshape(gh * gw, dim)
    tx, ty = row_taps(wx), row_taps(wy)
    assert tx <= (4 if gw >= g0 else 10) and ty <= (4 if gh >= g0 else 10)
    bound = 2 * (tx + ty + 2) * U * torch.einsum("ip,pqc,jq->ijc", Wy.abs().double(), P.abs().double(),
                                                 Wx.abs().double()).reshape(gh * gw, dim)
    err = (got.double() - want[0, has_cls:].double()).abs()
    print(f"tables {g0} -> {gh} x {gw}: taps {tx} / {ty}, worst error / bound {float((err / bound).max()):.2e}")
    assert tuple(want.shape) == (1, has_cls + gh * gw, dim) and bool((err <= bound).all())
    assert torch.equal(want[0, :has_cls], pos[0, :has_cls])


def test_a_kept_axis_is_the_identity():
    from dvt_amd import s3
    assert s3.pos_table(7, 7) is None
    assert s3.pos_tables(7, 7, 9)[0] is None and s3.pos_tables(7, 7, 9)[1] is not None


@pytest.mark.parametrize("n_reg", [0, 4])
def test_layout_keeps_the_checkpoints_table(built_lib, n_reg):
    from dvt_amd import s3
    cfg = s3.make_config(384, 3, 14, 14, 98, 98, n_reg)
    total0, base = s3.param_layout(cfg)
    total, layout = s3.param_layout(cfg, pos_grid=5)
    assert layout["pos_embed"][1] == (1, 25 if n_reg else 26, 384)
    assert base["pos_embed"][1] == (1, 49 if n_reg else 50, 384)
    assert list(layout) == list(base)
    assert all(layout[k][1] == base[k][1] for k in base if k != "pos_embed")
    assert all(o % 4 == 0 for o, _ in layout.values()) and total % 4 == 0
    ends = sorted((o, o + math.prod(s)) for o, s in layout.values())
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= total
    assert total0 - total == 24 * 384
    # the run's own grid through the new entry point is today's layout
    assert s3.param_layout(cfg, pos_grid=7) == (total0, base)
    assert s3.tensor_shapes(cfg, 5)[4] == (1, 25 if n_reg else 26, 384) and s3.tensor_shapes(cfg) == s3.tensor_shapes(cfg, 7)


def test_refusals(built_lib):
    """Every refusal comes back before a pointer is touched: all pointers are null here."""
    from dvt_amd import s3
    L = built_lib
    cfg = s3.make_config(384, 2, 14, 14, 98, 98)  # 7 x 7
    out = (C.c_int64 * (8 + 14 * 2))()
    null = None
    assert L.dvt_s3_param_offsets_pos(C.byref(cfg), 0, out) == -1
    assert L.dvt_s3_param_offsets_pos(C.byref(cfg), 5, None) == -1
    assert L.dvt_s3_param_offsets_pos(C.byref(cfg), 5, out) == 0
    assert L.dvt_s3_workspace_bytes_pos(C.byref(cfg), 1, 0) == -1
    assert L.dvt_s3_workspace_bytes_pos(C.byref(cfg), 0, 5) == -1
    need, same = L.dvt_s3_workspace_bytes_pos(C.byref(cfg), 2, 5), L.dvt_s3_workspace_bytes(C.byref(cfg), 2)
    assert need > same > 0 and L.dvt_s3_workspace_bytes_pos(C.byref(cfg), 2, 7) == same

    def step(c, g0, work_bytes=0):
        return L.dvt_s3_train_slice_pos(C.byref(c), g0, null, null, null, null, null, null, null, 2, 2, null, work_bytes, null,
                                        null)
    assert step(cfg, 0) == -1 and step(cfg, -3) == -1   # g0 < 1
    assert step(cfg, 5) == -1                           # null tables although 5 is not the run's 7
    assert step(cfg, 5, need - 1) == -1                 # a workspace that is too small
    bad = s3.make_config(384, 2, 14, 14, 98, 98)
    bad.dim = 386                                       # dim % 4 != 0
    assert step(bad, 5) == -1 and L.dvt_s3_workspace_bytes_pos(C.byref(bad), 1, 5) == -1
    assert L.dvt_s3_param_offsets_pos(C.byref(bad), 5, out) == -1
    for fn in (L.dvt_pos_resample_fwd, L.dvt_pos_resample_bwd):
        assert fn(null, null, null, null, null, 0, 7, 7, 384, 1, null) == -1   # g0 < 1
        assert fn(null, null, null, null, null, 5, 7, 7, 384, 1, null) == -1   # null tables, 5 -> 7
        assert fn(null, null, null, null, null, 7, 7, 7, 386, 1, null) == -1   # dim % 4 != 0
        assert fn(null, null, null, null, null, 7, 7, 7, 384, 2, null) == -1
        assert fn(null, null, null, null, null, 7, 7, 7, 384, 1, null) == -1   # null maps


def test_load_timm_refuses_by_name(built_lib):
    """The engine needs a HIP device; the message of the refusal is host code and is pinned through a stand-in."""
    from dvt_amd import _lib, s3
    from dvt_amd.vit import random_state_dict

    class Stub(s3.Stage3Engine):
        def __init__(self, cfg, pos_grid):  # the arenas on the CPU: load_timm touches nothing else
            self.cfg, self.pos_grid = cfg, pos_grid
            s3.FlatAdamW.__init__(self, *s3.param_layout(cfg, pos_grid), torch.device("cpu"))

    cfg = s3.make_config(384, 1, 14, 14, 98, 98)
    sd5 = random_state_dict(384, 1, 14, 1 + 25)
    eng = Stub(cfg, 5)
    eng.load_timm(sd5)
    assert torch.equal(eng.state_dict()["pos_embed"], sd5["pos_embed"])
    with pytest.raises(NotImplementedError, match="pos_grid=5"):
        Stub(cfg, None).load_timm(sd5)
    with pytest.raises(NotImplementedError, match="pos_grid=4"):
        eng.load_timm(random_state_dict(384, 1, 14, 1 + 16))
    with pytest.raises(_lib.DvtError, match="not a square grid"):
        eng.load_timm(random_state_dict(384, 1, 14, 1 + 24))


def test_teacher_grid_follows_the_denoiser_checkpoint():
    from dvt_amd import _lib, stage3
    pe = lambda n: {"pos_embed": torch.zeros(1, n, 384)}  # noqa: E731
    assert stage3.teacher_grid(pe(25), 384, 7, 7) == (5, 5)      # the checkpoint's square grid; the run's is served resized
    assert stage3.teacher_grid(pe(63), 384, 7, 9) == (7, 9)      # exactly the run's rows: built there, as before
    assert stage3.teacher_grid({}, 384, 7, 9) == (7, 9)          # no pos_embed: any grid
    with pytest.raises(_lib.DvtError, match="not a square grid"):
        stage3.teacher_grid(pe(24), 384, 7, 7)
    assert stage3.square_grid(1369, "t") == 37
