"""CPU: the host side of the tapped extractor forward -- the three entry points and their struct mirror, the tap-list check
(every refusal comes back as DVT_E_BADARG with poisoned device pointers in the call: nothing is touched before the check),
the index arithmetic of PretrainedViTWrapper.get_intermediate_layers on a stubbed engine, and the Denoiser's assert."""
import ctypes as C
import warnings

import pytest
import torch

BADARG = -1
POISON = 0xDEAD0000DEAD0000  # a pointer no process owns: a call that reads or launches on it cannot return a clean code
ENTRIES = ("dvt_vit_forward_taps", "dvt_vit_forward_f32_taps", "dvt_vit_forward_f32x3_taps")


@pytest.fixture(scope="module")
def L(built_lib):
    import dvt_amd.vit  # noqa: F401 registers signatures
    return built_lib


def test_symbols_and_struct_size(L):
    from dvt_amd.vit import DVT_VIT_MAX_TAPS, VitTaps
    for name in ENTRIES:
        assert hasattr(L, name)
    assert DVT_VIT_MAX_TAPS >= 8
    assert int(L.dvt_vit_taps_struct_size()) == C.sizeof(VitTaps) == 8 + DVT_VIT_MAX_TAPS * (4 + 8 + 8)


def make_taps(blocks, n_taps=None, feat=POISON, prefix=None, norm=1):
    from dvt_amd.vit import VitTaps
    t = VitTaps()
    t.n_taps, t.norm = len(blocks) if n_taps is None else n_taps, norm
    for i, b in enumerate(blocks):
        t.block[i], t.feat[i], t.prefix[i] = b, feat, prefix
    return t


@pytest.mark.parametrize("entry", ENTRIES)
def test_bad_tap_lists_are_refused_before_any_pointer_is_touched(L, entry):
    from dvt_amd.vit import DVT_VIT_MAX_TAPS, VitWeights, vit_config
    cfg = vit_config(384, 12, 14, 14, 56, 56)  # (s_pad 128: a config all three arithmetics take)
    w = VitWeights()
    fn = getattr(L, entry)

    def call(taps, c=cfg, batch=2):
        return fn(C.byref(c), C.byref(w), POISON, C.byref(taps) if taps is not None else None, batch, POISON, None)

    bad = {
        "no list": None,
        "empty": make_taps([]),
        "negative count": make_taps([1], n_taps=-1),
        "too long": make_taps(list(range(DVT_VIT_MAX_TAPS)), n_taps=DVT_VIT_MAX_TAPS + 1),
        "unsorted": make_taps([2, 1]),
        "duplicate": make_taps([1, 1]),
        "duplicate behind a good pair": make_taps([0, 3, 3]),
        "at depth": make_taps([3, 12]),
        "negative index": make_taps([-1, 2]),
        "NULL feat": make_taps([1, 2], feat=None),
    }
    for what, taps in bad.items():
        assert call(taps) == BADARG, what
    # a prefix output where the config has no prefix rows
    c0 = vit_config(384, 12, 14, 14, 56, 56)
    c0.n_prefix, c0.n_tokens = 0, c0.grid_h * c0.grid_w
    assert call(make_taps([1], prefix=POISON), c=c0) == BADARG
    # what the plain forward refuses, with its code: no images, a NULL config, a config it does not take
    assert call(make_taps([1, 2]), batch=0) == BADARG
    assert fn(None, C.byref(w), POISON, C.byref(make_taps([1])), 2, POISON, None) == BADARG
    odd = vit_config(384, 12, 14, 14, 56, 56)
    odd.heads = 5
    assert call(make_taps([1, 2]), c=odd) == BADARG


class StubEngine:
    """Stands for HipViT: records every forward_taps call and returns maps filled with their block index."""

    def __init__(self, gh=2, gw=3, dim=384, n_prefix=1):
        self.calls, self.shape, self.n_prefix = [], (gh, gw, dim), n_prefix

    def forward_taps(self, img, blocks, norm=True, return_prefix=False, outs=None, max_batch=128):
        self.calls.append((list(blocks), norm, return_prefix))
        B = img.shape[0]
        maps = [torch.full((B, *self.shape), float(b)) for b in blocks]
        if not return_prefix:
            return maps
        return [(m, torch.full((B, self.n_prefix, self.shape[2]), float(b) + 0.5)) for m, b in zip(maps, blocks)]


@pytest.fixture(scope="module")
def wrapper():
    from dvt_amd.models import PretrainedViTWrapper
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        w = PretrainedViTWrapper("vit_small_patch14_dinov2.lvd142m", stride=14, img_size=56, allow_random_init=True)
    assert w.num_blocks == 12
    return w


def test_index_normalisation_runs_one_forward(wrapper, monkeypatch):
    x = torch.zeros(2, 3, 56, 56)
    eng = StubEngine()
    monkeypatch.setattr(wrapper, "_engine", lambda *a, **k: eng)

    assert wrapper.tap_indices(3) == ([9, 10, 11], [9, 10, 11])
    out = wrapper.get_intermediate_layers(x, n=3)
    assert eng.calls == [([9, 10, 11], True, False)]
    assert [float(o.flatten()[0]) for o in out] == [9.0, 10.0, 11.0]
    assert all(o.shape == (2, 384, 2, 3) for o in out)  # NCHW views of the NHWC maps

    eng.calls.clear()
    out = wrapper.get_intermediate_layers(x, n=[-1, 2], reshape=False, norm=False)
    assert eng.calls == [([2, 11], False, False)], "taps are unique and ascending, one forward"
    assert [float(o.flatten()[0]) for o in out] == [11.0, 2.0], "results come back in the order of n"
    assert all(o.shape == (2, 6, 384) for o in out)

    eng.calls.clear()
    out = wrapper.get_intermediate_layers(x, n=[5, 5])
    assert eng.calls == [([5], True, False)]
    assert len(out) == 2 and out[0] is out[1], "a repeated index is the same tensor"

    eng.calls.clear()
    out = wrapper.get_intermediate_layers(x, n=(11, 0, 11), return_prefix_tokens=True)
    assert eng.calls == [([0, 11], True, True)]
    assert [(float(f.flatten()[0]), float(p.flatten()[0])) for f, p in out] == [(11.0, 11.5), (0.0, 0.5), (11.0, 11.5)]
    assert out[0][0] is out[2][0] and out[0][1] is out[2][1] and out[0][1].shape == (2, 1, 384)

    for bad in (0, 13, [12], [-13], []):
        with pytest.raises(ValueError):
            wrapper.get_intermediate_layers(x, n=bad)


def test_denoiser_without_a_vit_has_no_class_token():
    """Denoiser(vit=None).forward(x, return_class_token=True) fails like the reference's assert; the module is built
    without its device engine (there is no GPU here), which the assert does not need."""
    from dvt_amd.models import Denoiser
    d = Denoiser.__new__(Denoiser)
    torch.nn.Module.__init__(d)
    d.vit = None
    with pytest.raises(AssertionError):
        d.forward(torch.zeros(1, 2, 2, 8), return_class_token=True)


@pytest.mark.parametrize("layout", ["dinov2", "reg4-swiglu", "deit3", "dino-stride"])
def test_reference_is_the_backbone_tests_reference_stopped_early(layout):
    """tests/taps_reference.py against the two float64 restatements the backbone tests use: the final LayerNorm of its rows
    after block b is their forward_features(n_blocks = b + 1), patch rows and cls row, in float64 and in the bf16 class."""
    from dvt_amd.vit import random_state_dict
    from tests import backbone_reference as bref
    from tests import taps_reference as tref
    from tests import vitg_reference as vref
    dim, patch, img, stride = 128, 14, 56, 14
    if layout == "dinov2":
        sd, ref = random_state_dict(dim, 3, patch, 17, seed=1, well_conditioned=True), vref
    elif layout == "reg4-swiglu":
        sd, ref = random_state_dict(dim, 3, patch, 16, seed=2, well_conditioned=True, n_reg=4, mlp="swiglu"), vref
    elif layout == "deit3":
        patch, img, stride = 16, 64, 16
        sd, ref = random_state_dict(dim, 3, patch, 16, seed=3, well_conditioned=True), bref
    else:
        stride = 7
        sd, ref = random_state_dict(dim, 3, patch, 17, seed=4, well_conditioned=True, layer_scale=False), bref
    x = torch.randn(2, 3, img, img, generator=torch.Generator().manual_seed(5))
    for kw in (dict(), dict(dtype=torch.float32, round_bf16=True)):
        rows, (gh, gw, n_prefix) = tref.residual_rows(sd, x, patch, stride, [0, 2], **kw)
        for b in (0, 2):
            want, want_cls = ref.forward_features(sd, x, patch, stride, n_blocks=b + 1, return_cls=True, **kw)
            got = tref.final_norm(sd, rows[b])
            assert rows[b].shape == (2, n_prefix + gh * gw, dim)
            assert torch.equal(got[:, n_prefix:].reshape(2, gh, gw, dim), want) and torch.equal(got[:, 0], want_cls)
