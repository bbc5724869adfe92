"""The stage-1 fit step's gradients, on every path the library ships, element by element against float64.

The observable needs no entry point of its own: with `beta1 = 0` Adam's first moment after a step IS that step's
g' = grad_scale * dloss/dp + wd * p (csrc/dvt_adam.hip: adam1(), within the three roundings of its two fmaf), in the dense
sweep, in the `touched`-gated region and -- because every call ends with a sweep that makes the arena exact -- in the lazy
levels; and with the call's last learning rate set to 0 the parameters that step differentiated at are still in the arena.
The float64 reference, its per-element magnitudes, the two comparators (the same chain at the kernels' precision, CPU) and
the seeded inputs are tests/fit_grads_reference.py; tests/test_fit_grads_cpu.py holds the reference to float64 autograd.

Per stepped tensor (the grid split into the swept and the lazy part), with err_i = |m_i - g'_i| and
scale_i = magnitude_i + |wd p_i|:
    relative L2 error        <= 2 x the comparator's
    max_i err_i / (u scale_i) <= 4 x the comparator's + 4
and m_i == 0 where scale_i == 0; tensors the phase does not step keep p, m, v bit for bit; the gradient arena and the
`touched` bitmap are zero; the five logged losses obey the same two bounds (their magnitudes: the sums of |terms|).

Worst figures per path on one MI355X, GPU error / comparator error (profiles/fit_grads/README.md has them per path with
the tensor each belongs to; the asserted bounds are 2 for the L2 ratio and 1 for max / (4 x comparator + 4)):
    bf16 operands, every single-step path (default, layer-by-layer, atomics grid backward, dense Adam, 16 / 32 rows,
        small workgroups): L2 1.00, max 0.25 -- the kernels reproduce the comparator's roundings to three digits;
        k = 2 / 4 fits, both XCD maps: L2 1.02 / 1.11 (the five losses), max 0.25 / 0.26
    bf16 in-call, 3 and 130 steps, default / (12, 0) / (11, 0): L2 1.29 (losses, C = 768, 3 steps), tensors 1.00; max 0.25
    fp32 operands, every single-step path: L2 1.95 (grid, C = 1024; 1.3 at C = 384, 1.8 at C = 768: the fp32 MFMA rounds its
        accumulator once per product, the comparator once per four -- tests/fit_grads_reference.py has the figures),
        max 0.52 (0.62 for k = 2 / 4)
    fp32 in-call: L2 1.90 (grid[lazy], C = 768, 3 steps) / 1.70 (wh1, C = 768, 130 steps), max 0.76 (grid[lazy], C = 384, 130 steps)
    Adam on the arena: v1 within 3.4 u (bound 5), p1 within 0.8 of its tolerance, every region, both replay arithmetics

What the bf16 cases of 130 steps do NOT constrain: after a hundred steps the residual pred - raw is small against pred, so the
2^-9 the bf16 weight shadow moves F by is a large part of it, and the bf16 comparator's own distance from float64 is
60 to 63 % of the grid and w1 gradients at C = 384 (17 to 21 % at C = 768; 2 to 31 % for the other tensors, 2e-4 for
the loss rows).  Twice 0.6 admits a tensor of zeros, and twice 0.2 a dropped list segment: in those six cases the grid
gradient is held loosely or not at all (the grid-join break below passes them), the MLP tensors and loss rows still are
(the stale-shadow and weight-gradient breaks fail them).  The grid gradient of the same call is held by the fp32 cases,
whose comparator is within 1e-5 of float64, and the bf16 arithmetic by the single-step and 3-step cases.  The break checks
in profiles/fit_grads/README.md show which cases notice what.
"""
import math
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch

from tests import fit_grads_reference as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = R.U

DEFAULT_KNOBS = ((6, 1), (6, 3), (7, 1), (9, 32), (10, 0), (11, 1), (12, 1), (13, 1), (14, 0), (16, 1))
_dev_inputs = {}


def _restore(lib):
    for k, v in DEFAULT_KNOBS:
        lib.dvt_tune_set(k, v)


def _inputs(C, fit):
    """device copies of a case's image, alive for the whole session (kernels in flight read them)"""
    if (C, fit) not in _dev_inputs:
        _, _, feat, xy, _, _ = R.case(C, fit)
        _dev_inputs[C, fit] = (torch.from_numpy(feat).to(DEV), torch.from_numpy(xy).to(DEV))
    return _dev_inputs[C, fit]


def _engine(C, bf16, num_iters, freeze, params, beta1=0.0, warmup=1):
    from dvt_amd.fit import FitEngine, FitSettings
    B, side, V = R.SHAPES[C]
    s = FitSettings(feat_dim=C, noise_map_height=side, noise_map_width=side, n_levels=16, log2_hashmap_size=16,
                    num_iters=num_iters, warmup_iters=warmup, freeze_shared_artifacts_after=freeze, pixel_bsz=B,
                    beta1=beta1, mlp_dtype="bfloat16" if bf16 else "float32")
    eng = FitEngine(s, V * side * side, DEV)
    cfg = R.cfg_of(C)
    lay, n = R.layout(cfg)
    assert n == int(eng.cfg.arena_floats) and all(int(getattr(eng.cfg, "off_" + k)) == o for k, (o, _) in lay.items())
    e0 = R.lazy_first_entry(cfg)
    assert e0 is not None and 0 < e0 < cfg.table.n_entries_total  # dense, hashed and lazy levels are all present
    eng.params.copy_(torch.from_numpy(params))
    return eng


def _stepped_mask(cfg, phase2):
    """bool [arena]: real elements of the tensors the phase steps"""
    lay, n = R.layout(cfg)
    mask = np.zeros(n, bool)
    for name in (R.PHASE2 if phase2 else R.PHASE1):
        o, s = lay[name]
        mask[o:o + math.prod(s)] = True
    return mask


def _idle_ranges(cfg, phase2):
    """[(begin, end)] arena ranges (padding included) of the tensors the phase does not step"""
    lay, n = R.layout(cfg)
    names = list(R.TENSORS)
    out = []
    for i, name in enumerate(names):
        if name not in (R.PHASE2 if phase2 else R.PHASE1):
            out.append((lay[name][0], lay[names[i + 1]][0] if i + 1 < len(names) else n))
    return out


def _check(eng, cfg, phase2, step, want, yard, ref, yard_loss, tag, fails, p_before=None, m_prev=None):
    """All assertions of one fit of one run; failures are collected so that a run reports every tensor."""
    lay, n = R.layout(cfg)
    m = eng.adam_m.cpu().numpy()
    if p_before is not None:
        p = eng.params.cpu().numpy()
        if not np.array_equal(p.view(np.uint32), p_before.view(np.uint32)):
            fails.append(f"{tag}: params changed although the step's learning rate is 0")
        v = eng.adam_v.cpu().numpy()
        for lo, hi in _idle_ranges(cfg, phase2):
            if m[lo:hi].any() or v[lo:hi].any():
                fails.append(f"{tag}: Adam state of an idle tensor at [{lo}, {hi}) changed")
    if float(eng.grads.abs().max()) != 0.0 or int(eng.touched.abs().max()) != 0:
        fails.append(f"{tag}: gradient arena / touched bitmap not cleared")
    if m[~_stepped_mask(cfg, phase2)].any() and p_before is not None:
        fails.append(f"{tag}: first moment of alignment padding / idle tensors is not zero")
    for label, name, sl in R.pieces(cfg, phase2):
        o, shape = lay[name]
        got = m[o:o + math.prod(shape)][sl]
        w, s = want[label]
        l2, mx, bad = R.ratios(w, s, got, None if m_prev is None else m_prev[o:o + math.prod(shape)][sl])
        yl2, ymx = yard[label]
        print(f"FG|{tag}|{label}|L2 {l2:.3e} cmp {yl2:.3e} x{l2 / yl2:.2f}|max {mx:.4g} cmp {ymx:.4g} x{mx / (4 * ymx + 4):.2f}")
        if not l2 <= 2 * yl2:
            fails.append(f"{tag} {label}: relative L2 {l2:.3e} > 2 x {yl2:.3e}")
        if not mx <= 4 * ymx + 4:
            fails.append(f"{tag} {label}: max error {mx:.4g} u*scale > 4 x {ymx:.4g} + 4")
        if bad:
            fails.append(f"{tag} {label}: {bad} elements of zero scale are not exactly zero")
    row = eng.losses[step].cpu().numpy()[:5].astype(np.float64)
    l2, mx = R.loss_ratios(ref, row)
    print(f"FG|{tag}|losses|L2 {l2:.3e} cmp {yard_loss[0]:.3e} x{l2 / yard_loss[0]:.2f}|max {mx:.4g} cmp {yard_loss[1]:.4g} "
          f"x{mx / (4 * yard_loss[1] + 4):.2f}")
    if not l2 <= 2 * yard_loss[0]:
        fails.append(f"{tag} losses: relative L2 {l2:.3e} > 2 x {yard_loss[0]:.3e}")
    if not mx <= 4 * yard_loss[1] + 4:
        fails.append(f"{tag} losses: max error {mx:.4g} u > 4 x {yard_loss[1]:.4g} + 4")
    return m


# ---------------------------------------------------------------------------------------------------------------------
# single-step cases: one call [1, 2) at lr = 0 from the seeded parameters, under every knob
# ---------------------------------------------------------------------------------------------------------------------
def _variants(bf16):
    solo = [("default", ()), ("layer-by-layer", ((6, 0),) if bf16 else ((6, 2),)), ("atomics grid backward", ((7, 0),)),
            ("dense Adam", ((9, 0),)), ("16 rows", ((13, 0),)), ("32 rows", ((13, 2),)), ("small workgroups", ((14, 1),))]
    many = [(f"k={k} xcd map {v}", ((16, v),), k) for k in (2, 4) for v in (1, 0)]
    return [(n, kn, 1) for n, kn in solo] + many


@pytest.mark.parametrize("phase2", [False, True], ids=["phase1", "phase2"])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [384, 768, 1024, 128])
def test_single_step_gradients(built_lib, C, bf16, phase2):
    from dvt_amd.fit import fit_many
    cfg = R.cfg_of(C)
    B = R.SHAPES[C][0]
    T, step = 4, 1
    freeze = 0.0 if phase2 else 1.0  # switch_step = 0: step 1 is phase 2;  = 4: every step is phase 1
    fails, kept = [], {}
    with ThreadPoolExecutor(R.N_FITS) as pool:  # the four fits' references and yardsticks side by side (cached from here on)
        list(pool.map(lambda fit: R.yardstick(C, fit, bf16, phase2), range(R.N_FITS)))
    for name, knobs, k in _variants(bf16):
        engines, args = [], ([], [], [])
        for fit in range(k):
            _, params, _, _, idx, _ = R.case(C, fit)
            eng = _engine(C, bf16, T, freeze, params)
            assert (step > eng.cfg.switch_step) == phase2
            eng.h_lr[:] = 0.0
            engines.append(eng)
            f, c = _inputs(C, fit)
            args[0].append(f)
            args[1].append(c)
            args[2].append(torch.from_numpy(np.tile(idx, (T, 1))).to(DEV))
        try:
            for key, val in knobs:
                assert built_lib.dvt_tune_set(key, val) == 0, (key, val)
            if k == 1:
                engines[0].fit(args[0][0], args[1][0], args[2][0], log_every=1, step_begin=step, step_end=step + 1)
            else:
                fit_many(engines, *args, log_every=1, step_begin=step, step_end=step + 1)
            torch.cuda.synchronize()
        finally:
            _restore(built_lib)
        for fit, eng in enumerate(engines):
            ref, want, yard, yard_loss = R.yardstick(C, fit, bf16, phase2)  # cached across the knob variants
            tag = f"C={C} {'bf16' if bf16 else 'fp32'} phase {2 if phase2 else 1} {name} fit {fit}"
            kept[name] = _check(eng, cfg, phase2, step, want, yard, ref, yard_loss, tag, fails, p_before=R.case(C, fit)[1])
        del engines
    if C == 1024 and bf16 and phase2:
        # dvt_tune_set(13, 2) asks for 32 rows per workgroup "wherever the LDS images fit"; at C = 1024 in phase 2 they do
        # not (206 KB), and the documented fallback is the 16-row kernel: the MLP gradients are those of (13, 0), bit for bit
        w1 = R.layout(cfg)[0]["w1"][0]
        assert np.array_equal(kept["32 rows"][w1:], kept["16 rows"][w1:])
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# in-call cases: the last step of a longer call (lr of that step = 0), reference at the parameters read back
# ---------------------------------------------------------------------------------------------------------------------
IN_CALL_MARGIN = 3e-8  # see _in_call: six times what two correct fp32 evaluations of a pre-activation differ by


def _in_call(built_lib, C, bf16, T, freeze, warmup, knobs, tag, fails):
    """One call [0, T) with a real schedule whose last entry is 0.  After a call with feedback the parameters are no longer
    the seeded ones, so no reseeding can keep the pre-activations of the LAST step away from zero in advance: where one
    lies within IN_CALL_MARGIN of zero in units of its magnitude sum (two correct float32 evaluations differ by
    u / sqrt(K) <= 5e-9 there (K >= 128), and would then disagree about a ReLU mask), the call is repeated with the next index stream.
    The first moment is not zero before the last step either: a twin engine runs the same call without that step, and its
    m is the m_prev of R.ratios()."""
    cfg = R.cfg_of(C)
    B = R.SHAPES[C][0]
    _, params, feat, xy, _, _ = R.case(C, 0)
    f, c = _inputs(C, 0)
    phase2 = T - 1 > int(freeze * T)
    allowed = np.flatnonzero(np.arange(feat.shape[0]) % cfg.lattice != R.EMPTY_ROW)
    for attempt in range(12):
        idx = allowed[np.random.RandomState(1000 * T + C + attempt).randint(0, len(allowed), (T, B))].astype(np.int32)
        idx_d = torch.from_numpy(idx).to(DEV)
        eng = _engine(C, bf16, T, freeze, params, warmup=warmup)
        twin = _engine(C, bf16, T, freeze, params, warmup=warmup)  # the same call without its last step: m before that step
        assert eng.h_lr[T - 2] > 0.0
        assert (T - 1 > eng.cfg.switch_step) == phase2 and 0 <= eng.cfg.switch_step < T - 1  # the call crosses the switch
        eng.h_lr[T - 1] = 0.0
        try:
            for key, val in knobs:
                assert built_lib.dvt_tune_set(key, val) == 0
            eng.fit(f, c, idx_d, log_every=1, step_begin=0, step_end=T)
            twin.fit(f, c, idx_d, log_every=0, step_begin=0, step_end=T - 1)
            torch.cuda.synchronize()
        finally:
            _restore(built_lib)
        p = eng.params.cpu().numpy()
        fwd = [R._chain(cfg, p, feat, xy, idx[T - 1], phase2, m, forward_only=True) for m in ("f64", "bf16" if bf16 else "f32")]
        margin = min(float((ch["pre"][n].double().abs() / mag).min()) for n, mag in fwd[0]["pre_mag"].items() for ch in fwd)
        if margin >= IN_CALL_MARGIN:
            break
        print(f"FG|{tag}: a pre-activation of the last step at {margin:.1e} of its magnitude sum, next index stream")
    else:
        fails.append(f"{tag}: no index stream kept the last step's pre-activations away from zero")
        return
    assert not np.array_equal(p, params)  # the earlier steps did move the parameters
    ref, want, yard, yard_loss = R.yardstick_at(cfg, p, feat, xy, idx[T - 1], bf16, phase2)
    _check(eng, cfg, phase2, T - 1, want, yard, ref, yard_loss, tag, fails, m_prev=twin.adam_m.cpu().numpy())


@pytest.mark.parametrize("knobs", [(), ((12, 0),), ((11, 0),)], ids=["default", "separate-shadow", "separate-catchup"])
@pytest.mark.parametrize("T", [3, 130])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("C", [384, 768])
def test_in_call_gradients(built_lib, C, bf16, T, knobs):
    """3 steps across the phase switch (switch_step 1: steps 0, 1 phase 1, step 2 phase 2) and 130 steps (switch at 65, a refresh of the lazy
    region at 32, 64 and 96, the sorted-list chunk boundary at 128): a stale weight shadow out of the merged Adam launch,
    the merged lazy catch-up and the list bookkeeping all end in the last step's gradients."""
    fails = []
    tag = f"C={C} {'bf16' if bf16 else 'fp32'} in-call T={T} {'+'.join(f'({k},{v})' for k, v in knobs) or 'default'}"
    _in_call(built_lib, C, bf16, T, 0.5, 1 if T == 3 else 13, knobs, tag, fails)
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------------------------------------------------
# Adam on the arena the fit builds: p, m, v of every element after one step at the shipped beta1 = 0.9, lr > 0
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1], ids=["rcp-sqrt-replay", "ieee-replay"])
@pytest.mark.parametrize("phase2", [False, True], ids=["phase1", "phase2"])
def test_adam_on_the_fit_arena(built_lib, phase2, exact):
    """From zero state, one call [s, s + 1): m1 = c1 g', so g' = m1 / c1 up to one rounding; then
        v1 = c2 g'^2            (two roundings + twice the one of g')
        p1 = p0 + ns m1 / (sqrt(v1) / bc2s + eps)   evaluated from the m1 and v1 read back: sqrt, /, +, /, fma = five roundings,
                                                    the lazy levels' default replay (v_rcp_f32 / v_sqrt_f32) one ulp more each
    with the fp32-narrowed scalars of dvt_adam_step_k / dvt_adam_lazy_tables and each segment's own step count; and m1 / c1
    obeys the gradient bounds of the cases above (+ 1 u for the division).  Swept grid levels, lazy levels, MLP and G / h."""
    C, bf16 = 384, True
    cfg = R.cfg_of(C)
    _, params, _, _, idx, _ = R.case(C, 0)
    T, step, lr = 4, (1 if phase2 else 0), 0.01
    eng = _engine(C, bf16, T, 0.0 if phase2 else 1.0, params, beta1=0.9)
    eng.h_lr[:] = lr
    f, c = _inputs(C, 0)
    idx_d = torch.from_numpy(np.tile(idx, (T, 1))).to(DEV)  # alive until the synchronise: the kernels in flight read it
    try:
        assert built_lib.dvt_tune_set(10, exact) == 0
        eng.fit(f, c, idx_d, log_every=1, step_begin=step, step_end=step + 1)
        torch.cuda.synchronize()
    finally:
        _restore(built_lib)
    p0 = params.astype(np.float64)
    p1, m1, v1 = (getattr(eng, n).cpu().numpy().astype(np.float64) for n in ("params", "adam_m", "adam_v"))
    c1, c2 = float(np.float32(1.0 - 0.9)), float(np.float32(1.0 - 0.99))
    eps = float(np.float32(1e-15))
    lay, n = R.layout(cfg)
    e0 = R.lazy_first_entry(cfg) * cfg.n_features
    fails = []
    t_field, t_h = step + 1, step - int(eng.cfg.switch_step)
    regions = [("grid[swept]", 0, e0, t_field, False), ("grid[lazy]", e0, lay["w1"][0], t_field, not exact),
               ("field MLP", lay["w1"][0], lay["G"][0], t_field, False)]
    regions.append(("h", lay["wh1"][0], n, t_h, False) if phase2 else ("G", lay["G"][0], lay["wh1"][0], t_field, False))
    for name, lo, hi, t, approx in regions:
        ns = float(np.float32(-(lr / (1.0 - 0.9 ** t))))
        bc2s = float(np.float32(math.sqrt(1.0 - 0.99 ** t)))
        if approx:  # the replay multiplies by the fp32 reciprocal instead
            bc2s = 1.0 / float(np.float32(1.0 / math.sqrt(1.0 - 0.99 ** t)))
        g = m1[lo:hi] / c1
        v_want = c2 * g * g
        v_err = np.abs(v1[lo:hi] - v_want)
        if not (v_err <= 5 * U * v_want + 1e-45).all():
            fails.append(f"{name}: v1 off by {float((v_err / np.maximum(v_want, 1e-300)).max() / U):.1f} u")
        stepv = ns * m1[lo:hi] / (np.sqrt(v1[lo:hi]) / bc2s + eps)
        p_err = np.abs(p1[lo:hi] - (p0[lo:hi] + stepv))
        tol = (8 if approx else 5) * U * np.abs(stepv) + U * np.abs(p1[lo:hi])
        if not (p_err <= tol).all():
            fails.append(f"{name}: p1 off by {float((p_err / np.maximum(tol, 1e-300)).max()):.2f} x its tolerance")
        print(f"FG|adam {name} t={t} exact={exact}: v1 max {float((v_err / np.maximum(v_want, 1e-300)).max() / U):.2f} u, "
              f"p1 max {float((p_err / np.maximum(tol, 1e-300)).max()):.2f} of tolerance, moved {float((p1[lo:hi] != p0[lo:hi]).mean()):.4f}")
    # untouched tensors of the phase: nothing moved
    for lo, hi in _idle_ranges(cfg, phase2):
        assert np.array_equal(p1[lo:hi], p0[lo:hi]) and not m1[lo:hi].any() and not v1[lo:hi].any()
    # m1 / c1 is the step's g': the bounds of the gradient cases, one more rounding
    ref, want, yard, _ = R.yardstick(C, 0, bf16, phase2)
    for label, name, sl in R.pieces(cfg, phase2):
        o, shape = lay[name]
        l2, mx, bad = R.ratios(*want[label], (m1[o:o + math.prod(shape)] / c1)[sl])
        if not (l2 <= 2 * yard[label][0] and mx <= 4 * yard[label][1] + 5 and bad == 0):
            fails.append(f"{label}: m1 / c1 L2 {l2:.3e} (cmp {yard[label][0]:.3e}), max {mx:.4g} (cmp {yard[label][1]:.4g}), {bad} nonzero pads")
    assert not fails, "\n".join(fails)
