"""One stage-1 fit step in float64, and the same chain at the kernels' precisions (CPU only, no GPU import).

`reference()` evaluates the step that `dvt_fit_run` enqueues (csrc/dvt_fit.hip: hash-grid encoding -> field MLP ->
loss of oracle/models.py -> autograd's backward, everything multiplied by grad_scale and never unscaled) in float64 and
returns, for every arena tensor, the gradient and a per-element MAGNITUDE: the sum of the absolute values of the terms
of the last contraction that forms the element.  `u * magnitude` is the unit in which a float32 evaluation of that
contraction errs, whatever its summation order, so element errors are judged in it.

`comparator_f32()` / `comparator_bf16()` are the same chain at the kernels' precision.  They are the yardsticks: how far
a correct evaluation at that precision lands from float64 on these very inputs.  The GPU tests hold the kernels to a
small multiple of that distance; nothing in here ever sees a GPU result.

  float32   torch float32 throughout, every contraction in ONE float32 accumulator per output: the GEMMs add four
            products per step along k (one v_mfma_f32_16x16x4_f32 worth of k), bias gradients and the batch
            sums of the loss rows run left to right.  torch's own sgemm / sum keep several partial sums per output
            (k-blocking, pairwise trees); that is systematically more accurate than a float32 accumulator, by sqrt(K / block),
            so it would be a yardstick for a precision the kernels do not claim.
            Four products per accumulator rounding is the MOST accurate thing that instruction could do.  The fp32 MFMA is
            in fact an fmaf chain (csrc/dvt_gemm_f32_dev.h: "bitwise an fmaf chain"): one accumulator rounding per product,
            four times as many, hence up to sqrt(4) = 2 x this comparator's rms error in a tensor whose error is all GEMM
            accumulation.  Replacing _mm_f32 by such a chain (fl32(acc + a_k b_k), the product exact in float64) moves the
            comparator's L2 error of the grid gradient at C = 1024 from 3.65e-07 to 6.97e-07; the kernels measure 7.13e-07.
            That is why the kernels' L2 ratios approach, but do not pass, the allowed 2 as K grows (1.3 at C = 384, 1.8 at
            768, 1.95 at 1024).  The comparator stays at four per step: it is the stricter yardstick of the two.
  bfloat16  fp32 accumulation, operands rounded to bf16 (RNE) exactly where the kernels round them ("bf16
            rounding points of the fit step"): enc, raw, h1, r1, r2 as GEMM operands; d_pred, d_Hres, dh1, dr2, dr1 as
            GEMM operands AND as the addends of the bias gradients; the weights (shadow copies).  F, Hres, d_enc, the loss
            rows and the gradients of G and of the grid are formed from unrounded fp32 rows.  The layer-by-layer bf16
            path (dvt_linear_group) rounds at the same points (operands while staged, bias gradients from the staged dy
            tile), so it has no variant of its own.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from oracle.hashgrid import corners, grid_table

U = 2.0 ** -24  # unit roundoff of float32
TINY = 2.0 ** -126  # smallest normal float32: the relative error model holds above it only (ratios())
TENSORS = ("grid", "w1", "b1", "w2", "b2", "G", "wh1", "bh1", "wh2", "bh2", "wh3", "bh3")
PHASE1 = ("grid", "w1", "b1", "w2", "b2", "G")
PHASE2 = ("grid", "w1", "b1", "w2", "b2", "wh1", "bh1", "wh2", "bh2", "wh3", "bh3")
LOSS_KEYS = ("loss", "patch_l2_loss", "cosine_similarity_loss", "residual_loss", "residual_sparsity_loss")


@dataclass(frozen=True)
class Cfg:
    feat_dim: int
    lattice: int
    n_levels: int = 16
    log2_hashmap_size: int = 16
    base_resolution: int = 16
    max_resolution: int = 1024
    n_features: int = 8
    grad_scale: float = 1024.0
    weight_decay: float = 1e-5

    @property
    def hidden(self):
        return self.feat_dim // 2

    @property
    def res_hidden(self):
        return self.feat_dim // 4

    @property
    def table(self):
        return _table(self.n_levels, self.n_features, self.base_resolution, self.max_resolution, self.log2_hashmap_size)

    @property
    def wd32(self) -> float:
        """weight decay as the kernels see it (torch narrows the python double to an fp32 scalar)"""
        return float(np.float32(self.weight_decay))


@functools.lru_cache(maxsize=None)
def _table(n_levels, n_features, base, mx, log2):
    return grid_table(n_levels, n_features, base, mx, log2)


def _up256(n):
    return (n + 255) // 256 * 256


def layout(cfg: Cfg):
    """{name: (offset, shape)} and the arena length, as dvt_fit_layout carves it (every tensor padded to 256 floats)."""
    C, H, R = cfg.feat_dim, cfg.hidden, cfg.res_hidden
    E = cfg.n_levels * cfg.n_features
    shapes = {"grid": (cfg.table.n_entries_total, cfg.n_features), "w1": (H, E), "b1": (H,), "w2": (C, H), "b2": (C,),
              "G": (cfg.lattice, C), "wh1": (R, C), "bh1": (R,), "wh2": (R, R), "bh2": (R,), "wh3": (C, R), "bh3": (C,)}
    out, o = {}, 0
    for name in TENSORS:
        out[name] = (o, shapes[name])
        o += _up256(math.prod(shapes[name]))
    return out, o


def lazy_first_entry(cfg: Cfg):
    """First grid entry the lazy Adam owns (lazy_range() of csrc/dvt_fit.hip), or None."""
    t = cfg.table
    for l in range(t.n_levels):
        if int(t.entries[l]) >= 65536:
            e = (int(t.offset[l]) + 31) & ~31
            return e if e < t.n_entries_total else None
    return None


def views(cfg: Cfg, arena):
    """{name: view of the tensor inside a flat arena (numpy or torch)}"""
    lay, _ = layout(cfg)
    return {n: arena[o:o + math.prod(s)].reshape(s) for n, (o, s) in lay.items()}


def _bf16(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def _seq_sum0(x: torch.Tensor) -> torch.Tensor:
    """left-to-right sum over dim 0 in x's own precision (numpy: torch's CPU cumsum accumulates float32 in double)"""
    a = x.numpy()
    return torch.from_numpy(np.cumsum(a, axis=0, dtype=a.dtype)[-1:].copy())[0]


def _mm_f32(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a [M, K] @ b [K, N] in float32 with one accumulator per output, four products per step along k"""
    M, K = a.shape
    pad = (-K) % 4
    if pad:
        a = torch.cat([a, a.new_zeros(M, pad)], 1)
        b = torch.cat([b, b.new_zeros(pad, b.shape[1])], 0)
    at = a.reshape(M, -1, 4).transpose(0, 1).contiguous()  # [K / 4, M, 4]
    bt = b.contiguous().reshape(-1, 4, b.shape[1])          # [K / 4, 4, N]
    acc = torch.zeros(M, b.shape[1], dtype=torch.float32)
    for i in range(at.shape[0]):
        acc.addmm_(at[i], bt[i])
    return acc


def _chain(cfg: Cfg, params, feat, xy, idx_row, phase2: bool, mode: str, forward_only: bool = False, order_seed=None):
    """order_seed (float32 mode): every contraction runs over a seeded permutation of its index -- another, equally valid
    float32 evaluation of the same step."""
    assert mode in ("f64", "f32", "bf16")
    assert order_seed is None or mode == "f32"
    ors = np.random.RandomState(order_seed) if order_seed is not None else None
    dt = torch.float64 if mode == "f64" else torch.float32
    rb = _bf16 if mode == "bf16" else (lambda t: t)
    seq = mode != "f64"

    def mm(a, b):
        if mode != "f32":  # (bf16 operands: the 2^-9 roundings dwarf any accumulation order)
            return a @ b
        if ors is not None:
            perm = torch.from_numpy(ors.permutation(a.shape[1]))
            a, b = a[:, perm], b[perm]
        return _mm_f32(a, b)

    def seq_sum0(x):
        return _seq_sum0(x if ors is None else x[torch.from_numpy(ors.permutation(x.shape[0]))])
    C, B = cfg.feat_dim, len(idx_row)
    L, NF = cfg.n_levels, cfg.n_features
    idx_row = np.asarray(idx_row).astype(np.int64)
    P = {n: torch.from_numpy(np.ascontiguousarray(v)).to(dt) for n, v in views(cfg, np.asarray(params, np.float32)).items()}
    raw = torch.from_numpy(np.asarray(feat, np.float32)[idx_row]).to(dt)
    pts = np.asarray(xy, np.float32)[idx_row]
    ci, cw = corners(cfg.table, pts)  # bit-exact fp32 by contract: exact numbers from here on
    ci = torch.from_numpy(ci.astype(np.int64))  # [B, L, 4]
    cw = torch.from_numpy(cw).to(dt)
    # ---- forward
    vals = P["grid"][ci.reshape(-1)].view(B, L, 4, NF)
    if mode == "f64":
        enc = (cw.unsqueeze(-1) * vals).sum(2)
    else:  # the kernels' fmaf chain over the four corners: exact product + one rounding per step
        acc = torch.zeros(B, L, NF, dtype=torch.float64)
        for c in range(4):
            acc = (cw[:, :, c, None].double() * vals[:, :, c].double() + acc).float().double()
        enc = acc.float()
    enc = enc.reshape(B, L * NF)
    out = {"mode": mode}

    def linear(x, w, b):
        return mm(rb(x), rb(P[w]).T) + P[b]

    pre_h1 = linear(enc, "w1", "b1")
    h1 = pre_h1.clamp_min(0)
    F = linear(h1, "w2", "b2")
    lat = torch.from_numpy(idx_row % cfg.lattice)
    fg = F + P["G"][lat]
    if phase2:
        pre_r1 = linear(raw, "wh1", "bh1")
        r1 = pre_r1.clamp_min(0)
        pre_r2 = linear(r1, "wh2", "bh2")
        r2 = pre_r2.clamp_min(0)
        Hres = linear(r2, "wh3", "bh3")
        pred = fg + Hres
    else:
        Hres, pred = None, fg
    out["pre"] = {"h1": pre_h1, **({"r1": pre_r1, "r2": pre_r2, "Hres": Hres} if phase2 else {})}
    if mode == "f64":  # magnitude sums of the contractions in front of the ReLUs and of sign(Hres)
        pm = {"h1": enc.abs() @ P["w1"].abs().T + P["b1"].abs()}
        if phase2:
            pm["r1"] = raw.abs() @ P["wh1"].abs().T + P["bh1"].abs()
            pm["r2"] = r1.abs() @ P["wh2"].abs().T + P["bh2"].abs()
            pm["Hres"] = r2.abs() @ P["wh3"].abs().T + P["bh3"].abs()
        out["pre_mag"] = pm
    if forward_only:
        return out
    # ---- loss rows (csrc/dvt_loss_row.h)
    diff = pred - raw
    sse = (diff * diff).sum(1)
    dot = (pred * raw).sum(1)
    npp = (pred * pred).sum(1)
    nrr = (raw * raw).sum(1)
    denom = npp.sqrt().clamp_min(1e-8) * nrr.sqrt().clamp_min(1e-8)
    cosv = dot / denom
    one = torch.ones((), dtype=dt)
    nc = one * B * C

    rsse = rabs = None
    if phase2:
        e_res = Hres - (raw - fg)
        rsse, rabs = (e_res * e_res).sum(1), Hres.abs().sum(1)

    def five(order=None):  # the five logged scalars (loss_reduce_kernel), the batch summed in the given order
        def total(rows):
            return _seq_sum0(rows if order is None else rows[order]) if seq else rows.sum()
        l2 = total(sse) / nc
        cosl = one - total(cosv) / B
        res = (one * 0.1) * total(rsse) / nc if phase2 else torch.zeros((), dtype=dt)
        spars = (one * 0.02) * total(rabs) / nc if phase2 else torch.zeros((), dtype=dt)
        return np.array([float(l2 + cosl + res + spars), float(l2), float(cosl), float(res), float(spars)])

    out["loss"] = five()
    if seq:  # the error of a sum depends on the order of its terms: LOSS_ORDERS orders of the batch (see loss_ratios)
        rs = np.random.RandomState(B)
        out["loss_orders"] = [out["loss"]] + [five(torch.from_numpy(rs.permutation(B))) for _ in range(LOSS_ORDERS - 1)]
    l2, res, spars = (float(v) for v in out["loss"][[1, 3, 4]])
    if mode == "f64":
        m = [float(l2), 1.0 + float(cosv.abs().sum() / B), float(res), float(spars)]
        out["loss_mag"] = np.array([sum(m)] + m)
    # ---- gradients of the rows, times grad_scale
    gs = one * cfg.grad_scale
    inv_n, inv_nc = one / B, one / nc
    a_r = (-inv_n / denom).unsqueeze(1)
    a_p = torch.where(npp.sqrt() < 1e-8, torch.zeros_like(cosv), inv_n * cosv / npp).unsqueeze(1)
    d_pred = gs * ((2.0 * inv_nc) * diff + a_r * raw + a_p * pred)
    dh1 = mm(rb(d_pred), rb(P["w2"])) * (h1 > 0)
    d_enc = mm(rb(dh1), rb(P["w1"]))
    g, mag = {}, {}

    def wgrad(name_w, name_b, dy, x):
        dyr, xr = rb(dy), rb(x)
        g[name_w] = mm(dyr.T, xr)
        g[name_b] = seq_sum0(dyr) if seq else dyr.sum(0)
        if mode == "f64":
            mag[name_w] = dyr.abs().T @ xr.abs()
            mag[name_b] = dyr.abs().sum(0)

    wgrad("w2", "b2", d_pred, h1)
    wgrad("w1", "b1", dh1, enc)
    if phase2:
        d_H = gs * ((0.2 * inv_nc) * e_res + (0.02 * inv_nc) * torch.sign(Hres))
        dr2 = mm(rb(d_H), rb(P["wh3"])) * (r2 > 0)
        dr1 = mm(rb(dr2), rb(P["wh2"])) * (r1 > 0)
        wgrad("wh3", "bh3", d_H, r2)
        wgrad("wh2", "bh2", dr2, r1)
        wgrad("wh1", "bh1", dr1, raw)
        out.update(d_Hres=d_H)
    else:  # G trains: row r of its gradient = the sum of the d(pred) rows of the samples on lattice row r
        order = torch.from_numpy(np.argsort(lat.numpy(), kind="stable"))
        g["G"] = torch.zeros(cfg.lattice, C, dtype=dt).index_add_(0, lat[order], d_pred[order])
        if mode == "f64":
            mag["G"] = torch.zeros(cfg.lattice, C, dtype=dt).index_add_(0, lat, d_pred.abs())
    contrib = cw.unsqueeze(-1) * d_enc.view(B, L, 1, NF)  # [B, L, 4, NF]
    n_ent = cfg.table.n_entries_total
    g["grid"] = torch.zeros(n_ent, NF, dtype=dt).index_add_(0, ci.reshape(-1), contrib.reshape(-1, NF))
    if mode == "f64":
        mag["grid"] = torch.zeros(n_ent, NF, dtype=dt).index_add_(0, ci.reshape(-1), contrib.abs().reshape(-1, NF))
        out["mag"] = {n: v.numpy() for n, v in mag.items()}
        out["corner_idx"], out["corner_w"] = ci.numpy(), cw.numpy()
    out["g"] = {n: v.double().numpy() for n, v in g.items()}
    out.update(F=F, Hres=Hres, d_pred=d_pred, d_enc=d_enc, enc=enc)
    return out


def reference(cfg, params, feat, xy, idx_row, phase2):
    """float64: {'g': {tensor: gradient}, 'mag': {tensor: magnitude}, 'loss': [5], 'loss_mag': [5], 'F', 'Hres', 'd_pred',
    'd_enc', 'pre': {layer: pre-activation}, 'pre_mag': {layer: its magnitude sum}}.  Tensors the phase does not step are absent."""
    return _chain(cfg, params, feat, xy, idx_row, phase2, "f64")


def comparator_f32(cfg, params, feat, xy, idx_row, phase2):
    return _chain(cfg, params, feat, xy, idx_row, phase2, "f32")


def comparator_bf16(cfg, params, feat, xy, idx_row, phase2):
    return _chain(cfg, params, feat, xy, idx_row, phase2, "bf16")


# ---------------------------------------------------------------------------------------------------------------------
# The observable and its error measures.  With beta1 = 0, Adam's first moment after a step is that step's
#   g' = fmaf(wd, p, g)   followed by   m = fmaf(g' - m_prev, 1, m_prev)
# i.e. g' within u (|g' - m_prev| + |g'|) (csrc/dvt_adam.hip: adam1()).
# ---------------------------------------------------------------------------------------------------------------------
def pieces(cfg: Cfg, phase2: bool):
    """[(label, tensor name, element slice inside the tensor's flat storage)]: the stepped tensors of a phase, the grid
    split into the part the dense / `touched`-gated sweep steps and the part the lazy Adam owns."""
    e0 = lazy_first_entry(cfg)
    out = []
    for name in (PHASE2 if phase2 else PHASE1):
        if name == "grid" and e0 is not None:
            out.append(("grid[swept]", "grid", slice(0, e0 * cfg.n_features)))
            out.append(("grid[lazy]", "grid", slice(e0 * cfg.n_features, None)))
        else:
            out.append((name, name, slice(None)))
    return out


def expected_moment(cfg: Cfg, ref, params, phase2: bool):
    """{label: (g' in float64, scale = mag + |wd p|)} of every piece."""
    pv = views(cfg, np.asarray(params, np.float32))
    out = {}
    for label, name, sl in pieces(cfg, phase2):
        wdp = cfg.wd32 * pv[name].reshape(-1)[sl].astype(np.float64)
        out[label] = (ref["g"][name].reshape(-1)[sl] + wdp, ref["mag"][name].reshape(-1)[sl] + np.abs(wdp))
    return out


def moment_of(cfg: Cfg, chain_out, params, phase2: bool):
    """What a correct fp32 Adam holds in m after the step when the gradients are `chain_out`'s: fl32(g + wd p)."""
    pv = views(cfg, np.asarray(params, np.float32))
    out = {}
    for label, name, sl in pieces(cfg, phase2):
        wdp = cfg.wd32 * pv[name].reshape(-1)[sl].astype(np.float64)
        out[label] = (chain_out["g"][name].reshape(-1)[sl] + wdp).astype(np.float32)
    return out


def ratios(want, scale, got, m_prev=None):
    """(relative L2 error of the tensor, max_i |got_i - want_i| / (u * scale_i) over scale_i > 0, elements with scale 0
    that are not exactly 0).  m_prev: the first moment BEFORE the step, where it was not zero -- adam1() forms
    fl(fl(g' - m_prev) + m_prev), whose first rounding is worth u |g' - m_prev| <= u (|g'| + |m_prev|): the part u |m_prev| has
    nothing to do with the gradient and is taken off an element's error before the maximum.
    Underflow: fl(x) = x (1 + d), |d| <= u, holds for normal results only; below 2^-126 a float32 result is off by up to
    a subnormal spacing (or is flushed) whatever its scale.  That happens here: weight decay alone drives the grid entries
    that no sample ever touches to |p| ~ 1e-41 within a hundred Adam steps, and their g' = wd p ~ 1e-46 is 0 in ANY
    float32 evaluation -- an error of exactly 1 scale = 2^24 u scale, which would be the maximum of every grid tensor of the
    130-step cases, the comparator's included, and make that bound say nothing.  So the absolute floor 2^-126 is taken
    off an element's error as well: nothing against a gradient of these cases, which carry grad_scale = 1024."""
    got = np.asarray(got, np.float64).reshape(-1)
    err = np.abs(got - want)
    nz = scale > 0
    l2 = float(np.sqrt((err * err).sum()) / max(np.sqrt((want * want).sum()), 1e-300))
    err = np.maximum(err - TINY, 0.0)
    if m_prev is not None:
        err = np.maximum(err - U * np.abs(np.asarray(m_prev, np.float64).reshape(-1)), 0.0)
    mx = float((err[nz] / (U * scale[nz])).max()) if nz.any() else 0.0
    return l2, mx, int(np.count_nonzero(got[~nz]))


def loss_ratios(ref, loss5):
    """(relative L2 error of the five logged scalars as one vector, max_i error / (u * magnitude_i)).  Given a comparator's
    output instead of five numbers: the worst of its LOSS_ORDERS batch orders.  Five sums are too few to average the luck
    of one order away (a single sum lands within 0.1 u of the exact value one time in ten), and the kernels are free to
    choose theirs; a tensor's figures average over thousands of sums and need no such care."""
    want, scale = ref["loss"], ref["loss_mag"]
    if isinstance(loss5, dict):
        each = [ratios(want, scale, v)[:2] for v in loss5["loss_orders"]]
        return max(e[0] for e in each), max(e[1] for e in each)
    return ratios(want, scale, loss5)[:2]


# ---------------------------------------------------------------------------------------------------------------------
# Seeded inputs of the test cases (shared by the CPU and the GPU tests).
# ---------------------------------------------------------------------------------------------------------------------
# C -> (batch, lattice side, views).  The smallest shapes at which each kernel can still go wrong (tests/test_gpu_fit_grads.py).
SHAPES = {384: (1024, 7, 3), 768: (1024, 37, 2), 1024: (512, 12, 3), 128: (384, 9, 3)}
N_FITS = 4           # images per shape (fit_many: k = 2 uses the first two, k = 4 all)
EMPTY_ROW = 3        # lattice row that no sample of any case lands on
MAX_ORDERS = 8      # float32 evaluation orders behind the comparator's maximum (yardstick_at)
LOSS_ORDERS = 8     # batch orders in which the comparators sum the loss rows
MARGIN = 1e-6        # no ReLU / sign pre-activation closer to zero than MARGIN x its magnitude sum


def cfg_of(C: int) -> Cfg:
    side = SHAPES[C][1]
    return Cfg(feat_dim=C, lattice=side * side)


def make_data(cfg: Cfg, B: int, V: int, seed: int):
    """(feat [V * lattice, C], xy [V * lattice, 2], idx [B]): V - 1 random crop boxes and the full image, features =
    lattice artefact + noise, a batch that never lands on lattice row EMPTY_ROW."""
    rs = np.random.RandomState(seed)
    side = int(round(math.sqrt(cfg.lattice)))
    xy = np.zeros((V, side, side, 2), np.float32)
    for v in range(V):
        w, h = (1.0, 1.0) if v == V - 1 else rs.uniform(0.3, 0.8, 2)
        x0, y0 = rs.uniform(0, 1 - w), rs.uniform(0, 1 - h)
        gy, gx = np.meshgrid(np.linspace(y0, y0 + h, side), np.linspace(x0, x0 + w, side), indexing="ij")
        xy[v] = np.stack([gx, gy], -1)
    xy = np.clip(xy.reshape(-1, 2), 0.0, 1.0).astype(np.float32)
    art = rs.standard_normal((1, cfg.lattice, cfg.feat_dim)) * 0.5
    feat = (art + rs.standard_normal((V, cfg.lattice, cfg.feat_dim)) * 0.7).reshape(-1, cfg.feat_dim).astype(np.float32)
    allowed = np.flatnonzero(np.arange(V * cfg.lattice) % cfg.lattice != EMPTY_ROW)
    idx = allowed[rs.randint(0, len(allowed), B)].astype(np.int32)
    return feat, xy, idx


def make_params(cfg: Cfg, feat, xy, idx, seed: int):
    """A flat fp32 arena.  Grid U(-0.5, 0.5) and G ~ N(0, 0.3^2) so that every branch carries signal; nn.Linear-style
    weights.  The bias in front of a ReLU sits about two standard deviations of its unit's matrix product ABOVE zero: the
    mask still depends on the row (a unit is off in ~2 % of the rows), few pre-activations come near zero, where rounding
    would decide the sign, and no unit is on in only a handful of rows -- the gradient elements of such a unit consist of
    a few barely-positive activations whose RELATIVE error is (error of the pre-activation) / (distance from zero), thousands
    of u in any float32 evaluation, and a maximum over the tensor would then compare two draws of one element's luck.
    The bias of Hres (whose sign carries the sparsity term) sits three deviations away, either side."""
    rs = np.random.RandomState(seed)
    lay, n = layout(cfg)
    arena = np.zeros(n, np.float32)
    v = views(cfg, arena)
    v["grid"][...] = rs.uniform(-0.5, 0.5, v["grid"].shape)
    v["G"][...] = rs.standard_normal(v["G"].shape) * 0.3
    for w in ("w1", "w2", "wh1", "wh2", "wh3"):
        bound = 1.0 / math.sqrt(v[w].shape[1])
        v[w][...] = rs.uniform(-bound, bound, v[w].shape)

    def offset_bias(x, w, sigmas=2.0, both_sides=False):  # x [B, K] float64
        pre = x @ v[w].astype(np.float64).T
        sd = pre.std(0) + 1e-3
        side = rs.choice([-1.0, 1.0], sd.shape) if both_sides else 1.0
        b = side * rs.uniform(0.8 * sigmas, 1.2 * sigmas, sd.shape) * sd - pre.mean(0)
        return b.astype(np.float32), np.maximum(pre + b.astype(np.float32), 0.0)

    ci, cw = corners(cfg.table, xy[idx])
    enc = (cw[..., None].astype(np.float64) * v["grid"].astype(np.float64)[ci.astype(np.int64)]).sum(2).reshape(len(idx), -1)
    v["b1"][...], _ = offset_bias(enc, "w1")
    v["b2"][...] = rs.uniform(-0.05, 0.05, v["b2"].shape)
    raw = feat[idx].astype(np.float64)
    v["bh1"][...], r1 = offset_bias(raw, "wh1")
    v["bh2"][...], r2 = offset_bias(r1, "wh2")
    v["bh3"][...], _ = offset_bias(r2, "wh3", 3.0, both_sides=True)
    return arena


def input_conditions(cfg: Cfg, params, feat, xy, idx):
    """The conditions that make a case meaningful -> list of the ones that do NOT hold (empty: all hold)."""
    bad = []
    idx = np.asarray(idx)
    if len(np.unique(idx)) == len(idx):
        bad.append("no repeated row index in the batch")
    cnt = np.bincount(idx % cfg.lattice, minlength=cfg.lattice)
    if cnt.min() != 0 or cnt.max() < 3:
        bad.append("G rows: need one without a sample and one with three or more")
    t = cfg.table
    ci, _ = corners(t, np.asarray(xy, np.float32)[idx])
    shared = False
    for l in np.flatnonzero(t.hashed):
        e = ci[:, l, :].reshape(-1)  # (sample, corner) pairs of the level
        shared = shared or len(np.unique(e)) < len(e)
    if not shared:
        bad.append("no two (sample, corner) pairs of a hashed level share an entry")
    e0 = lazy_first_entry(cfg)
    if e0 is None:
        bad.append("no lazy level")
    else:
        hit = np.zeros(t.n_entries_total, bool)
        hit[ci.reshape(-1).astype(np.int64)] = True
        if not hit[e0:].any() or hit[e0:].all():
            bad.append("lazy levels: need a touched and an untouched entry")
    ref = _chain(cfg, params, feat, xy, idx, True, "f64", forward_only=True)
    chains = [ref] + [_chain(cfg, params, feat, xy, idx, True, m, forward_only=True) for m in ("f32", "bf16")]
    for name, mag in ref["pre_mag"].items():
        for ch in chains:  # (the comparators' own pre-activations too: a mask must not hinge on THEIR summation order either)
            worst = float((ch["pre"][name].double().abs() / mag).min())
            if worst < MARGIN:
                bad.append(f"{name} ({ch['mode']}): a pre-activation at {worst:.1e} of its magnitude sum")
    return bad


# first seed per (C, fit) at which input_conditions() hold: found by the loop below, which starts there and, for a seed
# from this table, leaves the (slow) check to tests/test_fit_grads_cpu.py, which asserts it for every case
FIRST_SEED = {
    (128, 0): 12800000, (128, 1): 12810000, (128, 2): 12820000, (128, 3): 12830000,
    (384, 0): 38400000, (384, 1): 38410000, (384, 2): 38420000, (384, 3): 38430000,
    (768, 0): 76800012, (768, 1): 76810027, (768, 2): 76820010, (768, 3): 76830000,
    (1024, 0): 102400001, (1024, 1): 102410002, (1024, 2): 102420014, (1024, 3): 102430000,
}


@functools.lru_cache(maxsize=None)
def case(C: int, fit: int):
    """Seeded inputs of fit `fit` at shape C: (cfg, params, feat, xy, idx, seed), reseeded until input_conditions() hold.
    Every fit has its own parameters and its own image (the engines of a batched launch share nothing)."""
    cfg = cfg_of(C)
    B, _, V = SHAPES[C]
    base = 100000 * C + 10000 * fit
    seed = FIRST_SEED.get((C, fit), base)
    while True:
        if seed - base > 2000:
            raise RuntimeError(f"C = {C}, fit {fit}: no seed satisfies the input conditions")
        feat, xy, idx = make_data(cfg, B, V, seed)
        params = make_params(cfg, feat, xy, idx, seed)
        if FIRST_SEED.get((C, fit)) == seed or not input_conditions(cfg, params, feat, xy, idx):
            return cfg, params, feat, xy, idx, seed
        seed += 1


@functools.lru_cache(maxsize=None)
def yardstick(C: int, fit: int, bf16: bool, phase2: bool):
    """(reference, {label: (g', scale)}, {label: (comparator L2, comparator max)}, comparator loss ratios) of a seeded case
    at its initial parameters."""
    cfg, params, feat, xy, idx, _ = case(C, fit)
    return yardstick_at(cfg, params, feat, xy, idx, bf16, phase2)


def yardstick_at(cfg, params, feat, xy, idx, bf16, phase2):
    ref = reference(cfg, params, feat, xy, idx, phase2)
    cmp_ = (comparator_bf16 if bf16 else comparator_f32)(cfg, params, feat, xy, idx, phase2)
    want = expected_moment(cfg, ref, params, phase2)
    m_cmp = moment_of(cfg, cmp_, params, phase2)
    yard = {label: ratios(w, s, m_cmp[label])[:2] for label, (w, s) in want.items()}
    if not bf16:
        # The maximum of a float32 evaluation is, in the tensors whose last contraction has few terms (grid entries, rows of
        # G with one sample), set by ONE element: one whose d_enc / d_pred cancels to nearly nothing, so that the error it
        # inherits from its own contraction is large in units of the little that is left.  Which evaluation order loses
        # most THERE is luck, so the comparator's maximum is the worst of MAX_ORDERS equally valid float32 evaluations;
        # the L2 figure, an average, is the plain order's.
        # MAX_ORDERS follows from arithmetic alone, not from any kernel's result.  The error of that one element is, in
        # a correct evaluation, a draw X ~ N(0, s^2) with s its inherited (upstream) error; the comparators' are draws Y_1..n of
        # the same law.  A correct kernel misses "4 x the comparator's maximum" with probability
        #     P(|X| > 4 max_n |Y|) = E[erf(|X| / (4 sqrt 2))^n] = 1.6e-1, 3.7e-2, 3.9e-3, 1.3e-4 for n = 1, 2, 4, 8.
        # The GPU file holds 4 shapes x 4 fits x (3 such tensors in phase 1 + 2 in phase 2) + 8 in-call = 88 such
        # (tensor, input) pairs, each under up to four different summation orders of the library (sorted gather, atomics,
        # layer launches, batched fits): ~350 draws.  The smallest power of two at which a correct library fails the file
        # less than one time in ten is n = 8 (350 x 1.3e-4 = 0.05; n = 4 gives 1.4 expected false failures, n = 1 gives 55).
        # What this costs in sharpness is measured, not argued: profiles/fit_grads/README.md, break checks on the fp32 cases.
        for seed in range(1, MAX_ORDERS):
            alt = moment_of(cfg, _chain(cfg, params, feat, xy, idx, phase2, "f32", order_seed=seed), params, phase2)
            for label, (w, s) in want.items():
                yard[label] = (yard[label][0], max(yard[label][1], ratios(w, s, alt[label])[1]))
    return ref, want, yard, loss_ratios(ref, cmp_)
