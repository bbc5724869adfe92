"""Plain torch references of the exact-fp32 trainer kernels behind include/dvt_parts.h, and the seeded inputs of their tests.

Every `ref_*` function evaluates ONE kernel's operation from the formulas in the comment above that kernel, in the dtype of
the tensors it is given: float64 is the reference, float32 (ordinary CPU torch) is the yardstick of what fp32 arithmetic
itself loses.  It returns {output name: (value, mag, L)}:

  value  the result
  mag    the same expression with every term replaced by its absolute value -- and, where the element depends on a row
         statistic (a mean, an rstd, a norm), that statistic's own magnitude carried through to first order
  L      the longest reduction that feeds an element of this output

A row / elementwise kernel is held to  c * L * u * mag  per element, u = 2^-24, c = max(1, 4 * c_ref) with
c_ref = max |f32 - f64| / (L u mag) measured here on the same inputs (`yardstick`).  The factor 4: the device uses erff,
__expf and the hardware exp2 (about 2 ulp against libm's <= 1) and tree-ordered wave sums where the CPU sums in its own
order; it is a margin over the reference's own fp32 error, not a fitted number.

Contractions are held to the a-priori bound of an fp32 FMA chain in any order, (K + S + 4) u (|A| . |B|) (+ 2 u |bias|),
S = number of k-splits (`gemm_tol`); a function of a contraction gets that bound pushed through the function's derivative
to first order plus c u |ref|.

The `*_inputs` functions build the CPU float32 inputs (seeded, scaled so that nothing overflows fp32);
tests/test_parts_reference_cpu.py checks the references against torch itself and the conditions on the inputs,
tests/test_gpu_parts.py compares the kernels.
"""
import math

import torch

U = 2.0 ** -24
DIMS = (384, 768, 1024)
LN_EPS = 1e-6


MAG_FLOOR = 2e-30  # an element that is exactly zero in any arithmetic (gelu(0), P = 0) keeps a non-zero tolerance


def _floor(out):
    return {k: (v, mag.clamp_min(MAG_FLOOR), L) for k, (v, mag, L) in out.items()}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).float()


def cast(inp, dt):
    """The inputs in dtype dt (None and non-floating entries unchanged)."""
    return {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in inp.items()}


def yardstick(ref, inp):
    """{output: c_ref}: the error of the SAME expression in float32 CPU torch against float64, in units of L u mag."""
    r64, r32 = ref(cast(inp, torch.float64)), ref(cast(inp, torch.float32))
    out = {}
    for k, (v, mag, L) in r64.items():
        d = (r32[k][0].double() - v).abs()
        out[k] = float((d / (L * U * mag)).max()) if v.numel() else 0.0
    return out


def row_tol(ref64, c_ref):
    """{output: per-element tolerance}  c * L * u * mag, c = max(1, 4 c_ref)."""
    return {k: max(1.0, 4.0 * c_ref[k]) * L * U * mag for k, (v, mag, L) in ref64.items()}


def gemm_tol(absprod, K, splits=1, bias=None):
    t = (K + splits + 4) * U * absprod
    return t if bias is None else t + 2 * U * bias.abs()


def ex_splits(M, N, K, accumulate):
    """k-split of dvt_gemm_f32_ex (unbatched): (splits, k-tiles of each split); restated from dvt_gemm_f32_glds.hip."""
    ktiles = K // 64
    if not accumulate:
        return 1, [ktiles]
    tiles = -(-M // 64) * -(-N // 64)
    s = max(1, min(-(-1024 // tiles), ktiles // 4))
    chunk = -(-ktiles // s)
    n = -(-ktiles // chunk)
    return n, [min(chunk, ktiles - i * chunk) for i in range(n)]


def wgrad_big_splits(rows, n, k):
    """k-split of dvt_linear_wgrad_big with accumulate: (splits, 32-row tiles of each split)."""
    ktiles = rows // 32
    tiles = (n // 128) * (k // 128)
    s = max(1, min(-(-1024 // tiles), ktiles // 8))
    chunk = -(-ktiles // s)
    cnt = -(-ktiles // chunk)
    return cnt, [min(chunk, ktiles - i * chunk) for i in range(cnt)]


# ------------------------------------------------------------------------------------------------ LayerNorm backward
def ln_bwd_inputs(C, R, seed, zero_rows=3):
    g = gen(seed)
    x = randn(g, R, C) * (0.5 + torch.rand(R, 1, generator=g) * 2) + randn(g, R, 1)
    x64 = x.double()
    mean = x64.mean(1)
    rstd = 1.0 / torch.sqrt(x64.var(1, unbiased=False) + LN_EPS)
    mean, rstd = mean.float(), rstd.float()
    zr = [r for r in (0, R // 2, R - 1)][:zero_rows] if R >= 3 else []
    for r in set(zr):  # as padded rows are kept: mean = rstd = 0
        mean[r] = 0.0
        rstd[r] = 0.0
    return dict(dy=randn(g, R, C), x=x, mean=mean, rstd=rstd, gamma=1.0 + randn(g, C, scale=0.3), dres=randn(g, R, C),
                dgamma0=randn(g, C), dbeta0=randn(g, C), zero_rows=sorted(set(zr)))


def ref_ln_bwd(i, with_dres=True):
    dy, x, mu, rs, gm = i["dy"], i["x"], i["mean"][:, None], i["rstd"][:, None], i["gamma"]
    R, C = x.shape
    xh = (x - mu) * rs
    xh_mag = (x.abs() + mu.abs()) * rs
    g = dy * gm
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    m1m, m2m = g.abs().mean(1, keepdim=True), (g.abs() * xh_mag).mean(1, keepdim=True)
    dres = i["dres"] if with_dres else torch.zeros_like(x)
    dx = dres + rs * (g - m1 - xh * m2)
    dx_mag = dres.abs() + rs * (g.abs() + m1m + xh_mag * m2m)
    dg = i["dgamma0"] + (dy * xh).sum(0)
    dg_mag = i["dgamma0"].abs() + (dy.abs() * xh_mag).sum(0)
    db = i["dbeta0"] + dy.sum(0)
    db_mag = i["dbeta0"].abs() + dy.abs().sum(0)
    return _floor({"dx": (dx, dx_mag, C), "dgamma": (dg, dg_mag, R + 1), "dbeta": (db, db_mag, R + 1)})


# ------------------------------------------------------------------------------------- (a [+ b | + ls f]) -> LayerNorm
def add_ln_inputs(C, seed, T=5, Tp=8, batch=2, offset=False):
    g = gen(seed)
    R = batch * Tp
    sc = 1.0
    a_pad, b_pad, f_pad = randn(g, R, C, scale=sc), randn(g, R, C, scale=sc), randn(g, R, C, scale=sc)
    if offset:  # rows of mean 100 and deviation 1: a one-pass variance loses them
        a_pad = a_pad + 100.0
        b_pad = b_pad * 0.0
        f_pad = f_pad * 0.01
    return dict(a_pad=a_pad, a_packed=randn(g, batch, T, C) + (100.0 if offset else 0.0), b_pad=b_pad,
                pos=randn(g, T, C, scale=0.0 if offset else 1.0), f=f_pad, ls=randn(g, C, scale=0.5),
                gamma=1.0 + randn(g, C, scale=0.3), beta=randn(g, C, scale=0.3), T=T, Tp=Tp, batch=batch)


def _ln_rows(x, x_mag, gamma, beta, C):
    """LayerNorm of the rows x (two passes, 1 / sqrt(var + eps)) with first-order magnitudes."""
    mu = x.mean(1, keepdim=True)
    mu_mag = x_mag.mean(1, keepdim=True)
    d = x - mu
    d_mag = x_mag + mu_mag
    var = (d * d).mean(1, keepdim=True)
    var_mag = (2 * d.abs() * d_mag).mean(1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + LN_EPS)
    rs_mag = rs + 0.5 * rs ** 3 * var_mag
    xn = d * rs * gamma + beta
    xn_mag = (d_mag * rs + d.abs() * rs_mag) * gamma.abs() + beta.abs()
    return xn, xn_mag, mu[:, 0], mu_mag[:, 0], rs[:, 0], rs_mag[:, 0]


def _valid_rows(T, Tp, batch):
    return (torch.arange(batch * Tp) % Tp) < T


def ref_add_ln(i, mode):
    """mode: 'packed_pos' (a packed + pos_embed), 'pad_pad' (padded a + padded b), 'no_b' (padded a alone),
    'ls' (padded a + ls (.) f, dvt_parts_ls_add_ln), 'no_ls' (padded a alone through dvt_parts_ls_add_ln)."""
    T, Tp, batch = i["T"], i["Tp"], i["batch"]
    C = i["gamma"].shape[0]
    valid = _valid_rows(T, Tp, batch)
    if mode == "packed_pos":
        a = torch.zeros(batch, Tp, C, dtype=i["gamma"].dtype)
        a[:, :T] = i["a_packed"]
        b = torch.zeros_like(a)
        b[:, :T] = i["pos"]
        a, b = a.reshape(-1, C), b.reshape(-1, C)
    elif mode == "pad_pad":
        a, b = i["a_pad"], i["b_pad"]
    elif mode in ("no_b", "no_ls"):
        a, b = i["a_pad"], torch.zeros_like(i["a_pad"])
    else:
        a, b = i["a_pad"], i["ls"] * i["f"]
    x, x_mag = a + b, a.abs() + b.abs()
    x, x_mag = x[valid], x_mag[valid]
    xn, xn_mag, mu, mu_mag, rs, rs_mag = _ln_rows(x, x_mag, i["gamma"], i["beta"], C)

    def full(v, fill=0.0):
        o = torch.full((batch * Tp, *v.shape[1:]), fill, dtype=v.dtype)
        o[valid] = v
        return o
    # padded rows are exactly zero: their magnitude is irrelevant (compared with ==), 1 keeps the tolerance finite
    return _floor({"sum": (full(x), full(x_mag, 1.0), 2), "xn": (full(xn), full(xn_mag, 1.0), C), "mean": (full(mu), full(mu_mag, 1.0), C),
            "rstd": (full(rs), full(rs_mag, 1.0), C)})


# ------------------------------------------------------------------------------------------------ LayerScale backward
def ls_bwd_inputs(C, R, seed):
    g = gen(seed)
    return dict(dy=randn(g, R, C), f=randn(g, R, C), ls=randn(g, C, scale=0.5), dls0=randn(g, C))


def ref_ls_bwd(i):
    R = i["dy"].shape[0]
    df = i["ls"] * i["dy"]
    dls = i["dls0"] + (i["f"] * i["dy"]).sum(0)
    dls_mag = i["dls0"].abs() + (i["f"].abs() * i["dy"].abs()).sum(0)
    return _floor({"df": (df, df.abs(), 1), "dls": (dls, dls_mag, R + 1)})


# ------------------------------------------------------------------------------------------------------------- GELU
def gelu_inputs(seed, n=4000):
    g = gen(seed)
    special = torch.tensor([0.0, -0.0, 1e-4, -1e-4, 1.0, -1.0, 8.0, -8.0, 30.0, -30.0])
    h = randn(g, n, scale=2.0)
    h[:special.numel()] = special
    h[-special.numel():] = special.flip(0)
    return dict(h=h, da=randn(g, n))


def ref_gelu(i):
    h = i["h"]
    e = torch.erf(h / math.sqrt(2.0))
    v = 0.5 * h * (1.0 + e)
    return _floor({"a": (v, 0.5 * h.abs() * (1.0 + e.abs()), 2)})


def ref_gelu_bwd(i):
    h, da = i["h"], i["da"]
    cdf = 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * h * h) / math.sqrt(2.0 * math.pi)
    cdf_mag = 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)).abs())
    v = da * (cdf + h * pdf)
    # exp(-h^2 / 2) carries the rounding of its argument: relative error h^2 / 2 u on top of its own
    mag = da.abs() * (cdf_mag + h.abs() * pdf * (1.0 + 0.5 * h * h))
    return _floor({"da": (v, mag, 3)})


# ------------------------------------------------------------------------------------------- fallback softmax passes
def softmax_inputs(seed, Tp=64, T=49, nb=4):
    g = gen(seed)
    S = randn(g, nb, Tp, Tp, scale=8.0)  # logits scale * S of a few units
    P = torch.zeros(nb, Tp, Tp, dtype=torch.float64)
    P[:, :T, :T] = torch.softmax(0.125 * S[:, :T, :T].double(), -1)
    return dict(S=S, P=P.float(), dP=randn(g, nb, Tp, Tp), T=T, Tp=Tp, scale=0.125)


def ref_softmax(i):
    T, Tp, sc = i["T"], i["Tp"], i["scale"]
    z = sc * i["S"][:, :T, :T]
    p = torch.softmax(z, -1)
    out = torch.zeros_like(i["S"])
    out[:, :T, :T] = p
    # exp(z - m) carries the rounding of its argument (|z| + |m|) u; the row sum has T terms
    m = z.max(-1, keepdim=True).values
    mag = torch.ones_like(i["S"])
    mag[:, :T, :T] = p * (1.0 + (z.abs() + m.abs()) / T)
    return _floor({"P": (out, mag, T)})


def ref_softmax_bwd(i):
    Tp, sc = i["Tp"], i["scale"]
    P, dP = i["P"], i["dP"]
    dot = (P * dP).sum(-1, keepdim=True)
    dot_mag = (P * dP.abs()).sum(-1, keepdim=True)
    v = sc * P * (dP - dot)
    mag = sc * P * (dP.abs() + dot_mag)
    return _floor({"dS": (v, mag, Tp)})


# ------------------------------------------------------------------------------------------------------------ rowdot
def rowdot_inputs(C, seed, Tp=3, R=6):
    g = gen(seed)
    return dict(dO=randn(g, R, C), O=randn(g, R, C), Tp=Tp)


def ref_rowdot(i):
    dO, O, Tp = i["dO"], i["O"], i["Tp"]
    R, C = dO.shape
    H = C // 64
    v = (dO * O).reshape(R // Tp, Tp, H, 64).sum(-1).permute(0, 2, 1)  # [b][h][t]
    mag = (dO.abs() * O.abs()).reshape(R // Tp, Tp, H, 64).sum(-1).permute(0, 2, 1)
    return _floor({"D": (v.reshape(-1), mag.reshape(-1), 64)})


# -------------------------------------------------------------------------------------------------------------- loss
def loss_inputs(C, seed, n_prefix, T=9, Tp=12, batch=2):
    g = gen(seed)
    R = batch * Tp
    tgt = randn(g, batch, T - n_prefix, C)
    tgt[0, 1] = 0.0  # an all-zero target row: the 1e-8 clamp of its norm
    return dict(a=randn(g, R, C), b=randn(g, R, C, scale=0.5), target=tgt, n_prefix=n_prefix, T=T, Tp=Tp, batch=batch)


def ref_loss(i, add, norm_batch):
    T, Tp, batch, npf = i["T"], i["Tp"], i["batch"], i["n_prefix"]
    C = i["a"].shape[1]
    o_all = i["a"] + i["b"] if add else i["a"]
    o_mag_all = i["a"].abs() + i["b"].abs() if add else i["a"].abs()
    o = o_all.reshape(batch, Tp, C)[:, npf:T]
    o_mag = o_mag_all.reshape(batch, Tp, C)[:, npf:T]
    t = i["target"]
    N = float(norm_batch * (T - npf))
    d = o - t
    d_mag = o_mag + t.abs()
    se = (d * d).sum()
    se_mag = (2 * d.abs() * d_mag).sum()
    no_raw, nt_raw = o.norm(dim=-1, keepdim=True), t.norm(dim=-1, keepdim=True)
    no, nt = no_raw.clamp_min(1e-8), nt_raw.clamp_min(1e-8)
    ot = (o * t).sum(-1, keepdim=True)
    ot_mag = (o_mag * t.abs()).sum(-1, keepdim=True)
    cos = ot / (no * nt)
    # first order: |o|, |t| are sums of squares (relative error of a norm <= that of its square); o itself may carry its add
    no_rel = (o.abs() * o_mag).sum(-1, keepdim=True) / (no * no)
    cos_mag = ot_mag / (no * nt) + cos.abs() * (no_rel + 1.0)
    l2 = se / (N * C)
    cl = 1.0 - cos.sum() / N
    l2_mag, cl_mag = se_mag / (N * C), 1.0 + cos_mag.sum() / N
    loss3 = torch.stack([l2 + cl, l2, cl, torch.zeros_like(l2)])
    loss3_mag = torch.stack([l2_mag + cl_mag, l2_mag, cl_mag, torch.ones_like(l2)])
    kt, ko = 1.0 / (N * no * nt), cos / (N * no * no)
    kt_mag, ko_mag = kt * (1.0 + no_rel), (cos_mag + 2 * cos.abs() * no_rel) / (N * no * no)
    gq = 2.0 * d / (N * C) - (kt * t - ko * o)
    gq_mag = 2.0 * d_mag / (N * C) + kt_mag * t.abs() + ko_mag * o.abs() + ko.abs() * o_mag
    dout = torch.zeros(batch, Tp, C, dtype=o.dtype)
    dout[:, npf:T] = gq
    dmag = torch.ones(batch, Tp, C, dtype=o.dtype)
    dmag[:, npf:T] = gq_mag
    return _floor({"dout": (dout.reshape(-1, C), dmag.reshape(-1, C), C), "out": (o.reshape(-1, C), o_mag.reshape(-1, C), 2),
            "loss": (loss3, loss3_mag, batch * (T - npf) * C)})


# ---------------------------------------------------------------------------- pos_embed gradient and the token assembly
def embed_inputs(seed, n_prefix, pos_has_cls, dim=384, batch=3, gh=2, gw=3, s_pad=128):
    g = gen(seed)
    n_tokens = n_prefix + gh * gw
    return dict(y=randn(g, batch * s_pad, dim), prefix=randn(g, n_prefix, dim), pos=randn(g, pos_has_cls + gh * gw, dim),
                dx=randn(g, batch * s_pad, dim), dprefix0=randn(g, n_prefix, dim), dpos0=randn(g, pos_has_cls + gh * gw, dim),
                n_prefix=n_prefix, n_tokens=n_tokens, s_pad=s_pad, pos_has_cls=pos_has_cls, batch=batch)


def ref_embed(i):
    npf, nt, sp, hc, B = i["n_prefix"], i["n_tokens"], i["s_pad"], i["pos_has_cls"], i["batch"]
    dim = i["y"].shape[1]
    y = i["y"].reshape(B, sp, dim)
    x = torch.zeros_like(y)
    mag = torch.ones_like(y)
    x[:, :npf] = i["prefix"]
    mag[:, :npf] = i["prefix"].abs()
    if hc:
        x[:, 0] = x[:, 0] + i["pos"][0]
        mag[:, 0] = mag[:, 0] + i["pos"][0].abs()
    x[:, npf:nt] = y[:, npf:nt] + i["pos"][hc:]
    mag[:, npf:nt] = y[:, npf:nt].abs() + i["pos"][hc:].abs()
    return _floor({"x": (x.reshape(-1, dim), mag.reshape(-1, dim), 2)})


def ref_embed_bwd(i):
    npf, nt, sp, hc, B = i["n_prefix"], i["n_tokens"], i["s_pad"], i["pos_has_cls"], i["batch"]
    dim = i["dx"].shape[1]
    dx = i["dx"].reshape(B, sp, dim)
    s, sm = dx.sum(0), dx.abs().sum(0)
    dprefix, dpm = i["dprefix0"] + s[:npf], i["dprefix0"].abs() + sm[:npf]
    dpos, dposm = i["dpos0"].clone(), i["dpos0"].abs()
    if hc:
        dpos[0] = dpos[0] + s[0]
        dposm[0] = dposm[0] + sm[0]
    dpos[hc:] = dpos[hc:] + s[npf:nt]
    dposm[hc:] = dposm[hc:] + sm[npf:nt]
    dxo = dx.clone()
    dxo[:, :npf] = 0
    return _floor({"dx": (dxo.reshape(-1, dim), torch.ones_like(i["dx"]), 1), "dprefix": (dprefix, dpm, B + 1), "dpos": (dpos, dposm, B + 1)})


def pos_grad_inputs(seed, C=384, batch=3, T=7, Tp=128):
    g = gen(seed)
    return dict(dx=randn(g, batch * Tp, C), dpos0=randn(g, T, C), T=T, Tp=Tp, batch=batch)


def ref_pos_grad(i):
    T, Tp, B = i["T"], i["Tp"], i["batch"]
    C = i["dx"].shape[1]
    dx = i["dx"].reshape(B, Tp, C)[:, :T]
    return _floor({"dpos": (i["dpos0"] + dx.sum(0), i["dpos0"].abs() + dx.abs().sum(0), B + 1)})


# ------------------------------------------------------------------------------------------------------------ im2col
IM2COL = dict(patch=14, stride=7, img_h=28, img_w=35, k_patch=640, n_prefix=5, s_pad=128, batch=2)


def im2col_inputs(seed):
    g = gen(seed)
    c = dict(IM2COL)
    c["grid_h"] = (c["img_h"] - c["patch"]) // c["stride"] + 1
    c["grid_w"] = (c["img_w"] - c["patch"]) // c["stride"] + 1
    c["img"] = randn(g, c["batch"], 3, c["img_h"], c["img_w"])
    return c


def ref_im2col(i):
    """col [batch * s_pad][k_patch]: a copy, so L = 1 and the comparison is exact."""
    B, sp, kp, npf, p = i["batch"], i["s_pad"], i["k_patch"], i["n_prefix"], i["patch"]
    n = i["grid_h"] * i["grid_w"]
    col = torch.zeros(B, sp, kp, dtype=i["img"].dtype)
    for b in range(B):
        for py in range(i["grid_h"]):
            for px in range(i["grid_w"]):
                y0, x0 = py * i["stride"], px * i["stride"]
                col[b, npf + py * i["grid_w"] + px, :3 * p * p] = i["img"][b, :, y0:y0 + p, x0:x0 + p].reshape(-1)
    assert npf + n <= sp
    return _floor({"col": (col.reshape(-1, kp), torch.ones(B * sp, kp, dtype=col.dtype), 1)})


# ------------------------------------------------------------------------------------------------- attention rows
ATTN_PADS = [(128, 1), (128, 31), (128, 33), (128, 100), (128, 128), (256, 129), (256, 200)]


def attn_inputs(Tp, T, seed, late_key=False, batch=2, heads=2):
    """qkv [batch * Tp][3 C] (q | k | v), padded rows random too (the kernel masks by index, not by value).
    late_key: the key in the LAST valid position of every (image, head) scaled so that its logit tops every query's running
    maximum by more than 40."""
    g = gen(seed)
    C = heads * 64
    qkv = randn(g, batch, Tp, 3 * C)
    if late_key:
        # every query gets the component 4 along d = 0 of its head (the rest scaled to 0.3), the key in the LAST valid position
        # is 100 e_0: its logit is 0.125 * 4 * 100 = 50 for every query while every other key's stays within a few units --
        # the running maximum jumps by more than 40 at the last valid key, and exp(-50 -+ few) stays far above 1e-30
        qkv[:, :, :C] *= 0.3
        qkv[:, :, 0:C:64] = 4.0
        qkv[:, T - 1, C:2 * C] = 0.0
        qkv[:, T - 1, C:2 * C:64] = 100.0
    return dict(qkv=qkv.reshape(batch * Tp, 3 * C), T=T, Tp=Tp, batch=batch, heads=heads, scale=0.125)


def ref_attn_fwd(i):
    """P [batch][heads][Tp][Tp], its tolerance parts: the logits' |q|.|k| (for the contraction bound) and P."""
    T, Tp, B, H, sc = i["T"], i["Tp"], i["batch"], i["heads"], i["scale"]
    C = H * 64
    qkv = i["qkv"].reshape(B, Tp, 3 * C)
    q = qkv[:, :, :C].reshape(B, Tp, H, 64).permute(0, 2, 1, 3)
    k = qkv[:, :, C:2 * C].reshape(B, Tp, H, 64).permute(0, 2, 1, 3)
    z = sc * (q[:, :, :T] @ k[:, :, :T].transpose(-1, -2))
    zabs = sc * (q[:, :, :T].abs() @ k[:, :, :T].abs().transpose(-1, -2))
    p = torch.softmax(z, -1)
    P = torch.zeros(B, H, Tp, Tp, dtype=z.dtype)
    P[:, :, :T, :T] = p
    return P, z, zabs


def attn_fwd_tol(i64, c):
    """Per-element tolerance of mode 0: the logits' contraction bound dz = (64 + 1 + 4) u scale |q|.|k| pushed through the
    softmax (dp_j = p_j (dz_j - sum_i p_i dz_i), so |dp_j| <= p_j (dz_j + sum_i p_i dz_i)) plus c u p."""
    P, z, zabs = ref_attn_fwd(i64)
    T = i64["T"]
    dz = gemm_tol(zabs, 64)
    p = P[:, :, :T, :T]
    tol = torch.zeros_like(P)
    tol[:, :, :T, :T] = p * (dz + (p * dz).sum(-1, keepdim=True)) + c * U * p
    return P, tol


def softmax_cref(z32):
    """c_ref of the softmax alone, L = 1, mag = p: float32 softmax of the float32-rounded logits against float64 of the same."""
    p64 = torch.softmax(z32.double(), -1)
    p32 = torch.softmax(z32, -1)
    return float(((p32.double() - p64).abs() / (U * p64.clamp_min(1e-300))).max())


def attn_bwd_inputs(Tp, T, seed, batch=2, heads=2):
    i = attn_inputs(Tp, T, seed, batch=batch, heads=heads)
    g = gen(seed + 1000)
    C = heads * 64
    P, _, _ = ref_attn_fwd(cast(i, torch.float64))
    i["P"] = P.float()  # the fp64 softmax rounded to fp32, its padding zeros kept
    i["dao"] = randn(g, batch * Tp, C)
    i["D"] = randn(g, batch, heads, Tp)
    return i


def ref_attn_bwd(i):
    """dS = scale P (.) (dao v^T - D) over ALL Tp x Tp (P's zeros make the padding zero); returns dS, the |dao|.|v|."""
    Tp, B, H, sc = i["Tp"], i["batch"], i["heads"], i["scale"]
    C = H * 64
    v = i["qkv"].reshape(B, Tp, 3 * C)[:, :, 2 * C:].reshape(B, Tp, H, 64).permute(0, 2, 1, 3)
    dao = i["dao"].reshape(B, Tp, H, 64).permute(0, 2, 1, 3)
    dp = dao @ v.transpose(-1, -2)
    dpabs = dao.abs() @ v.abs().transpose(-1, -2)
    D = i["D"][..., None]
    return sc * i["P"] * (dp - D), dp, dpabs


def ref_pmul(i):
    """The epilogue alone, elementwise: s * P * (acc - D) from an accumulator already rounded to fp32 (L = 1, mag = |ref|)."""
    v = i["s"] * i["P"] * (i["acc"] - i["D"])
    return _floor({"dS": (v, v.abs(), 1)})


def pmul_tol(s, P, acc, accabs, D, K=64):
    """s P (.) (acc - D), acc a K-term contraction: its bound through the derivative s P, plus c u |ref| with c from the float32
    CPU evaluation of the epilogue on the fp32-rounded accumulator.  All arguments fp64; returns (ref, tol)."""
    c_ref = yardstick(ref_pmul, dict(s=torch.tensor(s), P=P.float(), acc=acc.float(), D=D.float()))["dS"]
    ref = s * P * (acc - D)
    return ref, s * P.abs() * gemm_tol(accabs, K) + max(1.0, 4.0 * c_ref) * U * ref.abs()


def attn_bwd_tol(i64):
    dS, dp, dpabs = ref_attn_bwd(i64)
    ref, tol = pmul_tol(i64["scale"], i64["P"], dp, dpabs, i64["D"][..., None].expand_as(dp))
    assert torch.equal(ref, dS)
    return dS, tol

# ------------------------------------------------------------------------------------------------------ contractions
def gemm_inputs(M, N, K, seed, nb=1):
    """C = A . Bm with A [nb][M][K], Bm [nb][K][N] (the tests lay them out in memory as each layout wants them)."""
    g = gen(seed)
    return dict(A=randn(g, nb, M, K), Bm=randn(g, nb, K, N, scale=K ** -0.5), bias=randn(g, N, scale=0.3), C0=randn(g, nb, M, N),
                colsum0=randn(g, M), gamma=randn(g, N, scale=0.5))


def ref_gemm(i, bias=False, accumulate=False):
    """(C, |A|.|B| (+ |C0|), colsum, its magnitude) in the dtype of the inputs."""
    c = i["A"] @ i["Bm"]
    mag = i["A"].abs() @ i["Bm"].abs()
    if bias:
        c = c + i["bias"]
    if accumulate:
        c = c + i["C0"]
        mag = mag + i["C0"].abs()
    cs = i["colsum0"] + i["A"][0].sum(1)
    cs_mag = i["colsum0"].abs() + i["A"][0].abs().sum(1)
    return c, mag, cs, cs_mag


def gelu_parts(v):
    """gelu(v), its elementwise magnitude (ref_gelu) and |gelu'(v)|."""
    e = torch.erf(v / math.sqrt(2.0))
    cdf = 0.5 * (1.0 + e)
    pdf = torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)
    return 0.5 * v * (1.0 + e), (0.5 * v.abs() * (1.0 + e.abs())).clamp_min(MAG_FLOOR), (cdf + v * pdf).abs()


# ------------------------------------------------------------------------------ the cases both test files walk through
GEMM_EX_CASES = [  # unbatched: (layout, M, N, K, bias, accumulate + colsum)
    (0, 100, 72, 64, True, False), (0, 100, 72, 64, False, False), (0, 100, 72, 192, True, False), (0, 100, 72, 192, False, False),
    (1, 100, 128, 128, False, False), (2, 64, 128, 576, False, True), (2, 64, 128, 128, False, True)]
BIG_EPI_SHAPES = [(m, n, k) for m in (128, 256) for n in (128, 256) for k in (32, 96)]
BIG_FALLBACK_SHAPES = [(192, 128, 64), (128, 128, 36)]  # not the 128 x 128 tile: the 64 x 64 LDS-DMA kernel / the register-staged one
LIN_SHAPES = [(128, 256, 128), (544, 128, 128), (64, 128, 64)]  # (R, n, k)
LIN_MASKS = [63, 0, 31]
LN_BWD_CASES = [(C, R) for C in DIMS for R in (1, 33, 70)]
ADD_LN_MODES = ["packed_pos", "pad_pad", "no_b", "no_sum"]  # dvt_parts_add_ln
LS_ADD_LN_MODES = ["ls", "no_ls", "no_sum"]  # dvt_parts_ls_add_ln
LOSS_CASES = [(C, add, npf, nb) for C in DIMS for add in (0, 1) for npf in (0, 5) for nb in (2, 4)]
EMBED_CASES = [(npf, hc) for npf in (1, 5) for hc in (0, 1)]
ROWDOT_DIMS = (128, 384, 1024)


def seed_of(*key):
    """One seed per case, the same in both test files."""
    h = 17
    for v in key:
        h = (h * 1000003 + (hash(v) if not isinstance(v, str) else sum(map(ord, v)))) % (2 ** 31 - 1)
    return h
