"""The key census of the extractor's attention kernels (csrc/dvt_vit_attn.hip, attention_f32_kernel in csrc/dvt_vit_f32.hip):
seeded CPU inputs, the float64 value, a per-element tolerance built from named terms, and CPU restatements of each method.

V IS A PROBE.  v[b, k, h, :] is zero except column d(k) = (k % 64 + 7 (k // 64) + 3 h) % 64, which holds w(k) = 1 + (k % 3) / 2
(exact in bf16).  out[q, d] is then the sum of the probabilities of the few keys that map to d, every term positive: no
cancellation, so the bound is RELATIVE per element, and a key that is dropped, duplicated, mis-masked or multiplied with another
tile's V^T moves one element by its whole share (1 / 22 of it at 1370 keys, all of it below 65 keys).  The shift 7 (k // 64)
gives every 64-key tile its own column order.  Pad keys (n_valid <= k < s_pad) hold K rows along the mean query, scaled so that
they would top the softmax of the mean query (by e^20, capped where a query's logit would leave the exp2 range) if let in, and V rows of 2^14 in every column.

One logit pattern per batch slot (`PATTERNS`), heads differ by seed:
  flat       q = 0: uniform weights, the value needs no transcendental function
  random     the distribution of tests/test_gpu_vit.py
  stairs     k and q share a direction: for the odd queries the tile maximum RISES by 12 (natural-log units) on every 64-key tile,
             for the even ones it falls by 12 -- both kinds in every wave, growth in consecutive tiles, and for the falling
             queries the late tiles' P underflow to 0
  spikes7.5 / spikes8.5   single dominant keys at in-tile offsets 3, 22, 41, 60 in tiles 1..4, the second-to-last and the last
             tile; queries i % 4 == 1 meet all of them, each RISE above the one before, queries i % 4 == 3 meet one each.  8.5 is
             past the 2980 row-sum vote of the deferred-max kernels (e^8.5 + 15 > 2980), 7.5 below it (P up to e^7.5 is formed
             against the old maximum and nothing is rescaled)
  massive+ / massive-     a common offset of +-60 on every logit of a row: the S chain starts from C = -m with |m| large

TOLERANCE, derived and not measured:  tol = e ref + 2^-100, per element, e per query row (`rel_bound`):
  dz    the error of one natural-log logit, from A = max_k sum_d |q_d k_d| (natural-log units) and M = max_k |z_k| >= |running max|
          log2q   67 u (M + A)            the S chain of 64 products started from C = -m: dvt_vit_attn.hip, A2_S `dst[mt] = L2D ? cinit`
          v2/f32  u (68 A + 3 M)          the chain from 0 (66 u A), then `fma(sv, l2e2, nmb2)` with mb = m_run * LOG2E rounded:
                                          one rounding of LOG2E, of mb and of the fma; the fp32 kernel's `qp[2 s] * (0.125f * LOG2E)`
                                          and `s[r] - m_new` are the same count
          x3      u (196 A + 3 M) + 2^-16 A   three chained products (A2_S, X3 branch) and what the method drops: q_lo k_lo
                                          and the two splits' residues (`split_pair`)
  e32 = 2 (dz + 4 u) + 2 (n_valid + 8) u    p_j = e^z_j / sum: a logit error enters numerator and denominator (2 dz); 4 u: the
                                          2-ulp `__builtin_amdgcn_exp2f` and the final `o * inv`; (n_valid + 8) u twice: the fp32
                                          sums `l_run += psum` and the P.V accumulators, any order
  bf16 kernels  e = 2 * 2^-8 + 4 e32        `pack2` of P and `pack2(o * inv)` of the output, one round-to-nearest-even each; l is
                                          summed from the unrounded P (`pv` before `pack()`), so the denominator adds none.  The
                                          factor 4 on e32 is parts_reference.py's margin (summation order, v_exp_f32); the bf16
                                          term gets none
  fp32 kernel   e = 4 e32
  bf16x3        e = 4 e32 + 2 * 2^-16       P = hi + lo (`lo2`) and V = hi + lo (v_split_transpose_kernel), each to 2^-16
  x3_presplit   ... + 2^-16                 the output's own split (`hh` / `ll` in the split_out branch)
"""
import functools

import torch

from tests.parts_reference import U, gen, seed_of

LN2 = 0.6931471805599453
LOG2E = 1.4426950408889634
Q_PRESCALE = 0.125 * LOG2E
FLOOR = 2.0 ** -100   # an element that is exactly zero (no key maps to its column, or P underflowed) keeps a non-zero tolerance
BF16 = 2.0 ** -8      # one round-to-nearest-even to bf16, as the issue counts it
X3 = 2.0 ** -16
V_PAD = 2.0 ** 14
PATTERNS = ("flat", "random", "stairs", "spikes7.5", "spikes8.5", "massive+", "massive-")
BIG_PATTERNS = ("flat", "random", "spikes8.5")   # the 1370-key shapes
SPIKE_OFFSETS = (3, 22, 41, 60)                  # the four lane groups (4 g + r of key % 16) and both k-halves
STAIR_STEP = 12.0
KERNELS = ("log2q", "v2", "f32", "x3", "x3_presplit")


def probe_column(k, h):
    return (k % 64 + 7 * (k // 64) + 3 * h) % 64


def probe_weight(k):
    return 1.0 + (k % 3) / 2.0


def spike_keys(n_valid):
    """[(tile, key)]: tiles 1..4 (every kt % 4), the second-to-last and the last, offsets cycling through SPIKE_OFFSETS
    (in a short last tile: the largest offset that is still a valid key)."""
    nt = -(-n_valid // 64)
    tiles = sorted({t for t in (1, 2, 3, 4, nt - 2, nt - 1) if 0 <= t < nt})
    out = []
    for i, t in enumerate(tiles):
        off = SPIKE_OFFSETS[i % 4]
        left = n_valid - 64 * t
        if off >= left:
            ok = [o for o in SPIKE_OFFSETS if o < left]
            off = ok[-1] if ok else left - 1
        out.append((t, 64 * t + off))
    return out


def _orthonormal(g, n):
    return torch.linalg.qr(torch.randn(64, n, generator=g, dtype=torch.float64))[0].T.float()  # [n][64]


def _pattern(name, n_valid, s_pad, g):
    """q [s_pad][64], k [s_pad][64] of one (image, head), float32; natural-log logit = 0.125 q . k."""
    q = torch.randn(s_pad, 64, generator=g)
    k = torch.randn(s_pad, 64, generator=g)
    i = torch.arange(s_pad)
    if name == "flat":
        q = torch.zeros(s_pad, 64)
    elif name == "random":
        k = k + torch.linspace(-1, 1, 64)
    elif name == "stairs":
        u = _orthonormal(g, 1)[0]
        nt = -(-n_valid // 64)
        a = STAIR_STEP * ((i // 64).float() - (nt - 1) / 2.0)          # the tile's level, centred: |logit| <= 12 * 4
        k = 0.5 * (k - (k @ u)[:, None] * u) + a[:, None] * u
        sign = torch.where(i % 2 == 1, 1.0, -1.0)
        q = 0.5 * (q - (q @ u)[:, None] * u) + 8.0 * sign[:, None] * u
    elif name.startswith("spikes"):
        rise = float(name[6:])
        sp = spike_keys(n_valid)
        w = _orthonormal(g, len(sp) + 1)
        k = k - (k @ w.T) @ w                                          # every other key: logit 0 for the spiked queries
        for n, (_, key) in enumerate(sp):
            k[key] = (n + 1) * rise * w[0] + rise * w[n + 1]
        q[i % 4 == 1] = 8.0 * w[0]                                     # meets every spike, each `rise` above the last
        for n in range(len(sp)):
            q[(i % 4 == 3) & ((i // 4) % len(sp) == n)] = 8.0 * w[n + 1]  # meets spike n alone
    elif name.startswith("massive"):
        u = torch.full((64,), 0.125)
        mu = 20.0 if name.endswith("+") else -20.0
        k = k - (k @ u)[:, None] * u + 24.0 * u                        # 0.125 * 20 * 24 = 60, the same for every key
        q = q + mu * u
    else:
        raise ValueError(name)
    # pad keys: along the mean valid query, 20 above the mean query's largest valid logit (and above 0), no query's logit beyond
    # 85 (inside the exp2 range), no component beyond 1e4
    qbar = q[:n_valid].mean(0)
    nrm2 = float(qbar @ qbar)
    if nrm2 > 0:
        c = (max(float((0.125 * k[:n_valid] @ qbar).max()), 0.0) + 20.0) / (0.125 * nrm2)
        c = min(c, 85.0 / max(float((0.125 * q @ qbar).abs().max()), 1e-30), 1e4 / float(qbar.abs().max()))
        k[n_valid:] = c * qbar
    else:
        k[n_valid:] = 100.0
    return q, k


@functools.lru_cache(maxsize=4)
def census_inputs(n_valid, s_pad, heads, patterns=PATTERNS):
    """q, k, v [batch][s_pad][heads][64] float32, batch = len(patterns)."""
    B = len(patterns)
    q = torch.empty(B, s_pad, heads, 64)
    k = torch.empty(B, s_pad, heads, 64)
    for b, name in enumerate(patterns):
        for h in range(heads):
            q[b, :, h], k[b, :, h] = _pattern(name, n_valid, s_pad, gen(seed_of("census", name, h, n_valid, s_pad)))
    v = torch.zeros(B, s_pad, heads, 64)
    key = torch.arange(s_pad)
    for h in range(heads):
        v[:, key, h, probe_column(key, h)] = probe_weight(key).float()
    v[:, n_valid:] = V_PAD
    return dict(q=q, k=k, v=v, n_valid=n_valid, s_pad=s_pad, heads=heads, patterns=tuple(patterns))


def operands(inp, kernel):
    """(the q, k, v a kernel is handed, the float64 q of the reference's natural-log logits q . k, float64 k, v)."""
    q, k, v = inp["q"], inp["k"], inp["v"]
    if kernel == "log2q":  # q pre-scaled by log2(e) / 8, one rounding to bf16: 2^(q' . k) = e^(ln 2 q' . k)
        qh, kh, vh = (q * Q_PRESCALE).bfloat16(), k.bfloat16(), v.bfloat16()
        return (qh, kh, vh), qh.double() * LN2, kh.double(), vh.double()
    if kernel == "v2":
        qh, kh, vh = q.bfloat16(), k.bfloat16(), v.bfloat16()
        return (qh, kh, vh), qh.double() * 0.125, kh.double(), vh.double()
    assert kernel in ("f32", "x3", "x3_presplit"), kernel
    return (q, k, v), q.double() * 0.125, k.double(), v.double()


def reference(qref, k64, v64, n_valid):
    """float64 softmax attention over the valid keys, for every query row (pad rows too).  out [B][S][H][64]; z, p [B][H][S][n];
    A = max_k sum_d |q_d k_d| and M = max_k |z_k| [B][H][S]."""
    kv = k64[:, :n_valid]
    z = torch.einsum("bqhd,bkhd->bhqk", qref, kv)
    A = torch.einsum("bqhd,bkhd->bhqk", qref.abs(), kv.abs()).amax(-1)
    m = z.amax(-1, keepdim=True)
    e = torch.exp(z - m)
    p = e / e.sum(-1, keepdim=True)
    out = torch.einsum("bhqk,bkhd->bqhd", p, v64[:, :n_valid])
    return dict(out=out, z=z, p=p, A=A, M=z.abs().amax(-1))


def rel_bound(ref, kernel, n_valid):
    """e [B][S][H][1] of the module docstring."""
    A, M = ref["A"], ref["M"]
    if kernel == "log2q":
        dz = 67 * U * (M + A)                    # A2_S: dst[mt] = cinit (-m), then 64 products
    elif kernel in ("v2", "f32"):
        dz = U * (68 * A + 3 * M)                # A2_S from zero4; softmax(): fma(sv, l2e2, nmb2), mb = m_run * LOG2E
    else:
        dz = U * (196 * A + 3 * M) + X3 * A      # A2_S, X3 branch: K_lo.Q_hi + K_hi.Q_lo + K_hi.Q_hi; lo.lo and the split residues dropped
    e32 = 2 * (dz + 4 * U) + 2 * (n_valid + 8) * U  # exp2f, o * inv; l_run += psum and the P.V MFMA chains
    if kernel in ("log2q", "v2"):
        e = 2 * BF16 + 4 * e32                   # pack(): P to bf16; the output's pack2(o * inv)
    elif kernel == "f32":
        e = 4 * e32
    else:
        e = 4 * e32 + 2 * X3                     # pack(), lo2: P = hi + lo; v_split_transpose_kernel: V = hi + lo
        if kernel == "x3_presplit":
            e = e + X3                           # split_out: hh / ll of o * inv
    return e.permute(0, 2, 1)[..., None]


def tolerance(ref, kernel, n_valid):
    return rel_bound(ref, kernel, n_valid) * ref["out"] + FLOOR


@functools.lru_cache(maxsize=2)
def case(kernel, n_valid, s_pad, heads, patterns=PATTERNS):
    """Everything one (kernel, shape) needs, computed once and shared: the inputs, the handed operands, reference, tolerance."""
    inp = census_inputs(n_valid, s_pad, heads, patterns)
    handed, qref, k64, v64 = operands(inp, "x3" if kernel == "x3_presplit" else kernel)
    ref = reference(qref, k64, v64, n_valid)
    return dict(inp=inp, handed=handed, ref=ref, tol=tolerance(ref, kernel, n_valid))


# ---------------------------------------------------------------------------------------------------- CPU restatements
def emulate_bf16(handed, n_valid, log2_domain):
    """The bf16 method on the CPU: fp32 logits, a running maximum that LAGS (exact on tile 0; later it grows, with a rescale of
    o and l, only where a P of the tile would pass e^8), P rounded to bf16 for P.V, l summed from the unrounded fp32 P, bf16
    output.  Per query row where the kernel votes per wave: a wave rescales more rows than this, exactly."""
    qh, kh, vh = handed
    B, S, H, _ = qh.shape
    q = qh.float().permute(0, 2, 1, 3)
    k = kh.float().permute(0, 2, 1, 3)[:, :, :n_valid]
    v = vh.float().permute(0, 2, 1, 3)[:, :, :n_valid]
    s = q @ k.transpose(-1, -2) if log2_domain else ((q * 0.125) @ k.transpose(-1, -2)) * LOG2E   # log2 units
    m = s[..., :64].amax(-1, keepdim=True)
    o = torch.zeros(B, H, S, 64)
    l = torch.zeros(B, H, S, 1)
    for t0 in range(0, n_valid, 64):
        st = s[..., t0:t0 + 64]
        d = (st.amax(-1, keepdim=True) - m).clamp_min(0.0)
        d = torch.where(d > 8.0 * LOG2E, d, torch.zeros_like(d))  # growth only past the vote
        alpha = torch.exp2(-d)
        o, l, m = o * alpha, l * alpha, m + d
        p = torch.exp2(st - m)
        l = l + p.sum(-1, keepdim=True)
        o = o + p.bfloat16().float() @ v[:, :, t0:t0 + 64]
    return (o / l).bfloat16().double().permute(0, 2, 1, 3)


def emulate_f32(handed, n_valid):
    q, k, v = (t.permute(0, 2, 1, 3) for t in handed)
    p = torch.softmax((q * 0.125) @ k[:, :, :n_valid].transpose(-1, -2), -1)
    return (p @ v[:, :, :n_valid]).double().permute(0, 2, 1, 3)


def emulate_x3(handed, n_valid):
    from oracle import bf16x3
    q, k, v = handed
    B, S, H, _ = q.shape
    out = torch.empty(B, S, H, 64, dtype=torch.float64)
    for b in range(B):
        for h in range(H):
            out[b, :, h] = bf16x3.attention_x3(q[b, :, h], k[b, :n_valid, h], v[b, :n_valid, h], 0.125).double()
    return out


def emulate(kernel, handed, n_valid):
    if kernel in ("log2q", "v2"):
        return emulate_bf16(handed, n_valid, kernel == "log2q")
    if kernel == "f32":
        return emulate_f32(handed, n_valid)
    out = emulate_x3(handed, n_valid)
    if kernel == "x3_presplit":
        from oracle import bf16x3
        hi, lo = bf16x3.split(out.float())
        out = hi.double() + lo.double()
    return out


def worst_ratio(got, c, n_valid):
    """max |got - ref| / tol over the valid query rows, per pattern: [batch]."""
    r = ((got - c["ref"]["out"]).abs() / c["tol"])[:, :n_valid]
    return r.nan_to_num(nan=float("inf")).amax(dim=(1, 2, 3))


# ------------------------------------------------------------------------------ the cases both test files walk through
def _up(n, m):
    return -(-n // m) * m


def _heads(t, r):
    return 2 + (t + r) % 2


BF16_SHAPES = [(64 * t + r, _up(64 * t + r, 32), _heads(t, r), PATTERNS) for t in range(9) for r in (1, 26, 32, 33, 63, 64)]
BF16_SHAPES += [(64 * t + r, _up(64 * t + r, 128), _heads(t, r + 1), PATTERNS) for t in (0, 1, 4) for r in (1, 26, 32, 33, 63, 64)
                if _up(64 * t + r, 128) != _up(64 * t + r, 32)]
BF16_SHAPES += [(1370, 1376, 3, BIG_PATTERNS), (1370, 1408, 2, BIG_PATTERNS), (1376, 1376, 3, BIG_PATTERNS)]
F32_SHAPES = [(32 * t + r, _up(32 * t + r, 32), _heads(t, r), PATTERNS) for t in range(6) for r in (1, 31, 32)]
F32_SHAPES += [(1370, 1376, 2, BIG_PATTERNS)]
X3_SHAPES = [(64 * t + r, _up(64 * t + r, 128), _heads(t, r), PATTERNS) for t in range(7) for r in (1, 32, 33, 64)]
X3_SHAPES += [(1370, 1408, 2, BIG_PATTERNS)]
SHAPES = {"log2q": BF16_SHAPES, "v2": BF16_SHAPES, "f32": F32_SHAPES, "x3": X3_SHAPES, "x3_presplit": X3_SHAPES}
# the developer library's kernels: one shape per tail kind (half, whole, 1 key) on whole 128-row blocks, and the 1370-key one
LAB_SHAPES = [(1, 128, 2, PATTERNS), (26 + 64, 128, 3, PATTERNS), (64 * 5 + 33, 384, 2, PATTERNS), (64 * 8 + 64, 640, 3, PATTERNS),
              (1370, 1408, 2, BIG_PATTERNS)]


def workgroups(n_valid, s_pad, heads, patterns, q_block=128):
    return -(-s_pad // q_block) * heads * len(patterns)


def shape_id(s):
    return f"n{s[0]}-s{s[1]}-h{s[2]}-b{len(s[3])}"
