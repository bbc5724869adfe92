"""CPU: the fp64 references of tests/parts_reference.py (what tests/test_gpu_parts.py holds the trainer kernels to).

(a) every reference that torch can differentiate or compute itself agrees with torch in fp64;
(b) the yardstick: the same expressions in ordinary float32 CPU torch, on the inputs and seeds of the GPU tests, stay within
    L u mag of fp64 (c_ref <= 1) -- so `mag` is a sound magnitude and the GPU tolerance c L u mag, c = max(1, 4 c_ref), is a
    margin over fp32 arithmetic itself; the worst c_ref per kernel is printed;
(c) the conditions on every input set: finite references inside fp32's range, every mag above 1e-30, every valid softmax row
    with a finite maximum.
"""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import parts_reference as pr

D = torch.float64
FMAX = 3.0e38


def close(a, b, rtol=1e-11, atol=1e-12):
    assert torch.allclose(a, b, rtol=rtol, atol=atol), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------- (a) references vs torch
@pytest.mark.parametrize("C", pr.DIMS)
def test_ln_bwd_is_autograd_of_layer_norm(C):
    i = pr.cast(pr.ln_bwd_inputs(C, 33, 5, zero_rows=0), D)
    x = i["x"].clone().requires_grad_(True)
    gamma = i["gamma"].clone().requires_grad_(True)
    beta = torch.zeros(C, dtype=D, requires_grad=True)
    i["mean"] = x.detach().mean(1)
    i["rstd"] = 1.0 / torch.sqrt(x.detach().var(1, unbiased=False) + pr.LN_EPS)
    F.layer_norm(x, (C,), gamma, beta, pr.LN_EPS).backward(i["dy"])
    r = pr.ref_ln_bwd(i)
    close(r["dx"][0], i["dres"] + x.grad)
    close(r["dgamma"][0], i["dgamma0"] + gamma.grad)
    close(r["dbeta"][0], i["dbeta0"] + beta.grad)
    close(pr.ref_ln_bwd(i, with_dres=False)["dx"][0], x.grad)


@pytest.mark.parametrize("mode", ["packed_pos", "pad_pad", "no_b", "ls", "no_ls"])
def test_add_ln_is_layer_norm_of_the_sum(mode):
    C = 384
    i = pr.cast(pr.add_ln_inputs(C, 3), D)
    T, Tp, B = i["T"], i["Tp"], i["batch"]
    r = pr.ref_add_ln(i, mode)
    if mode == "packed_pos":
        s = i["a_packed"] + i["pos"]
    else:
        add = {"pad_pad": i["b_pad"], "ls": i["ls"] * i["f"]}.get(mode, 0.0)
        s = (i["a_pad"] + add).reshape(B, Tp, C)[:, :T]
    want = torch.zeros(B, Tp, C, dtype=D)
    want[:, :T] = F.layer_norm(s, (C,), i["gamma"], i["beta"], pr.LN_EPS)
    close(r["xn"][0], want.reshape(-1, C))
    ws = torch.zeros(B, Tp, C, dtype=D)
    ws[:, :T] = s
    close(r["sum"][0], ws.reshape(-1, C))
    assert bool((r["mean"][0].reshape(B, Tp)[:, T:] == 0).all()) and bool((r["rstd"][0].reshape(B, Tp)[:, T:] == 0).all())
    close(r["mean"][0].reshape(B, Tp)[:, :T], s.mean(-1))


def test_softmax_and_its_backward_are_autograd():
    i = pr.cast(pr.softmax_inputs(1, Tp=16, T=16), D)
    S = i["S"].clone().requires_grad_(True)
    P = torch.softmax(i["scale"] * S, -1)
    close(pr.ref_softmax(i)["P"][0], P.detach())
    P.backward(i["dP"])
    i["P"] = P.detach()
    close(pr.ref_softmax_bwd(i)["dS"][0], S.grad)
    j = pr.cast(pr.softmax_inputs(1), D)  # T < Tp: padded rows and columns zero, valid rows sum to 1
    p = pr.ref_softmax(j)["P"][0]
    T = j["T"]
    assert bool((p[:, T:] == 0).all()) and bool((p[:, :, T:] == 0).all())
    close(p[:, :T].sum(-1), torch.ones(p.shape[0], T, dtype=D))


def test_gelu_and_its_gradient_are_autograd():
    i = pr.cast(pr.gelu_inputs(2), D)
    h = i["h"].clone().requires_grad_(True)
    a = F.gelu(h)
    close(pr.ref_gelu(i)["a"][0], a.detach())
    a.backward(i["da"])
    close(pr.ref_gelu_bwd(i)["da"][0], h.grad)
    v, mag, dv = pr.gelu_parts(i["h"])
    close(v, a.detach())
    close(dv * i["da"].abs(), h.grad.abs())
    assert bool((mag >= v.abs()).all())


def test_layerscale_is_autograd():
    i = pr.cast(pr.ls_bwd_inputs(384, 70, 4), D)
    f = i["f"].clone().requires_grad_(True)
    ls = i["ls"].clone().requires_grad_(True)
    (ls * f).backward(i["dy"])
    r = pr.ref_ls_bwd(i)
    close(r["df"][0], f.grad)
    close(r["dls"][0], i["dls0"] + ls.grad)


@pytest.mark.parametrize("add,npf,nb", [(1, 0, 2), (0, 5, 2), (0, 5, 4), (1, 5, 4)])
def test_loss_and_its_gradient_are_torch(add, npf, nb):
    C = 384
    i = pr.cast(pr.loss_inputs(C, 9, npf), D)
    T, Tp, B = i["T"], i["Tp"], i["batch"]
    a = i["a"].clone().requires_grad_(True)
    o = ((a + i["b"]) if add else a).reshape(B, Tp, C)[:, npf:T]
    r = pr.ref_loss(i, add, nb)
    if nb == B:  # the whole batch is here: exactly the reference's loss
        loss = F.mse_loss(o, i["target"]) + 1 - F.cosine_similarity(o, i["target"], dim=-1).mean()
    else:  # a slice of a batch of nb images: the sums over this slice's rows with the whole batch's normalisation
        n = nb * (T - npf)
        loss = ((o - i["target"]) ** 2).sum() / (n * C) + 1 - F.cosine_similarity(o, i["target"], dim=-1).sum() / n
    close(r["loss"][0][0], loss.detach())
    close(r["loss"][0][1] + r["loss"][0][2], r["loss"][0][0])
    loss.backward()
    close(r["dout"][0], a.grad, atol=1e-14)
    assert bool((r["dout"][0].reshape(B, Tp, C)[:, :npf] == 0).all()) and bool((r["dout"][0].reshape(B, Tp, C)[:, T:] == 0).all())
    close(r["out"][0], o.detach().reshape(-1, C))


def test_im2col_is_unfold():
    i = pr.cast(pr.im2col_inputs(6), D)
    r = pr.ref_im2col(i)["col"][0].reshape(i["batch"], i["s_pad"], i["k_patch"])
    p, npf, n = i["patch"], i["n_prefix"], i["grid_h"] * i["grid_w"]
    assert (i["grid_h"], i["grid_w"]) == (3, 4)
    want = F.unfold(i["img"], p, stride=i["stride"]).transpose(1, 2)  # [B][n][3 p p]
    assert torch.equal(r[:, npf:npf + n, :3 * p * p], want)
    assert bool((r[:, :npf] == 0).all()) and bool((r[:, npf + n:] == 0).all()) and bool((r[:, :, 3 * p * p:] == 0).all())


@pytest.mark.parametrize("npf,hc", pr.EMBED_CASES)
def test_embed_backward_is_autograd(npf, hc):
    i = pr.cast(pr.embed_inputs(7, npf, hc), D)
    y, prefix, pos = (i[k].clone().requires_grad_(True) for k in ("y", "prefix", "pos"))
    j = dict(i, y=y, prefix=prefix, pos=pos)
    x = pr.ref_embed(j)["x"][0]
    x.backward(i["dx"])
    r = pr.ref_embed_bwd(i)
    close(r["dprefix"][0], i["dprefix0"] + prefix.grad)
    close(r["dpos"][0], i["dpos0"] + pos.grad)
    B, sp = i["batch"], i["s_pad"]
    close(r["dx"][0].reshape(B, sp, -1)[:, npf:i["n_tokens"]], y.grad.reshape(B, sp, -1)[:, npf:i["n_tokens"]])
    assert bool((r["dx"][0].reshape(B, sp, -1)[:, :npf] == 0).all())
    g = pr.cast(pr.pos_grad_inputs(8), D)
    close(pr.ref_pos_grad(g)["dpos"][0], g["dpos0"] + g["dx"].reshape(g["batch"], g["Tp"], -1)[:, :g["T"]].sum(0))


def test_attention_references():
    i = pr.cast(pr.attn_bwd_inputs(128, 100, 11), D)
    P, z, zabs = pr.ref_attn_fwd(i)
    T, B, H, Tp = i["T"], i["batch"], i["heads"], i["Tp"]
    qkv = i["qkv"].reshape(B, Tp, 3, H, 64)
    q, k, v = (qkv[:, :T, j].transpose(1, 2) for j in range(3))
    want = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1)
    close(P[:, :, :T, :T], want)
    # dS of timm's attention by autograd: through P = softmax(S / 8), ao = P v with D = rowsum(dP (.) P)
    S = (q @ k.transpose(-1, -2)).clone().requires_grad_(True)
    Pa = torch.softmax(S * 0.125, -1)
    dao = i["dao"].reshape(B, Tp, H, 64)[:, :T].transpose(1, 2)
    (Pa @ v).backward(dao)
    dP = dao @ v.transpose(-1, -2)
    j = dict(i)
    j["P"] = P
    j["D"] = torch.zeros(B, H, Tp, dtype=D)
    j["D"][:, :, :T] = (dP * Pa.detach()).sum(-1)
    dS, _, _ = pr.ref_attn_bwd(j)
    close(dS[:, :, :T, :T], S.grad)
    assert bool((dS[:, :, T:] == 0).all()) and bool((dS[:, :, :, T:] == 0).all())
    d = pr.cast(pr.rowdot_inputs(384, 3), D)
    r = pr.ref_rowdot(d)["D"][0].reshape(2, 6, 3)
    close(r[1, 4, 2], (d["dO"][5, 256:320] * d["O"][5, 256:320]).sum())


def test_gemm_struct_mirror_size():
    """DvtPartsGemmEx is padded explicitly; dvt_gemm_f32_glds.hip asserts the same 160 bytes at compile time."""
    import ctypes
    from dvt_amd._lib import PartsGemmEx
    assert ctypes.sizeof(PartsGemmEx) == 160 and PartsGemmEx.oscale.offset == 152 and PartsGemmEx.sA0.offset == 88


def test_split_arithmetic_of_the_issue_cases():
    """The k-splits the GPU tests count on, restated from dvt_gemm_f32_ex / dvt_linear_wgrad_big."""
    assert pr.ex_splits(64, 128, 576, True) == (2, [5, 4])
    assert pr.ex_splits(64, 128, 128, True) == (1, [2])
    assert pr.ex_splits(128, 64, 64, True) == (1, [1])
    assert pr.wgrad_big_splits(544, 128, 128) == (2, [9, 8])
    assert pr.wgrad_big_splits(128, 256, 128) == (1, [4])


# ------------------------------------------------------------------------ (b) the yardstick and (c) the conditions
def row_cases():
    """(name, reference, inputs) of every row / elementwise case of the GPU tests."""
    for C, R in pr.LN_BWD_CASES:
        i = pr.ln_bwd_inputs(C, R, pr.seed_of("ln_bwd", C, R))
        yield f"ln_bwd C{C} R{R}", pr.ref_ln_bwd, i
        yield f"ln_bwd C{C} R{R} no dres", lambda j: pr.ref_ln_bwd(j, with_dres=False), i
    for C in pr.DIMS:
        for off in (False, True):
            i = pr.add_ln_inputs(C, pr.seed_of("add_ln", C, off), offset=off)
            for m in ("packed_pos", "pad_pad", "no_b", "ls", "no_ls"):
                yield f"add_ln C{C} {m} offset{int(off)}", (lambda j, m=m: pr.ref_add_ln(j, m)), i
        yield f"ls_bwd C{C}", pr.ref_ls_bwd, pr.ls_bwd_inputs(C, 70, pr.seed_of("ls_bwd", C))
    i = pr.gelu_inputs(pr.seed_of("gelu"))
    yield "gelu", pr.ref_gelu, i
    yield "gelu_bwd", pr.ref_gelu_bwd, i
    i = pr.softmax_inputs(pr.seed_of("softmax"))
    yield "softmax", pr.ref_softmax, i
    yield "softmax_bwd", pr.ref_softmax_bwd, i
    for C in pr.ROWDOT_DIMS:
        yield f"rowdot C{C}", pr.ref_rowdot, pr.rowdot_inputs(C, pr.seed_of("rowdot", C))
    for C, add, npf, nb in pr.LOSS_CASES:
        i = pr.loss_inputs(C, pr.seed_of("loss", C, npf), npf)
        yield f"loss C{C} add{add} prefix{npf} norm{nb}", (lambda j, add=add, nb=nb: pr.ref_loss(j, add, nb)), i
    for npf, hc in pr.EMBED_CASES:
        i = pr.embed_inputs(pr.seed_of("embed", npf, hc), npf, hc)
        yield f"embed prefix{npf} cls{hc}", pr.ref_embed, i
        yield f"embed_bwd prefix{npf} cls{hc}", pr.ref_embed_bwd, i
    yield "pos_grad", pr.ref_pos_grad, pr.pos_grad_inputs(pr.seed_of("pos_grad"))
    yield "im2col", pr.ref_im2col, pr.im2col_inputs(pr.seed_of("im2col"))


def test_yardstick_and_conditions_of_the_row_kernels():
    worst = {}
    for name, ref, inp in row_cases():
        r64 = ref(pr.cast(inp, D))
        for k, (v, mag, L) in r64.items():
            assert bool(torch.isfinite(v).all()) and float(v.abs().max()) < FMAX, (name, k)
            assert bool(torch.isfinite(mag).all()) and float(mag.min()) > 1e-30, (name, k, float(mag.min()))
            assert L >= 1
        for k, c in pr.yardstick(ref, inp).items():
            assert math.isfinite(c), (name, k)
            # float32 CPU torch stays inside L u mag: mag is a sound magnitude (and c = max(1, 4 c_ref) = 1 ... 4)
            assert c <= 1.0, (name, k, c)
            key = name.split(" ")[0] + "." + k
            worst[key] = max(worst.get(key, 0.0), c)
    for key in sorted(worst):
        print(f"c_ref {key}: {worst[key]:.3f}")


def test_conditions_of_the_attention_inputs():
    worst = 0.0
    for Tp, T in pr.ATTN_PADS:
        for late in (False, True):
            i = pr.cast(pr.attn_inputs(Tp, T, pr.seed_of("attn", Tp, T, late), late_key=late), D)
            P, z, zabs = pr.ref_attn_fwd(i)
            assert bool(torch.isfinite(z).all()) and bool(torch.isfinite(z.max(-1).values).all())
            assert float(P[:, :, :T, :T].min()) > 1e-30, (Tp, T, late, float(P[:, :, :T, :T].min()))
            close(P[:, :, :T].sum(-1), torch.ones_like(P[:, :, :T, 0]))
            if late and T > 1:  # the last valid key tops the maximum over the keys in front of it by more than 40
                lead = z[..., T - 1] - z[..., :T - 1].max(-1).values
                assert float(lead.min()) > 40.0, float(lead.min())
            _, tol = pr.attn_fwd_tol(i, 1.0)
            assert float(tol[:, :, :T, :T].min()) > 0.0
            worst = max(worst, pr.softmax_cref(z.float()))
    for Tp, T in [(128, 100), (256, 129)]:
        i = pr.cast(pr.attn_bwd_inputs(Tp, T, pr.seed_of("attn_bwd", Tp, T)), D)
        dS, tol = pr.attn_bwd_tol(i)
        assert bool(torch.isfinite(dS).all()) and float(tol[:, :, :T, :T].min()) > 0.0
        assert bool((i["P"][:, :, T:] == 0).all()) and bool((i["P"][:, :, :, T:] == 0).all())
    print(f"c_ref softmax of the attention logits (L = 1, mag = p): {worst:.3f}")
    assert worst < 64.0  # exp of an argument rounded to fp32: |z - m| u relative, |z - m| <= ~60 here


def test_conditions_of_the_contraction_inputs():
    shapes = [(M, N, K) for (_, M, N, K, _, _) in pr.GEMM_EX_CASES] + pr.BIG_EPI_SHAPES + pr.BIG_FALLBACK_SHAPES
    shapes += [(R, n, k) for (R, n, k) in pr.LIN_SHAPES] + [(n, k, R) for (R, n, k) in pr.LIN_SHAPES]
    cases = [(M, N, K, pr.seed_of("gemm", M, N, K), 1) for M, N, K in shapes]
    cases += [(M, N, K, pr.seed_of("gemm_b", kind), 6) for kind, (M, N, K) in
              {"qk": (128, 128, 64), "dS": (128, 128, 64), "pv": (128, 64, 128), "dv": (128, 64, 128)}.items()]
    for M, N, K, seed, nb in cases:
        i = pr.cast(pr.gemm_inputs(M, N, K, seed, nb=nb), D)
        c, mag, cs, csm = pr.ref_gemm(i, bias=True, accumulate=True)
        assert bool(torch.isfinite(c).all()) and float(c.abs().max()) < FMAX and float(mag.min()) > 1e-30 and float(csm.min()) > 1e-30
        # the float32 product stays inside the contraction bound of any summation order
        c32 = pr.ref_gemm(pr.cast(pr.gemm_inputs(M, N, K, seed, nb=nb), torch.float32), True, True)[0]
        assert bool(((c32.double() - c).abs() <= pr.gemm_tol(mag, K, 1, i["bias"])).all())
