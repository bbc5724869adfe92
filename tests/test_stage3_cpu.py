"""CPU: the stage-3 driver's host pieces -- argument handling, learning rate and schedule, the ImageFolder restatement,
the arena layout's names, the checkpoint format, loading a distilled checkpoint into the wrapper -- and a world-size-2
gloo run through `model_factory` with a CPU stand-in engine against one process with the whole batch."""
import math
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from oracle import vit as OV
from tests import s3_reference as REF


def _args(extra=()):
    from dvt_amd import stage3
    return stage3.get_args(["--denoiser_ckpt", "x.pth", *extra])


def test_args_input_size_and_iterations():
    from dvt_amd import stage3
    a = _args()
    assert a.input_size == (518, 518) and a.stride_size == 14 and a.num_iterations is None and a.num_epochs == 10
    assert a.batch_size == 32 and a.blr == 2e-4 and a.min_lr == 1e-6 and a.weight_decay == 1e-5 and a.save_freq == 5000
    assert _args(["--input_size", "518", "518", "--auto_stride"]).input_size == (518, 518)
    assert _args(["--input_size", "224", "448"]).input_size == (224, 448)
    with pytest.raises(SystemExit):
        _args(["--input_size", "518"])
    with pytest.raises(SystemExit):
        _args(["--input_size", "500", "500"])  # not divisible by the stride
    a = _args(["--grad_checkpointing", "--vis_freq", "10", "--num_vis_samples", "2", "--warmup_iters", "7"])
    assert a.grad_checkpointing and a.micro_batch == 0
    # num_iterations = len(ds) // (batch * world) * num_epochs unless given
    a = _args(["--batch_size", "64", "--num_epochs", "5"])
    assert stage3.num_iterations(a, 1_281_167, 8) == 1_281_167 // 512 * 5
    assert stage3.num_iterations(_args(["--num_iterations", "17"]), 1000, 8) == 17


def test_learning_rate_and_warmup():
    from dvt_amd import stage3
    a = _args(["--batch_size", "64"])
    lr = stage3.learning_rate(a, 8)
    assert lr == pytest.approx(2e-4 * math.sqrt(64 * 8 / 256))
    s = stage3.scheduler(a, lr, 1000)
    assert s[0] == 0.0 and s[149] == pytest.approx(lr) and s[150] == pytest.approx(lr)  # int(0.15 * 1000) warm-up steps
    assert s[999] > a.min_lr and s[1000] == a.min_lr


def test_image_folder_order_and_extensions(tmp_path):
    from dvt_amd import stage3
    files = ["b/z.JPG", "b/sub/a.png", "b/a.webp", "a/2.jpeg", "a/1.txt", "a/x/y/3.bmp", "a/10.PNG", "c/notes.md"]
    for f in files:
        os.makedirs(os.path.dirname(tmp_path / f), exist_ok=True)
        (tmp_path / f).write_bytes(b"")
    ds = stage3.ImageFolderList(str(tmp_path))
    assert ds.classes == ["a", "b", "c"]
    got = [(os.path.relpath(p, tmp_path), c) for p, c in ds.samples]
    assert got == [("a/10.PNG", 0), ("a/2.jpeg", 0), ("a/x/y/3.bmp", 0), ("b/a.webp", 1), ("b/z.JPG", 1),
                   ("b/sub/a.png", 1)]


def test_load_image_resize_flip_normalise(tmp_path):
    from PIL import Image
    from dvt_amd import stage3
    rng = np.random.default_rng(0)
    a = rng.integers(0, 255, (30, 50, 3), dtype=np.uint8)
    Image.fromarray(a).save(tmp_path / "i.png")
    x = stage3.load_image(str(tmp_path / "i.png"), (28, 42), False)
    xf = stage3.load_image(str(tmp_path / "i.png"), (28, 42), True)
    assert x.shape == (3, 28, 42) and x.dtype == np.float32
    assert np.array_equal(xf, x[:, :, ::-1])
    want = np.asarray(Image.fromarray(a).resize((42, 28), Image.BICUBIC), np.float32) / 255.0
    assert np.allclose(x[0], (want[..., 0] - 0.485) / 0.229, atol=1e-6)
    flips = [stage3.flip_decision(42, 3, j) for j in range(64)]
    assert flips == [stage3.flip_decision(42, 3, j) for j in range(64)] and 10 < sum(flips) < 54


def test_layout_names_equal_random_state_dict(built_lib):
    from dvt_amd import s3
    from dvt_amd.vit import random_state_dict
    for n_reg, depth in ((0, 12), (4, 2)):
        cfg = s3.make_config(768, depth, 14, 14, 518, 518, n_reg)
        total, layout = s3.param_layout(cfg)
        sd = random_state_dict(768, depth, 14, (0 if n_reg else 1) + 37 * 37, n_reg=n_reg)
        assert set(layout) == set(sd)
        assert all(tuple(sd[k].shape) == tuple(s) for k, (_, s) in layout.items())
        assert all(o % 4 == 0 for o, _ in layout.values()) and total % 4 == 0
        assert total >= sum(v.numel() for v in sd.values())
    cfg = s3.make_config(768, 12, 14, 14, 518, 518)
    assert cfg.s_pad == 1408 and cfg.n_tokens == 1370
    with pytest.raises(Exception):
        s3.Stage3Engine(cfg, torch.device("cpu"))  # no CPU fallback


# ---- a CPU stand-in engine: flat arenas, oracle/vit.py + autograd for the step ---------------------------------------
DIM, DEPTH, IMG = 128, 1, 28


def tiny_state(seed):
    from dvt_amd.vit import random_state_dict
    return random_state_dict(DIM, DEPTH, 14, 1 + 4, seed=seed, well_conditioned=True)


class FlatOracleViTEngine:
    """The Stage3Engine interface computing with the oracle on the CPU (float64 arenas)."""

    def __init__(self, sd):
        self.names = list(sd)
        self.shapes = [tuple(sd[n].shape) for n in self.names]
        self.params = torch.cat([sd[n].double().reshape(-1) for n in self.names]).clone()
        self.grads = torch.zeros_like(self.params)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.loss = torch.zeros(4, dtype=torch.float64)
        self.step = 0

    def views(self, arena=None):
        arena = self.params if arena is None else arena
        out, o = {}, 0
        for n, s in zip(self.names, self.shapes):
            out[n] = arena[o:o + math.prod(s)].view(s)
            o += math.prod(s)
        return out

    def state_dict(self):
        return {k: v.clone() for k, v in self.views().items()}

    def train_step(self, img, target, feat=None, micro_batch=None):
        _, (loss, l2, cos), g = REF.step(self.views(), img, target)
        self.grads += torch.cat([g[n].reshape(-1) for n in self.names])
        self.loss = torch.tensor([loss, l2, cos, 0.0], dtype=torch.float64)
        return self.loss

    def adamw_step(self, lr, weight_decay, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0):
        self.step += 1
        g = self.grads * grad_scale
        self.params *= 1 - lr * weight_decay
        self.exp_avg.mul_(betas[0]).add_(g, alpha=1 - betas[0])
        self.exp_avg_sq.mul_(betas[1]).addcmul_(g, g, value=1 - betas[1])
        bc1, bc2 = 1 - betas[0] ** self.step, 1 - betas[1] ** self.step
        self.params -= (lr / bc1) * self.exp_avg / (self.exp_avg_sq.sqrt() / math.sqrt(bc2) + eps)
        self.grads.zero_()


def teacher_fn(img, return_dict=True):
    """A frozen stand-in teacher: another tiny ViT's features (float64)."""
    return {"denoised_feats": OV.forward_features({k: v.double() for k, v in tiny_state(99).items()}, img.double(),
                                                  patch=14, stride=14)}


def factory(args, device):
    return FlatOracleViTEngine(tiny_state(5)), teacher_fn


def _write_images(root, n):
    from PIL import Image
    rng = np.random.default_rng(3)
    for i in range(n):
        d = os.path.join(root, "images", f"c{i % 2}")
        os.makedirs(d, exist_ok=True)
        h, w = 20 + 7 * i, 40 - 3 * i
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(d, f"{i}.png"))


def _driver_args(root, iters, bs):
    from dvt_amd import stage3
    return stage3.get_args(["--model", "vit_small_patch14_dinov2.lvd142m", "--denoiser_ckpt", "unused.pth", "--data_root",
                            f"{root}/images", "--input_size", str(IMG), str(IMG), "--batch_size", str(bs),
                            "--num_iterations", str(iters), "--output_root", f"{root}/work", "--device", "cpu",
                            "--save_freq", "3", "--log_freq", "1", "--num_workers", "2"])


def _rank_main(rank, world, root, port, iters, bs, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from dvt_amd import dist as D
    from dvt_amd import stage3
    dev = torch.device("cpu")
    D.init(dev, world)
    out = stage3.train(_driver_args(root, iters, bs), rank, world, dev, model_factory=factory)
    q.put((rank, [h["loss"] for h in out["history"]], out["engine"].params.clone().numpy()))
    D.finish()


def test_data_parallel_step_equals_single_process(tmp_path):
    from dvt_amd import stage2, stage3
    root, world, iters, bs, n = str(tmp_path), 2, 4, 2, 6
    _write_images(root, n)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + os.getpid() % 90
    procs = [ctx.Process(target=_rank_main, args=(r, world, root, port, iters, bs, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert np.array_equal(res[0][2], res[1][2])  # both ranks hold the same parameters

    # one process, the ranks' batches concatenated, torch.optim.AdamW (the reference's optimizer)
    args = _driver_args(root, iters, bs)
    ds = stage3.ImageFolderList(f"{root}/images")
    streams = [stage2.sampler_indices(len(ds), world, r, True) for r in range(world)]
    p = REF.leaves(tiny_state(5))
    opt = torch.optim.AdamW(list(p.values()), betas=(0.9, 0.999), eps=1e-8, weight_decay=args.weight_decay)
    sched = stage3.scheduler(args, stage3.learning_rate(args, world), iters)
    losses = []
    for step in range(iters):
        idx = [next(s) for s in streams for _ in range(bs)]
        img = torch.from_numpy(np.stack([stage3.load_image(ds.samples[i][0], (IMG, IMG),
                                                           stage3.flip_decision(args.seed, step, j))
                                         for j, i in enumerate(idx)]))
        for g in opt.param_groups:
            g["lr"] = float(sched[step])
        opt.zero_grad()
        loss, _, _ = REF.loss_fn(OV.forward_features(p, img.double(), patch=14, stride=14),
                                 teacher_fn(img)["denoised_feats"])
        loss.backward()
        opt.step()
        losses.append(loss.item())
    want = torch.cat([v.detach().reshape(-1) for v in p.values()]).numpy()
    assert np.allclose(res[0][2], want, atol=1e-9, rtol=1e-6), float(np.abs(res[0][2] - want).max())
    # a rank logs the loss of ITS half; with equal halves their mean is the loss of the whole batch
    assert np.allclose(np.mean([res[0][1], res[1][1]], axis=0), losses, rtol=1e-9)

    # rank 0 wrote reference-format checkpoints: `model.`-prefixed timm keys, torch's AdamW state layout
    ck_dir = f"{root}/work/denosing-vit/debug/checkpoints"
    assert sorted(os.listdir(ck_dir)) == ["ckpt_000000.pth", "ckpt_000003.pth", "latest.pth"]
    assert os.path.realpath(f"{ck_dir}/latest.pth").endswith("ckpt_000003.pth")
    ck = torch.load(f"{ck_dir}/latest.pth", weights_only=False)
    assert ck["step"] == 3 and list(ck["model"])[:3] == ["model.cls_token", "model.pos_embed", "model.patch_embed.proj.weight"]
    assert set(ck["model"]) == {"model." + k for k in p}
    names = [k[len("model."):] for k in ck["model"]]
    ref_opt = torch.optim.AdamW([p[k] for k in names])
    ref_opt.load_state_dict(ck["optimizer"])
    assert ck["optimizer"]["state"][0]["exp_avg"].shape == p["cls_token"].shape


def test_wrapper_loads_distilled_checkpoint(tmp_path):
    from dvt_amd.models.vit_wrapper import PretrainedViTWrapper
    from dvt_amd.vit import random_state_dict
    sd = random_state_dict(384, 12, 14, 1 + 37 * 37, seed=2)
    torch.save({"model": {"model." + k: v for k, v in sd.items()}, "optimizer": {}, "step": 9}, tmp_path / "d.pth")
    w = PretrainedViTWrapper("vit_small_patch14_dinov2.lvd142m", stride=14, checkpoint_path=str(tmp_path / "d.pth"))
    assert set(w._state_dict) == set(sd)
    assert all(torch.equal(w._state_dict[k], sd[k]) for k in sd)
    # a plain timm state dict is taken as it is
    torch.save(sd, tmp_path / "t.pth")
    w = PretrainedViTWrapper("vit_small_patch14_dinov2.lvd142m", stride=14, checkpoint_path=str(tmp_path / "t.pth"))
    assert set(w._state_dict) == set(sd)
