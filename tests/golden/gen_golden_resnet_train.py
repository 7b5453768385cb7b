"""Generate the ResNet training golden vectors (tests/golden/rn*_coop*.npz, rn*_cocoop*.npz) by running the REFERENCE's own
``trainers.coop.CustomCLIP`` / ``trainers.cocoop.CustomCLIP`` over its own ``ModifiedResNet``.

Run in the build container only (needs the reference checkout, which never travels to the GPU box), on the CPU:

    python tests/golden/gen_golden_resnet_train.py

What runs: as tests/golden/gen_golden_coop.py and gen_golden.run_cocoop -- the reference's ``CustomCLIP`` imported unmodified, torch CPU fp32 --
with ``load_clip_to_cpu`` replaced by ``clip.model.CLIP(embed_dim, image_size, (l1, l2, l3, l4), width, 0, ...)`` (the tuple selects
``ModifiedResNet``, clip/model.py:686-694) in eval mode, as clip.build_model returns it: BatchNorm runs on its running statistics whatever
mode the prompt learner is in.  The text side is loaded from ``oracle.mudpt_oracle.make_frozen_state``, the tower from
``tests.resnet_reference.make_rn_state``; the fixture stores the seeds (frozen, tower, trainables, images), not the weights.

Stored per fixture: config (the text side and n_ctx; its ViT fields only seed the draws), rn_stages, rn_width, trainer, class names, tokenized
prompts, seeds, labels, the images' checksum, eval logits, training loss, the gradient of every trainable (``ctx``; CoCoOp: the four meta_net
tensors too), the raw ``image_features`` [B, e], logit_scale; CoOp: csc, class_token_position, name_lens and the drawn ctx; CoCoOp: ctx_init
and its token ids.  And the EMULATED TOWER TERMS, for fp16 and bf16: the same outputs once more with ``image_encoder`` replaced by
``tests.resnet_reference.image_features(rn, images, stages, heads, T)`` -- the float64 restatement rounded at the library's five sites -- as
deviations from the unreplaced run: ``emulated_logit`` [fp16 max, rms, bf16 max, rms] and ``emulated_grad.<key>`` [fp16 max, rms, bf16 max,
rms] of the difference, relative to the gradient's rms.  That is what the tower's number formats alone cost; tests/test_resnet_train_cpu.py
holds the logit term to half of helpers.check_logits' bound, tests/test_resnet_train_gpu.py adds three times the gradient terms to
helpers.check_fixture_grads' bounds.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import CLASSNAMES, ROOT, O, import_reference, seeded_images  # noqa: E402
from gen_golden_coop import TINY_NAMES  # noqa: E402
from oracle import cocoop_oracle as CO  # noqa: E402
from tests import resnet_reference as R  # noqa: E402


class EmulatedTower(torch.nn.Module):
    """Stands where ``clip_model.visual`` stood: the float64 restatement rounded to T at the library's five sites, as fp32 features."""

    def __init__(self, rn, stages, heads, T):
        super().__init__()
        self.rn, self.stages, self.heads, self.T = rn, stages, heads, T

    def forward(self, images):
        with torch.no_grad():
            return R.image_features(self.rn, images, self.stages, self.heads, self.T).float()


def run(name: str, stages, width: int, image_size: int, embed_dim: int, text: dict, trainer: str, batch: int, classnames, n_ctx: int, frozen_seed: int,
        rn_seed: int, train_seed: int, image_seed: int, csc: bool = False, position: str = "end", ctx_init: str = ""):
    names = list(classnames)
    cfg = O.Config(image_size=image_size, patch=32, v_width=64, v_layers=sum(stages), v_heads=1, embed_dim=embed_dim, n_ctx=n_ctx, depth=1, **text)
    clip, cm, _mudpt, CN = import_reference()
    from trainers import cocoop, coop
    frozen = O.make_frozen_state(cfg, frozen_seed)
    rn = R.make_rn_state(R.RnShape(stages, width, image_size, embed_dim), rn_seed)
    state = {k: v for k, v in frozen.items() if not k.startswith("visual.")}
    state.update(rn)
    ref_clip = cm.CLIP(embed_dim, image_size, tuple(stages), width, 0, cfg.ctx_len, cfg.vocab, cfg.t_width, cfg.t_heads, cfg.t_layers, None).float()
    assert type(ref_clip.visual).__name__ == "ModifiedResNet"
    missing, unexpected = ref_clip.load_state_dict(state, strict=False)
    assert not unexpected and all(k.endswith("num_batches_tracked") for k in missing), (missing, unexpected)
    ref_clip.eval()  # clip/model.py:921 build_model returns model.eval(); Dassl switches the registered prompt_learner only
    heads = width * 32 // 64
    images = seeded_images(cfg, batch, image_seed)
    labels = (torch.arange(batch) * 3 + 1) % len(names)
    extra = {}
    if trainer == "CoOp":
        ycfg = CN(TRAINER=CN(NAME="CoOp", COOP=CN(N_CTX=n_ctx, CTX_INIT="", PREC="fp32", CSC=csc, CLASS_TOKEN_POSITION=position)), INPUT=CN(SIZE=(image_size, image_size)))
        torch.manual_seed(train_seed)  # the reference draws ctx with nn.init.normal_ (coop.py:71) from the global generator
        model = coop.CustomCLIP(ycfg, names, ref_clip)
        keys = ["prompt_learner.ctx"]
        ctx = model.prompt_learner.ctx
        assert tuple(ctx.shape) == ((len(names),) if csc else ()) + (n_ctx, cfg.t_width)
        extra = {"csc": np.array(csc), "class_token_position": np.array(position), "name_lens": np.array(model.prompt_learner.name_lens, dtype=np.int32),
                 "ctx": ctx.detach().numpy().astype(np.float32).copy()}
    else:
        ycfg = CN(TRAINER=CN(NAME="CoCoOp", COCOOP=CN(N_CTX=n_ctx, CTX_INIT=ctx_init, PREC="fp32")), INPUT=CN(SIZE=(image_size, image_size)))
        model = cocoop.CustomCLIP(ycfg, names, ref_clip)
        keys = list(CO.TRAINABLE_ORDER)
        ctx_ids = [int(v) for v in clip.tokenize(ctx_init)[0, 1:1 + n_ctx]]
        params = CO.make_trainable_state(cfg, train_seed, frozen, ctx_ids)
        ref_params = dict(model.named_parameters())
        assert torch.equal(ref_params["prompt_learner.ctx"].detach(), params["prompt_learner.ctx"])  # the reference's own CTX_INIT rule
        assert tuple(ref_params["prompt_learner.meta_net.linear1.weight"].shape) == (embed_dim // 16, embed_dim)  # cocoop.py:104
        with torch.no_grad():
            for k in keys:
                ref_params[k].copy_(params[k])
        extra = {"ctx_init": np.array(ctx_init), "ctx_token_ids": np.array(ctx_ids, dtype=np.int32)}
    for k, p in model.named_parameters():  # freeze rule, trainers/coop.py:240-243, cocoop.py:222-226
        p.requires_grad_("prompt_learner" in k)
    trainables = dict((k, p) for k, p in model.named_parameters() if p.requires_grad)
    assert sorted(trainables) == sorted(keys)

    def outputs():
        """(eval logits, training loss, {key: gradient}) of the model as it stands."""
        model.prompt_learner.eval()
        with torch.no_grad():
            logits = model(images)  # cocoop.py:198: eval mode returns the logits
        model.prompt_learner.train()
        for p in trainables.values():
            p.grad = None
        loss = torch.nn.functional.cross_entropy(model(images), labels) if trainer == "CoOp" else model(images, labels)  # coop.py:281-296, cocoop.py:196-197
        loss.backward()
        return logits, loss.item(), {k: trainables[k].grad.detach().clone() for k in keys}

    tower = model.image_encoder
    with torch.no_grad():
        raw = tower(images)
    exact = R.feature_error(R.image_features(rn, images, stages, heads), raw)
    logits, loss, grads = outputs()
    emulated_logit, emulated_grad = [], {k: [] for k in keys}
    for T in (torch.float16, torch.bfloat16):
        model.image_encoder = EmulatedTower(rn, stages, heads, T)
        lg, _, gr = outputs()
        d = (lg - logits).double()
        emulated_logit += [d.abs().max().item(), d.pow(2).mean().sqrt().item()]
        for k in keys:
            dg, rms = (gr[k] - grads[k]).double(), grads[k].double().pow(2).mean().sqrt().item()
            emulated_grad[k] += [dg.abs().max().item() / rms, dg.pow(2).mean().sqrt().item() / rms]
    model.image_encoder = tower
    out = {
        "config": np.array(repr(cfg.asdict())), "rn_stages": np.array(stages, dtype=np.int64), "rn_width": np.array(width, dtype=np.int64),
        "trainer": np.array(trainer), "classnames": np.array(names), "tokenized_prompts": model.tokenized_prompts.numpy().astype(np.int32),
        "seeds": np.array([frozen_seed, rn_seed, train_seed, image_seed], dtype=np.int64), "labels": labels.numpy().astype(np.int64),
        "images_checksum": np.array([images.double().sum().item(), images.double().abs().sum().item()]),
        "logits": logits.numpy().astype(np.float32), "loss": np.array(loss, dtype=np.float64), "image_features": raw.numpy().astype(np.float32),
        "logit_scale": np.array(frozen["logit_scale"].item(), dtype=np.float32), "emulated_logit": np.array(emulated_logit, dtype=np.float64), **extra,
    }
    for k in keys:
        out["grad." + k] = grads[k].numpy()
        out["emulated_grad." + k] = np.array(emulated_grad[k], dtype=np.float64)
    path = os.path.join(ROOT, "tests", "golden", name + ".npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: loss {loss:.6f}, float64 restatement of the tower {exact:.2e}, emulated logits (max, rms) fp16 {emulated_logit[0]:.2e} {emulated_logit[1]:.2e} "
          f"bf16 {emulated_logit[2]:.2e} {emulated_logit[3]:.2e}, {os.path.getsize(path) / 1e3:.1f} KB")
    for k in keys:
        print(f"    {k}: emulated gradient (max, rms) / rms fp16 {emulated_grad[k][0]:.2e} {emulated_grad[k][1]:.2e} bf16 {emulated_grad[k][2]:.2e} {emulated_grad[k][3]:.2e}")


if __name__ == "__main__":
    tiny_text = dict(t_width=128, t_layers=3, t_heads=2, ctx_len=77, vocab=49408)
    rn50_text = dict(t_width=512, t_layers=12, t_heads=8, ctx_len=77, vocab=49408)
    tiny_names = TINY_NAMES[:5]  # names of 1, 2 and 3 BPE tokens: the middle splice moves the context by a different number of rows per class
    only = sys.argv[1:]
    fixtures = {
        # embed_dim != t_width in every one; rn_coop_tiny2_csc: an odd n_ctx, which "middle" splits 2 + 3
        "rn_coop_tiny": lambda n: run(n, (1, 1, 1, 1), 32, 64, 512, tiny_text, "CoOp", 3, tiny_names, 4, 31, 33, 51, 35),
        "rn_coop_tiny2_csc": lambda n: run(n, (2, 1, 2, 1), 64, 96, 1024, tiny_text, "CoOp", 2, tiny_names, 5, 31, 37, 52, 39, csc=True, position="middle"),
        "rn_cocoop_tiny": lambda n: run(n, (1, 1, 1, 1), 32, 64, 512, tiny_text, "CoCoOp", 2, tiny_names, 2, 31, 33, 53, 36, ctx_init="a photo"),
        "rn50_coop_b2": lambda n: run(n, (3, 4, 6, 3), 64, 224, 1024, rn50_text, "CoOp", 2, CLASSNAMES, 16, 0, 41, 54, 4321),  # CoOp's rn50 configs: N_CTX 16
        "rn50_cocoop_b1": lambda n: run(n, (3, 4, 6, 3), 64, 224, 1024, rn50_text, "CoCoOp", 1, CLASSNAMES, 4, 0, 41, 55, 4322, ctx_init="a photo of a"),  # B 1: the script's batch
    }
    for n, f in fixtures.items():
        if not only or n in only:
            f(n)
