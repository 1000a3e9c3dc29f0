"""ORACLE - TEST INFRASTRUCTURE ONLY.  Store what the CPU tests used to ask the live reference, so that they run anywhere.

Needs the reference checkout (oracle/ref_loader.py, CLIPA_REFERENCE):  python oracle/make_live_golden.py

  tests/golden/ref_init_bf16.npz     the recipe of a fresh random init of the reference CLIP (seed 5, toy config): per tensor
                                     its constant, or the scale of its uniform / normal draw (init_recipe); the weights that
                                     recipe redraws (weights_from_recipe, rounded to bf16) and the reference's features /
                                     logit scale / ClipLoss on the oracle's synthetic batch with them
  tests/golden/ref_host.npz          the reference's state_dict layout for ViT-S-16 @ 112, its resize_pos_embed
                                     (model.py:452-481) of an 84 px sin-cos table into a 224 px model, the trainable set
                                     after lock_image_tower(unlocked_groups=0..3), and its model_configs/*.json of the
                                     registry's models
  tests/golden/train_loop_trace.npz  the loop-level operation trace (oracle.trainer_harness.LoopTrace) of the reference's own
                                     training.train.train_one_epoch driving the engine (torch-CPU stand-in ops), accum_freq
                                     1 x 2 steps and 2 x 1 step
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

from oracle import clip_oracle as O  # noqa: E402
from oracle import ref_loader  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
INIT_CFG = {"embed_dim": 64,
            "vision_cfg": {"image_size": 64, "layers": 2, "width": 128, "patch_size": 16},
            "text_cfg": {"context_length": 12, "vocab_size": 300, "width": 128, "heads": 2, "layers": 2}}
REGISTRY = ("ViT-S-16", "ViT-B-16", "ViT-L-16", "ViT-L-16-CL8-Syntax-GAP", "ViT-L-16-CL32-GAP", "ViT-H-14")
TRACE_RUNS = ((1, 2), (2, 1))


def init_recipe(sd):
    """Per tensor of a state dict, in order: [name, shape, kind, value] - kind "const" (every element equal to value),
    "uniform" (draws in [-value, value]: max |x| / std ~ sqrt(3)) or "normal" (standard deviation value)."""
    recipe = []
    for k, v in sd.items():
        v = v.detach().double()
        if bool((v == v.reshape(-1)[0]).all()):
            recipe.append([k, list(v.shape), "const", float(v.reshape(-1)[0])])
        elif float(v.abs().max() / v.std()) < 2.0:
            recipe.append([k, list(v.shape), "uniform", float(v.abs().max())])
        else:
            recipe.append([k, list(v.shape), "normal", float(v.std())])
    return recipe


def weights_from_recipe(recipe, seed=5):
    """The state dict an init_recipe describes, drawn from one seeded CPU generator in recipe order, rounded to bf16 (kept
    as float32)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    sd = {}
    for k, shape, kind, val in recipe:
        if kind == "const":
            t = torch.full(shape, val, dtype=torch.float32)
        elif kind == "uniform":
            t = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * val
        else:
            t = torch.randn(shape, generator=g, dtype=torch.float32) * val
        sd[k] = t.bfloat16().float()
    return sd


def make_init(ref_model, ref_loss):
    torch.manual_seed(5)
    m = ref_model.CLIP(**INIT_CFG, output_dict=True).float()
    recipe = init_recipe(m.state_dict())
    m.load_state_dict(weights_from_recipe(recipe), strict=True)
    img_u8, txt = O.synthetic_batch(6, 64, 12, 300, 3)
    with torch.no_grad():
        out = m(O.normalize_images(img_u8), txt)
        loss = ref_loss.ClipLoss()(out["image_features"], out["text_features"], out["logit_scale"])
    return {"cfg": json.dumps(INIT_CFG), "recipe": json.dumps(recipe), "loss": np.float64(float(loss)),
            "image_features": out["image_features"].numpy(), "text_features": out["text_features"].numpy(),
            "logit_scale": out["logit_scale"].numpy()}


def make_host(ref_model):
    import tempfile
    import clipa_amd
    from oracle.make_golden import CASES
    cfg = clipa_amd.get_model_config("ViT-S-16")
    cfg["vision_cfg"]["image_size"] = 112
    ref_sd = ref_model.CLIP(**cfg).state_dict()
    arrays = {"layout_keys": np.array(list(ref_sd)),
              "layout_shapes": json.dumps({k: list(v.shape) for k, v in ref_sd.items()})}
    # the hand-off of tests/test_host_cpu.py::test_checkpoint_interchange_with_live_reference, resized by the reference
    cfg84 = clipa_amd.get_model_config("ViT-S-16")
    cfg84["vision_cfg"].update(image_size=84, pos_embed="sin_cos_2d")
    torch.manual_seed(0)
    small = clipa_amd.CLIP(**cfg84)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "epoch_1.pt")
        torch.save({"epoch": 1, "state_dict": {"module." + k: v for k, v in small.state_dict().items()}}, path)
        big = clipa_amd.create_model("ViT-S-16", pretrained=path, force_image_size=224, pos_embed="learnable")
    sd = {k: v.clone() for k, v in small.state_dict().items()}
    ref_model.resize_pos_embed(sd, big)
    arrays["resized_visual_pos"] = sd["visual.positional_embedding"].float().numpy()
    lock_cfg = CASES["cls_erf"]["cfg"]
    for unlocked in range(4):
        ref = ref_model.CLIP(**lock_cfg)
        ref.lock_image_tower(unlocked_groups=unlocked)
        arrays[f"lock_{unlocked}"] = json.dumps({k: p.requires_grad for k, p in ref.named_parameters()})
    cfg_dir = os.path.join(ref_loader.REF_ROOT, "open_clip", "model_configs")
    arrays["model_configs"] = json.dumps({n: json.load(open(os.path.join(cfg_dir, n + ".json"))) for n in REGISTRY})
    return arrays


def run_loop(accum, nsteps, loop):
    """The engine on the cls_erf toy model and its seeded batches, one epoch of `loop(model, batches, loss, opt, sched, args)`
    under a LoopTrace; returns the trace's events."""
    import clipa_amd
    from clipa_amd import engine, loss as loss_mod, model as model_mod, optim as optim_mod
    from oracle import trainer_harness as H
    from oracle.make_golden import CASES
    from tests import cpu_ops
    saved = [(m, m.ops) for m in (engine, loss_mod, model_mod, optim_mod)]
    for m, _ in saved:
        m.ops = cpu_ops
    try:
        spec = CASES["cls_erf"]
        cfg, B, S, seed = spec["cfg"], spec["B"], spec["S"], spec["seed"]
        m = clipa_amd.CLIP(**cfg, output_dict=True)
        m.load_state_dict(O.make_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()}, seed), strict=True)
        m.visual.image_mean, m.visual.image_std = H.IMAGE_MEAN, H.IMAGE_STD
        tc = cfg["text_cfg"]
        batches = H.synthetic_batches(nsteps * accum, B, S, tc["context_length"], tc["vocab_size"], seed + 100)
        args = H.make_args("cpu", batch_size=B, accum_freq=accum)
        opt = H.make_optimizer(m)
        loss = H.LossRecorder(clipa_amd.ClipLoss(local_loss=False, gather_with_grad=False, cache_labels=True, rank=0, world_size=1))
        trace = H.LoopTrace()
        loss, sched = trace.attach(m, loss, opt, H.make_scheduler(opt))
        with trace.patched():
            loop(m, batches, loss, opt, sched, args)
        return trace.events
    finally:
        for m, ops in saved:
            m.ops = ops


def make_trace():
    from oracle import trainer_harness as H
    train = H.load_trainer("engine")
    train.get_autocast = lambda precision: lambda: torch.autocast("cpu", dtype=torch.bfloat16)
    arrays = {}
    try:
        for accum, nsteps in TRACE_RUNS:
            ref = run_loop(accum, nsteps, lambda m, b, loss, opt, sched, args: train.train_one_epoch(
                m, {"train": H.DataInfo(H.ListLoader(b))}, loss, 0, opt, None, sched, None, args))
            restated = run_loop(accum, nsteps, lambda m, b, loss, opt, sched, args: H.restated_train_one_epoch(
                m, b, loss, opt, sched, args, lambda: torch.autocast("cpu", dtype=torch.bfloat16)))
            assert ref == restated, "the restated loop no longer follows the reference's"
            arrays[f"trace_a{accum}_n{nsteps}"] = np.array(ref)
            print(f"accum {accum} x {nsteps} steps: {len(ref)} operations")
    finally:
        H.unload()
    return arrays


def main():
    torch.set_num_threads(4)
    ref_model, ref_loss, _ = ref_loader.load()
    for name, arrays in (("ref_init_bf16", make_init(ref_model, ref_loss)), ("ref_host", make_host(ref_model)),
                         ("train_loop_trace", make_trace())):
        out = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(out, **arrays)
        print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
