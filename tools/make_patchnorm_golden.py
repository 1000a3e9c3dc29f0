"""Generate tests/golden/patchnorm_*.npz from the REAL reference (CPU): toy towers with dual PatchNorm
(input_patchnorm; open_clip/transformer.py:362-371,483-489), in the layout of the other toy goldens (oracle/make_golden.py:
run_case).

Run where the reference checkout is available (oracle/ref_loader.py finds it):  python tools/make_patchnorm_golden.py
The tests read only the .npz.  At the init values (gamma = 1, beta = 0) a wrong fold would pass, so before the reference runs
`visual.patchnorm_pre_ln.weight` is overwritten with seeded values of magnitude 0.5 - 1.5 and mixed sign,
`visual.patchnorm_pre_ln.bias` with values of magnitude up to 0.5 and `visual.conv1.bias` with non-zero values; they are stored
in the fixture (`stem_names`, `stem_<i>`) - the other weights are regenerated from the seed as for every toy golden (the
generator's draw for an overwritten tensor is consumed and then replaced, so the stream of the other tensors is the one
oracle.clip_oracle.make_state_dict gives).  The stem's gradients (patchnorm_pre_ln.*, conv1.*, class / positional embedding) are
stored as full arrays (`stem_grad_names`, `stem_grad_<i>`) beside the digests every golden holds.  Cases:
  * patchnorm_cls_erf:  16 px patches of 48 px images (K = 768), width 128, 2 layers, ln_pre, CLS pooling, causal text;
  * patchnorm_p14_gap:  14 px patches of 42 px images (K = 588: no multiple of 8, padded to 592), GAP, frozen sin-cos table,
                        tanh GELU.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import clip_oracle as O  # noqa: E402
from oracle import make_golden, ref_loader  # noqa: E402

CASES = {
    "patchnorm_cls_erf": dict(B=8, S=48, seed=41, cfg={
        "embed_dim": 64,
        "vision_cfg": {"image_size": 48, "layers": 2, "width": 128, "patch_size": 16, "input_patchnorm": True},
        "text_cfg": {"context_length": 16, "vocab_size": 512, "width": 128, "heads": 2, "layers": 2}}),
    "patchnorm_p14_gap": dict(B=8, S=42, seed=42, cfg={
        "embed_dim": 64,
        "vision_cfg": {"image_size": 42, "layers": 2, "width": 128, "patch_size": 14, "input_patchnorm": True,
                       "global_average_pool": True, "pos_embed": "sin_cos_2d", "gelu_approximate": "tanh"},
        "text_cfg": {"context_length": 8, "vocab_size": 512, "width": 64, "heads": 1, "layers": 2,
                     "gelu_approximate": "tanh"}}),
}
STEM = ("visual.patchnorm_pre_ln.weight", "visual.patchnorm_pre_ln.bias", "visual.conv1.weight", "visual.conv1.bias",
        "visual.class_embedding", "visual.positional_embedding")


def stem_values(shapes, seed):
    """{name: f32 array} of the three overwritten tensors: gamma with |value| uniform in [0.5, 1.5] and sign by a fair coin, beta
    uniform in [-0.5, 0.5], conv1.bias uniform in +-[0.05, 0.3]."""
    rng = np.random.RandomState(seed + 7000)
    k, d = tuple(shapes["visual.patchnorm_pre_ln.weight"]), tuple(shapes["visual.conv1.bias"])
    sign = lambda shape: np.where(rng.randint(0, 2, size=shape) == 1, 1.0, -1.0)
    return {"visual.patchnorm_pre_ln.weight": (rng.uniform(0.5, 1.5, size=k) * sign(k)).astype(np.float32),
            "visual.patchnorm_pre_ln.bias": rng.uniform(-0.5, 0.5, size=k).astype(np.float32),
            "visual.conv1.bias": (rng.uniform(0.05, 0.3, size=d) * sign(d)).astype(np.float32)}


def main():
    torch.set_num_threads(4)
    ref_model, ref_loss, _ = ref_loader.load()
    plain = O.make_state_dict
    only = sys.argv[1:]
    for name, spec in CASES.items():
        if only and name not in only:
            continue
        used, grads = {}, {}

        def with_stem(shapes, seed, frozen=()):
            sd = plain(shapes, seed, frozen=frozen)
            used.update(stem_values(shapes, seed))
            for k, v in used.items():
                sd[k] = torch.from_numpy(v.copy())
            return sd

        # run_case keeps digests of the gradients only: catch the full arrays where it takes the digests
        digest = make_golden.grad_digest

        def keep_grads(named, seed):
            grads.update({k: v.detach().numpy().copy() for k, v in named.items() if k in STEM})
            return digest(named, seed)

        O.make_state_dict, make_golden.grad_digest = with_stem, keep_grads      # run_case reads both through the modules
        try:
            make_golden.run_case(name, spec, ref_model, ref_loss)
        finally:
            O.make_state_dict, make_golden.grad_digest = plain, digest
        path = os.path.join(make_golden.OUT, f"{name}.npz")
        z = dict(np.load(path, allow_pickle=False))
        assert len(used) == 3 and all(k in z["keys"] for k in used), sorted(used)
        names = sorted(used)
        z["stem_names"] = np.array(names)
        for i, k in enumerate(names):
            z[f"stem_{i}"] = used[k]
        gnames = sorted(grads)
        assert set(gnames) == {k for k in STEM if k in [str(n) for n in z["grad_names"]]} and len(gnames) >= 5, gnames
        z["stem_grad_names"] = np.array(gnames)
        for i, k in enumerate(gnames):
            z[f"stem_grad_{i}"] = grads[k]
        np.savez_compressed(path, **z)
        print(f"wrote {path} ({os.path.getsize(path)} bytes, stem tensors {names}, {len(gnames)} full gradients)")


if __name__ == "__main__":
    main()
