"""Generate tests/golden/layerscale_*.npz from the REAL reference (CPU): toy towers with LayerScale
(open_clip/transformer.py:43-50,210,221,248-249), in the layout of the other toy goldens (oracle/make_golden.py: run_case).

Run where the reference checkout is available (oracle/ref_loader.py finds it):  python tools/make_layerscale_golden.py
The tests read only the .npz.  At the init value 1e-4 the scaled branches all but vanish from every output and a wrong fold
would pass, so before the reference runs every `gamma` is overwritten with seeded values of magnitude 0.5 - 1.5 and mixed
sign; they are stored in the fixture (`gamma_names`, `gamma_<i>`) - the other weights are regenerated from the seed as for
every toy golden (the generator's draw for a gamma is consumed and then replaced, so the stream of the other tensors is the
one oracle.clip_oracle.make_state_dict gives).  Cases:
  * layerscale_cls_erf:         the cls_erf tower pair (CLS pooling, erf GELU, causal text) with LayerScale in BOTH towers;
  * layerscale_gap_sincos_tanh: the gap_sincos_tanh pair (GAP, frozen sin-cos table, tanh GELU) with LayerScale in the IMAGE
                                tower only.
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

LS_INIT = 1e-4
CASES = {
    "layerscale_cls_erf": dict(B=8, S=48, seed=31, cfg={
        "embed_dim": 64,
        "vision_cfg": {"image_size": 48, "layers": 2, "width": 128, "patch_size": 16, "ls_init_value": LS_INIT},
        "text_cfg": {"context_length": 16, "vocab_size": 512, "width": 128, "heads": 2, "layers": 2,
                     "ls_init_value": LS_INIT}}),
    "layerscale_gap_sincos_tanh": dict(B=8, S=40, seed=32, cfg={
        "embed_dim": 64,
        "vision_cfg": {"image_size": 40, "layers": 2, "width": 128, "patch_size": 16, "global_average_pool": True,
                       "pos_embed": "sin_cos_2d", "gelu_approximate": "tanh", "ls_init_value": LS_INIT},
        "text_cfg": {"context_length": 8, "vocab_size": 512, "width": 64, "heads": 1, "layers": 2,
                     "gelu_approximate": "tanh"}}),
}


def gammas(shapes, seed):
    """{name: f32 [D]} for every `...ls_N.gamma` of `shapes`: |value| uniform in [0.5, 1.5], sign by a fair coin."""
    rng = np.random.RandomState(seed + 5000)
    out = {}
    for name, shape in shapes.items():
        if name.endswith(".gamma"):
            mag = rng.uniform(0.5, 1.5, size=tuple(shape))
            sign = np.where(rng.randint(0, 2, size=tuple(shape)) == 1, 1.0, -1.0)
            out[name] = (mag * sign).astype(np.float32)
    return out


def main():
    torch.set_num_threads(4)
    ref_model, ref_loss, _ = ref_loader.load()
    plain = O.make_state_dict
    only = sys.argv[1:]
    for name, spec in CASES.items():
        if only and name not in only:
            continue
        used = {}

        def with_gammas(shapes, seed, frozen=()):
            sd = plain(shapes, seed, frozen=frozen)
            used.update(gammas(shapes, seed))
            for k, v in used.items():
                sd[k] = torch.from_numpy(v.copy())
            return sd

        O.make_state_dict = with_gammas          # run_case draws its weights through the module attribute
        try:
            make_golden.run_case(name, spec, ref_model, ref_loss)
        finally:
            O.make_state_dict = plain
        path = os.path.join(make_golden.OUT, f"{name}.npz")
        z = dict(np.load(path, allow_pickle=False))
        assert used and all(k in z["keys"] for k in used), sorted(used)
        names = sorted(used)
        z["gamma_names"] = np.array(names)
        for i, k in enumerate(names):
            z[f"gamma_{i}"] = used[k]
        np.savez_compressed(path, **z)
        print(f"wrote {path} ({os.path.getsize(path)} bytes, {len(names)} gammas)")


if __name__ == "__main__":
    main()
