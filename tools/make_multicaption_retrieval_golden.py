"""Generate tests/golden/multicaption_retrieval.npz from the REAL reference image-text retrieval evaluation
(clipa_jax/evaluators/proj/image_text/image_text_retrieval.py: image_to_text_retrieval_eval, text_to_image_retrieval_eval).

Run where the reference checkout is available (next to the one oracle/ref_loader.py finds; numpy only):
    python tools/make_multicaption_retrieval_golden.py
The GPU tests read the .npz and regenerate the features with `case_inputs` below; they never need the reference.  Cases:
  * A: 1000 images with 0-7 captions each (about one in eight has none), E = 256.  No near ties: every entry of a text's
       column is more than 1e-4 (fp64) from its positive, every entry of an image's row that is not one of its own
       captions more than 1e-4 from its best caption's score, so the reference's fp32 summation order cannot change a
       rank and the engine must match it exactly.
  * B: 777 images with 0-9 captions each, E = 200: ragged shapes.  About 5 % of the captions are exact copies of a caption
       of another image and about 2 % of the images exact copies of another image, so exact ties occur in both
       directions.  Every other entry is again more than 1e-4 from its positive.
Features: a concept vector per image, image = concept + noise, caption = concept of its image + noise, rows L2-normalised
in fp64 and stored as fp32.  The captions are stored in a shuffled order.  A caption or image near a tie is redrawn with
fresh noise; `txt_redraws` / `img_redraws` (stored) say how often, so the features are a pure function of the stored
seed, correspondence and redraws.  Stored: shapes, seeds, correspondence, redraws, duplicate maps, the reference's
Recall@{1,5,10} in both directions and the 0-based ranks read off the reference's own argsort (i2t: position of an
image's first own caption, N_txt when it has none; t2i: position of a caption's image).
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "multicaption_retrieval.npz")
CASES = {"A": dict(ni=1000, e=256, max_caps=7, noise=2.5, dup_txt=0.0, dup_img=0.0, seed=5101),
         "B": dict(ni=777, e=200, max_caps=9, noise=2.5, dup_txt=0.05, dup_img=0.02, seed=5102)}
MARGIN = 1e-4
THRESHOLDS = (1, 5, 10)


def correspondence(name):
    """-> c [Nt] int64 (shuffled caption order), dup_txt [Nt], dup_img [Ni] (index of the copied row, or -1)."""
    k = CASES[name]
    rng = np.random.RandomState(k["seed"])
    caps = rng.randint(0, k["max_caps"] + 1, size=k["ni"])
    c = np.repeat(np.arange(k["ni"]), caps)
    c = c[rng.permutation(len(c))]
    nt = len(c)
    dup_txt = np.full(nt, -1, dtype=np.int64)
    m = int(round(k["dup_txt"] * nt))
    if m:
        perm = rng.permutation(nt)
        src, dst = perm[m:2 * m], perm[:m]
        keep = c[src] != c[dst]                      # a copy describes ANOTHER image: an exact non-own tie
        dup_txt[dst[keep]] = src[keep]
    dup_img = np.full(k["ni"], -1, dtype=np.int64)
    m = int(round(k["dup_img"] * k["ni"]))
    if m:
        perm = rng.permutation(k["ni"])
        dup_img[perm[:m]] = perm[m:2 * m]
    return c, dup_txt, dup_img


def _unit(x):
    return (x / np.sqrt((x * x).sum(1, keepdims=True))).astype(np.float32)


def features(name, c, img_redraws, txt_redraws, dup_img, dup_txt):
    """-> image features fp32 [Ni, E], text features fp32 [Nt, E]."""
    k = CASES[name]
    ni, e = k["ni"], k["e"]
    base = np.random.RandomState(k["seed"] + 1).standard_normal((ni, e))
    img = np.stack([base[i] + k["noise"] * np.random.RandomState([k["seed"], 0, i, int(img_redraws[i])]).standard_normal(e)
                    for i in range(ni)])
    txt = np.stack([base[c[t]] + k["noise"] * np.random.RandomState([k["seed"], 1, t, int(txt_redraws[t])]).standard_normal(e)
                    for t in range(len(c))])
    img, txt = _unit(img), _unit(txt)
    src = dup_img >= 0
    img[src] = img[dup_img[src]]
    src = dup_txt >= 0
    txt[src] = txt[dup_txt[src]]
    return img, txt


def case_inputs(name, c, img_redraws, txt_redraws):
    _, dup_txt, dup_img = correspondence(name)
    return features(name, c, img_redraws, txt_redraws, dup_img, dup_txt)


def near_ties(img, txt, c):
    """-> (images, texts) whose row / column holds an entry within MARGIN of its positive that is not an exact tie."""
    x = img.astype(np.float64) @ txt.astype(np.float64).T
    nt = len(c)
    p = x[c, np.arange(nt)]
    d = np.abs(x - p[None, :])
    own = c[None, :] == np.arange(len(img))[:, None]
    col_bad = ((d <= MARGIN) & (d > 0) & ~own).any(0)
    m = np.where(own, x, -np.inf).max(1)
    d = np.abs(x - m[:, None])
    row_bad = ((d <= MARGIN) & (d > 0) & ~own).any(1) & np.isfinite(m)
    return np.nonzero(row_bad)[0], np.nonzero(col_bad)[0]


def solve_redraws(name, c):
    _, dup_txt, dup_img = correspondence(name)
    ri, rt = np.zeros(CASES[name]["ni"], dtype=np.int64), np.zeros(len(c), dtype=np.int64)
    for _ in range(60):
        img, txt = features(name, c, ri, rt, dup_img, dup_txt)
        bad_i, bad_t = near_ties(img, txt, c)
        if len(bad_i) == 0 and len(bad_t) == 0:
            return ri, rt
        # a copy follows its source: redraw the source
        ri[np.where(dup_img[bad_i] >= 0, dup_img[bad_i], bad_i)] += 1
        rt[np.where(dup_txt[bad_t] >= 0, dup_txt[bad_t], bad_t)] += 1
    raise RuntimeError(f"case {name}: near ties remain")


def load_reference():
    from oracle import ref_loader
    path = os.path.join(os.path.dirname(ref_loader.REF_ROOT), "clipa_jax", "evaluators", "proj", "image_text",
                        "image_text_retrieval.py")
    spec = importlib.util.spec_from_file_location("_ref_image_text_retrieval", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def ref_ranks(dist, c):
    """0-based ranks read off the reference's own argsorts of dist = -similarities."""
    ni, nt = dist.shape
    per_text = dist.argsort(axis=0)                         # as text_to_image_retrieval_eval
    t2i = np.argmax(per_text == c[None, :], axis=0)
    per_image = dist.argsort(axis=1)                        # as image_to_text_retrieval_eval
    own = c[per_image] == np.arange(ni)[:, None]
    i2t = np.where(own.any(1), np.argmax(own, axis=1), nt)
    return i2t, t2i


def generate():
    ref = load_reference()
    arrays = {}
    for name, k in CASES.items():
        c, dup_txt, dup_img = correspondence(name)
        ri, rt = solve_redraws(name, c)
        img, txt = case_inputs(name, c, ri, rt)
        sim = np.dot(img, txt.T)                            # the reference's similarities (retrieval.py), fp32
        i2t_ref = ref.image_to_text_retrieval_eval(-sim, list(c))
        t2i_ref = ref.text_to_image_retrieval_eval(-sim, list(c))
        i2t, t2i = ref_ranks(-sim, c)
        has = np.bincount(c, minlength=k["ni"]) > 0
        for kk in THRESHOLDS:                                # the ranks reproduce the reference's recalls
            assert np.mean(has & (i2t < kk)) == i2t_ref[f"Recall@{kk}"]
            assert np.mean(t2i < kk) == t2i_ref[f"Recall@{kk}"]
        arrays.update({f"{name}_ni": np.int64(k["ni"]), f"{name}_nt": np.int64(len(c)), f"{name}_e": np.int64(k["e"]),
                       f"{name}_seed": np.int64(k["seed"]), f"{name}_c": c.astype(np.int32),
                       f"{name}_img_redraws": ri.astype(np.int8), f"{name}_txt_redraws": rt.astype(np.int8),
                       f"{name}_dup_img": dup_img.astype(np.int32), f"{name}_dup_txt": dup_txt.astype(np.int32),
                       f"{name}_i2t": i2t.astype(np.int32), f"{name}_t2i": t2i.astype(np.int32),
                       f"{name}_thresholds": np.array(THRESHOLDS, dtype=np.int64),
                       f"{name}_img2txt": np.array([np.float64(i2t_ref[f"Recall@{kk}"]) for kk in THRESHOLDS]),
                       f"{name}_txt2img": np.array([np.float64(t2i_ref[f"Recall@{kk}"]) for kk in THRESHOLDS])})
        print(name, "Ni", k["ni"], "Nt", len(c), "captionless", int((~has).sum()), "img2txt",
              [round(float(v), 4) for v in arrays[f"{name}_img2txt"]], "txt2img",
              [round(float(v), 4) for v in arrays[f"{name}_txt2img"]], "redrawn images / texts:", int((ri > 0).sum()),
              int((rt > 0).sum()))
    return arrays


def main():
    arrays = generate()
    np.savez_compressed(OUT, **arrays)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
