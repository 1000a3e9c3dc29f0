"""Top-k similarity search (clipa_amd.search.topk_similarity, csrc/topk.hip) against stock PyTorch on the same GPU in the same
process: fp32 torch.matmul + torch.topk, chunked over the gallery with a running merge (cat + topk) wherever the [Nq, Ng] matrix
is not to be held at once.
    python tools/topk_bench.py [--cases zero-shot,retrieval,knn,few-queries] [--iters 3] >> profiles/topk_bench.jsonl
One JSON line per case:
  zero-shot     50 000 x 1 000 x 768, k = 5        one call, the matrix fits
  retrieval     5 000 x 25 000 x 768, k = 10       one call, the matrix fits
  knn           10 000 x 1 281 167 x 1024, k = 20  shards of 65 536 gallery rows on both sides
  few-queries   8 x 4 000 000 x 768, k = 10        shards of 500 000 rows; one extra timing per --splits value (0 = the entry
                                                   point's own rule), which is where the column splits matter
Data: seeded unit-norm rows around seeded prototypes (non-zero, with structure: a query has near neighbours).  Times are wall
clock of one whole search ending in a device synchronise, the median of --iters runs after one warm-up run.  `agree` is the
fraction of query rows whose index lists are identical on both sides (they differ where two fp32 values round differently in
the two summation orders); `engine_mib` / `torch_mib` the peak device memory each side allocated beyond the inputs.  There is
no pass / fail threshold.  Every number is a measurement of the run that printed it, on the device named in the record."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from clipa_amd import ops, search  # noqa: E402

DEV = "cuda"
CASES = {"zero-shot": dict(nq=50000, ng=1000, e=768, k=5, shard=None),
         "retrieval": dict(nq=5000, ng=25000, e=768, k=10, shard=None),
         "knn": dict(nq=10000, ng=1281167, e=1024, k=20, shard=65536),
         "few-queries": dict(nq=8, ng=4000000, e=768, k=10, shard=500000)}


def make_rows(n, e, proto, gen, noise=4.0, chunk=1 << 18):
    out = torch.empty((n, e), device=DEV)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        y = torch.randint(0, proto.shape[0], (b - a,), device=DEV, generator=gen)
        out[a:b] = torch.nn.functional.normalize(proto[y] + noise * torch.randn(b - a, e, device=DEV, generator=gen), dim=1)
    return out


def torch_topk(q, shards, k):
    """The yardstick: per shard one fp32 matmul and one topk, merged into the running lists by cat + topk."""
    val = idx = None
    base = 0
    for g in shards:
        v, i = torch.topk(q @ g.T, min(k, g.shape[0]), dim=1)
        i = i + base
        if val is not None:
            v, j = torch.topk(torch.cat([val, v], dim=1), k, dim=1)
            i = torch.gather(torch.cat([idx, i], dim=1), 1, j)
        val, idx, base = v, i, base + g.shape[0]
    return val, idx


def engine_topk(q, shards, k, splits=0):
    carry, base = None, 0
    for g in shards:
        carry = ops.topk_similarity(q, g, k, index_base=base, carry=carry, splits=min(splits, (g.shape[0] + 127) // 128))
        base += g.shape[0]
    return carry


def wall(fn, iters):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], out, (torch.cuda.max_memory_allocated() - before) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--splits", default="0,1,32,128,512,2048", help="column splits timed in the few-queries case")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench: no GPU visible; nothing is measured without one")
    for name in args.cases.split(","):
        c = CASES[name]
        gen = torch.Generator(device=DEV).manual_seed(c["nq"] + c["ng"] + c["e"])
        proto = torch.randn(1000, c["e"], device=DEV, generator=gen)
        q = make_rows(c["nq"], c["e"], proto, gen)
        g = make_rows(c["ng"], c["e"], proto, gen)
        shards = [g] if c["shard"] is None else [g[a:a + c["shard"]] for a in range(0, c["ng"], c["shard"])]
        t_ms, (tv, ti), t_mib = wall(lambda: torch_topk(q, shards, c["k"]), args.iters)
        e_ms, (ev, ei), e_mib = wall(lambda: engine_topk(q, shards, c["k"]), args.iters)
        pub_ms, (pv, pi), _ = wall(lambda: search.topk_similarity(q, shards if c["shard"] else g, c["k"]), args.iters)
        assert torch.equal(pi, ei) and torch.equal(pv, ev)
        rec = {"case": name, "Nq": c["nq"], "Ng": c["ng"], "E": c["e"], "k": c["k"], "shard_rows": c["shard"], "iters": args.iters,
               "device": torch.cuda.get_device_name(0), "torch_ms": round(t_ms, 3), "engine_ms": round(e_ms, 3),
               "public_ms": round(pub_ms, 3), "engine_tflops": round(2.0 * c["nq"] * c["ng"] * c["e"] / e_ms / 1e9, 1),
               "torch_mib": round(t_mib, 1), "engine_mib": round(e_mib, 1),
               "agree": round(float((ti == ei).all(dim=1).float().mean()), 5),
               "top1_agree": round(float((ti[:, 0] == ei[:, 0]).float().mean()), 5)}
        if name == "few-queries":
            rec["splits_ms"] = {}
            for s in (int(v) for v in args.splits.split(",")):
                ms, (sv, si), _ = wall(lambda: engine_topk(q, shards, c["k"], splits=s), args.iters)
                assert torch.equal(si, ei) and torch.equal(sv, ev)           # every split count: the same bits
                rec["splits_ms"][str(s)] = round(ms, 3)
        print(json.dumps(rec), flush=True)
        del q, g, shards


if __name__ == "__main__":
    main()
