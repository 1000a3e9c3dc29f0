"""A/B of clipa_attention_fwd / clipa_attention_bwd between builds of libclipa_hip.so loaded side by side (first = baseline).

    python tools/attn_lib_ab.py [--shapes "B,H,L,dh,causal;..."] clipa_amd/lib/libclipa_hip_parent.so clipa_amd/lib/libclipa_hip.so
        timing: interleaved rounds, median per library, outputs compared bit for bit; the built-in production shapes, then --shapes
    python tools/attn_lib_ab.py --cases libA.so libB.so
        every kernel instantiation: the cases of tests/attention_cases.py (SHORT_CASES, LONG_CASES; its B, H and random_case
        inputs) through each library, out / stats / dqkv filled with 0xFF bytes before every call and compared with torch.equal

One JSON line per shape or case."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from clipa_amd.lib import SIGNATURES  # noqa: E402

PRODUCTION = ((4096, 16, 197, 64, 0), (4096, 12, 197, 64, 0), (4096, 12, 77, 64, 1), (2048, 16, 257, 80, 0), (4096, 16, 50, 64, 0))
ap = argparse.ArgumentParser()
ap.add_argument("libs", nargs="+")
ap.add_argument("--cases", action="store_true")
ap.add_argument("--shapes", default="", help='further timing shapes, "B,H,L,dh,causal;..."')
ap.add_argument("--no-production", action="store_true", help="time the --shapes only")
args = ap.parse_args()

libs = [ctypes.CDLL(os.path.abspath(p)) for p in args.libs]
for lib in libs:
    for name in ("clipa_attention_fwd", "clipa_attention_bwd", "clipa_last_error"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = SIGNATURES[name]
NL = len(libs)
dev = "cuda"
st = torch.cuda.current_stream().cuda_stream


class Case:
    """Inputs of one shape on the device and one set of outputs per library."""

    def __init__(self, B, H, L, dh, causal, qkv, do):
        self.B, self.H, self.L, self.dh, self.causal, self.D = B, H, L, dh, causal, H * dh
        self.qkv, self.do = qkv.to(dev), do.to(dev)
        D = self.D
        self.out = [torch.empty(B * L, D, device=dev, dtype=torch.bfloat16) for _ in libs]
        self.stats = [torch.empty(B * H * L, 2, device=dev) for _ in libs]
        self.dqkv = [torch.empty(B * L, 3 * D, device=dev, dtype=torch.bfloat16) for _ in libs]

    def poison(self, i):
        for t in (self.out[i], self.stats[i], self.dqkv[i]):
            t.view(torch.uint8).fill_(0xFF)

    def fwd(self, i):
        D, q = self.D, self.qkv
        rc = libs[i].clipa_attention_fwd(q[:, :D].data_ptr(), q[:, D:2 * D].data_ptr(), q[:, 2 * D:].data_ptr(), self.out[i].data_ptr(),
                                         self.stats[i].data_ptr(), self.B, self.H, self.L, self.dh, 3 * D, D, self.dh ** -0.5, self.causal, st)
        assert rc == 0, libs[i].clipa_last_error()

    def bwd(self, i):
        D, q, g = self.D, self.qkv, self.dqkv[i]
        rc = libs[i].clipa_attention_bwd(q[:, :D].data_ptr(), q[:, D:2 * D].data_ptr(), q[:, 2 * D:].data_ptr(), self.out[i].data_ptr(),
                                         self.do.data_ptr(), self.stats[i].data_ptr(), g[:, :D].data_ptr(), g[:, D:2 * D].data_ptr(),
                                         g[:, 2 * D:].data_ptr(), self.B, self.H, self.L, self.dh, 3 * D, D, 3 * D, self.dh ** -0.5, self.causal, st)
        assert rc == 0, libs[i].clipa_last_error()

    def same(self):
        """Poison, run forward and backward through every library, compare everything with the first library's."""
        for i in range(NL):
            self.poison(i)
            self.fwd(i)
            self.bwd(i)
        torch.cuda.synchronize()
        return {k: all(torch.equal(v[0], v[i]) for i in range(1, NL)) for k, v in (("out", self.out), ("stats", self.stats), ("dqkv", self.dqkv))}


if args.cases:
    import attention_cases as ac
    cases = [(ac.short_id(c), c[0].dh, ac.SHORT_H, ac.SHORT_B, c[1], c[0].causal) for c in ac.SHORT_CASES]
    cases += [(ac.long_id(c), c[0], ac.LONG_H, ac.LONG_B, c[1], c[2]) for c in ac.LONG_CASES]
    bad = 0
    for cid, dh, H, B, L, causal in cases:
        qkv, do = ac.random_case(dh, H, B, L, ac.case_seed(dh, L, causal))
        same = Case(B, H, L, dh, int(causal), qkv, do).same()
        bad += not all(same.values())
        print(json.dumps({"case": cid, "B": B, "H": H, "L": L, "dh": dh, "causal": int(causal), "bit_identical": all(same.values()), **same}), flush=True)
    print(json.dumps({"cases": len(cases), "bit_identical": len(cases) - bad, "differ": bad}), flush=True)
    sys.exit(1 if bad else 0)

shapes = [] if args.no_production else list(PRODUCTION)
shapes += [tuple(int(x) for x in s.split(",")) for s in args.shapes.split(";") if s.strip()]
for B, H, L, dh, causal in shapes:
    D = H * dh
    torch.manual_seed(0)
    case = Case(B, H, L, dh, causal, torch.randn(B * L, 3 * D, device=dev).to(torch.bfloat16), torch.randn(B * L, D, device=dev).to(torch.bfloat16))
    row = {"B": B, "H": H, "L": L, "dh": dh, "causal": causal, "bit_identical": all(case.same().values())}
    for name, fn in (("fwd", case.fwd), ("bwd", case.bwd)):
        ts = [[] for _ in libs]
        for _ in range(5):
            for i in range(NL):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(3):
                    fn(i)
                e1.record()
                torch.cuda.synchronize()
                ts[i].append(e0.elapsed_time(e1) / 3)
        ms = [statistics.median(t) for t in ts]
        row[name + "_ms"] = [round(m, 4) for m in ms]
        row[name + "_speedup"] = [round(ms[0] / m, 3) for m in ms]
    print(json.dumps(row), flush=True)
    del case
