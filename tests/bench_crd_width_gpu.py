"""Timing of the CRD bank kernels at the three row widths (not a pytest file):

    python tests/bench_crd_width_gpu.py [--lib PATH ...] [--widths 64 128 256] [--rounds N] [--dump DIR]

  gathers   the MICCAI call sequence ph_crd_score, ph_crd_select, ph_crd_loss_grad, ph_crd_update at B = 64, P + K = 300 + 700,
            P2 + K2 = 20 + 512, n_data = 65 536
  scan      ph_crd_bank_topk (the MIA-2023 KNN) at 65 536 rows x 64 queries, num_pos 6

Device events around back-to-back calls, warmed up, the repeat count chosen so that a figure is at least one second of device
work.  Next to each time: the algorithmic bytes from the shapes (2 banks x B x (P + K) x 4 D for the gathers of ph_crd_score,
2 x n x 4 D for the scan) and the rate as a fraction of the 6.29 TB/s copy rate the project normalises by.

Several --lib (builds of libpathomic_hip.so, e.g. the parent commit's twice and this one) are timed alternately, round by round,
in one process on one device: the spread between two copies of one build is the noise a difference has to exceed.  A width a
build refuses is reported as refused.  --dump DIR writes every output of both workloads at every width as <DIR>/<lib index>_<D>.npz;
with several libraries the dumps are compared bit for bit."""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np      # noqa: E402
import torch            # noqa: E402

from multimodal_learning_amd import _lib      # noqa: E402

COPY_RATE = 6.29e12
NEEDED = ("ph_crd_score", "ph_crd_select", "ph_crd_loss_grad", "ph_crd_loss_grad_workspace_bytes", "ph_crd_update",
          "ph_crd_bank_topk", "ph_crd_bank_topk_workspace_bytes")


def load(path):
    l = C.CDLL(path)
    for name in NEEDED:
        fn = getattr(l, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return l


def timed(call, min_seconds=1.0):
    """Microseconds per call over at least `min_seconds` of device time."""
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(50):
        call()
    e1.record(); torch.cuda.synchronize()
    reps = max(50, int(min_seconds * 1e3 / (e0.elapsed_time(e1) / 50)) + 1)
    e0.record()
    for _ in range(reps):
        call()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3


class Gathers:
    B, P, K, P2, K2, n = 64, 300, 700, 20, 512, 65536

    def __init__(self, D):
        g = torch.Generator().manual_seed(1)
        B, PK, S2, n = self.B, self.P + self.K, self.P2 + self.K2, self.n
        nrm = lambda x: torch.nn.functional.normalize(x, dim=1)
        self.D = D
        self.mem0 = [nrm(torch.randn(n, D, generator=g)).cuda() for _ in range(2)]
        self.mem = [m.clone() for m in self.mem0]
        self.v = [nrm(torch.randn(B, D, generator=g)).cuda() for _ in range(2)]
        self.y = torch.randperm(n, generator=g)[:B].cuda()
        self.idx = torch.randint(0, n, (B, PK), generator=g).cuda()
        self.idx[:, 0] = self.y
        f = lambda *s: torch.empty(*s, device="cuda")
        self.out1, self.out2, self.diff = f(B, PK), f(B, PK), f(B, PK)
        self.sel, self.xs, self.xt = torch.empty(B, S2, dtype=torch.int32, device="cuda"), f(B, S2), f(B, S2)
        self.lossp, self.dv1, self.dv2 = f(B), f(B, D), f(B, D)
        self.params = torch.tensor([self.K, 0.07, 5.0e4, 6.0e4, 0.5, self.P], dtype=torch.float32).cuda()
        self.bytes = 2.0 * B * PK * 4 * D

    def call(self, L):
        p, st = _lib.ptr, _lib.stream()
        B, P, K, P2, K2, D = self.B, self.P, self.K, self.P2, self.K2, self.D
        rc = L.ph_crd_score(p(self.v[0]), p(self.v[1]), p(self.idx), None, p(self.mem[0]), p(self.mem[1]), p(self.out1), p(self.out2),
                            p(self.diff), B, P + K, D, 0.07, st)
        rc |= L.ph_crd_select(p(self.diff), p(self.out1), p(self.out2), None, p(self.sel), p(self.xs), p(self.xt), B, P, K, P2, K2, 1, 1, st)
        rc |= L.ph_crd_loss_grad(p(self.xs), p(self.xt), p(self.sel), p(self.idx), None, None, None, p(self.mem[0]), p(self.mem[1]),
                                 p(self.params), p(self.lossp), p(self.dv1), p(self.dv2), B, P + K, P2, K2, D, float(self.n), 1.0 / B,
                                 None, st)
        rc |= L.ph_crd_update(p(self.mem[0]), p(self.mem[1]), p(self.v[0]), p(self.v[1]), p(self.y), p(self.params), B, D, st)
        return rc

    def outputs(self, L):
        for m, m0 in zip(self.mem, self.mem0):
            m.copy_(m0)
        assert self.call(L) == 0
        torch.cuda.synchronize()
        names = ("out1", "out2", "diff", "sel", "xs", "xt", "lossp", "dv1", "dv2")
        o = {"g_" + k: getattr(self, k).cpu().numpy() for k in names}
        o["g_rows1"], o["g_rows2"] = self.mem[0][self.y].cpu().numpy(), self.mem[1][self.y].cpu().numpy()
        return o


class Scan:
    n, B, NP = 65536, 64, 6

    def __init__(self, D, ws_bytes):
        g = torch.Generator().manual_seed(2)
        n, B, NP = self.n, self.B, self.NP
        self.D = D
        self.mem = [(torch.rand(n, D, generator=g) - 0.5).cuda() for _ in range(2)]
        self.labels = torch.randint(0, 3, (n,), generator=g).int().cuda()
        self.idx = torch.randint(0, n, (B, 5), generator=g).cuda()
        self.bl = self.labels[self.idx[:, 0]].long()
        self.nb = [torch.empty(B, NP, dtype=torch.int64, device="cuda") for _ in range(2)]
        self.sim = [torch.empty(B, NP, device="cuda") for _ in range(2)]
        self.ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        self.bytes = 2.0 * n * 4 * D

    def call(self, L):
        p = _lib.ptr
        return L.ph_crd_bank_topk(p(self.mem[0]), p(self.mem[1]), p(self.labels), p(self.idx), 5, p(self.bl), self.B, self.n, self.NP,
                                  self.D, p(self.nb[0]), p(self.nb[1]), p(self.sim[0]), p(self.sim[1]), p(self.ws), _lib.stream())

    def outputs(self, L):
        assert self.call(L) == 0
        torch.cuda.synchronize()
        return {"s_nb1": self.nb[0].cpu().numpy(), "s_nb2": self.nb[1].cpu().numpy(), "s_sim1": self.sim[0].cpu().numpy(),
                "s_sim2": self.sim[1].cpu().numpy()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=None)
    ap.add_argument("--widths", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    paths = a.lib or [_lib.LIB_PATH]
    libs = [load(p) for p in paths]
    for k, p in enumerate(paths):
        print("lib %d = %s" % (k, p))
    dumps = {}
    for D in a.widths:
        works = {"gathers": Gathers(D), "scan": Scan(D, libs[0].ph_crd_bank_topk_workspace_bytes(Scan.B, Scan.n))}
        for name, w in works.items():
            ok = [w.call(L) == 0 for L in libs]
            torch.cuda.synchronize()
            for r in range(a.rounds):
                for k, L in enumerate(libs):
                    if not ok[k]:
                        if r == 0:
                            print("D %3d %-8s lib %d: refused" % (D, name, k))
                        continue
                    us = timed(lambda: w.call(L))
                    print("D %3d %-8s lib %d round %d: %8.2f us   %7.1f MB algorithmic   %5.1f %% of 6.29 TB/s"
                          % (D, name, k, r, us, w.bytes / 1e6, 100.0 * w.bytes / (us * 1e-6) / COPY_RATE), flush=True)
            if a.dump:
                for k, L in enumerate(libs):
                    if ok[k]:
                        dumps.setdefault((k, D), {}).update(w.outputs(L))
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        for (k, D), o in dumps.items():
            np.savez(os.path.join(a.dump, "%d_%d.npz" % (k, D)), **o)
        for D in a.widths:
            have = [k for k in range(len(libs)) if (k, D) in dumps]
            for k in have[1:]:
                same = all(dumps[(have[0], D)][key].tobytes() == dumps[(k, D)][key].tobytes() for key in dumps[(have[0], D)])
                print("D %3d outputs of lib %d and lib %d: %s" % (D, have[0], k, "bit for bit the same" if same else "DIFFERENT"))


if __name__ == "__main__":
    main()
